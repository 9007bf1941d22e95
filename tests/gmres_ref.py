"""numpy restarted GMRES(m), right-preconditioned or flexible: the yardstick of the GPU solver's
tests (test_gmres_ref.py checks it against dense least squares).

Semantics of pnp_capi.h PNP_METHOD_GMRES / PNP_METHOD_FGMRES: zero start; x = x0 + M^-1 V y
(flexible: x0 + Z y with Z_j = M(V_j) stored); the history holds |r0|, then after each Arnoldi step
the Givens estimate |g_{k+1}|, replaced at each restart boundary and at the end by the recomputed
true norm |b - A x|; stop when the norm < reduction * |r0|, or |r0| < 1e-30; when the estimate
meets the test but the true norm does not, a new cycle starts.  Orthogonalisation: classical
Gram-Schmidt applied twice, the new direction's norm taken from the vector itself.
"""
import numpy as np


class Result:
    def __init__(self):
        self.x = None
        self.history = []
        self.iterations = 0
        self.converged = False
        self.breakdown = 0


def gmres(A, b, M=None, restart=30, reduction=1e-8, maxit=20000, flexible=False, mgs=False):
    """A: scipy sparse matrix or ndarray; M: callable d -> M^-1 d (None: identity).
    mgs: modified Gram-Schmidt instead of CGS2 (to measure the spread between the two orders)."""
    n = b.size
    apply_m = (lambda d: d.copy()) if M is None else M
    out = Result()
    x = np.zeros(n)
    r = b.astype(np.float64).copy()
    norm0 = float(np.linalg.norm(r))
    hist = [norm0]
    it = 0
    if not norm0 >= 1e-30:
        out.x, out.history, out.converged = x, np.array(hist), True
        return out
    target = reduction * norm0
    nr = norm0
    while True:
        if nr < target:
            out.converged = True
            break
        if it >= maxit:
            break
        m = restart
        V = np.zeros((m + 1, n))
        Z = np.zeros((m, n)) if flexible else None
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = r / nr
        g[0] = nr
        k = 0
        for j in range(m):
            z = apply_m(V[j])
            if flexible:
                Z[j] = z
            w = A @ z
            if not np.any(w):
                out.breakdown = 5
                break
            if mgs:
                h = np.zeros(j + 1)
                for i in range(j + 1):
                    h[i] = V[i] @ w
                    w = w - h[i] * V[i]
            else:
                h1 = V[:j + 1] @ w
                w = w - h1 @ V[:j + 1]
                h2 = V[:j + 1] @ w
                w = w - h2 @ V[:j + 1]
                h = h1 + h2
            hn = float(np.sqrt(w @ w))
            col = np.concatenate([h, [hn]])
            if not np.all(np.isfinite(col)):
                out.breakdown = 5
                break
            for i in range(j):
                a, c = col[i], col[i + 1]
                col[i] = cs[i] * a + sn[i] * c
                col[i + 1] = -sn[i] * a + cs[i] * c
            d = float(np.sqrt(col[j] * col[j] + hn * hn))
            if not (d > 0.0 and np.isfinite(d)):
                out.breakdown = 5
                break
            cs[j], sn[j] = col[j] / d, hn / d
            col[j], col[j + 1] = d, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            H[:j + 2, j] = col
            if hn > 0.0:
                V[j + 1] = w / hn
            k = j + 1
            it += 1
            est = abs(g[j + 1])
            hist.append(est)
            if est < target or it >= maxit or hn == 0.0:
                break
        if k > 0:
            y = np.zeros(k)
            for i in range(k - 1, -1, -1):
                y[i] = (g[i] - H[i, i + 1:k] @ y[i + 1:k]) / H[i, i]
            x = x + (y @ Z[:k] if flexible else apply_m(y @ V[:k]))
        r = b - A @ x
        nr = float(np.linalg.norm(r))
        hist[it] = nr
        if out.breakdown:
            break
    out.x, out.history, out.iterations = x, np.array(hist), it
    return out
