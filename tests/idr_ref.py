"""numpy IDR(s), the bi-orthogonal variant of van Gijzen and Sonneveld (2011), right-preconditioned:
the yardstick of the GPU solver's tests (test_idr_ref.py checks it against its textbook form, a
plain BiCGSTAB and the dense host check of csrc/idr_small.h).

Semantics of pnp_capi.h PNP_METHOD_IDR.  Zero start, r = b, G = U = 0, M = I, omega = 1,
f = P^T r.  Per cycle, for k = 0 .. s-1:
    M[k:,k:] c = f[k:];  v = r - sum_{i>=k} c_i G_i;  U_k = omega B^-1 v + sum_{i>=k} c_i U_i
    G_k = A U_k;  q = P^T G_k                      (one block of s dot products)
    M[:k,:k] alpha = q[:k];  G_k -= sum_{i<k} alpha_i G_i;  U_k likewise
    M[k:,k] = q[k:] - M[k:,:k] alpha               (no second reduction)
    beta = f_k / M[k,k];  r -= beta G_k;  x += beta U_k;  f[:k+1] = 0;  f[k+1:] -= beta M[k+1:,k]
then t = A B^-1 r, omega = <t,r>/<t,t>, scaled by 0.7/|rho| when |rho| = |<t,r>|/(|t||r|) < 0.7,
r -= omega t, x += omega B^-1 r, f = P^T r.  The history holds |r0|, then the recurrence's |r|
after every operator application (s + 1 per cycle).  When that norm meets the test (or at maxit)
the true residual b - A x is formed (not counted) and its norm replaces the entry: if it meets the
test the solve ends, else it goes on from the true residual with G = U = 0, M = I, omega = 1 (a
residual replacement), at most 8 times.  Breakdown 6: a zero or non-finite pivot M[k,k] or omega.

textbook=True: the k sequential dot products of the paper's form (alpha_i = <p_i, G_k> / M[i,i]
against the partly corrected G_k) in place of the alpha solve: algebraically the same.
"""
import numpy as np

MAX_REPLACE = 8
ANGLE = 0.7


class Result:
    def __init__(self):
        self.x = None
        self.history = []
        self.iterations = 0
        self.converged = False
        self.breakdown = 0
        self.replacements = 0
        self.M = []      # M at the end of each cycle's k loop
        self.omega = []  # omega of each cycle


def shadow_entry(g, f, j):
    """csrc/idr_small.h idr_shadow_entry: splitmix64's finaliser over (vertex, field, column)."""
    m = (1 << 64) - 1
    z = (0x1d72a5b3c4e6f809 + 0x9e3779b97f4a7c15 * (g * 64 + f * 8 + j + 1)) & m
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m
    z ^= z >> 31
    return (float(z >> 11) + 0.5) * (2.0 / 9007199254740992.0) - 1.0


def shadow(nv, nf, s):
    """The s orthonormalised shadow columns, [s, nf * nv] in the external [phi | c+ | c-] layout."""
    P = np.array([[shadow_entry(g, f, j) for f in range(nf) for g in range(nv)] for j in range(s)])
    for j in range(s):
        for i in range(j):
            P[j] -= (P[i] @ P[j]) * P[i]
        P[j] /= np.sqrt(P[j] @ P[j])
    return P


def idr(A, b, P, M=None, reduction=1e-8, maxit=20000, textbook=False, norm_scale=None):
    """A: scipy sparse matrix or ndarray; M: callable d -> B^-1 d (None: identity); P: [s, n], the
    shadow vectors as rows.  norm_scale: callable (application index) -> factor on the recurrence's
    norm as the stop test and the history see it (a test hook for the replacement path)."""
    n = b.size
    P = np.asarray(P, dtype=np.float64)
    s = P.shape[0]
    apply_m = (lambda d: d.copy()) if M is None else M
    out = Result()
    x = np.zeros(n)
    r = b.astype(np.float64).copy()
    norm0 = float(np.linalg.norm(r))
    hist = [norm0]
    it = 0
    if not norm0 >= 1e-30:
        out.x, out.history, out.converged = x, np.array(hist), bool(np.isfinite(norm0))
        return out
    target = reduction * norm0
    first = True
    while True:
        # r is a true residual: the verdict (idr_begin)
        if not first:
            nr = float(np.linalg.norm(r))
            hist[it] = nr
            if out.breakdown or not np.isfinite(nr):
                out.breakdown = out.breakdown or 6
                break
            if nr < target:
                out.converged = True
                break
        if it >= maxit or (not first and out.replacements >= MAX_REPLACE):
            break
        if not first:
            out.replacements += 1
        first = False
        G, U = np.zeros((s, n)), np.zeros((s, n))
        Mm = np.eye(s)
        omega = 1.0
        f = P @ r
        ended = False

        def record(rr):
            nonlocal it, ended
            nr = float(np.sqrt(rr))
            if norm_scale is not None:
                nr *= norm_scale(it + 1)
            it += 1
            hist.append(nr)
            if not np.isfinite(nr):
                out.breakdown = 6
                ended = True
            elif nr < target or it >= maxit:
                ended = True

        while not ended:
            for k in range(s):
                c = np.zeros(s)
                for i in range(k, s):  # forward substitution on M[k:, k:]
                    d = Mm[i, i]
                    if d == 0.0 or not np.isfinite(d):
                        out.breakdown = 6
                        break
                    c[i] = (f[i] - Mm[i, k:i] @ c[k:i]) / d
                if out.breakdown:
                    ended = True
                    break
                v = r - c[k:] @ G[k:]
                U[k] = omega * apply_m(v) + c[k:] @ U[k:]
                G[k] = A @ U[k]
                if textbook:
                    for i in range(k):
                        a = (P[i] @ G[k]) / Mm[i, i]
                        G[k] -= a * G[i]
                        U[k] -= a * U[i]
                    Mm[k:, k] = P[k:] @ G[k]
                else:
                    q = P @ G[k]
                    alpha = np.zeros(k)
                    for i in range(k):
                        alpha[i] = (q[i] - Mm[i, :i] @ alpha[:i]) / Mm[i, i]
                    G[k] -= alpha @ G[:k]
                    U[k] -= alpha @ U[:k]
                    Mm[k:, k] = q[k:] - Mm[k:, :k] @ alpha
                piv = Mm[k, k]
                beta = f[k] / piv if piv != 0.0 else np.inf
                if piv == 0.0 or not np.isfinite(piv) or not np.isfinite(beta):
                    out.breakdown = 6
                    ended = True
                    break
                r = r - beta * G[k]
                x = x + beta * U[k]
                record(r @ r)
                if ended:
                    break
                f[:k + 1] = 0.0
                f[k + 1:] -= beta * Mm[k + 1:, k]
            if ended:
                break
            out.M.append(Mm.copy())
            vh = apply_m(r)
            t = A @ vh
            tr, tt, rr = t @ r, t @ t, r @ r
            with np.errstate(all="ignore"):
                om = tr / tt
                rho = abs(tr / (np.sqrt(tt) * np.sqrt(rr)))
                if rho < ANGLE:
                    om = om * (ANGLE / rho)
            if om == 0.0 or not np.isfinite(om):
                out.breakdown = 6
                break
            omega = float(om)
            out.omega.append(omega)
            r = r - omega * t
            x = x + omega * vh
            record(r @ r)
            f = P @ r
        r = b - A @ x
    out.x, out.history, out.iterations = x, np.array(hist), it
    return out


def bicgstab(A, b, rt=None, reduction=1e-8, maxit=1000):
    """Plain unpreconditioned BiCGSTAB with the shadow residual rt (default b), no safeguard on
    omega; returns the residual norms after every full iteration ([0] = |b|) and the solution.
    IDR(1) with P = [rt] is this method, two operator applications per iteration."""
    rt = b if rt is None else rt
    x = np.zeros(b.size)
    r = b.copy()
    rho = alpha = om = 1.0
    v = p = np.zeros(b.size)
    hist = [float(np.linalg.norm(r))]
    for _ in range(maxit):
        rho_new = rt @ r
        beta = (rho_new / rho) * (alpha / om)
        rho = rho_new
        p = r + beta * (p - om * v)
        v = A @ p
        alpha = rho / (rt @ v)
        sv = r - alpha * v
        t = A @ sv
        om = (t @ sv) / (t @ t)
        x = x + alpha * p + om * sv
        r = sv - om * t
        hist.append(float(np.linalg.norm(r)))
        if hist[-1] < reduction * hist[0]:
            break
    return np.array(hist), x
