"""numpy restatement of PNP_PREC_CHEBYSHEV (include/pnp_capi.h) on a scipy CSR
matrix in the external layout (dof f * nv + g; constrained rows are identity rows, as
Context.jacobian exports them).

    D_i   the nf x nf diagonal block of vertex i: D_i[f, g] = A[f nv + i, g nv + i]
    theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta
    r_0 = d, rho_0 = 1 / sigma, p_0 = D^-1 d / theta, z = p_0
    i = 1 .. k-1:  r_i = r_{i-1} - A p_{i-1},  rho_i = 1 / (2 sigma - rho_{i-1}),
                   p_i = rho_i rho_{i-1} p_{i-1} + (2 rho_i / delta) D^-1 r_i,  z += p_i
    steps 1: z = D^-1 d.
    bounds: lmax = boost x lambda_est (or the caller's), lmin = lmax / ratio;
    lambda_est = |w_m| / |w_{m-1}|, w_j = D^-1 A w_{j-1}, w_0(g, f) = idr_ref.shadow_entry(g, 4, f)

`owned` (a boolean array over the vertices) gives the rank-local form the AMG's level-0 smoother
runs: the owned x owned part of A, results on the owned rows, zero elsewhere.

Also the yardsticks of the GPU tests' solves: BiCGSTAB and CG with ISTL's counting and a
preconditioner given as a function."""
import numpy as np
import scipy.sparse as sp

import idr_ref

DEFAULTS = dict(steps=3, eig_ratio=10.0, eig_iters=20, eig_boost=1.1, lambda_max=0.0)


def diag_blocks(A, nf):
    """[nv, nf, nf]: the vertex blocks of the diagonal"""
    A = sp.csr_matrix(A)
    nv = A.shape[0] // nf
    i = np.arange(nv)
    D = np.zeros((nv, nf, nf))
    for f in range(nf):
        for g in range(nf):
            D[:, f, g] = np.asarray(A[f * nv + i, g * nv + i]).ravel()
    return D


def block_solve(D, v):
    """D^-1 v, v in the external layout"""
    nv, nf, _ = D.shape
    x = np.linalg.solve(D, v.reshape(nf, nv).T[:, :, None])[:, :, 0]
    return np.ascontiguousarray(x.T).ravel()


def restrict(A, nf, owned):
    """(owned x owned part of A, the dof mask) of a boolean vertex mask"""
    m = np.tile(np.asarray(owned, dtype=bool), nf)
    S = sp.diags(m.astype(float))
    return (S @ sp.csr_matrix(A) @ S).tocsr(), m


def coefficients(steps, lmax, lmin):
    """(1 / theta, [a_1 .. a_{k-1}], [b_1 .. b_{k-1}])"""
    assert lmax > lmin > 0
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho, a, b = 1.0 / sigma, [], []
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        a.append(rho_new * rho)
        b.append(2.0 * rho_new / delta)
        rho = rho_new
    return 1.0 / theta, a, b


def bounds(lambda_est, eig_boost=1.1, eig_ratio=10.0, lambda_max=0.0):
    lmax = lambda_max if lambda_max > 0 else eig_boost * lambda_est
    return lmax, lmax / eig_ratio


def apply(A, nf, d, steps, lmax=None, lmin=None, owned=None):
    """z = q(D^-1 A) D^-1 d"""
    A = sp.csr_matrix(A)
    D = diag_blocks(A, nf)
    d = np.asarray(d, dtype=float)
    if owned is not None:
        A, m = restrict(A, nf, owned)
        own = np.asarray(owned, dtype=bool)
        D = D.copy()
        D[~own] = np.eye(nf)
        d = np.where(m, d, 0.0)
    if steps == 1:
        return block_solve(D, d)
    it, a, b = coefficients(steps, lmax, lmin)
    r = d.copy()
    p = block_solve(D, d) * it
    z = p.copy()
    for i in range(1, steps):
        r = r - A @ p
        p = a[i - 1] * p + b[i - 1] * block_solve(D, r)
        z = z + p
    return z


def start_vector(nv, nf):
    return np.array([idr_ref.shadow_entry(g, 4, f) for f in range(nf) for g in range(nv)])


def power_estimate(A, nf, iters=20):
    """lambda_est of the global operator"""
    A = sp.csr_matrix(A)
    D = diag_blocks(A, nf)
    w = start_vector(A.shape[0] // nf, nf)
    prev = w
    for _ in range(iters):
        prev, w = w, block_solve(D, A @ w)
    return float(np.linalg.norm(w) / np.linalg.norm(prev))


def preconditioner(A, nf, steps=3, eig_ratio=10.0, eig_iters=20, eig_boost=1.1, lambda_max=0.0):
    """d -> z with the library's defaults for the bounds"""
    lmax = lmin = None
    if steps > 1:
        est = 0.0 if lambda_max > 0 else power_estimate(A, nf, eig_iters)
        lmax, lmin = bounds(est, eig_boost, eig_ratio, lambda_max)
    return lambda d: apply(A, nf, d, steps, lmax, lmin)


def polynomial(steps, lmax, lmin):
    """q as a numpy Chebyshev-basis polynomial in lambda: 1 - lambda q(lambda) =
    T_k((theta - lambda) / delta) / T_k(sigma), k = steps"""
    from numpy.polynomial import chebyshev as C, polynomial as Pn
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    tk = C.Chebyshev.basis(steps)
    # T_k(s) as a power series in lambda, s = (theta - lambda) / delta
    s = Pn.Polynomial([theta / delta, -1.0 / delta])
    res = tk.convert(kind=Pn.Polynomial)(s) / tk(sigma)
    one_minus = Pn.Polynomial([1.0]) - res
    assert abs(one_minus.coef[0]) <= 1e-12 * max(1.0, np.max(np.abs(one_minus.coef)))
    return Pn.Polynomial(one_minus.coef[1:])  # divided by lambda


def bicgstab(A, b, M=None, reduction=1e-8, maxit=20000):
    """ISTL BiCGSTABSolver with its half-step counting (zero start): (x, it_half, converged)"""
    M = M or (lambda v: v)
    x = np.zeros_like(b)
    r = b.copy()
    rt = b.copy()
    p = np.zeros_like(b)
    v = np.zeros_like(b)
    rho = alpha = omega = 1.0
    norm0 = np.linalg.norm(r)
    if norm0 == 0:
        return x, 0.0, True
    for it in range(1, maxit + 1):
        rho_new = rt @ r
        if abs(rho) <= 1e-80 or abs(omega) <= 1e-80:
            return x, it - 1.0, False
        beta = (rho_new / rho) * (alpha / omega)
        p = r.copy() if it == 1 else r + beta * (p - omega * v)
        y = M(p)
        v = A @ y
        h = rt @ v
        if abs(h) <= 1e-80:
            return x, it - 1.0, False
        alpha = rho_new / h
        x = x + alpha * y
        r = r - alpha * v
        if np.linalg.norm(r) < reduction * norm0:
            return x, it - 0.5, True
        y = M(r)
        t = A @ y
        omega = (t @ r) / (t @ t)
        x = x + omega * y
        r = r - omega * t
        rho = rho_new
        if np.linalg.norm(r) < reduction * norm0:
            return x, float(it), True
    return x, float(maxit), False


def cg(A, b, M=None, reduction=1e-8, maxit=20000):
    """ISTL CGSolver (zero start): (x, iterations, converged)"""
    M = M or (lambda v: v)
    x = np.zeros_like(b)
    r = b.copy()
    norm0 = np.linalg.norm(r)
    if norm0 == 0:
        return x, 0, True
    p = M(r)
    rho = p @ r
    for it in range(1, maxit + 1):
        q = A @ p
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        if np.linalg.norm(r) < reduction * norm0:
            return x, it, True
        q = M(r)
        rho_new = q @ r
        p = q + (rho_new / rho) * p
        rho = rho_new
    return x, maxit, False
