"""The aggregation AMG (PNP_PREC_AMG) restated in plain numpy / scipy: the V-cycle of
pnp_ctx::amg_apply, the level-0 smoothers it is built from (the multicolour SSOR sweep of
k_sgs_color, the multicolour ILU(0)), the aggregation of amg_setup.cc and the conditioning of what
the cycle inverts.  No GPU; test infrastructure only.  tests/test_amg_ref_host.py holds the pieces
to each other on the CPU, tests/test_gpu_amg.py and tests/test_gpu_amg_edges.py hold the kernels
to them.  The single applications of PNP_PREC_ILU0 (every PNP_OPT_ILU_F32 storage), PNP_PREC_SSOR
and PNP_PREC_JACOBI restated here are held to themselves by tests/test_sweep_ref_host.py and the
kernels to them by tests/test_gpu_sweep_edges.py.

Orders.  External vectors are field-major over the global vertices, f * nv + g.  The kernels work
in the layout's order: P.Layout rows 0 .. n_owned - 1 (colour-major), the fields of a row ascending;
local_perm() lists the external index of every unknown in that order, and every matrix here is
J[perm][:, perm] -- on more than one rank the owned x owned block, ghost columns dropped."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

MAX_DENSE = 3072           # amg.h kAmgMaxDense
MAX_COARSE = MAX_DENSE // 3
MAX_LEVELS = 16

# stored block patterns (dune-pnp_amd/csrc/kernels.h kPatPnp / kPatPnpIE): PnpOperator has no
# c+/c- coupling; PnpTOperator's c- mass term lands in the c+ rows (quirk Q2) -> (1,2) present
PATS = {"pnp": [(f, g) for f in range(3) for g in range(3) if (f, g) not in ((1, 2), (2, 1))],
        "pnp_ie": [(f, g) for f in range(3) for g in range(3) if (f, g) != (2, 1)],
        "pb": [(0, 0)]}
# the scalar operators (P1 names of tests/test_gpu_fan_walks.py, P_k names of tests/test_gpu_pk.py)
PATS.update({k: [(0, 0)] for k in ("poisson", "diff", "diff+", "diff-", "diff_ie", "diff_ie+",
                                   "diff_ie-")})


def interleave(A, nv, nf):
    perm = np.array([f * nv + v for v in range(nv) for f in range(nf)])
    return A[perm][:, perm].tocsr(), perm


def local_perm(lay, nf, nv):
    """external index of (row r, field f), rows 0 .. n_owned - 1, fields ascending inside a row"""
    own = lay.l2g[:lay.n_owned].astype(np.int64)
    return (own[:, None] + nv * np.arange(nf)[None, :]).ravel()


def numpy_vcycle(A0, nf, aggs, omega, d, sweeps=2, pre0=True, f32=True, smooth0=None, inv=None):
    """The V-cycle of amg.hip restated: level-0 smoothing x0 = smooth0(d) before (pre0) and
    y + smooth0(d - A0 y) after the correction (smooth0 None: pointwise Jacobi), `sweeps` damped
    block-Jacobi sweeps before and after the correction on the coarse levels, exact solve on the
    coarsest; one coarse level (len(aggs) == 1) is restriction, that solve and prolongation.
    f32 (PNP_AMG_F32, the default): the coarse levels' sweeps and residuals multiply by
    the block values rounded to single precision, the coarsest solve by the inverse rounded to
    single precision; the Galerkin products and the diagonal inverses use the fp64 values.
    inv: the dense inverse that is rounded (numpy.linalg.inv)."""
    As, Ps = [A0], []
    for agg in aggs:
        n = As[-1].shape[0] // nf
        Pv = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, int(agg.max()) + 1))
        Pm = sp.kron(Pv, sp.identity(nf), format="csr")
        Ps.append(Pm)
        As.append((Pm.T @ As[-1] @ Pm).tocsr())
    K = len(aggs)
    Ad = As  # fp64: Galerkin (above), diagonal inverses, coarsest solve
    if f32:
        As = [A if k in (0, K) else sp.csr_matrix(
            (A.data.astype(np.float32).astype(np.float64), A.indices, A.indptr), shape=A.shape)
            for k, A in enumerate(Ad)]

    def dinv(A):
        nb = A.shape[0] // nf
        D = np.zeros((nb, nf, nf))
        C = A.tocoo()
        m = (C.row // nf) == (C.col // nf)
        np.add.at(D, (C.row[m] // nf, C.row[m] % nf, C.col[m] % nf), C.data[m])
        return np.linalg.inv(D)

    def bj(A, Di, r):
        return np.einsum("bij,bj->bi", Di, r.reshape(-1, nf)).ravel()

    Dis = [None] + [dinv(Ad[k]) for k in range(1, K)]
    if smooth0 is None:
        diag0 = A0.diagonal()

        def smooth0(r):
            return r / diag0
    x0 = smooth0(d) if pre0 else np.zeros_like(d)
    b, x = [None] * (K + 1), [None] * (K + 1)
    b[1] = Ps[0].T @ (d - A0 @ x0)
    if K > 1:
        x[1] = omega * bj(As[1], Dis[1], b[1])
    for k in range(1, K):
        for _ in range(sweeps - 1):
            x[k] = x[k] + omega * bj(As[k], Dis[k], b[k] - As[k] @ x[k])
        b[k + 1] = Ps[k].T @ (b[k] - As[k] @ x[k])
        if k + 1 < K:
            x[k + 1] = omega * bj(As[k + 1], Dis[k + 1], b[k + 1])
    if f32:
        e = (inv or np.linalg.inv)(Ad[K].toarray()).astype(np.float32).astype(np.float64) @ b[K]
    else:
        e = np.linalg.solve(Ad[K].toarray(), b[K])
    for k in range(K - 1, 0, -1):
        xc = x[k] + Ps[k] @ e
        e = xc + omega * bj(As[k], Dis[k], b[k] - As[k] @ xc)
        for _ in range(sweeps - 1):
            e = e + omega * bj(As[k], Dis[k], b[k] - As[k] @ e)
    y = x0 + Ps[0] @ e
    return y + smooth0(d - A0 @ y)


# ---- the multicolour sweeps -------------------------------------------------------------------
def mask_same_colour(A, lay, nf):
    """A (the owned unknowns in the layout's order) with every coupling between two different rows
    of one colour (the absorbed thin colour's conflicts, mesh.cc absorb_top) set to zero: the
    sweeps' split storage has no slot for them"""
    C = A.tocoo()
    colour = lay.rowcolor[:lay.n_owned].astype(np.int64)
    ri, ci = C.row // nf, C.col // nf
    keep = (ri == ci) | (colour[ri] != colour[ci])
    Ap = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=C.shape)
    Ap.sum_duplicates()
    Ap.sort_indices()
    return Ap


def colour_masked(J, lay, nf):
    """(Ap, perm): the Jacobian on the owned unknowns in the layout's order, same-colour couplings
    dropped"""
    perm = local_perm(lay, nf, J.shape[0] // nf)
    return mask_same_colour(J.tocsr()[perm][:, perm], lay, nf), perm


def ssor_sweep(Ap, r):
    """one point Gauss-Seidel sweep forward from zero, then one backward (ISTL SeqSSOR, one
    iteration, w = 1): (D + U)^-1 D (D + L)^-1 r by two sparse triangular solves"""
    lo = sp.tril(Ap, 0, format="csr")
    up = sp.triu(Ap, 0, format="csr")
    w = spla.spsolve_triangular(lo, np.asarray(r, dtype=np.float64), lower=True)
    return spla.spsolve_triangular(up, Ap.diagonal() * w, lower=False)


def ssor_sweep_oracle(Ap, r):
    """the same sweep by the CPU oracle's natural-order SeqSSOR on Ap"""
    import oracle_py as O
    return O.prec_apply(Ap, r, O.PREC_SSOR)


def multicolour_ssor(J, lay, nf, d, owned=None, oracle=False):
    """pnp_prec_apply(PNP_PREC_SSOR) restated from k_sgs_color: the sweep of ssor_sweep over the
    layout's owned rows in their colour-major order, fields ascending, same-colour couplings
    dropped.  d and the result are external vectors; the result is zero outside the rank's owned
    unknowns.  owned: the owned global vertices when the caller has them (checked against the
    layout's); oracle: the sweep by the CPU oracle's SeqSSOR instead of the triangular solves."""
    Ap, perm = colour_masked(J, lay, nf)
    assert owned is None or np.array_equal(np.sort(owned), np.sort(lay.l2g[:lay.n_owned]))
    v = np.zeros(J.shape[0])
    v[perm] = (ssor_sweep_oracle if oracle else ssor_sweep)(Ap, np.asarray(d)[perm])
    return v


def ilu0_dense(A, M):
    """Textbook IKJ ILU(0) restricted to the pattern M (Saad, Alg. 10.4); pivots not inverted."""
    A = A.copy()
    n = A.shape[0]
    for i in range(n):
        for k in np.nonzero(M[i, :i])[0]:
            A[i, k] /= A[k, k]
            q = np.nonzero(M[i, k + 1:] & M[k, k + 1:])[0] + k + 1
            A[i, q] -= A[i, k] * A[k, q]
    return A


def ilu0_dense_recip(A, M):
    """(F, dinv): the same factorisation in the kernels' form (k_ilu0_factor, k_ilu0_factor_fused):
    a row's pivot is inverted once, when the row is finished, and the rows below multiply by the
    stored reciprocal.  F's diagonal holds the pivots themselves, dinv their reciprocals.  Differs
    from ilu0_dense by rounding only."""
    A = A.copy()
    n = A.shape[0]
    dinv = np.zeros(n)
    for i in range(n):
        for k in np.nonzero(M[i, :i])[0]:
            A[i, k] *= dinv[k]
            q = np.nonzero(M[i, k + 1:] & M[k, k + 1:])[0] + k + 1
            A[i, q] -= A[i, k] * A[k, q]
        dinv[i] = 1.0 / A[i, i]
    return A, dinv


# The factors' storage roundings, from linalg.hip: the fused factorisation computes in fp64 and
# writes every value of the split L / U storage -- the couplings, the diagonal block's lower and
# upper entries and its inverted pivots -- once, as float(x) (PNP_OPT_ILU_F32 = 1) or as
# to_bf16(float(x)) (= 2, 3); the sweeps convert back and compute in fp64.
def round_f32(a):
    """double -> float, round to nearest even (the kernels' float(x)), as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def round_bf16(a):
    """linalg.hip to_bf16(float(x)): the double rounded to float, the float's upper 16 bits after
    adding 0x7FFF and the lowest kept bit (round to nearest, ties to even), as float64"""
    u = np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


STORE_ROUND = {0: lambda a: np.asarray(a, dtype=np.float64), 1: round_f32, 2: round_bf16}


def ilu0_mode(mode, nf):
    """(storage, y32) of PNP_OPT_ILU_F32 = mode on a system of nf fields (ctx.h ilu_eff / ilu_fac /
    ilu_y32): storage 0 fp64, 1 float, 2 bfloat16; y32: the forward intermediate in single
    precision.  Scalar systems run modes 2 and 3 as mode 1."""
    if nf == 1 and mode >= 2:
        mode = 1
    return (2, True) if mode == 3 else (mode, False)


def ilu0_system(J, lay, nf, pat, drop=True):
    """(Ap, M, perm): the rank's owned x owned block of J in the layout's order (dense; ghost
    columns are outside the pattern, k_ilu0_factor's m >= L.n_owned) and the stored block pattern
    `pat` (a list of (f, g)) on it as a mask -- drop: without the couplings of two different rows
    of one colour, which the split storage has no slot for"""
    nv, n = J.shape[0] // nf, lay.n_owned
    perm = local_perm(lay, nf, nv)
    Ap = J.tocsr()[perm][:, perm].toarray()
    M = np.zeros_like(Ap, dtype=bool)
    colour = lay.rowcolor[:n]
    same = []
    for r in range(n):
        for c in lay.row_cols(r):
            if c >= n:
                continue
            for f, g in pat:
                M[r * nf + f, c * nf + g] = True
            if c != r and colour[c] == colour[r]:
                same.append((r, c))
    assert not np.any(Ap[~M]), "Jacobian has entries outside the stored pattern"
    if drop:
        for r, c in same:
            M[r * nf:(r + 1) * nf, c * nf:(c + 1) * nf] = False
    return Ap, M, perm


def ilu0_factors(Ap, M, recip=False, store=0):
    """(L, U, dinv): strictly lower and strictly upper factors (CSR) and the inverse pivots of the
    ILU(0) of Ap on the pattern M, by ilu0_dense (recip False) or ilu0_dense_recip, each stored
    value rounded once as the storage `store` does (STORE_ROUND)"""
    return ilu0_stored(*ilu0_fp64(Ap, M, recip), store)


def ilu0_fp64(Ap, M, recip=False):
    """(L, U, dinv) in fp64, before any storage rounding: the factorisation is done once, however
    many storages are then restated from it"""
    if recip:
        F, dinv = ilu0_dense_recip(Ap, M)
    else:
        F = ilu0_dense(Ap, M)
        dinv = 1.0 / np.diag(F)
    F = np.where(M, F, 0.0)  # a dropped coupling is in neither factor
    return sp.csr_matrix(np.tril(F, -1)), sp.csr_matrix(np.triu(F, 1)), dinv


def ilu0_stored(L, U, dinv, store):
    """the fp64 factors as the storage `store` holds them: every value rounded once"""
    rnd = STORE_ROUND[store]
    return (sp.csr_matrix((rnd(L.data), L.indices, L.indptr), shape=L.shape),
            sp.csr_matrix((rnd(U.data), U.indices, U.indptr), shape=U.shape), rnd(dinv))


def ilu0_sweep(L, U, dinv, r, nf=1, y32=None):
    """(LU)^-1 r as k_ilu0_solve does it: y = r - L y forward, x = (y - U x) dinv backward (the
    pivots multiply), in fp64.  y32 (PNP_OPT_ILU_F32 = 3): a boolean per unknown, true where the
    row's colour is not the last -- such a row's finished y is stored in single precision, and
    the rows of other vertices and its own backward step read it from there; the fields of one
    vertex are finished in registers first, so they read each other unrounded."""
    n = len(r)
    y, ys = np.zeros(n), np.zeros(n)
    for i in range(n):
        s, e = L.indptr[i], L.indptr[i + 1]
        idx = L.indices[s:e]
        src = y[idx] if y32 is None else np.where(idx // nf == i // nf, y[idx], ys[idx])
        y[i] = r[i] - L.data[s:e] @ src
        ys[i] = round_f32(y[i]) if y32 is not None and y32[i] else y[i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s, e = U.indptr[i], U.indptr[i + 1]
        x[i] = (ys[i] - U.data[s:e] @ x[U.indices[s:e]]) * dinv[i]
    return x


def ilu0_operator(J, lay, nf, pat, recip=False, mode=0, drop=True):
    """(apply, perm): apply(r) = (LU)^-1 r in the layout's order, L and U the ILU(0) factors of
    the rank's owned x owned block of the Jacobian on the stored block pattern `pat` without the
    same-colour couplings (drop False: with them, which no kernel does).  mode: PNP_OPT_ILU_F32,
    restated by ilu0_mode / ilu0_factors / ilu0_sweep; recip: the factorisation in the kernels'
    form.  Dense, so for a few thousand unknowns."""
    Ap, M, perm = ilu0_system(J, lay, nf, pat, drop)
    store, y32 = ilu0_mode(mode, nf)
    L, U, dinv = ilu0_factors(Ap, M, recip, store)
    rows32 = None
    if y32:
        rows32 = np.repeat(lay.rowcolor[:lay.n_owned] != lay.ncolors - 1, nf)

    def apply(r):
        return ilu0_sweep(L, U, dinv, np.asarray(r, dtype=np.float64), nf, rows32)
    return apply, perm


def ilu0_apply(J, lay, nf, pat, d, **kw):
    """pnp_prec_apply(PNP_PREC_ILU0) restated (fp64 factors unless mode says otherwise); external
    vectors, zero outside the rank's owned unknowns"""
    apply, perm = ilu0_operator(J, lay, nf, pat, **kw)
    v = np.zeros(J.shape[0])
    v[perm] = apply(np.asarray(d, dtype=np.float64)[perm])
    return v


def jacobi_apply(J, lay, nf, pat, d):
    """pnp_prec_apply(PNP_PREC_JACOBI) restated from k_jacobi: every owned unknown divided by its
    own diagonal entry (pointwise, not by the vertex block; a constrained row's is 1); external
    vectors, zero outside the rank's owned unknowns"""
    assert all((f, f) in pat for f in range(nf))
    perm = local_perm(lay, nf, J.shape[0] // nf)
    v = np.zeros(J.shape[0])
    v[perm] = np.asarray(d, dtype=np.float64)[perm] / J.tocsr()[perm][:, perm].diagonal()
    return v


# ---- the hierarchy ------------------------------------------------------------------------------
def aggregate(n, neighbours):
    """amg_aggregate (amg_setup.cc): neighbours[i] lists row i's graph neighbours (not i itself) in
    stored order.  Pass 1: a root whose neighbours are all free takes them; pass 2: the rest join
    the first pass-1 aggregate among their neighbours; pass 3: singletons.  Returns (agg, count)."""
    agg = np.full(n, -1, dtype=np.int64)
    na = 0
    for i in range(n):
        if agg[i] >= 0 or any(agg[j] >= 0 for j in neighbours[i]):
            continue
        agg[i] = na
        for j in neighbours[i]:
            agg[j] = na
        na += 1
    join = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        if agg[i] < 0:
            for j in neighbours[i]:
                if agg[j] >= 0:
                    join[i] = agg[j]
                    break
    take = (agg < 0) & (join >= 0)
    agg[take] = join[take]
    for i in range(n):
        if agg[i] < 0:
            agg[i] = na
            na += 1
    return agg, na


def hierarchy(lay, coarse_target=1024, max_levels=12):
    """amg_build (amg_setup.cc) restated: {"aggs": [aggregate of every row of level k, k = 0 ..],
    "rows": [rows of level 0, 1, ..], "blocks": [None, stored blocks of level 1, ..]}.  Level 0's
    graph: lay.row_cols(i) in slot order, owned columns only; a coarse level's: its distinct
    (aggregate, aggregate) pairs, columns ascending."""
    n = lay.n_owned
    coarse_target = max(1, min(coarse_target, MAX_COARSE))
    max_levels = max(2, min(max_levels, MAX_LEVELS))
    cols = [[j for j in lay.row_cols(i) if j < n] for i in range(n)]
    pr = np.repeat(np.arange(n), [len(c) for c in cols])
    pc = np.array([j for c in cols for j in c], dtype=np.int64)
    nbr = [[j for j in c if j != i] for i, c in enumerate(cols)]
    out = {"aggs": [], "rows": [n], "blocks": [None]}
    nrows = n
    while len(out["aggs"]) + 1 < max_levels:
        agg, na = aggregate(nrows, nbr)
        if na >= nrows and out["aggs"]:
            break  # no coarsening possible
        pairs = np.unique(np.stack([agg[pr], agg[pc]], axis=1), axis=0)  # sorted by (row, col)
        pr, pc = pairs[:, 0], pairs[:, 1]
        out["aggs"].append(agg)
        out["rows"].append(na)
        out["blocks"].append(len(pairs))
        nrows = na
        if nrows <= coarse_target:
            break
        nbr = [[] for _ in range(nrows)]
        for i, j in pairs:
            if i != j:
                nbr[i].append(int(j))
    return out


def galerkin(A0, nf, aggs):
    """[A0, A1, ..]: A_{k+1} = P^T A_k P with the piecewise-constant prolongation of aggs[k]"""
    As = [A0.tocsr()]
    for agg in aggs:
        n = As[-1].shape[0] // nf
        Pv = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, int(np.max(agg)) + 1))
        Pm = sp.kron(Pv, sp.identity(nf), format="csr")
        As.append((Pm.T @ As[-1] @ Pm).tocsr())
    return As


def diagonal_blocks(A, nf):
    nb = A.shape[0] // nf
    D = np.zeros((nb, nf, nf))
    C = A.tocoo()
    m = (C.row // nf) == (C.col // nf)
    np.add.at(D, (C.row[m] // nf, C.row[m] % nf, C.col[m] % nf), C.data[m])
    return D


def conditioning(A0, nf, aggs):
    """(cond_2 of the coarsest Galerkin matrix, the largest cond_2 over the diagonal blocks of the
    coarse levels that are smoothed: 0.0 when there is none).  The 1e-10 comparisons mean something
    only while an fp64 inverse of these is itself good to about 1e-12: both at most 1e6."""
    As = galerkin(A0, nf, aggs)
    worst = 0.0
    for A in As[1:-1]:
        worst = max(worst, float(np.max(np.linalg.cond(diagonal_blocks(A, nf)))))
    return float(np.linalg.cond(As[-1].toarray())), worst
