"""The case table of tests/sweep_cases.py held to P.Layout and to the reference alone, and the new
pieces of tests/amg_ref.py held to themselves (no GPU).

tests/test_gpu_sweep_edges.py compares one application of the multicolour ILU(0), of the
multicolour SSOR and of Jacobi with the restatements of tests/amg_ref.py.  A case is named after
what its layout reaches (a colour of exactly 256 rows, a same-colour coupling, a staging list past
1,024 entries, ..), and a comparison at 1e-10 means something only while the reference itself is
that good.  Both are properties of the mesh, the layout and the Jacobian, so they are checked here
with P.Layout and the CPU oracle's Jacobians:
  * the layout figures of every rank (rows, colour sizes, conflicts, max_slots, sx_max), exactly;
    sweep_usable = 1; at P_k the layout's graph in l2g numbering is the pattern of the oracle's
    PkSpace Jacobian entry for entry, so the oracle's matrix is ordered by lay.l2g directly;
  * every pivot of the textbook ILU(0) on the colour-major order is finite and non-zero;
  * N, the distance between two fp64 forms of the reference that differ by rounding only (dividing
    by the pivot, multiplying by its stored reciprocal), is at most 1e-12 of max|v|;
  * rounding the stored factors to float moves the application by at most 2e-5, to bfloat16 (block
    systems only: scalar systems never store bfloat16) by at most 2e-2, the project's bounds for
    these storages (tests/test_gpu.py);
  * in a case with same-colour couplings the reference with and without the dropping differ by more
    than 1e-6 for the ILU(0) and for the SSOR sweep, so a kernel that forgot to drop would show;
    where the rows pass 16 slots, so does a factorisation that only lets the dropped couplings
    into its updates (forgetful_update).
A case that misses one of these for the reference alone is replaced, not loosened."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import amg_ref as R
import pnp_amd as P
import sweep_cases as SC
from test_gpu_fan_walks import set_kind
from test_gpu_pk import KINDS as PK_KINDS, args as pk_args

N_BOUND, F32_BOUND, BF16_BOUND, SEES_DROP = 1e-12, 2e-5, 2e-2, 1e-6


def pk_operator(orc, S, kind, degree):
    """(oracle operator, state) of a P_k case's kind, seeded as the GPU test seeds it"""
    x, kw = pk_args(kind, S.nn, 100 * degree + SC.PK_KINDS.index(kind))
    field = 2 if kind.startswith("diff") else 0
    return orc.operator(PK_KINDS[kind][1], flux=orc.flux(), mask=S.mask(field), **kw), x, kw


@functools.lru_cache(maxsize=None)
def oracle_jacobian(case_id, kind):
    """the CPU oracle's Jacobian of one kind of a case, over the global vertices / nodes"""
    c = SC.BY_ID[case_id]
    if c.degree == 1:
        _, _, orc, st = SC.p1_problem(case_id)
        op, x = set_kind(None, orc, st, kind)
        return orc.jacobian(op, x).tocsr()
    _, _, orc, S = SC.pk_problem(case_id)
    op, x, _ = pk_operator(orc, S, kind, c.degree)
    return S.jacobian(op, x).tocsr()


def relative(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def reference_figures(J, lay, nf, pat, d):
    """pivots, N and the rounded-factor distances of the reference on one rank's block"""
    Ap, M, perm = R.ilu0_system(J, lay, nf, pat)
    r = d[perm]
    fp64 = {recip: R.ilu0_fp64(Ap, M, recip) for recip in (False, True)}
    fac = {(recip, st): R.ilu0_stored(*fp64[recip], st) for recip in (False, True)
           for st in (0, 1, 2)}
    v = {k: R.ilu0_sweep(*f, r, nf) for k, f in fac.items()}
    piv = 1.0 / fac[(False, 0)][2]
    fig = dict(n=len(r), pivot_min=float(np.min(np.abs(piv))), pivot_max=float(np.max(np.abs(piv))),
               N=relative(v[(True, 0)], v[(False, 0)]), f32=relative(v[(True, 1)], v[(True, 0)]))
    if nf > 1:
        fig["bf16"] = relative(v[(True, 2)], v[(True, 0)])
    return fig, (Ap, M, perm, v[(False, 0)])


def forgetful_update(J, lay, nf, pat, r):
    """the ILU(0) application of a factorisation that neither eliminates by a same-colour coupling
    nor stores it, but lets it take part in the updates (the update step of k_ilu0_factor_fused
    without its dropped() line, on a layout whose rows live in the scratch: max_slots > 16)"""
    Ap, M, _ = R.ilu0_system(J, lay, nf, pat)
    kept = R.ilu0_system(J, lay, nf, pat, drop=False)[1]
    F = R.ilu0_dense(Ap, M | np.triu(kept & ~M, 1))
    dinv = 1.0 / np.diag(F)
    F = np.where(M, F, 0.0)
    return R.ilu0_sweep(sp.csr_matrix(np.tril(F, -1)), sp.csr_matrix(np.triu(F, 1)), dinv, r, nf)


@pytest.mark.parametrize("case_id", SC.IDS)
def test_layout_figures(case_id):
    c = SC.BY_ID[case_id]
    mesh = SC.mesh_of(case_id)
    figs = []
    for rank in range(c.nranks):
        lay = P.Layout(mesh, rank, c.nranks, degree=c.degree)
        fig = SC.layout_figures(lay)
        figs.append(fig)
        print(f"{c.id} rank {rank}: {fig}")
        for key, want in c.expect[rank].items():
            assert fig[key] == want, (c.id, rank, key, fig[key], want)
        assert fig["sweep_usable"] == 1 and fig["lsx_entries"] > 0
        if c.nranks > 1:
            assert 0 < lay.n_owned < len(set(lay.l2g)) and lay.n_ghost > 0
    for flag in c.flags:
        assert any(SC.flag_holds(flag, f, c.degree) for f in figs), (c.id, flag, figs)
    if c.family != "conflict":
        assert all(f["conflicts"] == 0 for f in figs)


@pytest.mark.parametrize("case_id", [c.id for c in SC.TABLE if c.degree > 1 and c.nranks == 1])
def test_pk_layout_graph_is_the_oracles_pattern(case_id):
    """product and oracle number the P_k nodes alike: (l2g[row], l2g[column]) over the layout's
    slots is the oracle Jacobian's stored pattern, entry for entry"""
    c = SC.BY_ID[case_id]
    mesh, _, _, S = SC.pk_problem(case_id)
    lay = P.Layout(mesh, degree=c.degree)
    assert lay.n_owned == S.nn and lay.n_ghost == 0
    rows = np.repeat(np.arange(S.nn), [lay.row_len(i) for i in range(S.nn)])
    cols = np.array([q for i in range(S.nn) for q in lay.row_cols(i)])
    G = sp.csr_matrix((np.ones(len(rows)), (lay.l2g[rows], lay.l2g[cols])), shape=(S.nn, S.nn))
    assert G.nnz == len(rows)  # no pair twice
    Jo = oracle_jacobian(case_id, "pb")
    Jo.sort_indices()
    G.sort_indices()
    assert np.array_equal(G.indptr, Jo.indptr) and np.array_equal(G.indices, Jo.indices)


@pytest.mark.parametrize("case_id", SC.IDS)
def test_reference_is_well_conditioned_on_the_case(case_id):
    c = SC.BY_ID[case_id]
    mesh = SC.mesh_of(case_id)
    for kind in c.kinds:
        J = oracle_jacobian(case_id, kind)
        nf = SC.nfields(kind)
        d = SC.rhs(J.shape[0])
        for rank in range(c.nranks):
            lay = P.Layout(mesh, rank, c.nranks, degree=c.degree)
            fig, (Ap, M, perm, v) = reference_figures(J, lay, nf, R.PATS[kind], d)
            print(f"{c.id}/{kind} rank {rank}: colours {SC.layout_figures(lay)['colours']} conflicts "
                  f"{lay.color_conflicts} sx_max {lay.derived.sx_max} " +
                  " ".join(f"{k} {q:.2e}" if isinstance(q, float) else f"{k} {q}"
                           for k, q in fig.items()))
            assert np.isfinite(fig["pivot_max"]) and fig["pivot_min"] > 0
            assert fig["N"] <= N_BOUND and fig["f32"] <= F32_BOUND
            assert fig.get("bf16", 0.0) <= BF16_BOUND
            if lay.color_conflicts:
                vk = R.ilu0_sweep(*R.ilu0_factors(*R.ilu0_system(J, lay, nf, R.PATS[kind],
                                                                 drop=False)[:2]), d[perm], nf)
                A = sp.csr_matrix(Ap)
                sd = R.ssor_sweep(R.mask_same_colour(A, lay, nf), d[perm])
                sk = R.ssor_sweep(A, d[perm])
                di, ds = relative(vk, v), relative(sk, sd)
                print(f"{c.id}/{kind}: kept against dropped couplings: ILU(0) {di:.2e} "
                      f"SSOR {ds:.2e}")
                assert di > SEES_DROP and ds > SEES_DROP
                if lay.max_slots > 16:
                    du = relative(forgetful_update(J, lay, nf, R.PATS[kind], d[perm]), v)
                    print(f"{c.id}/{kind}: updates through the dropped couplings: ILU(0) {du:.2e}")
                    assert du > SEES_DROP
        if c.family == "conflict":
            assert P.Layout(mesh, degree=c.degree).color_conflicts >= 1


# ---- the reference against itself ----------------------------------------------------------------
def random_system(n=40, seed=6, density=0.25):
    rng = np.random.default_rng(seed)
    M = rng.uniform(size=(n, n)) < density
    M |= M.T | np.eye(n, dtype=bool)
    A = np.where(M, rng.standard_normal((n, n)), 0.0) + n * density * np.eye(n)
    return A, M, rng.standard_normal(n)


def test_the_two_fp64_forms_agree():
    A, M, r = random_system()
    Fd = R.ilu0_dense(A, M)
    Fr, dinv = R.ilu0_dense_recip(A, M)
    assert np.max(np.abs(Fd - Fr)) <= 1e-13 * np.max(np.abs(Fd))
    assert np.max(np.abs(dinv * np.diag(Fd) - 1.0)) <= 1e-13
    assert np.array_equal(Fd[~M], A[~M])  # nothing outside the pattern is touched
    a = R.ilu0_sweep(*R.ilu0_factors(A, M, False), r)
    b = R.ilu0_sweep(*R.ilu0_factors(A, M, True), r)
    assert relative(b, a) <= 1e-13


def test_recip_form_of_a_full_pattern_is_lu():
    rng = np.random.default_rng(6)
    A = rng.standard_normal((12, 12)) + 12 * np.eye(12)
    Fm, dinv = R.ilu0_dense_recip(A, np.ones_like(A, dtype=bool))
    assert np.allclose((np.tril(Fm, -1) + np.eye(12)) @ np.triu(Fm), A, rtol=0, atol=1e-12)
    L, U, di = R.ilu0_factors(A, np.ones_like(A, dtype=bool), True)
    r = rng.standard_normal(12)
    assert relative(R.ilu0_sweep(L, U, di, r), np.linalg.solve(A, r)) <= 1e-12


def test_sweep_is_the_two_triangular_solves():
    A, M, r = random_system(seed=7)
    L, U, dinv = R.ilu0_factors(A, M)
    lo = L.toarray() + np.eye(len(r))
    up = U.toarray() + np.diag(1.0 / dinv)
    ref = sla.solve_triangular(up, sla.solve_triangular(lo, r, lower=True), lower=False)
    assert relative(R.ilu0_sweep(L, U, dinv, r), ref) <= 1e-13
    # a dropped coupling is in neither factor although the matrix has it
    M2 = M.copy()
    i, j = np.argwhere(np.tril(M, -1))[0]
    M2[i, j] = M2[j, i] = False
    L2, U2, _ = R.ilu0_factors(A, M2)
    assert A[i, j] != 0 and L2[i, j] == 0 and U2[j, i] == 0


def test_single_precision_intermediate():
    """mode 3's y: no row marked is the fp64 sweep bit for bit; all rows marked with scalar rows is
    a forward sweep whose every stored entry is a float; inside a vertex the fields read each
    other unrounded"""
    A, M, r = random_system(n=30, seed=8)
    L, U, dinv = R.ilu0_factors(A, M, True, 2)
    base = R.ilu0_sweep(L, U, dinv, r)
    assert np.array_equal(R.ilu0_sweep(L, U, dinv, r, 1, np.zeros(30, dtype=bool)), base)
    v3 = R.ilu0_sweep(L, U, dinv, r, 3, np.ones(30, dtype=bool))
    assert 0 < relative(v3, base) <= 1e-6
    # by hand: the forward sweep with vertex blocks of 3
    y, ys = np.zeros(30), np.zeros(30)
    Ld = L.toarray()
    for b in range(10):
        for f in range(3):
            i = 3 * b + f
            y[i] = r[i] - Ld[i, :3 * b] @ ys[:3 * b] - Ld[i, 3 * b:i] @ y[3 * b:i]
        ys[3 * b:3 * b + 3] = np.float32(y[3 * b:3 * b + 3])
    x = np.zeros(30)
    Ud = U.toarray()
    for i in range(29, -1, -1):
        x[i] = (ys[i] - Ud[i] @ x) * dinv[i]
    assert relative(v3, x) <= 1e-14


def test_rounding_helpers():
    rng = np.random.default_rng(9)
    a = np.concatenate([rng.standard_normal(1000) * 10.0 ** rng.integers(-20, 20, 1000),
                        [0.0, -0.0, 1.0, -1.0]])
    assert np.array_equal(R.round_f32(a), np.float32(a).astype(np.float64))
    assert np.array_equal(R.STORE_ROUND[0](a), a)
    b = R.round_bf16(a)
    nz = a != 0
    assert np.all(np.abs(b[nz] - a[nz]) <= 2.0 ** -8 * np.abs(a[nz]))  # half an ulp of 8 bits
    assert np.array_equal(R.round_bf16(b), b)  # idempotent
    assert np.all((np.float32(b).view(np.uint32) & 0xFFFF) == 0)
    e = 2.0 ** -8  # half a bfloat16 ulp at 1
    ties = [(1.0, 1.0), (1.0 + e, 1.0),                # a tie goes to the even mantissa: down
            (1.0 + 3 * e, 1.0 + 4 * e),                # up
            (1.0 + 5 * e, 1.0 + 4 * e), (1.0 + 7 * e, 1.0 + 8 * e),
            (-(1.0 + 3 * e), -(1.0 + 4 * e)), (-(1.0 + e), -1.0),
            (1.0 + e + 2.0 ** -23, 1.0 + 2 * e),       # one float ulp above the tie
            (1.0 + 3 * e - 2.0 ** -23, 1.0 + 2 * e),   # one float ulp below the tie
            (2.0 - e, 2.0),                            # the carry into the exponent
            (0.5 + e / 2, 0.5), (0.5 + 3 * e / 2, 0.5 + 2 * e),
            # the double is rounded to float first: 2^-30 above the tie is lost, the tie goes down
            (1.0 + e + 2.0 ** -30, 1.0),
            (0.0, 0.0), (3.0, 3.0), (1e-3, 0.00099945068359375)]
    for x, want in ties:
        assert R.round_bf16(np.array([x]))[0] == want, (x, want)


def test_modes_of_scalar_and_block_systems():
    assert [R.ilu0_mode(m, 3) for m in range(4)] == [(0, False), (1, False), (2, False), (2, True)]
    assert [R.ilu0_mode(m, 1) for m in range(4)] == [(0, False), (1, False), (1, False),
                                                     (1, False)]
    for kind in ("diff+", "diff-", "diff_ie+", "diff_ie-", "diff", "diff_ie", "poisson", "pb"):
        assert R.PATS[kind] == [(0, 0)]
    assert len(R.PATS["pnp"]) == 7 and len(R.PATS["pnp_ie"]) == 8


@pytest.mark.parametrize("case_id,kind", [("pinwheel_4_3_2", "pnp_ie"), ("half_wheel_21-P2", "pb"),
                                          ("chain32-P2-2ranks", "diff_ie")])
def test_jacobi_is_the_solve_with_the_diagonal(case_id, kind):
    c = SC.BY_ID[case_id]
    J = oracle_jacobian(case_id, kind)
    nf = SC.nfields(kind)
    d = SC.rhs(J.shape[0])
    total = np.zeros(J.shape[0])
    for rank in range(c.nranks):
        lay = P.Layout(SC.mesh_of(case_id), rank, c.nranks, degree=c.degree)
        v = R.jacobi_apply(J, lay, nf, R.PATS[kind], d)
        perm = R.local_perm(lay, nf, J.shape[0] // nf)
        assert np.count_nonzero(v) <= perm.size
        # the diagonal blocks of the pointwise sweep are 1 x 1, one solve per unknown
        ref = np.linalg.solve(J.diagonal()[perm].reshape(-1, 1, 1), d[perm].reshape(-1, 1, 1))
        assert relative(v[perm], ref.ravel()) <= 1e-15
        total += v
    assert relative(total, np.linalg.solve(np.diag(J.diagonal()), d)) <= 1e-15


def test_operator_on_a_rank_uses_the_owned_block():
    """ghost columns are outside the pattern: a rank's factors are those of its owned x owned
    block, whatever the rows couple to beyond it"""
    c = SC.BY_ID["chain32-P2-2ranks"]
    J = oracle_jacobian(c.id, "pb")
    d = SC.rhs(J.shape[0])
    coupled = 0
    for rank in range(2):
        lay = P.Layout(SC.mesh_of(c.id), rank, 2, degree=2)
        apply, perm = R.ilu0_operator(J, lay, 1, R.PATS["pb"])
        ghost = np.ones(J.shape[0])
        ghost[perm] = 0.0
        J2 = (J + 3.0 * J @ sp.diags(ghost)).tocsr()  # the ghost columns' values changed
        coupled += (J2 != J)[perm].nnz  # (a rank whose interface rows are constrained has none)
        apply2, perm2 = R.ilu0_operator(J2, lay, 1, R.PATS["pb"])
        assert np.array_equal(perm, perm2)
        assert np.array_equal(apply(d[perm]), apply2(d[perm]))
        Ap, M, _ = R.ilu0_system(J, lay, 1, R.PATS["pb"])
        assert Ap.shape == (lay.n_owned, lay.n_owned) and M.sum() < sum(
            lay.row_len(i) for i in range(lay.n_owned))
    assert coupled > 0  # the ghost columns did carry values
