"""tests/amg_ref.py held to itself, and the case table of tests/test_gpu_amg_edges.py held to the
reference alone (no GPU).

The GPU tests compare one V-cycle of PNP_PREC_AMG with amg_ref.numpy_vcycle; a case is named after
the kernel path it runs (a coarsest GEMV of several loop trips, a hierarchy down to one block, ..)
and carries the condition under which a 1e-10 comparison means something: cond_2 of the coarsest
Galerkin matrix and of every inverted coarse diagonal block at most 1e6.  Both are properties of
the mesh, the partition and the Jacobian, so they are checked here with the CPU oracle's Jacobians
and the restated aggregation; the GPU tests assert them again on what the library built."""
import collections
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as R
import meshio
import oracle_py as O
import pnp_amd as P
from conftest import DATA
from test_gpu_fan_walks import problem as fan_problem, set_kind

COND_CAP = 1e6
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the case table -----------------------------------------------------------------------------
# n = rows of the coarsest level x fields, the size of the dense coarsest solve.  f32: the default
# process (k_coarse_apply_f32 on rows padded to ld = 4 ceil(n / 4), 64 lanes each taking every 64th
# float4); f64: a process with PNP_AMG_F32=0 (k_coarse_apply<1> for even n, 64 lanes on double2
# pairs two at a time; k_coarse_apply<0> for odd n, four accumulators 64 columns apart).
CLASSES = {
    "f32_one_trip_padded": lambda n: (n + 3) // 4 <= 64 and n % 4 != 0,
    "f32_ragged_trips": lambda n: (n + 3) // 4 > 64 and ((n + 3) // 4) % 64 != 0,
    "f32_scalar_gt_1000": lambda n: n > 1000 and ((n + 3) // 4) % 64 != 0,
    "f64_scalar_gt_1000": lambda n: n > 1000,
    "f64_odd_tail_only": lambda n: n % 2 == 1 and n <= 192,
    "f64_odd_four_accumulators": lambda n: n % 2 == 1 and n > 192,
    "f64_vec2_tail_only": lambda n: n % 2 == 0 and n // 2 <= 64,
    "f64_vec2_loop_and_tail": lambda n: n % 2 == 0 and 64 < n // 2 <= 128,
    "f64_vec2_several_trips": lambda n: n % 2 == 0 and n // 2 > 128,
}

Case = collections.namedtuple(
    "Case", "id src kind smoother opts nranks cls_rank cls32 cls64 levels one_block slow")


def case(id, src, kind, smoother, opts=None, nranks=1, cls_rank=0, cls32=None, cls64=None,
         levels=None, one_block=False, slow=False):
    return Case(id, src, kind, smoother, dict(opts or {}), nranks, cls_rank, cls32, cls64, levels,
                one_block, slow)


CYL0 = ("cfg", "cylinder_config.cfg", 0)
CYL2 = ("cfg", "cylinder_config.cfg", 2)
PORE1 = ("cfg", os.path.join("pore_pnp", "pore.cfg"), 1)


def fan(mesh_id, variant="mixed"):
    return ("fan", mesh_id, variant)


S1P0 = dict(coarse_sweeps=1, level0_presmooth=0)
# A. the default cycle: multicolour SSOR and ILU(0) on level 0
PART_A = [
    case("cyl0-pnp-ssor", CYL0, "pnp", "ssor", cls32="f32_one_trip_padded",
         cls64="f64_vec2_tail_only", levels=2),
    case("cyl0-pb-ssor", CYL0, "pb", "ssor", cls32="f32_one_trip_padded",
         cls64="f64_vec2_tail_only", levels=2),
    case("cyl0-pnp-ssor-s1p0", CYL0, "pnp", "ssor", S1P0, levels=2),
    case("cyl0-pb-ssor-s1p0", CYL0, "pb", "ssor", S1P0, levels=2),
    case("cyl0-pnp_ie-ilu0", CYL0, "pnp_ie", "ilu0", levels=2),
    case("cyl0-pb-ilu0", CYL0, "pb", "ilu0", levels=2),
    case("cyl0-pnp-ilu0-bf16", CYL0, "pnp", "ilu0_default", levels=2),
    case("cyl2-pnp-ssor", CYL2, "pnp", "ssor", cls32="f32_ragged_trips",
         cls64="f64_odd_four_accumulators", levels=2),
    case("cyl2-pb-ssor", CYL2, "pb", "ssor", cls32="f32_ragged_trips",
         cls64="f64_odd_four_accumulators", levels=2),
]
# B. the coarsest-solve kernels; Jacobi on level 0, so that the coarse part is all that is tested
PART_B = [
    case("one_triangle-pb", fan("one_triangle"), "pb", "jacobi", cls32="f32_one_trip_padded",
         cls64="f64_odd_tail_only", levels=2, one_block=True),
    case("pore1-pb-two-levels", PORE1, "pb", "jacobi", dict(max_levels=2),
         cls32="f32_scalar_gt_1000", cls64="f64_scalar_gt_1000", levels=2, slow=True),
    case("pore1-pb", PORE1, "pb", "jacobi", cls64="f64_vec2_tail_only", slow=True),
    case("chain86-pb", fan("diamond_chain_86"), "pb", "jacobi", cls64="f64_odd_tail_only",
         levels=2),
    case("cyl2-2ranks-pb", CYL2, "pb", "jacobi", nranks=2, cls64="f64_vec2_loop_and_tail",
         levels=2),
    case("cyl2-2ranks-pnp", CYL2, "pnp", "jacobi", nranks=2, cls64="f64_vec2_several_trips",
         levels=2),
]
# C. hierarchy shapes and row lengths
ONE_AGGREGATE = [
    case(f"{m}-{kind}-{sm}", fan(m), kind, sm, levels=2, one_block=True)
    for m in ("one_triangle", "split_triangle", "half_wheel_30", "pinwheel_13_1_12")
    for kind in ("pb", "diff_ie+", "pnp_ie") for sm in ("jacobi", "ssor")
    if (m, kind, sm) != ("one_triangle", "pb", "jacobi")]  # in part B
# coarse_sweeps 2 and 3: the buffer swap of the extra pre- and post-sweeps, an odd and an even count
DEEP = [
    case(f"{m}-{tag}-{kind}-{sm}{sw}", fan(m), kind, sm,
         dict(opts, coarse_sweeps=sw), levels=lv, one_block=ob)
    for m, tag, opts, lv, ob in (
        ("diamond_chain_86", "to1", dict(coarse_target=1), 6, True),
        ("diamond_chain_171", "to1", dict(coarse_target=1), 7, True),
        # stops at the level limit although the target is not met
        ("diamond_chain_171", "l3", dict(coarse_target=1, max_levels=3), 3, False))
    for kind in ("pb", "pnp_ie") for sm, sw in (("ssor", 2), ("jacobi", 3))]
RANKS = [
    case(f"{tag}-{n}ranks-{kind}", src, kind, "ssor", nranks=n)
    for tag, src in (("chain86", fan("diamond_chain_86")), ("cyl0", CYL0))
    for n in (2, 3) for kind in ("pb", "pnp_ie")]
TABLE = PART_A + PART_B + ONE_AGGREGATE + DEEP + RANKS
BY_ID = {c.id: c for c in TABLE}
assert len(BY_ID) == len(TABLE)


@functools.lru_cache(maxsize=None)
def problem(src):
    """(P.Mesh, P.Params, oracle problem, states, vertices whose row has break bits) of a case's
    mesh, as test_gpu_fan_walks.problem; shared and never modified"""
    if src[0] == "fan":
        return fan_problem(src[1], src[2])
    cfg = P.read_config(os.path.join(DATA, src[1]))
    mesh = P.Mesh.load(cfg.meshfile).refine(src[2])
    par = P.Params.from_config(cfg)
    s = cfg.system
    surf = [meshio.Surface(q.cb, q.cflux, q.cpot, q.pb, q.pflux, q.pconc, q.mb, q.mflux, q.mconc)
            for q in cfg.surfaces]
    orc = O.Problem(meshio.Mesh(mesh.xy, mesh.tri, mesh.bseg, mesh.bgroup), surf, l_b=s["l_b"],
                    c0=s["c0"], tau=s["tau"], cylindrical=s["cylindrical"])
    nv = mesh.nv
    rng = np.random.default_rng(1000 + nv)
    conc = lambda: 0.06 * rng.uniform(0.5, 1.5, nv)  # noqa: E731
    st = {"phi": rng.uniform(-1, 1, nv), "cp": conc(), "cm": conc(),
          "diff_phi": rng.uniform(-1, 1, nv), "old_phi": rng.uniform(-1, 1, nv), "old_cp": conc(),
          "old_cm": conc(), "c": conc()}
    return mesh, par, orc, st, np.zeros(0, dtype=np.int32)


def nfields(kind):
    return 3 if kind.startswith("pnp") else 1


def build_opts(c):
    """the amg_configure options of a case that shape the hierarchy"""
    return c.opts.get("coarse_target", 1024), c.opts.get("max_levels", 12)


def check_class(c, rank, n, f32):
    """the coarsest-solve path the case is named after runs in this process"""
    name = c.cls32 if f32 else c.cls64
    if name is not None and rank == c.cls_rank:
        assert CLASSES[name](n), (c.id, name, n)


def check_shape(c, H):
    if c.levels is not None:
        assert len(H["rows"]) == c.levels, (c.id, H["rows"])
    if c.one_block:
        assert H["rows"][-1] == 1, (c.id, H["rows"])


def reference_figures(c):
    """hierarchy rows, n and conditioning of every rank of a case, from the oracle's Jacobian"""
    mesh, par, orc, st, pinch = problem(c.src)
    op, x = set_kind(None, orc, st, c.kind)
    Jo = orc.jacobian(op, x)
    nf = nfields(c.kind)
    out = []
    for rank in range(c.nranks):
        lay = P.Layout(mesh, rank, c.nranks)
        H = R.hierarchy(lay, *build_opts(c))
        perm = R.local_perm(lay, nf, mesh.nv)
        A0 = Jo[perm][:, perm].tocsr()
        out.append((H, H["rows"][-1] * nf, R.conditioning(A0, nf, H["aggs"]), lay, pinch))
    return out


def _params():
    return [pytest.param(c.id, marks=pytest.mark.slow) if c.slow else c.id for c in TABLE]


@pytest.mark.parametrize("case_id", _params())
def test_case_table_holds_for_the_reference(case_id):
    c = BY_ID[case_id]
    for rank, (H, n, (cc, cb), lay, pinch) in enumerate(reference_figures(c)):
        print(f"{c.id} rank {rank}: rows {H['rows']} blocks {H['blocks'][1:]} n {n} "
              f"cond(coarsest) {cc:.2e} cond(blocks) {cb:.2e}")
        assert H["rows"][-1] * nfields(c.kind) <= R.MAX_DENSE
        assert cc <= COND_CAP and cb <= COND_CAP
        check_class(c, rank, n, True)
        check_class(c, rank, n, False)
        if c.nranks == 1:
            check_shape(c, H)


def test_pinch_rows_sit_inside_aggregates():
    """the chains' pinch vertices (rows with break bits) are members of aggregates of several rows"""
    for m in ("diamond_chain_86", "diamond_chain_171"):
        mesh, _, _, _, pinch = problem(fan(m))
        lay = P.Layout(mesh)
        agg = np.full(mesh.nv, -1)
        agg[lay.l2g[:lay.n_owned]] = R.hierarchy(lay, 1, 12)["aggs"][0]
        assert pinch.size and np.any(np.bincount(agg)[agg[pinch]] > 1)


def test_half_wheel_is_one_aggregate_of_31_rows():
    mesh = problem(fan("half_wheel_30"))[0]
    H = R.hierarchy(P.Layout(mesh))
    assert H["rows"] == [31, 1] and H["blocks"][1] == 1


def test_aggregate_passes():
    """a path 0 .. 6 and a vertex without neighbours: root 0 takes 1; 2 is blocked (1 is taken); 3
    takes 2 and 4; 5 is blocked; 6 takes 5; 7 is a root of its own.  A path of three: 2 is blocked
    in pass 1 and joins its neighbour's aggregate in pass 2."""
    nbr = [[1], [0, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5], []]
    agg, na = R.aggregate(8, nbr)
    assert na == 4 and list(agg) == [0, 0, 1, 1, 1, 2, 2, 3]
    agg, na = R.aggregate(3, [[1], [0, 2], [1]])
    assert na == 1 and list(agg) == [0, 0, 0]


# ---- the sweeps -----------------------------------------------------------------------------------
def golden(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    mesh = P.Mesh(z["xy"], z["tri"], z["bseg"], z["bgroup"])
    surfs = [meshio.Surface(int(s[0]), s[1], s[2], int(s[3]), s[4], s[5], int(s[6]), s[7], s[8])
             for s in z["surfaces"]]
    l_b, c0, tau, cyl, pi = z["params"]
    orc = O.Problem(meshio.Mesh(mesh.xy, mesh.tri, mesh.bseg, mesh.bgroup), surfs, l_b=l_b, c0=c0,
                    tau=tau, cylindrical=int(cyl), pi=pi)
    return z, mesh, orc


def sweep_systems():
    """(tag, Jacobian, layout, fields) of the systems the two forms of the sweep are compared on"""
    z, mesh, orc = golden("cylinder_k0")
    for kind, ko, nf in (("pnp", O.OP_PNP, 3), ("pb", O.OP_PB, 1)):
        op = orc.operator(ko, flux=orc.flux(), mask=orc.mask(nf))
        yield f"cylinder_k0/{kind}", orc.jacobian(op, z[kind + "_x"]), P.Layout(mesh), nf
    for m in ("pinwheel_13_1_12", "diamond_chain_86"):
        for variant in ("free", "mixed"):
            mesh, _, orc, st, _ = fan_problem(m, variant)
            for kind in ("pnp", "pb"):
                op, x = set_kind(None, orc, st, kind)
                yield f"{m}/{variant}/{kind}", orc.jacobian(op, x), P.Layout(mesh), nfields(kind)


def test_the_two_forms_of_the_multicolour_sweep_agree():
    for tag, J, lay, nf in sweep_systems():
        d = np.random.default_rng(3).standard_normal(J.shape[0])
        a = R.multicolour_ssor(J, lay, nf, d)
        b = R.multicolour_ssor(J, lay, nf, d, oracle=True)
        err = np.max(np.abs(a - b)) / np.max(np.abs(a))
        print(f"{tag}: triangular solves against the oracle's SeqSSOR {err:.2e}")
        assert err <= 1e-13, tag


def test_sweep_equals_the_dense_formula_without_colour_conflicts():
    seen = 0
    for tag, J, lay, nf in sweep_systems():
        if lay.color_conflicts:
            continue
        seen += 1
        Ap, perm = R.colour_masked(J, lay, nf)
        A = J.toarray()[np.ix_(perm, perm)]
        assert np.array_equal(Ap.toarray(), A)  # nothing to mask
        d = np.random.default_rng(4).standard_normal(J.shape[0])
        D = np.diag(np.diag(A))
        ref = np.linalg.solve(np.triu(A), D @ np.linalg.solve(np.tril(A), d[perm]))
        v = R.multicolour_ssor(J, lay, nf, d)[perm]
        assert np.max(np.abs(v - ref)) <= 1e-12 * np.max(np.abs(ref)), tag
    assert seen >= 2


def test_colour_mask_drops_exactly_the_same_colour_couplings():
    """a layout with conflicts: the masked matrix differs from the permuted one exactly in the
    couplings of two different rows of one colour (if no committed or generated mesh has a
    conflict, the mask is checked on an artificial colouring)"""
    tag, J, lay, nf = next(s for s in sweep_systems() if s[0].endswith("/pnp"))
    lay.rowcolor = lay.rowcolor.copy()
    lay.rowcolor[:lay.n_owned] = np.arange(lay.n_owned) % 2  # conflicts for certain
    Ap, perm = R.colour_masked(J, lay, nf)
    A = J.toarray()[np.ix_(perm, perm)]
    row = np.arange(A.shape[0]) // nf
    same = (row[:, None] % 2 == row[None, :] % 2) & (row[:, None] != row[None, :])
    assert np.any(A[same] != 0)
    assert np.array_equal(Ap.toarray(), np.where(same, 0.0, A))


def test_ilu0_of_a_full_pattern_is_lu():
    """ilu0_dense on the full pattern is the LU factorisation without pivoting"""
    rng = np.random.default_rng(6)
    A = rng.standard_normal((12, 12)) + 12 * np.eye(12)
    Fm = R.ilu0_dense(A, np.ones_like(A, dtype=bool))
    assert np.allclose((np.tril(Fm, -1) + np.eye(12)) @ np.triu(Fm), A, rtol=0, atol=1e-12)


# ---- the cycle ------------------------------------------------------------------------------------
def frozen_vcycle(A0, nf, aggs, omega, d, sweeps=2, pre0=True, f32=True):
    """numpy_vcycle as tests/test_gpu_amg.py had it before the level-0 smoother became an argument:
    the yardstick of test_generalised_cycle_reproduces_the_jacobi_cycle, never changed"""
    As, Ps = [A0], []
    for agg in aggs:
        n = As[-1].shape[0] // nf
        Pv = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, int(agg.max()) + 1))
        Pm = sp.kron(Pv, sp.identity(nf), format="csr")
        Ps.append(Pm)
        As.append((Pm.T @ As[-1] @ Pm).tocsr())
    K = len(aggs)
    Ad = As
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
    diag0 = A0.diagonal()
    x0 = d / diag0 if pre0 else np.zeros_like(d)
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
        e = np.linalg.inv(Ad[K].toarray()).astype(np.float32).astype(np.float64) @ b[K]
    else:
        e = np.linalg.solve(Ad[K].toarray(), b[K])
    for k in range(K - 1, 0, -1):
        xc = x[k] + Ps[k] @ e
        e = xc + omega * bj(As[k], Dis[k], b[k] - As[k] @ xc)
        for _ in range(sweeps - 1):
            e = e + omega * bj(As[k], Dis[k], b[k] - As[k] @ e)
    y = x0 + Ps[0] @ e
    return y + (d - A0 @ y) / diag0


def cycle_system(case_id):
    c = BY_ID[case_id]
    mesh, _, orc, st, _ = problem(c.src)
    op, x = set_kind(None, orc, st, c.kind)
    nf = nfields(c.kind)
    lay = P.Layout(mesh)
    perm = R.local_perm(lay, nf, mesh.nv)
    A0 = orc.jacobian(op, x)[perm][:, perm].tocsr()
    return A0, nf, lay, R.hierarchy(lay, *build_opts(c))["aggs"]


@pytest.mark.parametrize("case_id", ["diamond_chain_171-to1-pnp_ie-jacobi3",
                                     "diamond_chain_86-to1-pb-ssor2", "cyl0-pnp-ssor"])
def test_generalised_cycle_reproduces_the_jacobi_cycle(case_id):
    A0, nf, _, aggs = cycle_system(case_id)
    d = np.random.default_rng(8).standard_normal(A0.shape[0])
    for sweeps, pre0, f32 in ((1, True, True), (2, False, True), (3, True, False),
                              (2, True, False)):
        new = R.numpy_vcycle(A0, nf, aggs, 0.8, d, sweeps, pre0, f32)
        old = frozen_vcycle(A0, nf, aggs, 0.8, d, sweeps, pre0, f32)
        assert np.array_equal(new, old), (case_id, sweeps, pre0, f32)


@pytest.mark.parametrize("case_id", ["cyl0-pnp-ssor", "half_wheel_30-pnp_ie-ssor",
                                     "chain86-pb"])
def test_one_coarse_level_is_the_two_grid_closed_form(case_id):
    """one coarse level, exact coarsest solve, smooth0 = M^-1: x0 + P Ac^-1 P^T (d - A x0), then
    the post-smoothing step, written densely"""
    A0, nf, lay, aggs = cycle_system(case_id)
    assert len(aggs) == 1
    A = A0.toarray()
    n = A.shape[0]
    Ap = R.mask_same_colour(A0, lay, nf)
    Minv = np.column_stack([R.ssor_sweep(Ap, e) for e in np.eye(n)])
    Pm = np.zeros((n, (int(aggs[0].max()) + 1) * nf))
    for i in range(n):
        Pm[i, aggs[0][i // nf] * nf + i % nf] = 1.0
    d = np.random.default_rng(9).standard_normal(n)
    for pre0 in (True, False):
        x0 = Minv @ d if pre0 else np.zeros(n)
        y = x0 + Pm @ np.linalg.solve(Pm.T @ A @ Pm, Pm.T @ (d - A @ x0))
        ref = y + Minv @ (d - A @ y)
        v = R.numpy_vcycle(A0, nf, aggs, 0.8, d, 2, pre0, False, smooth0=lambda r: Minv @ r)
        assert np.max(np.abs(v - ref)) <= 1e-12 * np.max(np.abs(ref)), (case_id, pre0)
