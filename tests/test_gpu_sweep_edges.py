"""One application of the multicolour ILU(0), of the multicolour SSOR and of Jacobi on block-edge,
conflict and P_k layouts, against the restatements of tests/amg_ref.py (-m gpu).

A wrong sweep does not fail a solve, it costs iterations; what sees it is one application
v = M^-1 d compared entry by entry with a reference.  tests/test_gpu.py does that for the ILU(0) on
two meshes whose colours have 62 .. 88 rows, at most 9 slots and no same-colour coupling, so every
colour launch there is one partial 256-row block.  The cases of tests/sweep_cases.py (held to
P.Layout and to the reference alone by tests/test_sweep_ref_host.py) reach colours of 255 .. 513
rows (blk0[c] != c, lsx_ptr[blk0 + bl]), same-colour couplings (dropped() / same_color() in the
factorisations, no slot in the split storage), and P2 / P3 node layouts: rows of 61 and 63 slots,
the fused factorisation with its own rows in scratch, staging lists past ILU_SU * 256 entries.

Every case, every kind, every rank: the context's info() carries the host figures (color_conflicts,
max_slots, lsx_entries), J is the one-rank context's exported Jacobian, d is seeded, and
  * ILU(0), PNP_OPT_ILU_F32 = 0, 1, 2, 3: max|v - v_ref| <= bound max|v_ref| on the owned unknowns,
    v_ref the restatement that rounds what the kernel rounds (amg_ref.ilu0_mode / ilu0_stored /
    ilu0_sweep), from the factorisation in the kernels' form (ilu0_dense_recip).  D is the distance
    to the same restatement from the dividing form (ilu0_dense): what last-bit differences of the
    fp64 factors cost after the storage rounding.  bound = max(floor, 8 D), floor 1e-10 for fp64
    and bfloat16 storage and 1e-7 for float storage and the single-precision intermediate (a float
    that rounds to its neighbour costs 6e-8), never above 1e-10 / 2e-5 / 2e-2 / 2e-2.  Scalar
    systems run modes 2 and 3 as mode 1: bitwise mode 1's result, mode 1's bound;
  * SSOR against amg_ref.multicolour_ssor and Jacobi against amg_ref.jacobi_apply at 1e-10.
The sweep variants (PNP_ILU_LDS=0, PNP_ILU_LDS_B=8 / 3, PNP_SPLIT_SORT=0; each knob is read once per
process, so one child each) are bitwise this process's results on sweep_cases.VARIANT_IDS.
PNP_SWEEP=2x4 sums a row's slots in two lanes and adds the two partial sums, another order of
additions, so it is not bitwise equal by construction: it is held to the reference at the bounds
above.  One fused BiCGSTAB + ILU(0) solve per block-edge layout (launch_update_fwd0 with c0_end =
255, 513, 512, 257) converges, leaves a true residual of at most 1e-9 |rhs| on the exported
Jacobian, and agrees with the PNP_FUSE=0 child's solution to 1e-8.

Measured on an MI355X (profiles/sweep_edges/figures.jsonl holds one SWEEP-FIG record per case, kind
and rank: distance, bound and D of every mode).  Largest distance / max|v_ref| per family, the
bound in the heading; bfloat16 columns over the block systems, which alone store it:
    family               fp64     float    bf16     bf16 + y32  SSOR     Jacobi   largest D
                         (1e-10)  (1e-7)   (1e-10)  (1e-7)      (1e-10)  (1e-10)
    P1 long rows / tiny  1.6e-16  1.8e-16  1.8e-16  1.8e-16     1.8e-16  0        0
    P1 block-edge        4.2e-16  3.5e-16  2.6e-16  2.4e-16     3.7e-16  0        2.2e-16
    conflict (P1, P2)    3.2e-16  2.4e-16  3.2e-16  1.6e-16     3.9e-16  0        3.2e-16
    P2                   1.9e-16  1.9e-16  -        -           3.8e-16  0        4.7e-16
    P3                   6.1e-14  5.1e-14  -        -           7.6e-16  0        7.8e-14
    2 ranks              3.3e-16  2.4e-16  2.5e-16  1.6e-16     3.9e-16  0        1.7e-16
    PNP_SWEEP=2x4 child  6.1e-14  5.1e-14  3.6e-16  2.4e-16     5.1e-16  -        7.8e-14
No bound had to use 8 D: the largest D is 7.8e-14 (P3 wheel_on_chain(10, 100), diff_ie, whose
smallest pivot is 4.6e-5), far under every floor.  No float and no bfloat16 value rounded to its
neighbour between kernel and restatement, so a miss is a wrong kernel, not rounding.  The solves
took 1 .. 8 iterations and left true residuals of 7.5e-15 .. 2.3e-11 |rhs|, the same with and
without the fused colour-0 step (profiles/sweep_edges/solves.txt).

What the cases see, each tried on a scratch build that changed values only (never committed):
  * dropped() removed from k_ilu0_factor_fused's update step: wheel3_chain127-P2 alone fails (ILU(0)
    off by 1.8e-1 pb, 2.9e-2 diff_ie, the figures test_sweep_ref_host.forgetful_update predicts),
    and the PNP_SWEEP=2x4 test through the same case.  The P1 conflict cases (at most 8 slots,
    KMAX = 10) cannot see it, and a first run without the P2 case passed whole: with a row's own
    blocks in LDS its same-colour blocks never reach the scratch that the update reads, so the
    line guards only the KMAX = 0 form (rows past 16 slots; pore_pnp at P3).
  * the long-list staging loop of k_ilu0_solve_lds starting one block late: wheel10_chain100-P3 and
    chain139-P3 fail, chain64-P3 (897 entries) passes; the four bitwise variants fail too (the
    unstaged LDS entries differ from process to process).
  * blk0[c + 1] = blk0[c] + 1 in launch_ilu0_apply: exactly the layouts with a colour over 256
    rows fail (chain172, chain341, chain342, wheel5_chain340, wheel7_chain340, chain140-P2,
    chain139-P3, wheel5_chain340-2ranks, and three of the four solves); chain170 (255) and
    chain128-P2 (256) pass.
"""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as R
import pk_util as U
import pnp_amd as P
import sweep_cases as SC
from test_gpu_fan_walks import set_kind
from test_gpu_pk import KINDS as PK_OPS
from test_gpu_pk_edges import run_ranks
from test_sweep_ref_host import pk_operator, relative

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = (0, 1, 2, 3)
FLOOR = {0: 1e-10, 1: 1e-7, 2: 1e-10, 3: 1e-7}
CAP = {0: 1e-10, 1: 2e-5, 2: 2e-2, 3: 2e-2}  # mode 3 takes mode 2's
KNOBS = ("PNP_ILU_LDS", "PNP_ILU_LDS_B", "PNP_SWEEP", "PNP_SWEEP_NT", "PNP_SPLIT_SORT", "PNP_FUSE",
         "PNP_ILU_F32", "PNP_ILU_FLOW")


def effective(mode, nf):
    """the mode a system of nf fields runs PNP_OPT_ILU_F32 = mode as"""
    return 1 if nf == 1 and mode >= 2 else mode


# ---- the library's side --------------------------------------------------------------------------
def set_operator(ctx, case_id, kind, perm=None):
    """the operator of (case, kind) on ctx (None: nowhere); returns the state in ctx's numbering"""
    c = SC.BY_ID[case_id]
    if c.degree == 1:
        _, _, orc, st = SC.p1_problem(case_id)
        return set_kind(ctx, orc, st, kind)[1]
    _, _, orc, S = SC.pk_problem(case_id)
    _, x, kw = pk_operator(orc, S, kind, c.degree)
    pk = {q: (v[perm] if isinstance(v, np.ndarray) else v) for q, v in kw.items()}
    if kind.startswith("diff"):
        pk["field"] = 2
    if ctx is not None:
        ctx.set_operator(PK_OPS[kind][0], **pk)
    return x[perm]


def applications(ctx, case_id, kind, perm, export):
    """what a (case, kind) asks of one context (also run on the rank threads: no assertion here)"""
    x = set_operator(ctx, case_id, kind, perm)
    d = SC.rhs(x.size)
    out = {"J": ctx.jacobian(x, export=export), "d": d}
    for mode in MODES:
        ctx.set_option(P.OPT_ILU_F32, mode)
        out[f"ilu{mode}"] = ctx.prec_apply(d, P.PREC_ILU0)
    out["ssor"] = ctx.prec_apply(d, P.PREC_SSOR)
    out["jacobi"] = ctx.prec_apply(d, P.PREC_JACOBI)
    out["info"] = ctx.info()
    return out


def node_perm(ctx, case_id):
    """product node i = oracle node perm[i] (P1: None, the vertices are the mesh's)"""
    if SC.BY_ID[case_id].degree == 1:
        return None
    S = SC.pk_problem(case_id)[3]
    xy, en = ctx.space()
    assert xy.shape[0] == S.nn == ctx.nn
    perm = U.match_nodes(xy, S.xy)
    np.testing.assert_array_equal(perm[en], S.enode)
    return perm


@functools.lru_cache(maxsize=None)
def gpu_case(case_id):
    """{kind: (one-rank results, [results of every rank])}: computed once, shared, never modified"""
    c = SC.BY_ID[case_id]
    mesh, par = (SC.p1_problem if c.degree == 1 else SC.pk_problem)(case_id)[:2]
    res = {}
    ctx = P.Context(mesh, par, device=0, degree=c.degree)
    try:
        perm = node_perm(ctx, case_id)
        for kind in c.kinds:
            res[kind] = applications(ctx, case_id, kind, perm, True)
    finally:
        ctx.close()
    if c.nranks == 1:
        return {kind: (one, [one]) for kind, one in res.items()}
    out = {}
    for kind in c.kinds:
        outs, errs = run_ranks(c.nranks, mesh, par, c.degree,
                               lambda rc: applications(rc, case_id, kind, perm, False))
        assert not errs, errs
        out[kind] = (res[kind], outs)
    return out


# ---- the reference's side ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(case_id, kind, rank):
    """the restated applications of one rank from the one-rank exported Jacobian: {"perm", "ssor",
    "jacobi", mode: (v_ref, D)}; the two fp64 factorisations are done once"""
    c = SC.BY_ID[case_id]
    one = gpu_case(case_id)[kind][0]
    J, d = one["J"].tocsr(), one["d"]
    nf = SC.nfields(kind)
    lay = P.Layout(SC.mesh_of(case_id), rank, c.nranks, degree=c.degree)
    Ap, M, perm = R.ilu0_system(J, lay, nf, R.PATS[kind])
    fp64 = [R.ilu0_fp64(Ap, M, recip) for recip in (True, False)]
    last = np.repeat(lay.rowcolor[:lay.n_owned] != lay.ncolors - 1, nf)
    ref = {"perm": perm, "lay": SC.layout_figures(lay)}
    for mode in sorted({effective(m, nf) for m in MODES}):
        store, y32 = R.ilu0_mode(mode, nf)
        va, vb = (R.ilu0_sweep(*R.ilu0_stored(*f, store), d[perm], nf, last if y32 else None)
                  for f in fp64)
        ref[mode] = (va, relative(vb, va))
    ref["ssor"] = R.multicolour_ssor(J, lay, nf, d)[perm]
    ref["jacobi"] = R.jacobi_apply(J, lay, nf, R.PATS[kind], d)[perm]
    return ref


def bound_of(mode, D):
    return min(CAP[mode], max(FLOOR[mode], 8.0 * D))


def figures(case_id, kind, rank, out, tag=""):
    """one rank's applications against the reference: (the SWEEP-FIG record, the misses)"""
    c = SC.BY_ID[case_id]
    nf = SC.nfields(kind)
    ref = reference(case_id, kind, rank)
    perm = ref["perm"]
    fig = dict(id=c.id, family=c.family, kind=kind, rank=rank, n=int(perm.size), variant=tag)
    bad = []
    for mode in MODES:
        eff = effective(mode, nf)
        vref, D = ref[eff]
        err = relative(out[f"ilu{mode}"][perm], vref)
        b = bound_of(eff, D)
        fig[f"ilu{mode}"] = dict(err=err, bound=b, D=D)
        if not err <= b:
            bad.append(f"{c.id}/{kind} rank {rank} {tag}: ILU(0) mode {mode} {err:.3e} > {b:.1e}")
        if eff != mode and not np.array_equal(out[f"ilu{mode}"], out["ilu1"]):
            bad.append(f"{c.id}/{kind} rank {rank} {tag}: scalar mode {mode} is not mode 1 bitwise")
    for name in ("ssor", "jacobi"):
        err = relative(out[name][perm], ref[name])
        fig[name] = err
        if not err <= 1e-10:
            bad.append(f"{c.id}/{kind} rank {rank} {tag}: {name} {err:.3e} > 1e-10")
    return fig, bad


def info_misses(case_id, kind, rank, info):
    """the context ran the layout the host test measured"""
    lay = reference(case_id, kind, rank)["lay"]
    want = dict(SC.BY_ID[case_id].expect[rank])
    bad = []
    for key, got in (("conflicts", info["color_conflicts"]), ("max_slots", info["max_slots"]),
                     ("rows", info["nv_owned"]), ("lsx_entries", info["lsx_entries"])):
        if got != lay[key] or got != want.get(key, got):
            bad.append(f"{case_id}/{kind} rank {rank}: info {key} {got}, layout {lay[key]}")
    if not info["lsx_entries"] > 0:
        bad.append(f"{case_id}/{kind} rank {rank}: no staging lists")
    return bad


@pytest.mark.parametrize("case_id", SC.IDS)
def test_applications_match_the_reference(case_id):
    c = SC.BY_ID[case_id]
    bad = []
    for kind in c.kinds:
        for rank, out in enumerate(gpu_case(case_id)[kind][1]):
            bad += info_misses(case_id, kind, rank, out["info"])
            fig, miss = figures(case_id, kind, rank, out)
            print("SWEEP-FIG " + json.dumps(fig))
            bad += miss
            nf = SC.nfields(kind)
            if nf == 3:  # the storages do differ: the modes are not one kernel run four times
                assert not np.array_equal(out["ilu0"], out["ilu1"])
                assert not np.array_equal(out["ilu1"], out["ilu2"])
                if c.expect[rank]["rows"] > 64:
                    assert not np.array_equal(out["ilu2"], out["ilu3"])
    assert not bad, "\n".join(bad)


# ---- the sweep variants, one child process each --------------------------------------------------
CHILD = r"""
import sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_sweep_edges as T
T.child_main(WHAT, PATH)
"""
VECTORS = tuple(f"ilu{m}" for m in MODES) + ("ssor",)


def sweep_outputs():
    """{"case/kind/name": vector} over sweep_cases.VARIANT_IDS, and the Jacobians' values"""
    out = {}
    for case_id in SC.VARIANT_IDS:
        for kind, (one, _) in gpu_case(case_id).items():
            for name in VECTORS:
                out[f"{case_id}/{kind}/{name}"] = one[name]
            out[f"{case_id}/{kind}/J"] = one["J"].tocsr().data
    return out


def solve_outputs():
    """one BiCGSTAB + ILU(0) solve per (case, kind) of sweep_cases.SOLVE_CASES with the default
    factor storage: {"case/kind/z", "/J" (values), "/Jcol", "/Jptr", "/res" (converged,
    iterations)}"""
    out = {}
    for case_id, kinds, _ in SC.SOLVE_CASES:
        c = SC.BY_ID[case_id]
        mesh, par = (SC.p1_problem if c.degree == 1 else SC.pk_problem)(case_id)[:2]
        ctx = P.Context(mesh, par, device=0, degree=c.degree)
        try:
            perm = node_perm(ctx, case_id)
            for kind in kinds:
                x = set_operator(ctx, case_id, kind, perm)
                J = ctx.jacobian(x).tocsr()
                z, res = ctx.linear_solve(SC.rhs(x.size, 29), prec=P.PREC_ILU0, reduction=1e-10,
                                          maxit=2000)
                key = f"{case_id}/{kind}"
                out[key + "/z"], out[key + "/J"] = z, J.data
                out[key + "/Jcol"], out[key + "/Jptr"] = J.indices, J.indptr
                out[key + "/res"] = np.array([res["converged"], res["iterations"]])
        finally:
            ctx.close()
    return out


def child_main(what, path):
    np.savez(path, **(sweep_outputs() if what == "sweeps" else solve_outputs()))


@functools.lru_cache(maxsize=None)
def run_child(what, knob, value):
    """the outputs of a child process with one PNP_* knob set; only the project's own knobs"""
    env = {q: v for q, v in os.environ.items() if q not in KNOBS}
    env[knob] = value
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        code = CHILD.replace("HERE", repr(HERE)).replace("WHAT", repr(what)).replace(
            "PATH", repr(path))
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                           timeout=300, cwd=HERE)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        with np.load(path) as z:
            return {q: z[q] for q in z.files}


@pytest.mark.parametrize("knob,value", [("PNP_ILU_LDS", "0"), ("PNP_ILU_LDS_B", "8"),
                                        ("PNP_ILU_LDS_B", "3"), ("PNP_SPLIT_SORT", "0")])
def test_variant_is_bitwise_the_default(knob, value):
    """the direct-gather sweeps, the slot batches and the identity lane order keep every row's slot
    order and arithmetic: every ILU(0) mode and the SSOR sweep bit for bit, on colours of several
    blocks, same-colour couplings, 61 / 63-slot rows and staging lists past 1,024 entries"""
    mine, theirs = sweep_outputs(), run_child("sweeps", knob, value)
    assert set(mine) == set(theirs) and len(mine) >= 6 * len(SC.VARIANT_IDS)
    diff = sorted(q for q in mine if not np.array_equal(mine[q], theirs[q]))
    assert not diff, diff


def test_two_lane_sweep_matches_the_reference():
    """PNP_SWEEP=2x4: two lanes per row, each summing every second batch of four slots, the partial
    sums added at the end -- not this process's order of additions, so not bitwise its results
    (asserted for the long rows: were it bitwise, the knob would not have been read).  Held to the
    reference at the bounds of test_applications_match_the_reference.  Same Jacobian, bit for
    bit."""
    mine, theirs = sweep_outputs(), run_child("sweeps", "PNP_SWEEP", "2x4")
    bad, differs = [], 0
    for case_id in SC.VARIANT_IDS:
        for kind in SC.BY_ID[case_id].kinds:
            key = f"{case_id}/{kind}/"
            assert np.array_equal(mine[key + "J"], theirs[key + "J"])
            out = {name: theirs[key + name] for name in VECTORS}
            out["jacobi"] = gpu_case(case_id)[kind][0]["jacobi"]
            fig, miss = figures(case_id, kind, 0, out, "PNP_SWEEP=2x4")
            print("SWEEP-FIG " + json.dumps(fig))
            bad += miss
            differs += sum(not np.array_equal(mine[key + name], theirs[key + name])
                           for name in VECTORS)
    assert not bad, "\n".join(bad)
    assert differs > 0


@pytest.mark.parametrize("case_id,kinds,c0_end", SC.SOLVE_CASES)
def test_fused_solve_on_block_edge_layouts(case_id, kinds, c0_end):
    """BiCGSTAB + ILU(0), whose vector updates also run colour 0 of the forward sweep
    (launch_update_fwd0) over c0_end rows: one block less a row, two blocks and a row, two full
    blocks, a block and a row"""
    c = SC.BY_ID[case_id]
    lay = P.Layout(SC.mesh_of(case_id), degree=c.degree)
    assert int(lay.color_ptr[1]) == c0_end and lay.ncolors > 2 and lay.n_owned >= 64
    fused, apart = solve_outputs_cached(), run_child("solves", "PNP_FUSE", "0")
    for kind in kinds:
        key = f"{case_id}/{kind}"
        n = fused[key + "/Jptr"].size - 1
        J = sp.csr_matrix((fused[key + "/J"], fused[key + "/Jcol"], fused[key + "/Jptr"]),
                          shape=(n, n))
        assert np.array_equal(fused[key + "/J"], apart[key + "/J"])
        rhs = SC.rhs(n, 29)
        for name, o in (("fused", fused), ("PNP_FUSE=0", apart)):
            z, (conv, its) = o[key + "/z"], o[key + "/res"]
            rel = float(np.linalg.norm(J @ z - rhs) / np.linalg.norm(rhs))
            print(f"SWEEP-SOLVE {key} {name}: {its} iterations, |Jz - rhs| / |rhs| {rel:.2e}")
            assert conv == 1 and rel <= 1e-9, (key, name, conv, rel)
        za, zb = fused[key + "/z"], apart[key + "/z"]
        assert np.max(np.abs(za - zb)) <= 1e-8 * np.max(np.abs(za)), key


@functools.lru_cache(maxsize=None)
def solve_outputs_cached():
    return solve_outputs()
