"""One V-cycle of PNP_PREC_AMG with every level-0 smoother and at edge hierarchy sizes, against the
numpy restatement of tests/amg_ref.py (-m gpu).

A wrong preconditioner does not fail a solve, it costs iterations; what can see it is one
application v = B d compared entry by entry.  tests/test_gpu_amg.py does that for the Jacobi
smoother on one mesh with a coarsest system of at most 48 unknowns.  The cases here (the table of
tests/test_amg_ref_host.py, which holds it to the reference alone on the CPU) run what that leaves
out: the default cycle (multicolour SSOR, and ILU(0) with its fused last sweep), the coarsest GEMV
kernels past their first loop trip, hierarchies of one coarse level and down to one block,
aggregates and coarse rows longer than the 8 lanes that share a row, the rank-local cycle on 2 and
3 ranks, P_k contexts, and the coarse values after a second assembly and a reconfiguration.

Every case: assemble, amg_configure, v = prec_apply(d, PREC_AMG); then
  * the hierarchy is the restated one (amg_ref.hierarchy on the rank's P.Layout): aggregates equal,
    rows equal, blocks = distinct (aggregate, aggregate) pairs; level-0 aggregates are -1 exactly at
    the vertices the rank does not own;
  * the path the case is named after ran (test_amg_ref_host.CLASSES on n = coarsest rows x fields);
  * cond_2 of the coarsest Galerkin matrix and of every inverted coarse diagonal block, from the
    exported Jacobian, is at most 1e6;
  * max|v - v_ref| <= bound max|v_ref| on the rank's owned unknowns, v_ref built from the exported
    Jacobian of a one-rank context (its owned x owned block).
As a by-product the bare sweep prec_apply(d, PREC_SSOR) is held to amg_ref.multicolour_ssor at
1e-10 in every P1 case.

Bounds.  fp64 (the PNP_AMG_F32=0 child, which runs the whole table once): 1e-10, the project's
number.  f32 (this process): the reference rounds what the kernels round, the bound of
tests/test_gpu_amg.py is 1e-7; it was set at n <= 48.  For larger n the bound is taken from the
reference alone: N is the distance between two restated cycles whose rounded inverses come from
inv(A) and inv(A.T).T (two fp64 inverses that differ by rounding only), and the bound is
max(1e-7, 8 N), the factor for rocSOLVER's pivot order against LAPACK's; never above 1e-5.

P_k: the node layout (row order, colours) is read on the host as the P1 one is, P.Layout(mesh, rank,
nranks, degree=k), so the SSOR cycle's level-0 sweep is amg_ref.multicolour_ssor on that layout
(tests/test_gpu_sweep_edges.py holds the bare P_k sweep to the same restatement); the aggregates are
held to the exported Jacobian's graph (a partition; blocks = distinct pairs), not to the restated
aggregation.  Only the bf16 ILU(0) case takes a sweep from the library, a second context's.

Measured on an MI355X (distance / max|v_ref|; N as above), part B and the large part A cases:
    case                   n      f32: N     distance   fp64: distance
    cyl0-pnp-ssor          90     3.5e-16    5.8e-16    4.2e-15
    cyl0-pb-ssor           30     3.1e-17    6.1e-17    6.1e-17
    cyl2-pnp-ssor          1263   1.6e-15    9.7e-16    4.1e-15
    cyl2-pb-ssor           421    5.7e-16    3.8e-16    8.5e-16
    one_triangle-pb        1      0          0          0
    pore1-pb-two-levels    1095   1.2e-16    1.2e-16    1.2e-16
    pore1-pb               110    1.2e-17    1.2e-16    2.5e-16
    chain86-pb             43     1.7e-16    8.6e-17    8.6e-17
    cyl2-2ranks-pb (r. 0)  220    7.0e-16    3.0e-16    9.0e-16
    cyl2-2ranks-pnp (r. 0) 660    3.1e-14    1.1e-15    4.0e-15
Over the whole table: largest distance 4.5e-15 (f32) and 5.8e-15 (fp64), largest N 3.1e-14, largest
distance of the bare SSOR sweep 3.8e-16.  So no case needed more than 1e-7: the rocSOLVER inverse
and numpy's round to the same floats almost everywhere, and a miss is a wrong kernel, not rounding.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amg_ref as R
import fan_meshes as F
import pnp_amd as P
from test_amg_ref_host import (BY_ID, COND_CAP, CYL0, PORE1, TABLE, build_opts, check_class,
                               check_shape, fan, nfields, problem)
from test_gpu_asm_const import second_state
from test_gpu_fan_walks import set_kind
from test_gpu_pk import args, bind
from test_gpu_pk_edges import check_space, problem as pk_problem, run_ranks

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = os.environ.get("PNP_AMG_F32", "1") != "0"
SMOOTHER = {"jacobi": P.PREC_JACOBI, "ssor": P.PREC_SSOR, "ilu0": P.PREC_ILU0,
            "ilu0_default": P.PREC_ILU0}
OMEGA = 0.8  # the default of amg_configure


def rhs(n):
    return np.random.default_rng(11).standard_normal(n)


def library_calls(ctx, c, x, d):
    """what a case asks of one context (also run on the rank threads: no assertion in here)"""
    _, _, orc, st, _ = problem(c.src)
    set_kind(ctx, orc, st, c.kind)
    if c.smoother == "ilu0":
        ctx.set_option(P.OPT_ILU_F32, 0)
    J = ctx.jacobian(x)
    ctx.amg_configure(smoother=SMOOTHER[c.smoother], **c.opts)
    v = ctx.prec_apply(d, P.PREC_AMG)
    info = ctx.amg_info()
    aggs = [ctx.amg_aggregates(k) for k in range(info["levels"] - 1)]
    return dict(J=J, v=v, info=info, aggs=aggs, ssor=ctx.prec_apply(d, P.PREC_SSOR))


def held_hierarchy(lay, nv, info, aggs, opts):
    """the library's hierarchy is the restated one; returns it"""
    H = R.hierarchy(lay, *opts)
    assert info["levels"] == len(H["rows"]) and info["rows"] == H["rows"], (info, H["rows"])
    assert info["blocks"][1:] == H["blocks"][1:], (info, H["blocks"])
    a0 = np.full(nv, -1)
    a0[lay.l2g[:lay.n_owned]] = H["aggs"][0]
    assert np.array_equal(aggs[0], a0)  # -1 exactly at the vertices this rank does not own
    for k in range(1, len(aggs)):
        assert np.array_equal(aggs[k], H["aggs"][k]), k
    return H


def cycle_figures(A0, nf, aggs, d, v, sweeps, pre0, smooth0):
    """(distance, bound, N) of v from the restated cycle in this process's precision"""
    kw = dict(sweeps=sweeps, pre0=pre0, f32=F32, smooth0=smooth0)
    vref = R.numpy_vcycle(A0, nf, aggs, OMEGA, d, **kw)
    scale = np.max(np.abs(vref))
    err = float(np.max(np.abs(v - vref)) / scale)
    if not F32:
        return err, 1e-10, 0.0
    v2 = R.numpy_vcycle(A0, nf, aggs, OMEGA, d, inv=lambda A: np.linalg.inv(A.T).T, **kw)
    N = float(np.max(np.abs(v2 - vref)) / scale)
    return err, min(max(1e-7, 8 * N), 1e-5), N


def compare(c, rank, out, J1, d, smooth_ctx=None):
    """one rank's results against the restatement; the figures"""
    mesh, _, _, _, pinch = problem(c.src)
    nv, nf = mesh.nv, nfields(c.kind)
    lay = P.Layout(mesh, rank, c.nranks)
    H = held_hierarchy(lay, nv, out["info"], out["aggs"], build_opts(c))
    n = H["rows"][-1] * nf
    check_class(c, rank, n, F32)
    if c.nranks == 1:
        check_shape(c, H)
        if pinch.size and len(H["rows"]) > 2:  # a pinch vertex inside an aggregate of several rows
            a0 = out["aggs"][0]
            assert np.any(np.bincount(a0)[a0[pinch]] > 1)
    else:
        assert 0 < lay.n_owned < nv and lay.n_ghost > 0
    perm = R.local_perm(lay, nf, nv)
    A0 = J1[perm][:, perm].tocsr()
    cc, cb = R.conditioning(A0, nf, H["aggs"])
    assert cc <= COND_CAP and cb <= COND_CAP, (c.id, cc, cb)
    Ap = R.mask_same_colour(A0, lay, nf)
    sref = R.ssor_sweep(Ap, d[perm])
    serr = float(np.max(np.abs(out["ssor"][perm] - sref)) / np.max(np.abs(sref)))
    if c.smoother == "jacobi":
        smooth0 = None
    elif c.smoother == "ssor":
        smooth0 = functools.partial(R.ssor_sweep, Ap)
    elif c.smoother == "ilu0":
        smooth0, p2 = R.ilu0_operator(J1, lay, nf, R.PATS[c.kind])
        assert np.array_equal(p2, perm) and A0.shape[0] <= 1000
    else:  # the default (reduced-precision) factors: another context's own ILU(0) application
        def smooth0(r):
            e = np.zeros(nf * nv)
            e[perm] = r
            return smooth_ctx.prec_apply(e, P.PREC_ILU0)[perm]
    err, bound, N = cycle_figures(A0, nf, H["aggs"], d[perm], out["v"][perm],
                                  c.opts.get("coarse_sweeps", 2),
                                  c.opts.get("level0_presmooth", -1) != 0, smooth0)
    fig = dict(id=c.id, rank=rank, f32=F32, rows=H["rows"], n=n, err=err, bound=bound, N=N,
               ssor=serr, cond=cc)
    print("AMG-FIG " + json.dumps(fig))
    return fig


def run_case(c):
    """the figures of every rank of a case; hierarchy, class and conditioning asserted on the way"""
    mesh, par, orc, st, _ = problem(c.src)
    _, x = set_kind(None, orc, st, c.kind)
    d = rhs(x.size)
    ctx = P.Context(mesh, par)
    try:
        one = library_calls(ctx, c, x, d)
        if c.nranks == 1:
            if c.smoother != "ilu0_default":
                return [compare(c, 0, one, one["J"], d)]
            c2 = P.Context(mesh, par)
            try:
                set_kind(c2, orc, st, c.kind)
                assert c2.get_option(P.OPT_ILU_F32) == ctx.get_option(P.OPT_ILU_F32) != 0
                c2.jacobian(x, export=False)
                return [compare(c, 0, one, one["J"], d, smooth_ctx=c2)]
            finally:
                c2.close()
    finally:
        ctx.close()
    outs, errs = run_ranks(c.nranks, mesh, par, 1, lambda rc: library_calls(rc, c, x, d))
    assert not errs, errs
    return [compare(c, r, outs[r], one["J"], d) for r in range(c.nranks)]


def misses(figs):
    bad = [f"{f['id']} rank {f['rank']} (n = {f['n']}): cycle {f['err']:.3e} > {f['bound']:.1e}"
           for f in figs if not f["err"] <= f["bound"]]
    bad += [f"{f['id']} rank {f['rank']}: bare SSOR sweep {f['ssor']:.3e} > 1e-10"
            for f in figs if not f["ssor"] <= 1e-10]
    return bad


@pytest.mark.parametrize("case_id", [c.id for c in TABLE])
def test_cycle_matches_restatement(case_id):
    figs = run_case(BY_ID[case_id])
    assert not misses(figs), "\n".join(misses(figs))


# ---- the fp64 values: the whole table once more in one child with PNP_AMG_F32=0 ------------------
CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_amg_edges as T
print("RESULT " + json.dumps(T.child_main()))
"""


def child_main():
    assert not F32
    figs, bad = [], []
    for c in TABLE:
        try:
            figs += run_case(c)
        except AssertionError as e:
            bad.append(f"{c.id}: {e!r}"[:500])
    return {"figs": figs, "bad": bad}


def test_fp64_values_child():
    """PNP_AMG_F32 is read once per process: every case of the table with fp64 coarse-level values
    and the fp64 coarsest GEMVs (k_coarse_apply<0> and <1>), each to 1e-10; the class assertions of
    the fp64 kernels are made in the child, where they run"""
    env = dict(os.environ, PNP_AMG_F32="0")
    p = subprocess.run([sys.executable, "-c", CHILD.replace("HERE", repr(HERE))], env=env,
                       capture_output=True, text=True, timeout=900, cwd=HERE)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for f in out["figs"]:
        print("AMG-FIG " + json.dumps(f))
    assert not out["bad"], "\n".join(out["bad"])
    assert {f["id"] for f in out["figs"]} == set(BY_ID)
    assert all(not f["f32"] and f["bound"] == 1e-10 for f in out["figs"])
    assert not misses(out["figs"]), "\n".join(misses(out["figs"]))


# ---- P_k contexts ------------------------------------------------------------------------------------
def graph_checks(J, info, aggs):
    """the aggregates partition every level, and blocks[k] is the number of distinct (aggregate,
    aggregate) pairs of the level below, from the exported Jacobian's pattern"""
    C = J.tocoo()  # stored zeros included
    r, c = C.row, C.col
    for k, a in enumerate(aggs):
        assert a.size == info["rows"][k] and a.min() == 0
        assert np.array_equal(np.unique(a), np.arange(info["rows"][k + 1]))
        pairs = np.unique(np.stack([a[r], a[c]], axis=1), axis=0)
        assert len(pairs) == info["blocks"][k + 1]
        r, c = pairs[:, 0], pairs[:, 1]


@pytest.mark.parametrize("smoother", ["jacobi", "ssor"])
@pytest.mark.parametrize("mesh_id,k,opts,levels", [
    ("wheel_20", 2, {}, 2),                              # the 61-slot hub row
    ("diamond_chain_64", 2, {}, 2),                      # 513 nodes
    ("diamond_chain_64", 2, dict(coarse_target=1, coarse_sweeps=3), None),
    ("wheel_10", 3, {}, 2)])
def test_pk_cycle(mesh_id, k, opts, levels, smoother):
    mesh, par, orc, S = pk_problem(mesh_id, k, "mixed")
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, mesh_id, k)
        assert ctx.info()["max_slots"] == F.pk_entry(mesh_id)[3][k][1]
        x, kw = args("pb", S.nn, 7)
        bind(ctx, orc, S, perm, "pb", kw)
        J = ctx.jacobian(x[perm]).tocsr()
        d = rhs(S.nn)
        ctx.amg_configure(smoother=SMOOTHER[smoother], **opts)
        v = ctx.prec_apply(d, P.PREC_AMG)
        info = ctx.amg_info()
        aggs = [ctx.amg_aggregates(q) for q in range(info["levels"] - 1)]
        graph_checks(J, info, aggs)
        assert info["rows"][0] == S.nn and (levels is None or info["levels"] == levels)
        if levels is None:
            assert info["levels"] >= 4 and info["rows"][-1] == 1
        cc, cb = R.conditioning(J, 1, aggs)
        assert cc <= COND_CAP and cb <= COND_CAP
        lay = P.Layout(mesh, degree=k)
        assert lay.n_owned == S.nn and lay.max_slots == ctx.info()["max_slots"]
        smooth0 = None if smoother == "jacobi" else (lambda r: R.multicolour_ssor(J, lay, 1, r))
        err, bound, N = cycle_figures(J, 1, aggs, d, v, opts.get("coarse_sweeps", 2), True, smooth0)
        print("AMG-FIG " + json.dumps(dict(id=f"{mesh_id}-P{k}-{smoother}", rows=info["rows"],
                                           err=err, bound=bound, N=N)))
        assert err <= bound
    finally:
        ctx.close()


# ---- stale values, reconfiguration, refusal, symmetry -------------------------------------------------
def single(src, kind):
    """(context with the operator set, mesh, layout, x, d); the caller closes the context"""
    mesh, par, orc, st, _ = problem(src)
    ctx = P.Context(mesh, par)
    _, x = set_kind(ctx, orc, st, kind)
    return ctx, mesh, P.Layout(mesh), x, rhs(x.size)


def reference_distance(ctx, J, mesh, lay, nf, d, v, opts=(1024, 12)):
    """hierarchy held, then (distance, bound) of v from the restated default cycle (SSOR)"""
    info = ctx.amg_info()
    aggs = [ctx.amg_aggregates(k) for k in range(info["levels"] - 1)]
    H = held_hierarchy(lay, mesh.nv, info, aggs, opts)
    perm = R.local_perm(lay, nf, mesh.nv)
    A0 = J[perm][:, perm].tocsr()
    cc, cb = R.conditioning(A0, nf, H["aggs"])
    assert cc <= COND_CAP and cb <= COND_CAP
    smooth0 = functools.partial(R.ssor_sweep, R.mask_same_colour(A0, lay, nf))
    err, bound, _ = cycle_figures(A0, nf, H["aggs"], d[perm], v[perm], 2, True, smooth0)
    return err, bound


def test_second_assembly_refreshes_the_coarse_values():
    ctx, mesh, lay, x1, d = single(CYL0, "pnp")
    try:
        J1 = ctx.jacobian(x1)
        ctx.amg_configure()
        v1 = ctx.prec_apply(d, P.PREC_AMG)
        J2 = ctx.jacobian(second_state(x1))
        v2 = ctx.prec_apply(d, P.PREC_AMG)
        e1, b1 = reference_distance(ctx, J1, mesh, lay, 3, d, v1)
        e2, b2 = reference_distance(ctx, J2, mesh, lay, 3, d, v2)
    finally:
        ctx.close()
    assert e1 <= b1 and e2 <= b2, (e1, b1, e2, b2)
    # the two cycles are far apart on the bound's scale: stale coarse values would show
    assert np.max(np.abs(v2 - v1)) > 1e3 * b2 * np.max(np.abs(v2))


def test_reconfiguration_rebuilds_and_returns():
    ctx, mesh, lay, x, d = single(CYL0, "pb")
    try:
        J = ctx.jacobian(x)
        res = []
        for target in (1024, 16, 1024):
            ctx.amg_configure(coarse_target=target)
            v = ctx.prec_apply(d, P.PREC_AMG)
            info = ctx.amg_info()
            res.append((v, info, reference_distance(ctx, J, mesh, lay, 1, d, v, (target, 12))))
    finally:
        ctx.close()
    assert [r[1]["levels"] for r in res] == [2, 3, 2] and res[1][1]["rows"][-1] <= 16
    assert np.array_equal(res[0][0], res[2][0])
    assert not np.array_equal(res[0][0], res[1][0])
    for _, _, (err, bound) in res:
        assert err <= bound


def test_too_large_a_coarsest_level_is_refused_and_the_context_recovers():
    """1,095 blocks x 3 fields > 3,072: an error return, and the context goes on.  (The pore's PNP
    systems fail the conditioning cap -- cond_2 of the coarsest matrix 1e9 .. 1e10 -- so the
    comparison after the refusal is made on the same context's PB operator.)"""
    ctx, mesh, lay, x, d = single(PORE1, "pnp")
    try:
        ctx.jacobian(x, export=False)
        ctx.amg_configure(max_levels=2)
        with pytest.raises(P.PnpError, match="coarsest level too large") as ei:
            ctx.prec_apply(d, P.PREC_AMG)
        assert ei.value.code == P.E_STATE
        ctx.amg_configure()
        v = ctx.prec_apply(d, P.PREC_AMG)
        info = ctx.amg_info()
        assert np.all(np.isfinite(v)) and np.any(v != 0)
        assert info["levels"] == 3 and info["rows"] == R.hierarchy(lay)["rows"]
        _, _, orc, st, _ = problem(PORE1)
        _, xb = set_kind(ctx, orc, st, "pb")
        Jb = ctx.jacobian(xb)
        db = rhs(xb.size)
        err, bound = reference_distance(ctx, Jb, mesh, lay, 1, db, ctx.prec_apply(db, P.PREC_AMG))
    finally:
        ctx.close()
    assert err <= bound, (err, bound)


def test_default_cycle_is_symmetric_positive_definite():
    """pinwheel_13_1_12, PB, no constrained row (a symmetric Jacobian), defaults: the cycle applied
    to the 30 unit vectors is a symmetric positive definite matrix, which CG relies on; and
    level0_presmooth = -1 is = 1 under pnp_prec_apply"""
    ctx, mesh, lay, x, d = single(fan("pinwheel_13_1_12", "free"), "pb")
    try:
        J = ctx.jacobian(x)
        assert abs(J - J.T).max() <= 1e-12 * abs(J).max()
        ctx.amg_configure()
        B = np.column_stack([ctx.prec_apply(e, P.PREC_AMG) for e in np.eye(mesh.nv)])
        va = ctx.prec_apply(d, P.PREC_AMG)
        ctx.amg_configure(level0_presmooth=1)
        vb = ctx.prec_apply(d, P.PREC_AMG)
        ctx.amg_configure(level0_presmooth=0)
        vc = ctx.prec_apply(d, P.PREC_AMG)
    finally:
        ctx.close()
    assert np.max(np.abs(B - B.T)) <= 1e-10 * np.max(np.abs(B))
    assert np.linalg.eigvalsh(0.5 * (B + B.T)).min() > 0
    assert np.array_equal(va, vb) and not np.array_equal(va, vc)
