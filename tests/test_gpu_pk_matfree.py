"""Matrix-free Jacobian application on P_k contexts of degree 2 and 3 (pnp_pk_matfree_set; the
kernels k_pk_elem_apply, k_pk_apply_gather and k_pk_diag of pk_assemble.hip) on the GPU (-m gpu).

Meshes: the generated ones of fan_meshes.PK_TABLE through the helpers of test_gpu_pk_edges.py --
1, 128 and 130 elements (the element pass runs 128 threads per workgroup: one element, one full
workgroup, a last one of 2), systems of 6, 65, 256 and 257 rows, a node in 1, 3, 4, 5, 8, 9, 10 and
20 elements (the row pass's batches of four), rows of 61 and 63 slots, pinch vertices.

Reference: the oracle's assembled P_k Jacobian Jo.  Bounds, all the project's own and unchanged:
    application          apply_error <= 1   (1e-12 max_i (|Jo| |v|)_i); constrained rows v, bitwise
    diagonal (Jacobi)    max|d - diag Jo| <= 1e-12 max|Jo|
    values on demand     bit for bit the assembled context's export (the same kernels at the same point)
    solves               converged, within 1e-8 max|x| of the assembled path's solution and +-1 of
                         its iteration count (test_gpu_matfree.test_cg_matches_oracle_cg's allowances)
    ranks                application as above; CG + Jacobi within 1e-9 relative of one rank's
    pnp_md_run           final state within 1e-8 max|u| of the assembled run's
    Newton               within 1e-6 of the assembled run's (the project's Newton bound)
The largest errors seen on the MI355X were 2.4e-3 of the application's bound and 3.3e-3 of the
diagonal's (both half_wheel_9 P3, free); the solves took the assembled path's iteration counts
exactly, their solutions within 7.7e-10 max|x|; the md states agreed to 1.1e-13 max|u|.  A miss is
a wrong kernel or table, not rounding.
tests/test_pk_apply_ref_host.py holds the same formulas to the oracle on the host."""
import json

import numpy as np
import pytest

import fan_meshes as F
import pnp_amd as P
from test_gpu_asm_const import second_state
from test_gpu_matfree import apply_error, random_z
from test_gpu_md_run import MAXIT, problem as md_problem
from test_gpu_pk import KINDS, args, bind, setup
from test_gpu_pk_edges import (KIND_ORDER, SPLIT_RUNS, _oracle_op, check_space, oracle_values,
                               problem, run_ranks, spoil)
from test_pk_edge_meshes_host import VARIANTS

pytestmark = pytest.mark.gpu


def mf_info(ctx):
    i = ctx.matfree_info()
    return i["applies"], i["value_assemblies"]


# ---- 1. application parity, 2. Jacobi without values ---------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id,k", F.PK_CASES)
def test_application_and_diagonal_match_oracle(mesh_id, k, variant):
    """the four operators at x and at second_state(x) on one context; between the Jacobian call and
    the application a residual at another state (the element buffer the two passes share with the
    residual then holds that residual's rows, and the context's state vector another state)"""
    mesh, par, orc, S = problem(mesh_id, k, variant)
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, mesh_id, k)
        ctx.pk_matfree(1)
        assert ctx.pk_matfree_get() == 1 and ctx.get_option(P.OPT_MATRIX_FREE) == 0
        bad, worst = [], {"apply": 0.0, "diag": 0.0}
        napp = 0
        for kind in KIND_ORDER:
            for second in (False, True):
                tag = f"{mesh_id}/P{k}/{variant}/{kind}/{int(second)}"
                x, kw, _, Jo, _ = oracle_values(mesh_id, k, variant, kind, second)
                op = bind(ctx, orc, S, perm, kind, kw) if not second else \
                    _oracle_op(orc, S, kind, kw)
                xp, Jo = x[perm], Jo[perm][:, perm]
                ctx.jacobian(xp, export=False)
                ctx.residual(spoil(xp))
                v = random_z(S.nn, 11 + int(second))
                y = ctx.jacobian_apply(v)
                napp += 1
                ea = apply_error(y, Jo, v)
                rows = np.nonzero(op._keep[1][perm])[0]
                if not np.array_equal(y[rows], v[rows]):
                    bad.append(f"{tag}: product on constrained rows is not v")
                d = random_z(S.nn, 13)
                w = ctx.prec_apply(d, P.PREC_JACOBI)
                ed = float(np.max(np.abs(d / w - Jo.diagonal())) / (1e-12 * abs(Jo).max()))
                worst["apply"], worst["diag"] = max(worst["apply"], ea), max(worst["diag"], ed)
                if not ea <= 1.0:
                    bad.append(f"{tag}: apply error / bound {ea:.3e}")
                if not ed <= 1.0:
                    bad.append(f"{tag}: diagonal error / bound {ed:.3e}")
                if mf_info(ctx) != (napp, 0):
                    bad.append(f"{tag}: counters {mf_info(ctx)} != {(napp, 0)}")
        print(f"PKMF-FIG {mesh_id} P{k} {variant} " + json.dumps(worst))
        assert not bad, bad
    finally:
        ctx.close()


# ---- 3. values on demand -------------------------------------------------------------------------
@pytest.mark.parametrize("mesh_id,k,kind", [("wheel_on_chain_20_100", 2, "pb"),
                                            ("wheel_on_chain_10_100", 3, "diff_ie"),
                                            ("half_wheel_21", 2, "diff"),
                                            ("diamond_chain_65", 3, "poisson")])
def test_values_on_demand_are_the_assembled_ones(mesh_id, k, kind):
    mesh, par, orc, S = problem(mesh_id, k, "mixed")
    x, kw, _, _, _ = oracle_values(mesh_id, k, "mixed", kind, False)
    ref = P.Context(mesh, par, device=0, degree=k)
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, mesh_id, k)
        bind(ref, orc, S, perm, kind, kw)
        bind(ctx, orc, S, perm, kind, kw)
        Jref = ref.jacobian(x[perm]).tocsr()
        assert ref.pk_matfree_get() == 0 and mf_info(ref) == (0, 1)
        ctx.pk_matfree(1)
        ctx.jacobian(x[perm], export=False)
        ctx.residual(spoil(x[perm]))
        assert mf_info(ctx) == (0, 0)
        for _ in range(2):  # the second export assembles nothing
            J = ctx.jacobian_export().tocsr()
            assert mf_info(ctx) == (0, 1)
            assert np.array_equal(J.indptr, Jref.indptr) and np.array_equal(J.indices, Jref.indices)
            assert np.array_equal(J.data, Jref.data)
        # turning the switch off with stale values assembles them once; the product is the SpMV's
        ctx.jacobian(second_state(x)[perm], export=False)
        assert mf_info(ctx) == (0, 1)
        ctx.pk_matfree(0)
        assert ctx.pk_matfree_get() == 0 and mf_info(ctx) == (0, 2)
        v = random_z(S.nn, 3)
        y = ctx.jacobian_apply(v)
        assert mf_info(ctx) == (0, 2)
        ref.jacobian(second_state(x)[perm], export=False)
        assert np.array_equal(y, ref.jacobian_apply(v))
    finally:
        ctx.close()
        ref.close()


def test_switch_surface():
    """E_STATE on a P1 context (and the getter reads 0), E_ARG for other values, the round trip, and
    PNP_OPT_MATRIX_FREE untouched on a P_k context"""
    mesh, par, _, _ = problem("half_wheel_5", 2, "free")
    c1 = P.Context(mesh, par, device=0)
    try:
        with pytest.raises(P.PnpError) as ei:
            c1.pk_matfree(1)
        assert ei.value.code == P.E_STATE
        with pytest.raises(P.PnpError) as ei:
            c1.pk_matfree(0)
        assert ei.value.code == P.E_STATE
        assert c1.pk_matfree_get() == 0
    finally:
        c1.close()
    ctx = P.Context(mesh, par, device=0, degree=2)
    try:
        assert ctx.pk_matfree_get() == 0
        for bad in (-1, 2):
            with pytest.raises(P.PnpError) as ei:
                ctx.pk_matfree(bad)
            assert ei.value.code == P.E_ARG
        ctx.pk_matfree(1)
        assert ctx.pk_matfree_get() == 1 and ctx.get_option(P.OPT_MATRIX_FREE) == 0
        with pytest.raises(P.PnpError) as ei:
            ctx.set_option(P.OPT_MATRIX_FREE, 1)
        assert ei.value.code == P.E_STATE
        ctx.set_option(P.OPT_MATRIX_FREE, 0)
        assert ctx.pk_matfree_get() == 1
        ctx.pk_matfree(0)
        assert ctx.pk_matfree_get() == 0
    finally:
        ctx.close()


# ---- 4. fused-dot modes and solves ---------------------------------------------------------------
def solve_system(kind, on):
    """a P2 context on the committed pore mesh with its Jacobian recorded / assembled, and a
    right-hand side: diff_ie with dt = 1e-3 (well conditioned, as test_gpu_matfree.diffusion_system)
    or PB at zero (symmetric positive definite: CG)"""
    mesh, ctx, orc = setup("pore_small", 2)
    ctx.pk_matfree(on)
    nn = ctx.nn
    x, kw = args(kind, nn, 5)
    if kind == "diff_ie":
        kw["dt"] = 1e-3
        ctx.set_operator(KINDS[kind][0], field=1, **kw)
    else:
        x = np.zeros(nn)
        ctx.set_operator(KINDS[kind][0])
    ctx.jacobian(x, export=False)
    # PB: the residual itself, zero on the constrained rows -- the iterates then stay zero there and
    # CG sees a symmetric operator although the columns of those rows are not eliminated
    rhs = ctx.residual(x) + (0.01 if kind == "diff_ie" else 0.0)
    ctx.residual(spoil(x))
    return ctx, rhs


SOLVES = [("bicgstab", "diff_ie", P.METHOD_BICGSTAB, P.PREC_NONE, 0),
          ("bicgstab_twored", "diff_ie", P.METHOD_BICGSTAB, P.PREC_NONE, 0),
          ("gmres", "diff_ie", P.METHOD_GMRES, P.PREC_NONE, 0),
          ("bicgstab_cheb3", "diff_ie", P.METHOD_BICGSTAB, P.PREC_CHEBYSHEV, 0),
          ("bicgstab_jacobi", "diff_ie", P.METHOD_BICGSTAB, P.PREC_JACOBI, 0),
          ("cg_none", "pb", P.METHOD_CG, P.PREC_NONE, 0),
          ("cg_jacobi", "pb", P.METHOD_CG, P.PREC_JACOBI, 0),
          ("bicgstab_ssor", "diff_ie", P.METHOD_BICGSTAB, P.PREC_SSOR, 1),
          ("bicgstab_ilu0", "pb", P.METHOD_BICGSTAB, P.PREC_ILU0, 1)]


@pytest.mark.parametrize("name,kind,method,prec,nval", SOLVES, ids=[s[0] for s in SOLVES])
def test_solves_match_the_assembled_path(name, kind, method, prec, nval):
    out = {}
    for on in (0, 1):
        ctx, rhs = solve_system(kind, on)
        try:
            if name == "bicgstab_twored":
                ctx.set_option(P.OPT_BICG_TWORED, 1)
            if prec == P.PREC_CHEBYSHEV:
                ctx.cheb_configure(steps=3)
            sol, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-10, maxit=5000,
                                        method=method, check_every=1)
            out[on] = (sol, res, mf_info(ctx))
        finally:
            ctx.close()
    (s0, r0, i0), (s1, r1, i1) = out[0], out[1]
    print(f"PKMF-SOLVE {name}: assembled {r0['iterations']} it, matrix-free {r1['iterations']} it, "
          f"max|dx| / max|x| {np.max(np.abs(s1 - s0)) / np.max(np.abs(s0)):.2e}, counters {i1}")
    assert r0["converged"] == 1 and r1["converged"] == 1, (r0, r1)
    assert np.max(np.abs(s1 - s0)) <= 1e-8 * np.max(np.abs(s0))
    assert abs(r1["iterations"] - r0["iterations"]) <= 1
    assert i0 == (0, 1)
    assert i1[0] > 0 and i1[1] == nval, i1


# ---- 5. ranks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("mesh_id,k", [("one_triangle", 2)] + SPLIT_RUNS)
def test_partitioned(mesh_id, k, n):
    """2 and 3 in-process ranks: the application of the four operators against the oracle (each
    rank returns its owned rows), and a CG + Jacobi solve against one rank's.  one_triangle at P2
    leaves a rank 2 of 6 nodes; the hub row of wheel_on_chain has ghosts on every other rank.  The
    solve's system is diff_ie with a zero potential and dt = 1e-3: mass + dt stiffness, symmetric
    positive definite at P2 and P3 (the rules of orders 5 and 2 have positive weights; the
    order-3 rule of PB / Poisson makes the P3 matrices indefinite)."""
    mesh, par, orc, S = problem(mesh_id, k, "mixed")
    c1 = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(c1, S, mesh_id, k)
    finally:
        c1.close()
    vals = {kind: oracle_values(mesh_id, k, "mixed", kind, False) for kind in KIND_ORDER}
    v = random_z(S.nn, 17)
    rng = np.random.default_rng(23)
    xold, rhs = rng.uniform(0.0, 0.1, S.nn), rng.uniform(-1.0, 1.0, S.nn)
    rhs[S.mask(2)[perm] != 0] = 0.0

    def fn(c):
        c.pk_matfree(1)
        res = {"owned": c.info()["nv_owned"]}
        for kind in KIND_ORDER:
            x, kw = vals[kind][:2]
            pk = {q: (a[perm] if isinstance(a, np.ndarray) else a) for q, a in kw.items()}
            if kind.startswith("diff"):
                pk["field"] = 2
            c.set_operator(KINDS[kind][0], **pk)
            c.jacobian(x[perm], export=False)
            c.residual(spoil(x[perm]))
            res[kind] = c.jacobian_apply(v)
        c.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=1e-3, z=-1.0, field=2, phi=np.zeros(S.nn),
                       x_old=xold)
        c.jacobian(xold, export=False)
        res["solve"] = c.linear_solve(rhs, prec=P.PREC_JACOBI, reduction=1e-12, maxit=5000,
                                      method=P.METHOD_CG, check_every=1)
        res["info"] = mf_info(c)
        return res

    c1 = P.Context(mesh, par, device=0, degree=k)
    try:
        one = [fn(c1)]
    finally:
        c1.close()
    out, err = run_ranks(n, mesh, par, k, fn)
    assert not err, err
    owned = [o["owned"] for o in out]
    print(f"PKMF-RANKS {mesh_id} P{k} {n} ranks own {owned}")
    assert sum(owned) == S.nn and min(owned) >= 1
    for kind in KIND_ORDER:
        Jo = vals[kind][3][perm][:, perm]
        y = sum(o[kind] for o in out)  # each rank writes its owned rows, zeros elsewhere
        assert apply_error(y, Jo, v) <= 1.0, kind
        rows = np.nonzero(S.mask(2 if kind.startswith("diff") else 0)[perm])[0]
        assert np.array_equal(y[rows], v[rows])
    s1, r1 = one[0]["solve"]
    sol = sum(o["solve"][0] for o in out)
    assert r1["converged"] == 1 and all(o["solve"][1]["converged"] == 1 for o in out)
    assert np.max(np.abs(sol - s1)) <= 1e-9 * np.max(np.abs(s1))
    assert all(o["info"][0] > 0 and o["info"][1] == 0 for o in out + one)


# ---- 6. pnp_md_run -------------------------------------------------------------------------------
@pytest.mark.parametrize("reuse", [0, 1])
def test_md_run_p2(reuse):
    """3 steps on the committed pore mesh at P2 from its Boltzmann state, CG + Jacobi (the
    reference's CG_Jacobi backend): no value assembly with the switch on, the assembled run's
    counts and final state.

    The time step is 1e-3, that of the well-conditioned diff_ie system above, not the 0.05 of
    test_gpu_md_run.problem: CG needs a symmetric operator, and the DiffusionTOperator's is
    mass + a dt (stiffness + drift) with a non-symmetric drift term that grows with dt and with the
    potential's gradient.  At dt = 0.05 CG + Jacobi does not bring the first diffusion solve of
    this P2 problem to its reduction of 1e-5 on either path (measured on the MI355X: status
    PNP_E_NOT_CONVERGED after 5,000 iterations, the switch off and on alike, steps_done 0), so
    there the two runs could only be compared on a failed step.  At 1e-3 the mass dominates."""
    mesh, par, _, freqs, u0 = md_problem("pore", 2)
    dt = 1e-3
    out = {}
    for on in (0, 1):
        ctx = P.Context(mesh, par, degree=2)
        try:
            ctx.pk_matfree(on)
            u, t, ip, im, res = ctx.md_run(u0, dt, 3, prec=P.PREC_JACOBI, method=P.METHOD_CG,
                                           maxit=MAXIT, reuse=reuse)
            out[on] = (u, res, mf_info(ctx))
        finally:
            ctx.close()
    (u_a, r_a, i_a), (u_m, r_m, i_m) = out[0], out[1]
    print(f"PKMF-MD reuse {reuse}: assembled {r_a}, matrix-free {r_m}, counters {i_m}, "
          f"max|du| / max|u| {np.max(np.abs(u_m - u_a)) / np.max(np.abs(u_a)):.2e}")
    assert r_a["status"] == r_m["status"] == P.OK
    assert r_a["assemblies"] > 0 and r_m["assemblies"] == 0 and i_m[1] == 0 and i_m[0] > 0
    for key in ("steps_done", "diffusion_solves", "poisson_solves", "prec_setups", "noutputs"):
        assert r_a[key] == r_m[key], key
    assert r_m["steps_done"] == 3
    assert np.max(np.abs(u_m - u_a)) <= 1e-8 * np.max(np.abs(u_a))


# ---- 7. Newton -----------------------------------------------------------------------------------
def test_pb_newton_p2():
    out = {}
    for on in (0, 1):
        mesh, ctx, orc = setup("pore_small", 2)
        try:
            ctx.pk_matfree(on)
            ctx.set_operator(P.OP_PB)
            u, res = ctx.newton(np.zeros(ctx.nn), prec=P.PREC_JACOBI, method=P.METHOD_CG)
            out[on] = (u, res, mf_info(ctx))
        finally:
            ctx.close()
    (u_a, r_a, i_a), (u_m, r_m, i_m) = out[0], out[1]
    assert r_a["converged"] == 1 and r_m["converged"] == 1, (r_a, r_m)
    assert i_a[1] > 0 and i_m[1] == 0 and i_m[0] > 0, (i_a, i_m)
    assert np.max(np.abs(u_m - u_a)) <= 1e-6 * np.max(np.abs(u_a))


# ---- 8. forward differences leave the switch alone -------------------------------------------------
@pytest.mark.parametrize("mesh_id,k", [("pinwheel_3_1_2", 2), ("half_wheel_9", 3)])
def test_fd_takes_the_assembled_path(mesh_id, k):
    mesh, par, orc, S = problem(mesh_id, k, "mixed")
    x, kw, _, _, _ = oracle_values(mesh_id, k, "mixed", "pb", False)
    v = random_z(S.nn, 29)
    ys = {}
    for on in (0, 1):
        ctx = P.Context(mesh, par, device=0, degree=k)
        try:
            perm = check_space(ctx, S, mesh_id, k)
            ctx.pk_matfree(on)
            bind(ctx, orc, S, perm, "pb", kw)
            ys[on] = ctx.jacobian_apply(v, x[perm], fd=True)
            assert mf_info(ctx) == (0, 1)
            assert ctx.pk_matfree_get() == on
        finally:
            ctx.close()
    assert np.array_equal(ys[0], ys[1])
