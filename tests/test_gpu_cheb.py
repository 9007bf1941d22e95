"""GPU tests (-m gpu) of the Chebyshev polynomial preconditioner on vertex-block Jacobi
(PNP_PREC_CHEBYSHEV).

Reference: tests/cheb_ref.py (held to itself by tests/test_cheb_ref_host.py) on J = ctx.jacobian(x)
with the bounds the library reports (cheb_info) unless a test says otherwise.  Bound of one
application: 1e-10 max|v|, the project's figure for an fp64 preconditioner application (DESIGN.md
4.6); the observed maxima are printed.  Solves: |J z - b| <= 1.001 reduction |b| (check2) and at
most twice the iterations of the numpy yardstick on the same J with the restated preconditioner
(BiCGSTAB's counts move by +-15 % with the last bit on these systems; the yardstick itself sets
the cap)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amg_ref
import cheb_ref as R
import pnp_amd as P
from test_cheb_ref_host import FAN_KINDS, FAN_MESHES, STEPS, VARIANTS, nf_of
from test_gpu import golden
from test_gpu_fan_walks import problem as fan_problem, set_kind
from test_gpu_gmres import assembled, check2, system
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-10
FUSED_ENV = "PNP_CHEB_FUSED"


def rhs(n, seed=11):
    return np.random.default_rng(seed).standard_normal(n)


def restated(ctx, J, nf, d, owned=None):
    """the restatement with the context's configured steps and the bounds it last used"""
    i = ctx.cheb_info()
    if i["steps"] == 1:
        assert i["lambda_max"] == 0 and i["lambda_min"] == 0 and i["lambda_est"] == 0
        return R.apply(J, nf, d, 1, owned=owned)
    assert i["lambda_max"] > i["lambda_min"] > 0
    return R.apply(J, nf, d, i["steps"], i["lambda_max"], i["lambda_min"], owned=owned)


def apply_error(ctx, J, nf, d, steps, lambda_max):
    ctx.cheb_configure(steps=steps, lambda_max=lambda_max)
    v = ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    i = ctx.cheb_info()
    if steps > 1 and lambda_max > 0:
        assert i["lambda_max"] == lambda_max and i["lambda_min"] == lambda_max / 10.0
        assert i["lambda_est"] == 0
    if steps > 1 and lambda_max == 0:
        assert i["lambda_max"] == 1.1 * i["lambda_est"] > 0
    vr = restated(ctx, J, nf, d)
    assert np.all(np.isfinite(v))
    return float(np.max(np.abs(v - vr)) / np.max(np.abs(vr)))


# ---- 1. the application against the restatement ---------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id", FAN_MESHES)
def test_application_on_fan_meshes(mesh_id, variant):
    mesh, par, orc, st, _ = fan_problem(mesh_id, variant)
    ctx = P.Context(mesh, par)
    worst, bad = 0.0, []
    try:
        for kind in FAN_KINDS:
            _, x = set_kind(ctx, orc, st, kind)
            J = ctx.jacobian(x).tocsr()
            d = rhs(x.size)
            for steps in STEPS:
                for lmax in (2.5, 0.0):
                    e = apply_error(ctx, J, nf_of(kind), d, steps, lmax)
                    worst = max(worst, e)
                    if not e <= BOUND:
                        bad.append(f"{kind} steps {steps} lambda_max {lmax}: {e:.3e}")
    finally:
        ctx.close()
    print(f"CHEB-FIG {mesh_id} {variant}: worst application error {worst:.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["pnp", "pb"])
def test_application_on_pore_pnp_k0(kind):
    """12 workgroups, staged lists of several hundred to over a thousand entries"""
    ctx, J, _ = assembled(f"pore_pnp_k0:{kind}")
    assert ctx.info()["nv_owned"] > 11 * 256
    d = rhs(J.shape[0])
    worst = 0.0
    for steps in STEPS:
        for lmax in (2.5, 0.0):
            worst = max(worst, apply_error(ctx, J, nf_of(kind), d, steps, lmax))
    i = ctx.cheb_info()
    ctx.close()
    print(f"CHEB-FIG pore_pnp_k0 {kind}: worst application error {worst:.3e}, "
          f"fused {i['fused_steps']} unfused {i['unfused_steps']}")
    assert worst <= BOUND


# ---- 2. the estimate -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pnp", "pb"])
def test_estimate(kind):
    which = f"cylinder_k0:{kind}"
    nf = nf_of(kind)
    ctx, J, b = assembled(which)
    assert ctx.cheb_info()["estimates"] == 0 and ctx.cheb_info()["lambda_est"] == 0
    d = rhs(J.shape[0])
    ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    i = ctx.cheb_info()
    ref = R.power_estimate(J, nf, 20)
    print(f"CHEB-FIG estimate {which}: {i['lambda_est']:.15g} against {ref:.15g}")
    assert i["steps"] == 3 and i["estimates"] == 1
    assert abs(i["lambda_est"] - ref) <= 1e-10 * ref
    assert i["lambda_max"] == 1.1 * i["lambda_est"] and i["lambda_min"] == i["lambda_max"] / 10.0
    # once per stored Jacobian, not per application or solve
    ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    for _ in range(2):
        _, res = ctx.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-6, maxit=5000)
        assert res["converged"] == 1
    assert ctx.cheb_info()["estimates"] == 1
    # a second context gives the same bits
    ctx2, _, _ = assembled(which)
    ctx2.prec_apply(d, P.PREC_CHEBYSHEV)
    assert ctx2.cheb_info()["lambda_est"] == i["lambda_est"]
    ctx2.close()
    # a second assembly re-estimates
    _, _, setup, _ = system(which)
    x2 = setup(ctx) + 0.01 * rhs(J.shape[0], 3) * (1 if kind == "pb" else 0.01)
    J2 = ctx.jacobian(x2).tocsr()
    ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    i2 = ctx.cheb_info()
    ref2 = R.power_estimate(J2, nf, 20)
    assert i2["estimates"] == 2 and abs(i2["lambda_est"] - ref2) <= 1e-10 * ref2
    # cheb_configure resets it; another iteration count gives the restated value for it
    ctx.cheb_configure(eig_iters=7)
    i3 = ctx.cheb_info()
    assert i3["lambda_est"] == 0 and i3["lambda_max"] == 0 and i3["estimates"] == 2
    ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    i3 = ctx.cheb_info()
    ref3 = R.power_estimate(J2, nf, 7)
    assert i3["estimates"] == 3 and abs(i3["lambda_est"] - ref3) <= 1e-10 * ref3
    # steps 1 runs none
    ctx.cheb_configure(steps=1)
    ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    assert ctx.cheb_info()["estimates"] == 3
    ctx.close()


# ---- 3. fused against unfused --------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_cheb as T
print("RESULT " + json.dumps(T.child_main()))
"""
CHILD_STEPS = (2, 3, 4, 7)


def child_cases():
    ctx, J, _ = assembled("pore_small_k0:pnp")
    yield "pore_small_k0", ctx, J, 3
    mesh, par, orc, st, _ = fan_problem("diamond_chain_86", "mixed")
    ctx = P.Context(mesh, par)
    _, x = set_kind(ctx, orc, st, "pnp")
    yield "diamond_chain_86", ctx, ctx.jacobian(x).tocsr(), 3


def child_main():
    out = {}
    for name, ctx, J, nf in child_cases():
        d = rhs(J.shape[0])
        for steps in CHILD_STEPS:
            ctx.cheb_configure(steps=steps, lambda_max=2.5)
            v = ctx.prec_apply(d, P.PREC_CHEBYSHEV)
            vr = restated(ctx, J, nf, d)
            out[f"{name}:{steps}"] = dict(v=v.tolist(), scale=float(np.max(np.abs(vr))),
                                          err=float(np.max(np.abs(v - vr))))
        i = ctx.cheb_info()
        out[name] = dict(fused=i["fused_steps"], unfused=i["unfused_steps"], applies=i["applies"])
        ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def child(fused):
    env = {k: v for k, v in os.environ.items() if k != FUSED_ENV}
    env[FUSED_ENV] = str(fused)
    p = subprocess.run([sys.executable, "-c", CHILD.replace("HERE", repr(HERE))], env=env,
                       capture_output=True, text=True, timeout=120, cwd=HERE)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_fused_against_unfused():
    a, b = child(1), child(0)
    nsteps = sum(s - 1 for s in CHILD_STEPS)
    worst = 0.0
    for name in ("pore_small_k0", "diamond_chain_86"):
        assert a[name] == dict(fused=nsteps, unfused=0, applies=len(CHILD_STEPS)), a[name]
        assert b[name] == dict(fused=0, unfused=nsteps, applies=len(CHILD_STEPS)), b[name]
        for steps in CHILD_STEPS:
            fa, fb = a[f"{name}:{steps}"], b[f"{name}:{steps}"]
            assert fa["err"] <= BOUND * fa["scale"] and fb["err"] <= BOUND * fb["scale"]
            diff = np.max(np.abs(np.array(fa["v"]) - np.array(fb["v"]))) / fa["scale"]
            worst = max(worst, float(diff))
    print(f"CHEB-FIG fused against unfused: {worst:.3e}")
    assert worst <= BOUND


# ---- 4. solves -------------------------------------------------------------------------------------
def yardstick_cap(J, nf, b, reduction, method="bicgstab", **opts):
    M = R.preconditioner(J, nf, **opts)
    solve = R.bicgstab if method == "bicgstab" else R.cg
    _, its, conv = solve(J, b, M, reduction, 5000)
    assert conv
    return int(np.ceil(its))


@pytest.mark.parametrize("which", ["cylinder_k0:pnp", "pore_small_k0:pnp", "pore_small_k0:diff_ie",
                                   "pore_pnp_k0:pnp"])
def test_bicgstab_with_three_steps(which):
    ctx, J, b = assembled(which)
    nf = 3 if which.endswith(":pnp") else 1
    z, res = ctx.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8, maxit=5000)
    cap = 2 * yardstick_cap(J, nf, b, 1e-8)
    print(f"CHEB-FIG bicgstab {which}: {res['iterations']} iterations, cap {cap}")
    ctx.close()
    assert res["converged"] == 1 and res["breakdown"] == 0, res
    check2(J, z, b, 1e-8)
    assert res["iterations"] <= cap


def test_cg_on_pb():
    ctx, J, b = assembled("pore_small_k0:pb")
    z, res = ctx.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8, maxit=5000,
                              method=P.METHOD_CG)
    cap = 2 * yardstick_cap(J, 1, b, 1e-8, method="cg")
    print(f"CHEB-FIG cg pore_small_k0:pb: {res['iterations']} iterations, cap {cap}")
    ctx.close()
    assert res["converged"] == 1, res
    check2(J, z, b, 1e-8)
    assert res["iterations"] <= cap


@pytest.mark.parametrize("method", [P.METHOD_GMRES, P.METHOD_FGMRES, P.METHOD_IDR])
def test_other_methods(method):
    ctx, J, b = assembled("cylinder_k0:pnp")
    z, res = ctx.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8, maxit=5000, method=method)
    ctx.close()
    assert res["converged"] == 1 and res["breakdown"] == 0, res
    check2(J, z, b, 1e-8)


@pytest.mark.parametrize("name,kind", [("cylinder_k0", "pnp"), ("sphere_k0", "pb")])
def test_newton(name, kind):
    z, mesh, par, _ = golden(name)
    ctx = P.Context(mesh, par)
    if kind == "pnp":
        ctx.set_operator(P.OP_PNP)
        u, res = ctx.newton(z["newton_pnp_x0"], prec=P.PREC_CHEBYSHEV)
        ref = z["newton_pnp_u"]
    else:
        ctx.set_operator(P.OP_PB)
        u, res = ctx.newton(np.zeros(mesh.nv), prec=P.PREC_CHEBYSHEV)
        ref = z["newton_pb_u"]
    i = ctx.cheb_info()
    ctx.close()
    assert res["status"] == 0 and res["converged"] == 1, res
    assert np.max(np.abs(u - ref)) <= 1e-6 * np.max(np.abs(ref))
    assert 0 < i["estimates"] <= res["iterations"]  # at most one per Newton step's Jacobian


def test_md_run_two_steps_bitwise():
    from test_gpu_md_run import check_bitwise
    check_bitwise("pore", 2, prec=P.PREC_CHEBYSHEV)


# ---- 5. matrix-free -------------------------------------------------------------------------------
def test_matrix_free():
    mesh, par, setup, _ = system("pore_pnp_k0:pnp")
    ctx, J, b = assembled("pore_pnp_k0:pnp")
    d = rhs(J.shape[0])
    ctx.cheb_configure(steps=4)
    va = ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    ctx.close()
    mf = P.Context(mesh, par)
    mf.set_option(P.OPT_MATRIX_FREE, 1)
    x = setup(mf)
    mf.jacobian(x, export=False)
    mf.cheb_configure(steps=4)
    va0 = mf.matfree_info()["value_assemblies"]
    z, res = mf.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8, maxit=5000)
    vm = mf.prec_apply(d, P.PREC_CHEBYSHEV)
    i = mf.cheb_info()
    va1 = mf.matfree_info()["value_assemblies"]
    mf.close()
    cap = 2 * yardstick_cap(J, 3, b, 1e-8, steps=4)
    print(f"CHEB-FIG matrix-free: {res['iterations']} iterations (cap {cap}), application against "
          f"the assembled one {np.max(np.abs(vm - va)) / np.max(np.abs(va)):.3e}")
    assert res["converged"] == 1, res
    check2(J, z, b, 1e-8)
    assert res["iterations"] <= cap
    assert va1 == va0 and i["unfused_steps"] > 0 and i["fused_steps"] == 0
    assert np.max(np.abs(vm - va)) <= BOUND * np.max(np.abs(va))


# ---- 6. ranks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_ranks(nranks):
    mesh, par, setup, _ = system("cylinder_k0:pnp")
    ctx, J, b = assembled("cylinder_k0:pnp")
    d = rhs(J.shape[0])
    one = {}
    for lmax in (2.5, 0.0):
        ctx.cheb_configure(lambda_max=lmax)
        one[lmax] = (ctx.prec_apply(d, P.PREC_CHEBYSHEV), ctx.cheb_info())
    ctx.close()

    def fn(c, r):
        x = setup(c)
        c.jacobian(x, export=False)
        out = {}
        for lmax in (2.5, 0.0):
            c.cheb_configure(lambda_max=lmax)
            out[lmax] = (c.sync_vector(c.prec_apply(d, P.PREC_CHEBYSHEV)), c.cheb_info())
        sol, res = c.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8, maxit=5000)
        return out, c.sync_vector(sol), res
    for out, sol, res in run_ranks(nranks, mesh, par, fn):
        for lmax in (2.5, 0.0):
            v1, i1 = one[lmax]
            v, i = out[lmax]
            assert np.max(np.abs(v - v1)) <= BOUND * np.max(np.abs(v1))
            assert i["fused_steps"] == 0 and i["unfused_steps"] > 0
            if lmax == 0.0:
                assert abs(i["lambda_est"] - i1["lambda_est"]) <= 1e-12 * i1["lambda_est"]
        assert res["converged"] == 1, res
        check2(J, sol, b, 1e-8)


# ---- 7. AMG ----------------------------------------------------------------------------------------
def amg_calls(ctx, setup, d, steps):
    x = setup(ctx)
    J = ctx.jacobian(x)
    ctx.cheb_configure(steps=steps)
    ctx.amg_configure(smoother=P.PREC_CHEBYSHEV, coarse_target=16)
    v = ctx.prec_apply(d, P.PREC_AMG)
    info = ctx.amg_info()
    aggs = [ctx.amg_aggregates(k) for k in range(info["levels"] - 1)]
    return dict(J=J, v=v, info=info, aggs=aggs, cheb=ctx.cheb_info())


def amg_compare(out, J1, mesh, nf, d, rank, nranks):
    nv = mesh.nv
    lay = P.Layout(mesh, rank, nranks)
    perm = amg_ref.local_perm(lay, nf, nv)
    owned = out["aggs"][0] >= 0
    assert owned.sum() == lay.n_owned
    A0 = J1[perm][:, perm].tocsr()
    c = out["cheb"]

    def smooth0(r):  # the rank-local form, on the owned rows in the layout's order
        e = np.zeros(nf * nv)
        e[perm] = r
        return R.apply(J1, nf, e, c["steps"], c["lambda_max"] or None, c["lambda_min"] or None,
                       owned=owned)[perm]
    aggs = [out["aggs"][0][lay.l2g[:lay.n_owned]]] + out["aggs"][1:]
    f32 = os.environ.get("PNP_AMG_F32", "1") != "0"
    vr = amg_ref.numpy_vcycle(A0, nf, aggs, 0.8, d[perm], 2, True, f32, smooth0=smooth0)
    return float(np.max(np.abs(out["v"][perm] - vr)) / np.max(np.abs(vr)))


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("kind", ["pnp", "pb"])
@pytest.mark.parametrize("nranks", [1, 2])
def test_amg_cycle(nranks, kind, steps):
    mesh, par, setup, _ = system(f"cylinder_k0:{kind}")
    nf = nf_of(kind)
    d = rhs(nf * mesh.nv)
    ctx = P.Context(mesh, par)
    one = amg_calls(ctx, setup, d, steps)
    ctx.close()
    J1 = one["J"].tocsr()
    if nranks == 1:
        outs = [one]
    else:
        outs = run_ranks(nranks, mesh, par, lambda c, r: amg_calls(c, setup, d, steps))
    for r, out in enumerate(outs):
        assert out["info"]["smoother"] == P.PREC_CHEBYSHEV and out["info"]["levels"] >= 2
        e = amg_compare(out, J1, mesh, nf, d, r, nranks)
        print(f"CHEB-FIG amg {kind} steps {steps} rank {r}/{nranks}: {e:.3e}")
        assert e <= 1e-7


def test_amg_solve():
    ctx, J, b = assembled("pore_small_k0:pnp")
    ctx.amg_configure(smoother=P.PREC_CHEBYSHEV)
    z, res = ctx.linear_solve(b, prec=P.PREC_AMG, reduction=1e-8, maxit=5000)
    ctx.close()
    assert res["converged"] == 1 and res["breakdown"] == 0, res
    check2(J, z, b, 1e-8)


# ---- 8. P_k, device pointers, edges ---------------------------------------------------------------
def test_pk_degree_two():
    import fan_meshes as F
    from test_gpu_fans import SURF
    from test_gpu_fan_walks import PHYS
    xy, tri, bseg, bgroup = F.pk_make("half_wheel_6", "alt")
    mesh = P.Mesh(xy, tri, bseg, bgroup)
    par = P.Params([P.Surface(**s) for s in SURF], **PHYS)
    ctx = P.Context(mesh, par, degree=2)
    ctx.set_operator(P.OP_PB)
    x = 0.3 * rhs(ctx.nn, 5)
    J = ctx.jacobian(x).tocsr()
    d = rhs(ctx.nn)
    errs = [apply_error(ctx, J, 1, d, 3, lmax) for lmax in (2.5, 0.0)]
    ctx.close()
    print(f"CHEB-FIG P2 half_wheel_6: {max(errs):.3e}")
    assert max(errs) <= BOUND


def test_device_pointers():
    from test_gpu_boundary import _Hip
    ctx, J, b = assembled("pore_small_k0:pb")
    sol, res = ctx.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8)
    hip = _Hip()
    bd, zd = hip.h2d(b), hip.h2d(np.zeros(b.size))
    rd = ctx.linear_solve_dev(bd, zd, prec=P.PREC_CHEBYSHEV, reduction=1e-8)
    assert rd["converged"] == 1 and rd["iterations"] == res["iterations"]
    np.testing.assert_array_equal(hip.d2h(zd, b.size, np.float64), sol)
    ctx.close()
    hip.free()


def test_edges():
    mesh, par, setup, _ = system("pore_small_k0:pb")
    ctx = P.Context(mesh, par)
    x = setup(ctx)
    d = rhs(mesh.nv)
    with pytest.raises(P.PnpError) as ei:  # before an assembly
        ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    assert ei.value.code == P.E_STATE
    for bad in (dict(steps=0), dict(steps=17), dict(eig_ratio=1.0), dict(eig_ratio=float("nan")),
                dict(eig_iters=0), dict(eig_iters=101), dict(eig_boost=0.99),
                dict(lambda_max=-1.0)):
        with pytest.raises(P.PnpError) as ei:
            ctx.cheb_configure(**bad)
        assert ei.value.code == P.E_ARG, bad
    assert ctx.cheb_info()["steps"] == 3
    assert P.lib().pnp_cheb_configure(ctx.h, None) == P.OK  # NULL: the defaults
    assert P.PREC_BY_NAME["cheb"] == P.PREC_CHEBYSHEV == 6
    # reference-order mode keeps refusing it
    ctx.set_option(P.OPT_SEQ_ORDER, 1)
    ctx.jacobian(x, export=False)
    with pytest.raises(P.PnpError) as ei:
        ctx.prec_apply(d, P.PREC_CHEBYSHEV)
    assert ei.value.code == P.E_ARG
    with pytest.raises(P.PnpError) as ei:
        ctx.linear_solve(d, prec=P.PREC_CHEBYSHEV)
    assert ei.value.code == P.E_ARG
    ctx.close()


def test_graph_replay_across_two_assemblies():
    mesh, par, setup, _ = system("cylinder_k0:pnp")
    outs = {}
    for graph in (0, 1):
        ctx = P.Context(mesh, par)
        ctx.set_option(P.OPT_GRAPH, graph)
        x = setup(ctx)
        outs[graph] = []
        for k in range(2):  # the second Jacobian changes the bounds under the captured graph
            xk = x * (1.0 + 0.05 * k)
            ctx.jacobian(xk, export=False)
            b = ctx.residual(xk) + 0.01
            sol, res = ctx.linear_solve(b, prec=P.PREC_CHEBYSHEV, reduction=1e-8, maxit=5000,
                                        check_every=4)
            assert res["converged"] == 1, res
            outs[graph].append((sol, res["it_half"], ctx.cheb_info()["lambda_est"]))
        ctx.close()
    assert outs[1][0][2] != outs[1][1][2]
    for (s0, h0, l0), (s1, h1, l1) in zip(outs[0], outs[1]):
        assert h0 == h1 and l0 == l1
        np.testing.assert_array_equal(s0, s1)
