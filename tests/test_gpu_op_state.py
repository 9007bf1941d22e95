"""What a context holds of its operator and Jacobian across operator, form, precision and mode
changes (-m gpu): one long-lived context walks a scripted sequence, and after every step what it
returns equals, bit for bit, what a fresh context returns that was given only that step's operator
and options.  The counters of the walks (pnp_asm_info, pnp_matfree_info, the factorisation timer)
pin that a transition invalidates neither more nor less than it did.

data/cylinder.msh (311 vertices) and data/pore.msh (320 vertices), unrefined: the logic under test
is host bookkeeping.
"""
import numpy as np
import pytest

import pnp_amd as P
from test_gpu_md_run import MAXIT, problem, yardstick
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

MESHES = ["cyl", "pore"]
PRECS = (P.PREC_JACOBI, P.PREC_SSOR, P.PREC_ILU0, P.PREC_AMG)
NV = {"cyl": 311, "pore": 320}


def fresh_ctx(name, **kw):
    mesh, par, _, _, _ = problem(name)
    ctx = P.Context(mesh, par, **kw)
    configure(ctx)
    return ctx


def configure(ctx):
    # a real hierarchy on 300 vertices (the default coarse target is above them)
    ctx.amg_configure(smoother=P.PREC_SSOR, coarse_target=32)


def operators(name):
    """the walk of case 1: (label, set_operator arguments, state) -- seeded states off the
    Boltzmann state, so that no residual is zero"""
    mesh, par, dt, _, u0 = problem(name)
    nn = mesh.nv
    assert nn == NV[name]
    rng = np.random.default_rng(20261020)
    phi, cp, cm = (u0[k * nn:(k + 1) * nn] for k in range(3))
    x3 = u0 * (1.0 + 0.05 * rng.uniform(-1, 1, 3 * nn))
    x1 = {k: v * (1.0 + 0.05 * rng.uniform(-1, 1, nn)) + 0.01 * rng.uniform(-1, 1, nn)
          for k, v in (("phi", phi), ("cp", cp), ("cm", cm))}
    return [
        ("pnp", dict(kind=P.OP_PNP), x3),
        ("pb", dict(kind=P.OP_PB), x1["phi"]),
        ("pnp_ie", dict(kind=P.OP_PNP_IMPLICIT_EULER, dt=dt, x_old=u0), x3),
        ("diff1", dict(kind=P.OP_DIFF, z=+1.0, field=1, phi=phi), x1["cp"]),
        ("diff2", dict(kind=P.OP_DIFF, z=-1.0, field=2, phi=phi), x1["cm"]),
        ("poisson", dict(kind=P.OP_POISSON, cp=cp, cm=cm), x1["phi"]),
        ("pnp_again", dict(kind=P.OP_PNP), x3),
    ]


def solve(ctx, rhs, prec, **kw):
    z, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=2000, **kw)
    return [z, np.array([res[k] for k in ("iterations", "converged", "breakdown")]),
            ctx.solve_history()]


def take(ctx, x, seed=7):
    """case 1's quantities of the current operator at x, as a list of raw arrays"""
    r = ctx.residual(x)
    J = ctx.jacobian(x, export=True)
    d = np.random.default_rng(seed).uniform(-1, 1, x.size)
    out = [r, J.indptr, J.indices, J.data]
    out += [ctx.prec_apply(d, p) for p in PRECS]
    return out + solve(ctx, r, P.PREC_ILU0)


def same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{what}: quantity {k} differs"


def walk_operators(ctx, name):
    for label, args, x in operators(name):
        ctx.set_operator(**args)
        got = take(ctx, x)
        ref = fresh_ctx(name)
        ref.set_operator(**args)
        want = take(ref, x)
        ref.close()
        same(got, want, f"{name} after set_operator({label})")


# ---- 1. operator changes -------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_operator_changes(name):
    ctx = fresh_ctx(name)
    walk_operators(ctx, name)
    ctx.close()


# ---- 2. form changes on one operator -------------------------------------------------------------
# pnp_asm_info's (full, reused) after the sequence, recorded from the parent of the change that
# routed the transitions through pnp_ctx's members (commit ea168f6).  Full: the first analytic
# assembly, the forward-difference one, and the analytic one after it (set_fd dropped the constant
# planes).  Reusing them: the matrix-free Jacobian's values for ILU(0), and the assembly after
# PNP_OPT_SEQ_ORDER went on and off again, which leaves vals alone
ASM_COUNTS = {"cyl": (3, 2), "pore": (3, 2)}


def expect_no_jacobian(ctx, d):
    for call in (lambda: ctx.linear_solve(d, prec=P.PREC_JACOBI),
                 lambda: ctx.prec_apply(d, P.PREC_JACOBI)):
        with pytest.raises(P.PnpError) as ei:
            call()
        assert ei.value.code == P.E_STATE and "no Jacobian assembled" in str(ei.value)


@pytest.mark.parametrize("name", MESHES)
def test_form_changes(name):
    _, _, x = operators(name)[0]
    ctx = fresh_ctx(name)
    ctx.set_operator(P.OP_PNP)
    r = ctx.residual(x)

    def step(what, fn, opts=(), jac=False):
        """fn(ctx) against fn of a fresh context with `opts` and the PNP operator (jac: and its
        Jacobian at x)"""
        got = fn(ctx)
        ref = fresh_ctx(name)
        for o, v in opts:
            ref.set_option(o, v)
        ref.set_operator(P.OP_PNP)
        if jac:
            ref.jacobian(x, export=False)
        want = fn(ref)
        ref.close()
        same(got, want, f"{name}: {what}")

    def exported(c, fd=False):
        J = c.jacobian(x, export=True, fd=fd)
        return [J.indptr, J.indices, J.data]

    def assemblies():
        return ctx.matfree_info()["value_assemblies"]
    step("analytic", exported)
    step("forward differences", lambda c: exported(c, fd=True))
    step("analytic again", exported)
    # matrix-free: the Jacobi solve needs no values, the ILU(0) solve exactly one assembly of them
    mf = [(P.OPT_MATRIX_FREE, 1)]
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    va0 = assemblies()
    ctx.jacobian(x, export=False)
    step("matrix-free, Jacobi", lambda c: solve(c, r, P.PREC_JACOBI), mf, jac=True)
    assert assemblies() == va0
    step("matrix-free, ILU(0)", lambda c: solve(c, r, P.PREC_ILU0), mf, jac=True)
    assert assemblies() == va0 + 1
    ctx.set_option(P.OPT_MATRIX_FREE, 0)  # the Jacobian goes on as an assembled one
    step("matrix-free off", lambda c: solve(c, r, P.PREC_SSOR) + [c.jacobian_export().data],
         jac=True)
    assert assemblies() == va0 + 1
    ctx.set_option(P.OPT_SEQ_ORDER, 1)
    expect_no_jacobian(ctx, r)
    step("reference order", lambda c: exported(c) + solve(c, r, P.PREC_SSOR_NATURAL),
         [(P.OPT_SEQ_ORDER, 1)])
    ctx.set_option(P.OPT_SEQ_ORDER, 0)
    expect_no_jacobian(ctx, r)
    step("reference order off", lambda c: exported(c) + solve(c, r, P.PREC_ILU0))
    info = ctx.asm_info()
    ctx.close()
    print(f"{name}: asm_info {info}")
    assert (info["full"], info["reused"]) == ASM_COUNTS[name]


# ---- 3. precision changes ------------------------------------------------------------------------
# the factorisation timer's launches (ilu_factor and split count one each) over the sequence,
# recorded from the same parent commit: the first solve factorises; ILU_F32 2 -> 2 changes nothing;
# each change of the precision drops the split copy, which the fused path refactorises (3); setting
# ILU_FUSED_FACTOR drops the factors whatever the value (3), and the three-pass path splits after
# it has factorised (1 more)
FACTOR_LAUNCHES = 8
PRECISION_STEPS = [(None, None), (P.OPT_ILU_F32, 2), (P.OPT_ILU_F32, 0), (P.OPT_ILU_F32, 1),
                   (P.OPT_ILU_F32, 2), (P.OPT_ILU_FUSED_FACTOR, 1), (P.OPT_ILU_FUSED_FACTOR, 0),
                   (P.OPT_ILU_FUSED_FACTOR, 1)]


@pytest.mark.parametrize("name", MESHES)
def test_precision_changes(name):
    _, _, x = operators(name)[0]
    ctx = fresh_ctx(name)
    ctx.timers(enable=True, reset=True)
    ctx.set_operator(P.OP_PNP)
    r = ctx.residual(x)
    ctx.jacobian(x, export=False)
    now = {}
    for opt, val in PRECISION_STEPS:
        if opt is not None:
            ctx.set_option(opt, val)
            now[opt] = val
        ref = fresh_ctx(name)
        for o, v in now.items():
            ref.set_option(o, v)
        ref.set_operator(P.OP_PNP)
        ref.jacobian(x, export=False)
        same(solve(ctx, r, P.PREC_ILU0), solve(ref, r, P.PREC_ILU0), f"{name}: after {opt} = {val}")
        ref.close()
    n = ctx.timers()["factor_launches"]
    ctx.close()
    print(f"{name}: factor launches {n}")
    assert n == FACTOR_LAUNCHES


# ---- 4. the device loop after other use ----------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_md_run_after_the_operator_walk(name):
    mesh, par, dt, _, u0 = problem(name)
    nn = mesh.nv
    u_ref, out_ref, its = yardstick(name, 1, 3, 2, 1, P.PREC_SSOR_NATURAL, P.METHOD_BICGSTAB)
    ctx = fresh_ctx(name)
    walk_operators(ctx, name)
    for reuse in (0, 1):
        u, t, ip, im, res = ctx.md_run(u0, dt, 3, 2, 1, maxit=MAXIT, reuse=reuse)
        assert res["status"] == P.OK and res["linear_iterations"] == its
        assert np.array_equal(u, u_ref)
        assert [o[0] for o in out_ref] == list(t)
        assert np.array_equal(ip, np.array([o[1] for o in out_ref]))
        assert np.array_equal(im, np.array([o[2] for o in out_ref]))
        # the Poisson operator of the last solve is current
        phi = u[:nn]
        got = [ctx.residual(phi)]
        J = ctx.jacobian(phi, export=True)
        ref = fresh_ctx(name)
        ref.set_operator(P.OP_POISSON, cp=u[nn:2 * nn], cm=u[2 * nn:])
        Jr = ref.jacobian(phi, export=True)
        same(got + [J.indptr, J.indices, J.data],
             [ref.residual(phi), Jr.indptr, Jr.indices, Jr.data], f"{name}: after md_run({reuse})")
        ref.close()
    ctx.close()


# ---- 5. two in-process ranks ---------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_operator_changes_two_ranks(name):
    """test_gpu_multirank's comparisons with one rank (sums of the ranks' residuals and Jacobians to
    1e-13 of the maximum, the solve to its reduction, the same iterations and bits on every rank),
    and the long-lived ranks against fresh ranks bit for bit"""
    mesh, par, _, _, _ = problem(name)
    ops = operators(name)[:3]

    def quantities(ctx, args, x):
        ctx.set_operator(**args)
        nf = x.size // mesh.nv
        r = ctx.residual(x)
        J = ctx.jacobian(x)
        rhs = ctx.sync_vector(r, nf)
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=1e-8, maxit=20000)
        return r, J, rhs, ctx.sync_vector(sol, nf), res

    def walk(ctx, rank):
        configure(ctx)
        return [quantities(ctx, args, x) for _, args, x in ops]
    walked = run_ranks(2, mesh, par, walk)
    for k, (label, args, x) in enumerate(ops):
        def one(ctx, rank):
            configure(ctx)
            return quantities(ctx, args, x)
        fresh = run_ranks(2, mesh, par, one)
        ctx1 = fresh_ctx(name)
        ctx1.set_operator(**args)
        r1, J1 = ctx1.residual(x), ctx1.jacobian(x)
        ctx1.close()
        outs = [w[k] for w in walked]
        r, J, rhs = sum(o[0] for o in outs), sum(o[1] for o in outs), outs[0][2]
        assert np.max(np.abs(r - r1)) <= 1e-13 * np.max(np.abs(r1))
        assert abs(J - J1).max() <= 1e-13 * abs(J1).max()
        for (_, _, _, sol, res), f in zip(outs, fresh):
            assert res["converged"] == 1, (label, res)
            assert np.linalg.norm(J @ sol - rhs) <= 1.001e-8 * np.linalg.norm(rhs)
            assert res["iterations"] == f[4]["iterations"]
            same([outs[0][0], sol], [fresh[0][0], f[3]], f"{name}, two ranks, {label}")
        assert len({o[4]["iterations"] for o in outs}) == 1
        assert np.array_equal(outs[0][3], outs[1][3])
        for o, f in zip(outs, fresh):
            same([o[0], o[1].data, o[2]], [f[0], f[1].data, f[2]], f"{name}, two ranks, {label}")
