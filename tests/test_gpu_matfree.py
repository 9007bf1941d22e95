"""Matrix-free Jacobian application (OPT_MATRIX_FREE, jac_apply.hip) on the GPU (-m gpu).

With the option on, the operator application inside the Krylov methods and in jacobian_apply is
computed from the linearisation point by the assembly's fan walk, and the SELL values are assembled
only when something reads them.  The oracle's analytic matrix Jo is the reference throughout.

Bounds.  An application: max|y - Jo z| <= 1e-12 max_i (|Jo| |z|)_i -- the project's Jacobian
tolerance (1e-12 of the scale, tests/test_gpu.py) carried to the product: every entry within
1e-12 |Jo| gives exactly this row bound.  Solves: the bounds of the assembled path's tests."""
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import meshio
import oracle_py as O
import pnp_amd as P
from test_gpu import golden, set_ops
from test_gpu_fans import SURF, wheel

pytestmark = pytest.mark.gpu
_grp = itertools.count()


def run_ranks(nranks, mesh, par, fn):
    """fn(ctx, rank) on nranks in-process ranks (one local group, one host thread each), as
    test_gpu_multirank.run_ranks"""
    name = f"mf{next(_grp)}"

    def work(r):
        ctx = P.Context(mesh, par, device=0, rank=r, size=nranks, local_group=name)
        try:
            return fn(ctx, r)
        finally:
            ctx.close()
    with ThreadPoolExecutor(nranks) as ex:
        return list(ex.map(work, range(nranks)))


def mf_context(name, kind):
    z, mesh, par, orc = golden(name)
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    op = set_ops(z, ctx, orc, kind)
    return z, mesh, orc, ctx, op


def random_z(n, seed):
    """non-zero everywhere, constrained DOFs included"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)


def apply_error(y, Jo, z):
    """max|y - Jo z| in units of the row bound 1e-12 max_i (|Jo| |z|)_i"""
    return float(np.max(np.abs(y - Jo @ z)) / (1e-12 * np.max(abs(Jo) @ np.abs(z))))


def constrained_rows(op):
    """the Dirichlet rows of the oracle's operator (its mask)"""
    return np.nonzero(op._keep[1])[0]


# ---- 1. application parity, every operator -----------------------------------------------------
@pytest.mark.parametrize("name,kind", [("pore_small_k0", "pnp"), ("pore_small_k0", "pnp_ie"),
                                       ("pore_small_k0", "pb"), ("pore_small_k0", "diff"),
                                       ("pore_small_k0", "poisson"), ("cylinder_k0", "pnp"),
                                       ("cylinder_k0", "pb"), ("one_wall_k1", "pnp"),
                                       ("one_wall_k1", "pb")])
def test_application_parity(name, kind):
    z, mesh, orc, ctx, op = mf_context(name, kind)
    x = z[kind + "_x"]
    Jo = orc.jacobian(op, x, fd=False)
    v = random_z(x.size, 1)
    y = ctx.jacobian_apply(v, x)
    err = apply_error(y, Jo, v)
    print(f"matrix-free apply {name} {kind}: error / bound {err:.2e}")
    assert err <= 1.0
    rows = constrained_rows(op)
    assert rows.size > 0 or kind != "pnp"
    np.testing.assert_array_equal(y[rows], v[rows])
    info = ctx.matfree_info()
    assert info["applies"] >= 1 and info["value_assemblies"] == 0, info
    ctx.close()


# ---- 2. fan-length variants ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 14])
@pytest.mark.parametrize("kind", ["pnp", "pb"])
def test_high_degree_fans(k, kind):
    xy, tri, bseg, bgroup = wheel(k)
    mesh = P.Mesh(xy, tri, bseg, bgroup)
    par = P.Params([P.Surface(**s) for s in SURF], l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)
    orc = O.Problem(meshio.Mesh(xy, tri, bseg, bgroup), [meshio.Surface(**s) for s in SURF],
                    l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    assert ctx.info()["max_slots"] == k + 1
    nv = mesh.nv
    rng = np.random.default_rng(k)
    if kind == "pnp":
        ctx.set_operator(P.OP_PNP)
        op = orc.operator(O.OP_PNP, flux=orc.flux(), mask=orc.mask(3))
        x = np.concatenate([rng.uniform(-1, 1, nv), 0.06 * rng.uniform(0.5, 1.5, nv),
                            0.06 * rng.uniform(0.5, 1.5, nv)])
    else:
        ctx.set_operator(P.OP_PB)
        op = orc.operator(O.OP_PB, flux=orc.flux(), mask=orc.mask(1))
        x = rng.uniform(-1, 1, nv)
    Jo = orc.jacobian(op, x)
    v = random_z(x.size, 2)
    y = ctx.jacobian_apply(v, x)
    assert apply_error(y, Jo, v) <= 1.0
    rows = constrained_rows(op)
    np.testing.assert_array_equal(y[rows], v[rows])
    assert ctx.matfree_info() == {"applies": 1, "value_assemblies": 0}
    # the diagonal-only walk (Jacobi without SELL values): v = d / diag recovers the diagonal, held
    # to the Jacobian's own tolerance, 1e-12 max|Jo|
    d = random_z(x.size, 3)
    w = ctx.prec_apply(d, P.PREC_JACOBI)
    assert np.max(np.abs(d / w - Jo.diagonal())) <= 1e-12 * abs(Jo).max()
    assert ctx.matfree_info() == {"applies": 1, "value_assemblies": 0}
    ctx.close()


# ---- 3. fused-dot modes and exact counts ---------------------------------------------------------
def diffusion_system(matrix_free):
    """test_gpu.test_bicgstab_half_step_counting_matches_istl's well-conditioned system"""
    z, mesh, par, orc = golden("pore_small_k0")
    nv = mesh.nv
    phi = np.ascontiguousarray(z["diff_phi"])
    xo_ = np.ascontiguousarray(z["pnp_ie_x_old"][nv:2 * nv])
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_MATRIX_FREE, int(matrix_free))
    ctx.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=1e-3, z=1.0, field=1, phi=phi, x_old=xo_)
    op = orc.operator(O.OP_DIFF_IE, flux=orc.flux(),
                      mask=np.ascontiguousarray(orc.mask(3)[nv:2 * nv]), dt=1e-3, z=1.0, phi=phi,
                      x_old=xo_)
    x = xo_.copy()
    ctx.jacobian(x, export=False)
    rhs = ctx.residual(x) + 0.01
    rhs[op._keep[1] == 1] = 0.0
    return ctx, orc, op, x, rhs


@pytest.mark.parametrize("reduction", [1e-3, 1e-6, 1e-9])
def test_bicgstab_counts_match_istl(reduction):
    """BiCGSTAB's fused dots (modes 1 and 2): half-step counter, iteration count and flag equal
    the oracle's, as on the assembled path."""
    ctx, orc, op, x, rhs = diffusion_system(True)
    sol, res = ctx.linear_solve(rhs, prec=P.PREC_NONE, reduction=reduction, maxit=1000,
                                check_every=1)
    xo, ro = O.bicgstab(orc.jacobian(op, x), rhs, prec=O.PREC_NONE, reduction=reduction,
                        maxit=1000)
    assert res["converged"] == ro.converged == 1
    assert res["it_half"] == ro.it_half
    assert res["iterations"] == ro.iterations
    assert np.max(np.abs(sol - xo)) <= 1e-9 * np.max(np.abs(xo))
    info = ctx.matfree_info()
    assert info["applies"] > 0 and info["value_assemblies"] == 0, info
    ctx.close()


def test_two_reduction_bicgstab_counts_match_istl():
    """mode 4 (three fused dots): the two-reduction iteration keeps the counts too"""
    ctx, orc, op, x, rhs = diffusion_system(True)
    ctx.set_option(P.OPT_BICG_TWORED, 1)
    sol, res = ctx.linear_solve(rhs, prec=P.PREC_NONE, reduction=1e-6, maxit=1000, check_every=1)
    xo, ro = O.bicgstab(orc.jacobian(op, x), rhs, prec=O.PREC_NONE, reduction=1e-6, maxit=1000)
    assert res["converged"] == ro.converged == 1
    assert res["it_half"] == ro.it_half and res["iterations"] == ro.iterations
    assert np.max(np.abs(sol - xo)) <= 1e-9 * np.max(np.abs(xo))
    assert ctx.matfree_info()["value_assemblies"] == 0
    ctx.close()


def test_gmres_history_equals_the_assembled_paths():
    """modes 0 and 3 (plain product, residual form): GMRES's history against the assembled path's
    on the same system, 1e-10 relative on the first cycle's estimates (test_gpu_gmres.py's
    tolerance for two histories of one operator), the recomputed last norm to the rounding of
    b - J x as there."""
    hist = {}
    for mf in (0, 1):
        ctx, orc, op, x, rhs = diffusion_system(mf)
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_NONE, reduction=1e-9, maxit=1000,
                                    method=P.METHOD_GMRES)
        assert res["converged"] == 1, res
        hist[mf] = (ctx.solve_history(), res, sol, ctx.matfree_info())
        ctx.close()
    h0, h1 = hist[0][0], hist[1][0]
    assert hist[0][1]["iterations"] == hist[1][1]["iterations"] and h0.size == h1.size
    k = min(30, h0.size - 1)
    assert np.max(np.abs(h1[:k] - h0[:k]) / h0[:k]) <= 1e-10
    Jo = orc.jacobian(op, x)
    R = float(np.linalg.norm(np.abs(rhs) + abs(Jo) @ np.abs(hist[0][2])))
    eps = 2.220446049250313e-16
    assert abs(h1[-1] - h0[-1]) / h0[-1] <= 1e-10 + 4 * eps * R / h0[-1]
    assert np.max(np.abs(hist[1][2] - hist[0][2])) <= 1e-9 * np.max(np.abs(hist[0][2]))
    assert hist[0][3] == {"applies": 0, "value_assemblies": 1}
    assert hist[1][3]["applies"] > 0 and hist[1][3]["value_assemblies"] == 0


@pytest.mark.parametrize("prec", [P.PREC_NONE, P.PREC_JACOBI])
def test_cg_matches_oracle_cg(prec):
    """test_gpu.test_cg_matches_oracle_cg's PB system (CG's fused <p, A p>, and Jacobi on the
    diagonal blocks of a walk of its own): no value assembly."""
    z, mesh, orc, ctx, op = mf_context("pore_small_k0", "pb")
    x = np.zeros(mesh.nv)
    Jo = orc.jacobian(op, x)
    ctx.jacobian(x, export=False)
    rhs = ctx.residual(x)
    sol, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-10, maxit=5000, method=P.METHOD_CG)
    assert res["converged"] == 1, res
    assert np.linalg.norm(Jo @ sol - rhs) <= 1.001e-10 * np.linalg.norm(rhs)
    xo, ro = O.cg(Jo, rhs, prec=O.PREC_JACOBI if prec == P.PREC_JACOBI else O.PREC_NONE,
                  reduction=1e-10, maxit=5000)
    assert ro.converged
    assert abs(res["iterations"] - ro.iterations) <= 1
    assert np.max(np.abs(sol - xo)) <= 1e-8 * np.max(np.abs(xo))
    info = ctx.matfree_info()
    assert info["applies"] > 0 and info["value_assemblies"] == 0, info
    ctx.close()


# ---- 4. linear solves ----------------------------------------------------------------------------
def check_solve(Jo, sol, res, rhs, xo):
    assert res["converged"] == 1, res
    assert np.linalg.norm(Jo @ sol - rhs) <= 1.001e-8 * np.linalg.norm(rhs)
    assert np.max(np.abs(sol - xo)) <= 1e-5 * np.max(np.abs(xo))


def first_newton_system(kind, orc, op, z, mesh):
    x = z["newton_pnp_x0"] if kind == "pnp" else np.zeros(mesh.nv)
    Jo = orc.jacobian(op, x)
    return x, Jo


@pytest.mark.parametrize("kind,prec", [("pnp", P.PREC_NONE), ("pnp", P.PREC_SSOR),
                                       ("pnp", P.PREC_ILU0), ("pb", P.PREC_JACOBI),
                                       ("pb", P.PREC_SSOR), ("pb", P.PREC_ILU0)])
def test_linear_solve(kind, prec):
    """The systems of test_gpu.test_linear_solve_reduces_residual, in its call order
    (jacobian, residual, linear_solve: the residual overwrites the context's state, the
    linearisation point must not move).

    The unpreconditioned PNP case is sensitive to the last bits of the operator application, on
    either path.  Measured on an MI355X, 16 right-hand sides (the system's own and 15 perturbed
    by 1e-14 relative): the assembled path converges 15 times in 803 .. 1,196.5 half steps and
    breaks down once (rho at rounding level, half step 407); the matrix-free path converges 16 of
    16 (773 .. 1,149.5).  The operator itself agrees with the assembled one to 3.3e-16 of each
    row's scale."""
    z, mesh, orc, ctx, op = mf_context("pore_small_k0", kind)
    x, Jo = first_newton_system(kind, orc, op, z, mesh)
    ctx.jacobian(x, export=False)
    rhs = ctx.residual(x)
    sol, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=20000)
    xo, ro = O.bicgstab(Jo, rhs, prec=O.PREC_ILU0, reduction=1e-12, maxit=20000)
    assert ro.converged
    check_solve(Jo, sol, res, rhs, xo)
    info = ctx.matfree_info()
    assert info["applies"] > 0, info
    assert info["value_assemblies"] == (0 if prec in (P.PREC_NONE, P.PREC_JACOBI) else 1), info
    ctx.close()


# ---- 5. stale-state trap -------------------------------------------------------------------------
def test_linearisation_point_survives_a_residual():
    z, mesh, orc, ctx, op = mf_context("pore_small_k0", "pnp")
    x1, x2 = z["pnp_x"], z["newton_pnp_x0"]
    assert np.max(np.abs(x1 - x2)) > 0
    J1, J2 = orc.jacobian(op, x1), orc.jacobian(op, x2)
    v = random_z(x1.size, 5)
    ctx.jacobian(x1, export=False)
    ctx.residual(x2)
    y = ctx.jacobian_apply(v)
    assert apply_error(y, J1, v) <= 1.0
    assert apply_error(y, J2, v) > 1e3  # the two points are told apart
    assert ctx.matfree_info()["value_assemblies"] == 0
    J = ctx.jacobian_export()
    assert abs(J - J1).max() <= 1e-12 * abs(J1).max()
    assert ctx.matfree_info()["value_assemblies"] == 1
    J = ctx.jacobian_export()
    assert abs(J - J1).max() <= 1e-12 * abs(J1).max()
    assert ctx.matfree_info()["value_assemblies"] == 1
    ctx.close()


# ---- 6. Newton -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("cylinder_k0", P.PREC_SSOR), ("pore_small_k0", P.PREC_SSOR),
                                       ("cylinder_k0", P.PREC_ILU0), ("pore_small_k0", P.PREC_ILU0)])
def test_newton_pnp_matches_golden(name, prec):
    z, mesh, par, orc = golden(name)
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    ctx.set_operator(P.OP_PNP)
    u, res = ctx.newton(z["newton_pnp_x0"], prec=prec, linear_maxit=20000)
    assert res["status"] == 0 and res["converged"] == 1, res
    ref = z["newton_pnp_u"]
    assert np.max(np.abs(u - ref)) <= 1e-6 * np.max(np.abs(ref))
    assert res["defect"] <= 1e-9 * res["first_defect"]
    info = ctx.matfree_info()
    assert info["applies"] > 0 and info["value_assemblies"] == res["iterations"], (info, res)
    ctx.close()


@pytest.mark.parametrize("name", ["sphere_k0", "pore_small_k0"])
def test_newton_pb_jacobi_never_assembles(name):
    z, mesh, par, orc = golden(name)
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    ctx.set_operator(P.OP_PB)
    u, res = ctx.newton(np.zeros(mesh.nv), prec=P.PREC_JACOBI)
    assert res["converged"] == 1, res
    ref = z["newton_pb_u"]
    assert np.max(np.abs(u - ref)) <= 1e-6 * max(np.max(np.abs(ref)), 1e-12)
    info = ctx.matfree_info()
    assert info["applies"] > 0 and info["value_assemblies"] == 0, info
    ctx.close()


# ---- 7. partitioned ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_solution():
    """the single-rank assembled solution of the first PNP Newton system (computed once)"""
    z, mesh, par, orc = golden("pore_small_k0")
    x = z["newton_pnp_x0"]
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PNP)
    ctx.jacobian(x, export=False)
    rhs = ctx.residual(x)
    sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=1e-8, maxit=20000)
    assert res["converged"] == 1
    ctx.close()
    return rhs, sol


@pytest.mark.parametrize("nranks", [2, 4])
def test_partitioned(nranks, one_rank_solution):
    """ghost columns and the interior / boundary block subsets of the halo-split application"""
    z, mesh, par, orc = golden("pore_small_k0")
    x = z["newton_pnp_x0"]
    rhs, sol1 = one_rank_solution
    v = random_z(x.size, 7)

    def fn(ctx, r):
        ctx.set_option(P.OPT_MATRIX_FREE, 1)
        ctx.set_operator(P.OP_PNP)
        y = ctx.sync_vector(ctx.jacobian_apply(v, x))
        after_apply = ctx.matfree_info()
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=1e-8, maxit=20000)
        return y, after_apply, ctx.sync_vector(sol), res, ctx.matfree_info()
    outs = run_ranks(nranks, mesh, par, fn)
    op = orc.operator(O.OP_PNP, flux=orc.flux(), mask=orc.mask(3))
    Jo = orc.jacobian(op, x)
    for y, after_apply, sol, res, info in outs:
        assert apply_error(y, Jo, v) <= 1.0
        assert after_apply == {"applies": 1, "value_assemblies": 0}
        assert res["converged"] == 1, res
        assert np.max(np.abs(sol - sol1)) <= 1e-5 * np.max(np.abs(sol1))
        assert info["applies"] > 1 and info["value_assemblies"] == 1, info


# ---- 8. option hygiene ---------------------------------------------------------------------------
def test_option_off_again_is_the_assembled_path_bit_for_bit():
    z, mesh, orc, ctx, op = mf_context("pore_small_k0", "pnp")
    x = z["pnp_x"]
    v = random_z(x.size, 8)
    ctx.jacobian_apply(v, x)
    assert ctx.get_option(P.OPT_MATRIX_FREE) == 1
    ctx.set_option(P.OPT_MATRIX_FREE, 0)
    assert ctx.get_option(P.OPT_MATRIX_FREE) == 0
    # the Jacobian held as a point goes on as an assembled one
    assert ctx.matfree_info() == {"applies": 1, "value_assemblies": 1}
    fresh = P.Context(mesh, ctx.params)
    set_ops(z, fresh, orc, "pnp")
    ref = fresh.jacobian_apply(v, x)
    np.testing.assert_array_equal(ctx.jacobian_apply(v), ref)      # materialised at the point
    np.testing.assert_array_equal(ctx.jacobian_apply(v, x), ref)   # assembled anew
    assert ctx.matfree_info() == {"applies": 1, "value_assemblies": 2}
    assert fresh.matfree_info() == {"applies": 0, "value_assemblies": 1}
    fresh.close()
    ctx.close()


def test_graph_replay_tells_the_two_forms_apart():
    """OPT_GRAPH = 1, the option toggled between solves.  check_every = 8 makes the solver replay
    blocks of 8 iterations as one graph from iteration 8 on (the first block it captures counts
    its launches, a replayed one does not), so a matrix-free solve of at least 24 iterations that
    used graphs counts fewer than two applications per iteration; run eagerly it counts two for
    every iteration launched."""
    z, mesh, par, orc = golden("pore_small_k0")
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_GRAPH, 1)
    op = set_ops(z, ctx, orc, "pnp")
    x, Jo = first_newton_system("pnp", orc, op, z, mesh)
    xo, ro = O.bicgstab(Jo, ctx.residual(x), prec=O.PREC_ILU0, reduction=1e-12, maxit=20000)
    for mf in (1, 0, 1):
        ctx.set_option(P.OPT_MATRIX_FREE, mf)
        before = ctx.matfree_info()["applies"]
        ctx.jacobian(x, export=False)
        rhs = ctx.residual(x)
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_SSOR, reduction=1e-8, maxit=20000,
                                    check_every=8)
        check_solve(Jo, sol, res, rhs, xo)
        applies = ctx.matfree_info()["applies"] - before
        print(f"graph replay, matrix-free {mf}: {res['iterations']} iterations, {applies} applies")
        assert res["iterations"] >= 24, res
        if mf:
            assert 0 < applies < 2 * res["iterations"]  # graphs replayed
        else:
            assert applies == 0
    ctx.close()


def test_graph_replay_across_an_operator_change_with_the_option_off():
    """A graph captured in matrix-free form holds the operator's kind and scalars.  PB and Poisson
    share the field count, the block pattern and the mask buffer, so nothing but the option's own
    change tells their graphs apart: matrix-free solve (captured), option off, another operator,
    option on, solve -- the second solve must be the new operator's.  check_every = 8: iterations
    0 .. 7 run eagerly, the blocks of 8 after them as graphs."""
    z, mesh, par, orc = golden("pore_small_k0")
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_GRAPH, 1)
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    for kind, x in (("pb", np.zeros(mesh.nv)), ("poisson", z["poisson_x"])):
        op = set_ops(z, ctx, orc, kind)
        ctx.set_option(P.OPT_MATRIX_FREE, 1)
        Jo = orc.jacobian(op, x)
        # (turning the option off below assembles the values of the Jacobian it leaves behind)
        assembled = ctx.matfree_info()["value_assemblies"]
        ctx.jacobian(x, export=False)
        rhs = ctx.residual(x)
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_JACOBI, reduction=1e-10, maxit=20000,
                                    check_every=8)
        print(f"graph replay {kind}: {res['iterations']} iterations")
        # not converged at the poll after iteration 8: the block 8 .. 15 ran as a graph
        assert res["converged"] == 1 and res["iterations"] >= 9, res
        assert np.linalg.norm(Jo @ sol - rhs) <= 1.001e-10 * np.linalg.norm(rhs)
        assert ctx.matfree_info()["value_assemblies"] == assembled  # the solve assembled nothing
        ctx.set_option(P.OPT_MATRIX_FREE, 0)
    ctx.close()


def test_pk_contexts_refuse_the_option():
    z, mesh, par, orc = golden("pore_small_k0")
    ctx = P.Context(mesh, par, degree=2)
    with pytest.raises(P.PnpError) as e:
        ctx.set_option(P.OPT_MATRIX_FREE, 1)
    assert e.value.code == P.E_STATE
    assert ctx.get_option(P.OPT_MATRIX_FREE) == 0
    ctx.set_option(P.OPT_MATRIX_FREE, 0)
    ctx.close()


# every PNP_OPT_* with its legal range (include/pnp_capi.h)
OPTION_RANGES = {
    P.OPT_ILU_F32: (0, 3), P.OPT_ILU_FUSED_FACTOR: (0, 1), P.OPT_JAC_FD: (0, 1),
    P.OPT_BICG_TWORED: (-1, 1), P.OPT_AMG_FALLBACK: (0, 1), P.OPT_GRAPH: (-1, 1),
    P.OPT_SEQ_ORDER: (0, 1), P.OPT_ILU_FLOW: (0, 2), P.OPT_NAT_FLOW: (-1, 1),
    P.OPT_ILU_RETRY: (0, 1), P.OPT_GMRES_RESTART: (2, 128), P.OPT_MATRIX_FREE: (0, 1),
    P.OPT_ASM_REUSE_CONST: (0, 1), P.OPT_IDR_S: (1, 8),
}


def test_every_option_round_trips():
    """Every option takes each legal value and reads it back (PNP_OPT_NAT_FLOW too); one below and
    one above the range is E_ARG and leaves the stored value alone; an unknown option is E_ARG."""
    assert sorted(OPTION_RANGES) == list(range(1, 15))
    z, mesh, par, orc = golden("pore_small_k0")
    ctx = P.Context(mesh, par)
    for opt, (lo, hi) in OPTION_RANGES.items():
        default = ctx.get_option(opt)
        assert lo <= default <= hi, (opt, default)
        for v in range(lo, hi + 1):
            ctx.set_option(opt, v)
            assert ctx.get_option(opt) == v, (opt, v)
            for bad in (lo - 1, hi + 1):
                with pytest.raises(P.PnpError) as e:
                    ctx.set_option(opt, bad)
                assert e.value.code == P.E_ARG and " takes " in str(e.value), (opt, bad)
                assert ctx.get_option(opt) == v, (opt, v, bad)
        ctx.set_option(opt, default)
    for call in (lambda: ctx.set_option(15, 0), lambda: ctx.get_option(15)):
        with pytest.raises(P.PnpError) as e:
            call()
        assert e.value.code == P.E_ARG
    ctx.close()


def test_pk_contexts_refuse_p1_only_options():
    """PNP_OPT_SEQ_ORDER = 1 (E_ARG) and PNP_OPT_MATRIX_FREE = 1 (E_STATE) on a P2 context: refused
    with their codes, the options stay 0 and still take 0."""
    z, mesh, par, orc = golden("pore_small_k0")
    ctx = P.Context(mesh, par, degree=2)
    for opt, code in ((P.OPT_SEQ_ORDER, P.E_ARG), (P.OPT_MATRIX_FREE, P.E_STATE)):
        with pytest.raises(P.PnpError) as e:
            ctx.set_option(opt, 1)
        assert e.value.code == code, (opt, e.value)
        assert ctx.get_option(opt) == 0
        ctx.set_option(opt, 0)
    ctx.close()


def test_fd_jacobians_ignore_the_option():
    z, mesh, orc, ctx, op = mf_context("pore_small_k0", "pnp")
    ctx.set_option(P.OPT_JAC_FD, 1)
    x = z["pnp_x"]
    v = random_z(x.size, 9)
    y = ctx.jacobian_apply(v, x)
    assert ctx.matfree_info() == {"applies": 0, "value_assemblies": 1}
    fd = P.Context(mesh, ctx.params)
    set_ops(z, fd, orc, "pnp")
    fd.set_option(P.OPT_JAC_FD, 1)
    np.testing.assert_array_equal(y, fd.jacobian_apply(v, x))
    # the per-call flag too
    ctx.set_option(P.OPT_JAC_FD, 0)
    np.testing.assert_array_equal(ctx.jacobian_apply(v, x, fd=True), y)
    assert ctx.matfree_info()["applies"] == 0
    fd.close()
    ctx.close()
