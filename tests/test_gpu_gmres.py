"""GPU tests (-m gpu) of restarted GMRES / flexible GMRES (PNP_METHOD_GMRES, PNP_METHOD_FGMRES).

GMRES's residual history is mathematically unique, so it is pinned step by step against the numpy
yardstick (tests/gmres_ref.py, itself pinned against dense least squares in test_gmres_ref.py)
iterating on the same operator: J = ctx.jacobian(x) and M = the GPU's own preconditioner through
ctx.prec_apply.  Tolerances: 1e-10 relative on the history inside the first restart cycle (the CPU
spread between two orthogonalisation orders is 4e-14; the margin covers the GPU's summation
order), iteration counts equal up to one, solutions against a sparse direct solve to 1e-6 of
max|x|, and |J sol - rhs| <= 1.001 reduction |rhs| for every converged solve.
"""
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gmres_ref
import pnp_amd as P
from conftest import DATA
from test_gpu import golden
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

_CACHE = {}


def system(which):
    """(mesh, par, setup(ctx) -> x) of the named system; setup sets the operator."""
    if which in _CACHE:
        return _CACHE[which]
    if which == "big_pb":
        cfg = P.read_config(os.path.join(DATA, "cylinder_config.cfg"))
        mesh = P.Mesh.read_gmsh(os.path.join(DATA, "cylinder.msh")).refine(2)
        par = P.Params.from_config(cfg)
        out = (mesh, par, lambda ctx: (ctx.set_operator(P.OP_PB), np.zeros(mesh.nv))[1], None)
    else:
        name, kind = which.split(":")
        z, mesh, par, orc = golden(name)
        nv = mesh.nv
        if kind == "pb":
            def setup(ctx):
                ctx.set_operator(P.OP_PB)
                return np.zeros(nv)
        elif kind == "diff_ie":
            phi = np.ascontiguousarray(z["diff_phi"])
            xo = np.ascontiguousarray(z["pnp_ie_x_old"][nv:2 * nv])

            def setup(ctx):
                ctx.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=1e-3, z=1.0, field=1, phi=phi,
                                 x_old=xo)
                return xo.copy()
        else:
            x = np.ascontiguousarray(z["newton_pnp_x0"] if name == "pore_small_k0" else z["pnp_x"])

            def setup(ctx):
                ctx.set_operator(P.OP_PNP)
                return x
        out = (mesh, par, setup, z)
    _CACHE[which] = out
    return out


def assembled(which):
    """Context with the system's Jacobian assembled, J (scipy), rhs."""
    mesh, par, setup, _ = system(which)
    ctx = P.Context(mesh, par)
    x = setup(ctx)
    J = ctx.jacobian(x).tocsr()
    rhs = ctx.residual(x)
    if which.endswith("diff_ie"):  # as test_gpu's half-step test: a right-hand side of full support
        rhs = rhs + 0.01
    return ctx, J, rhs


def reference(ctx, J, rhs, prec, restart, reductions, maxit, flexible=False):
    """The yardstick's solve on the GPU's own operator; the first reduction whose stopping step is
    clear of the threshold by more than 1e-6 relative (so that rounding cannot move the count)."""
    M = None if prec == P.PREC_NONE else (lambda d: ctx.prec_apply(d, prec))
    for red in reductions:
        ref = gmres_ref.gmres(J, rhs, M=M, restart=restart, reduction=red, maxit=maxit,
                              flexible=flexible)
        thr = red * ref.history[0]
        h = ref.history
        if not ref.converged or all(abs(v - thr) > 1e-6 * thr for v in h[-2:]):
            return red, ref
    raise AssertionError("no reduction clear of the threshold")


def check2(J, sol, rhs, reduction):
    assert np.linalg.norm(J @ sol - rhs) <= 1.001 * reduction * np.linalg.norm(rhs)


def first_cycle_error(hist, ref, restart):
    """Worst relative difference of |r0| and the Givens estimates inside the first cycle.  The
    entries that are recomputed true norms (the restart boundary, the last entry) carry the
    rounding of b - A x itself -- an absolute error of the order eps |A| |x|, 1e-8 relative at a
    residual of 1e-8 |b| -- and are compared by recomputed_error."""
    k = min(restart, hist.size - 1, ref.size - 1)  # entries 0 .. k - 1: none of them recomputed
    return float(np.max(np.abs(hist[:k] - ref[:k]) / ref[:k]))


EPS = 2.220446049250313e-16


def rscale(J, rhs, x):
    """| |b| + |J| |x| |_2: the scale of the rounding error of a computed residual b - J x, whose
    entries each carry an error of the order eps (|b| + |J| |x|)_i."""
    return float(np.linalg.norm(np.abs(rhs) + abs(J) @ np.abs(x)))


def history_ratios(hist, ref, restart, R, resolution=None):
    """Two histories of the same operator, compared entry by entry; returns the worst
    error / tolerance of (the first cycle's estimates, later cycles' estimates, recomputed norms).
    * first cycle, Givens estimates: 1e-10 relative (the issue's bound).
    * a recomputed true norm |b - J x| (every restart boundary, the last entry): each of the two
      carries the rounding of the residual itself, an absolute error of the order eps R (R =
      rscale), and as much again from the rounding of x: 1e-10 + 4 eps R / norm, relative.
    * estimates of a later cycle, each relative to its own cycle's start: the cycle's start vector
      r / |r| is the recomputed residual, perturbed relatively by the same 4 eps R / |r|, which
      enters every estimate of that cycle: 1e-10 + 4 eps R / (the cycle's start norm).  That is
      first order with constant one, which holds between two runs of the GPU solver on the same
      vectors (FGMRES against GMRES, restart lengths).  Against the numpy yardstick the
      perturbation is amplified along the cycle as in the first cycle (a 1-ulp change of the
      right-hand side moves step 20 by 1e-14 .. 1e-9 depending on the system), so there
      `resolution` adds ten times the yardstick's own measured change at that entry under a 1-ulp
      relative perturbation of the right-hand side (yardstick_resolution)."""
    n = min(hist.size, ref.size)
    last = n - 1 if hist.size == ref.size else -1
    worst = [0.0, 0.0, 0.0]
    for k in range(n):
        c0 = (k // restart) * restart
        if k > 0 and (k % restart == 0 or k == last):
            cls, err = 2, abs(hist[k] - ref[k]) / ref[k]
            tol = 1e-10 + 4 * EPS * R / ref[k]
        elif c0 == 0:
            cls, err, tol = 0, abs(hist[k] - ref[k]) / ref[k], 1e-10
        else:
            cls, err = 1, abs(hist[k] / hist[c0] - ref[k] / ref[c0]) / (ref[k] / ref[c0])
            tol = 1e-10 + 4 * EPS * R / ref[c0]
            if resolution is not None:
                tol += 10 * resolution[k]
        worst[cls] = max(worst[cls], err / tol)
    return worst


def yardstick_resolution(J, rhs, ref, **kw):
    """Relative change of the yardstick's history under a 1-ulp relative perturbation of the
    right-hand side (entries both runs have; zero beyond)."""
    rng = np.random.default_rng(7)
    other = gmres_ref.gmres(J, rhs * (1 + EPS * rng.standard_normal(rhs.size)), **kw).history
    out = np.zeros(ref.size)
    n = min(ref.size, other.size)
    out[:n] = np.abs(other[:n] - ref[:n]) / ref[:n]
    return out


PARITY = [("pore_small_k0:pb", P.PREC_NONE), ("pore_small_k0:pb", P.PREC_JACOBI),
          ("pore_small_k0:pb", P.PREC_SSOR), ("pore_small_k0:pb", P.PREC_ILU0),
          ("pore_small_k0:diff_ie", P.PREC_NONE),
          ("pore_small_k0:pnp", P.PREC_SSOR), ("pore_small_k0:pnp", P.PREC_ILU0),
          ("cylinder_k0:pnp", P.PREC_NONE), ("cylinder_k0:pnp", P.PREC_ILU0),
          ("big_pb", P.PREC_NONE), ("big_pb", P.PREC_ILU0)]


@pytest.mark.parametrize("which,prec", PARITY)
def test_history_parity(which, prec):
    """A context at its default options, J = ctx.jacobian(x), M = ctx.prec_apply (the in-solve
    application applies the same stored factors: measured equal to 2e-16; only PNP_OPT_ILU_F32 = 3
    makes the two differ).  First-cycle history error measured on an MI355X: 1.1e-15 .. 4.3e-14 in
    ten cases, 2.6e-13 for pore_small_k0 PNP with ILU(0) (steps 7 .. 9: above 1e-12 because the
    history is that sensitive there -- the GPU's own history moves by 7.8e-13 at those steps under
    a 1-ulp relative change of the right-hand side).  With fp64 ILU(0) factors that case is more
    sensitive still: test_history_parity_fp64_ilu0_within_the_yardsticks_resolution."""
    ctx, J, rhs = assembled(which)
    red, ref = reference(ctx, J, rhs, prec, 30, [1e-8, 3e-9, 1e-9], 3000)
    sol, res = ctx.linear_solve(rhs, prec=prec, reduction=red, maxit=3000, method=P.METHOD_GMRES)
    hist = ctx.solve_history()
    err = first_cycle_error(hist, ref.history, 30)
    print(f"gmres parity {which} prec {prec}: it {res['iterations']} / ref {ref.iterations}, "
          f"first-cycle history error {err:.2e}")
    assert res["converged"] == 1 and ref.converged, res
    assert hist.size == res["iterations"] + 1 and hist[0] == res["defect0"]
    assert hist[-1] == res["defect"]
    assert err <= 1e-10
    M = None if prec == P.PREC_NONE else (lambda d: ctx.prec_apply(d, prec))
    resol = yardstick_resolution(J, rhs, ref.history, M=M, restart=30, reduction=red, maxit=3000)
    ratios = history_ratios(hist, ref.history, 30, rscale(J, rhs, sol), resol)
    print(f"  error / tolerance: first cycle {ratios[0]:.2e}, later cycles {ratios[1]:.2e}, "
          f"recomputed norms {ratios[2]:.2e}")
    assert max(ratios) <= 1.0
    assert abs(res["iterations"] - ref.iterations) <= 1
    direct = spla.spsolve(J.tocsc(), rhs)
    assert np.max(np.abs(sol - direct)) <= 1e-6 * np.max(np.abs(direct))
    check2(J, sol, rhs, red)
    ctx.close()


def test_history_parity_fp64_ilu0_within_the_yardsticks_resolution():
    """pore_small_k0 PNP with fp64 ILU(0) factors (PNP_OPT_ILU_F32 = 0): A M^-1 is far from normal
    and the history around steps 16 and 17 is not determined to 1e-10 in double precision.  Measured
    on an MI355X: GPU against yardstick 1.06e-9 there (below 1e-11 before step 13 and after step
    21); under a 1-ulp relative change of the right-hand side the yardstick's own history moves
    by 9.9e-9 and the GPU's by 5.3e-9; the yardstick's two orthogonalisation orders differ by
    1.7e-10.  So each step is held to 1e-10 plus ten times the yardstick's own resolution at that
    step: the largest change of its history over four 1-ulp perturbations of the right-hand side
    and the change of orthogonalisation order; ten times, because five samples underestimate the
    spread and a solve rounds at every one of its steps, not once at the right-hand side.  Where
    the history is well determined (before step 10) that is still 1e-10 to within a few percent.
    Counts and solution as in test_history_parity, at reduction 1e-10: at 1e-8 this system's
    conditioning leaves the solution 1.05e-6 of max|x| from the direct solve."""
    ctx, J, rhs = assembled("pore_small_k0:pnp")
    ctx.set_option(P.OPT_ILU_F32, 0)
    M = lambda d: ctx.prec_apply(d, P.PREC_ILU0)  # noqa: E731
    ref = gmres_ref.gmres(J, rhs, M=M, restart=30, reduction=1e-10, maxit=3000)
    rng = np.random.default_rng(7)
    others = [gmres_ref.gmres(J, rhs, M=M, restart=30, reduction=1e-10, maxit=3000, mgs=True)]
    for _ in range(4):
        pert = rhs * (1 + EPS * rng.standard_normal(rhs.size))
        others.append(gmres_ref.gmres(J, pert, M=M, restart=30, reduction=1e-10, maxit=3000))
    k = 30
    resolution = np.max([np.abs(o.history[:k] - ref.history[:k]) / ref.history[:k]
                         for o in others], axis=0)
    sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=1e-10, maxit=3000,
                                method=P.METHOD_GMRES)
    hist = ctx.solve_history()
    err = np.abs(hist[:k] - ref.history[:k]) / ref.history[:k]
    print(f"gmres parity fp64 ILU(0): worst error {err.max():.2e} at step {int(err.argmax())}, "
          f"yardstick resolution there {resolution[int(err.argmax())]:.2e}, worst error / "
          f"tolerance {np.max(err / (1e-10 + 10 * resolution)):.2e}")
    assert res["converged"] == 1 and ref.converged
    assert abs(res["iterations"] - ref.iterations) <= 1
    assert np.all(err <= 1e-10 + 10 * resolution)
    direct = spla.spsolve(J.tocsc(), rhs)
    assert np.max(np.abs(sol - direct)) <= 1e-6 * np.max(np.abs(direct))
    check2(J, sol, rhs, 1e-10)
    ctx.close()


@pytest.mark.parametrize("restart", [2, 5, 7, 30, 33, 128])
def test_restart_lengths(restart):
    """PB system, maxit small enough to force at least two restarts where m allows (the system
    converges in ~95 unpreconditioned steps, so m = 128 is one cycle)."""
    ctx, J, rhs = assembled("pore_small_k0:pb")
    ctx.set_option(P.OPT_GMRES_RESTART, restart)
    assert ctx.get_option(P.OPT_GMRES_RESTART) == restart
    maxit = 2 * restart + 3 if restart < 64 else 3000
    ref = gmres_ref.gmres(J, rhs, restart=restart, reduction=1e-8, maxit=maxit)
    sol, res = ctx.linear_solve(rhs, reduction=1e-8, maxit=maxit, method=P.METHOD_GMRES)
    hist = ctx.solve_history()
    assert abs(res["iterations"] - ref.iterations) <= 1
    assert res["converged"] == int(ref.converged)
    assert hist.size == res["iterations"] + 1
    if not ref.converged:
        assert res["iterations"] == maxit
    err = first_cycle_error(hist, ref.history, restart)
    ratios = history_ratios(hist, ref.history, restart, rscale(J, rhs, ref.x))
    print(f"gmres restart {restart}: first-cycle error {err:.2e}; error / tolerance: first cycle "
          f"{ratios[0]:.2e}, later cycles {ratios[1]:.2e}, recomputed norms {ratios[2]:.2e}")
    assert err <= 1e-10
    assert max(ratios) <= 1.0
    assert np.max(np.abs(sol - ref.x)) <= 1e-6 * np.max(np.abs(ref.x))
    ctx.close()


@pytest.mark.parametrize("reduction", [1e-8, 1e-10])
@pytest.mark.parametrize("which,prec", [("pore_small_k0:pb", P.PREC_NONE),
                                        ("pore_small_k0:pb", P.PREC_SSOR),
                                        ("pore_small_k0:pnp", P.PREC_ILU0),
                                        ("cylinder_k0:pnp", P.PREC_SSOR),
                                        ("big_pb", P.PREC_JACOBI)])
def test_converged_solves_meet_the_reduction(which, prec, reduction):
    ctx, J, rhs = assembled(which)
    for method in (P.METHOD_GMRES, P.METHOD_FGMRES):
        sol, res = ctx.linear_solve(rhs, prec=prec, reduction=reduction, maxit=3000, method=method)
        assert res["converged"] == 1 and res["breakdown"] == 0, res
        assert res["defect"] < reduction * res["defect0"]
        check2(J, sol, rhs, reduction)
    ctx.close()


@pytest.mark.parametrize("which,prec", [("pore_small_k0:pnp", P.PREC_SSOR),
                                        ("pore_small_k0:pnp", P.PREC_ILU0),
                                        ("pore_small_k0:pb", P.PREC_ILU0)])
def test_fgmres_equals_gmres_with_a_linear_preconditioner(which, prec):
    ctx, J, rhs = assembled(which)
    ctx.set_option(P.OPT_ILU_F32, 2)
    sg, rg = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=3000, method=P.METHOD_GMRES)
    hg = ctx.solve_history()
    sf, rf = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=3000, method=P.METHOD_FGMRES)
    hf = ctx.solve_history()
    assert rg["converged"] == rf["converged"] == 1
    assert rg["iterations"] == rf["iterations"]
    eh = first_cycle_error(hf, hg, 30)
    ew = float(np.max(np.abs(hg - hf) / hg))
    es = float(np.max(np.abs(sg - sf)) / np.max(np.abs(sg)))
    ratios = history_ratios(hf, hg, 30, rscale(J, rhs, sg))
    print(f"fgmres vs gmres {which} prec {prec}: first-cycle history {eh:.2e}, whole history "
          f"{ew:.2e}, solution {es:.2e}; error / tolerance: first cycle {ratios[0]:.2e}, later "
          f"cycles {ratios[1]:.2e}, recomputed norms {ratios[2]:.2e}")
    # 1e-10 on every Givens estimate (later cycles relative to their own start), the recomputed
    # norms to the rounding of b - J x: history_ratios
    assert eh <= 1e-10
    assert max(ratios) <= 1.0
    assert es <= 1e-9
    ctx.close()


def test_fgmres_with_a_nonlinear_preconditioner():
    """PNP_OPT_ILU_F32 = 3 rounds the forward sweep's intermediate: M differs from application to
    application; the dataflow ILU(0) would run 3 as 2, so it is turned off."""
    ctx, J, rhs = assembled("pore_small_k0:pnp")
    ctx.set_option(P.OPT_ILU_FLOW, 0)
    ctx.set_option(P.OPT_ILU_F32, 3)
    for reduction in (1e-8, 1e-10):
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=reduction, maxit=3000,
                                    method=P.METHOD_FGMRES)
        assert res["converged"] == 1, res
        check2(J, sol, rhs, reduction)
    ctx.close()


@pytest.mark.parametrize("method", [P.METHOD_GMRES, P.METHOD_FGMRES])
@pytest.mark.parametrize("which", ["pore_small_k0:pnp", "cylinder_k0:pnp"])
def test_amg(which, method):
    ctx, J, rhs = assembled(which)
    sol, res = ctx.linear_solve(rhs, prec=P.PREC_AMG, reduction=1e-8, maxit=3000, method=method)
    assert res["converged"] == 1, res
    check2(J, sol, rhs, 1e-8)
    direct = spla.spsolve(J.tocsc(), rhs)
    assert np.max(np.abs(sol - direct)) <= 1e-6 * np.max(np.abs(direct))
    ctx.close()


@pytest.mark.parametrize("name,kind,prec", [("pore_small_k0", "pnp", P.PREC_ILU0),
                                            ("cylinder_k0", "pnp", P.PREC_ILU0),
                                            ("sphere_k0", "pb", P.PREC_SSOR)])
def test_newton_with_gmres(name, kind, prec):
    """The golden Newton solutions (newton_pnp_u / newton_pb_u, as test_gpu's Newton tests) to
    the existing Newton tolerance of 1e-6."""
    z, mesh, par, orc = golden(name)
    ctx = P.Context(mesh, par)
    if kind == "pnp":
        ctx.set_operator(P.OP_PNP)
        u, res = ctx.newton(z["newton_pnp_x0"], prec=prec, method=P.METHOD_GMRES)
        ref = z["newton_pnp_u"]
    else:
        ctx.set_operator(P.OP_PB)
        u, res = ctx.newton(np.zeros(mesh.nv), prec=prec, method=P.METHOD_GMRES)
        ref = z["newton_pb_u"]
    assert res["status"] == 0 and res["converged"] == 1, res
    assert np.max(np.abs(u - ref)) <= 1e-6 * np.max(np.abs(ref))
    its, _ = ctx.newton_history()
    assert its.size == res["iterations"] and np.all(its > 0)
    ctx.close()


def test_device_pointers_and_pk():
    """PNP_DEVICE_PTRS on a P1 context and a P2 context (external-layout device vectors)."""
    from test_gpu_boundary import _Hip

    ctx, J, rhs = assembled("pore_small_k0:pb")
    sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=1e-8, method=P.METHOD_GMRES)
    hip = _Hip()
    bd, zd = hip.h2d(rhs), hip.h2d(np.zeros(rhs.size))
    rd = ctx.linear_solve_dev(bd, zd, prec=P.PREC_ILU0, reduction=1e-8, method=P.METHOD_GMRES)
    assert rd["converged"] == 1 and rd["iterations"] == res["iterations"]
    np.testing.assert_array_equal(hip.d2h(zd, rhs.size, np.float64), sol)
    ctx.close()
    hip.free()
    z, mesh, par, orc = golden("sphere_k0")
    ctx = P.Context(mesh, par, degree=2)
    ctx.set_operator(P.OP_PB)
    x = np.zeros(ctx.nn)
    J = ctx.jacobian(x).tocsr()
    rhs = ctx.residual(x)
    for method in (P.METHOD_GMRES, P.METHOD_FGMRES):
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_SSOR, reduction=1e-8, method=method)
        assert res["converged"] == 1, res
        check2(J, sol, rhs, 1e-8)
    ctx.close()


def test_edges():
    ctx, J, rhs = assembled("pore_small_k0:pb")
    sol, res = ctx.linear_solve(np.zeros_like(rhs), method=P.METHOD_GMRES)
    assert res["converged"] == 1 and res["iterations"] == 0 and not sol.any()
    assert ctx.solve_history().size == 1
    # maxit smaller than needed
    ctx.set_option(P.OPT_GMRES_RESTART, 5)
    sol, res = ctx.linear_solve(rhs, reduction=1e-8, maxit=12, method=P.METHOD_GMRES)
    hist = ctx.solve_history()
    assert res["converged"] == 0 and res["iterations"] == 12 and hist.size == 13
    assert res["breakdown"] == 0
    R = rscale(J, rhs, sol)
    for k in range(1, 13):
        if k % 5 == 0 or k == 12:
            # a recomputed true norm in the place of the estimate: the minimal residual does not
            # grow, the computed one carries the absolute rounding error of b - J x (rscale)
            assert hist[k] <= hist[k - 1] + 4 * EPS * R
        else:
            assert hist[k] <= hist[k - 1]
    # the poll period changes when the host looks, not what the device computes
    ctx.set_option(P.OPT_GMRES_RESTART, 7)
    outs = []
    for ce in (1, 8):
        s, r = ctx.linear_solve(rhs, prec=P.PREC_JACOBI, reduction=1e-8, maxit=3000,
                                check_every=ce, method=P.METHOD_GMRES)
        assert r["converged"] == 1
        outs.append((s, ctx.solve_history()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    # option range
    for bad in (1, 129):
        with pytest.raises(P.PnpError) as ei:
            ctx.set_option(P.OPT_GMRES_RESTART, bad)
        assert ei.value.code == P.E_ARG
    assert ctx.get_option(P.OPT_GMRES_RESTART) == 7
    # no history after another method's solve
    ctx.linear_solve(rhs, prec=P.PREC_SSOR, reduction=1e-8)
    assert ctx.solve_history().size == 0
    # reference-order mode keeps refusing methods it does not know
    ctx.set_option(P.OPT_SEQ_ORDER, 1)
    ctx.jacobian(np.zeros(rhs.size))  # the mode assembles its own matrix
    with pytest.raises(P.PnpError) as ei:
        ctx.linear_solve(rhs, reduction=1e-8, method=P.METHOD_GMRES)
    assert ei.value.code == P.E_ARG
    ctx.close()


def _one_rank_history(which, prec, restart=30):
    ctx, J, rhs = assembled(which)
    ctx.set_option(P.OPT_GMRES_RESTART, restart)
    sol, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=3000, method=P.METHOD_GMRES)
    hist = ctx.solve_history()
    ctx.close()
    return res, hist


@pytest.mark.parametrize("prec", [P.PREC_NONE, P.PREC_JACOBI])
@pytest.mark.parametrize("nranks", [2, 3])
def test_multirank_history_equals_one_rank(nranks, prec):
    """NONE and Jacobi are the same operator on any partition, so the history is the one-rank
    one (ILU(0) / SSOR are block-Jacobi across ranks: another M)."""
    mesh, par, setup, _ = system("pore_small_k0:pb")
    res1, hist1 = _one_rank_history("pore_small_k0:pb", prec)

    def fn(ctx, r):
        x = setup(ctx)
        ctx.jacobian(x)
        rhs = ctx.sync_vector(ctx.residual(x))
        sol, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=3000,
                                    method=P.METHOD_GMRES)
        return res, ctx.solve_history()
    outs = run_ranks(nranks, mesh, par, fn)
    for res, hist in outs:
        assert res["converged"] == 1, res
        assert abs(res["iterations"] - res1["iterations"]) <= 1
        err = first_cycle_error(hist, hist1, 30)
        print(f"gmres {nranks} ranks prec {prec}: first-cycle error vs one rank {err:.2e}")
        assert err <= 1e-10
    np.testing.assert_array_equal(outs[0][1], outs[-1][1])


@pytest.mark.parametrize("method", [P.METHOD_GMRES, P.METHOD_FGMRES])
@pytest.mark.parametrize("nranks", [2, 3])
def test_multirank_pnp_ilu0(nranks, method):
    mesh, par, setup, _ = system("pore_small_k0:pnp")

    def fn(ctx, r):
        x = setup(ctx)
        J = ctx.jacobian(x)
        rhs = ctx.sync_vector(ctx.residual(x))
        sol, res = ctx.linear_solve(rhs, prec=P.PREC_ILU0, reduction=1e-8, maxit=3000,
                                    method=method)
        return ctx.sync_vector(sol), res, J, rhs
    outs = run_ranks(nranks, mesh, par, fn)
    J = sum(o[2] for o in outs)
    for sol, res, _, rhs in outs:
        assert res["converged"] == 1, res
        check2(J, sol, rhs, 1e-8)
    assert len({o[1]["iterations"] for o in outs}) == 1
