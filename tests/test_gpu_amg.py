"""GPU tests of the aggregation AMG (PNP_PREC_AMG, the reference's LINEARSOLVER CG_AMG_SSOR,
src/instationary_pnp_from_pb_md.hh:24,207-210).

dune-istl's Amg::AMG is not in the image, so its aggregation heuristics and
iteration counts are "parity unpinned".  What is pinned:
  * the V-cycle itself: one application through the C ABI equals a numpy restatement of the
    same V-cycle (Galerkin products, block-Jacobi, exact coarsest solve) built from the
    exported Jacobian and the exported aggregates, to 1e-10 relative;
  * the solves: CG / BiCGSTAB with the AMG reach the requested reduction on the true system
    (checked with the exported Jacobian) and agree with a direct solve.
"""
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import pnp_amd as P
from amg_ref import interleave, numpy_vcycle
from conftest import DATA

pytestmark = pytest.mark.gpu


def problem(cfgname, k):
    cfg = P.read_config(os.path.join(DATA, cfgname))
    mesh = P.Mesh.load(cfg.meshfile).refine(k)
    par = P.Params.from_config(cfg)
    return mesh, par


@pytest.mark.parametrize("kind,sweeps,pre0", [("pb", 1, 1), ("pb", 2, 1), ("pnp", 1, 1),
                                              ("pnp", 3, 1), ("pnp_ie", 2, 1), ("diff", 2, 1),
                                              ("poisson", 2, 1), ("pnp", 2, 0), ("pb", 2, 0)])
def test_amg_vcycle_matches_numpy_restatement(kind, sweeps, pre0):
    mesh, par = problem("cylinder_config.cfg", 2)
    nv = mesh.nv
    ctx = P.Context(mesh, par)
    rng = np.random.default_rng(7)

    def state3():
        return np.concatenate([rng.uniform(-1, 1, nv), 0.06 * rng.uniform(0.5, 1.5, nv),
                               0.06 * rng.uniform(0.5, 1.5, nv)])
    nf = 3 if kind.startswith("pnp") else 1
    if kind == "pnp":
        ctx.set_operator(P.OP_PNP)
        x = state3()
    elif kind == "pnp_ie":
        ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=0.5, x_old=state3())
        x = state3()
    elif kind == "diff":
        ctx.set_operator(P.OP_DIFF, z=-1.0, field=2, phi=rng.uniform(-1, 1, nv))
        x = 0.06 * rng.uniform(0.5, 1.5, nv)
    elif kind == "poisson":
        ctx.set_operator(P.OP_POISSON, cp=0.06 * rng.uniform(0.5, 1.5, nv),
                         cm=0.06 * rng.uniform(0.5, 1.5, nv))
        x = rng.uniform(-1, 1, nv)
    else:
        ctx.set_operator(P.OP_PB)
        x = rng.uniform(-1, 1, nv)
    J = ctx.jacobian(x)
    ctx.amg_configure(smoother=P.PREC_JACOBI, coarse_target=16, omega=0.8, coarse_sweeps=sweeps,
                      level0_presmooth=pre0)
    d = rng.standard_normal(nf * nv)
    v = ctx.prec_apply(d, P.PREC_AMG)
    info = ctx.amg_info()
    assert info["levels"] >= 3 and info["rows"][-1] <= 16
    aggs = [ctx.amg_aggregates(0)] + [ctx.amg_aggregates(k) for k in range(1, info["levels"] - 1)]
    assert aggs[0].min() >= 0 and aggs[0].max() + 1 == info["rows"][1]
    Ji, perm = interleave(J, nv, nf)
    vn = np.empty_like(d)
    f32 = os.environ.get("PNP_AMG_F32", "1") != "0"
    vn[perm] = numpy_vcycle(Ji, nf, aggs, 0.8, d[perm], sweeps, bool(pre0), f32)
    # f32: the coarsest solve multiplies by the inverse rounded to single precision (the GPU's
    # rocSOLVER inverse and numpy's differ in the last fp64 bits, so a few entries round to the
    # neighbouring float): ~1e-8 of the correction, against the 1e-10 of the fp64 cycle
    assert np.max(np.abs(v - vn)) <= (1e-7 if f32 else 1e-10) * np.max(np.abs(vn))


def test_amg_cg_solves_pb_system():
    """CG_AMG_SSOR: ISTL CGSolver preconditioned by the AMG with the SSOR smoother on the PB
    Jacobian; converges to the reduction far faster than CG_Jacobi, same solution."""
    mesh, par = problem(os.path.join("pore_pnp", "pore.cfg"), 2)
    nv = mesh.nv
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PB)
    x = np.zeros(nv)
    J = ctx.jacobian(x)
    b = ctx.residual(x)
    z, res = ctx.linear_solve(b, prec=P.PREC_AMG, reduction=1e-10, method=P.METHOD_CG,
                              maxit=500)
    assert res["converged"] == 1
    assert np.linalg.norm(J @ z - b) <= 1.01e-10 * np.linalg.norm(b)
    zd = spla.spsolve(J.tocsc(), b)
    assert np.max(np.abs(z - zd)) <= 1e-7 * np.max(np.abs(zd))
    _, rj = ctx.linear_solve(b, prec=P.PREC_JACOBI, reduction=1e-10, method=P.METHOD_CG,
                             maxit=20000)
    assert res["iterations"] * 4 < rj["iterations"]
    info = ctx.amg_info()
    assert info["smoother"] == P.PREC_SSOR and info["levels"] >= 3


@pytest.mark.parametrize("smoother", [P.PREC_ILU0, P.PREC_SSOR])
def test_amg_bicgstab_solves_pnp_system(smoother):
    mesh, par = problem("cylinder_config.cfg", 2)
    nv = mesh.nv
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PNP)
    rng = np.random.default_rng(20261015)
    x = np.concatenate([rng.uniform(-1, 1, nv), 0.06 * rng.uniform(0.5, 1.5, nv),
                        0.06 * rng.uniform(0.5, 1.5, nv)])
    J = ctx.jacobian(x)
    r = ctx.residual(x)
    ctx.amg_configure(smoother=smoother)
    z, res = ctx.linear_solve(r, prec=P.PREC_AMG, reduction=1e-10, maxit=2000)
    assert res["converged"] == 1
    assert np.linalg.norm(J @ z - r) <= 1.01e-10 * np.linalg.norm(r)
    _, ri = ctx.linear_solve(r, prec=smoother, reduction=1e-10, maxit=20000)
    assert res["iterations"] < ri["iterations"]


def test_amg_newton_pnp_matches_ilu0_newton():
    """PNP Newton with AMG-preconditioned BiCGSTAB reaches the same state as with ILU(0)."""
    mesh, par = problem("cylinder_config.cfg", 1)
    nv = mesh.nv
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PB)
    phi, _ = ctx.newton(np.zeros(nv), prec=P.PREC_ILU0)
    x0 = ctx.initial_state(phi)
    ctx.set_operator(P.OP_PNP)
    ctx.amg_configure(smoother=P.PREC_ILU0)
    ua, ra = ctx.newton(x0, prec=P.PREC_AMG, reduction=1e-10)
    ui, ri = ctx.newton(x0, prec=P.PREC_ILU0, reduction=1e-10)
    assert ra["converged"] == 1 and ri["converged"] == 1
    assert ra["linear_fallbacks"] == 0 and ri["linear_fallbacks"] == 0
    assert np.max(np.abs(ua - ui)) <= 1e-6 * np.max(np.abs(ui))


def test_cpp_driver_amg_matches_ilu0(tmp_path):
    """pnp_main --prec amg --pb-prec amg (the C++ driver over the PDELab-shaped adapter) reaches
    the same stationary PNP state as the ILU(0) run."""
    import subprocess
    exe = os.path.join(os.path.dirname(P.LIB_PATH), "pnp_main")
    cfgp = os.path.join(DATA, "cylinder_config.cfg")
    outs = {}
    for prec in ("amg", "ilu0"):
        out = subprocess.run([exe, cfgp, "--refine", "1", "--prec", prec, "--pb-prec", prec,
                              "--out", str(tmp_path / prec)],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[prec] = np.loadtxt(tmp_path / f"{prec}_pnp.dat")
    scale = np.max(np.abs(outs["ilu0"]))
    assert np.max(np.abs(outs["amg"] - outs["ilu0"])) <= 1e-6 * scale


def test_config4_steps_with_amg_need_no_fallback():
    """Config 4's systems (implicit Euler, dt = tau, pore_pnp refined twice) with BiCGSTAB +
    AMG(ILU0) at the default options: 10 steps, every AMG-preconditioned solve converges (the
    smoother fallback, PNP_OPT_AMG_FALLBACK, is off).  Round 1's divergence came from a coarsest
    level of <= 64 blocks: the 215- and 1,928-block levels then only get damped block-Jacobi
    sweeps (spectral radius 1 - 1.7e-7 on their smooth modes) and the preconditioned operator's
    smallest eigenvalue drops from 0.0145 to 0.0057 (tools/amg_c4_analyse.py,
    profiles/r02/amg_c4_analyse.log)."""
    cfg = P.read_config(os.path.join(DATA, "pore_pnp", "pore.cfg"))
    mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(2)
    ctx = P.Context(mesh, P.Params.from_config(cfg))
    assert ctx.get_option(P.OPT_AMG_FALLBACK) == 0
    ctx.set_operator(P.OP_PB)
    phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
    u = ctx.initial_state(phi)
    for i in range(10):
        ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=cfg.system["tau"], x_old=u)
        ctx.amg_configure(smoother=P.PREC_ILU0)
        u, res = ctx.newton(u, reduction=1e-8, abs_limit=1e-9, prec=P.PREC_AMG)
        assert res["converged"] == 1 and res["status"] == 0, (i, res)
        assert res["linear_fallbacks"] == 0


def test_amg_fp64_values_vcycle_child():
    """PNP_AMG_F32=0 (read once per process, so in a child process): the V-cycle with fp64
    coarse-level values and fp64 coarsest inverse matches the fp64 restatement to 1e-10, for a
    PNP and a PB cycle."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import conftest; import test_gpu_amg as T; "
            "T.test_amg_vcycle_matches_numpy_restatement('pnp', 2, 0); "
            "T.test_amg_vcycle_matches_numpy_restatement('pb', 2, 1); print('CHILD OK')" % here)
    env = dict(os.environ, PNP_AMG_F32="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=240, cwd=here)
    assert p.returncode == 0 and "CHILD OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
