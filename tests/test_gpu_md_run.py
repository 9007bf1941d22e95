"""pnp_md_run (-m gpu): the device-resident operator-split loop against the host-driven loop.

The yardstick is `host_loop` below: the driver's md_loop (driver/pnp_main.cc) restated statement
for statement over the binding -- set_operator, residual, jacobian, linear_solve, ion_flux,
sync_vector -- on a second context in the same process.  pnp_md_run launches the same kernels on
the same bits, so every comparison with it is assert_array_equal, with reuse 0 and with reuse 1.
The one bound in this file is the 1e-8 (of the field's / currents' max) against the oracle's loop
with exact solves, that of test_gpu.test_md_driver_matches_oracle_loop.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import meshio
import oracle_py as O
import pnp_amd as P
from conftest import DATA
from test_gpu import _md_oracle, golden
from test_gpu_boundary import _Hip
from test_gpu_fan_walks import problem as fan_problem
from test_gpu_matfree import run_ranks

pytestmark = pytest.mark.gpu

CFG = os.path.join(DATA, "cylinder_config.cfg")
MAXIT = 5000
# the order-3 rule's negative centroid weight makes the P3 matrices indefinite (DESIGN.md 5, quirk
# Q10): BiCGSTAB with SSOR or ILU(0) diverges on them, on the oracle as here
PK_PREC = {1: P.PREC_SSOR, 2: P.PREC_SSOR, 3: P.PREC_NONE}


# ---- problems and their Boltzmann state (PB Newton, then initial_state: the driver's start) ------
@functools.lru_cache(maxsize=None)
def cyl_config():
    cfg = P.read_config(CFG)
    return cfg, P.Mesh.read_gmsh(cfg.meshfile), P.Params.from_config(cfg)


@functools.lru_cache(maxsize=None)
def problem(name, degree=1):
    """(mesh, params, dt, (update freq, output freq), u0); shared and never modified"""
    if name == "cyl":
        cfg, mesh, par = cyl_config()
        s = cfg.system
        dt, freqs = s["tau"], (max(1, s["potentialUpdateFreq"]), max(1, s["outputFreq"]))
    elif name == "pore":
        _, mesh, par, _ = golden("pore_small_k0")
        # the golden carries no time step: one well under the charge relaxation time
        # 1 / (8 pi l_b c0) ~ 0.66, past which the split (phi frozen over a step) oscillates
        dt, freqs = 0.05, (1, 1)
    else:  # a mesh of tests/fan_meshes.py in its mixed boundary variant, from a random state
        mesh, par, _, st, _ = fan_problem(name, "mixed")
        u0 = np.concatenate([st["phi"], st["cp"], st["cm"]])
        u0.setflags(write=False)
        return mesh, par, 0.37, (1, 1), u0
    ctx = P.Context(mesh, par, degree=degree)
    ctx.set_operator(P.OP_PB)
    pbu, res = ctx.newton(np.zeros(ctx.nn), prec=PK_PREC[degree])
    assert res["converged"]
    u0 = ctx.initial_state(pbu)
    ctx.close()
    u0.setflags(write=False)
    return mesh, par, dt, freqs, u0


def host_loop(ctx, u, dt, nsteps, upd, outf, red_d, red_p, prec, method, maxit=MAXIT):
    """driver/pnp_main.cc md_loop over the binding; returns (u, [(t, ip, im)], iterations)"""
    nn = ctx.nn
    phi, cp, cm = (u[k * nn:(k + 1) * nn].copy() for k in range(3))
    a = 1.0 - 0.5 * np.sqrt(2.0)
    its = [0]

    def linear_problem(x, red):
        r = ctx.residual(x)
        ctx.jacobian(x, export=False)
        r = ctx.sync_vector(r, 1)
        z, res = ctx.linear_solve(r, prec=prec, reduction=red, maxit=maxit, method=method)
        assert res["converged"] and not res["breakdown"]
        z = ctx.sync_vector(z, 1)
        its[0] += res["iterations"]
        return x - z

    def poisson(phi):
        ctx.set_operator(P.OP_POISSON, cp=cp, cm=cm)
        return linear_problem(phi, red_p)

    def alexander2(c, z, field):
        u0 = c.copy()
        ctx.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=a * dt, z=z, field=field, phi=phi, x_old=u0)
        u1 = linear_problem(u0.copy(), red_d)
        ctx.set_operator(P.OP_DIFF, z=z, field=field, phi=phi)
        r1 = ctx.sync_vector(ctx.residual(u1), 1)
        r1 = r1 * ((1.0 - a) * dt)
        ctx.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=a * dt, z=z, field=field, phi=phi, x_old=u0,
                         c_extra=r1)
        return linear_problem(u1.copy(), red_d)

    t, out = 0.0, []
    for i in range(nsteps):
        cp = alexander2(cp, +1.0, 1)
        cm = alexander2(cm, -1.0, 2)
        t += dt
        if i % upd == 0:
            phi = poisson(phi)
        if i % outf == 0:
            ip, im = ctx.ion_flux(np.concatenate([phi, cp, cm]))
            out.append((t, ip, im))
    phi = poisson(phi)
    return np.concatenate([phi, cp, cm]), out, its[0]


@functools.lru_cache(maxsize=None)
def yardstick(name, degree, nsteps, upd, outf, prec, method, red_d=1e-5, red_p=1e-10, mf=0,
              idr_s=0, maxit=MAXIT):
    mesh, par, dt, freqs, u0 = problem(name, degree)
    ctx = P.Context(mesh, par, degree=degree)
    if mf:
        ctx.set_option(P.OPT_MATRIX_FREE, 1)
    if idr_s:
        ctx.set_option(P.OPT_IDR_S, idr_s)
    try:
        u, out, its = host_loop(ctx, u0, dt, nsteps, upd or freqs[0], outf or freqs[1], red_d,
                                red_p, prec, method, maxit)
    finally:
        ctx.close()
    u.setflags(write=False)
    return u, out, its


def expect_counters(res, nsteps, upd, reuse, its):
    npois = -(-nsteps // upd) + 1
    assert res["status"] == P.OK and res["steps_done"] == nsteps
    assert res["diffusion_solves"] == 4 * nsteps and res["poisson_solves"] == npois
    n = (2 if reuse else 4) * nsteps + npois
    assert res["assemblies"] == n and res["prec_setups"] == n
    assert res["linear_iterations"] == its


def check_bitwise(name, nsteps, prec=P.PREC_SSOR_NATURAL, method=P.METHOD_BICGSTAB, degree=1,
                  upd=0, outf=0, mf=0, idr_s=0, red_p=1e-10, maxit=MAXIT):
    """pnp_md_run with reuse 0 and 1 against the yardstick, bit for bit, counters included"""
    mesh, par, dt, freqs, u0 = problem(name, degree)
    upd, outf = upd or freqs[0], outf or freqs[1]
    u_ref, out_ref, its = yardstick(name, degree, nsteps, upd, outf, prec, method, mf=mf,
                                    idr_s=idr_s, red_p=red_p, maxit=maxit)
    for reuse in (0, 1):
        ctx = P.Context(mesh, par, degree=degree)
        if mf:
            ctx.set_option(P.OPT_MATRIX_FREE, 1)
        if idr_s:
            ctx.set_option(P.OPT_IDR_S, idr_s)
        va0 = ctx.matfree_info()["value_assemblies"]
        u, t, ip, im, res = ctx.md_run(u0, dt, nsteps, upd, outf, red_poisson=red_p, prec=prec,
                                       method=method, maxit=maxit, reuse=reuse)
        va1 = ctx.matfree_info()["value_assemblies"]
        # the Poisson operator of the final solve is the context's operator
        cp, cm = u[ctx.nn:2 * ctx.nn], u[2 * ctx.nn:]
        r_after = ctx.residual(u[:ctx.nn])
        ctx.set_operator(P.OP_POISSON, cp=cp, cm=cm)
        r_set = ctx.residual(u[:ctx.nn])
        ctx.close()
        np.testing.assert_array_equal(u, u_ref)
        assert res["noutputs"] == len(out_ref) == len(t)
        for k, (tr, ipr, imr) in enumerate(out_ref):
            assert t[k] == tr
            np.testing.assert_array_equal(ip[k], ipr)
            np.testing.assert_array_equal(im[k], imr)
        np.testing.assert_array_equal(r_after, r_set)
        assert res["assemblies"] == va1 - va0
        if not mf:
            expect_counters(res, nsteps, upd, reuse, its)
        else:
            assert res["linear_iterations"] == its and res["steps_done"] == nsteps


# ---- 1. bitwise equality -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cyl", "pore"])
def test_eleven_steps_config_frequencies(name):
    check_bitwise(name, 11)


@pytest.mark.parametrize("name", ["cyl", "pore"])
def test_seven_steps_frozen_potential_and_sparse_outputs(name):
    """update every 3rd step, output every 4th: phi frozen across steps, an output step without a
    Poisson update (i = 4) and the reverse (i = 3, 6)"""
    check_bitwise(name, 7, upd=3, outf=4)


@pytest.mark.parametrize("nsteps", [0, 1])
def test_zero_and_one_step(nsteps):
    check_bitwise("cyl", nsteps)


@pytest.mark.parametrize("prec,method,idr_s", [
    (P.PREC_NONE, P.METHOD_BICGSTAB, 0), (P.PREC_JACOBI, P.METHOD_BICGSTAB, 0),
    (P.PREC_SSOR, P.METHOD_BICGSTAB, 0), (P.PREC_ILU0, P.METHOD_BICGSTAB, 0),
    (P.PREC_AMG, P.METHOD_BICGSTAB, 0), (P.PREC_JACOBI, P.METHOD_CG, 0),
    (P.PREC_SSOR, P.METHOD_IDR, 4)])
def test_methods_and_preconditioners(prec, method, idr_s):
    """(SSOR_NATURAL, the driver's default, is every other test's)"""
    check_bitwise("pore", 3, prec=prec, method=method, idr_s=idr_s)


@pytest.mark.parametrize("degree", [2, 3])
def test_pk(degree):
    """P3: the matrices are indefinite (quirk Q10).  Of BiCGSTAB, GMRES(128) and IDR(4), each
    without a preconditioner and with Jacobi, and GMRES with SSOR and ILU(0), only the
    unpreconditioned IDR(4) brings every solve of the host-driven loop to its reduction here (some
    11,000 iterations a step): one step of it, with a Poisson reduction of 1e-6"""
    if degree == 3:
        check_bitwise("cyl", 1, degree=3, prec=P.PREC_NONE, method=P.METHOD_IDR, red_p=1e-6,
                      maxit=20000)
    else:
        check_bitwise("cyl", 3, degree=2, prec=P.PREC_SSOR)


@pytest.mark.parametrize("name", ["one_triangle", "pinwheel_3_1_2", "diamond_chain_21"])
def test_tiny_and_pinch_meshes(name):
    """fewer rows than a wavefront; a pinch-vertex chain of 64 rows (one full SELL chunk)"""
    check_bitwise(name, 3, prec=P.PREC_SSOR)


def test_matrix_free():
    check_bitwise("pore", 3, prec=P.PREC_JACOBI, mf=1)


def raw_md_run(ctx, uptr, dt, nsteps, nsurf, cap, t, ip, im, flags=0, upd=1, outf=1,
               prec=P.PREC_SSOR_NATURAL, maxit=MAXIT, reuse=1, opts=True, res=True):
    o = P._MdOpts(dt, 0.0, nsteps, upd, outf, 1e-5, 1e-10,
                  P._SolveOpts(prec, 0.0, maxit, 8, P.METHOD_BICGSTAB), reuse)
    r = P._MdResult()
    pt = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = P.lib().pnp_md_run(ctx.h, uptr, C.byref(o) if opts else None, nsurf, cap, pt(t), pt(ip),
                            pt(im), C.byref(r) if res else None, flags)
    return rc, r


def test_cap_zero_and_cap_smaller_than_noutputs():
    mesh, par, dt, freqs, u0 = problem("cyl")
    u_ref, out_ref, _ = yardstick("cyl", 1, 3, 1, 1, P.PREC_SSOR_NATURAL, P.METHOD_BICGSTAB)
    ns = len(par.surfaces)
    ctx = P.Context(mesh, par)
    u = u0.copy()
    rc, r = raw_md_run(ctx, C.c_void_p(u.ctypes.data), dt, 3, ns, 0, None, None, None)
    assert rc == P.OK and r.noutputs == 3 and r.status == P.OK
    np.testing.assert_array_equal(u, u_ref)
    u = u0.copy()
    t, ip, im = np.full(3, -7.0), np.full((3, ns), -7.0), np.full((3, ns), -7.0)
    rc, r = raw_md_run(ctx, C.c_void_p(u.ctypes.data), dt, 3, ns, 2, t, ip, im)
    ctx.close()
    assert rc == P.OK and r.noutputs == 3
    np.testing.assert_array_equal(u, u_ref)
    for k in range(2):
        assert t[k] == out_ref[k][0]
        np.testing.assert_array_equal(ip[k], out_ref[k][1])
        np.testing.assert_array_equal(im[k], out_ref[k][2])
    assert t[2] == -7.0 and np.all(ip[2] == -7.0) and np.all(im[2] == -7.0)


def test_device_pointers():
    mesh, par, dt, freqs, u0 = problem("pore")
    u_ref, out_ref, _ = yardstick("pore", 1, 3, 1, 1, P.PREC_SSOR_NATURAL, P.METHOD_BICGSTAB)
    ctx = P.Context(mesh, par)
    hip = _Hip()
    try:
        ud = hip.h2d(u0)
        _, t, ip, im, res = ctx.md_run(ud, dt, 3, device_ptr=True)
        u = hip.d2h(ud, u0.size, np.float64)
    finally:
        hip.free()
        ctx.close()
    np.testing.assert_array_equal(u, u_ref)
    assert [x[0] for x in out_ref] == list(t)
    np.testing.assert_array_equal(ip, np.array([x[1] for x in out_ref]))
    np.testing.assert_array_equal(im, np.array([x[2] for x in out_ref]))


@pytest.mark.parametrize("nranks", [2, 3])
def test_in_process_ranks(nranks):
    mesh, par, dt, freqs, u0 = problem("pore")
    args = (dt, 3, 1, 1)

    def ref(ctx, r):
        return host_loop(ctx, u0, *args, 1e-5, 1e-10, P.PREC_SSOR, P.METHOD_BICGSTAB)

    def run(reuse):
        def fn(ctx, r):
            u, t, ip, im, res = ctx.md_run(u0, *args, prec=P.PREC_SSOR, maxit=MAXIT, reuse=reuse)
            return ctx.sync_vector(u, 3), t, ip, im, res
        return fn
    refs = run_ranks(nranks, mesh, par, ref)
    for reuse in (0, 1):
        outs = run_ranks(nranks, mesh, par, run(reuse))
        for (u_ref, out_ref, its), (u, t, ip, im, res) in zip(refs, outs):
            np.testing.assert_array_equal(u, u_ref)
            assert [x[0] for x in out_ref] == list(t)
            np.testing.assert_array_equal(ip, np.array([x[1] for x in out_ref]))
            np.testing.assert_array_equal(im, np.array([x[2] for x in out_ref]))
            expect_counters(res, 3, 1, reuse, its)
        np.testing.assert_array_equal(outs[0][0], outs[-1][0])  # global on every rank


# ---- 2. against the oracle's loop with exact solves ----------------------------------------------
def test_matches_oracle_loop():
    cfg, mesh, par = cyl_config()
    _, _, dt, freqs, u0 = problem("cyl")
    s = cfg.system
    orc = O.Problem(meshio.Mesh(mesh.xy, mesh.tri, mesh.bseg, mesh.bgroup), cfg.surfaces,
                    l_b=s["l_b"], c0=s["c0"], tau=s["tau"], cylindrical=s["cylindrical"])
    u_orc, fluxes = _md_oracle(orc, cfg, u0, 11)
    ctx = P.Context(mesh, par)
    u, t, ip, im, res = ctx.md_run(u0, dt, 11, freqs[0], freqs[1], red_diffusion=1e-12,
                                   red_poisson=1e-12, maxit=MAXIT, reuse=1)
    ctx.close()
    assert res["status"] == P.OK and res["steps_done"] == 11
    nv = mesh.nv
    for f in range(3):
        ref = u_orc[f * nv:(f + 1) * nv]
        err = np.max(np.abs(u[f * nv:(f + 1) * nv] - ref))
        print(f"field {f}: max error {err:.3e}, max {np.max(np.abs(ref)):.3e}")
        assert err <= 1e-8 * max(np.max(np.abs(ref)), 1e-30)
    assert len(t) == len(fluxes)
    for k, (tr, (ipr, imr)) in enumerate(fluxes):
        assert t[k] == pytest.approx(tr)
        scale = max(np.max(np.abs(ipr)), np.max(np.abs(imr)), 1e-30)
        assert np.max(np.abs(ip[k] - ipr)) <= 1e-8 * scale
        assert np.max(np.abs(im[k] - imr)) <= 1e-8 * scale


# ---- 3. counters (every bitwise case checks them; here: a frequency that does not divide S) ------
@pytest.mark.parametrize("nsteps,upd", [(5, 2), (4, 4)])
def test_counters(nsteps, upd):
    check_bitwise("cyl", nsteps, upd=upd, outf=2, prec=P.PREC_SSOR)


# ---- 4. failure path -----------------------------------------------------------------------------
def test_unconverged_solve_ends_the_run_and_leaves_the_context_usable():
    mesh, par, dt, freqs, u0 = problem("pore")
    ctx = P.Context(mesh, par)
    u, t, ip, im, res = ctx.md_run(u0, dt, 3, prec=P.PREC_NONE, maxit=1)
    assert res["status"] == P.E_NOT_CONVERGED and res["steps_done"] == 0
    assert res["noutputs"] == 0 and len(t) == 0
    np.testing.assert_array_equal(u, u0)
    fresh = P.Context(mesh, par)
    for c in (ctx, fresh):
        c.set_operator(P.OP_PNP)
    np.testing.assert_array_equal(ctx.residual(u0), fresh.residual(u0))
    ctx.close()
    fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_u_alone():
    mesh, par, dt, freqs, u0 = problem("cyl")
    ns = len(par.surfaces)
    ctx = P.Context(mesh, par)
    u = u0.copy()
    up = C.c_void_p(u.ctypes.data)
    t, ip, im = np.zeros(2), np.zeros((2, ns)), np.zeros((2, ns))
    assert raw_md_run(ctx, up, dt, -1, ns, 0, None, None, None)[0] == P.E_ARG
    assert raw_md_run(ctx, up, 0.0, 1, ns, 0, None, None, None)[0] == P.E_ARG
    assert raw_md_run(ctx, up, -dt, 1, ns, 0, None, None, None)[0] == P.E_ARG
    assert raw_md_run(ctx, None, dt, 1, ns, 0, None, None, None)[0] == P.E_ARG
    assert raw_md_run(ctx, up, dt, 1, ns, 0, None, None, None, opts=False)[0] == P.E_ARG
    assert raw_md_run(ctx, up, dt, 1, ns, 0, None, None, None, res=False)[0] == P.E_ARG
    assert raw_md_run(ctx, up, dt, 1, ns, 2, None, ip, im)[0] == P.E_ARG
    assert raw_md_run(ctx, up, dt, 1, ns, 2, t, None, im)[0] == P.E_ARG
    assert raw_md_run(ctx, up, dt, 1, ns, 2, t, ip, None)[0] == P.E_ARG
    ctx.set_option(P.OPT_SEQ_ORDER, 1)
    assert raw_md_run(ctx, up, dt, 1, ns, 2, t, ip, im)[0] == P.E_STATE
    ctx.set_option(P.OPT_SEQ_ORDER, 0)
    np.testing.assert_array_equal(u, u0)
    # and the same call now runs
    assert raw_md_run(ctx, up, dt, 1, ns, 2, t, ip, im)[0] == P.OK
    ctx.close()
    np.testing.assert_array_equal(
        u, yardstick("cyl", 1, 1, 1, 1, P.PREC_SSOR_NATURAL, P.METHOD_BICGSTAB)[0])


# ---- 6. isolation --------------------------------------------------------------------------------
def test_run_leaks_nothing_into_set_operator():
    """set_operator(PNP) + jacobian + linear_solve before and after a run: bitwise the same (the
    loop's operator data and the constant-planes flag must not survive into pnp_set_operator's
    path)"""
    mesh, par, dt, freqs, u0 = problem("pore")
    ctx = P.Context(mesh, par)

    def sequence():
        ctx.set_operator(P.OP_PNP)
        r = ctx.residual(u0)
        J = ctx.jacobian(u0)
        z, res = ctx.linear_solve(r, prec=P.PREC_ILU0, reduction=1e-8)
        return r, J, z, res["iterations"]
    r1, J1, z1, it1 = sequence()
    _, _, _, _, res = ctx.md_run(u0, dt, 2, reuse=1)
    assert res["status"] == P.OK
    r2, J2, z2, it2 = sequence()
    ctx.close()
    np.testing.assert_array_equal(r2, r1)
    np.testing.assert_array_equal(J2.indptr, J1.indptr)
    np.testing.assert_array_equal(J2.indices, J1.indices)
    np.testing.assert_array_equal(J2.data, J1.data)
    np.testing.assert_array_equal(z2, z1)
    assert it2 == it1


# ---- 7. the driver -------------------------------------------------------------------------------
def test_driver_device_loop_writes_the_host_loop_files(tmp_path):
    exe = os.path.join(os.path.dirname(P.LIB_PATH), "pnp_main")
    runs = {"host": ["--md-loop", "host"], "dev0": ["--md-loop", "device", "--md-reuse", "0"],
            "dev1": ["--md-loop", "device", "--md-reuse", "1"]}
    files = {}
    for key, extra in runs.items():
        pre = str(tmp_path / key)
        out = subprocess.run([exe, CFG, "--mode", "md", "--steps", "11", "--md-reduction", "1e-12",
                              "--out", pre] + extra, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        files[key] = [open(pre + sfx, "rb").read() for sfx in ("_pnp.dat", "_current.dat")]
        assert all(len(b) > 0 for b in files[key])
    assert files["dev0"] == files["host"]
    assert files["dev1"] == files["host"]
