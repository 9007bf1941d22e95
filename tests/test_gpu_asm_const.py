"""The Jacobian assembly that writes the state-independent planes of the PNP k-form (k0, k1) once
per operator (PNP_OPT_ASM_REUSE_CONST = 1, the default; k_assemble_ga<..., KC=1>) against the
assembly that writes every plane on every launch (option 0), -m gpu.

Every case runs the same sequence of context calls with the option at 1 and at 0; the exported
Jacobian values, residuals and Newton iterates must be bitwise the same, and pnp_asm_info's
counters must show that the reuse variant really ran where it may, and a full write where the
stored planes were invalidated (operator change, forward-difference Jacobian).  A stale or
misplaced plane shows in the export: the planes differ between operators and scale with dt.

The reuse variant exists for OP_PNP.  For OP_PNP_IE it was built and measured once: the compiler
then contracts the state-dependent k2 .. k4 differently (3 of 16,384 exported entries of
pore_small_k0 one ulp apart, 7.1e-15 against max |J| = 1,974; k0 / k1 entries and residuals bitwise
the same), which moves implicit-Euler Newton trajectories in their last bits, so PNP_IE keeps
writing every plane: its cases here check the equality with option 0 and that no assembly reuses.
assert_same_jacobian keeps the fallback the comparison was specified with (k0 / k1 entries bitwise,
the rest within 1e-12 of max |J|); nothing takes it today.

The goldens are small (a few hundred to a few thousand rows) with open and closed fans, Dirichlet
rows, a last chunk and a last 256-row block that are not full; none of their rows has a fan break
(the reuse walk on pinch vertices: tests/test_gpu_fan_walks.py).  The walk behind
the variant (direct gathers or LDS-staged) is chosen once per process, so the reuse and cold-hint
case also runs in child processes with PNP_ASM_LDS = 1 and 0, as test_gpu_asm_lds.py does."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_amd as P
from test_gpu import golden, set_ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("pore_small_k0", "cylinder_k0")


def kinds_of(name):
    return ("pnp", "pnp_ie") if name == "pore_small_k0" else ("pnp",)


def second_state(x):
    """Another state of the same size: every dof moved by a few per cent, deterministically."""
    k = np.arange(x.size, dtype=np.float64)
    return x * (1.0 + 0.05 * np.cos(0.37 * k)) + 1e-3 * np.sin(0.11 * k)


def new_ctx(mesh, par, opt, matrix_free=False):
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_ASM_REUSE_CONST, opt)
    assert ctx.get_option(P.OPT_ASM_REUSE_CONST) == opt
    if matrix_free:
        ctx.set_option(P.OPT_MATRIX_FREE, 1)
    return ctx


def counts(ctx):
    i = ctx.asm_info()
    return [i["full"], i["reused"]]


def case_second_state(opt):
    """Cases 1 and 2: full write at x1, reuse at x2, a linear solve, reuse by the cold-hint walk."""
    out = {}
    for name in NAMES:
        z, mesh, par, orc = golden(name)
        for kind in kinds_of(name):
            ctx = new_ctx(mesh, par, opt)
            set_ops(z, ctx, orc, kind)
            x1 = z[kind + "_x"]
            x2 = second_state(x1)
            J1 = ctx.jacobian(x1)
            c1 = counts(ctx)
            J2 = ctx.jacobian(x2)
            c2 = counts(ctx)
            r2 = ctx.residual(x2)  # a residual-only launch neither sets nor clears the planes
            sol, res = ctx.linear_solve(r2, prec=P.PREC_ILU0, reduction=1e-10, maxit=20000)
            J3 = ctx.jacobian(x1)  # follows a solve: the cold hint is set
            assert res["converged"] == 1, res
            out[f"{name}/{kind}"] = {"jac": [J1, J2, J3], "arrays": [r2],
                                     "counts": [c1, c2, counts(ctx)]}
            ctx.close()
    return out


def case_invalidation(opt):
    """Cases 3 and 4: another operator in between, a forward-difference Jacobian in between."""
    out = {}
    for name in NAMES:
        z, mesh, par, orc = golden(name)
        x1 = z["pnp_x"]
        x2 = second_state(x1)
        ctx = new_ctx(mesh, par, opt)
        set_ops(z, ctx, orc, "pnp")
        ctx.jacobian(x1, export=False)
        set_ops(z, ctx, orc, "pb")
        Jpb = ctx.jacobian(z["pb_x"])
        set_ops(z, ctx, orc, "pnp")
        before = counts(ctx)
        J = ctx.jacobian(x2)
        out[f"{name}/operator"] = {"jac": [Jpb, J], "counts": [before, counts(ctx)]}
        ctx.close()

        ctx = new_ctx(mesh, par, opt)
        set_ops(z, ctx, orc, "pnp")
        ctx.jacobian(x1, export=False)
        Jfd = ctx.jacobian(x1, fd=True)
        before = counts(ctx)
        J = ctx.jacobian(x2)
        mid = counts(ctx)
        Jr = ctx.jacobian(x1)  # the planes are valid again after that full write
        out[f"{name}/fd"] = {"jac": [Jfd, J, Jr], "counts": [before, mid, counts(ctx)]}
        ctx.close()
    return out


def case_implicit_euler(opt):
    """Cases 5 and 6: PnpTOperator with another dt (full write), and with the same dt and a new
    x_old (the time-step pattern), directly and over two Newton-solved time steps."""
    out = {}
    z, mesh, par, orc = golden("pore_small_k0")
    tau = float(z["params"][2])
    x = z["pnp_ie_x"]
    xo = z["pnp_ie_x_old"]
    ctx = new_ctx(mesh, par, opt)
    ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=tau, x_old=xo)
    Ja = ctx.jacobian(x)
    ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=2 * tau, x_old=xo)
    before = counts(ctx)
    Jb = ctx.jacobian(x)
    out["dt_change"] = {"jac": [Ja, Jb], "arrays": [ctx.residual(x)],
                        "counts": [before, counts(ctx)]}
    ctx.close()

    ctx = new_ctx(mesh, par, opt)
    ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=tau, x_old=xo)
    Ja = ctx.jacobian(x)
    xo2 = second_state(xo)
    x2 = second_state(x)
    ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=tau, x_old=xo2)
    before = counts(ctx)
    r = ctx.residual(x2)
    Jb = ctx.jacobian(x2)
    out["same_dt"] = {"jac": [Ja, Jb], "arrays": [r], "counts": [before, counts(ctx)]}
    ctx.close()

    # two implicit-Euler steps, each a Newton solve (its right-hand sides are the residuals of the
    # fused launches): test_gpu.py's test_implicit_euler_step_matches_oracle, twice
    ctx = new_ctx(mesh, par, opt)
    u = z["newton_pnp_x0"]
    arrays, ints = [], []
    for _ in range(2):
        ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=1.0, x_old=u)
        u, res = ctx.newton(u, prec=P.PREC_SSOR, reduction=1e-10)
        assert res["converged"] == 1, res
        arrays.append(u)
        ints += [res["iterations"], res["linear_iterations"]]
    out["time_steps"] = {"iterates": arrays, "steps": ints, "counts": [counts(ctx)]}
    ctx.close()
    return out


def case_matrix_free(opt):
    """Case 7: the values of a matrix-free Jacobian, materialised by the export (ensure_values)."""
    out = {}
    for name in NAMES:
        z, mesh, par, orc = golden(name)
        for kind in kinds_of(name):
            ctx = new_ctx(mesh, par, opt, matrix_free=True)
            set_ops(z, ctx, orc, kind)
            x1 = z[kind + "_x"]
            J1 = ctx.jacobian(x1)
            c1 = counts(ctx)
            J2 = ctx.jacobian(second_state(x1))
            out[f"{name}/{kind}"] = {"jac": [J1, J2], "counts": [c1, counts(ctx)]}
            ctx.close()
    return out


def case_newton(opt):
    """Case 8: a PNP Newton solve from the golden start."""
    out = {}
    for name in NAMES:
        z, mesh, par, orc = golden(name)
        ctx = new_ctx(mesh, par, opt)
        ctx.set_operator(P.OP_PNP)
        u, res = ctx.newton(z["newton_pnp_x0"], prec=P.PREC_ILU0, linear_maxit=20000)
        assert res["status"] == 0 and res["converged"] == 1, res
        out[name] = {"arrays": [u], "ints": [res["iterations"], res["linear_iterations"]],
                     "counts": [counts(ctx)]}
        ctx.close()
    return out


CASES = {"second_state": case_second_state, "invalidation": case_invalidation,
         "implicit_euler": case_implicit_euler, "matrix_free": case_matrix_free,
         "newton": case_newton}


@functools.lru_cache(maxsize=None)
def both(case):
    """The case with the option at 1 and at 0 (computed once, shared by the tests)."""
    return CASES[case](1), CASES[case](0)


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


NOT_BITWISE = []  # (case key, index): Jacobians that fell back to the parity bound


def assert_same_jacobian(key, k, A, B):
    """Bitwise the same values; failing that (the compiler contracting k2 .. k4 differently in the
    reuse instantiation) the entries made of k0 / k1 alone -- the potential's rows, (phi, phi) = k0
    and (phi, c+-) = +-k1 of every block (kernels.h expand_k): the first nv rows of the export --
    bitwise, and the rest within the project's parity bound, 1e-12 of max |J| (test_gpu.py)."""
    assert A.shape == B.shape and sha(A.indptr) == sha(B.indptr) and sha(A.indices) == sha(B.indices)
    if sha(A.data) == sha(B.data):
        return
    d = np.abs(A.data - B.data)
    print(f"{key} J[{k}]: max |difference| {d.max():.3e} of max |J| {np.abs(B.data).max():.3e}, "
          f"{np.count_nonzero(A.data != B.data)} of {A.data.size} entries")
    NOT_BITWISE.append((key, k))
    nphi = A.indptr[A.shape[0] // 3]
    assert sha(A.data[:nphi]) == sha(B.data[:nphi]), (key, k, "k0 / k1 entries")
    assert d.max() <= 1e-12 * np.abs(B.data).max(), (key, k)


def assert_same(on, off):
    """Every Jacobian (assert_same_jacobian), and bitwise every other array and integer of the two
    runs; option 0 never reuses."""
    assert on.keys() == off.keys() and len(on) > 0
    for key in on:
        a, b = on[key], off[key]
        assert len(a.get("jac", [])) == len(b.get("jac", []))
        for k, (A, B) in enumerate(zip(a.get("jac", []), b.get("jac", []))):
            assert_same_jacobian(key, k, A, B)
        assert len(a.get("arrays", [])) == len(b.get("arrays", []))
        for k, (u, v) in enumerate(zip(a.get("arrays", []), b.get("arrays", []))):
            assert u.shape == v.shape, (key, k)
            if sha(u) != sha(v):
                print(f"{key}[{k}]: max |difference| {np.max(np.abs(u - v)):.3e} of max "
                      f"{np.max(np.abs(v)):.3e}, {np.count_nonzero(u != v)} of {u.size} entries")
            assert sha(u) == sha(v), (key, k)
        assert a.get("ints") == b.get("ints"), key
        assert all(c[1] == 0 for c in b["counts"]), (key, b["counts"])


def test_reuse_at_second_state_and_after_solve():
    on, off = both("second_state")
    assert_same(on, off)
    assert len(on) == 3
    for key, v in on.items():  # one full write, then the reuse variant twice (warm, cold hint)
        want = [[1, 0], [2, 0], [3, 0]] if key.endswith("pnp_ie") else [[1, 0], [1, 1], [1, 2]]
        assert v["counts"] == want, (key, v["counts"])
    assert not NOT_BITWISE, NOT_BITWISE
    for key, v in off.items():
        assert v["counts"] == [[1, 0], [2, 0], [3, 0]], (key, v["counts"])


CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_asm_const as T
on, off = T.case_second_state(1), T.case_second_state(0)
T.assert_same(on, off)
print("RESULT " + json.dumps({k: v["counts"] for k, v in on.items()}))
"""


def run_child(lds):
    env = dict(os.environ, PNP_ASM_LDS=str(lds))
    p = subprocess.run([sys.executable, "-c", CHILD.replace("HERE", repr(HERE))], env=env,
                       capture_output=True, text=True, timeout=300, cwd=HERE)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_reuse_with_either_walk_forced():
    """PNP_ASM_LDS = 1 / 0: the LDS-staged and the direct reuse variants, each against option 0 in
    its own process (the child asserts the equality and reports the counters)."""
    a, b = run_child(1), run_child(0)
    assert len(a) == len(b) == 3
    for k in a:
        want = [[1, 0], [2, 0], [3, 0]] if k.endswith("pnp_ie") else [[1, 0], [1, 1], [1, 2]]
        assert a[k] == b[k] == want, k


def test_operator_change_and_fd_jacobian_invalidate():
    on, off = both("invalidation")
    assert_same(on, off)
    assert len(on) == 4
    for name in NAMES:
        before, after = on[f"{name}/operator"]["counts"]  # PNP, PB, then PNP again: all full
        assert before == [2, 0] and after == [3, 0], (name, before, after)
        before, mid, after = on[f"{name}/fd"]["counts"]   # PNP, FD | PNP full | PNP reused
        assert before == [2, 0] and mid == [3, 0] and after == [3, 1], (name, before, mid, after)


def test_implicit_euler_dt_change_writes_all_planes():
    on, off = both("implicit_euler")
    assert_same({"dt_change": on["dt_change"]}, {"dt_change": off["dt_change"]})
    assert on["dt_change"]["counts"] == [[1, 0], [2, 0]]
    Ja, Jb = on["dt_change"]["jac"]
    nphi = Ja.indptr[Ja.shape[0] // 3]
    assert sha(Ja.data[:nphi]) != sha(Jb.data[:nphi])  # the planes scale with dt


def test_implicit_euler_time_steps_write_all_planes():
    on, off = both("implicit_euler")
    assert_same({"same_dt": on["same_dt"]}, {"same_dt": off["same_dt"]})
    assert on["same_dt"]["counts"] == [[1, 0], [2, 0]]  # PNP_IE: every assembly writes all planes
    # two Newton-solved time steps: the same Newton and BiCGSTAB counts and bitwise the same
    # iterates
    a, b = on["time_steps"], off["time_steps"]
    for k, (u, v) in enumerate(zip(a["iterates"], b["iterates"])):
        print(f"time step {k}: max |difference| {np.max(np.abs(u - v)):.3e} of max "
              f"{np.max(np.abs(v)):.3e}; Newton / BiCGSTAB counts {a['steps']} {b['steps']}")
        assert sha(u) == sha(v), k
    assert a["steps"] == b["steps"]
    assert on["time_steps"]["counts"] == off["time_steps"]["counts"]
    assert on["time_steps"]["counts"][0][1] == 0 and on["time_steps"]["counts"][0][0] >= 3


def test_matrix_free_values_on_demand():
    on, off = both("matrix_free")
    assert_same(on, off)
    assert len(on) == 3
    for key, v in on.items():
        want = [[1, 0], [2, 0]] if key.endswith("pnp_ie") else [[1, 0], [1, 1]]
        assert v["counts"] == want, (key, v["counts"])


def test_newton_trajectory():
    on, off = both("newton")
    assert_same(on, off)
    for name in NAMES:
        full, reused = on[name]["counts"][0]
        total = off[name]["counts"][0][0]
        assert full == 1 and reused == total - 1 and total >= 2, (name, full, reused, total)
