"""The numpy IDR(s) yardstick (idr_ref.py) against its textbook form, finite termination, a plain
BiCGSTAB, its own residual-replacement path, and the dense part the device kernels call
(csrc/idr_small.h) through the host check program.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import idr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def system(n, seed=7, spread=8.0, offdiag=0.5):
    """Random, strictly diagonally dominant by rows, non-symmetric: a diagonal spread over
    [1, spread] in random order (so that 3 cycles of IDR(8) do not yet reach the rounding floor of
    a 60 x 60 system, where no two orders of the same arithmetic agree) plus dense uniform
    off-diagonal entries whose absolute row sums stay below offdiag / 2."""
    rng = np.random.default_rng(seed)
    A = offdiag / n * rng.uniform(-1.0, 1.0, (n, n))
    np.fill_diagonal(A, 0.0)
    A += np.diag(np.linspace(1.0, spread, n)[rng.permutation(n)])
    assert np.all(np.abs(A).sum(axis=1) < 2.0 * np.abs(np.diag(A)))
    return A, rng.uniform(-1.0, 1.0, n)


@pytest.fixture(scope="module")
def sys60():
    return system(60)


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_alpha_solve_equals_the_textbook_dot_products(sys60, s):
    A, b = sys60
    P = idr_ref.shadow(60, 1, s)
    k = 3 * (s + 1)
    # one application more than compared: entry k + 1 is each run's recomputed true norm, which
    # carries the rounding of b - A x itself; entries 0 .. k are the recurrence's
    a = idr_ref.idr(A, b, P, reduction=1e-300, maxit=k + 1)
    t = idr_ref.idr(A, b, P, reduction=1e-300, maxit=k + 1, textbook=True)
    assert a.iterations == t.iterations == k + 1 and a.history.size == k + 2
    err = np.abs(a.history - t.history)[:k + 1] / t.history[:k + 1]
    print(f"s={s}: worst relative difference of the two forms {err.max():.2e}")
    assert np.all(err <= 1e-10)
    assert len(a.M) == 3 and len(a.omega) == 3
    for Ma, Mt in zip(a.M, t.M):
        assert np.all(np.triu(Ma, 1) == 0.0)
        assert np.max(np.abs(Ma - Mt)) <= 1e-10 * np.max(np.abs(Mt))
    assert np.allclose(a.omega, t.omega, rtol=1e-10, atol=0)


def test_shadow_matrix_is_orthonormal_and_partition_free():
    P = idr_ref.shadow(311, 3, 8)
    assert np.max(np.abs(P @ P.T - np.eye(8))) <= 1e-13
    # the raw entries depend on (vertex, field, column) alone: a sub-range restates them
    assert idr_ref.shadow_entry(17, 2, 5) == idr_ref.shadow_entry(17, 2, 5)
    vals = {idr_ref.shadow_entry(g, f, j) for g in range(50) for f in range(3) for j in range(8)}
    assert len(vals) == 50 * 24 and all(-1.0 < v < 1.0 for v in vals)


def test_finite_termination():
    """IDR(s) ends within n + n / s applications in exact arithmetic: 24 + 6 here, and 2 more for
    rounding."""
    A, b = system(24, seed=3)
    r = idr_ref.idr(A, b, idr_ref.shadow(24, 1, 4), reduction=1e-10, maxit=200)
    assert r.converged and r.iterations <= 24 + 24 // 4 + 2
    assert np.linalg.norm(b - A @ r.x) < 1e-10 * np.linalg.norm(b)


def test_idr1_is_bicgstab(sys60):
    """IDR(1) with the shadow vector p is BiCGSTAB with the shadow residual p: the residual after
    every second application is BiCGSTAB's after a full iteration.  Holds while the omega safeguard
    (|rho| < 0.7) stays idle, as it does on this system: BiCGSTAB here has none."""
    A, b = sys60
    P = idr_ref.shadow(60, 1, 1)
    r = idr_ref.idr(A, b, P, reduction=1e-300, maxit=21)
    h, _ = idr_ref.bicgstab(A, b, rt=P[0], reduction=1e-300, maxit=10)
    assert r.history.size == 22 and h.size == 11
    got = r.history[0:21:2]  # 0, 2, .., 20: the recurrence's (entry 21 is the recomputed norm)
    print("worst relative difference to BiCGSTAB", np.max(np.abs(got - h) / h))
    assert np.all(np.abs(got - h) <= 1e-8 * h)


def test_residual_replacement(sys60):
    """The recurrence's norm is reported 1e8 times too small from application 10 on, once: the test
    is met early, the true norm fails it, the solve goes on from the true residual and converges."""
    A, b = sys60
    P = idr_ref.shadow(60, 1, 4)
    lied = []

    def scale(k):
        if k >= 10 and not lied:
            lied.append(k)
            return 1e-8
        return 1.0

    plain = idr_ref.idr(A, b, P, reduction=1e-8)
    r = idr_ref.idr(A, b, P, reduction=1e-8, norm_scale=scale)
    assert plain.converged and plain.replacements == 0 and plain.iterations > 10
    assert lied == [10] and r.converged and r.replacements == 1
    nb = np.linalg.norm(b)
    assert r.history[10] >= 1e-8 * nb  # the true norm, recorded in place of the lie
    assert abs(r.history[10] - plain.history[10]) <= 1e-6 * plain.history[10]
    assert r.history[-1] < 1e-8 * nb and np.linalg.norm(b - A @ r.x) <= 1.001e-8 * nb
    assert r.history.size == r.iterations + 1
    # a lie kept up: the replacements run out and the solve stops unconverged, no breakdown
    r = idr_ref.idr(A, b, P, reduction=1e-8, norm_scale=lambda k: 1e-6)
    assert not r.converged and r.breakdown == 0 and r.replacements == idr_ref.MAX_REPLACE


def test_edges(sys60):
    A, b = sys60
    P = idr_ref.shadow(60, 1, 4)
    r = idr_ref.idr(A, np.zeros_like(b), P)
    assert r.converged and r.iterations == 0 and r.history.size == 1
    r = idr_ref.idr(A, b, P, reduction=1e-10, maxit=3)  # maxit < s
    assert not r.converged and r.iterations == 3 and r.history.size == 4
    assert abs(r.history[3] - np.linalg.norm(b - A @ r.x)) <= 1e-12 * np.linalg.norm(b)
    r = idr_ref.idr(np.zeros((4, 4)), np.arange(1.0, 5.0), idr_ref.shadow(4, 1, 2))
    assert r.breakdown == 6 and not r.converged and r.iterations == 0


_HOST = []


def _host_check():
    """Builds and runs the host check program once per session: (its output, its path)."""
    if not (shutil.which("make") and shutil.which("g++")):
        pytest.skip("no host compiler: the host check program is not built")
    if not _HOST:
        out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "dune-pnp_amd"),
                              "idr_host_check"], capture_output=True, text=True)
        _HOST.append(out)
    out = _HOST[0]
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout, os.path.join(ROOT, "dune-pnp_amd", "build", "idr_host_check")


def test_host_pieces_run_clean_under_the_host_sanitizers():
    """The triangular solves, the M column, beta, omega, the stop / breakdown 6 / replacement logic
    the device kernels call (csrc/idr_small.h), driven by a stand-alone program built with
    -fsanitize=address,undefined."""
    stdout, _ = _host_check()
    assert "idr_host_check: ok" in stdout


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_host_pieces_follow_the_yardstick(sys60, s, tmp_path):
    """The same dense system through csrc/idr_small.h (the host check program's solve mode) and
    through the yardstick: the histories agree to 1e-10 over the first 3 cycles, the counts and
    the shadow entries exactly."""
    _, exe = _host_check()
    A, b = sys60
    P = idr_ref.shadow(60, 1, s)
    k = 3 * (s + 1)
    path = tmp_path / "sys.txt"
    with open(path, "w") as f:
        f.write(f"60 {s} 1e-300 {k + 1}\n")
        for arr in (A, b, P):
            f.write(" ".join(repr(float(v)) for v in np.asarray(arr).ravel()) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    done, it, repl, brk = (int(v) for v in lines[0].split())
    hist = np.array([float(v) for v in lines[1:] if v.strip()])
    ref = idr_ref.idr(A, b, P, reduction=1e-300, maxit=k + 1)
    assert (done, it, repl, brk) == (3, k + 1, 0, 0) and hist.size == k + 2
    err = np.abs(hist - ref.history)[:k + 1] / ref.history[:k + 1]  # the recurrence's entries
    print(f"s={s}: worst relative difference to the yardstick {err.max():.2e}")
    assert np.all(err <= 1e-10)


def test_binding_exposes_the_idr_constants():
    import pnp_amd as P

    assert P.METHOD_IDR == 4 and P.OPT_IDR_S == 14
    assert hasattr(P.Context, "idr_shadow") and hasattr(P.Context, "solve_history")
