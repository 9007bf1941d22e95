"""CPU tests of the GMRES yardstick (tests/gmres_ref.py) and of the binding's new constants.

The yardstick is pinned against dense least squares: after k Arnoldi steps of the first cycle,
GMRES's residual norm is min |b - A v| over v in the Krylov space K_k(A, b), which
numpy.linalg.lstsq computes on an orthonormalised power basis without any GMRES machinery.
Systems: the oracle's Jacobians of the golden fixtures (PB on pore_small_k0 at phi = 0, PNP on
cylinder_k0 at pnp_x), right-hand side the oracle's residual there.
"""
import os

import numpy as np
import pytest

import gmres_ref
import meshio
import oracle_py as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _problem(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    m = meshio.Mesh(z["xy"], z["tri"].astype(np.int32), z["bseg"].astype(np.int32),
                    z["bgroup"].astype(np.int32))
    surfs = [meshio.Surface(int(s[0]), s[1], s[2], int(s[3]), s[4], s[5], int(s[6]), s[7], s[8])
             for s in z["surfaces"]]
    l_b, c0, tau, cyl, pi = z["params"]
    return z, O.Problem(m, surfs, l_b=l_b, c0=c0, tau=tau, cylindrical=int(cyl), pi=pi)


def _system(which):
    if which == "pb":
        z, orc = _problem("pore_small_k0")
        op = orc.operator(O.OP_PB, flux=orc.flux(), mask=np.ascontiguousarray(orc.mask(1)))
        x = np.zeros(z["xy"].shape[0])
    else:
        z, orc = _problem("cylinder_k0")
        op = orc.operator(O.OP_PNP, flux=orc.flux(), mask=np.ascontiguousarray(orc.mask(3)))
        x = np.ascontiguousarray(z["pnp_x"])
    return orc.jacobian(op, x).tocsr(), orc.residual(op, x)


SYSTEMS = {}


def system(which):
    if which not in SYSTEMS:
        SYSTEMS[which] = _system(which)
    return SYSTEMS[which]


@pytest.mark.parametrize("which,iterations", [("pb", 95), ("cylinder_pnp", 475)])
def test_yardstick_matches_dense_least_squares(which, iterations):
    A, b = system(which)
    ref = gmres_ref.gmres(A, b, restart=30, reduction=1e-8, maxit=3000)
    assert ref.converged and ref.iterations == iterations
    assert ref.history.size == ref.iterations + 1
    assert np.linalg.norm(b - A @ ref.x) < 1e-8 * np.linalg.norm(b)
    # orthonormal basis of K_k(A, b), built incrementally so that it stays well conditioned:
    # q_{k+1} from A q_k, orthogonalised twice against q_1 .. q_k
    n = b.size
    Q = np.zeros((n, 30))
    Q[:, 0] = b / np.linalg.norm(b)
    worst = 0.0
    for k in range(1, 31):
        AQ = A @ Q[:, :k]
        y = np.linalg.lstsq(AQ, b, rcond=None)[0]
        best = np.linalg.norm(b - AQ @ y)
        worst = max(worst, abs(ref.history[k] - best) / best)
        if k < 30:
            w = AQ[:, k - 1]
            for _ in range(2):
                w = w - Q[:, :k] @ (Q[:, :k].T @ w)
            Q[:, k] = w / np.linalg.norm(w)
    assert worst <= 1e-10, worst


def test_orthogonalisation_orders_agree():
    """CGS2 and modified Gram-Schmidt: same iteration counts, histories equal to rounding inside
    the first cycle (the spread the GPU history tolerance of 1e-10 is set against)."""
    A, b = system("pb")
    a = gmres_ref.gmres(A, b, restart=30, reduction=1e-8, maxit=3000)
    m = gmres_ref.gmres(A, b, restart=30, reduction=1e-8, maxit=3000, mgs=True)
    assert a.iterations == m.iterations
    assert np.max(np.abs(a.history[:31] - m.history[:31]) / a.history[:31]) <= 1e-12


def test_flexible_equals_right_preconditioned_for_a_linear_preconditioner():
    A, b = system("pb")
    d = 1.0 / A.diagonal()
    a = gmres_ref.gmres(A, b, M=lambda v: d * v, restart=7, reduction=1e-10, maxit=3000)
    f = gmres_ref.gmres(A, b, M=lambda v: d * v, restart=7, reduction=1e-10, maxit=3000,
                        flexible=True)
    assert a.converged and f.converged and a.iterations == f.iterations
    # the recomputed norms at the restart boundaries carry the rounding of b - A x itself, an
    # absolute error of the order eps |A| |x| ~ 1e-14 |b| here, on top of the relative agreement
    assert np.all(np.abs(a.history - f.history) <= 1e-9 * a.history + 1e-13 * a.history[0])
    assert np.max(np.abs(a.x - f.x)) <= 1e-10 * np.max(np.abs(a.x))


def test_edges():
    A, b = system("pb")
    r = gmres_ref.gmres(A, np.zeros_like(b))
    assert r.converged and r.iterations == 0 and r.history.size == 1
    r = gmres_ref.gmres(A, b, restart=5, maxit=12)
    assert not r.converged and r.iterations == 12 and r.history.size == 13


def test_host_pieces_run_clean_under_the_host_sanitizers():
    """The Hessenberg / Givens / back-substitution / cycle logic the device kernels call
    (csrc/gmres_small.h), driven by a stand-alone program built with -fsanitize=address,undefined."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["make", "-s", "-C", os.path.join(root, "dune-pnp_amd"), "gmres_host_check"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gmres_host_check: ok" in out.stdout


def test_binding_exposes_the_gmres_constants():
    import pnp_amd as P

    assert P.METHOD_GMRES == 2 and P.METHOD_FGMRES == 3 and P.OPT_GMRES_RESTART == 11
    assert hasattr(P.Context, "solve_history")
