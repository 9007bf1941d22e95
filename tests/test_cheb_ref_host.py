"""tests/cheb_ref.py held to itself, and the case table of tests/test_gpu_cheb.py held to the
reference alone (no GPU): the oracle's Jacobians only.

  * steps 1 is the vertex-block solve;
  * the recurrence equals q(T) D^-1 d, T = D^-1 A, with q built from numpy.polynomial.chebyshev,
    on the dense pore_small_k0 PB matrix to 1e-10;
  * the Chebyshev bound on that SPD system: |1 - lambda q(lambda)| <= 1 / T_k(sigma) for every
    eigenvalue of D^-1 A inside [lmin, lmax];
  * the GPU tests' case table: cond_2(D_i) <= 1e4 for every diagonal block (a 1e-10 comparison of
    two block solves then means something), every reference result finite, and the boosted 20-step
    estimate at or above the dense spectral radius where the GPU tests rely on the estimate."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import cheb_ref as R
import oracle_py as O
from test_gpu import golden
from test_gpu_fan_walks import problem as fan_problem, set_kind

COND_CAP = 1e4
FAN_MESHES = ("one_triangle", "pinwheel_3_1", "half_wheel_30", "pinwheel_13_1_12",
              "diamond_chain_21", "diamond_chain_85", "diamond_chain_86")
FAN_KINDS = ("pnp", "pnp_ie", "pb", "poisson", "diff_ie+")
VARIANTS = ("free", "mixed")
STEPS = (1, 2, 3, 4, 7)
GOLDENS = ("cylinder_k0", "pore_small_k0", "pore_pnp_k0", "sphere_k0")


def nf_of(kind):
    return 3 if kind.startswith("pnp") else 1


@functools.lru_cache(maxsize=None)
def fan_jacobian(mesh_id, kind, variant):
    _, _, orc, st, _ = fan_problem(mesh_id, variant)
    op, x = set_kind(None, orc, st, kind)
    return orc.jacobian(op, x).tocsr()


@functools.lru_cache(maxsize=None)
def golden_jacobian(name, kind):
    z, mesh, _, orc = golden(name)
    if kind == "pb":
        op = orc.operator(O.OP_PB, flux=orc.flux(), mask=orc.mask(1))
        x = np.zeros(mesh.nv)
    else:
        op = orc.operator(O.OP_PNP, flux=orc.flux(), mask=orc.mask(3))
        x = np.ascontiguousarray(z["newton_pnp_x0"] if name == "pore_small_k0" else z["pnp_x"])
    return orc.jacobian(op, x).tocsr()


def scaled_dense(A, nf):
    """T = D^-1 A, dense"""
    D = R.diag_blocks(A, nf)
    Ad = A.toarray()
    return np.column_stack([R.block_solve(D, Ad[:, j]) for j in range(Ad.shape[1])])


def test_steps_one_is_the_block_solve():
    A = golden_jacobian("cylinder_k0", "pnp")
    nv = A.shape[0] // 3
    d = np.random.default_rng(1).standard_normal(3 * nv)
    z = R.apply(A, 3, d, 1)
    # block by block against a dense solve of the block-diagonal matrix
    i = np.arange(nv)
    idx = np.concatenate([f * nv + i for f in range(3)])
    B = sp.lil_matrix(A.shape)
    for f in range(3):
        for g in range(3):
            B[f * nv + i, g * nv + i] = np.asarray(A[f * nv + i, g * nv + i]).ravel()
    zd = np.linalg.solve(B.toarray(), d)
    assert idx.size == 3 * nv
    assert np.max(np.abs(z - zd)) <= 1e-12 * np.max(np.abs(zd))


@pytest.mark.parametrize("steps", [2, 3, 4, 7])
def test_recurrence_equals_the_closed_form_and_meets_the_chebyshev_bound(steps):
    A = golden_jacobian("pore_small_k0", "pb")
    n = A.shape[0]
    T = scaled_dense(A, 1)
    lam = np.linalg.eigvals(T)
    assert np.max(np.abs(lam.imag)) <= 1e-10 and lam.real.min() > 0  # SPD, diagonally scaled
    lam = lam.real
    lmax, lmin = R.bounds(R.power_estimate(A, 1, 20))
    assert lmax >= lam.max()
    d = np.random.default_rng(steps).standard_normal(n)
    z = R.apply(A, 1, d, steps, lmax, lmin)
    q = R.polynomial(steps, lmax, lmin)
    g = R.block_solve(R.diag_blocks(A, 1), d)
    zq = np.zeros(n)
    for c in q.coef[::-1]:  # Horner in T
        zq = T @ zq + c * g
    print(f"steps {steps}: closed-form difference {np.max(np.abs(z - zq)) / np.max(np.abs(zq)):.2e}")
    assert np.max(np.abs(z - zq)) <= 1e-10 * np.max(np.abs(zq))
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    tk = np.polynomial.chebyshev.Chebyshev.basis(steps)(theta / delta)
    inside = lam[(lam >= lmin) & (lam <= lmax)]
    assert inside.size > 0
    assert np.max(np.abs(1.0 - inside * q(inside))) <= (1 + 1e-9) / tk


@pytest.mark.parametrize("mesh_id", FAN_MESHES)
def test_fan_cases_are_well_conditioned_and_finite(mesh_id):
    worst = 0.0
    for variant in VARIANTS:
        for kind in FAN_KINDS:
            A = fan_jacobian(mesh_id, kind, variant)
            nf = nf_of(kind)
            D = R.diag_blocks(A, nf)
            worst = max(worst, float(np.max(np.linalg.cond(D))))
            d = np.random.default_rng(5).standard_normal(A.shape[0])
            est = R.power_estimate(A, nf, 20)
            assert np.isfinite(est) and est > 0
            for steps in STEPS:
                for lmax in (2.5, 1.1 * est):
                    z = R.apply(A, nf, d, steps, lmax, lmax / 10.0)
                    assert np.all(np.isfinite(z))
    print(f"{mesh_id}: worst cond_2(D_i) {worst:.3g}")
    assert worst <= COND_CAP


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_blocks_are_well_conditioned(name):
    for kind in ("pb", "pnp"):
        if kind == "pnp" and "pnp_x" not in golden(name)[0].files:
            continue  # a PB-only golden (sphere_k0)
        A = golden_jacobian(name, kind)
        c = float(np.max(np.linalg.cond(R.diag_blocks(A, nf_of(kind)))))
        print(f"{name} {kind}: worst cond_2(D_i) {c:.3g}")
        assert c <= COND_CAP


def spectral_radius(A, nf):
    if nf == 1:
        # constrained rows are identity rows: eigenvalue 1 each, and block triangular with the free
        # rows' block B, where D^-1 B is similar to the symmetric D^-1/2 B D^-1/2
        A = sp.csr_matrix(A, copy=True)
        A.eliminate_zeros()
        ident =(np.diff(A.indptr) == 1) & (A.diagonal() == 1.0)
        B = A[~ident][:, ~ident]
        dg = B.diagonal()
        assert dg.min() > 0
        S = sp.diags(1.0 / np.sqrt(dg))
        M = (S @ B @ S).toarray()
        if np.max(np.abs(M - M.T)) <= 1e-12 * np.max(np.abs(M)):
            rho = float(np.max(np.abs(np.linalg.eigvalsh(0.5 * (M + M.T)))))
            return max(rho, 1.0) if ident.any() else rho
    return float(np.max(np.abs(np.linalg.eigvals(scaled_dense(A, nf)))))


@pytest.mark.parametrize("name,kind", [(g, "pb") for g in GOLDENS] +
                         [("cylinder_k0", "pnp"), ("pore_small_k0", "pnp")])
def test_boosted_estimate_bounds_the_spectral_radius(name, kind):
    A = golden_jacobian(name, kind)
    nf = nf_of(kind)
    est = R.power_estimate(A, nf, 20)
    rho = spectral_radius(A, nf)
    print(f"{name} {kind}: estimate {est:.4f} x 1.1 = {1.1 * est:.4f}, spectral radius {rho:.4f}")
    assert 1.1 * est >= rho
