"""The flag byte per row that the P1 assembly's residual tail reads in place of the row's mask
bytes and, on rows with a zero constant load, of its cvec entries (AsmArgs::rowflag,
pnp_asm_row_flags), -m gpu, one process.

* Every operator kind the goldens carry: residual against the committed golden residual and the
  oracle, Jacobian against the oracle's analytic one, at test_gpu.py's bounds (1e-12 of the
  largest entry); the flags' mask bits are the oracle's Dirichlet mask, and the load bit is set
  on no interior row (the Neumann load lives on the boundary), on no row of the diffusion operator.
* c_extra in rows that otherwise have a zero load: the new residual is the correctly rounded
  residual_without_extra + c_extra on unmasked rows and 0 on masked rows, bitwise; and with
  c_extra in multiples of 2^80, which absorb the residual in the sum and in the difference,
  residual(x) - residual_without_extra(x) is c_extra itself on unmasked rows, 0 on masked ones.
* A c_extra entry of -0.0 flags its row (and changes no residual value).
* Implicit Euler: every row is flagged."""
import functools

import numpy as np
import pytest

import pnp_amd as P
from test_gpu import CASES, golden, set_ops

pytestmark = pytest.mark.gpu

KINDS = sorted({c for c in CASES if c[0] in ("pore_small_k0", "cylinder_k0")})


@functools.lru_cache(maxsize=None)
def gold(name):
    return golden(name)


@pytest.mark.parametrize("name,kind", KINDS)
def test_operator_residual_jacobian_and_flags(name, kind):
    z, mesh, par, orc = gold(name)
    ctx = P.Context(mesh, par)
    op = set_ops(z, ctx, orc, kind)
    x = z[kind + "_x"]
    nv, nf = mesh.nv, ctx.nf
    r = ctx.residual(x)
    ro = orc.residual(op, x)
    scale = np.max(np.abs(ro))
    print(name, kind, "residual", np.max(np.abs(r - ro)) / scale,
          np.max(np.abs(r - z[kind + "_r"])) / scale)
    assert np.max(np.abs(r - ro)) <= 1e-12 * scale
    assert np.max(np.abs(r - z[kind + "_r"])) <= 1e-12 * scale
    J = ctx.jacobian(x)
    Jo = orc.jacobian(op, x, fd=False)
    print(name, kind, "jacobian", abs(J - Jo).max() / abs(Jo).max())
    assert abs(J - Jo).max() <= 1e-12 * abs(Jo).max()

    fl = ctx.asm_row_flags()
    assert fl.shape == (nv,) and not np.any(fl == 0xff)
    mask = orc.mask(3)[2 * nv:] if kind == "diff" else orc.mask(nf)
    mask = np.asarray(mask).reshape(nf, nv) != 0
    for f in range(nf):
        assert np.array_equal((fl >> f) & 1, mask[f].astype(np.uint8)), (name, kind, f)
    assert not np.any(fl & 0x70) and not np.any((fl & 7) >> nf)
    loaded = (fl & P.ROW_FLAG_LOAD) != 0
    if kind == "pnp_ie":
        assert loaded.all()
    elif kind == "diff":
        assert not loaded.any()  # the diffusion operator has no Neumann load
    else:
        # the Neumann load lives on boundary vertices only: interior rows never read cvec
        interior = np.setdiff1d(np.arange(nv), np.unique(np.asarray(mesh.bseg).reshape(-1)))
        assert interior.size > 0 and not loaded[interior].any(), (name, kind)
    ctx.close()


@pytest.mark.parametrize("name", ["pore_small_k0", "cylinder_k0"])
def test_c_extra_in_rows_without_a_load(name):
    z, mesh, par, orc = gold(name)
    nv = mesh.nv
    x = z["pnp_x"]
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PNP)
    r0 = ctx.residual(x)
    fl0 = ctx.asm_row_flags()
    free = np.flatnonzero((fl0 & P.ROW_FLAG_LOAD) == 0)
    assert free.size > 8
    assert np.max(np.abs(r0)) < 2.0 ** 12
    # every 5th row without a load, and up to 16 masked rows without one
    masked_rows = np.flatnonzero((fl0 & 7) != 0)
    rows = np.union1d(free[::5], np.intersect1d(free, masked_rows)[:16])
    others = np.setdiff1d(np.arange(nv), rows)
    R0 = r0.reshape(3, nv)
    # pass 0: values of the residual's own size -- r0 = R + 0.0 = R on these rows, so the new
    # residual is the correctly rounded r0 + c_extra; pass 1: multiples of 2^80, which absorb any
    # |R| < 2^12 in the sum and in the difference, so r1 - r0 is c_extra itself
    for scale in (2.0 ** -3, 2.0 ** 80):
        ce = np.zeros((3, nv))
        for f in range(3):
            ce[f, rows] = (1 + (rows + f) % 7) * scale * (-1.0) ** f
        ctx.set_operator(P.OP_PNP, c_extra=ce.reshape(-1))
        fl = ctx.asm_row_flags()
        assert np.array_equal((fl & P.ROW_FLAG_LOAD) != 0,
                              ((fl0 & P.ROW_FLAG_LOAD) != 0) | np.isin(np.arange(nv), rows))
        assert np.array_equal(fl & 7, fl0 & 7)
        m = np.stack([(fl >> f) & 1 for f in range(3)]) != 0
        assert m[:, rows].any() and not m[:, rows].all()
        r1 = ctx.residual(x)
        R1 = r1.reshape(3, nv)
        assert np.array_equal(R1[:, rows], np.where(m, 0.0, R0 + ce)[:, rows])
        assert np.array_equal(R1[:, others], R0[:, others])
        assert np.all(R1[m] == 0.0) and not np.any(np.signbit(R1[m]))
        if scale > 1:
            assert np.array_equal((R1 - R0)[:, rows], np.where(m, 0.0, ce)[:, rows])
    ctx.close()


def test_negative_zero_c_extra_flags_the_row():
    z, mesh, par, orc = gold("pore_small_k0")
    nv = mesh.nv
    x = z["pnp_x"]
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PNP)
    r0 = ctx.residual(x)
    fl0 = ctx.asm_row_flags()
    free = np.flatnonzero((fl0 & P.ROW_FLAG_LOAD) == 0)
    rows = free[1::7]
    ce = np.zeros((3, nv))
    ce[1, rows] = -0.0
    assert np.signbit(ce[1, rows]).all()
    ctx.set_operator(P.OP_PNP, c_extra=ce.reshape(-1))
    fl = ctx.asm_row_flags()
    assert np.all(fl[rows] & P.ROW_FLAG_LOAD)
    assert np.array_equal(fl & ~np.uint8(P.ROW_FLAG_LOAD), fl0 & ~np.uint8(P.ROW_FLAG_LOAD))
    assert ((fl & P.ROW_FLAG_LOAD) != 0).sum() == ((fl0 & P.ROW_FLAG_LOAD) != 0).sum() + rows.size
    r1 = ctx.residual(x)
    # R + (-0.0) = R: the values are those of R + 0.0 wherever R is not -0.0 (there: -0.0)
    assert np.array_equal(r1, r0)
    ctx.close()


def test_implicit_euler_flags_every_row():
    z, mesh, par, orc = gold("pore_small_k0")
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PNP_IMPLICIT_EULER, dt=float(z["params"][2]), x_old=z["pnp_ie_x_old"])
    assert np.all(ctx.asm_row_flags() & P.ROW_FLAG_LOAD)
    ctx.set_operator(P.OP_PNP)  # and the next operator's flags replace them
    assert not np.all(ctx.asm_row_flags() & P.ROW_FLAG_LOAD)
    ctx.close()
