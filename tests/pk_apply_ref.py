"""The matrix-free P_k Jacobian application (pnp_pk_matfree_set; k_pk_elem_apply, k_pk_apply_gather
and k_pk_diag of pk_assemble.hip) restated in numpy on the oracle's P_k space: its basis
(O.PkSpace.basis), its element node lists (enode) and its quadrature rules (O.quadrature_rule).

Per element and quadrature point, with v the vector, vq = sum v_i phi_i, gv = sum v_i grad phi_i:
    PB / Poisson (order 3, f = w |det| [2 pi y]):  y_a += (grad phi_a . gv + c_q phi_a vq) f,
        c_q = 8 pi l_b c0 cosh(u_q) for PB (u_q = sum x_i phi_i), 0 for Poisson
    diffusion (order 2, f = w |det|):  y_a += sc (grad phi_a . gv + vq z (gP . grad phi_a)) f,
        gP = sum phi0_i grad phi_i the frozen potential's gradient, sc = dt for the implicit Euler
        operator, else 1
    implicit Euler also (order 5, f = w |det|):  y_a += phi_a vq f
The diagonal is the same sums with v replaced by the a-th unit vector, row by row.  A constrained
row (mask) gives y = v and a diagonal of 1; columns are not eliminated, as in the stored matrix.
tests/test_pk_apply_ref_host.py holds both to the oracle's assembled Jacobian."""
import numpy as np

import oracle_py as O


def _geometry(S):
    xy, en = S.xy, S.enode
    p0, p1, p2 = xy[en[:, 0]], xy[en[:, 1]], xy[en[:, 2]]
    J00, J01 = p1[:, 0] - p0[:, 0], p2[:, 0] - p0[:, 0]
    J10, J11 = p1[:, 1] - p0[:, 1], p2[:, 1] - p0[:, 1]
    det = J00 * J11 - J01 * J10
    # jacobianInverseTransposed
    it = np.stack([np.stack([J11 / det, -J10 / det], -1), np.stack([-J01 / det, J00 / det], -1)], 1)
    return p0[:, 1], J10, J11, np.abs(det), it


def _points(S, order, it):
    """per quadrature point: (xi, eta, w, phi [nl], physical gradients g [ne, nl, 2])"""
    for xi, eta, w in zip(*O.quadrature_rule(order)):
        phi, dphi = S.basis(xi, eta)
        yield xi, eta, w, phi, np.einsum("eij,aj->eai", it, dphi)


def _element_terms(S, orc, kind, x, kw, fn):
    """fn(f [ne], phi [nl], g [ne, nl, 2], c [ne] or None, drift [ne, nl] or None, mass) per point"""
    y0, J10, J11, adet, it = _geometry(S)
    en = S.enode
    p = orc.p
    if kind == "diff_ie":
        for xi, eta, w, phi, g in _points(S, 5, it):
            fn(w * adet, phi, g, None, None, True)
    if kind in ("pb", "poisson"):
        for xi, eta, w, phi, g in _points(S, 3, it):
            f = w * adet
            if p.cylindrical:
                f = f * (y0 + J10 * xi + J11 * eta) * 2 * p.pi
            c = None
            if kind == "pb":
                c = 8 * p.pi * p.l_b * p.c0 * np.cosh(x[en] @ phi)
            fn(f, phi, g, c, None, False)
    else:
        sc = kw["dt"] if kind == "diff_ie" else 1.0
        for xi, eta, w, phi, g in _points(S, 2, it):
            gP = np.einsum("ea,eai->ei", kw["phi"][en], g)
            drift = kw["z"] * np.einsum("ei,eai->ea", gP, g)
            fn(sc * w * adet, phi, g, None, drift, False)


def apply(S, orc, kind, x, kw, mask, v):
    """y = J(x) v over the oracle's nodes"""
    en = S.enode
    ye = np.zeros(en.shape)
    vl = v[en]

    def point(f, phi, g, c, drift, mass):
        vq = vl @ phi
        if mass:
            ye[:] += (f * vq)[:, None] * phi[None, :]
            return
        gv = np.einsum("ea,eai->ei", vl, g)
        t = np.einsum("eai,ei->ea", g, gv)
        if c is not None:
            t = t + (c * vq)[:, None] * phi[None, :]
        if drift is not None:
            t = t + vq[:, None] * drift
        ye[:] += f[:, None] * t

    _element_terms(S, orc, kind, x, kw, point)
    y = np.zeros(S.nn)
    np.add.at(y, en.ravel(), ye.ravel())
    m = np.asarray(mask) != 0
    y[m] = v[m]
    return y


def diagonal(S, orc, kind, x, kw, mask):
    """diag J(x) over the oracle's nodes"""
    en = S.enode
    de = np.zeros(en.shape)

    def point(f, phi, g, c, drift, mass):
        if mass:
            de[:] += f[:, None] * (phi * phi)[None, :]
            return
        t = np.einsum("eai,eai->ea", g, g)
        if c is not None:
            t = t + c[:, None] * (phi * phi)[None, :]
        if drift is not None:
            t = t + phi[None, :] * drift
        de[:] += f[:, None] * t

    _element_terms(S, orc, kind, x, kw, point)
    d = np.zeros(S.nn)
    np.add.at(d, en.ravel(), de.ravel())
    d[np.asarray(mask) != 0] = 1.0
    return d
