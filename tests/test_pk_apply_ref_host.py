"""The formulas of the matrix-free P_k Jacobian application (tests/pk_apply_ref.py, the numpy
restatement of k_pk_elem_apply / k_pk_apply_gather / k_pk_diag) against the CPU oracle's assembled
P_k Jacobian, and the public surface of the switch, without a GPU.

Bounds: the product within apply_error <= 1, i.e. 1e-12 max_i (|Jo| |v|)_i (the project's bound for
an operator application; the oracle reordered against itself stays under 3e-3 of it, see
tests/test_gpu_pk_edges.py); the diagonal within 1e-12 max|Jo| (the Jacobian's own tolerance)."""
import numpy as np
import pytest

import fan_meshes as F
import oracle_py as O
import pk_apply_ref as R
import pnp_amd as P
from test_gpu_asm_const import second_state
from test_gpu_matfree import apply_error, random_z
from test_gpu_pk import KINDS, args
from test_pk_edge_meshes_host import VARIANTS, space

KIND_ORDER = ("pb", "poisson", "diff", "diff_ie")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id,k", F.PK_CASES)
def test_formulas_match_the_assembled_jacobian(mesh_id, k, variant):
    orc, S = space(mesh_id, k, variant)
    worst = {"apply": 0.0, "diag": 0.0}
    for kind in KIND_ORDER:
        field = 2 if kind.startswith("diff") else 0
        mask = S.mask(field)
        x, kw = args(kind, S.nn, 100 * k + KIND_ORDER.index(kind))
        op = orc.operator(KINDS[kind][1], flux=orc.flux(), mask=mask, **kw)
        for xs in (x, second_state(x)):
            Jo = S.jacobian(op, xs)
            v = random_z(S.nn, 7)
            y = R.apply(S, orc, kind, xs, kw, mask, v)
            worst["apply"] = max(worst["apply"], apply_error(y, Jo, v))
            rows = np.nonzero(mask)[0]
            np.testing.assert_array_equal(y[rows], v[rows])
            d = R.diagonal(S, orc, kind, xs, kw, mask)
            worst["diag"] = max(worst["diag"],
                                float(np.abs(d - Jo.diagonal()).max() / (1e-12 * abs(Jo).max())))
    print(f"PK-APPLY-REF {mesh_id} P{k} {variant}: error / bound {worst}")
    assert worst["apply"] <= 1.0 and worst["diag"] <= 1.0, worst


def test_the_switch_is_declared():
    """pnp_pk_matfree_set / _get: in the header, exported by the library, mirrored by Context; no
    new PNP_OPT_* (option 15 stays unknown)"""
    syms = P.header_symbols()
    assert "pnp_pk_matfree_set" in syms and "pnp_pk_matfree_get" in syms
    assert hasattr(P.lib(), "pnp_pk_matfree_set") and hasattr(P.lib(), "pnp_pk_matfree_get")
    assert callable(P.Context.pk_matfree) and callable(P.Context.pk_matfree_get)
    opts = {q: v for q, v in P.header_constants().items() if q.startswith("PNP_OPT_")}
    assert max(opts.values()) == 14
    assert P.lib().pnp_pk_matfree_set(None, 1) == P.E_ARG
    assert P.lib().pnp_pk_matfree_get(None, None) == P.E_ARG
