"""OPT_MATRIX_FREE's public surface without a GPU: the header, the Python constants and the
library's exported symbols agree."""
import pnp_amd as P


def test_header_and_python_agree_on_the_matrix_free_option():
    assert "pnp_matfree_info" in P.header_symbols()
    consts = P.header_constants()
    assert "PNP_OPT_MATRIX_FREE" in consts
    assert P.OPT_MATRIX_FREE == consts["PNP_OPT_MATRIX_FREE"] == 12
    # every PNP_OPT_* of the header has its Python constant, with the header's value
    opts = {k: v for k, v in consts.items() if k.startswith("PNP_OPT_")}
    assert len(opts) >= 12 and len(set(opts.values())) == len(opts)
    for k, v in opts.items():
        assert getattr(P, k[len("PNP_"):]) == v, k
    assert hasattr(P.lib(), "pnp_matfree_info")
    assert callable(P.Context.matfree_info)
