"""PNP_OPT_ASM_REUSE_CONST and pnp_asm_info in the C header, the library and the Python package
(no GPU; the behaviour is tested in test_gpu_asm_const.py)."""
import pnp_amd as P


def test_option_and_query_are_declared_exported_and_wrapped():
    consts = P.header_constants()
    assert P.OPT_ASM_REUSE_CONST == consts["PNP_OPT_ASM_REUSE_CONST"] == 13
    opts = {k: v for k, v in consts.items() if k.startswith("PNP_OPT_")}
    assert len(set(opts.values())) == len(opts)  # the new value collides with no other option
    assert "pnp_asm_info" in P.header_symbols()
    assert hasattr(P.lib(), "pnp_asm_info")
    assert callable(P.Context.asm_info)
