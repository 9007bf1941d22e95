"""The pipelined assembly's knobs, pnp_asm_info's count of pipelined launches and the row-flag query
in the C header, the library and the Python package (no GPU; the behaviour is tested in
test_gpu_asm_pipe.py and test_gpu_asm_rowflags.py)."""
import re

import pnp_amd as P


def header_text():
    return open(P.HEADER).read()


def test_asm_info_counts_pipelined_launches_in_header_library_and_wrapper():
    assert "pnp_asm_info" in P.header_symbols()
    decl = re.search(r"int pnp_asm_info\(([^)]*)\);", header_text()).group(1)
    assert [a.split("*")[-1].strip() for a in decl.split(",")] == ["ctx", "full", "reused",
                                                                  "pipelined"]
    assert hasattr(P.lib(), "pnp_asm_info")
    doc = P.Context.asm_info.__doc__
    assert "pipelined" in doc


def test_knob_names_are_in_the_header_and_the_python_mirror():
    txt = header_text()
    assert P.ASM_PIPE_ENV == "PNP_ASM_PIPE" and P.ASM_PIPE_GRID_ENV == "PNP_ASM_PIPE_GRID"
    assert re.search(r"\bPNP_ASM_PIPE=0/1", txt) and re.search(r"\bPNP_ASM_PIPE_GRID=n\b", txt)


def test_row_flag_query_is_declared_exported_and_wrapped():
    assert "pnp_asm_row_flags" in P.header_symbols()
    assert hasattr(P.lib(), "pnp_asm_row_flags")
    assert callable(P.Context.asm_row_flags)
    m = re.search(r"^#define PNP_ROW_FLAG_LOAD (\d+)\s*$", header_text(), re.M)
    assert m and int(m.group(1)) == P.ROW_FLAG_LOAD == 8
