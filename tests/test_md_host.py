"""pnp_md_run without a GPU: the declaration, the export, the Python mirror of its structs."""
import ctypes as C
import re

import pnp_amd as P


def header_text():
    return open(P.HEADER).read()


def struct_fields(name):
    """field names of `typedef struct { ... } name;` in the header, in order"""
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", header_text()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    return out


def test_md_run_is_declared_exported_and_bound():
    assert "pnp_md_run" in P.header_symbols()
    assert hasattr(P.lib(), "pnp_md_run")
    assert callable(P.Context.md_run)


def test_struct_mirrors_follow_the_header():
    assert [f for f, _ in P._MdOpts._fields_] == struct_fields("pnp_md_opts")
    assert [f for f, _ in P._MdResult._fields_] == struct_fields("pnp_md_result")
    assert dict(P._MdOpts._fields_)["linear"] is P._SolveOpts


def test_no_option_was_added():
    opts = {k: v for k, v in P.header_constants().items() if k.startswith("PNP_OPT_")}
    assert sorted(opts.values()) == list(range(1, 15))


def test_null_arguments_are_refused_before_anything_touches_a_device():
    o, r = P._MdOpts(), P._MdResult()
    u = (C.c_double * 3)()
    assert P.lib().pnp_md_run(None, u, C.byref(o), 0, 0, None, None, None, C.byref(r), 0) == P.E_ARG
