"""PNP_PREC_CHEBYSHEV without a GPU: the declarations, the exports, the Python mirror, and the
argument checks that run before anything touches a device."""
import ctypes as C
import re

import pnp_amd as P
from test_md_host import struct_fields


def test_declared_exported_and_bound():
    syms = P.header_symbols()
    for name in ("pnp_cheb_configure", "pnp_cheb_info"):
        assert name in syms and hasattr(P.lib(), name)
    assert callable(P.Context.cheb_configure) and callable(P.Context.cheb_info)
    m = re.search(r"\bPNP_PREC_CHEBYSHEV = (\d+)", open(P.HEADER).read())
    assert m and int(m.group(1)) == P.PREC_CHEBYSHEV == 6
    assert P.PREC_BY_NAME["cheb"] == P.PREC_CHEBYSHEV
    # the preconditioners before it keep their values
    assert (P.PREC_NONE, P.PREC_SSOR, P.PREC_ILU0, P.PREC_JACOBI, P.PREC_AMG,
            P.PREC_SSOR_NATURAL) == tuple(range(6))


def test_struct_mirrors_follow_the_header():
    assert [f for f, _ in P._ChebOpts._fields_] == struct_fields("pnp_cheb_opts")
    assert [f for f, _ in P._ChebStats._fields_] == struct_fields("pnp_cheb_stats")
    assert C.sizeof(P._ChebOpts) == 40 and C.sizeof(P._ChebStats) == 64


def test_null_arguments_are_refused():
    o, s = P._ChebOpts(3, 10.0, 20, 1.1, 0.0), P._ChebStats()
    assert P.lib().pnp_cheb_configure(None, C.byref(o)) == P.E_ARG
    assert P.lib().pnp_cheb_info(None, C.byref(s)) == P.E_ARG
