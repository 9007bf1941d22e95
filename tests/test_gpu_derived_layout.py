"""The context uses the layout its host twin derives: pnp_get_info's counters of the uploaded
split and sweep lists are those of Layout(...).derived (tests/test_derived_layout_host.py checks
the arrays themselves on the host), and a BiCGSTAB + ILU(0) solve on that layout converges."""
import os

import numpy as np
import pytest

import fan_meshes as F
import pnp_amd as P
from asm_regular_cases import PHYS, SURF
from conftest import DATA

pytestmark = pytest.mark.gpu


def _cases():
    xy, tri, bseg, bgroup = F.make("diamond_chain_86", "alt")
    yield P.Mesh(xy, tri, bseg, bgroup), P.Params([P.Surface(**s) for s in SURF], **PHYS)
    cfg = P.read_config(os.path.join(DATA, "pore_pnp", "pore.cfg"))
    yield P.Mesh.read_gmsh(cfg.meshfile), P.Params.from_config(cfg)


def test_context_counters_are_the_host_twins():
    for mesh, par in _cases():
        L = P.Layout(mesh)
        d = L.derived
        ctx = P.Context(mesh, par, device=0)
        info = ctx.info()
        want = dict(lslots=d.lslots, uslots=d.uslots, lslots_live=d.lslots_live,
                    uslots_live=d.uslots_live, lsx_entries=d.lsx_entries,
                    usx_entries=d.usx_entries, ncolors=L.ncolors, nchunks=L.nchunks)
        assert {k: info[k] for k in want} == want
        assert d.sweep_usable and d.lsx_entries > 0
        ctx.set_operator(P.OP_PNP)
        nv = mesh.nv
        rng = np.random.default_rng(20261021)
        x = np.concatenate([rng.uniform(-1, 1, nv), 0.06 * rng.uniform(0.5, 1.5, nv),
                            0.06 * rng.uniform(0.5, 1.5, nv)])
        r = ctx.residual(x)
        ctx.jacobian(x)
        z, res = ctx.linear_solve(r, prec=P.PREC_ILU0, reduction=1e-8, maxit=2000)
        ctx.close()
        assert res["converged"] == 1 and np.all(np.isfinite(z))
