"""The P_k table of tests/fan_meshes.py against the CPU oracle's P_k space (no GPU): node count,
longest row of the oracle's Jacobian pattern, element count and the most elements at one node, for
every (mesh, degree) that tests/test_gpu_pk_edges.py assembles on the GPU; the refused meshes'
longest rows; and the boundary variants' masks.  The GPU tests take what a mesh reaches (a 63-slot
row, a hub in exactly 4 or 5 elements, 128 or 130 elements, 256 or 257 rows) from this table, so it
has to be right."""
import functools

import numpy as np
import pytest

import fan_meshes as F
import meshio
import oracle_py as O
from test_gpu_fans import SURF

PHYS = dict(l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)
VARIANTS = ("free", "mixed")


def oracle_problem(mesh, variant):
    xy, tri, bseg, bgroup = mesh
    surf = SURF[:1] if variant == "free" else SURF
    return O.Problem(meshio.Mesh(xy, tri, bseg, bgroup), [meshio.Surface(**s) for s in surf],
                     **PHYS)


@functools.lru_cache(maxsize=None)
def space(mesh_id, k, variant):
    orc = oracle_problem(F.pk_make(mesh_id, "zero" if variant == "free" else "alt"), variant)
    return orc, O.PkSpace(orc, k)


def row_lengths(orc, S):
    """stored entries per row of the oracle's Jacobian pattern (the diagonal included)"""
    op = orc.operator(O.OP_PB, flux=orc.flux(), mask=np.zeros(S.nn, dtype=np.uint8))
    return np.diff(S.jacobian(op, np.zeros(S.nn)).indptr)


@pytest.mark.parametrize("mesh_id,k", F.PK_CASES)
def test_table_figures_are_the_oracles(mesh_id, k):
    _, _, _, per_degree, nt, per_node, _ = F.pk_entry(mesh_id)
    orc, S = space(mesh_id, k, "free")
    lens = row_lengths(orc, S)
    got = (S.nn, int(lens.max())), S.enode.shape[0], int(np.bincount(S.enode.ravel()).max())
    print(f"{mesh_id} P{k}: (nodes, longest row), elements, elements at a node = {got}")
    assert got == (per_degree[k], nt, per_node)
    assert lens.max() <= 63


def test_rows_that_separate_the_split_states():
    """the gather split needs a longest row above 32 slots and a median 256-row block of at most
    half of it: in wheel_on_chain exactly one row (the hub's, 61 slots) is longer than 32 slots, and
    every other row has at most 30, so whichever block holds the hub is the only long one however
    the layout orders the rows; the rows left of the last quadrilateral are the chain's, 14 slots
    at P2 and 25 at P3"""
    for mesh_id, k, chain in (("wheel_on_chain_20_100", 2, 14), ("wheel_on_chain_10_100", 3, 25),
                              ("wheel_on_chain_20_31", 2, 14), ("wheel_on_chain_10_16", 3, 25)):
        orc, S = space(mesh_id, k, "free")
        lens = row_lengths(orc, S)
        srt = np.sort(lens)
        assert srt[-1] == 61 and srt[-2] <= 30
        n = F.pk_entry(mesh_id)[2][1]
        assert lens[S.xy[:, 0] < 2.0 * (n - 1) - 1e-9].max() == chain


@pytest.mark.parametrize("gen,args,k,slots", F.PK_REFUSED)
def test_refused_meshes_have_the_stated_longest_row(gen, args, k, slots):
    orc = oracle_problem(gen(*args), "free")
    S = O.PkSpace(orc, k)
    assert row_lengths(orc, S).max() == slots > 63


@pytest.mark.parametrize("mesh_id,k", F.PK_CASES)
def test_boundary_variants(mesh_id, k):
    """"free" constrains nothing; "mixed" constrains at least one node, and never the interior hub
    of a mesh that has one"""
    orc, S = space(mesh_id, k, "free")
    assert not any(S.mask(f).any() for f in range(3))
    orc, S = space(mesh_id, k, "mixed")
    hub = int(np.argmax(row_lengths(orc, S)))
    for f in range(3):
        m = S.mask(f)
        assert m.any()
        if F.pk_entry(mesh_id)[6]:
            assert m[hub] == 0
