"""The regular walk's host side (no GPU): the chunk counts of pnp_asm_regular_info against a numpy
restatement of the kernel's wave vote, the knob and the call in the header, the library and the
Python package.  The behaviour on the GPU is in tests/test_gpu_asm_regular.py.

pnp_asm_regular_info takes a context, which needs a GPU; pnp_layout_regular_info runs the same host
routine (mesh.h regular_chunks) on the layout pnp_layout_build makes, which is the layout the
context builds.  P.Layout carries its result as regular_info; the GPU test compares the context's
answer with it."""
import os
import re

import numpy as np
import pytest

import asm_regular_cases as R
import fan_meshes as F
import pnp_amd as P
from conftest import DATA

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ("cylinder_k0", "pore_small_k0", "pore_pnp_k0", "sphere_k0", "one_wall_k1")


def golden_mesh(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return P.Mesh(z["xy"], z["tri"], z["bseg"], z["bgroup"])


def check(mesh, nranks):
    """the library's counts equal the restated vote on every rank; returns the summed counts"""
    total = {"chunks": 0, "regular_chunks": 0}
    for r in range(nranks):
        L = P.Layout(mesh, r, nranks)
        want = R.regular_info(L)
        assert L.regular_info == want, (r, nranks, L.regular_info, want)
        assert 0 <= want["regular_chunks"] <= want["chunks"] == L.nchunks
        for k in total:
            total[k] += want[k]
    return total


@pytest.mark.parametrize("nranks", [1, 2])
@pytest.mark.parametrize("mesh_id", F.IDS)
def test_counts_on_the_fan_meshes(mesh_id, nranks):
    xy, tri, bseg, bgroup = F.make(mesh_id, "zero")
    check(P.Mesh(xy, tri, bseg, bgroup), nranks)


@pytest.mark.parametrize("nranks", [1, 2])
@pytest.mark.parametrize("name", GOLDENS)
def test_counts_on_the_goldens(name, nranks):
    t = check(golden_mesh(name), nranks)
    print(name, nranks, t)


def test_a_chunk_with_one_irregular_row_is_not_regular():
    """the restatement itself, on hand-made rowmeta: 7 slots closed no break is regular; an open
    fan, another length, a break bit are not"""
    ok = np.uint64(7 | 64)
    rows = np.array([ok, np.uint64(7), np.uint64(6 | 64), np.uint64(8 | 64),
                     ok | np.uint64(1 << (8 + 3)), ok | np.uint64(1 << 38)], dtype=np.uint64)
    np.testing.assert_array_equal(R.regular_rows(rows), [True, False, False, False, False, False])


def test_grid_is_the_smallest_with_a_regular_a_mixed_and_a_partial_chunk():
    seen = {}
    for n in range(40, R.GRID_N + 1):
        L = P.Layout(P.Mesh(*R.grid_mesh(n)))
        assert L.n_owned == n * n
        seen[n] = R.grid_has_all_three(L)
        assert L.regular_info == R.regular_info(L)
    assert seen[R.GRID_N] and not any(v for n, v in seen.items() if n < R.GRID_N), seen
    # interior vertices, and only they, are regular rows
    L = P.Layout(P.Mesh(*R.grid_mesh(R.GRID_N)))
    assert int(R.regular_rows(L.rowmeta).sum()) == (R.GRID_N - 2) ** 2
    for nranks in (1, 2):
        check(P.Mesh(*R.grid_mesh(R.GRID_N)), nranks)


def test_config3_share_of_regular_chunks():
    """bench.py's config 3 (pore_pnp refined 4 times), host layout only: the share of waves that
    take the regular walk (DESIGN.md 4.1 records the figure printed here)"""
    cfg = P.read_config(os.path.join(DATA, "pore_pnp", "pore.cfg"))
    mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(4)
    L = P.Layout(mesh)
    want = R.regular_info(L)
    assert L.regular_info == want
    reg = R.regular_rows(L.rowmeta)
    share = want["regular_chunks"] / want["chunks"]
    print(f"config 3: {L.n_owned} rows, {int(reg.sum())} regular rows, {want['chunks']} chunks, "
          f"{want['regular_chunks']} regular chunks ({100 * share:.2f} %)")
    # 99.1 % of the vertices are interior six-neighbour fans, sorted by slot count inside
    # 4,096-row windows: well over half of the waves must be regular
    assert share > 0.5


def test_call_and_knob_are_in_the_header_the_library_and_the_package():
    syms = P.header_symbols()
    assert "pnp_asm_regular_info" in syms and "pnp_layout_regular_info" in syms
    assert hasattr(P.lib(), "pnp_asm_regular_info") and hasattr(P.lib(), "pnp_layout_regular_info")
    txt = open(P.HEADER).read()
    decl = re.search(r"int pnp_asm_regular_info\(([^)]*)\);", txt).group(1)
    assert [a.split("*")[-1].strip() for a in decl.split(",")] == ["ctx", "chunks",
                                                                  "regular_chunks"]
    # pnp_asm_info keeps its signature
    decl = re.search(r"int pnp_asm_info\(([^)]*)\);", txt).group(1)
    assert [a.split("*")[-1].strip() for a in decl.split(",")] == ["ctx", "full", "reused",
                                                                  "pipelined"]
    assert P.ASM_REGULAR_ENV == "PNP_ASM_REGULAR" and re.search(r"\bPNP_ASM_REGULAR=0/1", txt)
    assert callable(P.Context.asm_regular_info)
