"""The fan convention the P1 kernels rely on, checked on the host (no GPU): for the meshes of
tests/fan_meshes.py -- pinch vertices, fans of up to 30 neighbours, systems of 3 rows -- the rows
that pnp_layout_build hands the kernels (colidx / rowmeta), walked as k_assemble, k_assemble_ga,
k_jac_apply and k_mass_apply walk them, give exactly the mesh's triangles.

The walk of a row i: slots 1 .. len-1; the successor of slot s is s + 1, or slot 1 when the fan is
closed and s is the last slot; no element where bit 8 + s of rowmeta is set (a fan break) or where
there is no successor.  The global triples (i, v_s, v_t) of all owned rows of all ranks must be the
mesh's CCW triangles in their three rotations, each once."""
import numpy as np
import pytest

import fan_meshes as F
import pnp_amd as P

BREAK_BITS = np.uint64(((1 << 31) - 1) << 8)  # bits 8 .. 38: slots 0 .. 30


def wheel(k):
    from test_gpu_fans import wheel as w
    return w(k)


# fan_meshes.TABLE and the closed 30-spoke hub of the wheel test (hub 0: 31 slots, no breaks)
CASES = [(t[0], (lambda t=t: t[1](*t[2])), t[3], t[4], t[5], t[6]) for t in F.TABLE]
CASES.append(("wheel_30", lambda: wheel(30), 91, 31, 0, 0))


def walk(mesh, nranks, use_breaks=True):
    """(sorted triples of the walk over every rank's owned rows, max_slots, break bits per row)"""
    triples, max_slots, breaks, owned = [], 0, [], 0
    for r in range(nranks):
        L = P.Layout(mesh, r, nranks)
        max_slots = max(max_slots, L.max_slots)
        owned += L.n_owned
        for i in range(L.n_owned):
            meta = int(L.rowmeta[i])
            n, closed = meta & 63, (meta >> 6) & 1
            assert n == L.row_len(i) and 2 <= n <= 31
            cols = L.row_cols(i)
            assert cols[0] == i  # slot 0 is the row itself
            breaks.append(bin(meta & int(BREAK_BITS)).count("1"))
            for s in range(1, n):
                t = s + 1 if s + 1 < n else (1 if closed else -1)
                if t < 0 or (use_breaks and (meta >> (8 + s)) & 1):
                    continue
                triples.append((int(L.l2g[i]), int(L.l2g[cols[s]]), int(L.l2g[cols[t]])))
    assert owned == mesh.nv
    return sorted(triples), max_slots, np.array(breaks)


def rotations(tri):
    return sorted((int(t[k]), int(t[(k + 1) % 3]), int(t[(k + 2) % 3])) for t in tri
                  for k in range(3))


@pytest.mark.parametrize("nranks", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_walk_gives_the_mesh_triangles(case, nranks):
    name, gen, rows, max_slots, break_rows, most = case
    xy, tri, bseg, bgroup = gen()
    mesh = P.Mesh(xy, tri, bseg, bgroup)
    assert mesh.nv == rows
    triples, slots, breaks = walk(mesh, nranks)
    assert triples == rotations(tri)
    assert slots == max_slots
    assert np.count_nonzero(breaks) == break_rows and breaks.max() == most
    if break_rows:
        # the break bits matter: a walk that ignores them invents elements across the gaps
        wrong, _, _ = walk(mesh, nranks, use_breaks=False)
        assert len(wrong) == len(triples) + breaks.sum() and wrong != triples


@pytest.mark.parametrize("groups", ["zero", "alt"])
def test_generators_list_every_boundary_edge_once(groups):
    for name, gen, args, rows, *_ in F.TABLE:
        xy, tri, bseg, bgroup = gen(*args, groups=groups)
        assert xy.shape == (rows, 2) and tri.dtype == np.int32 and bseg.dtype == np.int32
        assert np.all(bseg[:, 0] < bseg[:, 1])
        assert [tuple(b) for b in bseg] == sorted(set(tuple(b) for b in bseg))
        want = np.arange(len(bseg)) % 2 if groups == "alt" else np.zeros(len(bseg))
        np.testing.assert_array_equal(bgroup, want)
        assert np.unique(tri).size == rows


def test_thirty_one_neighbours_are_rejected():
    xy, tri, bseg, bgroup = F.half_wheel(31)
    with pytest.raises(P.PnpError) as e:
        P.Layout(P.Mesh(xy, tri, bseg, bgroup), 0, 1)
    assert e.value.code == P.E_MESH == -7
    assert "degree 31 (max supported 30)" in str(e.value)
