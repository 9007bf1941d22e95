"""What the sweep, SpMV and assembly kernels take on trust from the derived layout
(csrc/layout_derive.cc, uploaded by the context at creation), checked on the host (no GPU) through
pnp_layout_derived: the triangular split with its lane order, the LDS sweep lists, the LDS SpMV
lists, the block orders and the row lists.  Every expectation is restated here from the layout's
colidx / rowmeta / rowcolor, not taken from the code under test.

Layouts: every mesh of fan_meshes.TABLE at 1 and 2 ranks, and pore_pnp refined once at 3 ranks; the
knobs at their defaults and each one off.  A knob's case checks the blocks that knob reaches and
that the others are the default's arrays."""
import os
import types

import numpy as np
import pytest

import fan_meshes as F
import pnp_amd as P
from conftest import DATA

KNOBS = ("split_sort", "blkmap", "spmv_lds", "list_own_last", "halo_overlap")
SPLIT = ("lperm", "uperm", "lpinv", "upinv", "llen", "ulen", "ldl", "lchunk_len", "lchunk_off",
         "lcolidx", "lsrc", "uchunk_len", "uchunk_off", "ucolidx", "usrc")
SWEEP = ("lsx_ptr", "lsx_list", "lsx_idx", "usx_ptr", "usx_list", "usx_idx")
SPMV = ("uptr", "ulist", "uown", "lidx")
ROWS = ("rowoff", "rowcol")
HALO = ("blk_int", "blk_bnd")


def _mesh(name):
    if name == "pore_pnp_r1":
        return P.Mesh.read_gmsh(os.path.join(DATA, "pore_pnp", "pore.msh")).refine(1)
    t = F.entry(name)
    return P.Mesh(*t[1](*t[2]))


LAYOUTS = [(t[0], r, n) for t in F.TABLE for n in (1, 2) for r in range(n)]
LAYOUTS += [("pore_pnp_r1", r, 3) for r in range(3)]
_cache = {}


def layout(name, rank, nranks):
    """(Layout, its rows restated, derive() with the default knobs), built once per layout"""
    key = (name, rank, nranks)
    if key not in _cache:
        L = P.Layout(_mesh(name), rank, nranks)
        _cache[key] = (L, restate(L), L.derive(split_sort=1))
    return _cache[key]


def restate(L):
    """per owned row, from colidx / rowmeta / rowcolor alone: its live columns in slot order, and
    its sweep neighbours below (low) and above (up) it as (column, slot)"""
    no = L.n_owned
    R = types.SimpleNamespace(cols=[], low=[], up=[], ghost=np.zeros(no, bool))
    for i in range(no):
        cols = L.row_cols(i)
        assert cols[0] == i
        R.cols.append(cols)
        nb = [(j, s) for s, j in enumerate(cols) if s >= 1 and j < no and j != i and
              L.rowcolor[j] != L.rowcolor[i]]
        R.low.append([(j, s) for j, s in nb if j < i])
        R.up.append([(j, s) for j, s in nb if j > i])
        R.ghost[i] = any(j >= no for j in cols[1:])
    return R


def same(d, ref, names):
    for n in names:
        assert np.array_equal(getattr(d, n), getattr(ref, n)), n


def check_split(L, R, d, sort):
    no, nch, npos = L.n_owned, L.nchunks, 64 * L.nchunks
    assert d.npos == npos and all(len(getattr(d, n)) == npos for n in SPLIT[:7])
    base = 64 * (np.arange(npos) // 64)
    lane = np.arange(npos) % 64
    for side, perm, pinv, ln8, cl, co, col, src, nbrs, first in (
            ("L", d.lperm, d.lpinv, d.llen, d.lchunk_len, d.lchunk_off, d.lcolidx, d.lsrc, R.low, 0),
            ("U", d.uperm, d.upinv, d.ulen, d.uchunk_len, d.uchunk_off, d.ucolidx, d.usrc, R.up, 1)):
        row = base + perm  # the row at each position
        # a permutation of the lanes of each chunk, inside a colour segment; identity on padding
        assert np.array_equal(np.sort(perm.reshape(nch, 64), axis=1),
                              np.tile(np.arange(64), (nch, 1)))
        assert np.array_equal(row[no:], np.arange(no, npos))
        assert np.all(row[:no] < no)
        assert np.array_equal(L.rowcolor[row[:no]], L.rowcolor[:no])
        assert np.array_equal(pinv[row], lane)  # the inverse
        if not sort:
            assert np.array_equal(perm, lane)
        live = np.array([first + len(nbrs[r]) if r < no else first for r in row])
        assert np.array_equal(ln8, live)
        # longest first inside a segment (positions of one colour in one chunk)
        seg = (np.arange(no)[1:] // 64 == np.arange(no)[:-1] // 64) & \
            (L.rowcolor[1:no] == L.rowcolor[:no - 1])
        if sort:
            assert np.all(live[1:no][seg] <= live[:no - 1][seg])
        # chunk lengths and offsets
        want = np.maximum(first, live.reshape(nch, 64).max(axis=1)) if nch else np.zeros(0, int)
        assert np.array_equal(cl, want)
        assert np.array_equal(co, np.concatenate([[0], np.cumsum(64 * want)]))
        assert len(col) == len(src) == co[-1]
        # every position's slots: the row's sweep neighbours once each, in slot order, after the
        # diagonal slot in U; padding points at the row with source -1
        for p in range(npos):
            r, ch = int(row[p]), p // 64
            got_c = col[co[ch] + 64 * np.arange(cl[ch]) + p % 64]
            got_s = src[co[ch] + 64 * np.arange(cl[ch]) + p % 64]
            exp_c = np.full(cl[ch], r)
            exp_s = np.full(cl[ch], -1)
            if r < no:
                if first:
                    exp_s[0] = r << 6
                for k, (j, s) in enumerate(nbrs[r]):
                    exp_c[first + k], exp_s[first + k] = j, r << 6 | s
            assert np.array_equal(got_c, exp_c) and np.array_equal(got_s, exp_s), (side, p)
    assert np.array_equal(d.ldl, d.upinv[base + d.lperm])
    assert d.lslots == d.lchunk_off[-1] and d.uslots == d.uchunk_off[-1]
    assert d.lslots_live == sum(len(x) for x in R.low)
    assert d.uslots_live == no + sum(len(x) for x in R.up)
    # tests/test_gpu_ilu_lds.py's identity (one rank: no ghost column), here with the ghost slots
    ghosts = sum(1 for cols in R.cols for j in cols[1:] if j >= no)
    assert d.lslots_live + d.uslots_live + 2 * L.color_conflicts + ghosts == L.nblocks


def check_sweep_lists(L, d):
    assert d.sweep_usable == 1  # these layouts fit
    no = L.n_owned
    blocks = [(r0, min(L.color_ptr[c + 1], r0 + 256)) for c in range(L.ncolors)
              for r0 in range(L.color_ptr[c], L.color_ptr[c + 1], 256)]
    assert d.n_sweep_blocks == len(blocks)
    longest = 0
    for ptr, lst, idx, cl, co, col, src, first, n in (
            (d.lsx_ptr, d.lsx_list, d.lsx_idx, d.lchunk_len, d.lchunk_off, d.lcolidx, d.lsrc, 0,
             d.lsx_entries),
            (d.usx_ptr, d.usx_list, d.usx_idx, d.uchunk_len, d.uchunk_off, d.ucolidx, d.usrc, 1,
             d.usx_entries)):
        assert len(ptr) == len(blocks) + 1 and ptr[0] == 0 and ptr[-1] == len(lst) == n
        assert len(idx) == len(col)
        seen = np.zeros(len(col), bool)
        for b, (r0, r1) in enumerate(blocks):
            seg = lst[ptr[b]:ptr[b + 1]]
            assert np.all(np.diff(seg) > 0)  # sorted, unique
            longest = max(longest, len(seg))
            pos = np.concatenate([co[p // 64] + 64 * np.arange(first, cl[p // 64]) + p % 64
                                  for p in range(r0, r1)] + [np.zeros(0, int)]).astype(int)
            seen[pos] = True
            live = src[pos] != -1
            assert np.all(idx[pos][~live] == 0xFFFF) and np.all(idx[pos][live] < len(seg))
            assert np.array_equal(seg[idx[pos][live]], col[pos][live])
            assert set(seg) == set(col[pos][live])  # nothing staged that no slot reads
        # the rest: slots of padding positions, and the U diagonal slot
        assert np.all(idx[~seen] == 0xFFFF)
        if first:
            assert np.all(idx[(co[:-1][:, None] + np.arange(64)[None, :]).ravel()] == 0xFFFF)
    assert d.sx_max == longest
    assert np.all(d.lsx_list < no) and np.all(d.usx_list < no)


def check_spmv_lists(L, R, d, own_last):
    assert d.spmv_usable == 1
    no, nblk = L.n_owned, (L.n_owned + 255) // 256
    assert d.nblk == nblk and len(d.uptr) == nblk + 1 and len(d.uown) == nblk
    assert len(d.lidx) == L.nslots and d.uptr[0] == 0 and d.uptr[-1] == len(d.ulist)
    for b in range(nblk):
        rows = np.arange(256 * b, min(no, 256 * b + 256))
        seg = d.ulist[d.uptr[b]:d.uptr[b + 1]]
        pos = np.concatenate([L.chunk_off[i // 64] + 64 * np.arange(L.chunk_len[i // 64]) + i % 64
                              for i in rows]).astype(int)
        own = np.concatenate([np.full(L.chunk_len[i // 64], i) for i in rows])
        slot = np.concatenate([np.arange(L.chunk_len[i // 64]) for i in rows])
        assert np.array_equal(seg[d.lidx[pos]], L.colidx[pos])  # every slot, padding included
        assert len(set(seg)) == len(seg) and set(seg) == set(L.colidx[pos])
        nbr = set(L.colidx[pos][(slot >= 1) & (L.colidx[pos] != own)])
        if own_last:
            assert set(seg[:d.uown[b]]) == nbr and d.uown[b] == len(nbr)
        else:
            assert d.uown[b] == len(seg) and np.all(np.diff(seg) > 0)
    sizes = np.diff(d.uptr)
    assert d.umax == (sizes.max() if nblk else 0) and d.unmax == (d.uown.max() if nblk else 0)


def check_blocks(L, R, d, blkmap_on, halo_on):
    no, nblk = L.n_owned, (L.n_owned + 255) // 256
    if blkmap_on:
        assert d.n_blkmap == nblk and np.array_equal(np.sort(d.blkmap), np.arange(nblk))
        # one spatial slice of every colour after the other: the block's place inside its colour
        c = L.rowcolor[256 * np.arange(nblk)].astype(int)
        lo, hi = L.color_ptr[c].astype(float), L.color_ptr[c + 1].astype(float)
        key = (256 * np.arange(nblk) - lo) / np.maximum(1.0, hi - lo)
        assert np.all(np.diff(key[d.blkmap]) >= 0)
        order = d.blkmap
    else:
        assert d.n_blkmap == 0 and len(d.blkmap) == 0
        order = np.arange(nblk)
    if not halo_on:
        assert d.halo_usable == 0 and d.n_blk_int == 0 and d.n_blk_bnd == 0
        return
    assert d.halo_usable == 1
    bnd = np.array([R.ghost[256 * b:256 * b + 256].any() for b in order], bool)
    assert np.array_equal(d.blk_int, order[~bnd]) and np.array_equal(d.blk_bnd, order[bnd])
    assert d.n_blk_int + d.n_blk_bnd == nblk
    if L.n_ghost == 0:
        assert d.n_blk_bnd == 0


def check_rows(L, R, d):
    lens = np.array([len(c) for c in R.cols], int)
    assert np.array_equal(d.rowoff, np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(d.rowcol, np.concatenate(R.cols + [np.zeros(0, int)]))


@pytest.mark.parametrize("off", (None,) + KNOBS)
@pytest.mark.parametrize("name,rank,nranks", LAYOUTS, ids=[f"{n}-{r}of{k}" for n, r, k in LAYOUTS])
def test_derived_layout(name, rank, nranks, off):
    L, R, ref = layout(name, rank, nranks)
    d = ref if off is None else L.derive(**{off: 0})
    if off in (None, "split_sort"):
        check_split(L, R, d, sort=off is None)
        check_sweep_lists(L, d)
    else:
        same(d, ref, SPLIT + SWEEP)
    if off == "spmv_lds":
        assert d.spmv_usable == 0 and d.umax == 0 and d.unmax == 0
        assert all(len(getattr(d, n)) == 0 for n in SPMV)
    elif off in (None, "list_own_last"):
        check_spmv_lists(L, R, d, own_last=off is None)
    else:
        same(d, ref, SPMV)
    if off in (None, "blkmap", "halo_overlap"):
        check_blocks(L, R, d, blkmap_on=off != "blkmap", halo_on=off != "halo_overlap")
    else:
        same(d, ref, ("blkmap",) + HALO)
    if off is None:
        check_rows(L, R, d)
        assert d.xcd_remap == 0 and L.derive(xcd_remap=1).xcd_remap == 1
        assert np.array_equal(d.fseg[:, 3], d.fseg_group) and np.all(d.fseg[:, :3] >= 0)
        a, c = d.fseg[:, 0], d.fseg[:, 1]  # this rank owns the segment's lower global vertex
        assert np.all(np.where(L.l2g[a] < L.l2g[c], a, c) < L.n_owned)
    else:
        same(d, ref, ROWS + ("fseg", "fseg_group"))


def test_knobs_from_the_environment(monkeypatch):
    """no knob given: a context's reading of the environment, each variable with its own parsing"""
    L, _, ref = layout("diamond_chain_171", 0, 2)
    everything = SPLIT + SWEEP + SPMV + HALO + ("blkmap",)
    for knob in KNOBS:
        monkeypatch.setenv("PNP_" + knob.upper(), "0")
        same(L.derive(), L.derive(**{knob: 0}), everything)
        monkeypatch.delenv("PNP_" + knob.upper())
    same(L.derive(), ref, everything)
    monkeypatch.setenv("PNP_XCD_REMAP", "1")
    assert L.derive().xcd_remap == 1
    # "00" and "off": PNP_SPLIT_SORT and PNP_LIST_OWN_LAST look at the first character, the others
    # at atoi
    monkeypatch.delenv("PNP_XCD_REMAP")
    monkeypatch.setenv("PNP_SPLIT_SORT", "off")
    monkeypatch.setenv("PNP_BLKMAP", "off")
    d = L.derive()
    assert np.array_equal(d.lperm, ref.lperm) and d.n_blkmap == 0


def _raw_layout(mesh, rank, nranks):
    """pnp_layout_build itself (Layout goes through pnp_layout_build_pk)"""
    import ctypes as C
    buf, m, v = C.c_void_p(), mesh.c(), P._Layout()
    assert P.lib().pnp_layout_build(C.byref(m), rank, nranks, C.byref(buf)) == 0
    assert P.lib().pnp_layout_view(buf, C.byref(v)) == 0
    out = (v.n_owned, v.n_ghost, v.ncolors, v.nchunks, v.max_slots, v.nslots, v.nblocks,
           np.ctypeslib.as_array(v.colidx, (v.nslots,)).copy(),
           np.ctypeslib.as_array(v.rowmeta, (v.n_owned,)).copy(),
           np.ctypeslib.as_array(v.l2g, (v.n_owned + v.n_ghost,)).copy())
    P.lib().pnp_layout_free(buf)
    return out


@pytest.mark.parametrize("name,rank,nranks", [("pinwheel_4_3_2", 0, 1), ("diamond_chain_86", 1, 2)])
def test_build_pk_degree_1_is_layout_build(name, rank, nranks):
    mesh = _mesh(name)
    L = P.Layout(mesh, rank, nranks, degree=1)
    raw = _raw_layout(mesh, rank, nranks)
    assert raw[:7] == (L.n_owned, L.n_ghost, L.ncolors, L.nchunks, L.max_slots, L.nslots, L.nblocks)
    assert np.array_equal(raw[7], L.colidx) and np.array_equal(raw[8], L.rowmeta)
    assert np.array_equal(raw[9], L.l2g)


PK = [(t[0], k) for t in F.PK_TABLE for k in sorted(t[3])]


@pytest.mark.parametrize("name,degree", PK, ids=[f"{n}-P{k}" for n, k in PK])
def test_build_pk_row_counts(name, degree):
    t = F.pk_entry(name)
    rows, slots = t[3][degree]
    L = P.Layout(P.Mesh(*t[1](*t[2])), 0, 1, degree=degree)
    assert (L.n_owned, L.n_ghost, L.max_slots) == (rows, 0, slots)
    d = L.derive(split_sort=1)  # P_k: no elements in the node mesh, so no P1 flux segment
    assert d.nfseg == 0 and d.rowoff[-1] == L.nblocks
    assert d.lslots_live + d.uslots_live + 2 * L.color_conflicts == L.nblocks
