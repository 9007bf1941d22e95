"""Shared by tests/test_asm_regular_host.py and tests/test_gpu_asm_regular.py: the structured grid
mesh of the regular-walk tests, the numpy restatement of the kernel's wave vote, and the problem
data of the grid.  Plain numpy; nothing here needs a GPU.

A row is regular when its rowmeta says 7 slots (six neighbours), closed, no break bit; a 64-row
chunk (one wave of the assembly) is regular when every one of its rows is -- the last chunk may be
partial, and then only its live rows vote."""
import numpy as np

import fan_meshes as F

SURF = [dict(cb=1, cflux=0.3, cpot=0.0, pb=1, pflux=-0.2, pconc=0.0, mb=1, mflux=0.1, mconc=0.0),
        dict(cb=0, cflux=0.0, cpot=1.0, pb=0, pflux=0.0, pconc=0.05, mb=0, mflux=0.0,
             mconc=0.07)]
PHYS = dict(l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)


def grid_mesh(n, groups="alt"):
    """n x n vertices, (n - 1)^2 cells cut by the diagonal from (i, j) to (i + 1, j + 1): every
    interior vertex is a closed fan of six neighbours.  The vertices are shifted a little (smoothly,
    by less than a tenth of a cell) so that no two elements are congruent; y > 0."""
    j, i = np.meshgrid(np.arange(n), np.arange(n))
    i, j = i.ravel().astype(np.float64), j.ravel().astype(np.float64)
    x = i + 0.08 * np.sin(0.9 * i + 1.7 * j)
    y = 2.0 + j + 0.08 * np.cos(1.3 * i - 0.6 * j)
    v = lambda a, b: a * n + b
    tri = []
    for a in range(n - 1):
        for b in range(n - 1):
            tri.append((v(a, b), v(a + 1, b), v(a + 1, b + 1)))
            tri.append((v(a, b), v(a + 1, b + 1), v(a, b + 1)))
    return F._finish(np.stack([x, y], axis=1), tri, groups)


def regular_rows(rowmeta):
    m = np.asarray(rowmeta, dtype=np.uint64)
    return ((m & np.uint64(63)) == 7) & (((m >> np.uint64(6)) & np.uint64(1)) == 1) & \
        ((m >> np.uint64(8)) == 0)


def chunk_classes(L):
    """per 64-row chunk of a P.Layout: (rows of the chunk, regular rows among them)"""
    reg = regular_rows(L.rowmeta)
    assert L.nchunks == (L.n_owned + 63) // 64
    rows = np.array([min(64, L.n_owned - 64 * c) for c in range(L.nchunks)], dtype=np.int64)
    cnt = np.array([int(reg[64 * c:64 * c + 64].sum()) for c in range(L.nchunks)], dtype=np.int64)
    return rows, cnt


def regular_info(L):
    """the numpy restatement of pnp_asm_regular_info for one layout"""
    rows, cnt = chunk_classes(L)
    return {"chunks": int(L.nchunks), "regular_chunks": int(np.count_nonzero(cnt == rows))}


def grid_has_all_three(L):
    """a fully regular chunk, a mixed chunk (regular and other rows) and a partial last chunk"""
    rows, cnt = chunk_classes(L)
    return bool(np.any(cnt == rows) and np.any((cnt > 0) & (cnt < rows)) and rows[-1] < 64)


# the smallest n >= 40 whose one-rank layout shows all three (test_asm_regular_host.py checks that
# it is the smallest)
GRID_N = 41


def grid_state(nv, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1, 1, nv), 0.06 * rng.uniform(0.5, 1.5, nv),
                           0.06 * rng.uniform(0.5, 1.5, nv)])
