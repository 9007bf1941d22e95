"""Small triangle meshes, generated in the test, whose vertex fans the committed meshes never have:
pinch vertices (several open fans around one vertex, so the row's fan carries break bits), open and
closed fans up to the supported maximum of 30 neighbours, and systems of a handful of rows.  Plain
numpy; tests/test_fan_layout_host.py walks them on the host, tests/test_gpu_fan_walks.py assembles
them on the GPU.

Every generator returns (xy, tri, bseg, bgroup): CCW triangles, every boundary edge once in bseg as
(low vertex, high vertex) in sorted order, and bgroup by one of two policies -- groups="zero" (one
surface) or groups="alt" (segment index % 2).  All coordinates have y > 0 (the tests run with
cylindrical = 1, as the wheel of tests/test_gpu_fans.py).
"""
import numpy as np

Y0 = 3.0  # the hub's / the chain's height


def _finish(xy, tri, groups):
    xy = np.asarray(xy, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    a, b, c = xy[tri[:, 0]], xy[tri[:, 1]], xy[tri[:, 2]]
    area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    assert np.all(area2 > 0) and np.all(xy[:, 1] > 0)
    count = {}
    for t in tri:
        for k in range(3):
            e = (int(min(t[k], t[(k + 1) % 3])), int(max(t[k], t[(k + 1) % 3])))
            count[e] = count.get(e, 0) + 1
    assert max(count.values()) <= 2
    bseg = np.array(sorted(e for e, n in count.items() if n == 1), dtype=np.int32)
    assert groups in ("zero", "alt")
    bgroup = np.arange(len(bseg)) % 2 if groups == "alt" else np.zeros(len(bseg))
    return xy, tri, bseg, bgroup.astype(np.int32)


def one_triangle(groups="zero"):
    """3 vertices, 1 element: every row is an open fan of two neighbours"""
    return _finish([[0.0, Y0], [1.3, Y0 + 0.2], [0.4, Y0 + 1.1]], [(0, 1, 2)], groups)


def split_triangle(groups="zero"):
    """a triangle with its centroid (vertex 3) joined to the corners: one closed fan of 3, the
    shortest closed fan there is"""
    xy = np.array([[0.0, Y0], [1.3, Y0 + 0.2], [0.4, Y0 + 1.1]])
    xy = np.vstack([xy, xy.mean(axis=0)])
    return _finish(xy, [(3, 0, 1), (3, 1, 2), (3, 2, 0)], groups)


def _radius(j):
    """rim radii that vary a little, so no two elements are congruent"""
    return 1.0 + 0.15 * np.cos(2.3 * j + 0.7) + 0.01 * j


def pinwheel(fans, groups="zero"):
    """hub 0 with len(fans) open fans around it, in CCW order: fan f has fans[f] elements and
    fans[f] + 1 rim vertices of its own; half an element's angle of gap follows every fan.  The
    hub's row lists the fans in this order, so its break bits sit after slots fans[0] + 1,
    fans[0] + fans[1] + 2, ..."""
    fans = list(fans)
    assert len(fans) >= 2 and min(fans) >= 1
    unit = 2 * np.pi / (sum(fans) + 0.5 * len(fans))
    xy, tri = [[0.0, Y0]], []
    angle = 0.1
    for n in fans:
        first = len(xy)
        for k in range(n + 1):
            r = _radius(len(xy))
            xy.append([r * np.cos(angle + k * unit), Y0 + r * np.sin(angle + k * unit)])
        tri += [(0, first + k, first + k + 1) for k in range(n)]
        angle += (n + 0.5) * unit
    return _finish(xy, tri, groups)


def half_wheel(k, groups="zero"):
    """a boundary hub 0 with one open fan of k neighbours (k - 1 elements) over 200 degrees"""
    assert k >= 3
    ang = 0.1 + np.deg2rad(200.0) * np.arange(k) / (k - 1)
    r = _radius(1 + np.arange(k))
    xy = np.vstack([[0.0, Y0], np.c_[r * np.cos(ang), Y0 + r * np.sin(ang)]])
    return _finish(xy, [(0, 1 + j, 2 + j) for j in range(k - 1)], groups)


def diamond_chain(n, groups="zero"):
    """n quadrilaterals joined corner to corner along x: joints 3q (and 3n), top 3q + 1, bottom
    3q + 2.  Even quadrilaterals are split by the diagonal through the joints, odd ones by the
    other, so 3n + 1 vertices, and every inner joint is a pinch vertex with two open fans (5
    neighbours, one break).  The top vertex's height varies with q % 3."""
    assert n >= 1
    xy = np.zeros((3 * n + 1, 2))
    tri = []
    for q in range(n):
        j0, top, bot, j1 = 3 * q, 3 * q + 1, 3 * q + 2, 3 * q + 3
        xy[j0] = (2.0 * q, Y0)
        xy[top] = (2.0 * q + 1.0, Y0 + 0.8 + 0.15 * (q % 3))
        xy[bot] = (2.0 * q + 0.9, Y0 - 0.7)
        xy[j1] = (2.0 * q + 2.0, Y0)
        if q % 2 == 0:
            tri += [(j0, j1, top), (j0, bot, j1)]
        else:
            tri += [(j0, bot, top), (j1, top, bot)]
    return _finish(xy, tri, groups)


# (id, generator, argument tuple, rows, max_slots of the layout, rows with break bits, most break
# bits in one row).  max_slots selects the walk: <= 9 the gather-all walk with 9 column registers
# (FANR 9), <= 12 the pipelined walk with 12 (FANR 12), beyond it index loads in the walk (FANR 0).
TABLE = [
    ("one_triangle", one_triangle, (), 3, 3, 0, 0),
    ("split_triangle", split_triangle, (), 4, 4, 0, 0),
    ("pinwheel_1_1", pinwheel, ((1, 1),), 5, 5, 1, 1),
    ("pinwheel_1_1_1", pinwheel, ((1, 1, 1),), 7, 7, 1, 2),
    ("pinwheel_2_2", pinwheel, ((2, 2),), 7, 7, 1, 1),
    # a break at the slot where the gather-all Jacobian walk issues its second batch of gathers
    # (SPLIT - 2 = 4), and the last fan a single element
    ("pinwheel_3_1", pinwheel, ((3, 1),), 7, 7, 1, 1),
    # the longest fan of the gather-all walk (8 neighbours): breaks after slots 2 and 6
    ("pinwheel_1_3_1", pinwheel, ((1, 3, 1),), 9, 9, 1, 2),
    ("pinwheel_3_1_2", pinwheel, ((3, 1, 2),), 10, 10, 1, 2),
    # the longest fan with 12 column registers (11 neighbours)
    ("pinwheel_4_1_3", pinwheel, ((4, 1, 3),), 12, 12, 1, 2),
    ("pinwheel_4_3_2", pinwheel, ((4, 3, 2),), 13, 13, 1, 2),
    ("pinwheel_1_1_1_1_1_2", pinwheel, ((1, 1, 1, 1, 1, 2),), 14, 14, 1, 5),
    ("pinwheel_13_1_12", pinwheel, ((13, 1, 12),), 30, 30, 1, 2),
    ("half_wheel_12", half_wheel, (12,), 13, 13, 0, 0),
    ("half_wheel_30", half_wheel, (30,), 31, 31, 0, 0),  # the supported maximum
    ("diamond_chain_21", diamond_chain, (21,), 64, 6, 20, 1),    # one full SELL chunk
    ("diamond_chain_85", diamond_chain, (85,), 256, 6, 84, 1),   # one full workgroup
    ("diamond_chain_86", diamond_chain, (86,), 259, 6, 85, 1),   # a last workgroup of 3 live rows
    ("diamond_chain_171", diamond_chain, (171,), 514, 6, 170, 1),
]
IDS = [t[0] for t in TABLE]


def entry(mesh_id):
    return TABLE[IDS.index(mesh_id)]


def make(mesh_id, groups="zero"):
    _, gen, args, *_ = entry(mesh_id)
    return gen(*args, groups=groups)


def walk_class(max_slots):
    """the FANR of launch_assemble / launch_jac_apply for a layout's max_slots"""
    return 9 if max_slots <= 9 else (12 if max_slots <= 12 else 0)
