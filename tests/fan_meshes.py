"""Small triangle meshes, generated in the test, whose vertex fans the committed meshes never have:
pinch vertices (several open fans around one vertex, so the row's fan carries break bits), open and
closed fans up to the supported maximum of 30 neighbours, and systems of a handful of rows.  Plain
numpy; tests/test_fan_layout_host.py walks them on the host, tests/test_gpu_fan_walks.py assembles
them on the GPU.  PK_TABLE lists the meshes of the P_k (degree 2, 3) assembly tests
(tests/test_pk_edge_meshes_host.py on the host, tests/test_gpu_pk_edges.py on the GPU).

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


def wheel(k, groups="zero"):
    """an interior hub 0 with one closed fan of k elements and k rim vertices, nothing else (the
    wheel of tests/test_gpu_fans.py has two more rings around it, which P_k rows cannot afford: at
    degree 2 this hub's row already couples to all 3k other nodes)"""
    assert k >= 3
    ang = 0.1 + 2 * np.pi * np.arange(k) / k
    r = _radius(1 + np.arange(k))
    xy = np.vstack([[0.0, Y0], np.c_[r * np.cos(ang), Y0 + r * np.sin(ang)]])
    return _finish(xy, [(0, 1 + j, 1 + (j + 1) % k) for j in range(k)], groups)


def wheel_on_chain(k, n, groups="zero"):
    """diamond_chain(n) with a closed wheel of k rim vertices hung on its last joint 3n: hub 3n + 1
    at (2n + 1.2, Y0), rim vertex 0 the joint itself (at angle pi from the hub), rim vertex j at
    angle pi + 2 pi j / k and _radius(j) as vertex 3n + 1 + j.  The joint is a pinch vertex shared
    by a chain quadrilateral and the wheel; the hub is interior, and its row is the only long one
    among the many short rows of the chain."""
    assert k >= 3
    xy, tri, _, _ = diamond_chain(n)
    hub, joint = 3 * n + 1, 3 * n
    cx = 2.0 * n + 1.2
    j = np.arange(1, k)
    ang = np.pi + 2 * np.pi * j / k
    rim = np.c_[cx + _radius(j) * np.cos(ang), Y0 + _radius(j) * np.sin(ang)]
    xy = np.vstack([xy, [[cx, Y0]], rim])
    ring = [joint] + [hub + int(q) for q in j]
    tri = [tuple(t) for t in tri] + [(hub, ring[q], ring[(q + 1) % k]) for q in range(k)]
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


# The P_k table: (id, generator, argument tuple, {degree: (nodes, longest row)}, elements, most
# elements at one node, hub).  The longest row counts the diagonal, as pnp_info.max_slots does; a
# row holds at most 63 slots.  hub: the node of the longest row is interior, so no boundary variant
# constrains it and its row is compared in full (the boundary hubs of half_wheel and pinwheel sit
# on segments of both groups and are Dirichlet nodes of the "alt" variant).  All figures from the
# CPU oracle's P_k space; tests/test_pk_edge_meshes_host.py holds them to it.
PK_TABLE = [
    # one element: every node in exactly one element; 6 / 10 rows
    ("one_triangle", one_triangle, (), {2: (6, 6), 3: (10, 10)}, 1, 1, False),
    ("split_triangle", split_triangle, (), {2: (10, 10), 3: (19, 19)}, 3, 3, True),
    # a hub in 4 and in 5 elements: one full batch of four incidence codes of the residual gather,
    # and a batch with one live code
    ("half_wheel_5", half_wheel, (5,), {2: (15, 15), 3: (28, 28)}, 4, 4, False),
    ("half_wheel_6", half_wheel, (6,), {2: (18, 18), 3: (34, 34)}, 5, 5, False),
    # 8 and 9 elements; (10) is the longest open fan a P3 row accepts
    ("half_wheel_9", half_wheel, (9,), {2: (27, 27), 3: (52, 52)}, 8, 8, False),
    ("half_wheel_10", half_wheel, (10,), {2: (30, 30), 3: (58, 58)}, 9, 9, False),
    # 63 slots: the longest row the layout carries
    ("half_wheel_21", half_wheel, (21,), {2: (63, 63)}, 20, 20, False),
    ("wheel_10", wheel, (10,), {2: (31, 31), 3: (61, 61)}, 10, 10, True),  # P3's longest closed fan
    ("wheel_20", wheel, (20,), {2: (61, 61)}, 20, 20, True),              # P2's; hub in 20 elements
    ("pinwheel_3_1_2", pinwheel, ((3, 1, 2),), {2: (25, 25), 3: (46, 46)}, 6, 6, False),
    ("pinwheel_1_1_1_1_1_2", pinwheel, ((1, 1, 1, 1, 1, 2),), {2: (34, 34), 3: (61, 61)}, 7, 7,
     False),
    ("diamond_chain_8", diamond_chain, (8,), {2: (65, 14)}, 16, 3, False),    # a SELL chunk + 1 row
    ("diamond_chain_32", diamond_chain, (32,), {2: (257, 14)}, 64, 3, False),  # a workgroup + 1 row
    ("diamond_chain_17", diamond_chain, (17,), {3: (256, 25)}, 34, 3, False),  # one workgroup
    # 128 elements: one full workgroup of the Jacobian's element pass; 130: a last one of 2
    ("diamond_chain_64", diamond_chain, (64,), {2: (513, 14), 3: (961, 25)}, 128, 3, False),
    ("diamond_chain_65", diamond_chain, (65,), {2: (521, 14), 3: (976, 25)}, 130, 3, False),
    # one 61-slot row among short chain rows, 4 / 7 blocks of 256 rows: the gather split runs
    ("wheel_on_chain_20_100", wheel_on_chain, (20, 100), {2: (861, 61)}, 220, 20, True),
    ("wheel_on_chain_10_100", wheel_on_chain, (10, 100), {3: (1561, 61)}, 210, 10, True),
    # 2 blocks: the median block is the long one, no split
    ("wheel_on_chain_20_31", wheel_on_chain, (20, 31), {2: (309, 61)}, 82, 20, True),
    ("wheel_on_chain_10_16", wheel_on_chain, (10, 16), {3: (301, 61)}, 42, 10, True),
]
PK_IDS = [t[0] for t in PK_TABLE]
PK_CASES = [(t[0], k) for t in PK_TABLE for k in sorted(t[3])]
# (generator, argument tuple, degree, slots of its longest row): one node couples to more than 62
PK_REFUSED = [(wheel, (21,), 2, 64), (half_wheel, (22,), 2, 66), (half_wheel, (11,), 3, 64),
              (wheel, (11,), 3, 67)]


def pk_entry(mesh_id):
    return PK_TABLE[PK_IDS.index(mesh_id)]


def pk_make(mesh_id, groups="zero"):
    _, gen, args, *_ = pk_entry(mesh_id)
    return gen(*args, groups=groups)


def walk_class(max_slots):
    """the FANR of launch_assemble / launch_jac_apply for a layout's max_slots"""
    return 9 if max_slots <= 9 else (12 if max_slots <= 12 else 0)
