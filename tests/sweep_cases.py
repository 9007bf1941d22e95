"""The layouts on which single applications of the multicolour ILU(0), the multicolour SSOR and
Jacobi are held to the restatements of tests/amg_ref.py: tests/test_sweep_ref_host.py holds every
figure below to P.Layout and the reference to itself (no GPU), tests/test_gpu_sweep_edges.py holds
the kernels to the reference.  Plain data and problem builders; no test in here.

What the committed meshes (colours of 62 .. 88 rows, at most 9 slots, no same-colour coupling) never
reach, and a case here does:
  * a colour of 255, 256, 257, 258, 512 and 513 rows: one full 256-row block, a second block with
    one or two live rows, two full blocks, and with them the block numbering of the staging lists
    (lsx_ptr[blk0 + bl]) across colours of several blocks;
  * a same-colour coupling: wheel_on_chain(5, 340) is an odd wheel whose hub needs a fourth colour
    for one vertex, and mesh.cc absorb_top merges that colour into a lower one because
    ntop * 1024 <= n_owned holds from 1,024 rows on (so no layout below 1,024 rows has one); at P2
    wheel_on_chain(3, 127) has one in a layout of 17-slot rows;
  * P2 / P3 node layouts: 6 .. 10 colours, rows of 61 and 63 slots, the fused factorisation with its
    own rows in scratch (max_slots > 16), and more than ILU_SU * 256 = 1,024 staged neighbours in
    one block (sx_max 1,465 at P3 wheel_on_chain(10, 100); 897 at P3 diamond_chain(64)).
All meshes use the "alt" boundary groups (a Dirichlet and a Neumann surface, "mixed")."""
import collections
import functools

import numpy as np

import fan_meshes as F
import meshio
import oracle_py as O
import pnp_amd as P
from test_gpu_fans import SURF

PHYS = dict(l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)
P1_KINDS = ("pb", "pnp", "pnp_ie")
PK_KINDS = ("pb", "diff_ie")

# expect: one dict per rank, each key a figure of P.Layout / Layout.derived held exactly --
# rows, colours (the colour sizes), conflicts, max_slots, sx_max.  flags name what the case is for
# (checked from the same figures): "c255" .. a colour of exactly that many rows, "conflict",
# "kmax0" / "kmax16" the fused factorisation's form, "long_lists" sx_max > 1,024, "short_lists"
# sx_max <= 1,024 on a P3 layout.
Case = collections.namedtuple("Case", "id family gen args degree kinds nranks expect flags")


def _c(id, family, gen, args, degree=1, nranks=1, expect=(), flags=()):
    kinds = P1_KINDS if degree == 1 else PK_KINDS
    return Case(id, family, gen, tuple(args), degree, kinds, nranks, tuple(expect), tuple(flags))


TABLE = [
    # ---- P1: colours at the edges of the 256-row block ------------------------------------------
    _c("chain170", "p1-block-edge", "diamond_chain", (170,),
       expect=[dict(rows=511, colours=[255, 128, 128], conflicts=0, max_slots=6, sx_max=383)],
       flags=["c255"]),
    _c("chain172", "p1-block-edge", "diamond_chain", (172,),
       expect=[dict(rows=517, colours=[258, 130, 129], conflicts=0, max_slots=6, sx_max=388)],
       flags=["c258"]),
    _c("chain341", "p1-block-edge", "diamond_chain", (341,),
       expect=[dict(rows=1024, colours=[512, 256, 256], conflicts=0, max_slots=6, sx_max=768)],
       flags=["c256", "c512"]),
    _c("chain342", "p1-block-edge", "diamond_chain", (342,),
       expect=[dict(rows=1027, colours=[513, 257, 257], conflicts=0, max_slots=6, sx_max=770)],
       flags=["c257", "c513"]),
    # ---- P1: same-colour couplings --------------------------------------------------------------
    _c("wheel5_chain340", "conflict", "wheel_on_chain", (5, 340),
       expect=[dict(rows=1026, colours=[512, 257, 257], conflicts=1, max_slots=6, sx_max=768)],
       flags=["conflict", "c512", "c257"]),
    _c("wheel7_chain340", "conflict", "wheel_on_chain", (7, 340),
       expect=[dict(rows=1028, colours=[513, 258, 257], conflicts=2, max_slots=8, sx_max=768)],
       flags=["conflict", "c513"]),
    # ---- P1: long rows and tiny systems ---------------------------------------------------------
    _c("pinwheel_13_1_12", "p1-rows", "pinwheel", ((13, 1, 12),),
       expect=[dict(rows=30, colours=[15, 1, 14], conflicts=0, max_slots=30)], flags=["kmax0"]),
    _c("half_wheel_30", "p1-rows", "half_wheel", (30,),
       expect=[dict(rows=31, colours=[13, 12, 1, 5], conflicts=0, max_slots=31)], flags=["kmax0"]),
    _c("pinwheel_4_3_2", "p1-rows", "pinwheel", ((4, 3, 2),),
       expect=[dict(rows=13, colours=[7, 5, 1], conflicts=0, max_slots=13)], flags=["kmax16"]),
    _c("one_triangle", "p1-rows", "one_triangle", (),
       expect=[dict(rows=3, colours=[1, 1, 1], conflicts=0, max_slots=3)]),
    # ---- P2 -------------------------------------------------------------------------------------
    _c("chain128-P2", "p2", "diamond_chain", (128,), 2,
       expect=[dict(rows=1025, colours=[256, 192, 128, 129, 192, 128], conflicts=0, max_slots=14)],
       flags=["c256"]),
    _c("chain140-P2", "p2", "diamond_chain", (140,), 2,
       expect=[dict(rows=1121, colours=[257, 217, 180, 171, 168, 128], conflicts=0,
                    max_slots=14)], flags=["c257"]),
    _c("one_triangle-P2", "p2", "one_triangle", (), 2,
       expect=[dict(rows=6, colours=[1] * 6, conflicts=0, max_slots=6)]),
    _c("split_triangle-P2", "p2", "split_triangle", (), 2,
       expect=[dict(rows=10, conflicts=0, max_slots=10)]),
    _c("half_wheel_21-P2", "p2", "half_wheel", (21,), 2,
       expect=[dict(rows=63, conflicts=0, max_slots=63)], flags=["kmax0"]),
    _c("wheel_20-P2", "p2", "wheel", (20,), 2,
       expect=[dict(rows=61, conflicts=0, max_slots=61)], flags=["kmax0"]),
    # a same-colour coupling in colour 0 of a layout whose rows pass 16 slots: the fused
    # factorisation keeps its own rows in scratch (KMAX = 0), where the dropped blocks are stored
    # and dropped() alone keeps them out of the updates (with own rows in LDS they never reach the
    # scratch); 7 rows of later colours couple to both ends of the pair
    _c("wheel3_chain127-P2", "conflict", "wheel_on_chain", (3, 127), 2,
       expect=[dict(rows=1026, colours=[244, 206, 192, 192, 96, 96], conflicts=1, max_slots=17)],
       flags=["conflict", "kmax0"]),
    # ---- P3 -------------------------------------------------------------------------------------
    _c("chain139-P3", "p3", "diamond_chain", (139,), 3,
       expect=[dict(rows=2086, colours=[257, 278, 232, 246, 211, 177, 200, 186, 171, 128],
                    conflicts=0, max_slots=25, sx_max=1958)], flags=["c257", "long_lists"]),
    _c("chain64-P3", "p3", "diamond_chain", (64,), 3,
       expect=[dict(rows=961, conflicts=0, max_slots=25, sx_max=897)], flags=["short_lists"]),
    _c("wheel10_chain100-P3", "p3", "wheel_on_chain", (10, 100), 3,
       expect=[dict(rows=1561, conflicts=0, max_slots=61, sx_max=1465)],
       flags=["kmax0", "long_lists"]),
    _c("one_triangle-P3", "p3", "one_triangle", (), 3,
       expect=[dict(rows=10, colours=[1] * 10, conflicts=0, max_slots=10)]),
    _c("split_triangle-P3", "p3", "split_triangle", (), 3,
       expect=[dict(rows=19, colours=[2, 2, 2, 2, 2, 1, 2, 2, 2, 2], conflicts=0, max_slots=19)]),
    _c("wheel_10-P3", "p3", "wheel", (10,), 3,
       expect=[dict(rows=61, conflicts=0, max_slots=61)], flags=["kmax0"]),
    # ---- 2 ranks (in-process local group) -------------------------------------------------------
    _c("wheel5_chain340-2ranks", "ranks", "wheel_on_chain", (5, 340), 1, 2,
       expect=[dict(rows=513, colours=[257, 128, 128], conflicts=0),
               dict(rows=513, colours=[254, 128, 130, 1], conflicts=0)], flags=["c257"]),
    _c("chain32-P2-2ranks", "ranks", "diamond_chain", (32,), 2, 2,
       expect=[dict(rows=128, conflicts=0, max_slots=14),
               dict(rows=129, conflicts=0, max_slots=14)]),
]
BY_ID = {c.id: c for c in TABLE}
IDS = [c.id for c in TABLE]
assert len(BY_ID) == len(TABLE)

# the cases the sweep variants (one child process each) run: the block-edge and conflict P1 layouts,
# a 63-slot P2 row, a 61-slot P3 row, and the P3 layout whose staging lists pass 1,024 entries
VARIANT_IDS = ["chain170", "chain172", "chain341", "chain342", "wheel5_chain340",
               "wheel7_chain340", "wheel3_chain127-P2", "half_wheel_21-P2", "wheel_10-P3",
               "wheel10_chain100-P3"]
# one fused BiCGSTAB + ILU(0) solve each: (case, kinds, rows of colour 0 = launch_update_fwd0's
# c0_end).  The P_k case has no block system; it takes the two scalar kinds of its table row.
SOLVE_CASES = [("chain170", ("pb", "pnp_ie"), 255), ("chain342", ("pb", "pnp_ie"), 513),
               ("wheel5_chain340", ("pb", "pnp_ie"), 512), ("chain140-P2", ("pb", "diff_ie"), 257)]


def nfields(kind):
    return 3 if kind.startswith("pnp") else 1


def mesh_arrays(c):
    return getattr(F, c.gen)(*c.args, groups="alt")


def layout_figures(lay):
    """the figures a case's `expect` names, read from a rank's layout"""
    d = lay.derived
    return dict(rows=int(lay.n_owned), colours=[int(q) for q in np.diff(lay.color_ptr)],
                conflicts=int(lay.color_conflicts), max_slots=int(lay.max_slots),
                sweep_usable=int(d.sweep_usable), sx_max=int(d.sx_max),
                lsx_entries=int(d.lsx_entries))


def flag_holds(flag, fig, degree):
    if flag.startswith("c") and flag[1:].isdigit():
        return int(flag[1:]) in fig["colours"]
    return {"conflict": fig["conflicts"] >= 1,
            "kmax0": fig["max_slots"] > 16,
            "kmax16": 10 < fig["max_slots"] <= 16,
            "long_lists": fig["sx_max"] > 1024,
            "short_lists": degree == 3 and fig["sx_max"] <= 1024}[flag]


@functools.lru_cache(maxsize=None)
def p1_problem(case_id):
    """(P.Mesh, P.Params, oracle problem, states) of a P1 case, the states as
    test_gpu_fan_walks.problem draws them; shared and never modified"""
    c = BY_ID[case_id]
    assert c.degree == 1
    xy, tri, bseg, bgroup = mesh_arrays(c)
    mesh = P.Mesh(xy, tri, bseg, bgroup)
    par = P.Params([P.Surface(**s) for s in SURF], **PHYS)
    orc = O.Problem(meshio.Mesh(xy, tri, bseg, bgroup), [meshio.Surface(**s) for s in SURF], **PHYS)
    nv = mesh.nv
    rng = np.random.default_rng(1000 + nv)
    conc = lambda: 0.06 * rng.uniform(0.5, 1.5, nv)  # noqa: E731
    st = {"phi": rng.uniform(-1, 1, nv), "cp": conc(), "cm": conc(),
          "diff_phi": rng.uniform(-1, 1, nv), "old_phi": rng.uniform(-1, 1, nv), "old_cp": conc(),
          "old_cm": conc(), "c": conc()}
    return mesh, par, orc, st


@functools.lru_cache(maxsize=None)
def pk_problem(case_id):
    """(P.Mesh, P.Params, oracle problem, oracle P_k space) of a P_k case; shared, never modified"""
    c = BY_ID[case_id]
    assert c.degree > 1
    xy, tri, bseg, bgroup = mesh_arrays(c)
    par = P.Params([P.Surface(**s) for s in SURF], **PHYS)
    orc = O.Problem(meshio.Mesh(xy, tri, bseg, bgroup), [meshio.Surface(**s) for s in SURF], **PHYS)
    return P.Mesh(xy, tri, bseg, bgroup), par, orc, O.PkSpace(orc, c.degree)


def mesh_of(case_id):
    return (p1_problem if BY_ID[case_id].degree == 1 else pk_problem)(case_id)[0]


def rhs(n, seed=23):
    return np.random.default_rng(seed).standard_normal(n)
