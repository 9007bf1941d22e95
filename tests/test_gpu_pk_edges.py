"""The P_k (degree 2, 3) assembly on 61 .. 63-slot rows, pinch vertices and tiny meshes, against the
CPU oracle (-m gpu).

The committed meshes give a P_k node at most 8 elements and a row at most 49 slots (P3) / 25 (P2),
and thousands of elements.  The meshes of fan_meshes.PK_TABLE (held to the oracle on the host by
tests/test_pk_edge_meshes_host.py) reach what they never do: rows of 61 slots at P3 and 61 / 63 at
P2 (the layout's limit: the LDS accumulator of k_pk_row / k_pk_jac_gather at 122 .. 126 KB, byte
slot codes up to 62, the (row << 6 | slot) codes of the export and the CSR view, the SpMV); a node
in exactly 1, 3, 4, 5, 8, 9, 10 and 20 elements (the batches of four of k_pk_res_gather, the
prefetch of k_pk_row and k_pk_jac_gather); 1, 128 and 130 elements (one element, one full workgroup
of k_pk_elem_jac, a last one of 2); systems of 6, 65, 256 and 257 rows; pinch vertices; and the
Jacobian gather as two launches (wheel_on_chain with a 100-quadrilateral chain) and as one (the
same wheel on a short chain), told apart by pnp_info.pk_split_short / _long / _len.

Reference: the oracle's P_k space, nodes matched by coordinates.  Bounds: the project's own
(tests/test_gpu_pk.py, tests/test_gpu_matfree.py), unchanged --
    residual               max|r - ro|   <= 1e-12 max|ro|
    Jacobian               max|J - Jo|   <= 1e-12 max|Jo|,  equal nnz
    PNP_JAC_FD Jacobian    max|Jf - Jfo| <= 1e-7 max|Jfo|
    stored-matrix product  apply_error   <= 1   (1e-12 max_i (|Jo| |z|)_i); constrained rows z
The residual that a Jacobian assembly leaves for Newton is not readable through the C ABI; its
2-norm is: pnp_bicgstab_iterations reports it as defect0 before its first iteration (that one
unpreconditioned iteration is run only for this number; its other effect is that the next assembly
counts as the first after a solve).  The context keeps one residual buffer, so before every
Jacobian assembly a residual at another state is assembled: the buffer then holds the wrong
answer, and a gather that left some rows' residual unwritten shows in the norm.  Every entry within
1e-12 max|ro| puts the norm within sqrt(n) 1e-12 max|ro| of the oracle's, which is asserted.  What
this sees: rows not written, and wrong entries once their effect on the norm, |dr_i| |r_i| / ||r||,
passes that bound (an entry wrong by more than about n 1e-12 max|ro| in a row of typical size).
What it cannot see: per-entry agreement at 1e-12 max|ro|.  test_knobs_agree_bitwise requires the
norm to be the same to the last bit from the gather (one launch and two) and from the row walk,
which writes its residual in another kernel.
With the triangles of every table mesh permuted and their vertices rotated the oracle differs from
itself by at most 2.8e-3 of the residual bound (wheel_on_chain_10_16 P3 poisson), 2.9e-3 of the
Jacobian bound (half_wheel_9 P3 diff) and 7.9e-2 of the FD bound (diamond_chain_64 P3 poisson),
over both variants, the four operators and both states.  The largest GPU errors seen on the MI355X
were 3.3e-3 (residual, pinwheel_3_1_2 P3), 3.3e-3 (Jacobian, half_wheel_9 P3), 5.7e-2 (FD,
diamond_chain_65 P3), 2.3e-3 (product, half_wheel_9 P3) and 6.0e-4 (norm of the Jacobian
assembly's residual) of their bounds.  A miss is a wrong kernel or table, not rounding.

Two boundary variants, as tests/test_gpu_fan_walks.py: "free" is one all-Neumann surface (the
oracle's mask is all zero, every row compared in full), "mixed" groups index % 2 with a Dirichlet
surface (interior hubs stay unconstrained, the host test asserts it).

Partitions: a rank that would own no node is refused at creation on every rank alike (PNP_E_MESH,
"owns no vertices"), before any collective -- asserted here for more ranks than nodes; every rank
of the partitions below owns at least one node.  "P_k: element not local" cannot occur: a rank's
ghosts are all row neighbours of its owned nodes, and the nodes of an element are row neighbours
of each other."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import fan_meshes as F
import oracle_py as O
import pk_util as U
import pnp_amd as P
from test_gpu_asm_const import second_state
from test_gpu_fans import SURF
from test_gpu_matfree import apply_error, random_z
from test_gpu_pk import KINDS, args, bind
from test_pk_edge_meshes_host import PHYS, VARIANTS, oracle_problem

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KIND_ORDER = ("pb", "poisson", "diff", "diff_ie")
SPLIT_RUNS = [("wheel_on_chain_20_100", 2), ("wheel_on_chain_10_100", 3)]
SPLIT_IDLE = [("wheel_on_chain_20_31", 2), ("wheel_on_chain_10_16", 3)]


@functools.lru_cache(maxsize=None)
def problem(mesh_id, k, variant):
    """(P.Mesh, P.Params, oracle problem, oracle space) of one table mesh; shared, never modified"""
    xy, tri, bseg, bgroup = m = F.pk_make(mesh_id, "zero" if variant == "free" else "alt")
    surf = SURF[:1] if variant == "free" else SURF
    par = P.Params([P.Surface(**s) for s in surf], **PHYS)
    orc = oracle_problem(m, variant)
    S = O.PkSpace(orc, k)
    if variant == "free":
        assert not any(S.mask(f).any() for f in range(3))
    return P.Mesh(xy, tri, bseg, bgroup), par, orc, S


def check_space(ctx, S, mesh_id, k):
    """the product's space is the oracle's node for node; perm: product node i = oracle perm[i]"""
    xy, en = ctx.space()
    assert xy.shape[0] == S.nn == ctx.nn == F.pk_entry(mesh_id)[3][k][0]
    perm = U.match_nodes(xy, S.xy)
    np.testing.assert_array_equal(perm[en], S.enode)
    return perm


@functools.lru_cache(maxsize=None)
def oracle_values(mesh_id, k, variant, kind, second):
    """(x, kw, ro, Jo, Jfo or None) over the oracle's nodes: computed once, shared"""
    _, _, orc, S = problem(mesh_id, k, variant)
    x, kw = args(kind, S.nn, 100 * k + KIND_ORDER.index(kind))
    if second:
        x = second_state(x)
    op = _oracle_op(orc, S, kind, kw)
    return x, kw, S.residual(op, x), S.jacobian(op, x), \
        None if second else S.jacobian(op, x, fd=True)


def _oracle_op(orc, S, kind, kw):
    field = 2 if kind.startswith("diff") else 0
    return orc.operator(KINDS[kind][1], flux=orc.flux(), mask=S.mask(field), **kw)


def spoil(x):
    """a state whose residual differs from x's in every row (the residual buffer's content before
    a Jacobian assembly at x)"""
    return 0.5 * x[::-1] + 0.01


def figures(tag, ctx, S, perm, orc, mesh_id, k, variant, kind, second, worst):
    """one operator at one state on ctx against the oracle: the list of misses"""
    x, kw, ro, Jo, Jfo = oracle_values(mesh_id, k, variant, kind, second)
    if not second:
        op = bind(ctx, orc, S, perm, kind, kw)  # switches the operator
    else:
        op = _oracle_op(orc, S, kind, kw)
    xp = x[perm]
    Jo = Jo[perm][:, perm]
    rs, js = np.abs(ro).max(), abs(Jo).max()
    r = ctx.residual(xp)                 # two-pass residual (k_pk_elem_res, k_pk_res_gather)
    ctx.residual(spoil(xp))              # the residual buffer now holds another state's answer
    J = ctx.jacobian(xp)                 # k_pk_elem_jac, k_pk_jac_gather (one or two launches)
    d0 = ctx.bicgstab_iterations(1)["defect0"]   # ||r|| of the Jacobian assembly's residual
    z = random_z(S.nn, 5 + int(second))
    y = ctx.jacobian_apply(z)            # the stored matrix: SpMV
    fig = {"res": np.abs(r - ro[perm]).max() / (1e-12 * rs),
           "jac": abs(J - Jo).max() / (1e-12 * js),
           "jres": abs(d0 - np.linalg.norm(ro)) / (np.sqrt(S.nn) * 1e-12 * rs),
           "apply": apply_error(y, Jo, z)}
    bad = []
    if J.nnz != Jo.nnz:
        bad.append(f"{tag}: nnz {J.nnz} != {Jo.nnz}")
    rows = np.nonzero(op._keep[1][perm])[0]
    if not np.array_equal(y[rows], z[rows]):
        bad.append(f"{tag}: product on constrained rows is not z")
    if Jfo is not None:
        Jfo = Jfo[perm][:, perm]
        Jf = ctx.jacobian(xp, fd=True)   # k_pk_row<K, 2>
        fig["fd"] = abs(Jf - Jfo).max() / (1e-7 * abs(Jfo).max())
    for name, v in fig.items():
        worst[name] = max(worst.get(name, 0.0), float(v))
        if not v <= 1.0:
            bad.append(f"{tag}: {name} error / bound {v:.3e}")
    return bad


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id,k", F.PK_CASES)
def test_edge_mesh_matches_oracle(mesh_id, k, variant):
    """space, max_slots, the four operators (residual, Jacobian with its residual, FD Jacobian,
    stored-matrix product), then each again at a second state on the same context before the
    operator is switched: nothing stale in the accumulator's unused slots or the padding"""
    mesh, par, orc, S = problem(mesh_id, k, variant)
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, mesh_id, k)
        assert ctx.info()["max_slots"] == F.pk_entry(mesh_id)[3][k][1]
        bad, worst = [], {}
        for kind in KIND_ORDER + ("pb",):
            for second in (False, True):
                tag = f"{mesh_id}/P{k}/{variant}/{kind}/{int(second)}"
                bad += figures(tag, ctx, S, perm, orc, mesh_id, k, variant, kind, second, worst)
        print(f"EDGE-FIG {mesh_id} P{k} {variant} " + json.dumps(worst))
        assert not bad, bad
    finally:
        ctx.close()


def d2h(ptr, n, dtype):
    """n entries at a device address, through the HIP runtime the library itself links"""
    out = np.empty(n, dtype=dtype)
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes),
                         2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("mesh_id,k", [("half_wheel_21", 2), ("wheel_10", 3),
                                       ("wheel_on_chain_10_100", 3)])
def test_csr_view_of_long_rows(mesh_id, k):
    """pnp_jacobian_csr_device on 61 / 63-slot rows: the device CSR is the exported matrix, bit
    for bit"""
    mesh, par, orc, S = problem(mesh_id, k, "free")
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, mesh_id, k)
        x, kw, _, Jo, _ = oracle_values(mesh_id, k, "free", "diff_ie", False)
        bind(ctx, orc, S, perm, "diff_ie", kw)
        J = ctx.jacobian(x[perm]).tocsr()
        v = ctx.jacobian_csr_device()
        assert v["n"] == S.nn and v["nnz"] == J.nnz == Jo.nnz
        assert np.array_equal(d2h(v["rowptr"], v["n"] + 1, np.int32), J.indptr)
        assert np.array_equal(d2h(v["col"], v["nnz"], np.int32), J.indices)
        assert np.array_equal(d2h(v["val"], v["nnz"], np.float64), J.data)
    finally:
        ctx.close()


@pytest.mark.parametrize("mesh_id,k", SPLIT_RUNS + SPLIT_IDLE + [("wheel_10", 3), ("wheel_20", 2)])
def test_split_state_is_the_intended_one(mesh_id, k):
    """the Jacobian gather runs as two launches on the long chains and as one launch elsewhere;
    the short launch's accumulator is shorter than the longest row.  (The values of both states are
    compared with the oracle in test_edge_mesh_matches_oracle and with each other bit for bit in
    test_knobs_agree_bitwise.)"""
    mesh, par, _, _ = problem(mesh_id, k, "free")
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        i = ctx.info()
        print(f"EDGE-SPLIT {mesh_id} P{k}: short {i['pk_split_short']} long {i['pk_split_long']} "
              f"len {i['pk_split_len']} max_slots {i['max_slots']}")
        if (mesh_id, k) in SPLIT_RUNS:
            assert i["pk_split_long"] >= 1 and i["pk_split_short"] >= 1
            assert 0 < i["pk_split_len"] < i["max_slots"]
            assert i["pk_split_long"] + i["pk_split_short"] == (ctx.nn + 255) // 256
        else:
            assert (i["pk_split_short"], i["pk_split_long"], i["pk_split_len"]) == (0, 0, 0)
    finally:
        ctx.close()
    # a P1 context has no gather
    c1 = P.Context(mesh, par, device=0)
    try:
        i = c1.info()
        assert (i["pk_split_short"], i["pk_split_long"], i["pk_split_len"]) == (0, 0, 0)
    finally:
        c1.close()


@pytest.mark.parametrize("mesh_id,k", [("wheel_10", 2), ("wheel_10", 3), ("wheel_20", 2)]
                         + SPLIT_RUNS + SPLIT_IDLE)
def test_initial_state_and_ion_flux_match_oracle(mesh_id, k):
    mesh, par, orc, S = problem(mesh_id, k, "mixed")
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, mesh_id, k)
        phi = np.random.default_rng(k).uniform(-2, 2, S.nn)
        x0o = S.initial_state(phi)
        x0 = ctx.initial_state(phi[perm])
        nn = S.nn
        np.testing.assert_array_equal(
            x0, np.concatenate([x0o[f * nn:(f + 1) * nn][perm] for f in range(3)]))
        ipo, imo = S.ion_flux(x0o)
        ip, im = ctx.ion_flux(x0)
        scale = max(np.abs(ipo).max(), np.abs(imo).max())
        assert scale > 0
        assert np.abs(ip - ipo).max() <= 1e-12 * scale and np.abs(im - imo).max() <= 1e-12 * scale
    finally:
        ctx.close()


_group = iter(range(1 << 30))


def run_ranks(n, mesh, par, k, fn):
    """fn(ctx) on n in-process ranks (one local group, a thread each); fn makes library calls only,
    every assertion comes after the join.  Returns (results, errors)."""
    name = f"pkedge{next(_group)}"
    out, err = [None] * n, []

    def work(rank):
        try:
            c = P.Context(mesh, par, device=0, rank=rank, size=n, local_group=name, degree=k)
            try:
                out[rank] = fn(c)
            finally:
                c.close()
        except Exception as e:  # noqa: BLE001
            err.append((rank, e))

    th = [threading.Thread(target=work, args=(q,), daemon=True) for q in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank did not return"
    return out, err


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("mesh_id,k", [("one_triangle", 2), ("one_triangle", 3),
                                       ("pinwheel_3_1_2", 2), ("pinwheel_3_1_2", 3)] + SPLIT_RUNS)
def test_partitioned_matches_oracle(mesh_id, k, n):
    """2 and 3 in-process ranks: the synced residual and the sum of the ranks' exported Jacobians
    (each exports its owned rows) against the oracle, all four operators on one context per rank.
    one_triangle at P2 leaves a rank 2 of 6 nodes; the pinwheel's hub row has ghosts on every
    other rank."""
    mesh, par, orc, S = problem(mesh_id, k, "mixed")
    c1 = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(c1, S, mesh_id, k)
    finally:
        c1.close()
    vals = {kind: oracle_values(mesh_id, k, "mixed", kind, False) for kind in KIND_ORDER}

    def fn(c):
        res = {"owned": c.info()["nv_owned"]}
        for kind in KIND_ORDER:
            x, kw = vals[kind][:2]
            pk = {q: (v[perm] if isinstance(v, np.ndarray) else v) for q, v in kw.items()}
            if kind.startswith("diff"):
                pk["field"] = 2
            c.set_operator(KINDS[kind][0], **pk)
            r = c.sync_vector(c.residual(x[perm]), 1)
            res[kind] = (r, c.jacobian(x[perm]))
        return res

    out, err = run_ranks(n, mesh, par, k, fn)
    assert not err, err
    owned = [o["owned"] for o in out]
    print(f"EDGE-RANKS {mesh_id} P{k} {n} ranks own {owned}")
    assert sum(owned) == S.nn and min(owned) >= 1
    for kind in KIND_ORDER:
        _, _, ro, Jo, _ = vals[kind]
        Jo = Jo[perm][:, perm]
        for o in out:  # the synced residual is the whole vector on every rank
            assert np.abs(o[kind][0] - ro[perm]).max() <= 1e-12 * np.abs(ro).max()
        Jsum = sum(o[kind][1] for o in out)
        assert abs(Jsum - Jo).max() <= 1e-12 * abs(Jo).max()
        assert sum(o[kind][1].nnz for o in out) == Jo.nnz


def test_more_ranks_than_nodes_is_refused_on_every_rank():
    """one_triangle at P2 has 6 nodes: on 7 ranks one part is empty, and every rank's creation
    fails with PNP_E_MESH before it joins the group (no rank is left waiting)"""
    mesh, par, _, _ = problem("one_triangle", 2, "free")
    out, err = run_ranks(7, mesh, par, 2, lambda c: 0)
    assert len(err) == 7
    assert all(isinstance(e, P.PnpError) and e.code == P.E_MESH and "owns no" in str(e)
               for _, e in err)


@pytest.mark.parametrize("gen,gargs,k,slots", F.PK_REFUSED)
def test_rows_over_62_neighbours_are_refused(gen, gargs, k, slots):
    """a node with more than 62 neighbours is refused with the node and the count named, never cut
    to slots & 63; a context created right afterwards works"""
    xy, tri, bseg, bgroup = gen(*gargs)
    par = P.Params([P.Surface(**SURF[0])], **PHYS)
    with pytest.raises(P.PnpError) as ei:
        P.Context(P.Mesh(xy, tri, bseg, bgroup), par, device=0, degree=k)
    assert ei.value.code == P.E_MESH
    # the hub is vertex 0, so node 0, the first node over the limit
    assert f"P{k} node 0 couples to {slots - 1} nodes" in str(ei.value)
    mesh, par, orc, S = problem("one_triangle", k, "free")
    ctx = P.Context(mesh, par, device=0, degree=k)
    try:
        perm = check_space(ctx, S, "one_triangle", k)
        x, kw, ro, _, _ = oracle_values("one_triangle", k, "free", "pb", False)
        bind(ctx, orc, S, perm, "pb", kw)
        assert np.abs(ctx.residual(x[perm]) - ro[perm]).max() <= 1e-12 * np.abs(ro).max()
    finally:
        ctx.close()


# ---- the knobs, one child process each (PNP_PK_RES2 / PNP_PK_JAC2 are read once per process) ----
CHILD = r"""
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import pnp_amd as P
import fan_meshes as F
from test_gpu_fans import SURF
from test_gpu_pk import KINDS
PHYS = dict(l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)
def h(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
def sweep(ctx, out, tag):
    nn = ctx.nn
    rng = np.random.default_rng(nn)
    for kind in ("pb", "poisson", "diff", "diff_ie"):
        kw = {}
        if kind.startswith("diff"):
            kw = dict(z=-1.0, phi=rng.uniform(-1, 1, nn), field=2)
            if kind == "diff_ie":
                kw.update(dt=0.37, x_old=rng.uniform(0.0, 0.1, nn))
        if kind == "poisson":
            kw = dict(cp=rng.uniform(0.0, 0.1, nn), cm=rng.uniform(0.0, 0.1, nn))
        ctx.set_operator(KINDS[kind][0], **kw)
        x = rng.uniform(-1, 1, nn) if kind in ("pb", "poisson") else rng.uniform(0, 0.1, nn)
        r = ctx.residual(x)
        ctx.residual(0.5 * x[::-1] + 0.01)  # the residual buffer holds another state's answer
        J = ctx.jacobian(x).tocsr()
        d0 = ctx.bicgstab_iterations(1)["defect0"]  # norm of the Jacobian assembly's residual
        out[f"{tag}/{kind}"] = [h(r), h(J.data), h(J.indices), d0.hex()]
out, split = {}, {}
if MODE == "table":
    for mesh_id, k in F.PK_CASES:
        for variant in ("free", "mixed"):
            xy, tri, bseg, bgroup = F.pk_make(mesh_id, "zero" if variant == "free" else "alt")
            par = P.Params([P.Surface(**s) for s in (SURF[:1] if variant == "free" else SURF)],
                           **PHYS)
            ctx = P.Context(P.Mesh(xy, tri, bseg, bgroup), par, device=0, degree=k)
            i = ctx.info()
            split[f"{mesh_id}/{k}"] = [i["pk_split_short"], i["pk_split_long"], i["pk_split_len"]]
            sweep(ctx, out, f"{mesh_id}/{k}/{variant}")
            ctx.close()
else:  # the committed meshes at P3: PNP_PK_SPLIT is read at every context creation
    from test_gpu_pk import setup
    for name in ("pore_small", "cylinder"):
        for knob in (None, "1", "0"):
            os.environ.pop("PNP_PK_SPLIT", None)
            if knob is not None:
                os.environ["PNP_PK_SPLIT"] = knob
            mesh, ctx, orc = setup(name, 3)
            i = ctx.info()
            split[f"{name}/{knob}"] = [i["pk_split_short"], i["pk_split_long"],
                                       i["pk_split_len"], i["max_slots"], i["nv_owned"]]
            out[f"{name}/{knob}"] = {}
            sweep(ctx, out[f"{name}/{knob}"], name)
            ctx.close()
print("RESULT " + json.dumps({"out": out, "split": split}))
"""


def run_child(mode, **env):
    e = {q: v for q, v in os.environ.items() if not q.startswith("PNP_PK_")}
    e.update(env)
    code = CHILD.replace("HERE", repr(HERE)).replace("MODE", repr(mode))
    p = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True,
                       timeout=300, cwd=HERE)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [q for q in p.stdout.splitlines() if q.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_knobs_agree_bitwise():
    """every table mesh, both variants, four operators: the default, PNP_PK_SPLIT=0 (one gather
    launch) and PNP_PK_RES2=0 PNP_PK_JAC2=0 (the row walk k_pk_row) give the same residuals, matrix
    values, column indices and Jacobian-assembly residual norms bit for bit, as the kernels'
    comments claim"""
    a = run_child("table")
    b = run_child("table", PNP_PK_SPLIT="0")
    c = run_child("table", PNP_PK_RES2="0", PNP_PK_JAC2="0")
    assert len(a["out"]) == 2 * 4 * len(F.PK_CASES)
    for mesh_id, k in SPLIT_RUNS:  # the default child did split, so the comparison means something
        assert a["split"][f"{mesh_id}/{k}"][0] >= 1 and a["split"][f"{mesh_id}/{k}"][1] >= 1
    assert all(v == [0, 0, 0] for v in b["split"].values())
    diff_b = sorted(q for q in a["out"] if a["out"][q] != b["out"][q])
    diff_c = sorted(q for q in a["out"] if a["out"][q] != c["out"][q])
    assert not diff_b and not diff_c, (diff_b, diff_c)


def test_forced_split_on_committed_meshes_at_p3():
    """Does the split ever run on the committed meshes?  At P3 it does not, on pore.msh (2,593
    rows) or on cylinder.msh (2,554 rows; longest row 49 slots on both), neither by default nor
    with PNP_PK_SPLIT=1: the layout orders the rows by colour, every 256-row block holds vertex
    rows, and no block's longest row is at most half of 49.  On the MI355X all three fields were 0
    in all six runs; that is asserted, so that a layout which starts to split there shows up here.
    The rule itself is held too: forced, the split runs exactly when the median block is at most
    half the longest, and then with an accumulator shorter than the longest row.  Whatever ran,
    the values are bit for bit those of PNP_PK_SPLIT=0."""
    r = run_child("committed")
    print(f"EDGE-COMMITTED split fields (short, long, len, max_slots, rows): {r['split']}")
    for name in ("pore_small", "cylinder"):
        sp = {q: r["split"][f"{name}/{q}"] for q in ("None", "1", "0")}
        assert sp["0"][:3] == [0, 0, 0]
        assert r["out"][f"{name}/1"] == r["out"][f"{name}/0"] == r["out"][f"{name}/None"]
        ns, nl, ln, mx, rows = sp["1"]
        assert (ns, nl, ln) == (0, 0, 0) or \
            (ns >= 1 and nl >= 1 and 2 * ln <= mx and ns + nl == (rows + 255) // 256)
        # the default decides on the longest row alone (more than 64 KB of accumulator)
        assert sp["None"] == (sp["1"] if mx > 32 else sp["0"])
    assert r["split"]["pore_small/1"][:3] == r["split"]["cylinder/1"][:3] == [0, 0, 0]
