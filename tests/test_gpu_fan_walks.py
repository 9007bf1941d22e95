"""The P1 fan walks on pinch vertices, 30-spoke fans and tiny systems, against the oracle (-m gpu).

Every P1 kernel that produces an operator walks a row's vertex fan: the fused and residual-only
assembly (k_assemble; k_assemble_ga direct, LDS-staged and constant-planes), the matrix-free
product and its diagonal-only form (k_jac_apply), the implicit-Euler mass load (k_mass_apply).  The
committed meshes have one fan per vertex and at most 8 neighbours, so their rows carry no break
bits and only OP_PNP / OP_PB ever ran on the longer-fan walks.  The meshes of tests/fan_meshes.py
(generated here, checked on the host by tests/test_fan_layout_host.py) have pinch vertices with up
to five breaks in one row, open fans up to the supported 30 neighbours, a break at the slot where
the gather-all walk issues its second batch of gathers, and systems of 3 .. 514 rows (one
workgroup with 3 live rows, one full SELL chunk, exactly 256 rows, a last workgroup of 3 rows).

Reference: the CPU oracle, which loops over elements and knows nothing of fans.  Bounds: the
project's own (tests/test_gpu.py, tests/test_gpu_matfree.py) --
    residual             max|r - ro|  <= 1e-12 max|ro|
    Jacobian             max|J - Jo|  <= 1e-12 max|Jo|
    matrix-free product  apply_error  <= 1        (1e-12 max_i (|Jo| |z|)_i)
    FD Jacobian          test_gpu_boundary.FD_TOL
The oracle differs from itself by at most 6e-4 of these bounds when its triangles are permuted and
rotated (half_wheel(30), pinwheel([13,1,12]), wheel(30), diamond_chain(86), pinwheel([1,1]); PNP
and PB), so a miss is a wrong walk, not rounding.

Two boundary variants per mesh.  "free": one all-Neumann surface with non-zero fluxes, so no dof
is constrained (asserted: the oracle's mask is all zero) and the hub's rows and blocks are compared
in full -- a masked hub row would compare 0 with 0 and hide the walk.  "mixed": groups index % 2
with a Dirichlet surface; hubs and joints are then constrained (asserted for at least one row with
break bits): zero residual entries, identity rows, product entries bitwise z, while the
neighbours' rows still carry the couplings to the hub.

The exported pattern is compared with the oracle's per vertex pair: the scalar operators' patterns
are equal as they stand; the PNP block pattern stores 7 of the 9 (field, field) entries of a block
(kernels.h kPatPnp), the oracle all 9, so there the vertex pairs are compared and the stored
entries must be a subset (the two left out are zero in Jo by the value bound)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import fan_meshes as F
import meshio
import oracle_py as O
import pnp_amd as P
from test_gpu_asm_const import second_state
from test_gpu_boundary import FD_TOL
from test_gpu_fans import SURF
from test_gpu_matfree import apply_error, random_z, run_ranks

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("free", "mixed")
KINDS = ("pnp", "pnp_ie", "pb", "diff+", "diff-", "diff_ie+", "diff_ie-", "poisson")
DT = 0.37
PHYS = dict(l_b=0.7, c0=0.06, tau=1.0, cylindrical=1)
FANR9 = [i for i in F.IDS if F.walk_class(F.entry(i)[4]) == 9]
LONGER = [i for i in F.IDS if F.walk_class(F.entry(i)[4]) != 9]


@functools.lru_cache(maxsize=None)
def problem(mesh_id, variant):
    """(P.Mesh, P.Params, oracle problem, states, global vertices whose row has break bits) of one
    mesh and boundary variant; shared by the tests and never modified"""
    xy, tri, bseg, bgroup = F.make(mesh_id, "zero" if variant == "free" else "alt")
    surf = SURF[:1] if variant == "free" else SURF
    mesh = P.Mesh(xy, tri, bseg, bgroup)
    par = P.Params([P.Surface(**s) for s in surf], **PHYS)
    orc = O.Problem(meshio.Mesh(xy, tri, bseg, bgroup), [meshio.Surface(**s) for s in surf], **PHYS)
    nv = mesh.nv
    rng = np.random.default_rng(1000 + nv)
    conc = lambda: 0.06 * rng.uniform(0.5, 1.5, nv)
    st = {"phi": rng.uniform(-1, 1, nv), "cp": conc(), "cm": conc(), "diff_phi": rng.uniform(-1, 1, nv),
          "old_phi": rng.uniform(-1, 1, nv), "old_cp": conc(), "old_cm": conc(), "c": conc()}
    L = P.Layout(mesh)
    brk = (L.rowmeta >> np.uint64(8)) & np.uint64((1 << 31) - 1)
    pinch = L.l2g[:L.n_owned][brk != 0]
    mask3 = orc.mask(3)
    if variant == "free":
        assert not mask3.any()  # every row and block is compared in full
    elif F.entry(mesh_id)[5]:
        assert pinch.size == F.entry(mesh_id)[5]
        assert mask3[pinch].any()  # a row with break bits is constrained
    return mesh, par, orc, st, pinch


def set_kind(ctx, orc, st, kind, c_extra=None):
    """set the operator on the context (ctx None: the oracle's only); returns (oracle operator, a
    state of its size)"""
    nv = orc.nv
    mask3 = orc.mask(3)
    a = np.ascontiguousarray
    x3 = np.concatenate([st["phi"], st["cp"], st["cm"]])
    old3 = np.concatenate([st["old_phi"], st["old_cp"], st["old_cm"]])
    if kind == "pnp":
        kp, ko, x = (P.OP_PNP, {}), (O.OP_PNP, dict(mask=mask3)), x3
    elif kind == "pnp_ie":
        kp = (P.OP_PNP_IMPLICIT_EULER, dict(dt=DT, x_old=old3))
        ko, x = (O.OP_PNP_IE, dict(mask=mask3, dt=DT, x_old=old3)), x3
    elif kind == "pb":
        kp, ko, x = (P.OP_PB, {}), (O.OP_PB, dict(mask=orc.mask(1))), st["phi"]
    elif kind == "poisson":
        kp = (P.OP_POISSON, dict(cp=st["cp"], cm=st["cm"]))
        ko, x = (O.OP_POISSON, dict(mask=orc.mask(1), cp=st["cp"], cm=st["cm"])), st["phi"]
    else:  # diff / diff_ie with (z = +1, field 1) or (z = -1, field 2)
        z, field = (1.0, 1) if kind.endswith("+") else (-1.0, 2)
        m = a(mask3[field * nv:(field + 1) * nv])
        x = st["c"]
        if kind.startswith("diff_ie"):
            xo = st["old_cp"] if field == 1 else st["old_cm"]
            kp = (P.OP_DIFF_IMPLICIT_EULER, dict(dt=DT, z=z, field=field, phi=st["diff_phi"],
                                                 x_old=xo))
            ko = (O.OP_DIFF_IE, dict(mask=m, dt=DT, z=z, phi=st["diff_phi"], x_old=xo))
        else:
            kp = (P.OP_DIFF, dict(z=z, field=field, phi=st["diff_phi"]))
            ko = (O.OP_DIFF, dict(mask=m, z=z, phi=st["diff_phi"]))
    if ctx is not None:
        ctx.set_operator(kp[0], c_extra=c_extra, **kp[1])
    return orc.operator(ko[0], flux=orc.flux(), **ko[1]), x


def masked_rows(op):
    return np.nonzero(op._keep[1])[0]


def vertex_pairs(A, nv):
    """the (row vertex, column vertex) pairs of a field-major pattern, as a sorted CSR pattern"""
    C = A.tocoo()
    V = sp.csr_matrix((np.ones(C.nnz), (C.row % nv, C.col % nv)), shape=(nv, nv))
    V.sum_duplicates()
    V.sort_indices()
    return V


def ones(M):
    """the pattern of a CSR matrix, stored zeros included, with every value 1"""
    return sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)


def pattern_errors(J, Jo, nv):
    J, Jo = J.tocsr().copy(), Jo.tocsr().copy()
    J.sort_indices()
    Jo.sort_indices()
    if J.shape[0] == nv:
        ok = np.array_equal(J.indptr, Jo.indptr) and np.array_equal(J.indices, Jo.indices)
        return [] if ok else ["pattern"]
    out = []
    a, b = vertex_pairs(J, nv), vertex_pairs(Jo, nv)
    if not (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)):
        out.append("vertex pattern")
    if (ones(J) - ones(J).multiply(ones(Jo))).count_nonzero():
        out.append("stored entries outside the oracle's pattern")
    return out


def compare(tag, r, J, ro, Jo, op, nv, pattern=None):
    """the residual and Jacobian bounds, the pattern (of J, or the one given), and the constrained
    rows; a list of misses"""
    bad = []
    er = np.max(np.abs(r - ro)) / (1e-12 * np.max(np.abs(ro)))
    ej = abs(J - Jo).max() / (1e-12 * abs(Jo).max())
    print(f"{tag}: residual error / bound {er:.2e}, Jacobian error / bound {ej:.2e}")
    if not er <= 1.0:
        bad.append(f"{tag}: residual {er:.3e} of the bound")
    if not ej <= 1.0:
        bad.append(f"{tag}: Jacobian {ej:.3e} of the bound")
    bad += [f"{tag}: {e}" for e in pattern_errors(J if pattern is None else pattern, Jo, nv)]
    rows = masked_rows(op)
    if rows.size:
        if np.any(r[rows] != 0.0):
            bad.append(f"{tag}: constrained residual entries not 0")
        eye = sp.identity(J.shape[0], format="csr")
        if (J.tocsr()[rows] != eye[rows]).nnz:
            bad.append(f"{tag}: constrained rows not identity rows")
    return bad


def run_all_kinds(mesh_id, variant, digest=None):
    """Case 1 on one mesh: every operator, residual-only and fused; the list of misses"""
    mesh, par, orc, st, _ = problem(mesh_id, variant)
    ctx = P.Context(mesh, par)
    assert ctx.info()["max_slots"] == F.entry(mesh_id)[4]  # the intended walk runs
    bad = []
    for kind in KINDS:
        op, x = set_kind(ctx, orc, st, kind)
        r = ctx.residual(x)   # residual-only kernel (the implicit-Euler load: k_mass_apply)
        J = ctx.jacobian(x)   # fused residual + Jacobian kernel
        bad += compare(f"{mesh_id}/{variant}/{kind}", r, J, orc.residual(op, x),
                       orc.jacobian(op, x), op, mesh.nv)
        if digest is not None:
            digest[f"{mesh_id}/{variant}/{kind}"] = [sha(r), sha(J.data), sha(J.indices)]
    ctx.close()
    return bad


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- 1. all six operators, residual-only and fused ----------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id", F.IDS)
def test_operators_match_oracle(mesh_id, variant):
    bad = run_all_kinds(mesh_id, variant)
    assert not bad, "\n".join(bad)


# ---- 2. c_extra ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", ["pnp", "diff_ie+"])
@pytest.mark.parametrize("mesh_id", ["pinwheel_2_2", "pinwheel_3_1_2", "pinwheel_13_1_12"])
def test_c_extra(mesh_id, kind, variant):
    """one mesh per walk class: the oracle's residual plus c_extra on unmasked rows, 0 on masked
    ones; c_extra is at most half the residual's scale, and the bound stays 1e-12 of that scale"""
    mesh, par, orc, st, _ = problem(mesh_id, variant)
    op, x = set_kind(None, orc, st, kind)
    ro = orc.residual(op, x)
    scale = np.max(np.abs(ro))
    ce = 0.5 * scale * np.random.default_rng(7).uniform(-1, 1, x.size)
    ref = ro + ce
    ref[masked_rows(op)] = 0.0
    ctx = P.Context(mesh, par)
    set_kind(ctx, orc, st, kind, c_extra=ce)
    r = ctx.residual(x)
    ctx.jacobian(x, export=False)
    r2 = ctx.residual(x)
    ctx.close()
    print(f"c_extra {mesh_id} {kind} {variant}: error / bound "
          f"{np.max(np.abs(r - ref)) / (1e-12 * scale):.2e}")
    assert np.max(np.abs(r - ref)) <= 1e-12 * scale
    np.testing.assert_array_equal(r2, r)


# ---- 3. second assembly of one operator (the constant-planes walk) -------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id", F.IDS)
def test_second_assembly(mesh_id, variant):
    """OP_PNP assembled at x1, then at another state: on the meshes of the gather-all walk the
    second assembly keeps the stored k0 / k1 planes (reused >= 1); the longer-fan walks have no
    such variant (reused == 0).  Parity with the oracle at the second state either way."""
    mesh, par, orc, st, _ = problem(mesh_id, variant)
    ctx = P.Context(mesh, par)
    op, x1 = set_kind(ctx, orc, st, "pnp")
    x2 = second_state(x1)
    ctx.jacobian(x1, export=False)
    J = ctx.jacobian(x2)
    r = ctx.residual(x2)
    info = ctx.asm_info()
    ctx.close()
    bad = compare(f"{mesh_id}/{variant}/second", r, J, orc.residual(op, x2), orc.jacobian(op, x2),
                  op, mesh.nv)
    assert not bad, "\n".join(bad)
    if mesh_id in FANR9:
        assert info["reused"] >= 1, info
    else:
        assert info["reused"] == 0 and info["full"] == 2, info


# ---- 4. matrix-free ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mesh_id", F.IDS)
def test_matrix_free(mesh_id, variant):
    mesh, par, orc, st, _ = problem(mesh_id, variant)
    ctx = P.Context(mesh, par)
    ctx.set_option(P.OPT_MATRIX_FREE, 1)
    assert ctx.info()["max_slots"] == F.entry(mesh_id)[4]
    bad = []
    for k, kind in enumerate(KINDS):
        tag = f"{mesh_id}/{variant}/{kind}"
        op, x = set_kind(ctx, orc, st, kind)
        Jo = orc.jacobian(op, x)
        v = random_z(x.size, 20 + k)
        y = ctx.jacobian_apply(v, x)
        err = apply_error(y, Jo, v)
        rows = masked_rows(op)
        if not err <= 1.0:
            bad.append(f"{tag}: product {err:.3e} of the bound")
        if np.any(y[rows] != v[rows]):
            bad.append(f"{tag}: constrained product entries are not z")
        # the diagonal-only walk (Jacobi without SELL values; index loads in the walk whatever the
        # fan length): v = d / diag recovers the diagonal, at the Jacobian's own tolerance
        d = random_z(x.size, 40 + k)
        w = ctx.prec_apply(d, P.PREC_JACOBI)
        ed = np.max(np.abs(d / w - Jo.diagonal())) / (1e-12 * abs(Jo).max())
        print(f"{tag}: product error / bound {err:.2e}, diagonal error / bound {ed:.2e}")
        if not ed <= 1.0:
            bad.append(f"{tag}: diagonal {ed:.3e} of the bound")
    info = ctx.matfree_info()
    ctx.close()
    assert not bad, "\n".join(bad)
    assert info["applies"] >= len(KINDS) and info["value_assemblies"] == 0, info


# ---- 5. forward-difference Jacobian ------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", ["pnp", "pb"])
@pytest.mark.parametrize("mesh_id", ["pinwheel_1_1_1", "pinwheel_13_1_12", "diamond_chain_86"])
def test_fd_jacobian(mesh_id, kind, variant):
    mesh, par, orc, st, _ = problem(mesh_id, variant)
    ctx = P.Context(mesh, par)
    op, x = set_kind(ctx, orc, st, kind)
    J = ctx.jacobian(x, fd=True)
    Jo = orc.jacobian(op, x, fd=True)
    scale = abs(Jo).max()
    print(f"FD {mesh_id} {kind} {variant}: error / scale {abs(J - Jo).max() / scale:.2e}")
    assert abs(J - Jo).max() <= FD_TOL.get(kind, 1e-13) * scale
    Ja = ctx.jacobian(x)  # the analytic Jacobian is the default again afterwards
    ctx.close()
    assert abs(Ja - orc.jacobian(op, x)).max() <= 1e-12 * scale
    assert abs(Ja - J).max() <= 1e-5 * scale


# ---- 6. two in-process ranks ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind", ["pnp", "diff_ie+"])
@pytest.mark.parametrize("mesh_id", ["diamond_chain_86", "pinwheel_13_1_12"])
def test_two_ranks(mesh_id, kind, variant):
    """pinch vertices on the partition cut, with ghost neighbours: the ranks' owned residual
    entries, exported Jacobians and matrix-free products, summed, against the oracle"""
    mesh, par, orc, st, _ = problem(mesh_id, variant)
    op, x = set_kind(None, orc, st, kind)
    v = random_z(x.size, 6)

    def fn(ctx, rank):
        set_kind(ctx, orc, st, kind)
        r = ctx.residual(x)
        J = ctx.jacobian(x)
        ctx.set_option(P.OPT_MATRIX_FREE, 1)
        y = ctx.jacobian_apply(v, x)
        return r, J, y, ctx.info(), ctx.matfree_info()
    outs = run_ranks(2, mesh, par, fn)
    assert sum(o[3]["nv_owned"] for o in outs) == mesh.nv
    assert all(o[3]["nv_ghost"] > 0 for o in outs)
    assert all(o[4]["applies"] >= 1 for o in outs)
    r, J, y = (sum(o[k] for o in outs) for k in range(3))
    Jo = orc.jacobian(op, x)
    # (a sum of sparse matrices drops the entries that sum to zero, the constrained rows' stored
    # zeros among them: the pattern is the sum of the ranks' patterns)
    bad = compare(f"{mesh_id}/{variant}/{kind}/2 ranks", r, J, orc.residual(op, x), Jo, op, mesh.nv,
                  pattern=sum(ones(o[1]) for o in outs))
    assert not bad, "\n".join(bad)
    assert apply_error(y, Jo, v) <= 1.0
    rows = masked_rows(op)
    np.testing.assert_array_equal(y[rows], v[rows])


# ---- 7. knob-selected walks, in child processes -----------------------------------------------------
# The knobs are read once per process.  none: the default dispatch; PNP_ASM_LDS=1: the LDS-staged
# walks (what every Jacobian assembly after a solve takes through the cold hint, and every assembly
# past the Infinity Cache); PNP_ASM_FANR=0: index loads in the walk on short fans (k_assemble<., ., 0>);
# PNP_ASM_GA=0: the pipelined walk with 9 column registers (k_assemble<., 1, ., 9>).
CHILD_MESHES = ("diamond_chain_21", "diamond_chain_85", "diamond_chain_86", "diamond_chain_171",
                "pinwheel_1_1", "pinwheel_1_1_1", "pinwheel_2_2", "one_triangle")
KNOBS = {"none": {}, "lds1": {"PNP_ASM_LDS": "1"}, "lds0": {"PNP_ASM_LDS": "0"},
         "fanr0": {"PNP_ASM_FANR": "0"}, "ga0": {"PNP_ASM_GA": "0"}}
CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_fan_walks as T
print("RESULT " + json.dumps(T.child_main()))
"""


def child_main():
    """case 1 over CHILD_MESHES, checked against the oracle here; the misses and a hash of every
    residual and of every Jacobian's data"""
    bad, digest = [], {}
    for mesh_id in CHILD_MESHES:
        for variant in VARIANTS:
            bad += run_all_kinds(mesh_id, variant, digest)
    return {"bad": bad, "digest": digest}


@functools.lru_cache(maxsize=None)
def child(knob):
    env = {k: v for k, v in os.environ.items()
           if k not in ("PNP_ASM_LDS", "PNP_ASM_FANR", "PNP_ASM_GA")}
    env.update(KNOBS[knob])
    p = subprocess.run([sys.executable, "-c", CHILD.replace("HERE", repr(HERE))], env=env,
                       capture_output=True, text=True, timeout=120, cwd=HERE)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("knob", list(KNOBS))
def test_knob_selected_walks_match_oracle(knob):
    out = child(knob)
    assert len(out["digest"]) == len(CHILD_MESHES) * len(VARIANTS) * len(KINDS)
    assert not out["bad"], "\n".join(out["bad"])


def test_lds_staged_walk_bitwise_equals_direct_walk():
    """tests/test_gpu_asm_lds.py's claim, on rows with breaks and on a last workgroup with 3 live
    rows: only where the neighbour values come from differs"""
    a, b = child("lds1")["digest"], child("lds0")["digest"]
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert a[k] == b[k], k
