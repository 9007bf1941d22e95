"""The regular walk of the warm OP_PNP assembly (k_assemble_ga<..., REG = 1>, PNP_ASM_REGULAR = 1)
against the general walk for every wave (PNP_ASM_REGULAR = 0), -m gpu.

PNP_ASM_REGULAR is read once per process, so each setting runs in a child process of its own, one
at a time (the pattern of tests/test_gpu_asm_pipe.py).  Both children run the same calls with
OP_PNP on every mesh:

  a Jacobian at x1 (full write: the general walk in both children), one at a second state (keeps the
  constant planes: the warm walk, regular where the chunk is), a residual, a short ILU(0) solve,
  the Jacobian after the solve (cold hint: the LDS-staged walk where the layout has its lists),
  a warm one again, set_operator again and a Jacobian (full write) and a warm one after it, and a
  short Newton run.

Exported values, residuals -- also the one each Jacobian launch writes along with its blocks,
pnp_state_residual -- solutions and Newton iterates must be bitwise equal, the Newton and BiCGSTAB
counts equal.  Meshes:

  (a) the structured grid of tests/asm_regular_cases.py, whose layout has -- asserted through
      pnp_asm_regular_info -- a fully regular chunk, a mixed chunk and a partial last chunk, so both
      paths of the kernel run in one launch;
  (b) the goldens pore_small_k0 and cylinder_k0, mostly general chunks;
  (c) pore_pnp refined twice on 1 and on 2 in-process ranks, where regular fans have ghost columns.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import asm_regular_cases as R
import pnp_amd as P
from conftest import DATA
from test_gpu import golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("grid", "pore_small_k0", "cylinder_k0", "pore_pnp_r2_1", "pore_pnp_r2_2")


def second_state(x):
    k = np.arange(x.size, dtype=np.float64)
    return x * (1.0 + 0.05 * np.cos(0.37 * k)) + 1e-3 * np.sin(0.11 * k)


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def problem(case):
    """(mesh, params, x1, Newton start, ranks) of one case"""
    if case == "grid":
        mesh = P.Mesh(*R.grid_mesh(R.GRID_N))
        par = P.Params([P.Surface(**s) for s in R.SURF], **R.PHYS)
        return mesh, par, R.grid_state(mesh.nv, 41), R.grid_state(mesh.nv, 42), 1
    if case.startswith("pore_pnp_r2"):
        cfg = P.read_config(os.path.join(DATA, "pore_pnp", "pore.cfg"))
        mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(2)
        par = P.Params.from_config(cfg)
        return (mesh, par, R.grid_state(mesh.nv, 43), R.grid_state(mesh.nv, 44),
                int(case.rsplit("_", 1)[1]))
    z, mesh, par, orc = golden(case)
    return mesh, par, z["pnp_x"], z["newton_pnp_x0"], 1


def rank_sequence(ctx, x1, x0):
    """the calls of one rank (collective on more than one)"""
    ctx.set_operator(P.OP_PNP)
    x2 = second_state(x1)
    shas, info = [], []

    def jac(x):
        J = ctx.jacobian(x)
        # the blocks, and the residual the same launch wrote (Newton's right-hand side)
        shas.extend([sha(J.indptr), sha(J.indices), sha(J.data), sha(ctx.state_residual())])
        i = ctx.asm_info()
        info.append([i["full"], i["reused"]])

    jac(x1)                      # full write
    jac(x2)                      # keeps the constant planes: the warm walk
    r2 = ctx.sync_vector(ctx.residual(x2))
    shas.append(sha(r2))
    sol, res = ctx.linear_solve(r2, prec=P.PREC_ILU0, reduction=1e-6, maxit=300)
    shas.append(sha(sol))
    jac(x1)                      # follows a solve: the cold-hint walk
    jac(x2)                      # warm again
    ctx.set_operator(P.OP_PNP)
    jac(x1)                      # full write again
    jac(x2)                      # warm
    u, nres = ctx.newton(x0, prec=P.PREC_ILU0, maxit=3, linear_maxit=2000)
    shas.append(sha(u))
    return {"sha": shas, "info": info, "regular": ctx.asm_regular_info(),
            "ints": [res["converged"], res["iterations"], nres["status"], nres["converged"],
                     nres["iterations"], nres["linear_iterations"]]}


def sequence():
    """The calls of one child: {case: [per-rank results]}."""
    out = {}
    for case in CASES:
        mesh, par, x1, x0, nranks = problem(case)

        def work(r):
            ctx = P.Context(mesh, par, device=0, rank=r, size=nranks,
                            local_group=f"reg_{case}" if nranks > 1 else None)
            try:
                return rank_sequence(ctx, x1, x0)
            finally:
                ctx.close()
        with ThreadPoolExecutor(nranks) as ex:
            out[case] = list(ex.map(work, range(nranks)))
    return out


CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_asm_regular as T
print("RESULT " + json.dumps(T.sequence()))
"""


@functools.lru_cache(maxsize=None)
def child(regular):
    env = dict(os.environ, PNP_ASM_REGULAR=str(regular))
    for k in ("PNP_ASM_PIPE", "PNP_ASM_PIPE_GRID", "PNP_ASM_LDS", "PNP_ASM_GA", "PNP_ASM_FANR",
              "PNP_ASM_REUSE_CONST", "PNP_ASM_COLD_HINT", "PNP_ASM_WAVES"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", CHILD.replace("HERE", repr(HERE))], env=env,
                       capture_output=True, text=True, timeout=600, cwd=HERE)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_the_grid_runs_both_paths_in_one_launch():
    """through pnp_asm_regular_info and the host layout: the grid has a fully regular chunk, a mixed
    chunk and a partial last chunk, so its warm launches run the regular and the general walk"""
    mesh = problem("grid")[0]
    L = P.Layout(mesh)
    got = child(1)["grid"][0]["regular"]
    assert got == L.regular_info == R.regular_info(L), (got, L.regular_info)
    rows, cnt = R.chunk_classes(L)
    assert 0 < got["regular_chunks"] < got["chunks"]
    assert np.any((cnt > 0) & (cnt < rows)) and rows[-1] < 64
    assert R.grid_has_all_three(L)


def test_counts_match_the_host_layout_on_every_rank():
    got = child(1)
    for case in CASES:
        mesh, _, _, _, nranks = problem(case)
        for r in range(nranks):
            want = R.regular_info(P.Layout(mesh, r, nranks))
            assert got[case][r]["regular"] == want, (case, r)
        print(case, [g["regular"] for g in got[case]])
    # refined twice, the pore mesh is mostly regular chunks on either partition
    for case in ("pore_pnp_r2_1", "pore_pnp_r2_2"):
        for g in got[case]:
            assert g["regular"]["regular_chunks"] > g["regular"]["chunks"] // 2, (case, g["regular"])


@pytest.mark.parametrize("case", CASES)
def test_regular_walk_is_bitwise_the_general_walk(case):
    ref, got = child(0)[case], child(1)[case]
    assert len(ref) == len(got) == problem(case)[4]
    for r, (a, b) in enumerate(zip(got, ref)):
        print(case, r, a["info"], a["ints"], a["regular"])
        assert len(a["sha"]) == len(b["sha"]) == 27
        for k, (u, v) in enumerate(zip(a["sha"], b["sha"])):
            assert u == v, (case, r, k)
        assert a["ints"] == b["ints"], (case, r)
        # the walks the calls took: full | reuse | reuse (cold hint) | reuse | full | reuse
        assert a["info"] == b["info"] == [[1, 0], [1, 1], [1, 2], [1, 3], [2, 3], [2, 4]], (case, r)
