"""The persistent, prefetching PNP assembly walk (k_assemble_ga<..., PIPE = 1>, PNP_ASM_PIPE = 1)
against the direct constant-planes walk (PNP_ASM_PIPE = 0), -m gpu.

PNP_ASM_PIPE and PNP_ASM_PIPE_GRID are read once per process, so every configuration runs in a
child process of its own, one at a time: the reference child with PNP_ASM_PIPE = 0, the children
under test with PNP_ASM_PIPE = 1 and the grid cap unset, 1, 2 and 3.  With the cap at 1 one
workgroup walks every tile (prologue, steady state and epilogue in one chain); 2 and 3 give the
workgroups unequal tile counts, the partial last block among them; unset, the grid is the tile
count on these meshes (a workgroup per tile, each running prologue and epilogue alone).

Every child runs the same calls on the goldens pore_small_k0 and cylinder_k0 with OP_PNP: a
Jacobian at x1 (full write), one at a second state (reuses the constant planes), a residual, a
short linear solve, another Jacobian, and a short Newton run.  Exported Jacobian values,
residuals, solutions and Newton iterates must be bitwise those of the reference child, the Newton
and BiCGSTAB counts the same, and pnp_asm_info must count pipelined launches where the warm
constant-planes walk ran (the Jacobian after the solve takes the cold-hint walk, which is not
pipelined) and none with PNP_ASM_PIPE = 0."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_amd as P
from test_gpu import golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("pore_small_k0", "cylinder_k0")


def second_state(x):
    k = np.arange(x.size, dtype=np.float64)
    return x * (1.0 + 0.05 * np.cos(0.37 * k)) + 1e-3 * np.sin(0.11 * k)


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def sequence():
    """The calls of one child: {golden: {"sha": [...], "ints": [...], "info": [...]}}."""
    out = {}
    for name in NAMES:
        z, mesh, par, orc = golden(name)
        ctx = P.Context(mesh, par)
        ctx.set_operator(P.OP_PNP)
        x1 = z["pnp_x"]
        x2 = second_state(x1)
        shas, info = [], []

        def jac(x):
            J = ctx.jacobian(x)
            shas.extend([sha(J.indptr), sha(J.indices), sha(J.data)])
            i = ctx.asm_info()
            info.append([i["full"], i["reused"], i["pipelined"]])

        jac(x1)                      # full write
        jac(x2)                      # reuses the constant planes: the warm walk
        r2 = ctx.residual(x2)        # residual only
        shas.append(sha(r2))
        sol, res = ctx.linear_solve(r2, prec=P.PREC_ILU0, reduction=1e-6, maxit=2000)
        shas.append(sha(sol))
        jac(x1)                      # follows a solve: the cold-hint walk
        jac(x2)                      # warm again
        ctx.close()

        ctx = P.Context(mesh, par)
        ctx.set_operator(P.OP_PNP)
        u, nres = ctx.newton(z["newton_pnp_x0"], prec=P.PREC_ILU0, linear_maxit=20000)
        shas.append(sha(u))
        i = ctx.asm_info()
        out[name] = {"sha": shas, "info": info,
                     "ints": [res["converged"], res["iterations"], nres["converged"],
                              nres["iterations"], nres["linear_iterations"]],
                     "newton_info": [i["full"], i["reused"], i["pipelined"]]}
        ctx.close()
    return out


CHILD = r"""
import json, sys
sys.path.insert(0, HERE)
import conftest  # noqa: F401  (puts the package on the path)
import test_gpu_asm_pipe as T
print("RESULT " + json.dumps(T.sequence()))
"""


@functools.lru_cache(maxsize=None)
def child(pipe, grid):
    env = dict(os.environ, PNP_ASM_PIPE=str(pipe))
    env.pop("PNP_ASM_PIPE_GRID", None)
    for k in ("PNP_ASM_LDS", "PNP_ASM_GA", "PNP_ASM_FANR", "PNP_ASM_REUSE_CONST"):
        env.pop(k, None)
    if grid is not None:
        env["PNP_ASM_PIPE_GRID"] = str(grid)
    p = subprocess.run([sys.executable, "-c", CHILD.replace("HERE", repr(HERE))], env=env,
                       capture_output=True, text=True, timeout=300, cwd=HERE)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_reference_child_launches_no_pipelined_walk():
    ref = child(0, None)
    assert set(ref) == set(NAMES)
    for name in NAMES:
        assert ref[name]["info"] == [[1, 0, 0], [1, 1, 0], [1, 2, 0], [1, 3, 0]], ref[name]["info"]
        assert ref[name]["newton_info"][2] == 0
        assert ref[name]["ints"][0] == 1 and ref[name]["ints"][2] == 1, ref[name]["ints"]


@pytest.mark.parametrize("grid", [None, 1, 2, 3])
def test_pipelined_walk_is_bitwise_the_direct_walk(grid):
    ref, got = child(0, None), child(1, grid)
    for name in NAMES:
        a, b = got[name], ref[name]
        print(name, grid, a["info"], a["newton_info"], a["ints"])
        assert len(a["sha"]) == len(b["sha"]) == 15
        for k, (u, v) in enumerate(zip(a["sha"], b["sha"])):
            assert u == v, (name, grid, k)
        assert a["ints"] == b["ints"], (name, grid)
        # full write | warm reuse: pipelined | after the solve: the cold-hint walk, LDS-staged
        # where the layout has its lists (else the pipelined walk again) | warm again: pipelined
        assert [i[:2] for i in a["info"]] == [[1, 0], [1, 1], [1, 2], [1, 3]], (name, grid)
        p = [i[2] for i in a["info"]]
        assert p[:2] == [0, 1] and p[2] in (1, 2) and p[3] == p[2] + 1, (name, grid, a["info"])
        # Newton: the first Jacobian writes every plane, the others follow a solve (cold hint)
        assert a["newton_info"][:2] == b["newton_info"][:2]
