"""bench.py as a program (-m gpu): a plain run on the unrefined pore_pnp mesh prints the head of
the result line only, --steps sets the number of timed steps, and --dump-outputs writes what the
last timed assembly computed -- checked against the same system assembled in this process through
the host-vector calls (pnp_jacobian + export, pnp_residual) at the suite's 1e-12 parity bound."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pnp_amd as P
from conftest import DATA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(DATA)
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    return B


def test_plain_run_head_of_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--refine", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "assembled DOFs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0
    dofs = line["config"]["dofs"]
    assert line["value"] == pytest.approx(dofs / (1e-3 * line["ms_per_step"]), rel=1e-12)
    # no secondary leg ran
    for key in ("cpu_baseline", "roofline", "bicgstab_iters_per_s", "per_config", "strong_scaling",
                "measured_stream_gbs", "pnp_newton_time_to_solution"):
        assert key not in line
    assert sorted(os.listdir(out)) == ["jacobian_rowsum.npy", "jacobian_values.npy",
                                       "residual_norm.npy"]
    got = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in got.values())

    # the same system in this process: bench.py's own setup, then the host-vector calls
    B = _bench()
    cfg = P.read_config(os.path.join(DATA, "pore_pnp", "pore.cfg"))
    mesh = P.Mesh.read_gmsh(cfg.meshfile)
    ctx, x0, _, _ = B.make_context(mesh, cfg, 0, 1, 0, None)
    J = ctx.jacobian(x0)
    r = ctx.residual(x0)
    ctx.close()
    assert dofs == 3 * mesh.nv and J.nnz <= B.DUMP_CAP  # nothing sampled at this size
    scale = abs(J).max()
    assert got["jacobian_values"].shape == J.data.shape
    assert np.max(np.abs(got["jacobian_values"] - J.data)) <= 1e-12 * scale
    rowsum = J @ np.ones(J.shape[1])
    # a row sum adds up to max-row-length entries, each within the entry bound
    assert np.max(np.abs(got["jacobian_rowsum"] - rowsum)) <= 1e-12 * scale * np.diff(J.indptr).max()
    assert got["residual_norm"].shape == (1,)
    assert abs(got["residual_norm"][0] - np.linalg.norm(r)) <= 1e-12 * np.linalg.norm(r)
