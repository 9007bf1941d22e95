"""The Chebyshev preconditioner (PNP_PREC_CHEBYSHEV) on SURVEY config 3 (pore_pnp k=4), one GPU.
One session, the rows interleaved, medians of `repeats` rounds; JSON lines on stdout and, with the
children's logs, under profiles/cheb/.

Per application (the library's event timers, `napply` applications each, children of this script
because PNP_CHEB_FUSED is read once per process; each round runs the fused child, then the unfused):
    first        k_cheb_first alone (steps 1)
    step         one step i >= 1: (prec(4 steps) - prec(2 steps)) / 2 -- the fused launch, or the
                 operator application and k_cheb_update (the unfused pair)
    spmv         the SpMV of a BiCGSTAB iteration without a preconditioner
    ilu0         one ILU(0) application
Decision rule: the fused step stays the default form only if its median is below
the unfused pair's and the two ranges over the rounds are disjoint.

Per solve: the stationary PNP Newton from the Boltzmann state with BiCGSTAB -- time, linear
iterations, operator applications (2 per iteration, plus steps - 1 per preconditioner application
for Chebyshev) -- with ILU(0), AMG(ILU0), AMG(SSOR), Chebyshev 1..4 steps, AMG(Chebyshev 1..3) and
the Chebyshev rows again with PNP_OPT_MATRIX_FREE.

usage: python tools/bench_cheb.py [repeats=3] [napply=50] [rows=all|apply|solve]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-pnp_amd", "python"))
import pnp_amd as P  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "cheb")
MODEL_US = 60.0  # the issue's derived figure for a fused step (350 MB at the SpMV's achieved rate)


def config3():
    cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
    mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(4)
    ctx = P.Context(mesh, P.Params.from_config(cfg))
    ctx.set_operator(P.OP_PB)
    phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
    x0 = ctx.initial_state(phi)
    ctx.set_operator(P.OP_PNP)
    return ctx, mesh, x0


def emit(rec, fh=None):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


# ---- per application (a child process) -------------------------------------------------------------
def apply_child(napply):
    ctx, mesh, x0 = config3()
    ctx.jacobian(x0, export=False)
    d = np.random.default_rng(3).standard_normal(3 * mesh.nv)

    def prec_us(prec):
        ctx.prec_apply(d, prec)  # set-up and warm-up outside the timed span
        ctx.timers(enable=True, reset=True)
        for _ in range(napply):
            ctx.prec_apply(d, prec)
        return ctx.timers(enable=False)["prec_ms"] / napply * 1e3
    out = {"fused_env": os.environ.get("PNP_CHEB_FUSED", "1"), "dofs": 3 * mesh.nv}
    t = {}
    for steps in (1, 2, 3, 4):
        ctx.cheb_configure(steps=steps)
        t[steps] = prec_us(P.PREC_CHEBYSHEV)
    out["cheb_us_by_steps"] = {str(k): round(v, 2) for k, v in t.items()}
    out["first_us"] = round(t[1], 2)
    out["step_us"] = round((t[4] - t[2]) / 2, 2)
    out["ilu0_us"] = round(prec_us(P.PREC_ILU0), 2)
    ctx.timers(enable=True, reset=True)
    ctx.bicgstab_iterations(napply, P.PREC_NONE)
    tm = ctx.timers(enable=False)
    out["spmv_us"] = round(tm["spmv_ms"] / max(1, tm["spmv_launches"]) * 1e3, 2)
    i = ctx.cheb_info()
    out["fused_steps"], out["unfused_steps"] = i["fused_steps"], i["unfused_steps"]
    out["lambda_est"] = i["lambda_est"]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def apply_rows(repeats, napply, fh):
    recs = {"1": [], "0": []}
    for rep in range(repeats):
        for fused in ("1", "0"):
            env = dict(os.environ, PNP_CHEB_FUSED=fused)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(napply)],
                               env=env, capture_output=True, text=True, timeout=600)
            with open(os.path.join(OUT, f"apply_fused{fused}_round{rep}.log"), "w") as lf:
                lf.write(p.stdout + p.stderr)
            if p.returncode != 0:
                raise SystemExit(f"child failed ({p.returncode}): {p.stderr[-2000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
            rec = json.loads(line[len("RESULT "):])
            rec["round"] = rep
            recs[fused].append(rec)
            emit({"per_application": rec}, fh)
    f = [r["step_us"] for r in recs["1"]]
    u = [r["step_us"] for r in recs["0"]]
    keep = float(np.median(f)) < float(np.median(u)) and max(f) < min(u)
    emit({"decision": {"fused_step_us": f, "unfused_pair_us": u,
                       "fused_median": float(np.median(f)), "unfused_median": float(np.median(u)),
                       "model_fused_us": MODEL_US,
                       "spmv_us_median": float(np.median([r["spmv_us"] for r in recs["1"]])),
                       "ilu0_us_median": float(np.median([r["ilu0_us"] for r in recs["1"]])),
                       "first_us_median": float(np.median([r["first_us"] for r in recs["1"]])),
                       "fused_is_default_form": bool(keep)}}, fh)


# ---- per solve -------------------------------------------------------------------------------------
def solve_rows(repeats, fh):
    ctx, mesh, x0 = config3()
    rows = [("ILU0", P.PREC_ILU0, None, 0, 0), ("AMG(ILU0)", P.PREC_AMG, P.PREC_ILU0, 0, 0),
            ("AMG(SSOR)", P.PREC_AMG, P.PREC_SSOR, 0, 0)]
    rows += [(f"Cheb({k})", P.PREC_CHEBYSHEV, None, k, 0) for k in (1, 2, 3, 4)]
    rows += [(f"AMG(Cheb({k}))", P.PREC_AMG, P.PREC_CHEBYSHEV, k, 0) for k in (1, 2, 3)]
    rows += [(f"Cheb({k}) matrix-free", P.PREC_CHEBYSHEV, None, k, 1) for k in (1, 2, 3, 4)]
    times = {r[0]: [] for r in rows}
    last = {}
    for rep in range(repeats):
        for label, prec, smoother, k, mf in rows:
            ctx.set_option(P.OPT_MATRIX_FREE, mf)
            if smoother is not None:
                ctx.amg_configure(smoother=smoother)
            if k:
                ctx.cheb_configure(steps=k)
            a0 = ctx.cheb_info()
            t0 = time.perf_counter()
            try:
                _, r = ctx.newton(x0, reduction=1e-9, min_linear_reduction=1e-8, prec=prec, maxit=20)
            except P.PnpError as e:  # a linear solve that failed: the row says so
                r = {"converged": 0, "iterations": -1, "linear_iterations": -1, "error": str(e)}
            dt = time.perf_counter() - t0
            a1 = ctx.cheb_info()
            steps = (a1["fused_steps"] - a0["fused_steps"]) + (a1["unfused_steps"] - a0["unfused_steps"])
            times[label].append(dt)
            last[label] = dict(r, cheb_steps=steps)
            emit({"round": rep, "run": label, "newton_seconds": round(dt, 4),
                  "linear_iterations": r.get("linear_iterations")}, fh)
    for label, *_ in rows:
        r = last[label]
        li = r.get("linear_iterations", -1)
        emit({"run": label, "newton_seconds_median": round(float(np.median(times[label])), 4),
              "newton_seconds": [round(t, 4) for t in times[label]],
              "converged": r.get("converged"), "newton_its": r.get("iterations"),
              "linear_iterations": li, "error": r.get("error"),
              "operator_applications": (2 * li + r["cheb_steps"]) if li >= 0 else None}, fh)
    ctx.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        return apply_child(int(sys.argv[2]))
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    napply = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    which = sys.argv[3] if len(sys.argv) > 3 else "all"
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"bench_cheb_{which}.jsonl"), "w") as fh:
        emit({"config": 3, "repeats": repeats, "napply": napply, "rows": which}, fh)
        if which in ("all", "apply"):
            apply_rows(repeats, napply, fh)
        if which in ("all", "solve"):
            solve_rows(repeats, fh)


if __name__ == "__main__":
    main()
