"""The operator-split time loop (pnp_main --mode md) on pore_pnp refined 4x (SURVEY config 3 size)
and 2x, P1: ms per time step of
  (a) host    the host-driven loop through the binding -- the calls of the driver's md_loop:
              set_operator, residual, jacobian, linear_solve, ion_flux per solve and step;
  (b) dev0    pnp_md_run with reuse 0;
  (c) dev1    pnp_md_run with reuse 1 (stage 2 keeps stage 1's matrix and set-up),
with dt = cfg.tau, the reference's reductions (1e-5 diffusion, 1e-10 Poisson), BiCGSTAB with the
multicolour SSOR and with AMG(SSOR).  One session per mesh: after a warm-up of every loop, `rounds`
interleaved rounds (a, b, c, a, b, c, ...), each loop from the same Boltzmann state; medians and
ranges, and the counters of pnp_md_result.  With --timers one more run of (a) and (c) with the
library's timers on: where the device time goes.

Each mesh runs in a child process of its own under a time limit; the first failure ends the tool.

usage: python tools/bench_md.py [--steps 4] [--rounds 3] [--refine 4,2] [--timers] [--limit 500]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-pnp_amd", "python"))
import pnp_amd as P  # noqa: E402

RED_D, RED_P, MAXIT = 1e-5, 1e-10, 5000


def host_loop(ctx, u, dt, nsteps, upd, outf, prec):
    """driver/pnp_main.cc md_loop over the binding; returns (u, solves that missed the reduction)"""
    nn = ctx.nn
    phi, cp, cm = (u[k * nn:(k + 1) * nn].copy() for k in range(3))
    a = 1.0 - 0.5 * np.sqrt(2.0)
    missed = [0]

    def linear_problem(x, red):
        r = ctx.residual(x)
        ctx.jacobian(x, export=False)
        z, res = ctx.linear_solve(r, prec=prec, reduction=red, maxit=MAXIT)
        missed[0] += 0 if res["converged"] else 1
        return x - z

    def poisson(phi):
        ctx.set_operator(P.OP_POISSON, cp=cp, cm=cm)
        return linear_problem(phi, RED_P)

    def alexander2(c, z, field):
        u0 = c.copy()
        ctx.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=a * dt, z=z, field=field, phi=phi, x_old=u0)
        u1 = linear_problem(u0.copy(), RED_D)
        ctx.set_operator(P.OP_DIFF, z=z, field=field, phi=phi)
        r1 = ctx.residual(u1) * ((1.0 - a) * dt)
        ctx.set_operator(P.OP_DIFF_IMPLICIT_EULER, dt=a * dt, z=z, field=field, phi=phi, x_old=u0,
                         c_extra=r1)
        return linear_problem(u1.copy(), RED_D)

    for i in range(nsteps):
        cp = alexander2(cp, +1.0, 1)
        cm = alexander2(cm, -1.0, 2)
        if i % upd == 0:
            phi = poisson(phi)
        if i % outf == 0:
            ctx.ion_flux(np.concatenate([phi, cp, cm]))
    phi = poisson(phi)
    return np.concatenate([phi, cp, cm]), missed[0]


def worker(refine, steps, rounds, timers):
    cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
    mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(refine)
    s = cfg.system
    dt, upd, outf = s["tau"], max(1, s["potentialUpdateFreq"]), max(1, s["outputFreq"])
    ctx = P.Context(mesh, P.Params.from_config(cfg))
    ctx.set_operator(P.OP_PB)
    phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
    u0 = ctx.initial_state(phi)
    print(json.dumps({"mesh": "pore_pnp", "refine": refine, "vertices": mesh.nv, "dt": dt,
                      "steps": steps, "rounds": rounds}), flush=True)
    for pname, prec in (("SSOR", P.PREC_SSOR), ("AMG(SSOR)", P.PREC_AMG)):
        if prec == P.PREC_AMG:
            ctx.amg_configure(smoother=P.PREC_SSOR)
        info = {}

        def run(loop, n):
            t0 = time.perf_counter()
            if loop == "host":
                u, missed = host_loop(ctx, u0, dt, n, upd, outf, prec)
                info[loop] = {"missed": missed}
            else:
                u, _, _, _, res = ctx.md_run(u0, dt, n, upd, outf, red_diffusion=RED_D,
                                             red_poisson=RED_P, prec=prec, maxit=MAXIT,
                                             reuse=int(loop == "dev1"))
                info[loop] = res
            return time.perf_counter() - t0, u
        loops = ("host", "dev0", "dev1")
        finals = {lp: run(lp, 1)[1] for lp in loops}  # warm-up: graphs, hierarchies, allocations
        times = {lp: [] for lp in loops}
        for _ in range(rounds):
            for lp in loops:
                t, finals[lp] = run(lp, steps)
                times[lp].append(1e3 * t / steps)
        row = {"prec": pname, "same_bits": bool(np.array_equal(finals["host"], finals["dev0"]) and
                                                np.array_equal(finals["host"], finals["dev1"]))}
        for lp in loops:
            v = sorted(times[lp])
            row[lp] = {"ms_per_step_median": round(v[len(v) // 2], 3),
                       "range": [round(v[0], 3), round(v[-1], 3)], "result": info[lp]}
        print(json.dumps(row), flush=True)
        if timers:
            for lp in ("host", "dev1"):
                ctx.timers(enable=True, reset=True)
                run(lp, steps)
                t = ctx.timers(enable=False)
                print(json.dumps({"prec": pname, "loop": lp, "timers_ms_per_step":
                                  {k: round(v / steps, 3) for k, v in t.items() if k.endswith("_ms")}}),
                      flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--refine", default="4,2")
    ap.add_argument("--timers", action="store_true")
    ap.add_argument("--limit", type=int, default=500, help="seconds per mesh")
    ap.add_argument("--worker", type=int, default=-1)
    a = ap.parse_args()
    if a.worker >= 0:
        worker(a.worker, a.steps, a.rounds, a.timers)
        return 0
    for k in [int(v) for v in a.refine.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(k), "--steps",
               str(a.steps), "--rounds", str(a.rounds)] + (["--timers"] if a.timers else [])
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"refine": k, "error": f"no result within {a.limit} s"}), flush=True)
            return 1
        if rc != 0:  # nothing more on the GPU after a failure
            print(json.dumps({"refine": k, "error": f"worker exit status {rc}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
