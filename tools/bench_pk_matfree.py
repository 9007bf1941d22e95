"""Matrix-free Jacobian application on P_k contexts (pnp_pk_matfree_set, DESIGN.md 4.9 "P_k") next
to the assembled SELL SpMV, on test/pore_pnp/pore.msh refined r times (default 3) at P2 and P3, in
one process, the switch off (the assembled path) and on, alternating between repeats:

  apply   PBOperator at a random state and DiffusionTOperator (OP_DIFF_IE, dt = 0.05) with a random
          frozen potential: CG + Jacobi iterations per second (host clock around a linear_solve of
          exactly `iters` iterations, which ends in a synchronise), and the operator application's
          device time from the library's T_SPMV events in a second run of the same iterations with
          the timers on (element pass + row pass together, or the SpMV), once per repeat
  md      pnp_md_run, 3 steps of dt = 1e-3 from the uniform state (phi = 0), CG + Jacobi: ms per
          step (a small step: CG needs the diffusion step's operator close to symmetric); a run
          whose solve does not converge is reported with its status and the steps it completed

One JSON line per (degree, leg, operator, switch): the median, the range and the repeats
themselves.  A first untimed pass warms up every shape the timed windows use.

usage: python tools/bench_pk_matfree.py [refine=3] [degrees=2,3] [legs=apply,md] [repeats=5] [iters=500]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-pnp_amd", "python"))
import pnp_amd as P  # noqa: E402


def stats(v, nd):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd),
            "max": round(max(v), nd), "repeats": [round(q, nd) for q in v]}


def set_mode(ctx, on, x):
    ctx.pk_matfree(on)
    ctx.jacobian(x, export=False)  # the Jacobian in the selected form


def cg_run(ctx, rhs, iters):
    t0 = time.perf_counter()
    _, res = ctx.linear_solve(rhs, prec=P.PREC_JACOBI, reduction=1e-300, maxit=iters,
                              method=P.METHOD_CG)
    return res["iterations"], time.perf_counter() - t0


def apply_leg(ctx, k, repeats, iters, head):
    nn = ctx.nn
    rng = np.random.default_rng(k)
    ops = (("pb", dict(kind=P.OP_PB), rng.uniform(-1, 1, nn)),
           ("diff_ie", dict(kind=P.OP_DIFF_IMPLICIT_EULER, dt=0.05, z=1.0, field=1,
                            phi=rng.uniform(-1, 1, nn), x_old=rng.uniform(0.0, 0.1, nn)),
            rng.uniform(0.0, 0.1, nn)))
    for name, kw, x in ops:
        ctx.set_operator(**kw)
        rhs = rng.uniform(-1, 1, nn)
        rate, us, its = {0: [], 1: []}, {0: [], 1: []}, {0: 0, 1: 0}
        for rep in range(repeats + 1):  # the first pass is the warm-up
            for on in (0, 1):
                set_mode(ctx, on, x)
                n, dt = cg_run(ctx, rhs, iters)
                ctx.timers(enable=True, reset=True)
                cg_run(ctx, rhs, iters)
                tm = ctx.timers(enable=False)
                if rep:
                    rate[on].append(n / dt)
                    us[on].append(tm["spmv_ms"] / max(1, tm["spmv_launches"]) * 1e3)
                    its[on] = n
        for on in (0, 1):
            print(json.dumps({**head, "leg": "apply", "op": name, "matrix_free": on,
                              "cg_jacobi_iterations_run": its[on],
                              "cg_jacobi_it_per_s": stats(rate[on], 1),
                              "apply_us": stats(us[on], 2),
                              "matfree_info": ctx.matfree_info()}), flush=True)


def md_leg(ctx, k, repeats, head):
    u0 = ctx.initial_state(np.zeros(ctx.nn))
    ms, last = {0: [], 1: []}, {}
    for rep in range(repeats + 1):
        for on in (0, 1):
            ctx.pk_matfree(on)
            t0 = time.perf_counter()
            _, _, _, _, res = ctx.md_run(u0, 1e-3, 3, prec=P.PREC_JACOBI, method=P.METHOD_CG,
                                         maxit=20000)
            dt = time.perf_counter() - t0
            if rep and res["status"] == P.OK:
                ms[on].append(dt / res["steps_done"] * 1e3)
            last[on] = res
    for on in (0, 1):
        r = last[on]
        print(json.dumps({**head, "leg": "md", "matrix_free": on,
                          "ms_per_step": stats(ms[on], 2) if ms[on] else None,
                          "status": r["status"], "steps_done": r["steps_done"],
                          "assemblies": r["assemblies"],
                          "linear_iterations": int(r["linear_iterations"])}), flush=True)


def main():
    arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d  # noqa: E731
    refine = int(arg(1, "3"))
    degrees = [int(v) for v in arg(2, "2,3").split(",")]
    legs = arg(3, "apply,md").split(",")
    repeats, iters = int(arg(4, "5")), int(arg(5, "500"))
    cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
    mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(refine)
    par = P.Params.from_config(cfg)
    for k in degrees:
        ctx = P.Context(mesh, par, degree=k)
        head = {"mesh": f"pore_pnp k={refine}", "degree": k, "nodes": ctx.nn,
                "triangles": mesh.nt}
        print(json.dumps({**head, "repeats": repeats, "iters": iters}), flush=True)
        if "apply" in legs:
            apply_leg(ctx, k, repeats, iters, head)
        if "md" in legs:
            md_leg(ctx, k, repeats, head)
        ctx.close()


if __name__ == "__main__":
    main()
