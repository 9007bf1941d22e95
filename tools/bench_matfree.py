"""Matrix-free Jacobian application (OPT_MATRIX_FREE) next to the assembled SELL
SpMV on SURVEY config 3 (pore_pnp k=4) and config 5 (pore_without_dna .geo, scale 0.85, k=6), in
one process, the option off (the assembled path) and on, alternating between repeats:

  apply   per preconditioner (NONE, JACOBI, ILU0): BiCGSTAB iterations per second from
          bicgstab_iterations (host clock around a call that ends in a synchronise), and the
          operator application's device time from the library's T_SPMV events in a second run of
          the same iterations with the timers on, once per repeat
  newton  the stationary PNP Newton from the Boltzmann state, time to solution, with ILU0 and with
          AMG(ILU0)

One JSON line per (config, leg, preconditioner, option): the median of the repeats and the repeats
themselves.  The byte model of an application (what it must read and write once, HBM 8 TB/s) is
printed with each apply line; it is a model, not a measurement.

usage: python tools/bench_matfree.py [configs=3] [legs=apply,newton] [repeats=5] [iters=2000]
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

HBM = 8e12
PRECS = (("NONE", P.PREC_NONE), ("JACOBI", P.PREC_JACOBI), ("ILU0", P.PREC_ILU0))


def config(which):
    if which == 3:
        cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
        return cfg, P.Mesh.read_gmsh(cfg.meshfile).refine(4)
    cfg = P.read_config(os.path.join(ROOT, "data", "pore_without_dna", "pore.cfg"))
    return cfg, P.Mesh.load(cfg.meshfile, size_scale=0.85).refine(6)


def byte_model(info):
    """bytes one application moves at least, PNP (nf = 3): the SpMV streams the k-form values and
    column indices and gathers z; the matrix-free walk gathers x, z and the coordinates and reads
    the column indices, the row metadata and the mask.  Gathers counted once per vertex."""
    n, slots, nks = info["nv_owned"], info["nslots"], info["nks"]
    vec = 3 * 8 * n
    spmv = slots * (nks * 8 + 4) + 2 * vec
    free = slots * 4 + n * (8 + 3 + 16) + 3 * vec
    return spmv, free


def set_mode(ctx, on):
    ctx.set_option(P.OPT_MATRIX_FREE, on)
    ctx.assemble_state(1)  # the Jacobian in the selected form (and the residual the solves take)


def apply_leg(ctx, which, repeats, iters):
    info = ctx.info()
    spmv_b, free_b = byte_model(info)
    for pname, prec in PRECS:
        rate, us, launches = {0: [], 1: []}, {0: [], 1: []}, {0: 0, 1: 0}
        for on in (0, 1):  # warm up every shape the timed windows use
            set_mode(ctx, on)
            ctx.bicgstab_iterations(20, prec)
        for _ in range(repeats):
            for on in (0, 1):
                set_mode(ctx, on)
                t0 = time.perf_counter()
                r = ctx.bicgstab_iterations(iters, prec)
                rate[on].append(r["iterations"] / (time.perf_counter() - t0))
                # the application's own device time: the same run again with the timers on
                ctx.timers(enable=True, reset=True)
                ctx.bicgstab_iterations(iters, prec)
                tm = ctx.timers(enable=False)
                us[on].append(tm["spmv_ms"] / max(1, tm["spmv_launches"]) * 1e3)
                launches[on] = int(tm["spmv_launches"])
        for on in (0, 1):
            model = free_b if on else spmv_b
            med = statistics.median(us[on])
            print(json.dumps({
                "config": which, "leg": "apply", "prec": pname, "matrix_free": on,
                "bicgstab_it_per_s_median": round(statistics.median(rate[on]), 1),
                "bicgstab_it_per_s": [round(v, 1) for v in rate[on]],
                "apply_us_median": round(med, 2), "apply_us": [round(v, 2) for v in us[on]],
                "applies_per_timed_run": launches[on], "model_MB": round(model / 1e6, 1),
                "model_fraction_of_8TBs": round(model / (med * 1e-6) / HBM, 3),
                "matfree_info": ctx.matfree_info()}), flush=True)


def newton_leg(ctx, which, x0, repeats):
    for pname, prec in (("ILU0", P.PREC_ILU0), ("AMG(ILU0)", P.PREC_AMG)):
        if prec == P.PREC_AMG:
            ctx.amg_configure(smoother=P.PREC_ILU0)
        secs, last = {0: [], 1: []}, {}
        for rep in range(repeats + 1):  # the first pass warms up both forms
            for on in (0, 1):
                ctx.set_option(P.OPT_MATRIX_FREE, on)
                before = ctx.matfree_info()
                t0 = time.perf_counter()
                u, r = ctx.newton(x0, reduction=1e-9, min_linear_reduction=1e-8, prec=prec, maxit=20)
                dt = time.perf_counter() - t0
                after = ctx.matfree_info()
                if rep:
                    secs[on].append(dt)
                last[on] = (r, {k: after[k] - before[k] for k in after})
        for on in (0, 1):
            r, cnt = last[on]
            print(json.dumps({
                "config": which, "leg": "newton", "prec": pname, "matrix_free": on,
                "newton_seconds_median": round(statistics.median(secs[on]), 4),
                "newton_seconds": [round(v, 4) for v in secs[on]],
                "converged": r["converged"], "newton_its": r["iterations"],
                "linear_its": int(r["linear_iterations"]),
                "assemble_seconds": round(r["assemble_seconds"], 4),
                "solve_seconds": round(r["solve_seconds"], 4), "per_solve": cnt}), flush=True)


def main():
    arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d  # noqa: E731
    configs = [int(v) for v in arg(1, "3").split(",")]
    legs = arg(2, "apply,newton").split(",")
    repeats, iters = int(arg(3, "5")), int(arg(4, "2000"))
    for which in configs:
        cfg, mesh = config(which)
        ctx = P.Context(mesh, P.Params.from_config(cfg))
        print(json.dumps({"config": which, "dofs": 3 * mesh.nv, "repeats": repeats,
                          "iters": iters}), flush=True)
        ctx.set_operator(P.OP_PB)
        phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
        x0 = ctx.initial_state(phi)
        ctx.set_operator(P.OP_PNP)
        ctx.state_set(x0)
        if "apply" in legs:
            apply_leg(ctx, which, repeats, iters)
        if "newton" in legs:
            newton_leg(ctx, which, x0, max(1, repeats // 2 + 1))
        ctx.close()


if __name__ == "__main__":
    main()
