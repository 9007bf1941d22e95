"""Restarted GMRES / FGMRES next to BiCGSTAB on SURVEY config 3 (pore_pnp k=4) and config 5
(pore_without_dna .geo, scale 0.85, k=6): the stationary PNP Newton from the Boltzmann state with
ILU(0) and with AMG(ILU0).  Per run one JSON line: Newton time to solution, linear iterations, the
event split per linear iteration (spmv / prec / blas) and, for GMRES, the small-kernel time per
Arnoldi step against the orthogonalisation's byte model
    passes x (average j + 2) x 8 B x n
as a fraction of 8 TB/s, for passes = 3 (the design's aim) and passes = 4 (what the kernels issue:
the update fused with the second pass's dots reads its basis slice twice, and where the second read
is served from is not measured).  blas_ms also holds the Hessenberg kernel, the normalisation and the cycle
ends, so the fraction is a lower bound for the orthogonalisation kernels themselves.

usage: python tools/bench_gmres.py [configs=3,5] [restart=30]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-pnp_amd", "python"))
import pnp_amd as P  # noqa: E402

HBM = 8e12


def run(ctx, label, u0, prec, method, restart, n):
    if prec == P.PREC_AMG:
        ctx.amg_configure(smoother=P.PREC_ILU0)
    ctx.timers(enable=False)
    t0 = time.perf_counter()  # time to solution without the timers' events
    u, r = ctx.newton(u0, reduction=1e-9, min_linear_reduction=1e-8, prec=prec, method=method,
                      maxit=20)
    dt = time.perf_counter() - t0
    ctx.timers(enable=True, reset=True)
    u, r = ctx.newton(u0, reduction=1e-9, min_linear_reduction=1e-8, prec=prec, method=method,
                      maxit=20)
    tm = ctx.timers(enable=False)
    its, _ = ctx.newton_history()
    lin = max(1, int(r["linear_iterations"]))
    out = {"run": label, "newton_seconds": round(dt, 4), "converged": r["converged"],
           "newton_its": r["iterations"], "linear_its": int(r["linear_iterations"]),
           "per_step_linear_its": [int(v) for v in its],
           "us_per_it": {k: round(tm[k + "_ms"] / lin * 1e3, 2) for k in ("spmv", "prec", "blas")}}
    if method in (P.METHOD_GMRES, P.METHOD_FGMRES):
        # column index of every Arnoldi step (cycles that ended early on a recomputed norm are
        # rare enough not to matter for the average)
        js = np.concatenate([np.arange(v) % restart for v in its]) if len(its) else np.zeros(1)
        model = 3 * (float(js.mean()) + 2) * 8 * n
        blas_s = tm["blas_ms"] / lin * 1e-3
        out["avg_j"] = round(float(js.mean()), 2)
        out["orth_model_MB_per_step"] = round(model / 1e6, 2)
        out["orth_fraction_of_8TBs"] = round(model / blas_s / HBM, 3)
        out["orth_fraction_of_8TBs_4_reads"] = round(model * 4 / 3 / blas_s / HBM, 3)
    print(json.dumps(out), flush=True)


def config(which):
    if which == 3:
        cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
        return cfg, P.Mesh.read_gmsh(cfg.meshfile).refine(4)
    cfg = P.read_config(os.path.join(ROOT, "data", "pore_without_dna", "pore.cfg"))
    return cfg, P.Mesh.load(cfg.meshfile, size_scale=0.85).refine(6)


def main():
    configs = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "3,5").split(",")]
    restart = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    for which in configs:
        cfg, mesh = config(which)
        ctx = P.Context(mesh, P.Params.from_config(cfg))
        ctx.set_option(P.OPT_GMRES_RESTART, restart)
        n = 3 * mesh.nv
        print(json.dumps({"config": which, "dofs": n, "restart": restart}), flush=True)
        ctx.set_operator(P.OP_PB)
        phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
        x0 = ctx.initial_state(phi)
        ctx.set_operator(P.OP_PNP)
        for pname, prec in (("ILU0", P.PREC_ILU0), ("AMG(ILU0)", P.PREC_AMG)):
            for mname, method in (("BiCGSTAB", P.METHOD_BICGSTAB), (f"GMRES({restart})", P.METHOD_GMRES),
                                  (f"FGMRES({restart})", P.METHOD_FGMRES)):
                run(ctx, f"config {which} {mname}+{pname}", x0, prec, method, restart, n)
        ctx.close()


if __name__ == "__main__":
    main()
