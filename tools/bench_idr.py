"""IDR(s) next to BiCGSTAB on SURVEY config 3 (pore_pnp k=4): the stationary PNP Newton from the
Boltzmann state with ILU(0) and with AMG(ILU0), s = 1, 2, 4, 8.  One session, the methods
interleaved, medians of `repeats` runs.  Per row one JSON line: Newton time to solution, operator
applications per Newton step (BiCGSTAB: two per iteration), the event split per application
(spmv / prec / blas, from one extra run with the library's timers on) and, for IDR, the blas time
against the byte model of DESIGN.md 4.10,
    (3 s^2 + 14 s + 6) / (s + 1) vector passes of 8 n bytes per application (cycle average),
as a fraction of 8 TB/s.  blas also holds the one-thread state kernels and the column sums, so the
fraction is a lower bound for the streaming kernels themselves.

Then the breakdown count of BiCGSTAB and IDR(4) without a preconditioner on the first Newton
system of pore_small_k0 (tests/golden), 16 right-hand sides: the system's own and 15 perturbed by
1e-14 relative.

usage: python tools/bench_idr.py [repeats=3] [svalues=1,2,4,8]
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


def passes(s):
    """Vector passes per operator application, cycle average."""
    return (3 * s * s + 14 * s + 6) / (s + 1)


def newton(ctx, u0, prec, method):
    t0 = time.perf_counter()
    try:
        u, r = ctx.newton(u0, reduction=1e-9, min_linear_reduction=1e-8, prec=prec, method=method,
                          maxit=20)
    except P.PnpError as e:  # a linear solve that failed: the row says so
        r = {"converged": 0, "iterations": -1, "error": str(e)}
    return time.perf_counter() - t0, r


def applications(ctx, method):
    its, _ = ctx.newton_history()
    return [int(v) * (2 if method == P.METHOD_BICGSTAB else 1) for v in its]


def config3():
    cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
    return cfg, P.Mesh.read_gmsh(cfg.meshfile).refine(4)


def newton_rows(repeats, svalues):
    cfg, mesh = config3()
    ctx = P.Context(mesh, P.Params.from_config(cfg))
    n = 3 * mesh.nv
    print(json.dumps({"config": 3, "dofs": n, "repeats": repeats}), flush=True)
    ctx.set_operator(P.OP_PB)
    phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
    x0 = ctx.initial_state(phi)
    ctx.set_operator(P.OP_PNP)
    rows = []
    for pname, prec in (("ILU0", P.PREC_ILU0), ("AMG(ILU0)", P.PREC_AMG)):
        rows.append((f"BiCGSTAB+{pname}", prec, P.METHOD_BICGSTAB, 0))
        rows += [(f"IDR({s})+{pname}", prec, P.METHOD_IDR, s) for s in svalues]
    times = {row[0]: [] for row in rows}
    apps, results, split = {}, {}, {}
    ctx.timers(enable=False)
    for rep in range(repeats):
        for label, prec, method, s in rows:
            if prec == P.PREC_AMG:
                ctx.amg_configure(smoother=P.PREC_ILU0)
            if s:
                ctx.set_option(P.OPT_IDR_S, s)
            dt, r = newton(ctx, x0, prec, method)
            times[label].append(dt)
            print(json.dumps({"repeat": rep, "run": label, "newton_seconds": round(dt, 4)}),
                  flush=True)
            apps[label] = applications(ctx, method)
            results[label] = r
            if rep == 0:  # the event split, from a run of its own with the timers on
                ctx.timers(enable=True, reset=True)
                newton(ctx, x0, prec, method)
                tm = ctx.timers(enable=False)
                na = max(1, sum(applications(ctx, method)))
                split[label] = {k: tm[k + "_ms"] / na * 1e3 for k in ("spmv", "prec", "blas")}
    for label, prec, method, s in rows:
        r = results[label]
        out = {"run": label, "newton_seconds_median": round(float(np.median(times[label])), 4),
               "newton_seconds": [round(t, 4) for t in times[label]],
               "converged": r["converged"], "newton_its": r["iterations"],
               "error": r.get("error"),
               "applications": int(sum(apps[label])), "applications_per_step": apps[label],
               "us_per_application": {k: round(v, 2) for k, v in split[label].items()}}
        if s:
            model = passes(s) * 8 * n
            out["model_passes_per_application"] = round(passes(s), 2)
            out["model_MB_per_application"] = round(model / 1e6, 2)
            out["blas_fraction_of_8TBs"] = round(model / (split[label]["blas"] * 1e-6) / HBM, 3)
            out["replacements"] = ctx.idr_info()["replacements"]
        print(json.dumps(out), flush=True)
    ctx.close()


def breakdown_rows():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conftest  # noqa: F401
    from test_gpu import golden

    z, mesh, par, _ = golden("pore_small_k0")
    ctx = P.Context(mesh, par)
    ctx.set_operator(P.OP_PNP)
    x = np.ascontiguousarray(z["newton_pnp_x0"])
    ctx.jacobian(x, export=False)
    rhs = ctx.residual(x)
    rng = np.random.default_rng(11)
    rhss = [rhs] + [rhs * (1 + 1e-14 * rng.standard_normal(rhs.size)) for _ in range(15)]
    ctx.set_option(P.OPT_IDR_S, 4)
    for label, method in (("BiCGSTAB", P.METHOD_BICGSTAB), ("IDR(4)", P.METHOD_IDR)):
        res = [ctx.linear_solve(b, prec=P.PREC_NONE, reduction=1e-8, maxit=20000, method=method)[1]
               for b in rhss]
        its = [r["it_half"] * (2 if method == P.METHOD_BICGSTAB else 1) for r in res if r["converged"]]
        print(json.dumps({"run": f"pore_small_k0 first Newton system, no preconditioner, {label}",
                          "right_hand_sides": len(res),
                          "converged": sum(r["converged"] for r in res),
                          "breakdowns": sum(1 for r in res if r["breakdown"]),
                          "breakdown_codes": sorted({r["breakdown"] for r in res if r["breakdown"]}),
                          "applications_min_max": [min(its), max(its)] if its else None,
                          "replacements": ctx.idr_info()["replacements"]}), flush=True)
    ctx.close()


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    svalues = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1,2,4,8").split(",")]
    breakdown_rows()
    newton_rows(repeats, svalues)


if __name__ == "__main__":
    main()
