"""Every linear solver x preconditioner, two Newton runs and the device md loop on small systems:
iteration counts and solution digests, one JSON line each (PNP_AMD_LIB selects the library)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dune-pnp_amd", "python"))
import pnp_amd as P  # noqa: E402


def h(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def out(**kw):
    print(json.dumps(kw, sort_keys=True), flush=True)


cfg = P.read_config(os.path.join(ROOT, "data", "cylinder_config.cfg"))
mesh = P.Mesh.read_gmsh(cfg.meshfile).refine(2)
par = P.Params.from_config(cfg)
nv = mesh.nv
rng = np.random.default_rng(20261020)
x3 = np.concatenate([rng.uniform(-1, 1, nv), 0.06 * rng.uniform(0.5, 1.5, nv),
                     0.06 * rng.uniform(0.5, 1.5, nv)])
NAMES = {P.PREC_NONE: "none", P.PREC_JACOBI: "jacobi", P.PREC_SSOR: "ssor", P.PREC_ILU0: "ilu0",
         P.PREC_AMG: "amg", P.PREC_SSOR_NATURAL: "ssor_natural"}
ctx = P.Context(mesh, par)
ctx.set_operator(P.OP_PNP)
ctx.jacobian(x3, export=False)
rhs = ctx.residual(x3)
for mname, method in (("bicgstab", P.METHOD_BICGSTAB), ("gmres", P.METHOD_GMRES),
                      ("fgmres", P.METHOD_FGMRES), ("idr", P.METHOD_IDR)):
    for prec in NAMES:
        for graph, flow in ((0, 0), (1, 1)) if mname == "bicgstab" else ((0, 0),):
            ctx.set_option(P.OPT_GRAPH, graph)
            ctx.set_option(P.OPT_ILU_FLOW, flow)
            try:
                sol, res = ctx.linear_solve(rhs, prec=prec, reduction=1e-8, maxit=3000,
                                            method=method)
                out(op="pnp", method=mname, prec=NAMES[prec], graph=graph, flow=flow,
                    it=res["iterations"], it_half=res["it_half"], conv=res["converged"],
                    bd=res["breakdown"], defect=repr(res["defect"]), sol=h(sol),
                    hist=h(np.asarray(ctx.solve_history())) if mname != "bicgstab" else "")
            except P.PnpError as e:
                out(op="pnp", method=mname, prec=NAMES[prec], graph=graph, flow=flow, error=str(e))
ctx.set_option(P.OPT_GRAPH, -1)
ctx.set_option(P.OPT_ILU_FLOW, 0)
ctx.set_operator(P.OP_PB)
xb = np.zeros(nv)
ctx.jacobian(xb, export=False)
rb = ctx.residual(xb)
for prec in NAMES:
    try:
        sol, res = ctx.linear_solve(rb, prec=prec, reduction=1e-10, maxit=5000, method=P.METHOD_CG)
        out(op="pb", method="cg", prec=NAMES[prec], it=res["iterations"], conv=res["converged"],
            defect=repr(res["defect"]), sol=h(sol))
    except P.PnpError as e:
        out(op="pb", method="cg", prec=NAMES[prec], error=str(e))
u, nres = ctx.newton(np.zeros(nv), prec=P.PREC_ILU0)
out(op="pb", newton=nres["iterations"], linear=nres["linear_iterations"], conv=nres["converged"],
    sol=h(u))
ctx.set_operator(P.OP_PNP)
u, nres = ctx.newton(x3, prec=P.PREC_ILU0, maxit=10)
out(op="pnp", newton=nres["iterations"], linear=nres["linear_iterations"], conv=nres["converged"],
    sol=h(u))
ctx.close()

# the operator-split time loop on the device: pore_pnp unrefined, 3 steps from the Boltzmann state
cfg = P.read_config(os.path.join(ROOT, "data", "pore_pnp", "pore.cfg"))
mesh = P.Mesh.read_gmsh(cfg.meshfile)
s = cfg.system
ctx = P.Context(mesh, P.Params.from_config(cfg))
ctx.set_operator(P.OP_PB)
phi, _ = ctx.newton(np.zeros(mesh.nv), reduction=1e-9, prec=P.PREC_SSOR)
u0 = ctx.initial_state(phi)
for pname, prec in (("amg_ssor", P.PREC_AMG), ("ssor", P.PREC_SSOR)):
    if prec == P.PREC_AMG:
        ctx.amg_configure(smoother=P.PREC_SSOR)
    for reuse in (0, 1):
        # dt well under the charge relaxation time 1 / (8 pi l_b c0): every solve converges
        u, t, ip, im, res = ctx.md_run(u0, 0.05, 3, max(1, s["potentialUpdateFreq"]),
                                       max(1, s["outputFreq"]), prec=prec, reuse=reuse)
        res.pop("elapsed")
        out(op="md", prec=pname, reuse=reuse, state=h(u), t=h(t), ip=h(ip), im=h(im), **res)
ctx.close()
