// pnp_md_run: the operator-split time loop of src/instationary_pnp_from_pb_md.hh:411-454 with
// its state resident on the device.  The loop is the driver's md_loop
// (driver/pnp_main.cc) statement for statement; what changes is where the data lives:
//   - phi, c+, c- are scalar vectors in the internal layout with their ghosts, uploaded once and
//     downloaded once, their ghosts refreshed through halo() after every update;
//   - the static part of each operator (Dirichlet mask, Neumann load, row flags) is computed on
//     the host once per (kind, field) and copied device to device into the context's operator
//     buffers when the operator becomes current; the frozen fields, x_old and
//     cvec = (load + c_extra) - M(x_old) are built on the device;
//   - every right-hand side is the residual-only launch's output, the arithmetic and its order
//     are the host-driven loop's, so the results are that loop's bit for bit.
#include "ctx.h"

#define CKH(expr, what)                             \
  do {                                              \
    hipError_t e_ = (expr);                         \
    if (e_ != hipSuccess) return hipfail(e_, what); \
  } while (0)

struct pnp_ctx::MdRun {
  DBuf<double> phi, cp, cm;        // the state, n_local each
  DBuf<double> u0;                 // the ion's old time level inside its Alexander2 step
  DBuf<double> s_phi, s_cp, s_cm;  // the state after the last completed step
  MdOp ie[2], sp[2], pois;         // DiffusionTOperator / DiffusionOperator per ion, Poisson
  pnp_md_opts o{};
  pnp_md_result *res = nullptr;
  int status = PNP_OK;  // of the run: a failed solve ends it
};

int pnp_ctx::md_op_build(MdOp &op, int k, int field, double z) {
  op.kind = k;
  op.field = field;
  op.z = z;
  std::vector<double> lload;
  op_static(k, field, 0.0, op.gmask, op.hmask, lload);
  // (every row of an implicit-Euler operator reads its load: the mass kernel rewrites cvec)
  op.hflag = row_flags(1, k == PNP_OP_DIFF_IMPLICIT_EULER, op.hmask, lload, nullptr);
  int rc;
  if ((rc = upv(op.mask, op.hmask, "md mask")) || (rc = upv(op.flag, op.hflag, "md row flags")) ||
      (rc = upv(op.load, lload, "md load")))
    return rc;
  return PNP_OK;
}

// `op` becomes the context's operator through op_activate, as in pnp_set_operator; the mask and
// flags from the operator's device copies, the frozen fields a0 / a1 (n_local, with ghosts) from
// the resident state.  cvec is md_cvec's.
int pnp_ctx::md_activate(const MdOp &op, double dt, const double *a0, const double *a1) {
  if (int rc = op_activate(op.kind, dt, op.z)) return rc;
  if (L.n_owned)
    CKH(hipMemcpyAsync(dmask.p, op.mask.p, size_t(L.n_owned), hipMemcpyDeviceToDevice, stream),
        "md mask");
  CKH(hipMemcpyAsync(rowflag.p, op.flag.p, rowflag.n, hipMemcpyDeviceToDevice, stream),
      "md row flags");
  hrowflag.assign(op.hflag.begin(), op.hflag.begin() + L.n_owned);
  hmask = op.hmask;
  // reference-order mode is refused by pnp_md_run; its copies are those of no operator
  seq_cextra = false;
  seq_mask_h.assign(size_t(mesh.nv), 0);
  seq_phi_h.clear();
  seq_cp_h.clear();
  seq_cm_h.clear();
  seq_xold_h.clear();
  const size_t nlb = sizeof(double) * size_t(L.n_owned + L.n_ghost);
  if (a0) CKH(hipMemcpyAsync(aux0.p, a0, nlb, hipMemcpyDeviceToDevice, stream), "md aux");
  if (a1) CKH(hipMemcpyAsync(aux1.p, a1, nlb, hipMemcpyDeviceToDevice, stream), "md aux");
  return PNP_OK;
}

// the current operator's cvec = (load + s r1) - M(xold) (r1 null: no extra term; xold null: no
// old mass), from the operator's load on the device
int pnp_ctx::md_cvec(const MdOp &op, double s, const double *r1, const double *xold) {
  CKH(pnp::launch_md_load(L.n_owned, op.load.p, s, r1, cvec.p, stream), "md load");
  if (!xold) return PNP_OK;
  CKH(hipMemcpyAsync(prevu.p, xold, sizeof(double) * size_t(L.n_owned + L.n_ghost),
                     hipMemcpyDeviceToDevice, stream),
      "md x_old");
  if (degree > 1)
    CKH(pnp::launch_pk_mass_apply(dl, pkd, prevu.p, cvec.p, stream), "mass apply");
  else
    CKH(pnp::launch_mass_apply(dl, pnp::OP_DIFF_IE, params.tau, params.pi, params.cylindrical,
                               prevu.p, cvec.p, stream),
        "mass apply");
  return PNP_OK;
}

// r = R(xdev) of the DiffusionOperator `op` while the DiffusionTOperator of the same ion is
// current (same mask, same frozen phi): a residual-only launch on the operator's own load and
// flag buffers, which leaves the stored matrix and every validity flag alone
int pnp_ctx::md_residual_of(const MdOp &op, const double *xdev) {
  const pnp::AsmArgs keep = aa;
  const int kind_keep = kind;
  kind = op.kind;
  aa.kind = op.kind;
  aa.dt = 0.0;
  aa.cvec = op.load.p;
  aa.rowflag = op.flag.p;
  const int rc = assemble(xdev, 0);
  aa = keep;
  kind = kind_keep;
  return rc;
}

// StationaryLinearProblemSolver::apply (src/instationary_pnp_from_pb_md.hh:349-350, 383-386) on
// the resident vector xvec: r = R(x), A = J(x) (jac; else the stored matrix and set-up), A z = r,
// x -= z on the owned rows, ghosts refreshed.  A failed solve sets R.status and leaves x.
int pnp_ctx::md_linear_problem(MdRun &R, double *xvec, bool jac, double reduction,
                               bool diffusion) {
  int rc;
  if ((rc = assemble(xvec, 0))) return rc;
  if (L.n_owned)
    CKH(hipMemcpyAsync(b.p, r.p, sizeof(double) * size_t(L.n_owned), hipMemcpyDeviceToDevice,
                       stream),
        "md right-hand side");
  if (jac) {
    if ((rc = assemble(xvec, 1))) return rc;
    R.res->prec_setups++;
  }
  pnp_solve_opts lo = R.o.linear;
  lo.reduction = reduction;
  pnp_solve_result sr{};
  if ((rc = krylov(b.p, z.p, lo, sr))) return rc;
  (diffusion ? R.res->diffusion_solves : R.res->poisson_solves)++;
  R.res->linear_iterations += sr.iterations;
  if (sr.breakdown) {
    R.status = PNP_E_BREAKDOWN;
    return PNP_OK;
  }
  if (!sr.converged) {
    R.status = PNP_E_NOT_CONVERGED;
    return PNP_OK;
  }
  CKH(pnp::launch_md_sub(L.n_owned, z.p, xvec, stream), "md update");
  return halo(xvec, 1);
}

// OneStepMethod<Alexander2>::apply for one ion (src/instationary_pnp_from_pb_md.hh:372-386), c in
// place; driver/pnp_main.cc alexander2
int pnp_ctx::md_alexander2(MdRun &R, double *c, const MdOp &ie, const MdOp &sp) {
  const double a = 1.0 - 0.5 * std::sqrt(2.0), dt = R.o.dt;
  const bool reuse = R.o.reuse == 1;
  int rc;
  CKH(hipMemcpyAsync(R.u0.p, c, sizeof(double) * size_t(L.n_owned + L.n_ghost),
                     hipMemcpyDeviceToDevice, stream),
      "md u0");
  if ((rc = md_activate(ie, a * dt, R.phi.p, nullptr)) ||
      (rc = md_cvec(ie, 0.0, nullptr, R.u0.p)) ||
      (rc = md_linear_problem(R, c, true, R.o.red_diffusion, true)) || R.status)
    return rc;
  if ((rc = md_residual_of(sp, c))) return rc;  // r1 = R(u1), in r
  // stage 2: the same a dt, z, phi and mask, and the operator is linear in c: stage 1's matrix
  if (!reuse && (rc = md_activate(ie, a * dt, R.phi.p, nullptr))) return rc;
  if ((rc = md_cvec(ie, (1.0 - a) * dt, r.p, R.u0.p))) return rc;
  return md_linear_problem(R, c, !reuse, R.o.red_diffusion, true);
}

int pnp_ctx::md_poisson(MdRun &R) {
  int rc;
  if ((rc = md_activate(R.pois, 0.0, R.cp.p, R.cm.p)) ||
      (rc = md_cvec(R.pois, 0.0, nullptr, nullptr)))
    return rc;
  return md_linear_problem(R, R.phi.p, true, R.o.red_poisson, false);
}

int pnp_ctx::md_run(double *u, const pnp_md_opts &o, int nsurf, int cap, double *t_out,
                    double *ip, double *im, pnp_md_result &res, bool devptr) {
  const double t_start = now_s();
  const int nloc = L.n_owned + L.n_ghost;
  const size_t nlb = sizeof(double) * size_t(nloc);
  MdRun R;
  R.o = o;
  R.res = &res;
  for (DBuf<double> *d : {&R.phi, &R.cp, &R.cm, &R.u0, &R.s_phi, &R.s_cp, &R.s_cm})
    CKH(d->alloc(std::max(1, nloc)), "md state");
  int rc;
  if ((rc = md_op_build(R.ie[0], PNP_OP_DIFF_IMPLICIT_EULER, 1, +1.0)) ||
      (rc = md_op_build(R.ie[1], PNP_OP_DIFF_IMPLICIT_EULER, 2, -1.0)) ||
      (rc = md_op_build(R.sp[0], PNP_OP_DIFF, 1, +1.0)) ||
      (rc = md_op_build(R.sp[1], PNP_OP_DIFF, 2, -1.0)) ||
      (rc = md_op_build(R.pois, PNP_OP_POISSON, 0, 0.0)))
    return rc;
  if ((rc = upload_ext(u, 3, fluxx.p, true, devptr))) return rc;
  CKH(pnp::launch_md_unpack(nloc, fluxx.p, R.phi.p, R.cp.p, R.cm.p, stream), "md unpack");
  const long long va0 = value_assemblies;
  const int upd = std::max(1, int(o.potential_update_freq)), outf = std::max(1, int(o.output_freq));
  std::vector<double> fp(size_t(std::max(1, nsurf))), fm(size_t(std::max(1, nsurf)));
  auto snapshot = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(R.s_phi.p, R.phi.p, nlb, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.s_cp.p, R.cp.p, nlb, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.s_cm.p, R.cm.p, nlb, hipMemcpyDeviceToDevice, stream);
    return e;
  };
  double time = o.t0;
  for (int i = 0; i < o.nsteps && !R.status; i++) {
    CKH(snapshot(), "md snapshot");
    if ((rc = md_alexander2(R, R.cp.p, R.ie[0], R.sp[0]))) return rc;
    if (R.status) break;
    if ((rc = md_alexander2(R, R.cm.p, R.ie[1], R.sp[1]))) return rc;
    if (R.status) break;
    time += o.dt;
    if (i % upd == 0) {
      if ((rc = md_poisson(R))) return rc;
      if (R.status) break;
    }
    if (i % outf == 0) {
      CKH(pnp::launch_md_pack(nloc, R.phi.p, R.cp.p, R.cm.p, fluxx.p, stream), "md pack");
      if ((rc = ion_flux_dev(fluxx.p, nsurf, fp.data(), fm.data()))) return rc;
      const int k = res.noutputs++;
      if (k < cap) {
        t_out[k] = time;
        for (int g = 0; g < nsurf; g++) {
          ip[size_t(k) * nsurf + g] = fp[size_t(g)];
          im[size_t(k) * nsurf + g] = fm[size_t(g)];
        }
      }
    }
    res.steps_done++;
  }
  if (!R.status) {
    CKH(snapshot(), "md snapshot");
    if ((rc = md_poisson(R))) return rc;
  }
  const bool failed = R.status != PNP_OK;
  CKH(pnp::launch_md_pack(nloc, failed ? R.s_phi.p : R.phi.p, failed ? R.s_cp.p : R.cp.p,
                          failed ? R.s_cm.p : R.cm.p, fluxx.p, stream),
      "md pack");
  if ((rc = download_ext(fluxx.p, 3, u, devptr))) return rc;  // synchronises the stream
  if (failed) {  // the operator a failed solve left behind is nobody's: none is current
    kind = -1;
    assembled = false;
  } else if (degree == 1 && !dist) {
    // the Poisson operator stays current: its reference-order copies as pnp_set_operator keeps them
    const size_t nv = size_t(mesh.nv);
    std::vector<double> h(3 * nv);
    CKH(hipMemcpy(h.data(), u, sizeof(double) * h.size(),
                  devptr ? hipMemcpyDeviceToHost : hipMemcpyHostToHost),
        "md final state");
    seq_mask_h = R.pois.gmask;
    seq_cp_h.assign(h.begin() + nv, h.begin() + 2 * nv);
    seq_cm_h.assign(h.begin() + 2 * nv, h.end());
  }
  res.status = R.status;
  res.assemblies = int32_t(value_assemblies - va0);
  res.elapsed = now_s() - t_start;
  return PNP_OK;
}

extern "C" int pnp_md_run(pnp_ctx *c, double *u, const pnp_md_opts *o, int32_t nsurf, int32_t cap,
                          double *t_out, double *ip, double *im, pnp_md_result *res,
                          int32_t flags) {
  if (!c || !u || !o || !res) return PNP_E_ARG;
  if (flags & ~PNP_DEVICE_PTRS) return c->fail(PNP_E_ARG, "unsupported flags for this call");
  if (o->nsteps < 0) return c->fail(PNP_E_ARG, "pnp_md_run: nsteps < 0");
  if (!(o->dt > 0)) return c->fail(PNP_E_ARG, "pnp_md_run: dt must be > 0");
  if (cap < 0 || (cap > 0 && (!t_out || !ip || !im)))
    return c->fail(PNP_E_ARG, "pnp_md_run: cap > 0 needs t_out, ip and im");
  if (nsurf < 0 || nsurf > 256) return c->fail(PNP_E_ARG, "pnp_md_run: nsurf outside [0, 256]");
  if (c->seq_opt)
    return c->fail(PNP_E_STATE, "pnp_md_run is not available in reference-order mode "
                                "(PNP_OPT_SEQ_ORDER)");
  hipSetDevice(c->device);
  std::memset(res, 0, sizeof *res);
  return c->md_run(u, *o, nsurf, cap, t_out, ip, im, *res, (flags & PNP_DEVICE_PTRS) != 0);
}
