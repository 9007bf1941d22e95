// The linear solvers of the context (ctx.h): the preconditioner application, BiCGSTAB, CG,
// restarted GMRES / FGMRES, IDR(s), the pieces they share, and the reference-order drivers.
#include "ctx.h"

// what a preconditioner needs before its first application: factors, split storage, CSR values,
// the AMG hierarchy (each a no-op while still valid)
int pnp_ctx::prec_prepare(int prec) {
  int rc = PNP_OK;
  if (prec == PNP_PREC_ILU0 && !(rc = ilu_factor())) rc = split(2);
  if (prec == PNP_PREC_JACOBI) rc = jacobi_prepare();
  if (prec == PNP_PREC_SSOR) rc = split(1);
  if (prec == PNP_PREC_SSOR_NATURAL) rc = csr_values();
  if (prec == PNP_PREC_AMG) rc = amg_setup();
  // Chebyshev: the diagonal blocks (of their own walk while the SELL values are stale), then the
  // bounds and coefficients
  if (prec == PNP_PREC_CHEBYSHEV && !(rc = jacobi_prepare())) rc = cheb_prepare();
  return rc;
}

// ---- Chebyshev polynomial preconditioner (kernels in linalg.hip) ---------------
// where the diagonal blocks are read from: the SELL values, or, for a Jacobian held as a
// linearisation point whose values nobody needed yet, the blocks of jacobi_prepare()
static const double *cheb_diag(pnp_ctx *c, pnp::DevLayout &Ld) {
  Ld = c->dl;
  if (c->mf_lin && c->vals_stale) {
    Ld.chunk_off = c->mf_choff.p;
    return c->mf_diag.p;
  }
  return c->vals.p;
}

// lambda_est = |w_m| / |w_{m-1}|, w_j = D^-1 A w_{j-1} with halo, no normalisation in between
// (m <= 100 stays inside the fp64 range); the two norms are read at the end
int pnp_ctx::cheb_estimate(double &lest) {
  pnp::DevLayout Ld;
  const double *dv = cheb_diag(this, Ld);
  if (mf_lin && vals_stale && !mf_diag_valid)
    return fail(PNP_E_STATE, "Chebyshev: no diagonal (jacobi_prepare)");
  const int m = cheb_opts.eig_iters;
  int nsp = 0, rc;
  hipError_t e = pnp::launch_cheb_w0(L.n_owned, nf, d_l2g.p, cheb_p[0].p, stream);
  for (int j = 1; j <= m && e == hipSuccess; j++) {
    double *w = cheb_p[(j - 1) & 1].p, *wn = cheb_p[j & 1].p;
    if ((rc = halo_spmv(w, cheb_t.p, 0, nullptr, nullptr, &nsp))) return rc;
    e = pnp::launch_cheb_first(Ld, nf, pat, dv, cheb_t.p, nullptr, nullptr, wn, stream);
  }
  if (e != hipSuccess) return hipfail(e, "chebyshev estimate");
  cheb_ghosts_dirty = true;
  double n0 = 0, n1 = 0;
  if ((rc = norm(cheb_p[(m - 1) & 1].p, n0)) || (rc = norm(cheb_p[m & 1].p, n1))) return rc;
  lest = n0 > 0 ? n1 / n0 : 0.0;
  cheb_estimates++;
  return PNP_OK;
}

// buffers (once), then per stored Jacobian and configuration: bounds, coefficients on the device
int pnp_ctx::cheb_prepare() {
  if (!assembled) return fail(PNP_E_STATE, "no Jacobian assembled");
  if (cheb_valid) return PNP_OK;
  if (!cheb_coef.p) {
    const size_t nl = std::max<size_t>(1, size_t(dl.n_local) * 3);
    hipError_t e;
    if ((e = cheb_r.alloc(nl)) != hipSuccess || (e = cheb_t.alloc(nl)) != hipSuccess ||
        (e = cheb_p[0].alloc(nl)) != hipSuccess || (e = cheb_p[1].alloc(nl)) != hipSuccess ||
        (e = cheb_coef.alloc(pnp::kChebCoefDoubles)) != hipSuccess)
      return hipfail(e, "chebyshev buffers");
  }
  cheb_lest = cheb_lmax = cheb_lmin = 0;
  if (cheb_opts.steps >= 2) {
    double lest = 0;
    if (!(cheb_opts.lambda_max > 0)) {
      hipEvent_t t0 = tb(T_FACT);
      if (int rc = cheb_estimate(lest)) return rc;
      te(T_FACT, t0);
    }
    double lmax, lmin;
    if (!pnp::cheb_bounds(cheb_opts.lambda_max, lest, cheb_opts.eig_boost, cheb_opts.eig_ratio,
                          lmax, lmin) ||
        !pnp::cheb_coefficients(cheb_opts.steps, lmax, lmin, cheb_hcoef))
      return fail(PNP_E_STATE, "Chebyshev: the eigenvalue estimate is zero or not finite");
    // (synchronous: the staging array may be rewritten by the next prepare)
    hipError_t e = hipMemcpyAsync(cheb_coef.p, cheb_hcoef, sizeof cheb_hcoef,
                                  hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hipfail(e, "chebyshev coefficients");
    cheb_lest = lest;
    cheb_lmax = lmax;
    cheb_lmin = lmin;
  }
  cheb_valid = true;
  return PNP_OK;
}

int pnp_ctx::cheb_apply(const double *d, double *vout, bool local) {
  if (!cheb_valid) return fail(PNP_E_STATE, "Chebyshev: not prepared (cheb_prepare)");
  const int k = cheb_opts.steps;
  pnp::DevLayout Ld;
  const double *dv = cheb_diag(this, Ld);
  if (mf_lin && vals_stale && !mf_diag_valid)
    return fail(PNP_E_STATE, "Chebyshev: no diagonal (jacobi_prepare)");
  hipError_t e = hipSuccess;
  cheb_applies++;
  if (local && cheb_ghosts_dirty && L.n_ghost > 0 && k > 1) {  // the rank-local form's zero ghosts
    const size_t off = size_t(L.n_owned) * nf, bytes = sizeof(double) * size_t(L.n_ghost) * nf;
    e = hipMemsetAsync(cheb_p[0].p + off, 0, bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(cheb_p[1].p + off, 0, bytes, stream);
    if (e != hipSuccess) return hipfail(e, "chebyshev ghosts");
    cheb_ghosts_dirty = false;
  }
  e = pnp::launch_cheb_first(Ld, nf, pat, dv, d, k > 1 ? cheb_coef.p : nullptr,
                             k > 1 ? cheb_p[0].p : nullptr, vout, stream);
  if (e != hipSuccess) return hipfail(e, "chebyshev first step");
  // the fused step reads the SELL values on this rank's rows and columns: one rank (or the
  // rank-local form), assembled values, a layout with the SpMV's LDS lists
  const bool fused = pnp::cheb_can_fuse(dl) && !(mf_lin && vals_stale) && (local || nranks == 1);
  for (int i = 1; i < k; i++) {
    double *po = cheb_p[(i - 1) & 1].p, *pn = cheb_p[i & 1].p;
    const double *rin = i == 1 ? d : cheb_r.p;  // step 1 reads d: it is never copied
    const int last = i == k - 1 ? 1 : 0;
    if (fused) {
      e = pnp::launch_cheb_step(dl, nf, pat, vals.p, cheb_coef.p, i, last, rin, cheb_r.p, po, pn,
                                vout, stream);
      cheb_fused++;
    } else {
      int nsp = 0;
      if (local) {
        e = pnp::launch_spmv(dl, nf, pat, vals.p, po, cheb_t.p, 0, nullptr, partials.p, &nsp,
                             stream);
        if (e != hipSuccess) return hipfail(e, "chebyshev spmv");
      } else {
        if (int rc = halo_spmv(po, cheb_t.p, 0, nullptr, nullptr, &nsp)) return rc;
        if (nranks > 1) cheb_ghosts_dirty = true;
      }
      e = pnp::launch_cheb_update(Ld, nf, pat, dv, cheb_coef.p, i, last, rin, cheb_t.p, cheb_r.p,
                                  po, pn, vout, stream);
      cheb_unfused++;
    }
    if (e != hipSuccess) return hipfail(e, "chebyshev step");
  }
  return PNP_OK;
}

// every solver's start: zout = 0, rs = b
int pnp_ctx::solve_start(const double *bdev, double *zout) {
  const size_t bytes = sizeof(double) * nown();
  hipError_t e = hipMemsetAsync(zout, 0, bytes, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(rs.p, bdev, bytes, hipMemcpyDeviceToDevice, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, "solver init");
}

// a solver's initial device state (or its header), from the pinned staging slot the caller filled
int pnp_ctx::state_upload(void *dev, const void *init, size_t bytes, const char *what) {
  hipError_t e = hipMemcpyAsync(dev, init, bytes, hipMemcpyHostToDevice, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, what);
}

// read a solver's device state (or its header) into pinned host memory and wait for it
int pnp_ctx::poll(void *host, const void *dev, size_t bytes, const char *what) {
  hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, what);
}

// allreduce of k device doubles under the allreduce timer (GMRES, IDR); nothing on one rank
int pnp_ctx::allred_timed(double *d, int k) {
  if (!dist) return PNP_OK;
  hipEvent_t t0 = tb(T_ALLRED);
  int rc = allreduce_dev(d, k);
  if (rc) return rc;
  te(T_ALLRED, t0);
  return PNP_OK;
}

// after a solve: the sticky timeout words of the dataflow sweeps the preconditioner may have run
int pnp_ctx::solve_checks(int prec) {
  if (prec == PNP_PREC_SSOR_NATURAL) return nat_check();
  if (prec == PNP_PREC_ILU0) return ilu_flow_check();
  return PNP_OK;
}

void pnp_ctx::solve_result(pnp_solve_result &res, int done, int breakdown, int it, double it_half,
                           double norm0, double norm, double t_start) {
  res.converged = done == 1 ? 1 : 0;
  res.breakdown = breakdown;
  res.iterations = it;
  res.it_half = it_half;
  res.defect0 = norm0;
  res.defect = norm;
  res.reduction = norm0 > 0 ? norm / norm0 : 0.0;
  res.elapsed = now_s() - t_start;
}

// the first `count` entries of a device history into gm_history (pnp_solve_history)
int pnp_ctx::history_download(const double *dev, int count) {
  gm_history.assign(size_t(count), 0.0);
  return poll(gm_history.data(), dev, sizeof(double) * gm_history.size(), "solve history");
}

// the single-level preconditioners, untimed, prerequisites (split / factors) in place
int pnp_ctx::smoother(int prec, const double *d, double *vout, bool in_amg) {
  hipError_t e = hipSuccess;
  if (prec == PNP_PREC_CHEBYSHEV) {
    return cheb_apply(d, vout, in_amg);
  } else if (prec == PNP_PREC_JACOBI && mf_lin && vals_stale) {
    // no SELL values: the diagonal blocks of jacobi_prepare(), one slot per chunk
    if (!mf_diag_valid) return fail(PNP_E_STATE, "Jacobi: no diagonal (jacobi_prepare)");
    pnp::DevLayout dv = dl;
    dv.chunk_off = mf_choff.p;
    e = pnp::launch_jacobi(dv, nf, pat, mf_diag.p, d, vout, stream);
  } else if (prec == PNP_PREC_JACOBI) {
    e = pnp::launch_jacobi(dl, nf, pat, vals.p, d, vout, stream);
  } else if (prec == PNP_PREC_SSOR) {
    e = pnp::launch_sgs(dl, L.color_ptr.data(), nf, pat, lvals.p, uvals.p, d, vout, tsgs.p, stream);
  } else if (prec == PNP_PREC_ILU0) {
    return ilu_apply(d, vout, 0, "preconditioner");
  } else if (prec == PNP_PREC_SSOR_NATURAL) {
    e = ssor_natural(d, vout);
  } else {
    e = hipMemcpyAsync(vout, d, sizeof(double) * nown(), hipMemcpyDeviceToDevice, stream);
  }
  return e == hipSuccess ? PNP_OK : hipfail(e, "preconditioner");
}

// v = M^{-1} d over owned rows (v sized n_local)
int pnp_ctx::precond(int prec, const double *d, double *vout) {
  int rc = prec_prepare(prec);
  if (rc) return rc;
  hipEvent_t t0 = tb(T_PREC);
  if ((rc = prec == PNP_PREC_AMG ? amg_apply(d, vout) : smoother(prec, d, vout))) return rc;
  te(T_PREC, t0);
  return PNP_OK;
}

// BiCGSTAB on J zout = bdev (owned rows), zout zero start.  fixed > 0: exactly that many
// iterations, no convergence stop (reduction 0), used by the benchmarks.
int pnp_ctx::bicgstab(const double *bdev, double *zout, const pnp_solve_opts &o,
                      pnp_solve_result &res, int fixed) {
  if (!assembled) return fail(PNP_E_STATE, "no Jacobian assembled");
  double t_start = now_s();
  long long n = nown();
  int np = pnp::blas_nparts(n);
  int rc, nsp = 0, npu = 0;
  if ((rc = solve_start(bdev, zout))) return rc;
  hipError_t e = hipMemcpyAsync(rt.p, bdev, sizeof(double) * n, hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess) e = hipMemsetAsync(v.p, 0, sizeof(double) * n, stream);
  if (e == hipSuccess) e = hipMemsetAsync(p.p, 0, sizeof(double) * n, stream);
  if (e != hipSuccess) return hipfail(e, "bicgstab init");
  // set reduction, reset flags
  pnp::Scalars &init = hS[2];  // pinned staging slot
  std::memset(&init, 0, sizeof init);
  init.reduction = fixed > 0 ? 0.0 : o.reduction;
  // divergence guard for the AMG preconditioner only (a non-symmetric V-cycle can make
  // BiCGSTAB diverge; ISTL semantics otherwise: run to maxit)
  init.divguard = (o.prec == PNP_PREC_AMG && fixed <= 0) ? 1 : 0;
  if ((rc = state_upload(S.p, &init, sizeof init, "bicgstab scalars"))) return rc;
  hipEvent_t t0 = tb(T_BLAS);
  e = pnp::launch_dot(n, rs.p, rs.p, 0, partials.p, stream);
  if (e != hipSuccess) return hipfail(e, "bicgstab norm0");
  if ((rc = reduce_derive(np, 1, 0))) return rc;
  te(T_BLAS, t0);
  const int maxit = fixed > 0 ? fixed : o.maxit, prec = o.prec;
  const int check = fixed > 0 ? fixed : (o.check_every > 0 ? o.check_every : 8);
  if ((rc = prec_prepare(prec))) return rc;
  // ILU(0): the two vector updates that feed the preconditioner also do colour 0 of its
  // forward sweep (launch_update_fwd0); PNP_FUSE=0 keeps them apart (A/B)
  static const bool fuse_env = [] {
    const char *ev = std::getenv("PNP_FUSE");
    return !(ev && std::atoi(ev) == 0);
  }();
  const bool fuse = fuse_env && prec == PNP_PREC_ILU0 && L.color_ptr.size() > 2;
  const int c0_end = L.color_ptr.size() > 1 ? L.color_ptr[1] : 0;
  // the colour launches record the timer events themselves: the first launch's start and the
  // last launch's end (no marker dispatch in the measured span)
  auto ilu_from1 = [&](const double *d, double *out) -> int {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (timing && L.n_owned > 0) {
      t0 = ev_get();
      t1 = ev_get();
    }
    const int rc1 = ilu_apply(d, out, 1, "preconditioner", t0, t1);
    if (rc1) return rc1;
    if (t1) {
      ev_pending[T_PREC].push_back({t0, t1});
      t_n[T_PREC]++;
    }
    return PNP_OK;
  };
  // two-reduction iteration (two allreduces per iteration instead of three: rho_new from the
  // same reduction as omega, the second half step's test lagged into the next h reduction):
  // on by default with more than one rank, where each reduction is an allreduce round trip;
  // PNP_OPT_BICG_TWORED (or PNP_BICG_TWORED) 0/1 forces it off/on.  Half-step counts keep
  // ISTL's semantics.
  const bool twored = twored_opt >= 0 ? twored_opt == 1 : dist;
  // fused ILU(0), one reduction per half step: the first half step's x += alpha y is applied by
  // the second half's update (one read and write of x per iteration fewer; the second
  // preconditioned vector then goes to y2).  PNP_XDEFER=0 keeps the two passes (A/B).
  static const bool xdefer_env = [] {
    const char *ev = std::getenv("PNP_XDEFER");
    return !(ev && std::atoi(ev) == 0);
  }();
  const bool xdefer = xdefer_env && fuse && !twored;
  double *const y2p = xdefer ? y2.p : y.p;
  int pending_np = 0;
  // one BiCGSTAB iteration; for k >= 1 (and without the two-reduction variant's host state) it
  // launches the same kernels with the same arguments every time, which is what the graph
  // replay below relies on
  auto body = [&](int k) -> int {
    // p = r + beta (p - omega v)
    hipEvent_t t0 = tb(T_BLAS);
    if (fuse)
      e = pnp::launch_update_fwd0(dl, nf, pat, c0_end, S.p, 0, k == 0 ? 1 : 0, nullptr, nullptr,
                                  rs.p, v.p, p.p, uvals.p, y.p, nullptr, nullptr, stream,
                                  f32_now(), nullptr, ilu_y32());
    else
      e = pnp::launch_update_p(n, S.p, rs.p, v.p, p.p, k == 0 ? 1 : 0, stream);
    if (e != hipSuccess) return hipfail(e, "update_p");
    te(T_BLAS, t0);
    // y = M^{-1} p ; v = A y ; h = <rt, v>
    const double *yin = p.p;
    if (fuse) {
      if ((rc = ilu_from1(p.p, y.p))) return rc;
      yin = y.p;
    } else if (prec != PNP_PREC_NONE) {
      if ((rc = precond(prec, p.p, y.p))) return rc;
      yin = y.p;
    }
    if ((rc = halo_spmv(const_cast<double *>(yin), v.p, 1, rt.p, nullptr, &nsp))) return rc;
    if (twored)  // h, with the previous iteration's second-half test (||r||^2 in partials2)
      rc = pending_np > 0 ? reduce_derive2(nsp, 1, pending_np, 1, 31) : reduce_derive(nsp, 1, 31);
    else
      rc = reduce_derive(nsp, 1, 1);
    if (rc) return rc;
    // x += alpha y ; r -= alpha v ; ||r|| (partials2: its half-step test is derived together
    // with omega below -- one reduction and one allreduce fewer per iteration; the second
    // half's kernels ignore a converged first half, update_xr skips on S->done).  Two-reduction
    // iteration (twored): also <rt, s> into partials2, for rho_new without a third reduction.
    t0 = tb(T_BLAS);
    if (fuse)
      e = pnp::launch_update_fwd0(dl, nf, pat, c0_end, S.p, 1, 0, xdefer ? nullptr : zout, yin,
                                  rs.p, v.p, nullptr, uvals.p, y2p, partials2.p, &npu, stream,
                                  f32_now(), twored ? rt.p : nullptr, ilu_y32());
    else
      e = pnp::launch_update_xr(n, S.p, 0, zout, yin, rs.p, v.p, twored ? rt.p : nullptr,
                                partials2.p, stream);
    if (e != hipSuccess) return hipfail(e, "update x r (1)");
    te(T_BLAS, t0);
    // y = M^{-1} r ; t = A y ; <t,r>, <t,t> (twored: and <t,rt>)
    const double *yin2 = rs.p;
    if (fuse) {
      if ((rc = ilu_from1(rs.p, y2p))) return rc;
      yin2 = y2p;
    } else if (prec != PNP_PREC_NONE) {
      if ((rc = precond(prec, rs.p, y.p))) return rc;
      yin2 = y.p;
    }
    if ((rc = halo_spmv(const_cast<double *>(yin2), t.p, twored ? 4 : 2, rs.p, rt.p, &nsp)))
      return rc;
    if (twored) {
      if ((rc = reduce_derive2(nsp, 3, fuse ? npu : np, 2, 32))) return rc;
      // x += omega y ; r -= omega t ; ||r||^2 into partials2, tested at the next h (stage 31)
      t0 = tb(T_BLAS);
      e = pnp::launch_update_xr(n, S.p, 1, zout, yin2, rs.p, t.p, nullptr, partials2.p, stream);
      if (e != hipSuccess) return hipfail(e, "update x r (2)");
      te(T_BLAS, t0);
      pending_np = np;
    } else {
      if ((rc = reduce_derive2(nsp, 2, fuse ? npu : np, 1, 23))) return rc;
      // x += omega y ; r -= omega t ; ||r||, <rt, r>
      t0 = tb(T_BLAS);
      e = pnp::launch_update_xr(n, S.p, 1, zout, yin2, rs.p, t.p, rt.p, partials.p, stream,
                                xdefer ? yin : nullptr);
      if (e != hipSuccess) return hipfail(e, "update x r (2)");
      if ((rc = reduce_derive(np, 2, 4))) return rc;
      te(T_BLAS, t0);
    }
    if (debug_trace) {
      (void)poll(hS, S.p, sizeof(pnp::Scalars), "bicgstab trace");
      std::fprintf(stderr,
                   "bicgstab it=%d it_half=%.1f rho=%.6e rho_new=%.6e alpha=%.6e omega=%.6e "
                   "h=%.6e norm=%.6e done=%d bd=%d\n",
                   k + 1, hS->it_half, hS->rho, hS->rho_new, hS->alpha, hS->omega, hS->h,
                   hS->norm, hS->done, hS->breakdown);
    }
    return PNP_OK;
  };
  // the iterations between two polls of the device scalars (every `check`): eagerly, or as one
  // hipGraph replay (small systems, where launching ~20 kernels per iteration from the host
  // costs more than running them: PNP_OPT_GRAPH)
  bool graphs = use_graphs() && !dist && !twored && !debug_trace && !timing &&
                prec != PNP_PREC_AMG && !graphs_failed;
  for (int k = 0; k < maxit;) {
    const int kend = std::min(maxit, (k / check + 1) * check);  // next poll
    if (k == 0) {
      if ((rc = body(0))) return rc;
      k = 1;
    }
    // whole graph blocks of glen iterations (one captured graph per block length, replayed as
    // often as the poll interval holds it), the remainder eagerly; a capture or instantiation
    // failure turns graphs off for the rest of the solve (eager launches, same results)
    const int glen = std::min(check, 16);
    while (graphs && glen > 1 && kend - k >= glen) {
      const GraphKey key{glen, prec, fuse ? 1 : 0, nf, pat, f32_now() + (ilu_y32() ? 4 : 0),
                         ilu_flow_opt * 4 + (nat_flow_opt + 1),
                         mf_lin ? (vals_stale ? 2 : 1) : 0, zout, dl.dmask, graph_epoch};
      bool captured = true;
      rc = graph_run(key, [&]() -> int {
        for (int i = 0; i < key.count; i++)
          if (int r2 = body(1)) return r2;
        return PNP_OK;
      }, &captured);
      if (rc && !captured) {  // the graph path failed before anything ran: eager from here
        graphs_failed = true;
        graphs = false;
        break;
      }
      if (rc) return rc;
      k += glen;
    }
    for (; k < kend; k++)
      if ((rc = body(k))) return rc;
    if ((rc = poll(hS, S.p, sizeof(pnp::Scalars), "bicgstab poll"))) return rc;
    if (hS->done) break;
  }
  if (twored && pending_np > 0 && (rc = reduce_derive(pending_np, 1, 33, true))) return rc;
  if ((rc = poll(hS, S.p, sizeof(pnp::Scalars), "bicgstab result"))) return rc;
  if ((rc = solve_checks(prec))) return rc;
  const double it = std::min(double(maxit), hS->it_half);
  solve_result(res, hS->done, hS->breakdown, int(std::ceil(it)), it, hS->norm0, hS->norm, t_start);
  return PNP_OK;
}

// ISTL CGSolver on J zout = bdev (owned rows), zout zero start; device-resident scalars
// (derive stages 10-14).  iterations = matrix-vector products.
int pnp_ctx::cg(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res) {
  if (!assembled) return fail(PNP_E_STATE, "no Jacobian assembled");
  double t_start = now_s();
  long long n = nown();
  int np = pnp::blas_nparts(n);
  int prec = o.prec, nsp = 0, rc;
  if ((rc = solve_start(bdev, zout))) return rc;
  pnp::Scalars &init = hS[2];
  std::memset(&init, 0, sizeof init);
  init.reduction = o.reduction;
  if ((rc = state_upload(S.p, &init, sizeof init, "cg scalars"))) return rc;
  hipError_t e = pnp::launch_dot(n, rs.p, rs.p, 0, partials.p, stream);
  if (e != hipSuccess) return hipfail(e, "cg norm0");
  if ((rc = reduce_derive(np, 1, 10))) return rc;
  if ((rc = precond(prec, rs.p, p.p))) return rc;  // p = M^{-1} r
  if ((e = pnp::launch_dot(n, p.p, rs.p, 0, partials.p, stream)) != hipSuccess)
    return hipfail(e, "cg rho");
  if ((rc = reduce_derive(np, 1, 11))) return rc;
  int check = o.check_every > 0 ? o.check_every : 8;
  for (int k = 0; k < o.maxit; k++) {
    if ((rc = halo_spmv(p.p, v.p, 1, p.p, nullptr, &nsp))) return rc;
    if ((rc = reduce_derive(nsp, 1, 12))) return rc;
    hipEvent_t t0 = tb(T_BLAS);
    e = pnp::launch_update_xr(n, S.p, 0, zout, p.p, rs.p, v.p, nullptr, partials.p, stream);
    if (e != hipSuccess) return hipfail(e, "cg update");
    if ((rc = reduce_derive(np, 1, 13))) return rc;
    te(T_BLAS, t0);
    if ((k + 1) % check == 0 || k + 1 == o.maxit) {
      if ((rc = poll(hS, S.p, sizeof(pnp::Scalars), "cg poll"))) return rc;
      if (hS->done) break;
    }
    if ((rc = precond(prec, rs.p, y.p))) return rc;  // q = M^{-1} r
    t0 = tb(T_BLAS);
    if ((e = pnp::launch_dot(n, y.p, rs.p, 0, partials.p, stream)) != hipSuccess)
      return hipfail(e, "cg rho'");
    if ((rc = reduce_derive(np, 1, 14))) return rc;
    if ((e = pnp::launch_cg_update_p(n, S.p, y.p, p.p, stream)) != hipSuccess)
      return hipfail(e, "cg p");
    te(T_BLAS, t0);
  }
  if ((rc = poll(hS, S.p, sizeof(pnp::Scalars), "cg result"))) return rc;
  if ((rc = solve_checks(prec))) return rc;
  solve_result(res, hS->done, 0, hS->iter, hS->iter, hS->norm0, hS->norm, t_start);
  return PNP_OK;
}

// Restarted GMRES(m) (flexible: the preconditioned basis Z is kept, x = x0 + Z y) on
// J zout = bdev (owned rows), zero start, right-preconditioned: the monitored norm is the true
// residual's.  DESIGN.md 4.8.  The state (Hessenberg matrix, rotations, history, flags) lives on
// the device (gmres_small.h); the host enqueues Arnoldi steps and reads the state's header only
// at the check_every poll.  A cycle ends on the device (phase 1: the step kernels idle) when the
// estimate meets the test, at the restart length or at maxit; the host enqueues the cycle end
// (x update, r = b - A x, the true norm, the next cycle's V_0) where it knows a cycle is over:
// after m steps, or after a poll that shows phase 1.  Until then the preconditioner and the
// SpMV of the enqueued steps run on vectors nobody reads.
int pnp_ctx::gmres_alloc(bool flexible) {
  const size_t ld = (size_t(nf) * size_t(dl.n_local) + 1) & ~size_t(1);
  const int m = gm_restart;
  hipError_t e = hipSuccess;
  if (gm_V.n != ld * size_t(m + 1)) e = gm_V.alloc(ld * size_t(m + 1));
  if (e == hipSuccess && flexible && gm_Z.n != ld * size_t(m)) e = gm_Z.alloc(ld * size_t(m));
  const size_t nps = size_t(pnp::gmres_nparts(nown()));
  if (e == hipSuccess && gm_part.n != nps * (pnp::kGmMaxRestart + 2))
    e = gm_part.alloc(nps * (pnp::kGmMaxRestart + 2));
  if (e == hipSuccess && !gm_S.p) e = gm_S.alloc(1);
  return e == hipSuccess ? PNP_OK : hipfail(e, "gmres basis");
}

void pnp_ctx::gmres_free() {
  gm_V.release();
  gm_Z.release();
  gm_part.release();
}

int pnp_ctx::gmres(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res,
                   bool flexible) {
  if (!assembled) return fail(PNP_E_STATE, "no Jacobian assembled");
  if (o.maxit < 0) return fail(PNP_E_ARG, "maxit must not be negative");
  static_assert(offsetof(pnp::GmresState, red1) <= sizeof(pnp::Scalars), "poll staging");
  const size_t hdr = offsetof(pnp::GmresState, red1);
  double t_start = now_s();
  const long long n = nown();
  const int m = gm_restart, prec = o.prec;
  if (prec == PNP_PREC_NONE) flexible = false;  // Z = V
  int rc;
  if ((rc = gmres_alloc(flexible))) return rc;
  const long long ld = (long long)((size_t(nf) * size_t(dl.n_local) + 1) & ~size_t(1));
  const int nps = pnp::gmres_nparts(n);
  hipError_t e = hipSuccess;
  // the history keeps the first kGmHistCap steps: a "no limit" maxit must not size a buffer
  const int hcap = std::min(o.maxit, pnp::kGmHistCap);
  if (gm_hist.n < size_t(hcap) + 2) e = gm_hist.alloc(size_t(hcap) + 2);
  if (e != hipSuccess) return hipfail(e, "gmres history");
  if ((rc = prec_prepare(prec))) return rc;
  pnp::GmresState *St = gm_S.p, *hp = reinterpret_cast<pnp::GmresState *>(hS);  // hp: header only
  pnp::GmresState *init = reinterpret_cast<pnp::GmresState *>(hS + 2);
  std::memset(init, 0, hdr);
  init->reduction = o.reduction;
  init->m = m;
  init->maxit = o.maxit;
  init->phase = 1;  // the start is a cycle end with no columns
  init->hcap = hcap;
  if ((rc = state_upload(St, init, hdr, "gmres init"))) return rc;
  if ((rc = solve_start(bdev, zout))) return rc;
  auto V = [&](int i) { return gm_V.p + size_t(i) * size_t(ld); };
  auto Z = [&](int i) { return gm_Z.p + size_t(i) * size_t(ld); };
  // ||rs||, the true norm's test, V_0 of the next cycle
  auto close_cycle = [&](int first) -> int {
    hipEvent_t t0 = tb(T_BLAS);
    hipError_t e2 = pnp::launch_gmres_norm2(St, rs.p, n, gm_part.p, nps, stream);
    if (e2 != hipSuccess) return hipfail(e2, "gmres norm");
    te(T_BLAS, t0);
    int r2 = allred_timed(St->red3, 1);
    if (r2) return r2;
    t0 = tb(T_BLAS);
    e2 = pnp::launch_gmres_restart(St, gm_hist.p, first, gm_V.p, ld, n, rs.p, stream);
    if (e2 != hipSuccess) return hipfail(e2, "gmres restart");
    te(T_BLAS, t0);
    return PNP_OK;
  };
  const bool direct = flexible || prec == PNP_PREC_NONE;  // the basis combination is x's update
  auto cycle_end = [&]() -> int {
    int nsp = 0, r2;
    hipEvent_t t0 = tb(T_BLAS);
    hipError_t e2 = pnp::launch_gmres_backsub(St, stream);
    if (e2 == hipSuccess)  // x += Z y (flexible) or x += V y (no preconditioner), else t = V y
      e2 = pnp::launch_gmres_combine(St, flexible ? gm_Z.p : gm_V.p, ld, n, direct ? zout : t.p,
                                     direct ? 1 : 0, stream);
    if (e2 != hipSuccess) return hipfail(e2, "gmres update");
    te(T_BLAS, t0);
    if (!direct) {  // x += M^-1 t
      if ((r2 = precond(prec, t.p, y.p))) return r2;
      t0 = tb(T_BLAS);
      if ((e2 = pnp::launch_gmres_xpy(St, zout, y.p, n, stream)) != hipSuccess)
        return hipfail(e2, "gmres update");
      te(T_BLAS, t0);
    }
    if ((r2 = halo_spmv(zout, rs.p, 3, bdev, nullptr, &nsp))) return r2;  // r = b - A x
    return close_cycle(0);
  };
  // one Arnoldi step with the host's column index hj (the device's own j while it steps)
  auto step = [&](int hj) -> int {
    int nsp = 0, r2;
    double *in = V(hj);
    if (prec != PNP_PREC_NONE) {
      in = flexible ? Z(hj) : y.p;
      if ((r2 = precond(prec, V(hj), in))) return r2;
    }
    if ((r2 = halo_spmv(in, V(hj + 1), 0, nullptr, nullptr, &nsp))) return r2;
    double *red[3] = {St->red1, St->red2, St->red3};
    const int cnt[3] = {hj + 2, hj + 1, 1};
    for (int pass = 0; pass < 3; pass++) {
      hipEvent_t t0 = tb(T_BLAS);
      hipError_t e2 = pnp::launch_gmres_orth(pass, St, gm_V.p, ld, n, gm_part.p, nps, hj, stream);
      if (e2 != hipSuccess) return hipfail(e2, "gmres orthogonalisation");
      te(T_BLAS, t0);
      if ((r2 = allred_timed(red[pass], cnt[pass]))) return r2;
    }
    hipEvent_t t0 = tb(T_BLAS);
    hipError_t e2 = pnp::launch_gmres_hess(St, gm_hist.p, gm_V.p, ld, n, stream);
    if (e2 != hipSuccess) return hipfail(e2, "gmres hessenberg");
    te(T_BLAS, t0);
    return PNP_OK;
  };
  auto poll_hdr = [&]() { return poll(hp, St, hdr, "gmres poll"); };
  if ((rc = close_cycle(1))) return rc;
  const int check = o.check_every > 0 ? o.check_every : 8;
  int hj = 0, it_known = 0;
  if ((rc = poll_hdr())) return rc;
  while (!hp->done) {
    // steps until the next poll: never past the restart length or maxit, and one at a time
    // once the estimate is within a decade of the target (a step enqueued after the device has
    // ended the cycle costs a whole preconditioner application and an SpMV for nothing)
    const bool near = hp->norm < 10.0 * o.reduction * hp->norm0;
    const int ns = std::max(1, std::min({near ? 1 : check, m - hj, o.maxit - it_known}));
    for (int q = 0; q < ns; q++, hj++)
      if ((rc = step(hj))) return rc;
    if (hj == m) {  // the device's cycle is over at the latest now
      if ((rc = cycle_end())) return rc;
      hj = 0;
    }
    if ((rc = poll_hdr())) return rc;
    if (hp->done) break;
    if (hp->phase == 1) {  // ended early on the device: estimate met, maxit or breakdown
      if ((rc = cycle_end())) return rc;
      hj = 0;
      if ((rc = poll_hdr())) return rc;
    }
    it_known = hp->it;
  }
  if ((rc = solve_checks(prec))) return rc;
  if ((rc = history_download(gm_hist.p, std::min(hp->it, hcap) + 1))) return rc;
  solve_result(res, hp->done, hp->breakdown, hp->it, hp->it, hp->norm0, hp->norm, t_start);
  return PNP_OK;
}

// IDR(s), bi-orthogonal variant, on J zout = bdev (owned rows), zero start, right-preconditioned:
// the monitored norm is the true system's residual's.  DESIGN.md 4.10.  The state (M, f, c,
// alpha, beta, omega, counters, flags) lives on the device (idr_small.h); the host enqueues the
// fixed sequence step 0 .. s - 1, omega step, step 0, ... and reads the state's header only at
// the check_every poll.  When the recurrence's norm meets the test (or at maxit, or on a
// breakdown) the device enters phase 2 and every later step kernel idles; the host, once a poll
// shows it, forms r = b - A x and the device judges the true norm: stop, or go on from that
// residual with G = U = 0, M = I, omega = 1 (a residual replacement).
long long pnp_ctx::idr_ld(bool ghosts) const {
  const size_t rows = ghosts ? size_t(dl.n_local) : size_t(L.n_owned);
  return (long long)((size_t(nf) * rows + 1) & ~size_t(1));
}

void pnp_ctx::idr_free() {
  idr_G.release();
  idr_U.release();
  idr_P.release();
  idr_part.release();
  idr_P_s = idr_P_nf = 0;
}

// the shadow matrix for the current s and field count: counter-based entries by global vertex,
// then modified Gram-Schmidt with one reduction (and allreduce) per dot product
int pnp_ctx::idr_shadow_build() {
  const int s = idr_s;
  if (idr_P_s == s && idr_P_nf == nf && idr_P.p) return PNP_OK;
  const long long n = nown(), ldg = idr_ld(false);
  const int nps = pnp::idr_nparts(n);
  hipError_t e = hipSuccess;
  idr_P_s = idr_P_nf = 0;
  if (idr_P.n != size_t(ldg) * s) e = idr_P.alloc(size_t(ldg) * s);
  if (e == hipSuccess && idr_part.n != size_t(nps) * (pnp::kIdrMaxS + 4))
    e = idr_part.alloc(size_t(nps) * (pnp::kIdrMaxS + 4));
  if (e == hipSuccess && !idr_S.p) e = idr_S.alloc(1);
  if (e == hipSuccess)
    e = pnp::launch_idr_shadow_fill(L.n_owned, nf, s, d_l2g.p, idr_P.p, ldg, stream);
  if (e != hipSuccess) return hipfail(e, "idr shadow");
  auto col = [&](int j) { return idr_P.p + size_t(j) * size_t(ldg); };
  int rc;
  for (int j = 0; j < s; j++) {
    for (int i = 0; i <= j; i++) {  // i == j: the norm
      e = pnp::launch_idr_dot(idr_S.p, col(i), col(j), n, idr_part.p, nps, stream);
      if (e != hipSuccess) return hipfail(e, "idr shadow");
      if ((rc = allreduce_dev(pnp::idr_red(idr_S.p), 1))) return rc;
      e = pnp::launch_idr_mgs(idr_S.p, col(j), i < j ? col(i) : nullptr, n, stream);
      if (e != hipSuccess) return hipfail(e, "idr shadow");
    }
  }
  idr_P_s = s;
  idr_P_nf = nf;
  return PNP_OK;
}

int pnp_ctx::idr_alloc() {
  const int s = idr_s;
  const size_t ldg = size_t(idr_ld(false)), ldu = size_t(idr_ld(true));
  hipError_t e = hipSuccess;
  if (idr_G.n != ldg * s) e = idr_G.alloc(ldg * s);
  if (e == hipSuccess && idr_U.n != ldu * s) e = idr_U.alloc(ldu * s);
  if (e != hipSuccess) return hipfail(e, "idr arrays");
  return idr_shadow_build();
}

int pnp_ctx::idr(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res) {
  if (!assembled) return fail(PNP_E_STATE, "no Jacobian assembled");
  if (o.maxit < 0) return fail(PNP_E_ARG, "maxit must not be negative");
  static_assert(offsetof(pnp::IdrState, red) <= sizeof(pnp::Scalars), "poll staging");
  const size_t hdr = offsetof(pnp::IdrState, red);
  double t_start = now_s();
  const long long n = nown();
  const int s = idr_s, prec = o.prec;
  int rc;
  if ((rc = idr_alloc())) return rc;
  const long long ldg = idr_ld(false), ldu = idr_ld(true);
  const int nps = pnp::idr_nparts(n);
  hipError_t e = hipSuccess;
  const int hcap = std::min(o.maxit, pnp::kIdrHistCap);
  if (idr_hist.n < size_t(hcap) + 2) e = idr_hist.alloc(size_t(hcap) + 2);
  if (e != hipSuccess) return hipfail(e, "idr history");
  if ((rc = prec_prepare(prec))) return rc;
  pnp::IdrState *St = idr_S.p, *hp = reinterpret_cast<pnp::IdrState *>(hS);  // hp: header only
  double *red = pnp::idr_red(St);
  pnp::IdrState *init = reinterpret_cast<pnp::IdrState *>(hS + 2);
  std::memset(init, 0, hdr);
  init->reduction = o.reduction;
  init->omega = 1.0;
  init->s = s;
  init->maxit = o.maxit;
  init->phase = 2;  // the start is a judged residual like any other
  init->hcap = hcap;
  if ((rc = state_upload(St, init, hdr, "idr init"))) return rc;
  if ((rc = solve_start(bdev, zout))) return rc;
  auto G = [&](int i) { return idr_G.p + size_t(i) * size_t(ldg); };
  auto U = [&](int i) { return idr_U.p + size_t(i) * size_t(ldu); };
  auto allred = [&](int k) { return allred_timed(red, k); };
  auto small = [&](int which, int hk) -> int {
    hipError_t e2 = pnp::launch_idr_small(St, idr_hist.p, which, hk, stream);
    return e2 == hipSuccess ? PNP_OK : hipfail(e2, "idr state");
  };
  // rs holds a true residual: its norm and P^T rs, the verdict, and a clean start if it goes on
  auto begin = [&](int first) -> int {
    hipEvent_t t0 = tb(T_BLAS);
    hipError_t e2 = pnp::launch_idr_resid_dots(St, s, rs.p, idr_P.p, ldg, n, idr_part.p, nps, stream);
    if (e2 == hipSuccess) e2 = hipMemsetAsync(idr_G.p, 0, sizeof(double) * idr_G.n, stream);
    if (e2 == hipSuccess) e2 = hipMemsetAsync(idr_U.p, 0, sizeof(double) * idr_U.n, stream);
    if (e2 != hipSuccess) return hipfail(e2, "idr residual");
    te(T_BLAS, t0);
    int r2 = allred(s + 1);
    if (r2) return r2;
    return small(4, first);
  };
  auto step = [&](int hk) -> int {
    int nsp = 0, r2;
    hipEvent_t t0 = tb(T_BLAS);
    hipError_t e2 = pnp::launch_idr_v(St, hk, rs.p, idr_G.p, ldg, n, t.p, stream);
    if (e2 != hipSuccess) return hipfail(e2, "idr v");
    te(T_BLAS, t0);
    const double *vh = t.p;
    if (prec != PNP_PREC_NONE) {
      if ((r2 = precond(prec, t.p, y.p))) return r2;
      vh = y.p;
    }
    t0 = tb(T_BLAS);
    if ((e2 = pnp::launch_idr_u(St, hk, vh, idr_U.p, ldu, n, stream)) != hipSuccess)
      return hipfail(e2, "idr u");
    te(T_BLAS, t0);
    if ((r2 = halo_spmv(U(hk), G(hk), 0, nullptr, nullptr, &nsp))) return r2;
    t0 = tb(T_BLAS);
    e2 = pnp::launch_idr_ptg(St, hk, s, idr_G.p, ldg, idr_P.p, n, idr_part.p, nps, stream);
    if (e2 != hipSuccess) return hipfail(e2, "idr shadow products");
    te(T_BLAS, t0);
    if ((r2 = allred(s))) return r2;
    t0 = tb(T_BLAS);
    if ((r2 = small(0, hk))) return r2;
    e2 = pnp::launch_idr_update(St, hk, idr_G.p, ldg, idr_U.p, ldu, rs.p, zout, n, idr_part.p,
                                nps, stream);
    if (e2 != hipSuccess) return hipfail(e2, "idr update");
    te(T_BLAS, t0);
    if ((r2 = allred(1))) return r2;
    return small(1, hk);
  };
  auto omega_step = [&]() -> int {
    int nsp = 0, r2;
    double *const vh = y.p;
    if (prec != PNP_PREC_NONE) {
      if ((r2 = precond(prec, rs.p, vh))) return r2;
    } else {  // the SpMV's input carries ghosts, which the exchange writes: not into rs
      hipError_t e2 = hipMemcpyAsync(vh, rs.p, sizeof(double) * n, hipMemcpyDeviceToDevice, stream);
      if (e2 != hipSuccess) return hipfail(e2, "idr copy");
    }
    if ((r2 = halo_spmv(vh, t.p, 0, nullptr, nullptr, &nsp))) return r2;
    hipEvent_t t0 = tb(T_BLAS);
    hipError_t e2 = pnp::launch_idr_om_dots(St, t.p, rs.p, n, idr_part.p, nps, stream);
    if (e2 != hipSuccess) return hipfail(e2, "idr omega");
    te(T_BLAS, t0);
    if ((r2 = allred(3))) return r2;
    t0 = tb(T_BLAS);
    if ((r2 = small(2, 0))) return r2;
    e2 = pnp::launch_idr_om_update(St, s, t.p, vh, rs.p, zout, idr_P.p, ldg, n, idr_part.p, nps,
                                   stream);
    if (e2 != hipSuccess) return hipfail(e2, "idr omega update");
    te(T_BLAS, t0);
    if ((r2 = allred(s + 1))) return r2;
    return small(3, 0);
  };
  auto poll_hdr = [&]() { return poll(hp, St, hdr, "idr poll"); };
  if ((rc = begin(1))) return rc;
  const int check = o.check_every > 0 ? o.check_every : 8;
  int hk = 0, it_known = 0;  // hk == s: the omega step is next
  if ((rc = poll_hdr())) return rc;
  while (!hp->done) {
    // applications until the next poll: never past maxit, and one at a time once the norm is
    // within a decade of the target (an application enqueued after the recurrence has ended
    // costs a preconditioner application and an SpMV for nothing)
    const bool near = hp->norm < 10.0 * o.reduction * hp->norm0;
    const int ns = std::max(1, std::min(near ? 1 : check, o.maxit - it_known));
    for (int q = 0; q < ns; q++) {
      if ((rc = hk < s ? step(hk) : omega_step())) return rc;
      hk = hk < s ? hk + 1 : 0;
    }
    if ((rc = poll_hdr())) return rc;
    if (hp->done) break;
    if (hp->phase == 2) {  // the recurrence has ended: the true residual decides
      int nsp = 0;
      if ((rc = halo_spmv(zout, rs.p, 3, bdev, nullptr, &nsp))) return rc;  // r = b - A x
      if ((rc = begin(0))) return rc;
      hk = 0;
      if ((rc = poll_hdr())) return rc;
    }
    it_known = hp->it;
  }
  if ((rc = solve_checks(prec))) return rc;
  if ((rc = history_download(idr_hist.p, std::min(hp->it, hcap) + 1))) return rc;
  idr_replacements += hp->replacements;
  solve_result(res, hp->done, hp->breakdown, hp->it, hp->it, hp->norm0, hp->norm, t_start);
  return PNP_OK;
}

// v = M^{-1} d with v zero on entry (ISTL's preconditioners from y = 0)
int pnp_ctx::seq_prec(int prec, const double *d, double *v) {
  const int n = nseq();
  hipError_t e;
  if (prec == PNP_PREC_NONE || prec == PNP_PREC_JACOBI) {
    e = pnp::launch_seq_prec_diag(n, prec == PNP_PREC_JACOBI, d, csr_diag.p, csr_val.p, v, stream);
  } else {  // SSOR_NATURAL: the natural-order sweep on the CSR view (internal positions)
    e = pnp::launch_gather_ext(L.n_owned, nf, mesh.nv, d_l2g.p, d, nat_di.p, stream);
    if (e == hipSuccess) e = nat_sweep(nat_di.p, nat_vi.p);
    if (e == hipSuccess) e = pnp::launch_scatter_ext(L.n_owned, nf, mesh.nv, d_l2g.p, nat_vi.p, v, stream);
  }
  return e == hipSuccess ? PNP_OK : hipfail(e, "seq preconditioner");
}

// ISTL BiCGSTABSolver::apply in the oracle's statements (oracle/pnp_oracle.c orc_bicgstab):
// x (zero start) and b (overwritten by the residual), external layout on the device
int pnp_ctx::seq_bicgstab(int prec, double reduction, int maxit, double *x, double *b,
                          pnp_solve_result &res) {
  const double EPSILON = 1e-80;
  const int n = nseq();
  double *r = b, *p = sq(SQ_P), *v = sq(SQ_V), *t = sq(SQ_T), *y = sq(SQ_Y), *rt = sq(SQ_RT);
  int rc = PNP_OK;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t ee) {
    if (e == hipSuccess) e = ee;
  };
  for (double *q : {p, v, t, y}) ck(hipMemsetAsync(q, 0, sizeof(double) * n, stream));
  std::memset(&res, 0, sizeof res);
  ck(pnp::launch_seq_spmv(n, csr_rowptr.p, csr_col.p, csr_val.p, x, t, stream));  // r = b - A x
  ck(pnp::launch_seq_aymx(n, 1.0, r, t, stream));
  ck(hipMemcpyAsync(rt, r, sizeof(double) * n, hipMemcpyDeviceToDevice, stream));
  if (e != hipSuccess) return hipfail(e, "seq bicgstab");
  double norm = std::sqrt(seq_dot(r, r, rc)), norm_0 = norm;
  if (rc) return rc;
  double rho = 1, alpha = 1, omega = 1, rho_new = 0, beta, h;
  res.defect0 = norm_0;
  double it = 0;
  if (norm < reduction * norm_0 || norm < 1e-30) {
    res.converged = 1;
    res.defect = norm;
    return PNP_OK;
  }
  for (it = 0.5; it < maxit; it += .5) {
    rho_new = seq_dot(rt, r, rc);
    if (rc) return rc;
    if (std::fabs(rho) <= EPSILON) { res.breakdown = 1; break; }
    if (std::fabs(omega) <= EPSILON) { res.breakdown = 2; break; }
    if (it < 1) {
      ck(hipMemcpyAsync(p, r, sizeof(double) * n, hipMemcpyDeviceToDevice, stream));
    } else {
      beta = (rho_new / rho) * (alpha / omega);
      ck(pnp::launch_seq_bicg_p(n, beta, omega, p, v, r, stream));
    }
    ck(hipMemsetAsync(y, 0, sizeof(double) * n, stream));
    if (e != hipSuccess) return hipfail(e, "seq bicgstab");
    if ((rc = seq_prec(prec, p, y))) return rc;
    ck(pnp::launch_seq_spmv(n, csr_rowptr.p, csr_col.p, csr_val.p, y, v, stream));
    if (e != hipSuccess) return hipfail(e, "seq bicgstab");
    h = seq_dot(rt, v, rc);
    if (rc) return rc;
    if (std::fabs(h) < EPSILON) { res.breakdown = 3; break; }
    alpha = rho_new / h;
    ck(pnp::launch_seq_axpy2(n, alpha, x, y, r, v, stream));
    if (e != hipSuccess) return hipfail(e, "seq bicgstab");
    norm = std::sqrt(seq_dot(r, r, rc));
    if (rc) return rc;
    if (norm < reduction * norm_0) { res.converged = 1; break; }
    it += .5;
    ck(hipMemsetAsync(y, 0, sizeof(double) * n, stream));
    if (e != hipSuccess) return hipfail(e, "seq bicgstab");
    if ((rc = seq_prec(prec, r, y))) return rc;
    ck(pnp::launch_seq_spmv(n, csr_rowptr.p, csr_col.p, csr_val.p, y, t, stream));
    if (e != hipSuccess) return hipfail(e, "seq bicgstab");
    const double tr = seq_dot(t, r, rc);
    if (rc) return rc;
    const double tt = seq_dot(t, t, rc);
    if (rc) return rc;
    omega = tr / tt;
    ck(pnp::launch_seq_axpy2(n, omega, x, y, r, t, stream));
    if (e != hipSuccess) return hipfail(e, "seq bicgstab");
    rho = rho_new;
    norm = std::sqrt(seq_dot(r, r, rc));
    if (rc) return rc;
    if (norm < reduction * norm_0 || norm < 1e-30) { res.converged = 1; break; }
  }
  if (it > maxit) it = maxit;
  res.it_half = it;
  res.iterations = int(std::ceil(it));
  res.defect = norm;
  res.reduction = norm / norm_0;
  return PNP_OK;
}

// ISTL CGSolver::apply (orc_cg's statements)
int pnp_ctx::seq_cg(int prec, double reduction, int maxit, double *x, double *b,
                    pnp_solve_result &res) {
  const int n = nseq();
  double *r = b, *p = sq(SQ_P), *q = sq(SQ_V);
  int rc = PNP_OK;
  hipError_t e = hipSuccess;
  auto ck = [&](hipError_t ee) {
    if (e == hipSuccess) e = ee;
  };
  ck(hipMemsetAsync(p, 0, sizeof(double) * n, stream));
  ck(hipMemsetAsync(q, 0, sizeof(double) * n, stream));
  std::memset(&res, 0, sizeof res);
  ck(pnp::launch_seq_spmv(n, csr_rowptr.p, csr_col.p, csr_val.p, x, q, stream));
  ck(pnp::launch_seq_aymx(n, 1.0, r, q, stream));
  if (e != hipSuccess) return hipfail(e, "seq cg");
  const double def0 = std::sqrt(seq_dot(r, r, rc));
  if (rc) return rc;
  double def = def0;
  res.defect0 = def0;
  int it = 0;
  if (def0 < 1e-30) {
    res.converged = 1;
  } else {
    if ((rc = seq_prec(prec, r, p))) return rc;
    double rho = seq_dot(p, r, rc);
    if (rc) return rc;
    for (it = 1; it <= maxit; it++) {
      ck(pnp::launch_seq_spmv(n, csr_rowptr.p, csr_col.p, csr_val.p, p, q, stream));
      if (e != hipSuccess) return hipfail(e, "seq cg");
      const double pq = seq_dot(p, q, rc);
      if (rc) return rc;
      const double lambda = rho / pq;
      ck(pnp::launch_seq_axpy(n, lambda, x, p, stream));
      ck(pnp::launch_seq_aymx(n, lambda, r, q, stream));
      if (e != hipSuccess) return hipfail(e, "seq cg");
      def = std::sqrt(seq_dot(r, r, rc));
      if (rc) return rc;
      if (def < reduction * def0 || def < 1e-30) {
        res.converged = 1;
        break;
      }
      ck(hipMemsetAsync(q, 0, sizeof(double) * n, stream));
      if (e != hipSuccess) return hipfail(e, "seq cg");
      if ((rc = seq_prec(prec, r, q))) return rc;
      const double rho_new = seq_dot(q, r, rc);
      if (rc) return rc;
      const double beta = rho_new / rho;
      ck(pnp::launch_seq_cg_p(n, beta, p, q, stream));
      if (e != hipSuccess) return hipfail(e, "seq cg");
      rho = rho_new;
    }
    if (it > maxit) it = maxit;
  }
  res.it_half = it;
  res.iterations = it;
  res.defect = def;
  res.reduction = def0 > 0 ? def / def0 : 0.0;
  return PNP_OK;
}

int pnp_ctx::seq_krylov(const pnp_solve_opts &o, double *x, double *b, pnp_solve_result &res) {
  if (!assembled || !csr_vals_valid) return fail(PNP_E_STATE, "no Jacobian assembled");
  if (o.prec != PNP_PREC_NONE && o.prec != PNP_PREC_JACOBI && o.prec != PNP_PREC_SSOR_NATURAL)
    return fail(PNP_E_ARG, "PNP_OPT_SEQ_ORDER: preconditioner must be NONE, JACOBI or SSOR_NATURAL");
  double t0 = now_s();
  int rc;
  if (o.method == PNP_METHOD_CG)
    rc = seq_cg(o.prec, o.reduction, o.maxit, x, b, res);
  else if (o.method == PNP_METHOD_BICGSTAB)
    rc = seq_bicgstab(o.prec, o.reduction, o.maxit, x, b, res);
  else
    return fail(PNP_E_ARG, "unknown solver method");
  if (!rc && o.prec == PNP_PREC_SSOR_NATURAL) rc = nat_check();
  res.elapsed = now_s() - t0;
  return rc;
}

// the linear solver selected by o.method
int pnp_ctx::krylov(const double *bdev, double *zout, const pnp_solve_opts &o,
                    pnp_solve_result &res) {
  int rc;
  after_solve = true;
  gm_history.clear();
  if (o.method == PNP_METHOD_CG) {
    amg_symmetric = true;
    rc = cg(bdev, zout, o, res);
  } else if (o.method == PNP_METHOD_BICGSTAB) {
    amg_symmetric = false;
    rc = bicgstab(bdev, zout, o, res, 0);
  } else if (o.method == PNP_METHOD_GMRES || o.method == PNP_METHOD_FGMRES) {
    amg_symmetric = false;
    rc = gmres(bdev, zout, o, res, o.method == PNP_METHOD_FGMRES);
  } else if (o.method == PNP_METHOD_IDR) {
    amg_symmetric = false;
    rc = idr(bdev, zout, o, res);
  } else {
    return fail(PNP_E_ARG, "unknown solver method");
  }
  amg_symmetric = true;
  return rc;
}
