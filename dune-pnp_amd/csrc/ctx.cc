// C-ABI implementation (include/pnp_capi.h): context, device buffers, halo exchange over RCCL,
// device-resident BiCGSTAB (ISTL semantics) and PDELab-semantics Newton, host-orchestrated.
#include "ctx.h"

static thread_local std::string g_err;  // errors without a context (create / mesh calls)
std::mutex g_groups_m;
std::map<std::string, std::shared_ptr<LocalGroup>> g_groups;

// bookkeeping after a launch that wrote vals: kc = it relied on the stored constant planes,
// full = it was the P1 analytic assembly writing every plane
void pnp_ctx::asm_wrote(bool kc, bool full) {
  if (kc) {
    asm_reused++;
  } else {
    asm_full++;
    vals_const_valid = full;
  }
}

pnp_ctx::~pnp_ctx() {
  graphs_clear();
  for (auto &v : ev_pending)
    for (auto &pr : v) {
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
  for (auto e : ev_pool) hipEventDestroy(e);
  if (hS) hipHostFree(hS);
  if (h_send) hipHostFree(h_send);
  if (h_recv) hipHostFree(h_recv);
  if (h_red) hipHostFree(h_red);
  if (comm) ncclCommDestroy(comm);
  if (blas) rocblas_destroy_handle(blas);
  if (ev_ready) hipEventDestroy(ev_ready);
  if (ev_halo) hipEventDestroy(ev_halo);
  if (cstream) hipStreamDestroy(cstream);
  if (stream) hipStreamDestroy(stream);
}

// rocprofv3 (ROCm 7.2) --kernel-trace dies with SIGSEGV once it has traced some 12,000-15,000
// graph-launched kernels, whatever the graph (tools/micro/graph_capture_prof.hip):
// under the profiler (its launcher exports ROCPROF_* variables) graph replay stays off unless
// PNP_OPT_GRAPH forces it; the eager launches give the same results bit for bit
bool pnp_ctx::profiled() {
  static const bool p = [] {
    extern char **environ;
    for (char **e = environ; e && *e; e++)
      if (std::strncmp(*e, "ROCPROF_", 8) == 0) return true;
    return false;
  }();
  return p;
}

void pnp_ctx::graphs_clear() {
  nat_graph_clear();
  for (auto &g : graph_cache)
    if (g.exec) hipGraphExecDestroy(g.exec);
  graph_cache.clear();
  graph_epoch++;
  graphs_failed = false;
}

// ---- timers -------------------------------------------------------------------------------
hipEvent_t pnp_ctx::ev_get() {
  if (!ev_pool.empty()) {
    hipEvent_t e = ev_pool.back();
    ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

void pnp_ctx::timers_flush() {
  hipStreamSynchronize(stream);
  for (int c = 0; c < T_NCAT; c++) {
    for (auto &pr : ev_pending[c]) {
      float ms = 0;
      hipEventElapsedTime(&ms, pr.first, pr.second);
      t_ms[c] += ms;
      ev_pool.push_back(pr.first);
      ev_pool.push_back(pr.second);
    }
    ev_pending[c].clear();
  }
}

int pnp_ctx::halo_on(double *vec, int nfv, hipStream_t hs) {
  if (nranks == 1) return PNP_OK;
  if (lg) return halo_local(vec, nfv);
  if (host_tr()) return halo_host(vec, nfv);
  if (L.nbr_ranks.empty()) return PNP_OK;
  hipEvent_t t0 = hs == stream ? tb(T_HALO) : nullptr;
  int ns = int(L.send_idx.size());
  hipError_t e = pnp::launch_pack(ns, nfv, d_send_idx.p, vec, sendbuf.p, hs);
  if (e != hipSuccess) return hipfail(e, "halo pack");
  if (ncclGroupStart() != ncclSuccess) return fail(PNP_E_RCCL, "ncclGroupStart");
  for (size_t q = 0; q < L.nbr_ranks.size(); q++) {
    int peer = L.nbr_ranks[q];
    size_t sc = size_t(L.send_ptr[q + 1] - L.send_ptr[q]) * nfv;
    size_t rc = size_t(L.recv_ptr[q + 1] - L.recv_ptr[q]) * nfv;
    if (ncclSend(sendbuf.p + size_t(L.send_ptr[q]) * nfv, sc, ncclDouble, peer, comm, hs) !=
        ncclSuccess)
      return fail(PNP_E_RCCL, "ncclSend");
    if (ncclRecv(vec + (size_t(L.n_owned) + L.recv_ptr[q]) * nfv, rc, ncclDouble, peer, comm,
                 hs) != ncclSuccess)
      return fail(PNP_E_RCCL, "ncclRecv");
  }
  if (ncclGroupEnd() != ncclSuccess) return fail(PNP_E_RCCL, "ncclGroupEnd");
  if (t0) te(T_HALO, t0);
  return PNP_OK;
}

// halo exchange of vin's ghosts + y = A vin (mode / dots as launch_spmv).  Multi-GPU with the
// split layout: the interior blocks (no ghost columns) run while the halo is in flight on
// cstream, then the boundary blocks; their partials follow each other, *nsp counts both.
int pnp_ctx::halo_spmv(double *vin, double *yout, int mode, const double *w, const double *w2,
                       int *nsp) {
  hipError_t e;
  if (mf_lin) mf_applies++;  // an interior + boundary pair counts once
  // the P_k element pass reads vin's ghosts in every element: halo, then both passes, unsplit
  if (!split_spmv || (mf_lin && degree > 1)) {
    int rc = halo(vin, nf);
    if (rc) return rc;
    // the launch records the timer events itself (the kernel's own duration)
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (timing && L.n_owned > 0) {
      t0 = ev_get();
      t1 = ev_get();
    }
    e = apply_op(dl, vin, yout, mode, w, partials.p, nsp, stream, w2, t0, t1);
    if (e != hipSuccess) return hipfail(e, "spmv");
    if (t1) {
      ev_pending[T_SPMV].push_back({t0, t1});
      t_n[T_SPMV]++;
    }
    return PNP_OK;
  }
  const int kd = mode == 4 ? 3 : (mode == 2 ? 2 : 1);
  const pnp::DevLayout dl_int = sub_layout(true), dl_bnd = sub_layout(false);
  int n1 = 0, n2 = 0, rc;
  if (lg || host_tr()) {  // in-process / host-staged transport: synchronous halo between the halves
    hipEvent_t t0 = tb(T_SPMV);
    e = apply_op(dl_int, vin, yout, mode, w, partials.p, &n1, stream, w2);
    if (e != hipSuccess) return hipfail(e, "spmv interior");
    te(T_SPMV, t0);
    if ((rc = halo(vin, nf))) return rc;
  } else {
    if ((e = hipEventRecord(ev_ready, stream)) != hipSuccess ||
        (e = hipStreamWaitEvent(cstream, ev_ready, 0)) != hipSuccess)
      return hipfail(e, "halo stream order");
    if ((rc = halo_on(vin, nf, cstream))) return rc;
    if ((e = hipEventRecord(ev_halo, cstream)) != hipSuccess) return hipfail(e, "halo event");
    hipEvent_t t0 = tb(T_SPMV);
    e = apply_op(dl_int, vin, yout, mode, w, partials.p, &n1, stream, w2);
    if (e != hipSuccess) return hipfail(e, "spmv interior");
    te(T_SPMV, t0);
    if ((e = hipStreamWaitEvent(stream, ev_halo, 0)) != hipSuccess)
      return hipfail(e, "halo wait");
  }
  hipEvent_t t1 = tb(T_SPMV);
  e = apply_op(dl_bnd, vin, yout, mode, w, partials.p + size_t(n1) * kd, &n2, stream, w2);
  if (e != hipSuccess) return hipfail(e, "spmv boundary");
  te(T_SPMV, t1);
  *nsp = n1 + n2;
  return PNP_OK;
}

// host-staged halo: pack on the device, copy to pinned host memory, the caller's exchange, copy
// the received ghosts back (synchronous, on the context's stream)
int pnp_ctx::halo_host(double *vec, int nfv) {
  hipEvent_t t0 = tb(T_HALO);
  const int ns = int(L.send_idx.size()), nq = int(L.nbr_ranks.size());
  const size_t nsend = size_t(ns) * nfv, nrecv = size_t(L.n_ghost) * nfv;
  hipError_t e = pnp::launch_pack(ns, nfv, d_send_idx.p, vec, sendbuf.p, stream);
  if (e == hipSuccess && nsend)
    e = hipMemcpyAsync(h_send, sendbuf.p, sizeof(double) * nsend, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "halo pack");
  std::vector<int64_t> soff(nq), scnt(nq), roff(nq), rcnt(nq);
  for (int q = 0; q < nq; q++) {
    soff[q] = int64_t(L.send_ptr[q]) * nfv;
    scnt[q] = int64_t(L.send_ptr[q + 1] - L.send_ptr[q]) * nfv;
    roff[q] = int64_t(L.recv_ptr[q]) * nfv;
    rcnt[q] = int64_t(L.recv_ptr[q + 1] - L.recv_ptr[q]) * nfv;
  }
  if (ht.exchange(ht.user, nq, L.nbr_ranks.data(), h_send, soff.data(), scnt.data(), h_recv,
                  roff.data(), rcnt.data()) != 0)
    return fail(PNP_E_RCCL, "host transport: exchange failed");
  if (nrecv)
    e = hipMemcpyAsync(vec + size_t(L.n_owned) * nfv, h_recv, sizeof(double) * nrecv,
                       hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);  // h_recv is reused by the next call
  if (e != hipSuccess) return hipfail(e, "halo copy");
  if (t0) te(T_HALO, t0);
  return PNP_OK;
}

int pnp_ctx::halo_local(double *vec, int nfv) {
  int ns = int(L.send_idx.size());
  hipError_t e = pnp::launch_pack(ns, nfv, d_send_idx.p, vec, sendbuf.p, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "halo pack");
  lg->barrier();  // every rank has packed
  for (size_t q = 0; q < L.nbr_ranks.size(); q++) {
    pnp_ctx *peer = lg->members[L.nbr_ranks[q]];
    const pnp::LocalLayout &PL = peer->L;
    size_t k = 0;
    while (k < PL.nbr_ranks.size() && PL.nbr_ranks[k] != rank) k++;
    if (k == PL.nbr_ranks.size()) return fail(PNP_E_STATE, "asymmetric halo");
    size_t cnt = size_t(L.recv_ptr[q + 1] - L.recv_ptr[q]) * nfv;
    if (cnt != size_t(PL.send_ptr[k + 1] - PL.send_ptr[k]) * nfv)
      return fail(PNP_E_STATE, "halo size mismatch");
    e = hipMemcpyAsync(vec + (size_t(L.n_owned) + L.recv_ptr[q]) * nfv,
                       peer->sendbuf.p + size_t(PL.send_ptr[k]) * nfv, sizeof(double) * cnt,
                       hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return hipfail(e, "halo copy");
  }
  e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "halo copy");
  lg->barrier();  // nobody repacks before every copy out of the send buffers is done
  return PNP_OK;
}

// in-place sum over ranks of k doubles in device memory
int pnp_ctx::allreduce_dev(double *d, int k) {
  if (!dist) return PNP_OK;
  if (lg) {
    std::vector<double> h(k);
    hipError_t e = hipMemcpyAsync(h.data(), d, sizeof(double) * k, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hipfail(e, "allreduce");
    lg->host[rank] = h;
    lg->barrier();
    std::vector<double> sum(k, 0.0);
    for (int r = 0; r < nranks; r++)  // fixed rank order: deterministic
      for (int j = 0; j < k; j++) sum[j] += lg->host[r][j];
    lg->barrier();
    e = hipMemcpyAsync(d, sum.data(), sizeof(double) * k, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? PNP_OK : hipfail(e, "allreduce");
  }
  if (host_tr()) {
    if (size_t(k) > h_red_n) {
      if (h_red) hipHostFree(h_red);
      h_red = nullptr;
      h_red_n = 0;
      hipError_t e = hipHostMalloc(&h_red, sizeof(double) * size_t(k));
      if (e != hipSuccess) return hipfail(e, "allreduce staging");
      h_red_n = size_t(k);
    }
    hipError_t e = hipMemcpyAsync(h_red, d, sizeof(double) * k, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hipfail(e, "allreduce");
    if (ht.allreduce_sum(ht.user, h_red, k) != 0)
      return fail(PNP_E_RCCL, "host transport: allreduce failed");
    e = hipMemcpyAsync(d, h_red, sizeof(double) * k, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? PNP_OK : hipfail(e, "allreduce");
  }
  ncclResult_t nr = ncclAllReduce(d, d, k, ncclDouble, ncclSum, comm, stream);
  if (nr != ncclSuccess)
    return fail(PNP_E_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(nr));
  return PNP_OK;
}

int pnp_ctx::allreduce_red(int k) {
  if (!dist) return PNP_OK;
  hipEvent_t t0 = tb(T_ALLRED);
  double *red = reinterpret_cast<double *>(reinterpret_cast<char *>(S.p) +
                                           offsetof(pnp::Scalars, red));
  int rc = allreduce_dev(red, k);
  if (rc) return rc;
  te(T_ALLRED, t0);
  return PNP_OK;
}

// S->red = sum of partials (all ranks), then the derive step of BiCGSTAB stage `stage`
int pnp_ctx::reduce_derive(int np, int k, int stage, bool from2) {
  hipError_t e;
  const double *src = from2 ? partials2.p : partials.p;
  if (!dist) {
    e = pnp::launch_reduce(src, np, k, S.p, stream, stage, redmw.p);
    return e == hipSuccess ? PNP_OK : hipfail(e, "reduce");
  }
  e = pnp::launch_reduce(src, np, k, S.p, stream, -1, redmw.p);
  if (e != hipSuccess) return hipfail(e, "reduce");
  int rc = allreduce_red(k);
  if (rc) return rc;
  e = pnp::launch_derive(S.p, stage, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, "derive");
}

// S->red[0..ka) = sum of partials (spmv), S->red[ka..) = sum of partials2, all ranks; derive
int pnp_ctx::reduce_derive2(int npa, int ka, int npb, int kb, int stage) {
  hipError_t e;
  if (!dist) {
    e = pnp::launch_reduce2(partials.p, npa, ka, partials2.p, npb, kb, S.p, stream, stage,
                            redmw.p);
    return e == hipSuccess ? PNP_OK : hipfail(e, "reduce");
  }
  e = pnp::launch_reduce2(partials.p, npa, ka, partials2.p, npb, kb, S.p, stream, -1, redmw.p);
  if (e != hipSuccess) return hipfail(e, "reduce");
  int rc = allreduce_red(ka + kb);
  if (rc) return rc;
  e = pnp::launch_derive(S.p, stage, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, "derive");
}

// norm over owned rows of a vector, synchronous
int pnp_ctx::norm(const double *vec, double &out) {
  hipEvent_t t0 = tb(T_BLAS);
  hipError_t e = pnp::launch_dot(nown(), vec, vec, 0, partials.p, stream);
  if (e == hipSuccess) {
    // reduce through the scalar block without touching the BiCGSTAB state: use a scratch
    // Scalars at S.p + 1
    e = pnp::launch_reduce(partials.p, pnp::blas_nparts(nown()), 1, S.p + 1, stream);
  }
  if (e != hipSuccess) return hipfail(e, "norm");
  te(T_BLAS, t0);
  if (dist) {
    double *red = reinterpret_cast<double *>(reinterpret_cast<char *>(S.p + 1) +
                                             offsetof(pnp::Scalars, red));
    int rc = allreduce_dev(red, 1);
    if (rc) return rc;
  }
  if (int rc = poll(hS + 1, S.p + 1, sizeof(pnp::Scalars), "norm readback")) return rc;
  out = std::sqrt(hS[1].red[0]);
  return PNP_OK;
}

// external (lexicographic, global) vector -> the internal layout; devptr: `host` is a device
// pointer (PNP_DEVICE_PTRS), gathered from directly
int pnp_ctx::upload_ext(const double *host, int nfv, double *dev, bool with_ghosts, bool devptr) {
  size_t ne = size_t(mesh.nv) * nfv;
  hipError_t e = hipSuccess;
  if (!devptr)
    e = hipMemcpyAsync(ext.p, host, sizeof(double) * ne, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = pnp::launch_gather_ext(with_ghosts ? L.n_owned + L.n_ghost : L.n_owned, nfv, mesh.nv,
                               d_l2g.p, devptr ? host : ext.p, dev, stream);
  if (e != hipSuccess) return hipfail(e, "upload");
  return PNP_OK;
}

// internal -> external; this rank's owned entries are written (devptr: into device memory,
// synchronised before return)
int pnp_ctx::download_ext(const double *dev, int nfv, double *host, bool devptr) {
  if (devptr) {
    hipError_t e = pnp::launch_scatter_ext(L.n_owned, nfv, mesh.nv, d_l2g.p, dev, host, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? PNP_OK : hipfail(e, "download");
  }
  size_t ne = size_t(mesh.nv) * nfv;
  hipError_t e = pnp::launch_scatter_ext(L.n_owned, nfv, mesh.nv, d_l2g.p, dev, ext.p, stream);
  std::vector<double> tmp(ne);
  if (e == hipSuccess)
    e = hipMemcpyAsync(tmp.data(), ext.p, sizeof(double) * ne, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "download");
  for (int i = 0; i < L.n_owned; i++) {
    int g = L.l2g[i];
    for (int f = 0; f < nfv; f++) host[size_t(f) * mesh.nv + g] = tmp[size_t(f) * mesh.nv + g];
  }
  return PNP_OK;
}

int pnp_ctx::assemble(const double *xdev, int jac) {
  if (kind < 0) return fail(PNP_E_STATE, "no operator set (pnp_set_operator)");
  int rc;
  if (jac && (rc = set_fd(fd_opt != 0))) return rc;
  // matrix-free (analytic; P1: PNP_OPT_MATRIX_FREE, P_k: pnp_pk_matfree_set): the Jacobian is the
  // recorded point; only the residual the fused assembly would also have produced is computed now
  // (Newton's right-hand side)
  const bool mf = jac && mf_on() && !fd_mode;
  if (mf && (rc = mf_record(xdev))) return rc;
  aa.x = xdev;
  aa.jac = (fd_mode || mf) ? 0 : jac;
  aa.r = r.p;
  aa.cold = after_solve ? 1 : 0;
  aa.kconst = (aa.jac && asm_kconst()) ? 1 : 0;
  // the P1 analytic assembly is one launch: it records its own start / end events (the
  // kernel's duration, as the kernel trace reports it); the other forms take an event pair
  const bool one = degree == 1 && !(jac && fd_mode);
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (timing && one) {
    t0 = ev_get();
    t1 = ev_get();
  } else {
    t0 = tb(T_ASM);
  }
  hipError_t e;
  int piped = 0;
  if (degree > 1)
    e = pnp::launch_pk_assemble(dl, aa, pkd, jac ? (fd_mode ? 2 : 1) : 0, stream);
  else
    e = pnp::launch_assemble(dl, aa, stream, t1 ? t0 : nullptr, t1, &piped);
  if (e == hipSuccess && jac && fd_mode && degree == 1)
    e = pnp::launch_fd_jacobian(dl, aa, nf, pat, fd_ne, fd_etri.p, fd_rptr.p, fd_cdata.p,
                                fd_jel.p, stream);
  if (e != hipSuccess) {
    if (jac && !mf) vals_const_valid = false;
    return hipfail(e, "assemble");
  }
  if (jac && !mf) asm_wrote(aa.kconst != 0, degree == 1 && !fd_mode);
  asm_piped += piped;
  if (t1) {
    ev_pending[T_ASM].push_back({t0, t1});
    t_n[T_ASM]++;
  } else {
    te(T_ASM, t0);
  }
  if (jac) {
    jacobian_stored(mf);
    after_solve = false;
    if (!mf) value_assemblies++;
  }
  return PNP_OK;
}

// the linearisation point of a matrix-free Jacobian: the state with its ghosts in a buffer of
// its own (a later residual overwrites x) and the operator's arguments as they are now
int pnp_ctx::mf_record(const double *xdev) {
  const size_t nl = size_t(dl.n_local) * 3;
  hipError_t e = hipSuccess;
  if (mf_x.n < nl) e = mf_x.alloc(std::max<size_t>(1, nl));
  if (e == hipSuccess)
    e = hipMemcpyAsync(mf_x.p, xdev, sizeof(double) * size_t(dl.n_local) * nf,
                       hipMemcpyDeviceToDevice, stream);
  if (e != hipSuccess) return hipfail(e, "linearisation point");
  mf_aa = aa;
  mf_aa.x = mf_x.p;
  mf_aa.jac = 1;
  mf_aa.r = nullptr;
  mf_aa.cold = 0;
  return PNP_OK;
}

// the SELL values of a Jacobian held as a linearisation point, for whoever reads vals: the
// ordinary fused assembly at the point, once (its residual goes to a scratch vector)
int pnp_ctx::ensure_values() {
  if (!mf_lin || !vals_stale) return PNP_OK;
  const size_t no = size_t(L.n_owned) * 3;
  hipError_t e = hipSuccess;
  if (mf_r.n < no) e = mf_r.alloc(std::max<size_t>(1, no));
  if (e != hipSuccess) return hipfail(e, "assemble at the linearisation point");
  pnp::AsmArgs fa = mf_aa;
  fa.r = mf_r.p;
  fa.vals = vals.p;
  fa.cold = after_solve ? 1 : 0;
  fa.kconst = asm_kconst() ? 1 : 0;
  hipEvent_t t0 = tb(T_ASM);
  int piped = 0;
  if (degree > 1)
    e = pnp::launch_pk_assemble(dl, fa, pkd, 1, stream);
  else
    e = pnp::launch_assemble(dl, fa, stream, nullptr, nullptr, &piped);
  if (e != hipSuccess) {
    vals_const_valid = false;
    return hipfail(e, "assemble at the linearisation point");
  }
  asm_wrote(fa.kconst != 0, degree == 1);
  asm_piped += piped;
  te(T_ASM, t0);
  vals_stale = false;
  value_assemblies++;
  return PNP_OK;
}

// Jacobi on a matrix-free Jacobian whose values were never needed: its diagonal blocks alone
int pnp_ctx::jacobi_prepare() {
  if (!mf_lin || !vals_stale || mf_diag_valid) return PNP_OK;
  hipError_t e = hipSuccess;
  if (!mf_choff.p) {
    std::vector<int> co(size_t(L.nchunks) + 1);
    for (size_t c = 0; c < co.size(); c++) co[c] = int(c) * pnp::kRows;
    int rc = upv(mf_choff, co, "diagonal layout");
    if (rc) return rc;
    e = mf_diag.alloc(std::max<size_t>(1, size_t(L.nchunks) * pnp::kRows * 6));
  }
  if (e == hipSuccess)
    e = degree > 1 ? pnp::launch_pk_jac_diag(dl, mf_aa, pkd, mf_diag.p, stream)
                   : pnp::launch_jac_diag(dl, mf_aa, mf_diag.p, stream);
  if (e != hipSuccess) return hipfail(e, "jacobi diagonal");
  mf_diag_valid = true;
  return PNP_OK;
}

// structure of the external-layout CSR view of the current block pattern (host, once per
// pattern): rows f*nv + g of the owned vertices, columns sorted; per entry the source block
// (row << 6 | slot) and the value's index in the block pattern.  Also the natural-order SSOR
// level schedule over these rows.
int pnp_ctx::csr_structure() {
  const int nv = mesh.nv, mask = pat & 0x1FF;
  if (csr_pat == mask && csr_nf == nf) return PNP_OK;
  // the BiCGSTAB block graphs captured with SSOR_NATURAL hold csr_val, nat_d / nat_v and the level
  // buffers, all rebuilt below: drop every graph (bumps graph_epoch, part of GraphKey)
  graphs_clear();
  const int n = nf * nv;
  std::vector<int> cnt(n + 1, 0);
  for (int i = 0; i < L.n_owned; i++) {
    const int len = pnp::meta_len(L.rowmeta[i]);
    for (int f = 0; f < nf; f++) {
      int k = 0;
      for (int g = 0; g < nf; g++) k += pnp::pat_index(mask, f, g) >= 0;
      cnt[f * nv + L.l2g[i] + 1] += k * len;
    }
  }
  for (int i = 0; i < n; i++) cnt[i + 1] += cnt[i];
  const long long nnz = cnt[n];
  std::vector<int> col(nnz), src(nnz);
  std::vector<unsigned char> vid(nnz);
  struct E {
    int col, src;
    unsigned char v;
  };
  std::vector<E> tmp;
  for (int i = 0; i < L.n_owned; i++) {
    const int chunk = i / pnp::kRows, lane = i % pnp::kRows, len = pnp::meta_len(L.rowmeta[i]);
    for (int f = 0; f < nf; f++) {
      tmp.clear();
      for (int sl = 0; sl < len; sl++) {
        const int j = L.colidx[size_t(L.chunk_off[chunk]) + size_t(sl) * pnp::kRows + lane];
        for (int g = 0; g < nf; g++) {
          const int v = pnp::pat_index(mask, f, g);
          if (v >= 0) tmp.push_back({g * nv + L.l2g[j], i << 6 | sl, (unsigned char)v});
        }
      }
      std::sort(tmp.begin(), tmp.end(), [](const E &a, const E &b) { return a.col < b.col; });
      long long q = cnt[f * nv + L.l2g[i]];
      for (const E &e : tmp) {
        col[q] = e.col;
        src[q] = e.src;
        vid[q] = e.v;
        q++;
      }
    }
  }
  int rc;
  if ((rc = upv(csr_rowptr, cnt, "csr rowptr")) || (rc = upv(csr_col, col, "csr col")) ||
      (rc = upv(csr_src, src, "csr src")) || (rc = upv(csr_vidx, vid, "csr vidx")))
    return rc;
  hipError_t e = csr_val.alloc(std::max<long long>(1, nnz));
  if (e != hipSuccess) return hipfail(e, "csr values");
  // natural-order SSOR schedule.  A row R must run after every row it shares a matrix entry with
  // (A_RC or A_CR stored) that comes before it in the sweep, and before every such later row:
  // level(R) = 1 + max level of its earlier partners, computed in sweep order with the partners
  // of the transposed entries pushed forward.  Rows of other ranks' vertices are empty and stay
  // out (their columns read zero).
  auto empty = [&](int R) { return cnt[R] == cnt[R + 1]; };
  std::vector<int> diag(n, -1);
  for (int R = 0; R < n; R++)
    for (int k = cnt[R]; k < cnt[R + 1]; k++)
      if (col[k] == R) diag[R] = k;
  for (int R = 0; R < n; R++)
    if (!empty(R) && diag[R] < 0) return fail(PNP_E_STATE, "natural SSOR: row without diagonal");
  if ((rc = upv(csr_diag, diag, "csr diagonal"))) return rc;
  // the dataflow sweeps keep their results and operands in the external (lexicographic) layout
  // R = f * nv + g, which is local in the sweep order (indexing them by internal position
  // instead made the PNP heads 10-16 % slower, profiles/r05/nat_split_r5e.txt), but read d at
  // the row's INTERNAL position g2l[g] * nf + f (info.w / rec.w), so that the preconditioner's
  // input needs no scatter into an external copy (PNP config 3: 20 us per application,
  // profiles/r05/nat_split_r5d.txt); the result is gathered out of vb afterwards
  auto P = [&](int R) { return L.g2l[R % nv] * nf + R / nv; };
  // NatSweep::info packs a row's entry count and its diagonal's offset into one int as
  // len | offset << 8 (the kernels decode len & 255): at most 255 entries per row (P1 PNP rows
  // have <= 3 * 21); a wider pattern would corrupt both, so refuse it here
  for (int R = 0; R < n; R++)
    if (cnt[R + 1] - cnt[R] > 255)
      return fail(PNP_E_STATE, "natural SSOR: a row has more than 255 CSR entries (row " +
                                   std::to_string(R) + ")");
  auto schedule = [&](bool fwd, NatDir &W) -> int {
    std::vector<int> &lptr = W.lptr;
    std::vector<int> lev(n, -1), push(n, 0);
    int nlev = 0;
    for (int s = 0; s < n; s++) {
      const int R = fwd ? s : n - 1 - s;
      if (empty(R)) continue;
      int l = push[R];
      for (int k = cnt[R]; k < cnt[R + 1]; k++) {
        const int C = col[k];
        if (C != R && (fwd ? C < R : C > R) && !empty(C)) l = std::max(l, lev[C] + 1);
      }
      lev[R] = l;
      nlev = std::max(nlev, l + 1);
      for (int k = cnt[R]; k < cnt[R + 1]; k++) {
        const int C = col[k];
        if (C != R && (fwd ? C > R : C < R) && !empty(C)) push[C] = std::max(push[C], l + 1);
      }
    }
    lptr.assign(nlev + 1, 0);
    for (int R = 0; R < n; R++)
      if (lev[R] >= 0) lptr[lev[R] + 1]++;
    for (int l = 0; l < nlev; l++) lptr[l + 1] += lptr[l];
    std::vector<int> fill(lptr.begin(), lptr.end() - 1), rl(std::max(1, lptr[nlev]));
    for (int R = 0; R < n; R++)
      if (lev[R] >= 0) rl[fill[lev[R]]++] = R;
    // per level an ELL of its rows' entries (CSR order), width = its longest row, padding
    // slots with value index -1, stored unit by unit: the level's rows in groups of UR (the
    // dataflow units), each group's entries k-major, entry k of the group's row r at
    // (group * width + k) * UR + r.  A unit's slots are then one contiguous run of lines that no
    // other unit touches (column-major over the whole level, 4 units shared every line of a
    // slot, fetched once per XCD that ran one of them: the PNP head missed L2 ~16.7 M times per
    // launch, profiles/r05/nat_pmc_mem_r5a.json)
    const int UR = pnp::ssor_natural_unit_rows();
    std::vector<int4> info(std::max(1, lptr[nlev]));
    std::vector<int> lwidth(nlev, 0);
    W.eoff.assign(nlev + 1, 0);
    for (int l = 0; l < nlev; l++) {
      int w = 0;
      for (int t = lptr[l]; t < lptr[l + 1]; t++) w = std::max(w, cnt[rl[t] + 1] - cnt[rl[t]]);
      lwidth[l] = w;
      W.eoff[l + 1] = W.eoff[l] + (long long)w * UR * ((lptr[l + 1] - lptr[l] + UR - 1) / UR);
    }
    // operand codes (NatSweep): the forward sweep reads the new value of an earlier row (C < R)
    // and zero for the row itself and later rows; the backward sweep reads the forward value of
    // rows C <= R and the new backward value of later rows; rows of other ranks read zero
    std::vector<int> ecol(std::max<long long>(1, W.eoff[nlev]), -1);
    for (int l = 0; l < nlev; l++) {
      for (int t = lptr[l]; t < lptr[l + 1]; t++) {
        const int R = rl[t], len = cnt[R + 1] - cnt[R], tl = t - lptr[l];
        info[t] = make_int4(R, len | (diag[R] - cnt[R]) << 8, cnt[R], P(R));
        for (int k = 0; k < len; k++) {
          const size_t q =
              size_t(W.eoff[l]) + (size_t(tl / UR) * lwidth[l] + k) * UR + size_t(tl % UR);
          const int C = col[cnt[R] + k];
          ecol[q] = empty(C) ? -1 : fwd ? (C < R ? C : -1) : (C <= R ? C : -(C + 2));
        }
      }
    }
    // dataflow units for the one-launch sweep: up to ssor_natural_unit_rows() consecutive rows of one level,
    // {first sweep position, rows | width << 8, the ELL stride between a row's entries (UR), ELL
    // index of the unit's first row}; forward units in level order, then backward units in level
    // order.  The
    // sweep's tail -- the levels from the last one wider than PNP_NAT_TAIL rows to its end --
    // can run in one workgroup (ssor_natural.hip); default 0 (no tail): one CU is slower
    // (PNP config 3: 2.36 ms per application without, 3.29 / 4.83 ms with 512 / 1024-row tails,
    // profiles/r04/ssor_natural_tail_r4e.log)
    static const int tail_rows = [] {
      const char *ev = std::getenv("PNP_NAT_TAIL");
      return ev ? std::max(0, std::atoi(ev)) : 0;
    }();
    // PNP_NAT_CHAIN (rows): the tail as chains (k_ssor_nat_chain; takes precedence over
    // PNP_NAT_TAIL).  Default: the levels of at most as many rows as the chain kernel keeps
    // groups resident (8,192 on MI355X), so that no two chains share a group at one level
    // (pore_pnp k=4 per application, PB 1.31 -> 0.57 ms, PNP config 3 2.22 -> 1.57 ms;
    // threshold sweep profiles/r04/chain2/).  PNP_NAT_CHAIN=0: dataflow units only
    static const int chain_rows = [] {
      const char *ev = std::getenv("PNP_NAT_CHAIN");
      return ev ? std::max(0, std::atoi(ev)) : std::max(0, pnp::ssor_natural_chain_capacity());
    }();
    const int trows = chain_rows > 0 ? chain_rows : tail_rows;
    int ltail = nlev;
    while (trows > 0 && ltail > 0 && lptr[ltail] - lptr[ltail - 1] <= trows) ltail--;
    W.chain_ok = false;
    if (chain_rows > 0 && ltail < nlev) {
      // heavy-path chains of the tail: parent = the first dependency on the level just before
      // (inside the tail); each row continues the chain of its child with the longest path
      // below it; chains packed into lane groups by level interval (greedy, by start level)
      const int t0 = lptr[ltail], t1 = lptr[nlev];
      auto isdep = [&](int R, int C) {
        return C != R && !empty(C) && (fwd ? C < R : C > R);
      };
      std::vector<int> parent(n, -1), heavy(n, -1), hbest(n, 0);
      int wmax = 0;
      for (int t = t0; t < t1; t++) {
        const int R = rl[t];
        wmax = std::max(wmax, cnt[R + 1] - cnt[R]);
        for (int k = cnt[R]; k < cnt[R + 1]; k++) {
          const int C = col[k];
          if (isdep(R, C) && lev[C] == lev[R] - 1 && lev[C] >= ltail) {
            parent[R] = C;
            break;
          }
        }
      }
      for (int t = t1 - 1; t >= t0; t--) {  // decreasing level
        const int R = rl[t], P = parent[R], h = 1 + hbest[R];
        if (P >= 0 && h > hbest[P]) {
          hbest[P] = h;
          heavy[P] = R;
        }
      }
      // at most the grid's resident lane groups (the kernel's progress needs them all
      // resident): past that, a chain shares the group that frees first, its rows interleaved
      // by level (a row whose parent is not the group's previous row reads it from memory)
      const int gcap = std::max(1, pnp::ssor_natural_chain_capacity());
      std::vector<std::vector<int>> grows;
      std::priority_queue<std::pair<int, int>, std::vector<std::pair<int, int>>,
                          std::greater<std::pair<int, int>>> freeq;  // (end level, group)
      bool shared = false;
      long long rr = 0;  // over the cap: chains dealt round-robin (a balanced share per group)
      std::vector<int> gend;  // each group's last level; heap entries that disagree are stale
      for (int t = t0; t < t1; t++) {
        const int R = rl[t];
        if (parent[R] >= 0 && heavy[parent[R]] == R) continue;  // inside a chain
        while (!freeq.empty() && freeq.top().first != gend[freeq.top().second]) freeq.pop();
        int g;
        if (!freeq.empty() && freeq.top().first < lev[R]) {
          g = freeq.top().second;
          freeq.pop();
        } else if (int(grows.size()) >= gcap) {
          g = int(rr++ % gcap);
          shared = true;
        } else {
          g = int(grows.size());
          grows.emplace_back();
          gend.push_back(-1);
        }
        int X = R, last = lev[R];
        for (; X >= 0; X = heavy[X]) {
          grows[g].push_back(X);
          last = lev[X];
        }
        gend[g] = std::max(gend[g], last);
        freeq.push({gend[g], g});
      }
      if (shared)  // every group's rows in level order (stable: a chain's rows stay in order)
        for (auto &G : grows)
          std::stable_sort(G.begin(), G.end(), [&](int a, int b) { return lev[a] < lev[b]; });
      const int wpad = wmax;
      if (wpad <= pnp::ssor_natural_chain_width()) {
        std::vector<int> gptr(1, 0), ecode;
        std::vector<int4> rec;
        for (const auto &G : grows) {
          const int H = pnp::ssor_natural_chain_history();
          for (size_t t = 0; t < G.size(); t++) {
            const int R = G[t];
            const int len = cnt[R + 1] - cnt[R];
            rec.push_back(make_int4(R, len | (diag[R] - cnt[R]) << 8, cnt[R], P(R)));
            for (int k = 0; k < wpad; k++) {
              if (k < len) {
                const int C = col[cnt[R] + k];
                const int fc = empty(C) ? -1 : fwd ? (C < R ? C : -1) : (C <= R ? C : -(C + 2));
                // kind: 0 zero, 1 forward value, 2 backward value, 3 in the wave's registers
                int code = fc == -1 ? 0 : fc >= 0 ? (fc << 2 | 1) : ((-(fc + 2)) << 2 | 2);
                const bool fresh = fwd ? (code & 3) == 1 : (code & 3) == 2;  // this sweep's value
                for (int h = 1; fresh && h <= H && size_t(h) <= t; h++)
                  if (G[t - h] == C) {
                    code = h << 2 | 3;
                    break;
                  }
                ecode.push_back(code);
              } else {
                ecode.push_back(0);
              }
            }
          }
          gptr.push_back(int(rec.size()));
        }
        int rc2;
        if ((rc2 = upv(W.cgptr, gptr, "natural SSOR chains")) ||
            (rc2 = upv(W.crec, rec, "natural SSOR chains")) ||
            (rc2 = upv(W.cecode, ecode, "natural SSOR chains")))
          return rc2;
        W.chain_groups = int(grows.size());
        W.chain_wpad = wpad;
        W.chain_ok = true;
      }
    }
    if (chain_rows > 0 && !W.chain_ok) {
      // no chains (rows wider than the chain kernel takes): the tail is PNP_NAT_TAIL's again
      // (default none), not the chain threshold's -- a one-workgroup tail of ~8K rows would run
      // every narrow level on one CU
      ltail = nlev;
      while (tail_rows > 0 && ltail > 0 && lptr[ltail] - lptr[ltail - 1] <= tail_rows) ltail--;
    }
    for (int l = 0; l < nlev && nat_units_ok; l++) {
      if (l == ltail) (fwd ? nat_tail_f : nat_tail_b) = int(nat_units.size());
      const long long w = lwidth[l];
      for (int t0 = lptr[l]; t0 < lptr[l + 1]; t0 += UR) {
        const long long e0 = W.eoff[l] + (t0 - lptr[l]) / UR * w * UR;
        if (w > 255 || W.eoff[l + 1] > INT32_MAX) {
          nat_units_ok = false;
          break;
        }
        const int rows = std::min(UR, lptr[l + 1] - t0);
        nat_units.push_back(make_int4(t0, rows | int(w) << 8 | (fwd ? 0 : 1 << 16), UR, int(e0)));
        nat_max_width = std::max(nat_max_width, int(w));
      }
    }
    if (ltail >= nlev) (fwd ? nat_tail_f : nat_tail_b) = int(nat_units.size());
    if (fwd) nat_units_f = int(nat_units.size());
    int rc2;
    if ((rc2 = upv(W.info, info, "natural SSOR rows"))) return rc2;
    return upv(W.ecol, ecol, "natural SSOR columns");
  };
  nat_units.clear();
  nat_units_ok = true;
  nat_resident = -1;
  nat_max_width = 0;
  if ((rc = schedule(true, nat_f)) || (rc = schedule(false, nat_b))) return rc;
  if (nat_units_ok && (rc = upv(d_nat_units, nat_units, "natural SSOR units"))) return rc;
  const int ni = std::max(1, nf * (L.n_owned + L.n_ghost));  // internal layout
  if ((e = nat_d.alloc(std::max(1, n))) != hipSuccess || (e = nat_v.alloc(std::max(1, n))) != hipSuccess ||
      (e = nat_vf.alloc(std::max(1, n))) != hipSuccess || (e = nat_di.alloc(ni)) != hipSuccess ||
      (e = nat_vi.alloc(ni)) != hipSuccess || (e = nat_abort.alloc(4)) != hipSuccess ||
      (e = hipMemset(nat_abort.p, 0, 16)) != hipSuccess)
    return hipfail(e, "natural SSOR vectors");
  csr_nnz = nnz;
  csr_pat = mask;
  csr_nf = nf;
  csr_vals_valid = false;
  return PNP_OK;
}

// the CSR view's values from the current k-form matrix (once per assembly)
int pnp_ctx::csr_values() {
  int rc;
  if ((rc = csr_structure())) return rc;
  if (csr_vals_valid) return nat_probe_run();
  if ((rc = ensure_values())) return rc;
  hipError_t e = pnp::launch_csr_fill(dl, nf, pat, vals.p, csr_nnz, csr_src.p, csr_vidx.p,
                                      csr_val.p, stream);
  if (e != hipSuccess) return hipfail(e, "csr fill");
  csr_vals_valid = true;
  return nat_probe_run();
}

// one launch for both sweeps (ssor_natural.hip, launch_ssor_natural_flow) whenever this context
// owns its GPU: one rank, or one rank of an RCCL communicator (one process per GPU, each rank
// sweeping its owned rows -- block Jacobi across ranks, as ISTL's NOVLP SeqSSOR on the local
// matrix).  The in-process local group keeps the level launches: its ranks share one device, and
// the dataflow needs every workgroup of its grid resident.  PNP_NAT_FLOW=0 keeps the level
// launches everywhere
bool pnp_ctx::use_nat_flow() const {
  static const bool env_on = [] {
    const char *ev = std::getenv("PNP_NAT_FLOW");
    return !(ev && std::atoi(ev) == 0);
  }();
  return nat_resident != 0 &&
         (nat_flow_opt == 0   ? false
          : nat_flow_opt == 1 ? nat_units_ok
                              : env_on && !lg && !host_tr() && nat_units_ok);
}

int pnp_ctx::nat_probe_run() {
  if (nat_resident >= 0 || !use_nat_flow()) return PNP_OK;
  // test hook: PNP_NAT_PROBE_FAIL=1 takes the probe's "not resident" answer without running it
  // (tests/test_gpu_ssor_natural.py: the level launches are then used, bitwise the same)
  if (const char *ev = std::getenv("PNP_NAT_PROBE_FAIL"); ev && std::atoi(ev) == 1) {
    nat_resident = 0;
    return PNP_OK;
  }
  hipError_t e = nat_probe.p ? hipSuccess : nat_probe.alloc(2);
  if (e != hipSuccess) return hipfail(e, "natural SSOR probe");
  const int r = pnp::ssor_natural_flow_resident(nat_flow_view(), nat_probe.p, stream);
  if (r < 0) return fail(PNP_E_HIP, "natural SSOR: co-residency probe failed");
  nat_resident = r;
  return PNP_OK;
}

hipError_t pnp_ctx::nat_sweep(const double *d, double *vout) {
  if (use_nat_flow()) {
    nat_flow_n++;
    return ssor_natural_flow(d, vout);
  }
  nat_level_n++;
  return ssor_natural_levels(d, vout);
}

pnp::NatFlow pnp_ctx::nat_flow_view() const {
  pnp::NatFlow F;
  F.units = d_nat_units.p;
  F.nunits = int(nat_units.size());
  F.nunits_f = nat_units_f;
  F.tail_f = nat_tail_f;
  F.tail_b = nat_tail_b;
  F.max_width = nat_max_width;
  F.chain_f = nat_f.chains();
  F.chain_b = nat_b.chains();
  F.fwd = nat_f.view();
  F.bwd = nat_b.view();
  F.abort_word = nat_abort.p;
  return F;
}

hipError_t pnp_ctx::ssor_natural_flow(const double *d, double *vout) {
  const pnp::NatFlow F = nat_flow_view();
  hipError_t e = pnp::launch_ssor_natural_flow(F, nf * mesh.nv, csr_val.p, d, nat_vf.p, nat_v.p,
                                               stream);
  // the result out of the external-layout vb (storing it at internal positions from the
  // backward kernels as well cost more than this gather: +40 against 22 us, r5f)
  if (e == hipSuccess)
    e = pnp::launch_gather_ext(L.n_owned, nf, mesh.nv, d_l2g.p, nat_v.p, vout, stream);
  return e;
}

// a dataflow sweep that timed out (never expected: every unit waits only on earlier units, all
// resident) leaves NaN results and a sticky word; the solve reports it as an error
int pnp_ctx::nat_check() {
  if (!use_nat_flow() || !nat_abort.p) return PNP_OK;
  unsigned w = 0;
  hipError_t e = hipMemcpyAsync(&w, nat_abort.p, 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "natural SSOR status");
  if (w) {
    hipMemsetAsync(nat_abort.p, 0, 16, stream);
    return fail(PNP_E_HIP, "natural SSOR: dataflow sweep timed out waiting for an operand");
  }
  return PNP_OK;
}

// ---- ILU(0) application as one dataflow launch (PNP_OPT_ILU_FLOW) -----------------------------
// Units in the colour launches' order (forward colours c_first .. nc-2, the last colour, backward
// colours nc-2 .. 0), one per 256-position block of the colour.  A unit's dependencies (all
// earlier in the order): forward / last -- the forward units of the rows in its L staging list;
// backward -- the backward (or last-colour) units of the rows in its U list, the forward units of
// its own rows (their forward values are its input) and every forward unit whose L list holds one
// of its rows (which must have read that row's forward value before it is overwritten).
int pnp_ctx::ilu_flow_build(int c_first, IluFlowDev &D) {
  D.built = true;
  D.ok = false;
  const int nc = int(L.color_ptr.size()) - 1;
  const std::vector<int> &cp = L.color_ptr;
  if (!dl.lsx_ptr || nc < 2 || hl.posrowL.empty()) return PNP_OK;
  std::vector<int> nb(nc), blk0(nc + 1, 0);
  for (int c = 0; c < nc; c++) {
    nb[c] = (cp[c + 1] - cp[c] + 255) / 256;
    blk0[c + 1] = blk0[c] + nb[c];
  }
  std::vector<std::pair<int, int>> stages;  // {kind, colour}
  for (int c = c_first; c < nc - 1; c++) stages.push_back({0, c});
  stages.push_back({2, nc - 1});
  for (int c = nc - 2; c >= 0; c--) stages.push_back({1, c});
  if (int(stages.size()) > pnp::kIluFlowMaxStages) return PNP_OK;
  pnp::IluFlow F;
  F.nstages = int(stages.size());
  int nu = 0;
  for (int s = 0; s < F.nstages; s++) {
    const int c = stages[s].second;
    F.unit0[s] = nu;
    F.kind[s] = stages[s].first;
    F.r0[s] = cp[c];
    F.r1[s] = cp[c + 1];
    F.blk0[s] = blk0[c];
    nu += nb[c];
  }
  F.unit0[F.nstages] = nu;
  F.nunits = nu;
  const int no = L.n_owned;
  std::vector<int> fwdu(no, -1), bwdu(no, -1);
  for (int s = 0; s < F.nstages; s++) {
    const int c = stages[s].second, kind = stages[s].first;
    for (int p = cp[c]; p < cp[c + 1]; p++) {
      const int u = F.unit0[s] + (p - cp[c]) / 256;
      if (kind != 1) fwdu[hl.posrowL[p]] = u;
      if (kind != 0) bwdu[hl.posrowU[p]] = u;
    }
  }
  // readers[r]: forward / last units whose L list holds row r (CSR)
  std::vector<int> rptr(no + 1, 0), rdr;
  auto lblock = [&](int s, int u) { return F.blk0[s] + (u - F.unit0[s]); };
  for (int pass = 0; pass < 2; pass++) {
    for (int s = 0; s < F.nstages; s++) {
      if (F.kind[s] == 1) continue;
      for (int u = F.unit0[s]; u < F.unit0[s + 1]; u++) {
        const int b = lblock(s, u);
        for (int k = hl.lsx_ptr[b]; k < hl.lsx_ptr[b + 1]; k++) {
          const int j = hl.lsx_list[k];
          if (pass == 0)
            rptr[j + 1]++;
          else
            rdr[rptr[j]++] = u;
        }
      }
    }
    if (pass == 0) {
      for (int r = 0; r < no; r++) rptr[r + 1] += rptr[r];
      rdr.assign(rptr[no], 0);
    } else {
      for (int r = no; r > 0; r--) rptr[r] = rptr[r - 1];
      rptr[0] = 0;
    }
  }
  std::vector<int> dptr(nu + 1, 0), dlist, dep;
  for (int s = 0; s < F.nstages; s++) {
    const int c = stages[s].second;
    for (int u = F.unit0[s]; u < F.unit0[s + 1]; u++) {
      const int b = lblock(s, u);
      dep.clear();
      if (F.kind[s] != 1) {
        for (int k = hl.lsx_ptr[b]; k < hl.lsx_ptr[b + 1]; k++)
          if (fwdu[hl.lsx_list[k]] >= 0) dep.push_back(fwdu[hl.lsx_list[k]]);
      } else {
        for (int k = hl.usx_ptr[b]; k < hl.usx_ptr[b + 1]; k++)
          if (bwdu[hl.usx_list[k]] >= 0) dep.push_back(bwdu[hl.usx_list[k]]);
        const int p0 = cp[c] + 256 * (u - F.unit0[s]), p1 = std::min(cp[c + 1], p0 + 256);
        for (int p = p0; p < p1; p++) {
          const int r = hl.posrowU[p];
          if (fwdu[r] >= 0) dep.push_back(fwdu[r]);
          for (int k = rptr[r]; k < rptr[r + 1]; k++) dep.push_back(rdr[k]);
        }
      }
      std::sort(dep.begin(), dep.end());
      dep.erase(std::unique(dep.begin(), dep.end()), dep.end());
      for (int w : dep)
        if (w >= u) return fail(PNP_E_STATE, "ILU(0) dataflow: a unit depends on a later one");
      dlist.insert(dlist.end(), dep.begin(), dep.end());
      dptr[u + 1] = int(dlist.size());
    }
  }
  if (dlist.empty()) dlist.push_back(0);
  int rc;
  if ((rc = upload(D.dep_ptr, dptr, "ILU(0) dataflow deps")) ||  // neither is empty
      (rc = upload(D.dep_list, dlist, "ILU(0) dataflow deps")))
    return rc;
  hipError_t e = D.flags.alloc(size_t(nu + 1 + 3) & ~size_t(3));
  if (e == hipSuccess && !ilu_flow_abort.p) {
    e = ilu_flow_abort.alloc(4);
    if (e == hipSuccess) e = hipMemset(ilu_flow_abort.p, 0, 16);
  }
  if (e != hipSuccess) return hipfail(e, "ILU(0) dataflow flags");
  F.dep_ptr = D.dep_ptr.p;
  F.dep_list = D.dep_list.p;
  F.flags = D.flags.p;
  F.abort_word = ilu_flow_abort.p;
  D.F = F;
  D.ok = true;
  return PNP_OK;
}

// v = ILU(0)^-1 d over the owned rows, colours from c_first (launch_ilu0_apply's contract): one
// dataflow launch when PNP_OPT_ILU_FLOW is on and d and v are distinct, else the colour launches
int pnp_ctx::ilu_apply(const double *d, double *vout, int c_first, const char *what,
                       hipEvent_t t0, hipEvent_t t1) {
  // the resident-grid form needs the device to itself: not with in-process ranks sharing it
  // (and one context per GPU at N > 1); PNP_ILU_FLOW_TICKET=1: the ticketed form (any residency)
  // PNP_ILU_FLOW_MODE: IluFlow::persistent (0 ticket, 1 static resident grid, the default).
  // A third form, a resident grid over 8 ticketed queues, hung in the bitwise tests (killed
  // after 180 s of silence, gpurun_out r4i) and was removed
  static const int mode = [] {
    const char *ev = std::getenv("PNP_ILU_FLOW_MODE");
    const int m = ev ? std::atoi(ev) : 1;
    return (m >= 0 && m <= 1) ? m : 1;
  }();
  // PNP_OPT_ILU_FLOW = 2 selects the ticketed form (any residency, so also ranks sharing a GPU)
  const int fmode = ilu_flow_opt == 2 ? 0 : mode;
  if (ilu_flow_opt && d != vout && (c_first == 0 || c_first == 1) && (fmode == 0 || !dist)) {
    IluFlowDev &D = ilu_flow[c_first];
    int rc;
    if (!D.built && (rc = ilu_flow_build(c_first, D))) return rc;
    D.F.persistent = fmode;
    if (D.ok) {
      if (t0) hipEventRecord(t0, stream);
      hipError_t e = pnp::launch_ilu0_flow(dl, D.F, nf, pat, lvals.p, uvals.p, d, vout, stream,
                                           f32_now());
      if (t1) hipEventRecord(t1, stream);
      if (e != hipSuccess) return hipfail(e, what);
      ilu_flow_used = true;
      ilu_flow_n++;
      return PNP_OK;
    }
  }
  hipError_t e = pnp::launch_ilu0_apply(dl, L.color_ptr.data(), nf, pat, lvals.p, uvals.p, d,
                                        vout, stream, c_first, nullptr, nullptr, f32_now(),
                                        ilu_y32(), t0, t1);
  return e == hipSuccess ? PNP_OK : hipfail(e, what);
}

// a dataflow application that timed out (never expected) leaves void results and a sticky word
int pnp_ctx::ilu_flow_check() {
  if (!ilu_flow_used || !ilu_flow_abort.p) return PNP_OK;
  ilu_flow_used = false;
  unsigned w = 0;
  hipError_t e = hipMemcpyAsync(&w, ilu_flow_abort.p, 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "ILU(0) dataflow status");
  if (w) {
    hipMemsetAsync(ilu_flow_abort.p, 0, 16, stream);
    return fail(PNP_E_HIP, "ILU(0) dataflow application timed out waiting for a unit");
  }
  return PNP_OK;
}

hipError_t pnp_ctx::ssor_natural_levels_fixed() {
  auto issue = [&] {
    hipError_t e0 = hipMemsetAsync(nat_v.p, 0, sizeof(double) * nat_v.n, stream);
    return e0 != hipSuccess ? e0
                            : pnp::launch_ssor_natural(nat_f.view(), nat_b.view(), csr_val.p,
                                                       nat_d.p, nat_v.p, stream);
  };
  static const bool env_on = [] {
    const char *ev = std::getenv("PNP_NAT_GRAPH");
    return !(ev && std::atoi(ev) == 0);
  }();
  // not with more than one rank: in-process ranks share the device, and another rank's thread
  // touching the legacy stream during a capture would invalidate it
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (!env_on || dist || nat_graph_failed || profiled() ||
      hipStreamIsCapturing(stream, &cs) != hipSuccess ||
      cs != hipStreamCaptureStatusNone)
    return issue();
  if (!nat_exec) {
    hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
      const hipError_t e1 = issue();
      hipGraph_t g = nullptr;
      const hipError_t e2 = hipStreamEndCapture(stream, &g);
      e = e1 != hipSuccess ? e1 : e2;
      if (e == hipSuccess) e = hipGraphInstantiate(&nat_exec, g, nullptr, nullptr, 0);
      if (g) hipGraphDestroy(g);
    }
    if (e != hipSuccess || !nat_exec) {  // nothing of the capture ran: launch eagerly
      (void)hipGetLastError();
      nat_exec = nullptr;
      nat_graph_failed = true;
      return issue();
    }
  }
  return hipGraphLaunch(nat_exec, stream);
}

// analytic (k-form) or forward-difference (expanded, kPat*FD) storage of the next Jacobian
int pnp_ctx::set_fd(bool on) {
  if (on == fd_mode) return PNP_OK;
  graphs_clear();
  int rc;
  // P_k: the element kernel differentiates by itself; scalar blocks need no FD value layout
  if (on && !fd_built && degree == 1 && (rc = fd_build())) return rc;
  pat = (on && nf == 3) ? (base_pat(kind) | pnp::kPatFD) : base_pat(kind);
  nks = pnp::nks_of(pat);
  fd_mode = on;
  jacobian_drop();           // assemble(), the only caller, stores one next or fails
  vals_const_valid = false;  // another value layout, zeroed below
  if (on && degree == 1) {
    // one-step operators keep two matrices per element (spatial, temporal: fd_jacobian.hip)
    const size_t need = size_t(fd_ne) * 9 * nf * nf * 2;
    if (fd_jel.n < need) {
      hipError_t e = fd_jel.alloc(need);
      if (e != hipSuccess) return hipfail(e, "fd element matrices");
    }
  }
  // padding slots must read as zeros in the new value layout (the SpMV multiplies them)
  hipError_t e = hipMemsetAsync(vals.p, 0, sizeof(double) * size_t(L.nslots) * nks, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, "clear matrix");
}

// P_k element lists (once per context): the local elements (every element with an owned node,
// ascending global id) and their local nodes (SoA); per owned row its incident elements in
// ascending order, in SELL-chunk layout (PkDev), with the row's slot of every element node
int pnp_ctx::pk_build() {
  const pnp::Mesh &m = tmesh;
  const int nl = pks.nl, nw = (nl + 3) / 4;
  std::vector<int> en;
  std::vector<int> elist;
  for (int e = 0; e < m.nt; e++) {
    const int *g = &pks.enode[size_t(e) * nl];
    bool mine = false, local = true;
    for (int a = 0; a < nl; a++) {
      const int l = L.g2l[g[a]];
      mine = mine || (l >= 0 && l < L.n_owned);
      local = local && l >= 0;
    }
    if (!mine) continue;
    if (!local) return fail(PNP_E_MESH, "P_k: element not local");
    elist.push_back(e);
  }
  const int ne = int(elist.size());
  if (ne >= (1 << 27)) return fail(PNP_E_MESH, "P_k: too many local elements");
  en.resize(size_t(ne) * nl);
  for (int e = 0; e < ne; e++)
    for (int a = 0; a < nl; a++) en[size_t(a) * ne + e] = L.g2l[pks.enode[size_t(elist[e]) * nl + a]];
  auto slot_of = [&](int row, int col) -> int {
    const int ch = row / pnp::kRows, ln = row % pnp::kRows, len = pnp::meta_len(L.rowmeta[row]);
    if (col == row) return 0;
    for (int sl = 1; sl < len; sl++)
      if (L.colidx[L.chunk_off[ch] + 64LL * sl + ln] == col) return sl;
    return -1;
  };
  // incidences per owned row, ascending element order
  std::vector<int> icnt(L.n_owned, 0);
  for (int e = 0; e < ne; e++)
    for (int a = 0; a < nl; a++) {
      const int ra = en[size_t(a) * ne + e];
      if (ra < L.n_owned) icnt[ra]++;
    }
  std::vector<int> ioff(L.nchunks + 1, 0);
  for (int c = 0; c < L.nchunks; c++) {
    int mx = 0;
    for (int ln = 0; ln < pnp::kRows && c * pnp::kRows + ln < L.n_owned; ln++)
      mx = std::max(mx, icnt[c * pnp::kRows + ln]);
    ioff[c + 1] = ioff[c] + pnp::kRows * mx;
  }
  std::vector<int> inc(std::max(1, ioff[L.nchunks]), 0), fill(L.n_owned, 0);
  std::vector<uint32_t> islot(size_t(std::max(1, ioff[L.nchunks])) * nw, 0);
  for (int e = 0; e < ne; e++)
    for (int a = 0; a < nl; a++) {
      const int ra = en[size_t(a) * ne + e];
      if (ra >= L.n_owned) continue;
      const int c = ra / pnp::kRows, ln = ra % pnp::kRows;
      const size_t p = size_t(ioff[c]) + size_t(pnp::kRows) * fill[ra]++ + ln;
      inc[p] = e << 4 | a;
      for (int b = 0; b < nl; b++) {
        const int sl = slot_of(ra, en[size_t(b) * ne + e]);
        if (sl < 0) return fail(PNP_E_MESH, "P_k: element pair outside the pattern");
        islot[p * nw + (b >> 2)] |= uint32_t(sl) << (8 * (b & 3));
      }
    }
  int rc;
  if ((rc = upv(pk_enode, en, "P_k elements")) || (rc = upv(pk_ioff, ioff, "P_k ioff")) ||
      (rc = upv(pk_icnt, icnt, "P_k icnt")) || (rc = upv(pk_inc, inc, "P_k incidences")) ||
      (rc = upv(pk_islot, islot, "P_k slots")))
    return rc;
  hipError_t e = pk_eres.alloc(std::max<size_t>(1, size_t(ne) * nl));
  if (e != hipSuccess) return hipfail(e, "P_k element residual scratch");
  e = pk_ejac.alloc(std::max<size_t>(1, size_t(ne) * nl * ((nl + 2) & ~1)));
  if (e != hipSuccess) return hipfail(e, "P_k element matrix scratch");
  e = pnp::pk_upload_tables(pks.k, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hipfail(e, "P_k tables");
  pkd.k = pks.k;
  pkd.nl = nl;
  pkd.ne = ne;
  pkd.enode = pk_enode.p;
  pkd.ioff = pk_ioff.p;
  pkd.icnt = pk_icnt.p;
  pkd.inc = pk_inc.p;
  pkd.islot = pk_islot.p;
  pkd.eres = pk_eres.p;
  pkd.ejac = pk_ejac.p;
  // the Jacobian gather pass accumulates a row's slots in LDS, sized for the longest row: the
  // vertex rows (up to 55 slots at P3) would hold every workgroup to one per CU.  When the
  // longest row needs more than 64 KB per workgroup, blocks whose rows are all at most the
  // median block length (the edge and interior node rows) run in a launch of their own with an
  // LDS accumulator of that length: P3 438 -> 395 us; at P2 (one launch at 3 workgroups per CU)
  // the second launch costs more than it gains, 135 -> 145 us (profiles/r02/ab_pk_split).
  // PNP_PK_SPLIT=0: always one launch, 1: split whenever the median is at most half the longest
  {
    const char *ev = getenv("PNP_PK_SPLIT");
    const int nblk = (L.n_owned + 255) / 256;
    std::vector<int> order(nblk), blen(nblk, 0);
    for (int b = 0; b < nblk; b++) order[b] = b;
    if (dl.blkmap && nblk > 0) order = hl.blkmap;
    for (int r = 0; r < L.n_owned; r++)
      blen[r / 256] = std::max(blen[r / 256], pnp::meta_len(L.rowmeta[r]));
    std::vector<int> srt(blen);
    std::nth_element(srt.begin(), srt.begin() + nblk / 2, srt.end());
    const int T = nblk > 0 ? srt[nblk / 2] : 0;
    const int mx = nblk > 0 ? *std::max_element(blen.begin(), blen.end()) : 0;
    const bool want = ev ? ev[0] == '1' : size_t(mx) * 256 * sizeof(double) > 64 * 1024;
    if (want && nblk > 0 && 2 * T <= mx) {
      std::vector<int> sh, lo;
      for (int b : order) (blen[b] <= T ? sh : lo).push_back(b);
      if ((rc = upv(pk_blk_short, sh, "P_k short blocks")) ||
          (rc = upv(pk_blk_long, lo, "P_k long blocks")))
        return rc;
      pkd.blk_short = pk_blk_short.p;
      pkd.blk_long = pk_blk_long.p;
      pkd.n_short = int(sh.size());
      pkd.n_long = int(lo.size());
      pkd.short_len = T;
    }
  }
  // ion-flux segments handled by this rank: those whose element is local and whose lower
  // global vertex is owned here, {local element, face, group}, in global segment order
  std::vector<int> eloc(m.nt, -1);
  for (int e2 = 0; e2 < ne; e2++) eloc[elist[e2]] = e2;
  std::vector<int4> segs;
  fseg_group.clear();
  for (int sg = 0; sg < m.nb; sg++) {
    const int a = m.bseg[2 * size_t(sg)], b = m.bseg[2 * size_t(sg) + 1];
    const int lo = L.g2l[std::min(a, b)];
    if (lo < 0 || lo >= L.n_owned) continue;
    const int bf = pks.bface[sg];
    if (bf < 0 || eloc[bf / 3] < 0) return fail(PNP_E_MESH, "ion flux: the element of a boundary segment is not local");
    segs.push_back(make_int4(eloc[bf / 3], bf % 3, m.bgroup[sg], 0));
    fseg_group.push_back(m.bgroup[sg]);
  }
  if ((rc = upv(d_fseg, segs, "P_k flux segments"))) return rc;
  e = fluxout.alloc(2 * segs.size() + 2);
  if (e != hipSuccess) return hipfail(e, "flux out");
  return PNP_OK;
}

// local elements (ascending global id, vertices in mesh order) and, per owned row and slot, the
// element entries summed into that block, in ascending element order
int pnp_ctx::fd_build() {
  const pnp::Mesh &m = mesh;
  std::vector<int> et;
  for (int e = 0; e < m.nt; e++) {
    const int *t = &m.tri[3 * size_t(e)];
    const int l0 = L.g2l[t[0]], l1 = L.g2l[t[1]], l2 = L.g2l[t[2]];
    const bool mine = (l0 >= 0 && l0 < L.n_owned) || (l1 >= 0 && l1 < L.n_owned) ||
                      (l2 >= 0 && l2 < L.n_owned);
    if (!mine) continue;
    if (l0 < 0 || l1 < 0 || l2 < 0) return fail(PNP_E_MESH, "FD Jacobian: element not local");
    et.push_back(l0);
    et.push_back(l1);
    et.push_back(l2);
  }
  const int ne = int(et.size() / 3);
  auto pos_of = [&](int row, int col) -> long long {
    const int ch = row / pnp::kRows, ln = row % pnp::kRows, len = pnp::meta_len(L.rowmeta[row]);
    if (col == row) return L.chunk_off[ch] + ln;
    for (int sl = 1; sl < len; sl++) {
      const long long p = L.chunk_off[ch] + 64LL * sl + ln;
      if (L.colidx[p] == col) return p;
    }
    return -1;
  };
  std::vector<int> cnt(size_t(L.nslots) + 1, 0);
  for (int e = 0; e < ne; e++)
    for (int a = 0; a < 3; a++) {
      const int va = et[3 * size_t(e) + a];
      if (va >= L.n_owned) continue;
      for (int b = 0; b < 3; b++) {
        const long long p = pos_of(va, et[3 * size_t(e) + b]);
        if (p < 0) return fail(PNP_E_MESH, "FD Jacobian: element pair outside the pattern");
        cnt[p]++;
      }
    }
  // per row: for each slot, the count then its codes
  std::vector<long long> rptr(L.n_owned + 1, 0);
  for (int i = 0; i < L.n_owned; i++) {
    const int ch = i / pnp::kRows, ln = i % pnp::kRows, len = pnp::meta_len(L.rowmeta[i]);
    long long n = 0;
    for (int sl = 0; sl < len; sl++) n += 1 + cnt[L.chunk_off[ch] + 64LL * sl + ln];
    rptr[i + 1] = rptr[i] + n;
  }
  std::vector<long long> at((size_t)L.nslots, -1LL);  // next free code position of each block
  std::vector<int> data((size_t)rptr[L.n_owned]);
  for (int i = 0; i < L.n_owned; i++) {
    const int ch = i / pnp::kRows, ln = i % pnp::kRows, len = pnp::meta_len(L.rowmeta[i]);
    long long q = rptr[i];
    for (int sl = 0; sl < len; sl++) {
      const long long p = L.chunk_off[ch] + 64LL * sl + ln;
      data[q] = cnt[p];
      at[p] = q + 1;
      q += 1 + cnt[p];
    }
  }
  for (int e = 0; e < ne; e++)
    for (int a = 0; a < 3; a++) {
      const int va = et[3 * size_t(e) + a];
      if (va >= L.n_owned) continue;
      for (int b = 0; b < 3; b++) {
        const long long p = pos_of(va, et[3 * size_t(e) + b]);
        data[at[p]++] = e * 9 + a * 3 + b;
      }
    }
  int rc;
  if ((rc = upv(fd_etri, et, "fd elements")) || (rc = upv(fd_rptr, rptr, "fd rptr")) ||
      (rc = upv(fd_cdata, data, "fd contributions")))
    return rc;
  fd_ne = ne;
  fd_built = true;
  return PNP_OK;
}

// ILU(0) factors of the current matrix (once per assembly).  Default: the fused factorisation
// (expand and split folded in, neighbour-row work hoisted; PNP_OPT_ILU_FUSED_FACTOR = 0 runs the
// three-pass path, the same bits)
int pnp_ctx::ilu_factor() {
  if (lu_valid) return PNP_OK;
  if (int rc = ensure_values()) return rc;
  hipEvent_t t0 = tb(T_FACT);
  hipError_t e;
  if (ilu_fused) {
    e = pnp::launch_ilu0_factor_fused(dl, L.color_ptr.data(), nf, pat, vals.p, d_rowoff.p,
                                      d_rowcol.p, lu.p, lvals.p, uvals.p, ilu_fac(), stream);
  } else {
    e = pnp::launch_expand(dl, nf, pat, vals.p, lu.p, stream);
    if (e == hipSuccess)
      e = pnp::launch_ilu0_factor(dl, L.color_ptr.data(), nf, pat, lu.p, stream);
  }
  if (e != hipSuccess) return hipfail(e, "ilu0 factorisation");
  te(T_FACT, t0);
  lu_valid = true;
  split_of = ilu_fused ? 2 : 0;
  return PNP_OK;
}

// bring the split storage up to date with the matrix (which = 1) or the factors (which = 2)
int pnp_ctx::split(int which) {
  if (split_of == which) return PNP_OK;
  if (which == 2 && ilu_fused) {  // the fused factorisation keeps no SELL copy: redo it
    lu_valid = false;
    return ilu_factor();
  }
  if (which == 1)
    if (int rc = ensure_values()) return rc;
  hipEvent_t t0 = tb(T_FACT);
  hipError_t e = pnp::launch_split(dl, nf, pat, which == 1 ? 1 : 0, which == 2 ? lu.p : vals.p,
                                   d_lsrc.p, (long long)d_lsrc.n, d_usrc.p, (long long)d_usrc.n,
                                   lvals.p, uvals.p, stream, which == 2 ? ilu_fac() : 0);
  if (e != hipSuccess) return hipfail(e, "split");
  te(T_FACT, t0);
  split_of = which;
  return PNP_OK;
}

// hierarchy patterns (once), value/vector buffers (per field count), coarse values (per
// assembly): Galerkin sums, block-diagonal inverses, the coarsest dense inverse
int pnp_ctx::amg_setup() {
  int rc;
  if (!assembled) return fail(PNP_E_STATE, "no Jacobian assembled");
  // the Galerkin products and the V-cycle's level-0 residuals read the SELL values
  if ((rc = ensure_values())) return rc;
  if (!amg_built) {
    amg_d.clear();
    if (!pnp::amg_build(L, amg_opts.coarse_target, amg_opts.max_levels, amg_h, err))
      return PNP_E_STATE;
    for (const auto &H : amg_h) {
      auto D = std::make_unique<AmgDev>();
      D->nb = H.nb;
      if ((rc = upv(D->rp, H.rp, "amg rp")) || (rc = upv(D->col, H.col, "amg col")) ||
          (rc = upv(D->dpos, H.dpos, "amg dpos")) || (rc = upv(D->mptr, H.mptr, "amg mptr")) ||
          (rc = upv(D->mem, H.mem, "amg mem")) || (rc = upv(D->agg, H.agg, "amg agg")) ||
          (rc = upv(D->csrc, H.csrc, "amg csrc")) || (rc = upv(D->cptr, H.cptr, "amg cptr")))
        return rc;
      amg_d.push_back(std::move(D));
    }
    amg_built = true;
    amg_nf = 0;
  }
  if (amg_d.empty()) return fail(PNP_E_STATE, "AMG: no owned rows");
  const int K = int(amg_d.size());
  if (amg_d[K - 1]->nb * nf > pnp::kAmgMaxDense)
    return fail(PNP_E_STATE, "AMG: coarsest level too large for the dense solve");
  if (amg_nf != nf) {
    const size_t nb2 = size_t(nf) * nf;
    for (auto &D : amg_d) {
      hipError_t e;
      if ((amg_f32() && D.get() != amg_d.back().get() &&
           (e = D->vf.alloc(std::max<size_t>(1, D->col.n) * nb2)) != hipSuccess) ||
          (e = D->v.alloc(std::max<size_t>(1, D->col.n) * nb2)) != hipSuccess ||
          (e = D->dinv.alloc(size_t(D->nb) * nb2)) != hipSuccess ||
          (e = D->b.alloc(size_t(D->nb) * nf)) != hipSuccess ||
          (e = D->x.alloc(size_t(D->nb) * nf)) != hipSuccess ||
          (e = D->x2.alloc(size_t(D->nb) * nf)) != hipSuccess)
        return hipfail(e, "amg level buffers");
    }
    const size_t nc = size_t(amg_d[K - 1]->nb) * nf, nl = size_t(L.n_owned + L.n_ghost) * nf;
    hipError_t e;
    amg_ld = int((nc + 3) & ~size_t(3));
    if ((amg_f32() && (e = amg_ainv_f.alloc(nc * size_t(amg_ld))) != hipSuccess) ||
        (e = amg_ainv.alloc(nc * nc)) != hipSuccess || (e = amg_ipiv.alloc(nc)) != hipSuccess ||
        (e = amg_info.alloc(1)) != hipSuccess ||
        (e = amg_x0.alloc(nl)) != hipSuccess || (e = amg_t.alloc(nl)) != hipSuccess ||
        (e = amg_y.alloc(nl)) != hipSuccess || (e = amg_r.alloc(nl)) != hipSuccess ||
        (e = amg_z.alloc(nl)) != hipSuccess)
      return hipfail(e, "amg vectors");
    amg_nf = nf;
    amg_valid = false;
  }
  // (a Jacobi smoother's prerequisite is a no-op here: ensure_values() above left vals current)
  if ((rc = prec_prepare(amg_opts.smoother))) return rc;
  if (amg_valid) return PNP_OK;
  hipEvent_t t0 = tb(T_FACT);
  double ts = now_s();
  hipError_t e = pnp::launch_amg_galerkin0(dl, nf, pat, vals.p, (long long)amg_h[0].col.size(),
                                           amg_d[0]->cptr.p, amg_d[0]->csrc.p, amg_d[0]->v.p,
                                           stream);
  for (int k = 1; k < K && e == hipSuccess; k++)
    e = pnp::launch_amg_galerkin(nf, (long long)amg_h[k].col.size(), amg_d[k]->cptr.p,
                                 amg_d[k]->csrc.p, amg_d[k - 1]->v.p, amg_d[k]->v.p, stream);
  for (int k = 0; k + 1 < K && e == hipSuccess; k++)
    e = pnp::launch_amg_dinv(nf, amg_d[k]->nb, amg_d[k]->dpos.p, amg_d[k]->v.p,
                             amg_d[k]->dinv.p, stream);
  for (int k = 0; k + 1 < K && e == hipSuccess; k++)
    if (amg_d[k]->vf.p)
      e = pnp::launch_amg_to_f32((long long)amg_d[k]->col.n * nf * nf, amg_d[k]->v.p,
                                 amg_d[k]->vf.p, stream);
  if (e == hipSuccess)
    e = pnp::launch_amg_coarse_dense(nf, amg_d[K - 1]->nb, amg_d[K - 1]->rp.p,
                                     amg_d[K - 1]->col.p, amg_d[K - 1]->v.p, amg_ainv.p, stream);
  if (e != hipSuccess) return hipfail(e, "amg setup");
  {  // coarsest inverse in place: LU with partial pivoting, then the inverse -- of A^T column-
     // major, which leaves A^-1 row-major for k_coarse_apply
    if (!blas) {
      if (rocblas_create_handle(&blas) != rocblas_status_success)
        return fail(PNP_E_HIP, "rocblas_create_handle failed");
    }
    if (rocblas_set_stream(blas, stream) != rocblas_status_success)
      return fail(PNP_E_HIP, "rocblas_set_stream failed");
    const int nc = amg_d[K - 1]->nb * nf;
    if (rocsolver_dgetrf(blas, nc, nc, amg_ainv.p, nc, amg_ipiv.p, amg_info.p) !=
            rocblas_status_success ||
        rocsolver_dgetri(blas, nc, amg_ainv.p, nc, amg_ipiv.p, amg_info.p) !=
            rocblas_status_success)
      return fail(PNP_E_HIP, "rocsolver getrf/getri of the AMG coarsest level failed");
    int info = 0;
    e = hipMemcpyAsync(&info, amg_info.p, sizeof info, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hipfail(e, "amg setup");
    if (info != 0)
      return fail(PNP_E_STATE, "AMG: coarsest matrix singular (getrf info " +
                                   std::to_string(info) + ")");
    if (amg_ainv_f.p &&
        (e = pnp::launch_amg_inverse_to_f32(nc, amg_ld, amg_ainv.p, amg_ainv_f.p, stream)) !=
            hipSuccess)
      return hipfail(e, "amg setup");
  }
  te(T_FACT, t0);
  amg_setup_ms = (now_s() - ts) * 1e3;  // host-side issue time (device time: T_FACT timers)
  amg_valid = true;
  return PNP_OK;
}

// one V-cycle: vout = B d (owned rows); see amg.hip for the kernels
int pnp_ctx::amg_apply(const double *d, double *vout) {
  const int K = int(amg_d.size()), sm = amg_opts.smoother, n = L.n_owned;
  const double om = amg_opts.omega;
  const long long nn = nown();
  int rc, nsp = 0;
  hipError_t e;
  // level 0 pre-smoothing from zero, residual (SpMV residual mode), restriction (+ level-1
  // pre-smoothing); without level-0 pre-smoothing x0 = 0 and the restriction takes d itself
  // amg_opts.level0_presmooth: 1 always, 0 never, -1 (auto) only when the V-cycle must stay
  // symmetric (CG, or a bare pnp_prec_apply); BiCGSTAB takes the post-smoothing-only cycle
  const bool pre0 = amg_opts.level0_presmooth > 0 ||
                    (amg_opts.level0_presmooth < 0 && amg_symmetric);
  if (pre0) {
    if ((rc = smoother(sm, d, amg_x0.p, true))) return rc;
    e = pnp::launch_spmv(dl, nf, pat, vals.p, amg_x0.p, amg_t.p, 3, d, partials.p, &nsp,
                         stream);
  } else {
    e = hipSuccess;  // x0 = 0: the restriction takes d, the prolongation no x0
  }
  if (e == hipSuccess)
    e = pnp::launch_amg_restrict(nf, amg_d[0]->nb, amg_d[0]->mptr.p, amg_d[0]->mem.p,
                                 pre0 ? amg_t.p : d, nullptr, amg_d[0]->b.p, amg_d[0]->dinv.p,
                                 om, K > 1 ? amg_d[0]->x.p : nullptr, stream);
  for (int k = 0; k + 1 < K && e == hipSuccess; k++) {
    AmgDev &C = *amg_d[k], &N = *amg_d[k + 1];
    for (int sw = 1; sw < amg_sweeps(k) && e == hipSuccess; sw++) {  // more pre-smoothing
      e = pnp::launch_amg_post(nf, C.nb, C.rp.p, C.col.p, C.v.p, C.vf.p, nullptr, C.x.p,
                               nullptr, C.b.p, C.dinv.p, om, C.x2.p, stream);
      std::swap(C.x.p, C.x2.p);
    }
    // residual of level k+1 into its x2 (free until its post-smoothing), then restriction
    if (e == hipSuccess)
      e = pnp::launch_amg_resid(nf, C.nb, C.rp.p, C.col.p, C.v.p, C.vf.p, C.x.p, C.b.p,
                                C.x2.p, stream);
    if (e == hipSuccess)
      e = pnp::launch_amg_restrict(nf, N.nb, N.mptr.p, N.mem.p, C.x2.p, nullptr, N.b.p,
                                   N.dinv.p, om, k + 2 < K ? N.x.p : nullptr, stream);
  }
  if (e == hipSuccess)
    e = amg_ainv_f.p
            ? pnp::launch_amg_coarse_apply_f32(amg_d[K - 1]->nb * nf, amg_ld, amg_ainv_f.p,
                                               amg_d[K - 1]->b.p, amg_d[K - 1]->x.p, stream)
            : pnp::launch_amg_coarse_apply(amg_d[K - 1]->nb * nf, amg_ainv.p, amg_d[K - 1]->b.p,
                                     amg_d[K - 1]->x.p, stream);
  const double *res = amg_d[K - 1]->x.p;  // the solution of the level just finished
  for (int k = K - 2; k >= 0 && e == hipSuccess; k--) {
    AmgDev &C = *amg_d[k];
    e = pnp::launch_amg_post(nf, C.nb, C.rp.p, C.col.p, C.v.p, C.vf.p, amg_d[k + 1]->agg.p,
                             C.x.p, res, C.b.p, C.dinv.p, om, C.x2.p, stream);
    res = C.x2.p;
    for (int sw = 1; sw < amg_sweeps(k) && e == hipSuccess; sw++) {  // more post-smoothing
      double *out = res == C.x2.p ? C.x.p : C.x2.p;
      e = pnp::launch_amg_post(nf, C.nb, C.rp.p, C.col.p, C.v.p, C.vf.p, nullptr, res,
                               nullptr, C.b.p, C.dinv.p, om, out, stream);
      res = out;
    }
  }
  // level 0: prolongation, post-smoothing x += M^{-1} (d - A x)
  if (e == hipSuccess)
    e = pnp::launch_amg_prolong0(nf, n, amg_d[0]->agg.p, pre0 ? amg_x0.p : nullptr, res,
                                 amg_y.p, stream);
  if (e == hipSuccess)
    e = pnp::launch_spmv(dl, nf, pat, vals.p, amg_y.p, amg_r.p, 3, d, partials.p, &nsp, stream);
  if (e != hipSuccess) return hipfail(e, "amg v-cycle");
  if (sm == PNP_PREC_ILU0) {  // vout = y + M^-1 r, written by the backward sweep
    e = pnp::launch_ilu0_apply(dl, L.color_ptr.data(), nf, pat, lvals.p, uvals.p, amg_r.p,
                               amg_z.p, stream, 0, amg_y.p, vout, f32_now(), ilu_y32());
    return e == hipSuccess ? PNP_OK : hipfail(e, "amg v-cycle");
  }
  if ((rc = smoother(sm, amg_r.p, amg_z.p, true))) return rc;
  e = pnp::launch_axpby(nn, 1.0, amg_y.p, 1.0, amg_z.p, vout, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, "amg v-cycle");
}

int pnp_ctx::seq_build() {
  if (seq_built) return PNP_OK;
  const int nv = mesh.nv, nt = mesh.nt;
  std::vector<int> vptr(nv + 1, 0), vinc(size_t(3) * nt);
  for (int e = 0; e < nt; e++)
    for (int a = 0; a < 3; a++) vptr[mesh.tri[3 * e + a] + 1]++;
  for (int v = 0; v < nv; v++) vptr[v + 1] += vptr[v];
  std::vector<int> fill(vptr.begin(), vptr.end() - 1);
  for (int e = 0; e < nt; e++)  // ascending element index per vertex
    for (int a = 0; a < 3; a++) vinc[fill[mesh.tri[3 * e + a]]++] = e << 2 | a;
  int rc;
  if ((rc = upv(seq_tri, mesh.tri, "seq tri")) || (rc = upv(seq_xy, mesh.xy, "seq xy")) ||
      (rc = upv(seq_vptr, vptr, "seq vptr")) || (rc = upv(seq_vinc, vinc, "seq vinc")))
    return rc;
  hipError_t e;
  if ((e = seq_vec.alloc(size_t(SQ_N) * 3 * nv)) != hipSuccess ||
      (e = seq_dotv.alloc(2)) != hipSuccess || (e = seq_rl.alloc(size_t(9) * nt)) != hipSuccess ||
      (e = seq_rlo.alloc(size_t(9) * nt)) != hipSuccess ||
      (e = seq_rlt.alloc(size_t(9) * nt)) != hipSuccess ||
      (e = seq_jl.alloc(size_t(81) * nt)) != hipSuccess ||
      (e = seq_jlt.alloc(size_t(81) * nt)) != hipSuccess)
    return hipfail(e, "seq buffers");
  seq_built = true;
  return PNP_OK;
}

// per operator: constrained rows, alpha_boundary's terms per (element, local index) in the order
// PDELab adds them into the element's local vector (the oracle's boundary_face statements: the
// element's faces in DUNE's order (0,1), (0,2), (1,2), each a boundary intersection when its edge
// is a boundary segment, run from its lower to its higher local vertex; 2-point Gauss; fields in
// order; every basis function of the element at the face point; rl += scale * (j * phi * factor)),
// frozen fields
int pnp_ctx::seq_prepare() {
  int rc;
  if ((rc = seq_build())) return rc;
  if (seq_op_valid) return PNP_OK;
  if (seq_cextra) return fail(PNP_E_ARG, "PNP_OPT_SEQ_ORDER: pnp_op_args.c_extra is not supported");
  const int nt = mesh.nt, nl = 3 * nf;
  std::vector<std::vector<double>> terms(size_t(nt) * nl);
  const bool bnd = kind == PNP_OP_PNP || kind == PNP_OP_PNP_IMPLICIT_EULER || kind == PNP_OP_PB ||
                   kind == PNP_OP_POISSON;
  if (bnd) {
    std::unordered_map<long long, int> seg;  // edge -> its (first) boundary segment
    auto key = [](int a, int b) { return (long long)std::min(a, b) << 32 | unsigned(std::max(a, b)); };
    for (int b = 0; b < mesh.nb; b++) seg.emplace(key(mesh.bseg[2 * b], mesh.bseg[2 * b + 1]), b);
    static const int kFaceV[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    static const double corner[3][2] = {{0.0, 0.0}, {1.0, 0.0}, {0.0, 1.0}};
    const double PI = params.pi;
    const double scale = kind == PNP_OP_PNP_IMPLICIT_EULER ? seq_dt : 1.0;
    const double gt[2] = {0.5 - 0.5 / std::sqrt(3.0), 0.5 + 0.5 / std::sqrt(3.0)};
    for (int e = 0; e < nt && !seg.empty(); e++)
      for (int k = 0; k < 3; k++) {
        const int ia = kFaceV[k][0], ib = kFaceV[k][1];
        const int va = mesh.tri[3 * e + ia], vb = mesh.tri[3 * e + ib];
        const auto it = seg.find(key(va, vb));
        if (it == seg.end()) continue;
        const pnp::Surface &S = params.surf[mesh.bgroup[it->second]];
        const double dx = mesh.xy[2 * vb] - mesh.xy[2 * va],
                     dy = mesh.xy[2 * vb + 1] - mesh.xy[2 * va + 1];
        const double len = std::sqrt(dx * dx + dy * dy);
        for (int q = 0; q < 2; q++) {
          double factor = 0.5 * len;
          const double y = mesh.xy[2 * va + 1] + gt[q] * dy;
          if (params.cylindrical) factor *= y * 2 * PI;
          const double lx = corner[ia][0] + (corner[ib][0] - corner[ia][0]) * gt[q];
          const double ly = corner[ia][1] + (corner[ib][1] - corner[ia][1]) * gt[q];
          const double phi[3] = {1.0 - lx - ly, lx, ly};
          for (int f = 0; f < nf; f++) {
            if (S.btype(f) == 0) continue;  // isDirichlet
            const double j = S.flux(f);
            for (int i = 0; i < 3; i++)
              terms[size_t(e) * nl + 3 * f + i].push_back(scale * (j * phi[i] * factor));
          }
        }
      }
  }
  std::vector<int> bptr(size_t(nt) * nl + 1, 0);
  std::vector<double> bval;
  for (size_t q = 0; q < terms.size(); q++) {
    bptr[q + 1] = bptr[q] + int(terms[q].size());
    bval.insert(bval.end(), terms[q].begin(), terms[q].end());
  }
  if ((rc = upv(seq_bptr, bptr, "seq boundary")) || (rc = upv(seq_bval, bval, "seq boundary")))
    return rc;
  std::vector<unsigned char> m(seq_mask_h.begin(), seq_mask_h.end());
  if ((rc = upv(seq_mask, m, "seq mask"))) return rc;
  if ((rc = upv(seq_phi, seq_phi_h, "seq phi")) || (rc = upv(seq_cp, seq_cp_h, "seq cp")) ||
      (rc = upv(seq_cm, seq_cm_h, "seq cm")) || (rc = upv(seq_xold, seq_xold_h, "seq x_old")))
    return rc;
  seq_op_valid = true;
  return PNP_OK;
}

pnp::SeqMesh pnp_ctx::seq_mesh() const {
  pnp::SeqMesh M;
  M.nv = mesh.nv;
  M.nt = mesh.nt;
  M.tri = seq_tri.p;
  M.vptr = seq_vptr.p;
  M.vinc = seq_vinc.p;
  M.xy = seq_xy.p;
  return M;
}

pnp::SeqOp pnp_ctx::seq_op() const {
  pnp::SeqOp P;
  P.kind = kind;
  P.nf = nf;
  P.cyl = params.cylindrical;
  P.pi = params.pi;
  P.l_b = params.l_b;
  P.c0 = params.c0;
  P.tau = params.tau;
  P.dt = seq_dt;
  P.z = seq_z;
  P.phi = seq_phi_h.empty() ? nullptr : seq_phi.p;
  P.cp = seq_cp_h.empty() ? nullptr : seq_cp.p;
  P.cm = seq_cm_h.empty() ? nullptr : seq_cm.p;
  P.x_old = seq_xold_h.empty() ? nullptr : seq_xold.p;
  return P;
}

// r = R(x), both external layout on the device (GridOperator::residual + constraints)
int pnp_ctx::seq_residual(const double *x, double *r) {
  int rc;
  if ((rc = seq_prepare())) return rc;
  const bool old = kind == PNP_OP_PNP_IMPLICIT_EULER || kind == PNP_OP_DIFF_IMPLICIT_EULER;
  hipError_t e = pnp::launch_seq_element(seq_mesh(), seq_op(), x, 0, seq_rl.p, seq_rlt.p,
                                         seq_rlo.p, seq_jl.p, seq_jlt.p, seq_bptr.p, seq_bval.p,
                                         stream);
  if (e == hipSuccess)
    e = pnp::launch_seq_residual_gather(seq_mesh(), nf, old ? 1 : 0, seq_rl.p, seq_rlt.p,
                                        seq_rlo.p, seq_mask.p, r, stream);
  return e == hipSuccess ? PNP_OK : hipfail(e, "seq residual");
}

// the CSR view = J(x) (GridOperator::jacobian + constrained rows to identity); fd: PDELab's
// NumericalJacobianVolume
int pnp_ctx::seq_jacobian(const double *x, bool fd) {
  int rc;
  if ((rc = seq_prepare()) || (rc = csr_structure())) return rc;
  const bool onestep = kind == PNP_OP_PNP_IMPLICIT_EULER || kind == PNP_OP_DIFF_IMPLICIT_EULER;
  hipError_t e = pnp::launch_seq_element(seq_mesh(), seq_op(), x, fd ? 2 : 1, seq_rl.p,
                                         seq_rlt.p, seq_rlo.p, seq_jl.p, seq_jlt.p, seq_bptr.p,
                                         seq_bval.p, stream);
  if (e == hipSuccess)
    e = pnp::launch_seq_jacobian_gather(seq_mesh(), nf, seq_jl.p, onestep ? seq_jlt.p : nullptr,
                                        csr_rowptr.p, csr_col.p,
                                        seq_mask.p, csr_val.p, stream);
  if (e != hipSuccess) return hipfail(e, "seq jacobian");
  seq_jacobian_stored();  // the CSR view holds this Jacobian; the k-form matrix does not
  return PNP_OK;
}

double pnp_ctx::seq_dot(const double *a, const double *b, int &rc) {
  rc = PNP_OK;
  double h = 0;
  hipError_t e = pnp::launch_seq_dot(nseq(), a, b, seq_dotv.p, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, seq_dotv.p, 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) rc = hipfail(e, "seq dot");
  return h;
}

using pnp_ctx_t = pnp_ctx;

// host copy of kernels.h expand_k + mask_rows for the CSR export
static void expand_host(int pat, const double *K, unsigned dm, bool diag, double *B) {
  if (pat == pnp::kPatPnpFD) {
    pnp::expand_k<pnp::kPatPnpFD>(K, B);
    pnp::mask_rows<3, pnp::kPatPnpFD>(B, dm, diag);
  } else if (pat == pnp::kPatPnpIEFD) {
    pnp::expand_k<pnp::kPatPnpIEFD>(K, B);
    pnp::mask_rows<3, pnp::kPatPnpIEFD>(B, dm, diag);
  } else if (pat == pnp::kPatPnp) {
    pnp::expand_k<pnp::kPatPnp>(K, B);
    pnp::mask_rows<3, pnp::kPatPnp>(B, dm, diag);
  } else if (pat == pnp::kPatPnpIE) {
    pnp::expand_k<pnp::kPatPnpIE>(K, B);
    pnp::mask_rows<3, pnp::kPatPnpIE>(B, dm, diag);
  } else {
    pnp::expand_k<pnp::kPatScalar>(K, B);
    pnp::mask_rows<1, pnp::kPatScalar>(B, dm, diag);
  }
}

// ---------------------------------------------------------------------------------------------
// mesh / comm
// ---------------------------------------------------------------------------------------------
extern "C" int pnp_mesh_read_gmsh(const char *path, pnp_mesh_buf **out) {
  if (!path || !out) return PNP_E_ARG;
  auto mb = std::make_unique<pnp_mesh_buf>();
  std::string err;
  if (!pnp::read_gmsh(path, mb->m, err)) {
    g_err = err;
    return err.rfind("cannot open", 0) == 0 ? PNP_E_IO : PNP_E_MESH;
  }
  *out = mb.release();
  return PNP_OK;
}

static bool mesh_from_view(const pnp_mesh *in, pnp::Mesh &m, std::string &err) {
  if (!in || in->nv <= 0 || in->nt <= 0 || !in->coords || !in->tri || in->nbseg < 0 ||
      (in->nbseg > 0 && (!in->bseg || !in->bseg_group))) {
    err = "invalid pnp_mesh";
    return false;
  }
  m.nv = in->nv;
  m.nt = in->nt;
  m.nb = in->nbseg;
  m.xy.assign(in->coords, in->coords + 2 * size_t(in->nv));
  m.tri.assign(in->tri, in->tri + 3 * size_t(in->nt));
  m.bseg.assign(in->bseg, in->bseg + 2 * size_t(in->nbseg));
  m.bgroup.assign(in->bseg_group, in->bseg_group + size_t(in->nbseg));
  return pnp::validate(m, err);
}

extern "C" int pnp_mesh_refine(const pnp_mesh *in, int32_t k, pnp_mesh_buf **out) {
  if (!out || k < 0) return PNP_E_ARG;
  pnp::Mesh m;
  std::string err;
  if (!mesh_from_view(in, m, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  auto mb = std::make_unique<pnp_mesh_buf>();
  mb->m = pnp::refine(m, k);
  *out = mb.release();
  return PNP_OK;
}

extern "C" int pnp_mesh_from_geo(const char *path, double size_scale, pnp_mesh_buf **out) {
  if (!path || !out || !(size_scale > 0)) return PNP_E_ARG;
  pnp::GeoModel g;
  std::string err;
  if (!pnp::read_geo(path, g, err)) {
    g_err = err;
    return err.rfind("cannot open", 0) == 0 ? PNP_E_IO : PNP_E_MESH;
  }
  auto mb = std::make_unique<pnp_mesh_buf>();
  if (!pnp::mesh_geo(g, size_scale, mb->m, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  *out = mb.release();
  return PNP_OK;
}

extern "C" int pnp_mesh_write_gmsh(const pnp_mesh *in, const char *path) {
  if (!path) return PNP_E_ARG;
  pnp::Mesh m;
  std::string err;
  if (!mesh_from_view(in, m, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  if (!pnp::write_gmsh(path, m, err)) {
    g_err = err;
    return PNP_E_IO;
  }
  return PNP_OK;
}

extern "C" int pnp_mesh_view(const pnp_mesh_buf *mb, pnp_mesh *view) {
  if (!mb || !view) return PNP_E_ARG;
  view->nv = mb->m.nv;
  view->coords = mb->m.xy.data();
  view->nt = mb->m.nt;
  view->tri = mb->m.tri.data();
  view->nbseg = mb->m.nb;
  view->bseg = mb->m.bseg.data();
  view->bseg_group = mb->m.bgroup.data();
  return PNP_OK;
}

extern "C" void pnp_mesh_free(pnp_mesh_buf *m) { delete m; }

extern "C" const char *pnp_last_error(const pnp_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_err.c_str();
}

extern "C" int pnp_rccl_unique_id(void *out128) {
  if (!out128) return PNP_E_ARG;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) {
    g_err = "ncclGetUniqueId failed";
    return PNP_E_RCCL;
  }
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  std::memcpy(out128, &id, 128);
  return PNP_OK;
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
static void params_from(const pnp_params *pp, pnp::Params &P) {
  P.l_b = pp->l_b;
  P.c0 = pp->c0;
  P.tau = pp->tau;
  P.pi = pp->pi;
  P.cylindrical = pp->cylindrical;
  P.surf.resize(pp->n_surfaces);
  for (int i = 0; i < pp->n_surfaces; i++) {
    const pnp_surface &s = pp->surfaces[i];
    pnp::Surface &d = P.surf[i];
    d.cb = s.coulomb_btype;
    d.cflux = s.coulomb_flux;
    d.cpot = s.coulomb_potential;
    d.pb = s.plus_btype;
    d.pflux = s.plus_flux;
    d.pconc = s.plus_concentration;
    d.mb = s.minus_btype;
    d.mflux = s.minus_flux;
    d.mconc = s.minus_concentration;
  }
}

#define CK(expr, what)                                 \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return c->hipfail(e_, what); \
  } while (0)

extern "C" int pnp_create(const pnp_mesh *mesh, const pnp_params *params, int32_t device,
                          const pnp_comm *comm, pnp_ctx **out) {
  return pnp_create_pk(mesh, params, 1, device, comm, out);
}

// mesh, parameters, rank and the host front half (layout_derive.cc): nothing here needs a device,
// and every rank fails here alike, before any collective
int pnp_ctx::create_host(const pnp_mesh *mesh_in, const pnp_params *pp, int degree_in,
                         const pnp_comm *comm_in) {
  std::string e;
  if (!mesh_from_view(mesh_in, mesh, e)) return fail(PNP_E_MESH, e);
  for (int s = 0; s < mesh.nb; s++)
    if (mesh.bgroup[s] < 0 || mesh.bgroup[s] >= pp->n_surfaces)
      return fail(PNP_E_ARG, "boundary segment " + std::to_string(s) + " has physical group " +
                                 std::to_string(mesh.bgroup[s]) + " but only " +
                                 std::to_string(pp->n_surfaces) + " surfaces are configured");
  params_from(pp, params);
  if (comm_in && comm_in->size > 1) {
    rank = comm_in->rank;
    nranks = comm_in->size;
    if (comm_in->rank < 0 || comm_in->rank >= comm_in->size ||
        (!comm_in->rccl_unique_id && !comm_in->local_group && !comm_in->host))
      return fail(PNP_E_ARG,
                  "invalid pnp_comm (need an RCCL unique id, a local group or a host transport)");
  }
  degree = degree_in;
  if (!pnp::build_host_layout(mesh, degree, rank, nranks, tmesh, pks, fans, L, e))
    return fail(PNP_E_MESH, e);
  return PNP_OK;
}

int pnp_ctx::create_device(int device_in, const pnp_comm *comm_in) {
  device = device_in;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hipfail(e, "hipSetDevice");
  e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
  if (e != hipSuccess) return hipfail(e, "hipStreamCreate");
  if (comm_in && comm_in->rccl_unique_id && (nranks > 1 || comm_in->size == 1)) {
    ncclUniqueId id;
    std::memcpy(&id, comm_in->rccl_unique_id, sizeof id);
    ncclResult_t nr = ncclCommInitRank(&comm, nranks, id, rank);
    if (nr != ncclSuccess)
      return fail(PNP_E_RCCL, std::string("ncclCommInitRank failed: ") + ncclGetErrorString(nr) +
                                  " (" + ncclGetLastError(nullptr) + ")");
  }
  dist = nranks > 1 || comm != nullptr;
  return PNP_OK;
}

// every array of the layout and of its derived lists (layout_derive.h) to the device, each
// DevLayout pointer set beside its upload.  Lists that are "not usable" leave their pointers null
int pnp_ctx::upload_layout(const pnp::DerivedLayout &D, const pnp::LayoutKnobs &K) {
  const int nloc = L.n_owned + L.n_ghost;
  std::vector<double> xy(2 * size_t(nloc));
  for (int i = 0; i < nloc; i++) {
    xy[2 * size_t(i)] = mesh.xy[2 * size_t(L.l2g[i])];
    xy[2 * size_t(i) + 1] = mesh.xy[2 * size_t(L.l2g[i]) + 1];
  }
  int rc;
  auto up = [&](auto &buf, const auto &vec, auto &dlp, const char *what) {
    const int r = upload(buf, vec, what);
    dlp = buf.p;
    return r;
  };
  const pnp::SplitLayout &S = D.split;
  if ((rc = up(d_lperm, S.lperm, dl.lperm, "lperm")) || (rc = up(d_uperm, S.uperm, dl.uperm, "uperm")) ||
      (rc = up(d_lpinv, S.lpinv, dl.lpinv, "lpinv")) || (rc = up(d_upinv, S.upinv, dl.upinv, "upinv")) ||
      (rc = up(d_llen, S.llen, dl.llen, "llen")) || (rc = up(d_ulen, S.ulen, dl.ulen, "ulen")) ||
      (rc = up(d_ldl, S.ldl, dl.ldl, "ldl")))
    return rc;
  if ((rc = up(d_lchunk_len, S.lchunk_len, dl.lchunk_len, "lchunk_len")) ||
      (rc = up(d_lchunk_off, S.lchunk_off, dl.lchunk_off, "lchunk_off")) ||
      (rc = up(d_lcolidx, S.lcolidx, dl.lcolidx, "lcolidx")) || (rc = upload(d_lsrc, S.lsrc, "lsrc")) ||
      (rc = up(d_uchunk_len, S.uchunk_len, dl.uchunk_len, "uchunk_len")) ||
      (rc = up(d_uchunk_off, S.uchunk_off, dl.uchunk_off, "uchunk_off")) ||
      (rc = up(d_ucolidx, S.ucolidx, dl.ucolidx, "ucolidx")) || (rc = upload(d_usrc, S.usrc, "usrc")))
    return rc;
  if (const pnp::SweepLists &X = D.sweep; X.usable) {
    if ((rc = up(d_lsx_ptr, X.lptr, dl.lsx_ptr, "lsx ptr")) ||
        (rc = up(d_lsx_list, X.llist, dl.lsx_list, "lsx list")) ||
        (rc = up(d_lsx_idx, X.lidx, dl.lsx_idx, "lsx idx")) ||
        (rc = up(d_usx_ptr, X.uptr, dl.usx_ptr, "usx ptr")) ||
        (rc = up(d_usx_list, X.ulist, dl.usx_list, "usx list")) ||
        (rc = up(d_usx_idx, X.uidx, dl.usx_idx, "usx idx")))
      return rc;
    dl.sx_max = X.sx_max;
    ilu_flow[0].built = ilu_flow[1].built = false;
  }
  if ((rc = upload(d_rowoff, D.rows.rowoff, "rowoff")) || (rc = upload(d_rowcol, D.rows.rowcol, "rowcol")))
    return rc;
  if (!D.blkmap.empty() && (rc = up(d_blkmap, D.blkmap, dl.blkmap, "blkmap"))) return rc;
  fseg_group = D.flux.group;
  if ((rc = upload(d_fseg, D.flux.segs, "flux segments"))) return rc;
  if ((rc = up(d_chunk_len, L.chunk_len, dl.chunk_len, "chunk_len")) ||
      (rc = up(d_chunk_off, L.chunk_off, dl.chunk_off, "chunk_off")) ||
      (rc = up(d_colidx, L.colidx, dl.colidx, "colidx")) ||
      (rc = up(d_rowmeta, L.rowmeta, dl.rowmeta, "rowmeta")) || (rc = up(d_xy, xy, dl.xy, "xy")) ||
      (rc = upload(d_l2g, L.l2g, "l2g")) || (rc = upload(d_send_idx, L.send_idx, "send_idx")) ||
      (rc = up(d_color_idx, L.color_idx, dl.color_idx, "color_idx")) ||
      (rc = up(d_rowcolor, L.rowcolor, dl.rowcolor, "rowcolor")))
    return rc;
  dl.xcd_remap = K.xcd_remap;
  dl.n_owned = L.n_owned;
  dl.n_local = nloc;
  dl.nchunks = L.nchunks;
  dl.max_slots = L.chunk_len.empty() ? 0 : *std::max_element(L.chunk_len.begin(), L.chunk_len.end());
  dl.ncolors = int(L.color_ptr.size()) - 1;
  if (const pnp::SpmvLists &U = D.spmv; U.usable) {
    if ((rc = up(d_uptr, U.uptr, dl.uptr, "uptr")) || (rc = up(d_ulist, U.ulist, dl.ulist, "ulist")) ||
        (rc = up(d_lidx, U.lidx, dl.lidx, "lidx")) || (rc = up(d_uown, U.uown, dl.uown, "uown")))
      return rc;
    dl.umax = U.umax;
    dl.unmax = U.unmax;
  }
  if (dist && D.halo.usable) {  // halo-overlapped SpMV (sub_layout)
    if ((rc = upload(d_blk_int, D.halo.interior, "interior blocks")) ||
        (rc = upload(d_blk_bnd, D.halo.boundary, "boundary blocks")))
      return rc;
    n_blk_int = int(D.halo.interior.size());
    n_blk_bnd = int(D.halo.boundary.size());
    split_spmv = true;
  }
  return PNP_OK;
}

// the matrix values, the solver vectors and the scratch buffers, zeroed
int pnp_ctx::alloc_vectors() {
  const int nloc = L.n_owned + L.n_ghost;
  size_t nv3 = 3 * size_t(nloc);
  int rc;
  auto al = [&](auto &buf, size_t n, const char *what) -> int {
    hipError_t e2 = buf.alloc(n);  // zeroed, and the zeroing finished (DBuf::alloc)
    if (e2 != hipSuccess) return hipfail(e2, what);
    return PNP_OK;
  };
  if ((rc = al(vals, size_t(L.nslots) * 8, "vals")) ||
      (rc = al(lu, size_t(L.nslots) * 8, "lu")) ||
      (rc = al(lvals, d_lsrc.n * 8, "lvals")) || (rc = al(uvals, d_usrc.n * 8, "uvals")) ||
      (rc = al(tsgs, nv3, "sgs scratch")) || (rc = al(fluxx, nv3, "flux state")) ||
      (rc = al(fluxout, 2 * fseg_group.size() + 2, "flux out")) ||
      (rc = al(fluxred, 2 * 256, "flux reduce")) || (rc = al(x, nv3, "x")) ||
      (rc = al(r, nv3, "r")) || (rc = al(rs, nv3, "rs")) || (rc = al(z, nv3, "z")) || (rc = al(rt, nv3, "rt")) ||
      (rc = al(p, nv3, "p")) || (rc = al(v, nv3, "v")) || (rc = al(t, nv3, "t")) ||
      (rc = al(y, nv3, "y")) || (rc = al(y2, nv3, "y2")) ||
      (rc = al(ilu_y32buf, nv3, "ILU(0) intermediate")) || (rc = al(b, nv3, "b")) || (rc = al(prevu, nv3, "prevu")) ||
      (rc = al(ext, 3 * size_t(mesh.nv), "ext")) ||
      (rc = al(sendbuf, 3 * std::max<size_t>(1, L.send_idx.size()), "sendbuf")) ||
      // up to 3 partials per workgroup (SpMV mode 4) / 2 (updates with <rt, s>)
      (rc = al(partials,
               3 * std::max<size_t>(size_t(pnp::blas_nparts(3LL * nloc)),
                                    size_t(pnp::spmv_parts(L.n_owned))) + 64,
               "partials")) ||
      (rc = al(partials2,
               2 * std::max<size_t>(size_t(pnp::blas_nparts(3LL * nloc)),
                                    size_t(pnp::spmv_parts(L.n_owned))) + 64,
               "partials2")) ||
      (rc = al(S, 2, "scalars")) || (rc = al(redmw, pnp::kRedMwDoubles, "reduce ticket")) ||
      (rc = al(dmask, 3 * size_t(L.n_owned), "dmask")) ||
      (rc = al(rowflag, size_t(L.nchunks + 1) * pnp::kRows, "row flags")) ||
      (rc = al(cvec, 3 * size_t(L.n_owned), "cvec")) || (rc = al(aux0, nloc, "aux0")) ||
      (rc = al(aux1, nloc, "aux1")))
    return rc;
  hipError_t e = hipHostMalloc(&hS, 3 * sizeof(pnp::Scalars));
  if (e != hipSuccess) return hipfail(e, "hipHostMalloc");
  return PNP_OK;
}

// the RCCL halo of the overlapped SpMV runs on a stream of its own
int pnp_ctx::create_halo_stream(const pnp_comm *comm_in) {
  if (!split_spmv || !comm_in->rccl_unique_id) return PNP_OK;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&ev_ready, hipEventDisableTiming)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&ev_halo, hipEventDisableTiming)) != hipSuccess)
    return hipfail(e, "halo stream");
  return PNP_OK;
}

int pnp_ctx::create_host_transport(const pnp_comm *comm_in) {
  if (!(nranks > 1 && !comm_in->rccl_unique_id && !comm_in->local_group)) return PNP_OK;
  if (!comm_in->host->exchange || !comm_in->host->allreduce_sum)
    return fail(PNP_E_ARG, "pnp_host_transport: exchange and allreduce_sum are required");
  ht = *comm_in->host;
  const size_t ns = 3 * std::max<size_t>(1, L.send_idx.size());
  const size_t nr = 3 * std::max<size_t>(1, size_t(L.n_ghost));
  hipError_t e;
  if ((e = hipHostMalloc(&h_send, sizeof(double) * ns)) != hipSuccess ||
      (e = hipHostMalloc(&h_recv, sizeof(double) * nr)) != hipSuccess)
    return hipfail(e, "host transport staging");
  return PNP_OK;
}

// join the in-process group; the barrier: all ranks created before any collective
int pnp_ctx::join_local_group(const pnp_comm *comm_in) {
  if (!(nranks > 1 && !comm_in->rccl_unique_id && comm_in->local_group)) return PNP_OK;
  std::shared_ptr<LocalGroup> g;
  {
    std::lock_guard<std::mutex> lk(g_groups_m);
    auto &slot = g_groups[comm_in->local_group];
    if (!slot || slot->size != nranks) {
      slot = std::make_shared<LocalGroup>();
      slot->size = nranks;
      slot->members.assign(nranks, nullptr);
      slot->host.assign(nranks, {});
    }
    g = slot;
    if (g->members[rank]) return fail(PNP_E_ARG, "rank already present in local group");
    g->members[rank] = this;
  }
  lg = g;
  g->barrier();
  return PNP_OK;
}

// The steps of pnp_create_pk after its argument checks.  Everything up to create_device fails on
// every rank alike before ncclCommInitRank; everything before join_local_group before its barrier
int pnp_ctx::create(const pnp_mesh *mesh_in, const pnp_params *pp, int degree_in, int device_in,
                    const pnp_comm *comm_in) {
  int rc;
  if ((rc = create_host(mesh_in, pp, degree_in, comm_in)) || (rc = create_device(device_in, comm_in)))
    return rc;
  const pnp::LayoutKnobs knobs = pnp::LayoutKnobs::from_env();
  pnp::DerivedLayout D;
  std::string e;
  if (!pnp::derive_layout(mesh, L, knobs, D, e)) return fail(PNP_E_MESH, e);
  if ((rc = upload_layout(D, knobs)) || (rc = alloc_vectors()) || (rc = create_halo_stream(comm_in)))
    return rc;
  hl = pnp::keep_layout(std::move(D));
  if (degree > 1 && (rc = pk_build())) return rc;
  if ((rc = create_host_transport(comm_in))) return rc;
  return join_local_group(comm_in);
}

extern "C" int pnp_create_pk(const pnp_mesh *mesh, const pnp_params *params, int32_t degree,
                             int32_t device, const pnp_comm *comm, pnp_ctx **out) {
  if (degree < 1 || degree > 3) {
    g_err = "pnp_create_pk: degree must be 1, 2 or 3 (PDEGREE)";
    return PNP_E_ARG;
  }
  if (!mesh || !params || !out) {
    g_err = "pnp_create: null argument";
    return PNP_E_ARG;
  }
  if (params->n_surfaces < 0 || (params->n_surfaces > 0 && !params->surfaces)) {
    g_err = "pnp_create: invalid surfaces";
    return PNP_E_ARG;
  }
  auto c = std::make_unique<pnp_ctx>();
  if (int rc = c->create(mesh, params, degree, device, comm)) {
    g_err = c->err;
    return rc;
  }
  *out = c.release();
  return PNP_OK;
}


extern "C" void pnp_destroy(pnp_ctx *ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  if (ctx->lg) {
    std::lock_guard<std::mutex> lk(g_groups_m);
    ctx->lg->members[ctx->rank] = nullptr;
  }
  delete ctx;
}

extern "C" int pnp_get_info(pnp_ctx *c, pnp_info *info) {
  if (!c || !info) return PNP_E_ARG;
  std::memset(info, 0, sizeof *info);
  info->nv_global = c->mesh.nv;
  info->nv_owned = c->L.n_owned;
  info->nv_ghost = c->L.n_ghost;
  info->nfields = c->nf;
  info->ncolors = int(c->L.color_ptr.size()) - 1;
  info->nchunks = c->L.nchunks;
  info->max_slots = c->fans.max_slots;
  info->nranks = c->nranks;
  info->nblocks = c->L.nblocks;
  info->nnz_reduced = c->L.nblocks * (c->nvb ? c->nvb : 1);
  info->nslots = c->L.nslots;
  info->nks = c->nks;
  info->nvb = c->nvb;
  info->lslots = (int64_t)c->d_lsrc.n;
  info->uslots = (int64_t)c->d_usrc.n;
  info->ilu_f32 = c->ilu_f32;
  info->degree = c->degree;
  info->color_conflicts = c->L.conflicts;
  info->transport = c->comm ? 2 : c->lg ? 1 : c->host_tr() ? 3 : 0;
  info->nat_flow_applies = c->nat_flow_n;
  info->nat_level_applies = c->nat_level_n;
  info->ilu_flow_applies = c->ilu_flow_n;
  info->lslots_live = c->hl.lslots_live;
  info->uslots_live = c->hl.uslots_live;
  info->lsx_entries = (int64_t)c->hl.lsx_list.size();
  info->usx_entries = (int64_t)c->hl.usx_list.size();
  info->pk_split_short = c->pkd.n_short;
  info->pk_split_long = c->pkd.n_long;
  info->pk_split_len = c->pkd.short_len;
  size_t b = 0;
  b += c->vals.n * 8 + (c->x.n + c->r.n + c->rs.n + c->z.n + c->rt.n + c->p.n + c->v.n + c->t.n + c->y.n +
                        c->y2.n + c->b.n + c->prevu.n + c->ext.n) * 8 + c->ilu_y32buf.n * 4;
  b += c->d_colidx.n * 4 + c->d_rowmeta.n * 8 + c->d_xy.n * 8;
  b += (c->mf_x.n + c->mf_r.n + c->mf_diag.n) * 8 + c->mf_choff.n * 4;  // PNP_OPT_MATRIX_FREE
  info->device_bytes = int64_t(b);
  return PNP_OK;
}

// ---------------------------------------------------------------------------------------------
// operators
// ---------------------------------------------------------------------------------------------
extern "C" int pnp_nfields(pnp_ctx *c) { return c ? c->nf : PNP_E_ARG; }

// the part of an operator that depends on the mesh and the parameters only: the Dirichlet mask
// (mask: every node, global order; lmask: owned rows) and the constant load (the Neumann flux of
// alpha_boundary, times dt for PnpTOperator) on the owned rows.  nf fields as `kind` has them.
void pnp_ctx::op_static(int k, int field, double dt, std::vector<uint8_t> &mask,
                        std::vector<uint8_t> &lmask, std::vector<double> &lload) const {
  const int nfk = nfields_of(k);
  const int field0 = (k == PNP_OP_DIFF || k == PNP_OP_DIFF_IMPLICIT_EULER) ? field : 0;
  if (degree > 1)
    pnp::pk_dirichlet_mask(tmesh, pks, params, nfk, field0, mask);
  else
    pnp::dirichlet_mask(mesh, params, nfk, field0, mask);
  std::vector<double> load(size_t(mesh.nv) * nfk, 0.0);
  if (k == PNP_OP_PNP || k == PNP_OP_PNP_IMPLICIT_EULER || k == PNP_OP_PB || k == PNP_OP_POISSON) {
    if (degree > 1)
      pnp::pk_neumann_load(tmesh, pks, params, nfk, 0, load);
    else
      pnp::neumann_load(mesh, params, nfk, 0, load);
    if (k == PNP_OP_PNP_IMPLICIT_EULER)
      for (auto &v : load) v *= dt;
  }
  lmask.resize(size_t(L.n_owned) * nfk);
  lload.resize(size_t(L.n_owned) * nfk);
  for (int i = 0; i < L.n_owned; i++)
    for (int f = 0; f < nfk; f++) {
      lmask[size_t(i) * nfk + f] = mask[size_t(L.l2g[i]) * nfk + f];
      lload[size_t(i) * nfk + f] = load[size_t(L.l2g[i]) * nfk + f];
    }
}

// a row's mask bits, and whether its load is to be read: every row of an implicit-Euler operator,
// else any load entry that is not bitwise +0.0 (-0.0 too), and any such entry of the caller's
// c_extra (external layout, or null) whatever the sum came to
std::vector<uint8_t> pnp_ctx::row_flags(int nfk, bool ie, const std::vector<uint8_t> &lmask,
                                        const std::vector<double> &lload,
                                        const double *c_extra) const {
  std::vector<uint8_t> flag(rowflag.n, 0);
  for (int i = 0; i < L.n_owned; i++) {
    unsigned fl = ie ? pnp::kRowFlagLoad : 0;
    for (int f = 0; f < nfk; f++) {
      if (lmask[size_t(i) * nfk + f]) fl |= 1u << f;
      uint64_t bits;
      std::memcpy(&bits, &lload[size_t(i) * nfk + f], sizeof bits);
      if (bits) fl |= pnp::kRowFlagLoad;
      if (c_extra) {
        std::memcpy(&bits, &c_extra[size_t(f) * mesh.nv + L.l2g[i]], sizeof bits);
        if (bits) fl |= pnp::kRowFlagLoad;
      }
    }
    flag[i] = uint8_t(fl);
  }
  return flag;
}

int pnp_ctx::op_activate(int k, double dt, double z) {
  kind = k;
  fd_mode = false;  // the next Jacobian picks its form (set_fd)
  nf = nfields_of(k);
  pat = base_pat(k);
  nvb = pnp::popc9(pat);
  nks = pnp::nks_of(pat);
  jacobian_drop();
  // a captured matrix-free application holds the operator's scalar arguments (dt, valency, ...) by
  // value, which the graph key does not see
  if (mf_opt || pk_mf_opt) graphs_clear();
  // SELL padding slots point at the row itself and are never written by the assembly, so they
  // must hold zeros in the k-form layout of THIS operator (the SpMV multiplies them)
  vals_const_valid = false;
  hipError_t e = hipMemsetAsync(vals.p, 0, sizeof(double) * size_t(L.nslots) * nks, stream);
  if (e != hipSuccess) return hipfail(e, "clear matrix");
  seq_op_valid = false;
  seq_dt = dt;
  seq_z = z;
  dl.dmask = dmask.p;
  aa = pnp::AsmArgs{};
  aa.kind = k;  // PNP_OP_* == pnp::OP_* by construction
  aa.l_b = params.l_b;
  aa.c0 = params.c0;
  aa.tau = params.tau;
  aa.pi = params.pi;
  aa.dt = dt;
  aa.z = z;
  aa.cylindrical = params.cylindrical;
  aa.aux0 = aux0.p;
  aa.aux1 = aux1.p;
  aa.cvec = cvec.p;
  aa.dmask = dmask.p;
  aa.rowflag = rowflag.p;
  aa.vals = vals.p;
  return PNP_OK;
}

extern "C" int pnp_set_operator(pnp_ctx *c, const pnp_op_args *a) {
  if (!c || !a) return PNP_E_ARG;
  // no graphs_clear() here: the operator's pattern and mask pointer are in the graph key; a change
  // of the CSR view's pattern (SSOR_NATURAL, pnp_jacobian_csr_device) clears the graphs in
  // csr_structure(), which rebuilds the buffers they captured
  if (a->kind < PNP_OP_PNP || a->kind > PNP_OP_POISSON)
    return c->fail(PNP_E_ARG, "unknown operator kind");
  hipSetDevice(c->device);
  int kind = a->kind;
  const bool ie = kind == PNP_OP_PNP_IMPLICIT_EULER || kind == PNP_OP_DIFF_IMPLICIT_EULER;
  if (ie && !(a->dt > 0)) return c->fail(PNP_E_ARG, "implicit Euler needs dt > 0");
  if (ie && !a->x_old) return c->fail(PNP_E_ARG, "implicit Euler needs x_old");
  if ((kind == PNP_OP_DIFF || kind == PNP_OP_DIFF_IMPLICIT_EULER) &&
      (!a->phi || (a->field != 1 && a->field != 2)))
    return c->fail(PNP_E_ARG, "diffusion operator needs phi and field 1 or 2");
  if (kind == PNP_OP_POISSON && (!a->cp || !a->cm))
    return c->fail(PNP_E_ARG, "Poisson operator needs cp and cm");
  if (c->degree > 1 && (kind == PNP_OP_PNP || kind == PNP_OP_PNP_IMPLICIT_EULER))
    return c->fail(PNP_E_ARG,
                   "PnpOperator / PnpTOperator are P1 in the reference (Pk2DLocalFiniteElementMap<..., 1>, "
                   "src/stationary_pnp_from_pb.hh:206-208); P_k contexts take PB, Poisson and diffusion");
  int rc;
  if ((rc = c->op_activate(kind, a->dt, a->z))) return rc;
  const pnp::Mesh &m = c->mesh;
  const pnp::LocalLayout &L = c->L;
  int nf = c->nf;
  // Dirichlet mask and constant load (Neumann flux of alpha_boundary), owned rows
  std::vector<uint8_t> mask, lmask;
  std::vector<double> lload;
  c->op_static(kind, a->field, a->dt, mask, lmask, lload);
  if (a->c_extra)
    for (int i = 0; i < L.n_owned; i++)
      for (int f = 0; f < nf; f++)
        lload[size_t(i) * nf + f] += a->c_extra[size_t(f) * m.nv + L.l2g[i]];
  CK(hipMemcpy(c->dmask.p, lmask.data(), lmask.size(), hipMemcpyHostToDevice), "dmask");
  {  // (implicit Euler: every row's load is read, the device mass kernel rewrites cvec below)
    const std::vector<uint8_t> flag = c->row_flags(nf, ie, lmask, lload, a->c_extra);
    CK(hipMemcpy(c->rowflag.p, flag.data(), flag.size(), hipMemcpyHostToDevice), "row flags");
    c->hrowflag.assign(flag.begin(), flag.begin() + L.n_owned);
  }
  // the reference-order mode's copies (external layout, global vertex order)
  c->seq_cextra = a->c_extra != nullptr;
  c->seq_mask_h.assign(size_t(nf) * m.nv, 0);
  if (c->degree == 1)
    for (int g = 0; g < m.nv; g++)
      for (int f = 0; f < nf; f++) c->seq_mask_h[size_t(f) * m.nv + g] = mask[size_t(g) * nf + f];
  auto hcopy = [&](const double *h, size_t cnt, std::vector<double> &out) {
    if (h) out.assign(h, h + cnt); else out.clear();
  };
  const bool dk = kind == PNP_OP_DIFF || kind == PNP_OP_DIFF_IMPLICIT_EULER;
  hcopy(dk ? a->phi : nullptr, m.nv, c->seq_phi_h);
  hcopy(kind == PNP_OP_POISSON ? a->cp : nullptr, m.nv, c->seq_cp_h);
  hcopy(kind == PNP_OP_POISSON ? a->cm : nullptr, m.nv, c->seq_cm_h);
  hcopy(ie ? a->x_old : nullptr, size_t(nf) * m.nv, c->seq_xold_h);
  c->hmask = lmask;
  CK(hipMemcpy(c->cvec.p, lload.data(), sizeof(double) * lload.size(), hipMemcpyHostToDevice),
     "cvec");
  int nloc = L.n_owned + L.n_ghost;
  auto up_field = [&](const double *h, double *d) -> int {
    std::vector<double> tmp(nloc);
    for (int i = 0; i < nloc; i++) tmp[i] = h[L.l2g[i]];
    hipError_t e = hipMemcpy(d, tmp.data(), sizeof(double) * nloc, hipMemcpyHostToDevice);
    return e == hipSuccess ? PNP_OK : c->hipfail(e, "aux upload");
  };
  if (kind == PNP_OP_DIFF || kind == PNP_OP_DIFF_IMPLICIT_EULER)
    if ((rc = up_field(a->phi, c->aux0.p))) return rc;
  if (kind == PNP_OP_POISSON)
    if ((rc = up_field(a->cp, c->aux0.p)) || (rc = up_field(a->cm, c->aux1.p))) return rc;
  if (ie) {  // cvec -= M(x_old), rows of this rank (x_old with ghosts)
    if ((rc = c->upload_ext(a->x_old, nf, c->prevu.p, true))) return rc;
    int k = kind == PNP_OP_PNP_IMPLICIT_EULER ? pnp::OP_PNP_IE : pnp::OP_DIFF_IE;
    if (c->degree > 1)
      CK(pnp::launch_pk_mass_apply(c->dl, c->pkd, c->prevu.p, c->cvec.p, c->stream), "mass apply");
    else
      CK(pnp::launch_mass_apply(c->dl, k, c->params.tau, c->params.pi, c->params.cylindrical,
                                c->prevu.p, c->cvec.p, c->stream),
         "mass apply");
    CK(hipStreamSynchronize(c->stream), "mass apply");
  }
  return PNP_OK;
}

// reference-order mode: an external-layout vector of the caller's (host, or dev: device) into /
// out of one of the mode's device vectors, on the stream
static hipError_t seq_in(pnp_ctx *c, double *dst, const double *src, bool dev) {
  return hipMemcpyAsync(dst, src, 8 * size_t(c->nseq()),
                        dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
}
static hipError_t seq_out(pnp_ctx *c, double *dst, const double *src, bool dev) {
  return hipMemcpyAsync(dst, src, 8 * size_t(c->nseq()),
                        dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream);
}

static int seq_residual_abi(pnp_ctx *c, const double *x, double *r, bool dev) {
  int rc;
  if ((rc = c->seq_build())) return rc;
  double *sx = c->sq(pnp_ctx::SQ_X), *sr = c->sq(pnp_ctx::SQ_R);
  CK(seq_in(c, sx, x, dev), "seq upload");
  if ((rc = c->seq_residual(sx, sr))) return rc;
  CK(seq_out(c, r, sr, dev), "seq download");
  CK(hipStreamSynchronize(c->stream), "seq residual");
  return PNP_OK;
}
static int seq_jacobian_abi(pnp_ctx *c, const double *x, bool dev, bool fd) {
  int rc;
  if ((rc = c->seq_build())) return rc;
  double *sx = c->sq(pnp_ctx::SQ_X);
  CK(seq_in(c, sx, x, dev), "seq upload");
  if ((rc = c->seq_jacobian(sx, fd))) return rc;
  CK(hipStreamSynchronize(c->stream), "seq jacobian");
  return PNP_OK;
}

extern "C" int pnp_residual(pnp_ctx *c, const double *x, double *r) {
  return pnp_residual_ex(c, x, r, 0);
}

extern "C" int pnp_jacobian(pnp_ctx *c, const double *x) { return pnp_jacobian_ex(c, x, 0); }

extern "C" int pnp_jacobian_export(pnp_ctx *c, int64_t *nnz, int32_t *rowptr, int32_t *col,
                                   double *val) {
  if (!c || !nnz) return PNP_E_ARG;
  if (!c->assembled) return c->fail(PNP_E_STATE, "no Jacobian assembled");
  if (c->seq_on()) {  // the reference-order Jacobian lives in the CSR view
    *nnz = c->csr_nnz;
    if (!rowptr || !col || !val) return PNP_OK;
    const size_t n = c->nseq();
    CK(hipMemcpy(rowptr, c->csr_rowptr.p, 4 * (n + 1), hipMemcpyDeviceToHost), "export");
    CK(hipMemcpy(col, c->csr_col.p, 4 * size_t(c->csr_nnz), hipMemcpyDeviceToHost), "export");
    CK(hipMemcpy(val, c->csr_val.p, 8 * size_t(c->csr_nnz), hipMemcpyDeviceToHost), "export");
    return PNP_OK;
  }
  const pnp::LocalLayout &L = c->L;
  int nf = c->nf, NV = c->nvb, nv = c->mesh.nv;
  long long total = 0;
  for (int i = 0; i < L.n_owned; i++) total += (long long)pnp::meta_len(L.rowmeta[i]);
  total *= NV;
  *nnz = total;
  if (!rowptr || !col || !val) return PNP_OK;
  hipSetDevice(c->device);
  if (int rc = c->ensure_values()) return rc;  // a matrix-free Jacobian: assemble its values now
  CK(hipStreamSynchronize(c->stream), "export");
  const int NKS = c->nks;
  std::vector<double> hv(size_t(L.nslots) * NKS);
  CK(hipMemcpy(hv.data(), c->vals.p, sizeof(double) * hv.size(), hipMemcpyDeviceToHost), "export");
  // rows of the external layout: f*nv + g ; count per row
  int n = nf * nv;
  std::vector<int> cnt(n + 1, 0);
  for (int i = 0; i < L.n_owned; i++) {
    int len = pnp::meta_len(L.rowmeta[i]);
    for (int f = 0; f < nf; f++) {
      int k = 0;
      for (int g = 0; g < nf; g++) k += pnp::pat_index(c->pat, f, g) >= 0;
      cnt[f * nv + L.l2g[i] + 1] += k * len;
    }
  }
  for (int i = 0; i < n; i++) cnt[i + 1] += cnt[i];
  std::vector<int> fill(n, 0);
  std::vector<std::pair<int, double>> tmp;
  for (int i = 0; i < L.n_owned; i++) {
    int chunk = i / pnp::kRows, lane = i % pnp::kRows;
    int len = pnp::meta_len(L.rowmeta[i]);
    for (int f = 0; f < nf; f++) {
      int R = f * nv + L.l2g[i];
      tmp.clear();
      unsigned dm = 0;
      for (int g = 0; g < nf; g++) dm |= unsigned(c->hmask[size_t(i) * nf + g] != 0) << g;
      for (int s = 0; s < len; s++) {
        int j = L.colidx[size_t(L.chunk_off[chunk]) + size_t(s) * pnp::kRows + lane];
        double K[9], B[9];
        for (int q = 0; q < NKS; q++)
          K[q] = hv[(size_t(L.chunk_off[chunk]) + size_t(s) * pnp::kRows) * NKS +
                    pnp::vin(NKS, q, lane)];
        expand_host(c->pat, K, dm, s == 0, B);
        for (int g = 0; g < nf; g++) {
          int v = pnp::pat_index(c->pat, f, g);
          if (v < 0) continue;
          tmp.push_back({g * nv + L.l2g[j], B[v]});
        }
      }
      std::sort(tmp.begin(), tmp.end());
      for (auto &pr : tmp) {
        col[cnt[R] + fill[R]] = pr.first;
        val[cnt[R] + fill[R]] = pr.second;
        fill[R]++;
      }
    }
  }
  for (int i = 0; i <= n; i++) rowptr[i] = cnt[i];
  return PNP_OK;
}

// ---------------------------------------------------------------------------------------------
// flags / device pointers / FD Jacobian / jacobian_apply / device CSR view
// ---------------------------------------------------------------------------------------------
static int check_flags(pnp_ctx *c, int32_t flags, int32_t allowed) {
  if (flags & ~allowed) return c->fail(PNP_E_ARG, "unsupported flags for this call");
  return PNP_OK;
}

extern "C" int pnp_residual_ex(pnp_ctx *c, const double *x, double *r, int32_t flags) {
  if (!c || !x || !r) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set");
  int rc;
  if ((rc = check_flags(c, flags, PNP_DEVICE_PTRS))) return rc;
  hipSetDevice(c->device);
  const bool dev = flags & PNP_DEVICE_PTRS;
  if (c->seq_on()) return seq_residual_abi(c, x, r, dev);
  if ((rc = c->upload_ext(x, c->nf, c->x.p, true, dev))) return rc;
  if ((rc = c->assemble(c->x.p, 0))) return rc;
  return c->download_ext(c->r.p, c->nf, r, dev);
}

extern "C" int pnp_jacobian_ex(pnp_ctx *c, const double *x, int32_t flags) {
  if (!c || !x) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set");
  int rc;
  if ((rc = check_flags(c, flags, PNP_DEVICE_PTRS | PNP_JAC_FD))) return rc;
  hipSetDevice(c->device);
  if (c->seq_on())
    return seq_jacobian_abi(c, x, flags & PNP_DEVICE_PTRS, c->fd_opt || (flags & PNP_JAC_FD));
  if ((rc = c->upload_ext(x, c->nf, c->x.p, true, flags & PNP_DEVICE_PTRS))) return rc;
  const int keep = c->fd_opt;
  if (flags & PNP_JAC_FD) c->fd_opt = 1;
  rc = c->assemble(c->x.p, 1);
  c->fd_opt = keep;
  if (rc) return rc;
  CK(hipStreamSynchronize(c->stream), "jacobian");
  return PNP_OK;
}

extern "C" int pnp_jacobian_apply(pnp_ctx *c, const double *x, const double *z, double *y,
                                  int32_t flags) {
  if (!c || !z || !y) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set");
  int rc;
  if ((rc = check_flags(c, flags, PNP_DEVICE_PTRS | PNP_JAC_FD))) return rc;
  hipSetDevice(c->device);
  const bool dev = flags & PNP_DEVICE_PTRS;
  if (x) {
    if ((rc = pnp_jacobian_ex(c, x, flags))) return rc;
  } else if (!c->assembled) {
    return c->fail(PNP_E_STATE, "no Jacobian assembled (pass x)");
  }
  if (c->seq_on()) {  // y = A z in BCRSMatrix::mv's order on the CSR view
    double *sz = c->sq(pnp_ctx::SQ_Z), *sy = c->sq(pnp_ctx::SQ_Y);
    CK(seq_in(c, sz, z, dev), "seq upload");
    CK(pnp::launch_seq_spmv(c->nseq(), c->csr_rowptr.p, c->csr_col.p, c->csr_val.p, sz, sy,
                            c->stream),
       "seq apply");
    CK(seq_out(c, y, sy, dev), "seq download");
    CK(hipStreamSynchronize(c->stream), "seq apply");
    return PNP_OK;
  }
  // z with ghosts (the halo of a global vector is local: every rank holds it), y = A z
  if ((rc = c->upload_ext(z, c->nf, c->y.p, true, dev))) return rc;
  int nsp = 0;
  if (c->mf_lin) c->mf_applies++;
  CK(c->apply_op(c->dl, c->y.p, c->t.p, 0, nullptr, c->partials.p, &nsp, c->stream),
     "jacobian apply");
  return c->download_ext(c->t.p, c->nf, y, dev);
}

static int seq_solve_abi(pnp_ctx *c, const double *rhs, double *z, const pnp_solve_opts &o,
                         pnp_solve_result &res, bool dev) {
  int rc;
  c->gm_history.clear();
  if ((rc = c->seq_build())) return rc;
  const size_t n = c->nseq();
  double *sb = c->sq(pnp_ctx::SQ_B), *sz = c->sq(pnp_ctx::SQ_Z);
  CK(seq_in(c, sb, rhs, dev), "seq upload");
  CK(hipMemsetAsync(sz, 0, 8 * n, c->stream), "seq upload");
  if ((rc = c->seq_krylov(o, sz, sb, res))) return rc;
  CK(seq_out(c, z, sz, dev), "seq download");
  CK(hipStreamSynchronize(c->stream), "seq solve");
  return res.breakdown ? PNP_E_BREAKDOWN : PNP_OK;
}

extern "C" int pnp_linear_solve_ex(pnp_ctx *c, const double *rhs, double *z,
                                   const pnp_solve_opts *o, pnp_solve_result *res, int32_t flags) {
  if (!c || !rhs || !z || !o || !res) return PNP_E_ARG;
  int rc;
  if ((rc = check_flags(c, flags, PNP_DEVICE_PTRS))) return rc;
  hipSetDevice(c->device);
  std::memset(res, 0, sizeof *res);
  const bool dev = flags & PNP_DEVICE_PTRS;
  if (c->seq_on()) return seq_solve_abi(c, rhs, z, *o, *res, dev);
  if ((rc = c->upload_ext(rhs, c->nf, c->b.p, false, dev))) return rc;
  if ((rc = c->krylov(c->b.p, c->z.p, *o, *res))) return rc;
  if ((rc = c->download_ext(c->z.p, c->nf, z, dev))) return rc;
  return res->breakdown ? PNP_E_BREAKDOWN : PNP_OK;
}

extern "C" int pnp_solve_history(pnp_ctx *c, double *defects, int32_t cap, int32_t *n) {
  if (!c || !n || cap < 0 || (cap > 0 && !defects)) return PNP_E_ARG;
  *n = int32_t(c->gm_history.size());
  for (int32_t k = 0; k < cap && k < *n; k++) defects[k] = c->gm_history[size_t(k)];
  return PNP_OK;
}

extern "C" int pnp_jacobian_csr_device(pnp_ctx *c, pnp_csr_view *out) {
  if (!c || !out) return PNP_E_ARG;
  if (!c->assembled) return c->fail(PNP_E_STATE, "no Jacobian assembled");
  hipSetDevice(c->device);
  int rc;
  if ((rc = c->csr_values())) return rc;
  CK(hipStreamSynchronize(c->stream), "csr fill");
  out->n = c->nf * c->mesh.nv;
  out->nnz = c->csr_nnz;
  out->rowptr = c->csr_rowptr.p;
  out->col = c->csr_col.p;
  out->val = c->csr_val.p;
  return PNP_OK;
}

// ---------------------------------------------------------------------------------------------
// solves
// ---------------------------------------------------------------------------------------------
extern "C" int pnp_linear_solve(pnp_ctx *c, const double *rhs, double *z, const pnp_solve_opts *o,
                                pnp_solve_result *res) {
  return pnp_linear_solve_ex(c, rhs, z, o, res, 0);
}

extern "C" int pnp_prec_apply(pnp_ctx *c, int32_t prec, const double *d, double *v) {
  if (!c || !d || !v || prec < PNP_PREC_NONE || prec > PNP_PREC_CHEBYSHEV) return PNP_E_ARG;
  if (!c->assembled) return c->fail(PNP_E_STATE, "no Jacobian assembled");
  hipSetDevice(c->device);
  int rc;
  if (c->seq_on()) {
    if (prec != PNP_PREC_NONE && prec != PNP_PREC_JACOBI && prec != PNP_PREC_SSOR_NATURAL)
      return c->fail(PNP_E_ARG, "PNP_OPT_SEQ_ORDER: preconditioner must be NONE, JACOBI or SSOR_NATURAL");
    const size_t n = c->nseq();
    double *sb = c->sq(pnp_ctx::SQ_B), *sz = c->sq(pnp_ctx::SQ_Z);
    CK(seq_in(c, sb, d, false), "seq upload");
    CK(hipMemsetAsync(sz, 0, 8 * n, c->stream), "seq upload");
    if ((rc = c->seq_prec(prec, sb, sz))) return rc;
    if (prec == PNP_PREC_SSOR_NATURAL && (rc = c->nat_check())) return rc;
    CK(seq_out(c, v, sz, false), "seq download");
    CK(hipStreamSynchronize(c->stream), "seq prec");
    return PNP_OK;
  }
  if ((rc = c->upload_ext(d, c->nf, c->b.p, false))) return rc;
  if ((rc = c->precond(prec, c->b.p, c->z.p))) return rc;
  if ((rc = c->solve_checks(prec))) return rc;
  return c->download_ext(c->z.p, c->nf, v);
}

// ---- context options: one row per PNP_OPT_*, read by pnp_set_option and pnp_get_option ----------
// on_set runs with the accepted value before it is stored; an error from it leaves the option as
// it was
static int opt_ilu_f32(pnp_ctx *c, int old, int now) {
  // not ilu_factors_drop(): the precision is that of the split copy alone, the fp64 factors in lu
  // survive and split(2) converts them again (the fused path, which keeps none, refactorises)
  if (old != now && c->split_of == 2) c->split_of = 0;
  return PNP_OK;
}
static int opt_ilu_fused(pnp_ctx *c, int, int) {
  c->ilu_factors_drop();
  return PNP_OK;
}
static int opt_gmres_restart(pnp_ctx *c, int old, int now) {
  if (old == now) return PNP_OK;
  hipSetDevice(c->device);
  c->gmres_free();
  return PNP_OK;
}
static int opt_idr_s(pnp_ctx *c, int old, int now) {
  if (old == now) return PNP_OK;
  hipSetDevice(c->device);
  c->idr_free();
  return PNP_OK;
}
static int opt_seq_order(pnp_ctx *c, int old, int now) {
  if (now && (c->degree > 1 || c->dist))
    return c->fail(PNP_E_ARG, "PNP_OPT_SEQ_ORDER: P1 contexts of one rank only");
  if (old != now) c->jacobian_drop();  // the next Jacobian is assembled in the newly selected form
  return PNP_OK;
}
static int opt_matrix_free(pnp_ctx *c, int, int now) {
  if (now && c->degree > 1)
    return c->fail(PNP_E_STATE,
                   "PNP_OPT_MATRIX_FREE: P1 contexts only (the option selects the P1 fan walk; a "
                   "P_k context takes pnp_pk_matfree_set)");
  if (!now && c->mf_lin) {
    hipSetDevice(c->device);
    if (int rc = c->mf_settle()) return rc;
  }
  // the graphs_clear() at the top of pnp_set_option has dropped every captured BiCGSTAB graph
  // and bumped graph_epoch: no graph captured in one form survives into the other, and none
  // outlives an operator change made while the option was off (pnp_set_operator clears only
  // while it is on)
  return PNP_OK;
}

static const struct OptRow {
  int id;
  const char *name;
  int lo, hi;
  int pnp_ctx::*field;
  int (*on_set)(pnp_ctx *, int old, int now);
} kOptions[] = {
    {PNP_OPT_GRAPH, "PNP_OPT_GRAPH", -1, 1, &pnp_ctx::graph_opt, nullptr},
    {PNP_OPT_ILU_F32, "PNP_OPT_ILU_F32", 0, 3, &pnp_ctx::ilu_f32, opt_ilu_f32},
    {PNP_OPT_ILU_FLOW, "PNP_OPT_ILU_FLOW", 0, 2, &pnp_ctx::ilu_flow_opt, nullptr},
    {PNP_OPT_NAT_FLOW, "PNP_OPT_NAT_FLOW", -1, 1, &pnp_ctx::nat_flow_opt, nullptr},
    {PNP_OPT_AMG_FALLBACK, "PNP_OPT_AMG_FALLBACK", 0, 1, &pnp_ctx::amg_fallback, nullptr},
    {PNP_OPT_ILU_RETRY, "PNP_OPT_ILU_RETRY", 0, 1, &pnp_ctx::ilu_retry, nullptr},
    {PNP_OPT_GMRES_RESTART, "PNP_OPT_GMRES_RESTART", pnp::kGmMinRestart, pnp::kGmMaxRestart,
     &pnp_ctx::gm_restart, opt_gmres_restart},
    {PNP_OPT_IDR_S, "PNP_OPT_IDR_S", pnp::kIdrMinS, pnp::kIdrMaxS, &pnp_ctx::idr_s, opt_idr_s},
    {PNP_OPT_BICG_TWORED, "PNP_OPT_BICG_TWORED", -1, 1, &pnp_ctx::twored_opt, nullptr},
    {PNP_OPT_SEQ_ORDER, "PNP_OPT_SEQ_ORDER", 0, 1, &pnp_ctx::seq_opt, opt_seq_order},
    {PNP_OPT_MATRIX_FREE, "PNP_OPT_MATRIX_FREE", 0, 1, &pnp_ctx::mf_opt, opt_matrix_free},
    // vals holds every plane either way: nothing to invalidate
    {PNP_OPT_ASM_REUSE_CONST, "PNP_OPT_ASM_REUSE_CONST", 0, 1, &pnp_ctx::asm_reuse_opt, nullptr},
    {PNP_OPT_JAC_FD, "PNP_OPT_JAC_FD", 0, 1, &pnp_ctx::fd_opt, nullptr},
    {PNP_OPT_ILU_FUSED_FACTOR, "PNP_OPT_ILU_FUSED_FACTOR", 0, 1, &pnp_ctx::ilu_fused,
     opt_ilu_fused},
};

static const OptRow *opt_row(int32_t option) {
  for (const OptRow &r : kOptions)
    if (r.id == option) return &r;
  return nullptr;
}

extern "C" int pnp_set_option(pnp_ctx *c, int32_t option, int64_t value) {
  if (!c) return PNP_E_ARG;
  c->graphs_clear();
  const OptRow *r = opt_row(option);
  if (!r) return c->fail(PNP_E_ARG, "unknown option");
  if (value < r->lo || value > r->hi) {  // "takes 0 or 1", "takes -1, 0 or 1", "takes 2 .. 128"
    const int n = r->hi - r->lo;
    const std::string a = std::to_string(r->lo), b = std::to_string(r->hi);
    return c->fail(PNP_E_ARG, std::string(r->name) + " takes " + a +
                                  (n == 1   ? " or " + b
                                   : n == 2 ? ", " + std::to_string(r->lo + 1) + " or " + b
                                            : " .. " + b));
  }
  if (r->on_set)
    if (int rc = r->on_set(c, c->*(r->field), int(value))) return rc;
  c->*(r->field) = int(value);
  return PNP_OK;
}

extern "C" int pnp_set_create_option(int32_t option, int64_t value) {
  if (option == PNP_CREATE_ABSORB_THIN_COLOR) {
    if (value < -1 || value > 1) {
      g_err = "PNP_CREATE_ABSORB_THIN_COLOR takes -1, 0 or 1";
      return PNP_E_ARG;
    }
    pnp::g_absorb_thin_color.store(int(value));
    return PNP_OK;
  }
  g_err = "unknown creation option";
  return PNP_E_ARG;
}

extern "C" int pnp_get_create_option(int32_t option, int64_t *value) {
  if (!value) return PNP_E_ARG;
  if (option == PNP_CREATE_ABSORB_THIN_COLOR) {
    *value = pnp::g_absorb_thin_color.load();
    return PNP_OK;
  }
  g_err = "unknown creation option";
  return PNP_E_ARG;
}

extern "C" int pnp_get_option(pnp_ctx *c, int32_t option, int64_t *value) {
  if (!c || !value) return PNP_E_ARG;
  const OptRow *r = opt_row(option);
  if (!r) return c->fail(PNP_E_ARG, "unknown option");
  *value = c->*(r->field);
  return PNP_OK;
}

extern "C" int pnp_matfree_info(pnp_ctx *c, int64_t *applies, int64_t *value_assemblies) {
  if (!c) return PNP_E_ARG;
  if (applies) *applies = c->mf_applies;
  if (value_assemblies) *value_assemblies = c->value_assemblies;
  return PNP_OK;
}

extern "C" int pnp_pk_matfree_set(pnp_ctx *c, int32_t on) {
  if (!c) return PNP_E_ARG;
  if (on != 0 && on != 1) return c->fail(PNP_E_ARG, "pnp_pk_matfree_set takes 0 or 1");
  if (c->degree == 1)
    return c->fail(PNP_E_STATE,
                   "pnp_pk_matfree_set: P_k contexts of degree 2 or 3 only (a P1 context takes "
                   "PNP_OPT_MATRIX_FREE)");
  // as pnp_set_option: no graph captured in one form survives into the other, and none outlives an
  // operator change made while the switch was off
  c->graphs_clear();
  if (!on && c->mf_lin) {
    hipSetDevice(c->device);
    if (int rc = c->mf_settle()) return rc;
  }
  c->pk_mf_opt = on;
  return PNP_OK;
}

extern "C" int pnp_pk_matfree_get(pnp_ctx *c, int32_t *on) {
  if (!c || !on) return PNP_E_ARG;
  *on = c->degree > 1 ? c->pk_mf_opt : 0;
  return PNP_OK;
}

extern "C" int pnp_idr_info(pnp_ctx *c, int64_t *replacements) {
  if (!c) return PNP_E_ARG;
  if (replacements) *replacements = c->idr_replacements;
  return PNP_OK;
}

extern "C" int pnp_idr_shadow(pnp_ctx *c, int32_t j, double *p) {
  if (!c || !p) return PNP_E_ARG;
  if (!c->idr_P.p || c->idr_P_s != c->idr_s || c->idr_P_nf != c->nf)
    return c->fail(PNP_E_STATE, "no IDR solve yet with the current PNP_OPT_IDR_S and operator");
  if (j < 0 || j >= c->idr_s) return c->fail(PNP_E_ARG, "shadow column out of range");
  hipSetDevice(c->device);
  return c->download_ext(c->idr_P.p + size_t(j) * size_t(c->idr_ld(false)), c->nf, p);
}

extern "C" int pnp_asm_row_flags(pnp_ctx *c, uint8_t *flags) {
  if (!c || !flags) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set (pnp_set_operator)");
  if (c->degree > 1) return c->fail(PNP_E_STATE, "row flags: P1 contexts only");
  std::memset(flags, 0xff, size_t(c->mesh.nv));
  for (int i = 0; i < c->L.n_owned; i++) flags[c->L.l2g[i]] = c->hrowflag[i];
  return PNP_OK;
}

extern "C" int pnp_asm_info(pnp_ctx *c, int64_t *full, int64_t *reused, int64_t *pipelined) {
  if (!c) return PNP_E_ARG;
  if (full) *full = c->asm_full;
  if (reused) *reused = c->asm_reused;
  if (pipelined) *pipelined = c->asm_piped;
  return PNP_OK;
}

extern "C" int pnp_asm_regular_info(pnp_ctx *c, int64_t *chunks, int64_t *regular_chunks) {
  if (!c) return PNP_E_ARG;
  long long n = 0, r = 0;
  pnp::regular_chunks(c->L, n, r);
  if (chunks) *chunks = n;
  if (regular_chunks) *regular_chunks = r;
  return PNP_OK;
}

extern "C" int pnp_amg_configure(pnp_ctx *c, const pnp_amg_opts *o) {
  if (!c || !o) return PNP_E_ARG;
  if (o->smoother != PNP_PREC_SSOR && o->smoother != PNP_PREC_ILU0 &&
      o->smoother != PNP_PREC_JACOBI && o->smoother != PNP_PREC_SSOR_NATURAL &&
      o->smoother != PNP_PREC_CHEBYSHEV)
    return c->fail(PNP_E_ARG,
                   "AMG smoother must be SSOR, SSOR_NATURAL, ILU0, JACOBI or CHEBYSHEV");
  if (o->coarse_target < 1 || o->coarse_target > pnp::kAmgMaxCoarse || o->max_levels < 2 ||
      o->max_levels > pnp::kAmgMaxLevels || !(o->omega > 0 && o->omega <= 2) ||
      o->coarse_sweeps < 1 || o->coarse_sweeps > 8 || o->level0_presmooth < -1 ||
      o->level0_presmooth > 1)
    return c->fail(PNP_E_ARG, "AMG options out of range");
  const bool rebuild = o->coarse_target != c->amg_opts.coarse_target ||
                       o->max_levels != c->amg_opts.max_levels;
  c->amg_opts = *o;
  if (rebuild) c->amg_built = false;
  c->amg_values_drop();
  return PNP_OK;
}

extern "C" int pnp_cheb_configure(pnp_ctx *c, const pnp_cheb_opts *o) {
  if (!c) return PNP_E_ARG;
  const pnp_cheb_opts def{3, 10.0, 20, 1.1, 0.0};
  if (!o) o = &def;
  if (!pnp::cheb_opts_valid(o->steps, o->eig_ratio, o->eig_iters, o->eig_boost, o->lambda_max))
    return c->fail(PNP_E_ARG, "Chebyshev options out of range: steps 1 .. 16, eig_ratio > 1, "
                              "eig_iters 1 .. 100, eig_boost >= 1, lambda_max >= 0");
  c->cheb_opts = *o;
  // the estimate and the coefficients go; steps enters the launches by value, so the graphs go too
  c->cheb_valid = false;
  c->cheb_lest = c->cheb_lmax = c->cheb_lmin = 0;
  hipSetDevice(c->device);
  c->graphs_clear();
  return PNP_OK;
}

extern "C" int pnp_cheb_info(pnp_ctx *c, pnp_cheb_stats *st) {
  if (!c || !st) return PNP_E_ARG;
  std::memset(st, 0, sizeof *st);
  st->steps = c->cheb_opts.steps;
  st->lambda_est = c->cheb_lest;
  st->lambda_max = c->cheb_lmax;
  st->lambda_min = c->cheb_lmin;
  st->applies = c->cheb_applies;
  st->estimates = c->cheb_estimates;
  st->fused_steps = c->cheb_fused;
  st->unfused_steps = c->cheb_unfused;
  return PNP_OK;
}

extern "C" int pnp_amg_info(pnp_ctx *c, pnp_amg_stats *st) {
  if (!c || !st) return PNP_E_ARG;
  std::memset(st, 0, sizeof *st);
  if (!c->amg_built) return c->fail(PNP_E_STATE, "AMG not set up (solve or apply with PNP_PREC_AMG)");
  st->levels = int(c->amg_h.size()) + 1;
  st->rows[0] = c->L.n_owned;
  st->blocks[0] = c->L.nblocks;
  for (size_t k = 0; k < c->amg_h.size() && k + 1 < 16; k++) {
    st->rows[k + 1] = c->amg_h[k].nb;
    st->blocks[k + 1] = (int64_t)c->amg_h[k].col.size();
  }
  st->omega = c->amg_opts.omega;
  st->smoother = c->amg_opts.smoother;
  return PNP_OK;
}

extern "C" int pnp_amg_aggregates(pnp_ctx *c, int32_t level, int32_t *agg) {
  if (!c || !agg || level < 0) return PNP_E_ARG;
  if (!c->amg_built) return c->fail(PNP_E_STATE, "AMG not set up");
  if (level >= int(c->amg_h.size())) return c->fail(PNP_E_ARG, "no such AMG level");
  const std::vector<int> &a = c->amg_h[level].agg;
  if (level == 0) {  // global vertex numbering, -1 for vertices this rank does not own
    for (int g = 0; g < c->mesh.nv; g++) agg[g] = -1;
    for (int i = 0; i < c->L.n_owned; i++) agg[c->L.l2g[i]] = a[i];
  } else {
    std::copy(a.begin(), a.end(), agg);
  }
  return PNP_OK;
}

extern "C" int pnp_ion_flux(pnp_ctx *c, const double *x, int32_t nsurf, double *ip, double *im) {
  if (!c || !ip || !im || nsurf < 0 || nsurf > 256) return PNP_E_ARG;
  hipSetDevice(c->device);
  const double *xd = c->x.p;
  int rc;
  if (x) {
    if ((rc = c->upload_ext(x, 3, c->fluxx.p, true))) return rc;
    xd = c->fluxx.p;
  } else if (c->nf != 3) {
    return c->fail(PNP_E_STATE, "ion flux of the context state needs a 3-field (PNP) operator");
  }
  return c->ion_flux_dev(xd, nsurf, ip, im);
}

// the currents of the 3-field interleaved device state xd (internal layout, with ghosts)
int pnp_ctx::ion_flux_dev(const double *xd, int nsurf, double *ip, double *im) {
  pnp_ctx *c = this;
  int rc;
  const int ns = int(c->fseg_group.size());
  if (c->degree > 1)
    CK(pnp::launch_pk_ion_flux(c->dl, c->pkd, ns, c->d_fseg.p, xd, c->params.cylindrical,
                               c->params.pi, c->fluxout.p, c->stream),
       "ion flux");
  else
    CK(pnp::launch_ion_flux(ns, c->d_fseg.p, c->d_xy.p, xd, c->params.cylindrical, c->params.pi,
                            c->fluxout.p, c->stream),
       "ion flux");
  std::vector<double> out(2 * size_t(ns)), acc(2 * size_t(nsurf), 0.0);
  if (ns) {
    CK(hipMemcpyAsync(out.data(), c->fluxout.p, sizeof(double) * out.size(),
                      hipMemcpyDeviceToHost, c->stream),
       "ion flux");
  }
  CK(hipStreamSynchronize(c->stream), "ion flux");
  for (int k = 0; k < ns; k++) {  // global segment order: independent of the launch
    const int g = c->fseg_group[k];
    if (g < 0 || g >= nsurf) return c->fail(PNP_E_ARG, "boundary group outside [0, nsurf)");
    acc[2 * size_t(g)] += out[2 * size_t(k)];
    acc[2 * size_t(g) + 1] += out[2 * size_t(k) + 1];
  }
  if (c->dist && nsurf > 0) {
    CK(hipMemcpy(c->fluxred.p, acc.data(), sizeof(double) * acc.size(), hipMemcpyHostToDevice),
       "ion flux");
    if ((rc = c->allreduce_dev(c->fluxred.p, 2 * nsurf))) return rc;
    CK(hipStreamSynchronize(c->stream), "ion flux");
    CK(hipMemcpy(acc.data(), c->fluxred.p, sizeof(double) * acc.size(), hipMemcpyDeviceToHost),
       "ion flux");
  }
  for (int g = 0; g < nsurf; g++) {
    ip[g] = acc[2 * size_t(g)];
    im[g] = acc[2 * size_t(g) + 1];
  }
  return PNP_OK;
}

// PDELab Newton in the reference's order (PNP_OPT_SEQ_ORDER; the oracle's orc_newton statements):
// external layout, GridOperator residual / Jacobian in element order, ISTL solves in their order,
// defect = sqrt(<r, r>) summed sequentially, u -= lambda z
static int seq_newton(pnp_ctx *c, double *u, const pnp_newton_opts *o, pnp_newton_result *res) {
  int rc;
  if ((rc = c->seq_build())) return rc;
  double t_start = now_s();
  const size_t n = c->nseq();
  double *x = c->sq(pnp_ctx::SQ_X), *r = c->sq(pnp_ctx::SQ_R), *z = c->sq(pnp_ctx::SQ_Z),
         *prevu = c->sq(pnp_ctx::SQ_PREVU);
  CK(hipMemcpyAsync(x, u, 8 * n, hipMemcpyHostToDevice, c->stream), "seq upload");
  double ta = now_s();
  if ((rc = c->seq_residual(x, r))) return rc;
  double defect = std::sqrt(c->seq_dot(r, r, rc));
  if (rc) return rc;
  res->assemble_seconds += now_s() - ta;
  res->first_defect = defect;
  double prev_defect = defect;
  res->status = PNP_OK;
  const bool fd = c->fd_opt != 0;
  for (;;) {
    res->converged = (defect < o->abs_limit || defect < res->first_defect * o->reduction) ? 1 : 0;
    if (res->converged) break;
    if (res->iterations >= o->maxit) {
      res->status = PNP_E_NOT_CONVERGED;
      break;
    }
    ta = now_s();
    if ((rc = c->seq_jacobian(x, fd))) return rc;
    CK(hipStreamSynchronize(c->stream), "seq jacobian");
    res->assemble_seconds += now_s() - ta;
    const double stop_defect = std::max(res->first_defect * o->reduction, o->abs_limit);
    double lin_red;
    if (stop_defect / (10 * defect) > defect * defect / (prev_defect * prev_defect))
      lin_red = stop_defect / (10 * defect);
    else
      lin_red = std::min(o->min_linear_reduction, defect * defect / (prev_defect * prev_defect));
    prev_defect = defect;
    CK(hipMemsetAsync(z, 0, 8 * n, c->stream), "seq z");
    pnp_solve_opts lo = o->linear;
    lo.reduction = lin_red;
    pnp_solve_result sr{};
    double ts = now_s();
    if ((rc = c->seq_krylov(lo, z, r, sr))) return rc;  // r: overwritten by the solve's residual
    res->solve_seconds += now_s() - ts;
    res->linear_iterations += sr.iterations;
    const int step_its = sr.iterations;
    if (sr.breakdown) {
      res->status = PNP_E_BREAKDOWN;
      break;
    }
    if (!sr.converged) {
      res->status = PNP_E_NOT_CONVERGED;
      break;
    }
    // hackbuschReuskenAcceptBest
    double lambda = 1.0, best_lambda = 0.0, best_defect = defect;
    CK(hipMemcpyAsync(prevu, x, 8 * n, hipMemcpyDeviceToDevice, c->stream), "seq prevu");
    int i = 0;
    bool ls_fail = false;
    for (;;) {
      CK(pnp::launch_seq_aymx(int(n), lambda, x, z, c->stream), "seq update");
      ta = now_s();
      if ((rc = c->seq_residual(x, r))) return rc;
      defect = std::sqrt(c->seq_dot(r, r, rc));
      if (rc) return rc;
      res->assemble_seconds += now_s() - ta;
      if (defect <= (1.0 - lambda / 4) * prev_defect) break;
      if (defect < best_defect) {
        best_defect = defect;
        best_lambda = lambda;
      }
      if (++i >= o->line_search_maxit) {
        if (best_lambda == 0.0) {
          ls_fail = true;
          break;
        }
        if (best_lambda != lambda) {
          CK(hipMemcpyAsync(x, prevu, 8 * n, hipMemcpyDeviceToDevice, c->stream), "seq prevu");
          CK(pnp::launch_seq_aymx(int(n), best_lambda, x, z, c->stream), "seq update");
          if ((rc = c->seq_residual(x, r))) return rc;
          defect = std::sqrt(c->seq_dot(r, r, rc));
          if (rc) return rc;
        }
        break;
      }
      lambda *= 0.5;
      CK(hipMemcpyAsync(x, prevu, 8 * n, hipMemcpyDeviceToDevice, c->stream), "seq prevu");
    }
    if (ls_fail) {
      res->status = PNP_E_NOT_CONVERGED;
      break;
    }
    res->iterations++;
    c->newton_its.push_back(step_its);
    c->newton_defects.push_back(defect);
  }
  res->defect = defect;
  CK(hipMemcpyAsync(u, x, 8 * n, hipMemcpyDeviceToHost, c->stream), "seq download");
  CK(hipStreamSynchronize(c->stream), "seq newton");
  res->elapsed = now_s() - t_start;
  return PNP_OK;
}

extern "C" int pnp_newton(pnp_ctx *c, double *u, const pnp_newton_opts *o, pnp_newton_result *res) {
  if (!c || !u || !o || !res) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set");
  hipSetDevice(c->device);
  std::memset(res, 0, sizeof *res);
  c->newton_its.clear();
  c->newton_defects.clear();
  if (c->seq_on()) return seq_newton(c, u, o, res);
  double t_start = now_s();
  int rc;
  long long n = c->nown();
  // PNP_OPT_ILU_RETRY: the factor precision a retry switched from, restored when this call ends
  int ilu_saved = -1;
  struct IluRestore {
    pnp_ctx *c;
    int &saved;
    ~IluRestore() {
      if (saved < 0) return;
      c->ilu_f32 = saved;
      c->ilu_factors_drop();
    }
  } ilu_restore{c, ilu_saved};
  if ((rc = c->upload_ext(u, c->nf, c->x.p, true))) return rc;
  double ta = now_s();
  if ((rc = c->assemble(c->x.p, 0))) return rc;
  double defect;
  if ((rc = c->norm(c->r.p, defect))) return rc;
  res->assemble_seconds += now_s() - ta;
  res->first_defect = defect;
  double prev_defect = defect;
  res->status = PNP_OK;
  for (;;) {
    res->converged = (defect < o->abs_limit || defect < res->first_defect * o->reduction) ? 1 : 0;
    if (res->converged) break;
    if (res->iterations >= o->maxit) {
      res->status = PNP_E_NOT_CONVERGED;
      break;
    }
    ta = now_s();
    if ((rc = c->assemble(c->x.p, 1))) return rc;  // reassemble every step (threshold 0)
    CK(hipStreamSynchronize(c->stream), "assemble");
    res->assemble_seconds += now_s() - ta;
    double stop_defect = std::max(res->first_defect * o->reduction, o->abs_limit);
    double lin_red;
    if (stop_defect / (10 * defect) > defect * defect / (prev_defect * prev_defect))
      lin_red = stop_defect / (10 * defect);
    else
      lin_red = std::min(o->min_linear_reduction, defect * defect / (prev_defect * prev_defect));
    prev_defect = defect;
    // z solves J z = r(u); r lives in c->r (owned rows); keep it in b for the solver
    CK(hipMemcpyAsync(c->b.p, c->r.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream),
       "rhs");
    pnp_solve_opts lo = o->linear;
    lo.reduction = lin_red;
    pnp_solve_result sr{};
    double ts = now_s();
    if ((rc = c->krylov(c->b.p, c->z.p, lo, sr))) return rc;
    res->linear_iterations += sr.iterations;
    int step_its = sr.iterations;
    if (lo.prec == PNP_PREC_AMG && c->amg_fallback && (sr.breakdown || !sr.converged)) {
      // AMG fallback: the V-cycle of a non-symmetric system can fail where its level-0
      // smoother alone converges (a far-from-converged state); redo this step's solve with the
      // smoother as the preconditioner
      lo.prec = c->amg_opts.smoother;
      CK(hipMemcpyAsync(c->b.p, c->r.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream),
         "rhs");
      if ((rc = c->krylov(c->b.p, c->z.p, lo, sr))) return rc;
      res->linear_iterations += sr.iterations;
      step_its += sr.iterations;
      res->linear_fallbacks++;
    }
    const bool uses_ilu = lo.prec == PNP_PREC_ILU0 ||
                          (lo.prec == PNP_PREC_AMG && c->amg_opts.smoother == PNP_PREC_ILU0);
    if (c->ilu_retry && uses_ilu && c->ilu_f32 != 0 && (sr.breakdown || !sr.converged)) {
      // reduced-precision ILU(0) factors stalled this solve: re-solve with fp64 factors (ISTL's
      // SeqILU0) and keep them for the rest of this call
      if (ilu_saved < 0) ilu_saved = c->ilu_f32;
      c->ilu_f32 = 0;
      c->ilu_factors_drop();
      CK(hipMemcpyAsync(c->b.p, c->r.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream),
         "rhs");
      if ((rc = c->krylov(c->b.p, c->z.p, lo, sr))) return rc;
      res->linear_iterations += sr.iterations;
      step_its += sr.iterations;
      res->precision_retries++;
    }
    res->solve_seconds += now_s() - ts;
    if (sr.breakdown) {
      res->status = PNP_E_BREAKDOWN;
      break;
    }
    if (!sr.converged) {  // PDELab NewtonLinearSolverError
      res->status = PNP_E_NOT_CONVERGED;
      break;
    }
    // hackbuschReuskenAcceptBest line search
    double lambda = 1.0, best_lambda = 0.0, best_defect = defect;
    CK(hipMemcpyAsync(c->prevu.p, c->x.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream),
       "prevu");
    int i = 0;
    bool ls_fail = false;
    for (;;) {
      CK(pnp::launch_axpby(n, 1.0, c->prevu.p, -lambda, c->z.p, c->x.p, c->stream), "axpby");
      if ((rc = c->halo(c->x.p, c->nf))) return rc;
      ta = now_s();
      if ((rc = c->assemble(c->x.p, 0))) return rc;
      if ((rc = c->norm(c->r.p, defect))) return rc;
      res->assemble_seconds += now_s() - ta;
      if (std::isfinite(defect) && defect <= (1.0 - lambda / 4) * prev_defect) break;
      if (std::isfinite(defect) && defect < best_defect) {
        best_defect = defect;
        best_lambda = lambda;
      }
      if (++i >= o->line_search_maxit) {
        if (best_lambda == 0.0) {
          ls_fail = true;
          break;
        }
        if (best_lambda != lambda) {
          CK(pnp::launch_axpby(n, 1.0, c->prevu.p, -best_lambda, c->z.p, c->x.p, c->stream),
             "axpby");
          if ((rc = c->halo(c->x.p, c->nf))) return rc;
          if ((rc = c->assemble(c->x.p, 0))) return rc;
          if ((rc = c->norm(c->r.p, defect))) return rc;
        }
        break;
      }
      lambda *= 0.5;
    }
    if (ls_fail) {
      res->status = PNP_E_NOT_CONVERGED;
      break;
    }
    res->iterations++;
    c->newton_its.push_back(step_its);
    c->newton_defects.push_back(defect);
  }
  res->defect = defect;
  if ((rc = c->download_ext(c->x.p, c->nf, u))) return rc;
  res->elapsed = now_s() - t_start;
  return PNP_OK;
}

// owner-masked dot of two external-layout vectors (this rank's owned entries), allreduced
static int dot_ext(pnp_ctx *c, const double *a, const double *b, int nfields, int32_t flags,
                   double *out) {
  if (!c || !a || !b || !out || nfields < 1 || nfields > 3) return PNP_E_ARG;
  int rc;
  if ((rc = check_flags(c, flags, PNP_DEVICE_PTRS))) return rc;
  hipSetDevice(c->device);
  const bool dev = flags & PNP_DEVICE_PTRS;
  if ((rc = c->upload_ext(a, nfields, c->t.p, false, dev))) return rc;
  if (b != a && (rc = c->upload_ext(b, nfields, c->y.p, false, dev))) return rc;
  const long long n = (long long)c->L.n_owned * nfields;
  CK(pnp::launch_dot(n, c->t.p, b != a ? c->y.p : c->t.p, 0, c->partials.p, c->stream), "dot");
  CK(pnp::launch_reduce(c->partials.p, pnp::blas_nparts(n), 1, c->S.p + 1, c->stream), "dot");
  if (c->dist) {
    double *red = reinterpret_cast<double *>(reinterpret_cast<char *>(c->S.p + 1) +
                                             offsetof(pnp::Scalars, red));
    if ((rc = c->allreduce_dev(red, 1))) return rc;
  }
  CK(hipMemcpyAsync(c->hS + 1, c->S.p + 1, sizeof(pnp::Scalars), hipMemcpyDeviceToHost, c->stream),
     "dot readback");
  CK(hipStreamSynchronize(c->stream), "dot readback");
  *out = c->hS[1].red[0];
  return PNP_OK;
}

extern "C" int pnp_dot(pnp_ctx *c, const double *a, const double *b, int32_t nfields,
                       int32_t flags, double *out) {
  return dot_ext(c, a, b, nfields, flags, out);
}

extern "C" int pnp_norm(pnp_ctx *c, const double *a, int32_t nfields, int32_t flags, double *out) {
  const int rc = dot_ext(c, a, a, nfields, flags, out);
  if (rc == PNP_OK) *out = std::sqrt(*out);
  return rc;
}

extern "C" int pnp_newton_history(pnp_ctx *c, int32_t *its, double *defects, int32_t cap,
                                  int32_t *nsteps) {
  if (!c || !nsteps || cap < 0) return PNP_E_ARG;
  const int n = int(c->newton_its.size());
  *nsteps = n;
  for (int k = 0; k < std::min(n, int(cap)); k++) {
    if (its) its[k] = c->newton_its[k];
    if (defects) defects[k] = c->newton_defects[k];
  }
  return PNP_OK;
}

extern "C" int pnp_sync_vector(pnp_ctx *c, double *v, int32_t nfields) {
  if (!c || !v || nfields < 1 || nfields > 3) return PNP_E_ARG;
  if (!c->dist) return PNP_OK;
  hipSetDevice(c->device);
  size_t nv = size_t(c->mesh.nv), n = nv * nfields;
  std::vector<double> mine(n, 0.0);
  for (int i = 0; i < c->L.n_owned; i++)
    for (int f = 0; f < nfields; f++) mine[f * nv + c->L.l2g[i]] = v[f * nv + c->L.l2g[i]];
  CK(hipMemcpy(c->ext.p, mine.data(), sizeof(double) * n, hipMemcpyHostToDevice), "sync upload");
  int rc = c->allreduce_dev(c->ext.p, int(n));
  if (rc) return rc;
  CK(hipStreamSynchronize(c->stream), "sync");
  CK(hipMemcpy(v, c->ext.p, sizeof(double) * n, hipMemcpyDeviceToHost), "sync download");
  return PNP_OK;
}

extern "C" int pnp_initial_state(pnp_ctx *c, const double *phi_pb, double *x0) {
  if (!c || !x0) return PNP_E_ARG;
  if (c->degree > 1)
    pnp::pk_initial_state(c->tmesh, c->pks, c->params, phi_pb, x0);
  else
    pnp::initial_state(c->mesh, c->params, phi_pb, x0);
  return PNP_OK;
}

extern "C" int pnp_space(pnp_ctx *c, pnp_space_info *info, double *xy, int32_t *enode) {
  if (!c || !info) return PNP_E_ARG;
  const bool pk = c->degree > 1;
  info->degree = c->degree;
  info->nnodes = c->mesh.nv;
  info->nt = pk ? c->tmesh.nt : c->mesh.nt;
  info->nlocal = pk ? c->pks.nl : 3;
  if (xy) std::memcpy(xy, c->mesh.xy.data(), sizeof(double) * c->mesh.xy.size());
  if (enode) {
    const std::vector<int> &en = pk ? c->pks.enode : c->mesh.tri;
    std::memcpy(enode, en.data(), sizeof(int) * en.size());
  }
  return PNP_OK;
}

// ---------------------------------------------------------------------------------------------
// device-resident hot path (benchmarks)
// ---------------------------------------------------------------------------------------------
extern "C" int pnp_state_set(pnp_ctx *c, const double *x) {
  if (!c || !x) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set");
  hipSetDevice(c->device);
  int rc = c->upload_ext(x, c->nf, c->x.p, true);
  if (rc) return rc;
  CK(hipStreamSynchronize(c->stream), "state_set");
  return PNP_OK;
}

extern "C" int pnp_state_get(pnp_ctx *c, double *x) {
  if (!c || !x) return PNP_E_ARG;
  hipSetDevice(c->device);
  return c->download_ext(c->x.p, c->nf, x);
}

extern "C" int pnp_state_residual(pnp_ctx *c, double *r) {
  if (!c || !r) return PNP_E_ARG;
  if (c->kind < 0) return c->fail(PNP_E_STATE, "no operator set");
  if (c->seq_on() || c->degree > 1)
    return c->fail(PNP_E_STATE, "pnp_state_residual: P1 contexts, not in reference-order mode");
  hipSetDevice(c->device);
  return c->download_ext(c->r.p, c->nf, r);
}

extern "C" int pnp_assemble_state(pnp_ctx *c, int32_t n) {
  if (!c) return PNP_E_ARG;
  hipSetDevice(c->device);
  const int jac = n >= 0 ? 1 : 0;  // n < 0: |n| residual-only assemblies (line-search kernel)
  for (int k = 0; k < (n >= 0 ? n : -n); k++) {
    int rc = c->assemble(c->x.p, jac);
    if (rc) return rc;
  }
  CK(hipStreamSynchronize(c->stream), "assemble_state");
  return PNP_OK;
}

extern "C" int pnp_assemble_state_timed(pnp_ctx *c, int32_t n, double *ms) {
  if (!c || !ms || n == 0) return PNP_E_ARG;
  hipSetDevice(c->device);
  // one event pair around the whole batch (no per-launch events inside it): the device time of
  // |n| back-to-back launches, as a kernel trace sees them
  const bool timing = c->timing;
  c->timing = false;
  hipEvent_t e0 = c->ev_get(), e1 = c->ev_get();
  hipEventRecord(e0, c->stream);
  int rc = PNP_OK;
  for (int k = 0; k < (n >= 0 ? n : -n) && rc == PNP_OK; k++) rc = c->assemble(c->x.p, n >= 0);
  hipEventRecord(e1, c->stream);
  c->timing = timing;
  const hipError_t e = hipStreamSynchronize(c->stream);
  float t = 0;
  if (rc == PNP_OK && e == hipSuccess) hipEventElapsedTime(&t, e0, e1);
  c->ev_pool.push_back(e0);
  c->ev_pool.push_back(e1);
  if (rc) return rc;
  CK(e, "assemble_state_timed");
  *ms = t;
  return PNP_OK;
}

extern "C" int pnp_bicgstab_iterations(pnp_ctx *c, int32_t n, int32_t prec, pnp_solve_result *res) {
  if (!c || !res || n <= 0) return PNP_E_ARG;
  hipSetDevice(c->device);
  std::memset(res, 0, sizeof *res);
  pnp_solve_opts o{};
  o.prec = prec;
  o.maxit = n;
  CK(hipMemcpyAsync(c->b.p, c->r.p, sizeof(double) * c->nown(), hipMemcpyDeviceToDevice,
                    c->stream),
     "rhs");
  c->amg_symmetric = false;  // as in krylov(): BiCGSTAB
  c->after_solve = true;
  int rc = c->bicgstab(c->b.p, c->z.p, o, *res, n);
  c->amg_symmetric = true;
  return rc;
}

extern "C" int pnp_probe_slot_stores(pnp_ctx *c, int32_t tile_elems, int32_t reps,
                                     pnp_store_probe *out) {
  if (!c || !out || tile_elems <= 0 || reps <= 0) return PNP_E_ARG;
  if (c->degree < 2) return c->fail(PNP_E_ARG, "pnp_probe_slot_stores: P_k contexts only");
  hipSetDevice(c->device);
  std::memset(out, 0, sizeof *out);
  const int nl = c->pks.nl, no = c->L.n_owned;
  // pk_build's local elements: ascending global id, every element with an owned node
  std::vector<int> first(no, -1), last(no, -1);
  int ne = 0;
  for (int e = 0; e < c->tmesh.nt; e++) {
    const int *g = &c->pks.enode[size_t(e) * nl];
    bool mine = false;
    for (int a = 0; a < nl; a++) {
      const int l = c->L.g2l[g[a]];
      mine = mine || (l >= 0 && l < no);
    }
    if (!mine) continue;
    for (int a = 0; a < nl; a++) {
      const int l = c->L.g2l[g[a]];
      if (l < 0 || l >= no) continue;
      if (first[l] < 0) first[l] = ne;
      last[l] = ne;
    }
    ne++;
  }
  std::vector<int> tile(no), tsort(no), rnd(no);
  long long slots = 0;
  for (int r = 0; r < no; r++) {
    tile[r] = tsort[r] = rnd[r] = r;
    slots += pnp::meta_len(c->L.rowmeta[r]);
    out->rows_whole += first[r] / tile_elems == last[r] / tile_elems;
  }
  std::stable_sort(tile.begin(), tile.end(), [&](int a, int b) { return first[a] < first[b]; });
  std::stable_sort(tsort.begin(), tsort.end(),
                   [&](int a, int b) { return first[a] / tile_elems < first[b] / tile_elems; });
  std::mt19937 rng(20261018);
  std::shuffle(rnd.begin(), rnd.end(), rng);
  const std::vector<int> *hv[3] = {&tile, &tsort, &rnd};
  DBuf<int> d_ord[3];
  DBuf<double> val;
  for (int k = 0; k < 3; k++) {
    CK(d_ord[k].alloc(std::max(1, no)), "probe order");
    CK(hipMemcpy(d_ord[k].p, hv[k]->data(), sizeof(int) * no, hipMemcpyHostToDevice), "probe order");
  }
  CK(val.alloc(std::max<size_t>(1, size_t(c->L.chunk_off[c->L.nchunks]))), "probe slots");
  const int *orders[4] = {nullptr, d_ord[0].p, d_ord[1].p, d_ord[2].p};
  double *res[4] = {&out->us_sell, &out->us_tile, &out->us_tile_sorted, &out->us_random};
  for (int k = 0; k < 4; k++) {
    for (int w = 0; w < 2; w++) CK(pnp::launch_slot_store_probe(c->dl, orders[k], val.p, c->stream), "probe");
    hipEvent_t e0 = c->ev_get(), e1 = c->ev_get();
    hipEventRecord(e0, c->stream);
    for (int i = 0; i < reps; i++) CK(pnp::launch_slot_store_probe(c->dl, orders[k], val.p, c->stream), "probe");
    hipEventRecord(e1, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    float t = 0;
    if (e == hipSuccess) hipEventElapsedTime(&t, e0, e1);
    c->ev_pool.push_back(e0);
    c->ev_pool.push_back(e1);
    CK(e, "probe");
    *res[k] = 1e3 * t / reps;
  }
  out->slot_bytes = 8 * slots;
  out->rows = no;
  out->tiles = (ne + tile_elems - 1) / tile_elems;
  out->elements = ne;
  return PNP_OK;
}

extern "C" int pnp_cache_scrub(pnp_ctx *c, int64_t bytes) {
  if (!c || bytes < 0) return PNP_E_ARG;
  hipSetDevice(c->device);
  const size_t n = size_t(bytes) / 8;
  if (c->scrub.n < n + 1) CK(c->scrub.alloc(n + 1), "scrub buffer");
  CK(pnp::launch_scrub(c->scrub.p, (long long)n, c->scrub.p + n, c->stream), "scrub");
  CK(hipStreamSynchronize(c->stream), "scrub");
  return PNP_OK;
}

extern "C" int pnp_timers_enable(pnp_ctx *c, int32_t on) {
  if (!c) return PNP_E_ARG;
  c->timing = on != 0;
  return PNP_OK;
}

extern "C" int pnp_timers_get(pnp_ctx *c, pnp_timers *t) {
  if (!c || !t) return PNP_E_ARG;
  c->timers_flush();
  t->assemble_ms = c->t_ms[T_ASM];
  t->spmv_ms = c->t_ms[T_SPMV];
  t->prec_ms = c->t_ms[T_PREC];
  t->blas_ms = c->t_ms[T_BLAS];
  t->halo_ms = c->t_ms[T_HALO];
  t->allreduce_ms = c->t_ms[T_ALLRED];
  t->assemble_launches = c->t_n[T_ASM];
  t->spmv_launches = c->t_n[T_SPMV];
  t->prec_launches = c->t_n[T_PREC];
  t->blas_launches = c->t_n[T_BLAS];
  t->factor_ms = c->t_ms[T_FACT];
  t->factor_launches = c->t_n[T_FACT];
  return PNP_OK;
}

extern "C" int pnp_timers_reset(pnp_ctx *c) {
  if (!c) return PNP_E_ARG;
  c->timers_flush();
  for (int k = 0; k < T_NCAT; k++) {
    c->t_ms[k] = 0;
    c->t_n[k] = 0;
  }
  return PNP_OK;
}

// ---------------------------------------------------------------------------------------------
// host-only setup / inspection
// ---------------------------------------------------------------------------------------------
struct pnp_layout_buf {
  pnp::Mesh mesh, tmesh;  // as pnp_ctx: for degree > 1 the node mesh and the triangle mesh
  pnp::PkSpace pks;
  pnp::Fans fans;
  pnp::LocalLayout L;
  pnp::DerivedLayout D;  // filled by pnp_layout_derived
};

extern "C" int pnp_setup_boundary(const pnp_mesh *mesh, const pnp_params *params, int32_t nfields,
                                  int32_t field0, uint8_t *mask, double *load) {
  if (!params || nfields < 1 || field0 < 0 || field0 + nfields > 3) return PNP_E_ARG;
  pnp::Mesh m;
  std::string err;
  if (!mesh_from_view(mesh, m, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  pnp::Params P;
  params_from(params, P);
  for (int s = 0; s < m.nb; s++)
    if (m.bgroup[s] < 0 || m.bgroup[s] >= int(P.surf.size())) return PNP_E_ARG;
  std::vector<uint8_t> mk;
  std::vector<double> ld;
  pnp::dirichlet_mask(m, P, nfields, field0, mk);
  pnp::neumann_load(m, P, nfields, field0, ld);
  for (int v = 0; v < m.nv; v++)
    for (int f = 0; f < nfields; f++) {
      if (mask) mask[size_t(f) * m.nv + v] = mk[size_t(v) * nfields + f];
      if (load) load[size_t(f) * m.nv + v] = ld[size_t(v) * nfields + f];
    }
  return PNP_OK;
}

extern "C" int pnp_setup_initial_state(const pnp_mesh *mesh, const pnp_params *params,
                                       const double *phi_pb, double *x0) {
  if (!params || !x0) return PNP_E_ARG;
  pnp::Mesh m;
  std::string err;
  if (!mesh_from_view(mesh, m, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  pnp::Params P;
  params_from(params, P);
  for (int s = 0; s < m.nb; s++)
    if (m.bgroup[s] < 0 || m.bgroup[s] >= int(P.surf.size())) return PNP_E_ARG;
  pnp::initial_state(m, P, phi_pb, x0);
  return PNP_OK;
}

extern "C" int pnp_layout_build(const pnp_mesh *mesh, int32_t rank, int32_t nranks,
                                pnp_layout_buf **out) {
  return pnp_layout_build_pk(mesh, 1, rank, nranks, out);
}

extern "C" int pnp_layout_build_pk(const pnp_mesh *mesh, int32_t degree, int32_t rank,
                                   int32_t nranks, pnp_layout_buf **out) {
  if (!out || degree < 1 || degree > 3 || nranks < 1 || rank < 0 || rank >= nranks)
    return PNP_E_ARG;
  auto b = std::make_unique<pnp_layout_buf>();
  std::string err;
  if (!mesh_from_view(mesh, b->mesh, err) ||
      !pnp::build_host_layout(b->mesh, degree, rank, nranks, b->tmesh, b->pks, b->fans, b->L, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  *out = b.release();
  return PNP_OK;
}

extern "C" int pnp_layout_derived(pnp_layout_buf *b, const pnp_layout_knobs *knobs,
                                  pnp_derived_layout *v) {
  if (!b || !v) return PNP_E_ARG;
  pnp::LayoutKnobs K = pnp::LayoutKnobs::from_env();
  if (knobs) {
    K.split_sort = knobs->split_sort != 0;
    K.blkmap = knobs->blkmap != 0;
    K.spmv_lds = knobs->spmv_lds != 0;
    K.list_own_last = knobs->list_own_last != 0;
    K.halo_overlap = knobs->halo_overlap != 0;
    K.xcd_remap = knobs->xcd_remap;
  }
  std::string err;
  if (!pnp::derive_layout(b->mesh, b->L, K, b->D, err)) {
    g_err = err;
    return PNP_E_MESH;
  }
  const pnp::DerivedLayout &D = b->D;
  static_assert(sizeof(pnp::FluxSeg) == 4 * sizeof(int32_t), "flux segment record");
  std::memset(v, 0, sizeof *v);
  v->lslots = int64_t(D.split.lsrc.size());
  v->uslots = int64_t(D.split.usrc.size());
  v->lslots_live = D.split.lslots_live;
  v->uslots_live = D.split.uslots_live;
  v->lsx_entries = int64_t(D.sweep.llist.size());
  v->usx_entries = int64_t(D.sweep.ulist.size());
  v->lperm = D.split.lperm.data();
  v->uperm = D.split.uperm.data();
  v->lpinv = D.split.lpinv.data();
  v->upinv = D.split.upinv.data();
  v->llen = D.split.llen.data();
  v->ulen = D.split.ulen.data();
  v->ldl = D.split.ldl.data();
  v->lchunk_len = D.split.lchunk_len.data();
  v->lchunk_off = D.split.lchunk_off.data();
  v->lcolidx = D.split.lcolidx.data();
  v->lsrc = D.split.lsrc.data();
  v->uchunk_len = D.split.uchunk_len.data();
  v->uchunk_off = D.split.uchunk_off.data();
  v->ucolidx = D.split.ucolidx.data();
  v->usrc = D.split.usrc.data();
  v->lsx_ptr = D.sweep.lptr.data();
  v->lsx_list = D.sweep.llist.data();
  v->usx_ptr = D.sweep.uptr.data();
  v->usx_list = D.sweep.ulist.data();
  v->lsx_idx = D.sweep.lidx.data();
  v->usx_idx = D.sweep.uidx.data();
  v->rowoff = D.rows.rowoff.data();
  v->rowcol = D.rows.rowcol.data();
  v->blkmap = D.blkmap.data();
  v->fseg = D.flux.segs.empty() ? nullptr : &D.flux.segs[0].a;
  v->fseg_group = D.flux.group.data();
  v->uptr = D.spmv.uptr.data();
  v->ulist = D.spmv.ulist.data();
  v->uown = D.spmv.uown.data();
  v->lidx = D.spmv.lidx.data();
  v->blk_int = D.halo.interior.data();
  v->blk_bnd = D.halo.boundary.data();
  v->npos = 64 * b->L.nchunks;
  v->sweep_usable = D.sweep.usable;
  v->sx_max = D.sweep.sx_max;
  v->n_sweep_blocks = D.sweep.usable ? int(D.sweep.lptr.size()) - 1 : 0;
  v->nblk = (b->L.n_owned + 255) / 256;
  v->n_blkmap = int(D.blkmap.size());
  v->nfseg = int(D.flux.segs.size());
  v->spmv_usable = D.spmv.usable;
  v->umax = D.spmv.umax;
  v->unmax = D.spmv.unmax;
  v->halo_usable = D.halo.usable;
  v->n_blk_int = int(D.halo.interior.size());
  v->n_blk_bnd = int(D.halo.boundary.size());
  v->xcd_remap = K.xcd_remap;
  return PNP_OK;
}

extern "C" int pnp_layout_view(const pnp_layout_buf *b, pnp_layout *v) {
  if (!b || !v) return PNP_E_ARG;
  const pnp::LocalLayout &L = b->L;
  v->n_owned = L.n_owned;
  v->n_ghost = L.n_ghost;
  v->ncolors = int(L.color_ptr.size()) - 1;
  v->nchunks = L.nchunks;
  v->nnbr = int(L.nbr_ranks.size());
  v->max_slots = b->fans.max_slots;
  v->nslots = L.nslots;
  v->nblocks = L.nblocks;
  v->l2g = L.l2g.data();
  v->color_ptr = L.color_ptr.data();
  v->color_idx = L.color_idx.data();
  v->rowcolor = L.rowcolor.data();
  v->chunk_len = L.chunk_len.data();
  v->chunk_off = L.chunk_off.data();
  v->colidx = L.colidx.data();
  v->rowmeta = L.rowmeta.data();
  v->nbr_ranks = L.nbr_ranks.data();
  v->recv_ptr = L.recv_ptr.data();
  v->send_ptr = L.send_ptr.data();
  v->send_idx = L.send_idx.data();
  v->color_conflicts = L.conflicts;
  return PNP_OK;
}

extern "C" int pnp_layout_regular_info(const pnp_layout_buf *b, int64_t *chunks,
                                       int64_t *regular_chunks) {
  if (!b) return PNP_E_ARG;
  long long n = 0, r = 0;
  pnp::regular_chunks(b->L, n, r);
  if (chunks) *chunks = n;
  if (regular_chunks) *regular_chunks = r;
  return PNP_OK;
}

extern "C" void pnp_layout_free(pnp_layout_buf *b) { delete b; }
