// IDR(s), the bi-orthogonal variant of van Gijzen and Sonneveld (2011), right-preconditioned: the
// streaming kernels over the n x s arrays G, U and the shadow matrix P, and the one-thread kernels
// on the device-resident state block (idr_small.h).  DESIGN.md 4.10.
//
// G and P hold owned rows only (column i at + i * ldg); a column of U is an SpMV input and carries
// its ghosts (+ i * ldu).  Every streaming kernel makes one pass over its vectors in fixed
// 1,024-entry slices with 16-byte loads; a reduction's partials are value-major (value v of slice
// b at part[v * nps + b]) and are summed by k_idr_colsum, one workgroup per value in a fixed
// order: no atomics, no ticket.  With more than one rank the host follows each k_idr_colsum with
// one allreduce of the summed block.  Every kernel reads phase / k / done from the state block and
// returns at once outside its step, so the host enqueues steps without knowing whether the
// recurrence has ended.
#include "idr_small.h"
#include "kernels.h"

namespace pnp {

namespace {

constexpr int kIdrBlock = 256;
constexpr int kIdrU = 2;                            // 16-byte loads per thread and vector
constexpr int kIdrSlice = kIdrBlock * 2 * kIdrU;    // entries per workgroup
constexpr int kIdrWaves = kIdrBlock / 64;
constexpr int kIdrVals = kIdrMaxS + 4;

// hk < 0: any k
__device__ __forceinline__ bool idr_active(const IdrState *S, int phase, int hk) {
  return !S->done && S->phase == phase && (hk < 0 || S->k == hk);
}

// entries e, e + 1 of p (e even, p 16-byte aligned), zero past n
__device__ __forceinline__ void idr_load2(const double *__restrict__ p, long long e, long long n,
                                          double &a, double &b) {
  if (e + 1 < n) {
    const double2 t = *reinterpret_cast<const double2 *>(p + e);
    a = t.x;
    b = t.y;
  } else {
    a = e < n ? p[e] : 0.0;
    b = 0.0;
  }
}
__device__ __forceinline__ void idr_store2(double *__restrict__ p, long long e, long long n,
                                           double a, double b) {
  if (e + 1 < n)
    *reinterpret_cast<double2 *>(p + e) = make_double2(a, b);
  else if (e < n)
    p[e] = a;
}

__device__ __forceinline__ double idr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__device__ __forceinline__ long long idr_entry(int u) {
  return (long long)blockIdx.x * kIdrSlice + u * (2 * kIdrBlock) + 2 * threadIdx.x;
}

// this workgroup's partials of <P_i, w>, i < s, into sm[.][base + i]: the s columns' loads are
// issued together
__device__ __forceinline__ void idr_pdots(const double *__restrict__ P, long long ldp, long long n,
                                          int s, const double (&wv)[2 * kIdrU],
                                          double (*sm)[kIdrVals], int base) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[kIdrMaxS];
#pragma unroll
  for (int i = 0; i < kIdrMaxS; i++) {
    acc[i] = 0.0;
    if (i < s) {  // uniform
      const double *__restrict__ pi = P + size_t(i) * ldp;
#pragma unroll
      for (int u = 0; u < kIdrU; u++) {
        double a, b;
        idr_load2(pi, idr_entry(u), n, a, b);
        acc[i] += a * wv[2 * u];
        acc[i] += b * wv[2 * u + 1];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kIdrMaxS; i++) {
    const double r = idr_wave_sum(acc[i]);
    if (lane == 0 && i < s) sm[wave][base + i] = r;
  }
}

__device__ __forceinline__ void idr_norm2(const double (&wv)[2 * kIdrU], double (*sm)[kIdrVals],
                                          int slot) {
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < 2 * kIdrU; q++) acc += wv[q] * wv[q];
  acc = idr_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][slot] = acc;
}

// after __syncthreads(): the workgroup's nvals sums to part (value-major)
__device__ __forceinline__ void idr_flush(double (*sm)[kIdrVals], int nvals,
                                          double *__restrict__ part, int nps) {
  for (int i = threadIdx.x; i < nvals; i += kIdrBlock) {
    double s = sm[0][i];
#pragma unroll
    for (int q = 1; q < kIdrWaves; q++) s += sm[q][i];
    part[size_t(i) * nps + blockIdx.x] = s;
  }
}

// (a) UPD = false: out = src - sum_{i >= k} c_i B_i      (v from r and G)
// (b) UPD = true:  B_k = omega src + sum_{i >= k} c_i B_i (U_k from v^ and U; the read of the old
//     U_k is element-wise, so in place is safe)
template <bool UPD>
__global__ __launch_bounds__(kIdrBlock) void k_idr_comb(const IdrState *__restrict__ S, int hk,
                                                        const double *__restrict__ src, double *B,
                                                        long long ldb, long long n, double *out) {
  if (!idr_active(S, 0, hk)) return;
  const int s = S->s, k = S->k;
  const double w0 = UPD ? S->omega : 1.0;
  long long e[kIdrU];
  double acc[2 * kIdrU];
#pragma unroll
  for (int u = 0; u < kIdrU; u++) {
    e[u] = idr_entry(u);
    double a, b;
    idr_load2(src, e[u], n, a, b);
    acc[2 * u] = w0 * a;
    acc[2 * u + 1] = w0 * b;
  }
#pragma unroll 4
  for (int i = k; i < s; i++) {
    const double *bi = B + size_t(i) * ldb;
    const double ci = UPD ? S->c[i] : -S->c[i];
#pragma unroll
    for (int u = 0; u < kIdrU; u++) {
      double a, b;
      idr_load2(bi, e[u], n, a, b);
      acc[2 * u] += ci * a;
      acc[2 * u + 1] += ci * b;
    }
  }
  double *dst = UPD ? B + size_t(k) * ldb : out;
#pragma unroll
  for (int u = 0; u < kIdrU; u++) idr_store2(dst, e[u], n, acc[2 * u], acc[2 * u + 1]);
}

// (c) partials of P^T G_k: values 0 .. s - 1
__global__ __launch_bounds__(kIdrBlock) void k_idr_ptg(const IdrState *__restrict__ S, int hk,
                                                       const double *__restrict__ G, long long ldg,
                                                       const double *__restrict__ P, long long n,
                                                       double *__restrict__ part, int nps) {
  if (!idr_active(S, 0, hk)) return;
  __shared__ double sm[kIdrWaves][kIdrVals];
  const int s = S->s;
  const double *__restrict__ gk = G + size_t(S->k) * ldg;
  double wv[2 * kIdrU];
#pragma unroll
  for (int u = 0; u < kIdrU; u++) idr_load2(gk, idr_entry(u), n, wv[2 * u], wv[2 * u + 1]);
  idr_pdots(P, ldg, n, s, wv, sm, 0);
  __syncthreads();
  idr_flush(sm, s, part, nps);
}

// (d) G_k -= sum_{i<k} alpha_i G_i, U_k -= sum_{i<k} alpha_i U_i, r -= beta G_k, x += beta U_k,
// partial of ||r||^2 (value 0)
__global__ __launch_bounds__(kIdrBlock) void k_idr_update(const IdrState *__restrict__ S, int hk,
                                                          double *G, long long ldg, double *U,
                                                          long long ldu, double *__restrict__ r,
                                                          double *__restrict__ x, long long n,
                                                          double *__restrict__ part, int nps) {
  if (!idr_active(S, 0, hk)) return;
  __shared__ double sm[kIdrWaves][kIdrVals];
  const int k = S->k;
  const double beta = S->beta;
  double *gk = G + size_t(k) * ldg, *uk = U + size_t(k) * ldu;
  long long e[kIdrU];
  double g[2 * kIdrU], uu[2 * kIdrU], rv[2 * kIdrU], xv[2 * kIdrU];
#pragma unroll
  for (int u = 0; u < kIdrU; u++) {
    e[u] = idr_entry(u);
    idr_load2(gk, e[u], n, g[2 * u], g[2 * u + 1]);
    idr_load2(uk, e[u], n, uu[2 * u], uu[2 * u + 1]);
    idr_load2(r, e[u], n, rv[2 * u], rv[2 * u + 1]);
    idr_load2(x, e[u], n, xv[2 * u], xv[2 * u + 1]);
  }
#pragma unroll 2
  for (int i = 0; i < k; i++) {
    const double *gi = G + size_t(i) * ldg, *ui = U + size_t(i) * ldu;
    const double ai = S->alpha[i];
#pragma unroll
    for (int u = 0; u < kIdrU; u++) {
      double a, b;
      idr_load2(gi, e[u], n, a, b);
      g[2 * u] -= ai * a;
      g[2 * u + 1] -= ai * b;
      idr_load2(ui, e[u], n, a, b);
      uu[2 * u] -= ai * a;
      uu[2 * u + 1] -= ai * b;
    }
  }
#pragma unroll
  for (int q = 0; q < 2 * kIdrU; q++) {
    rv[q] -= beta * g[q];
    xv[q] += beta * uu[q];
  }
#pragma unroll
  for (int u = 0; u < kIdrU; u++) {
    if (k > 0) {  // uniform: step 0 has nothing to correct
      idr_store2(gk, e[u], n, g[2 * u], g[2 * u + 1]);
      idr_store2(uk, e[u], n, uu[2 * u], uu[2 * u + 1]);
    }
    idr_store2(r, e[u], n, rv[2 * u], rv[2 * u + 1]);
    idr_store2(x, e[u], n, xv[2 * u], xv[2 * u + 1]);
  }
  idr_norm2(rv, sm, 0);
  __syncthreads();
  idr_flush(sm, 1, part, nps);
}

// (e) first half: partials of <t, r>, <t, t>, <r, r> (values 0, 1, 2)
__global__ __launch_bounds__(kIdrBlock) void k_idr_om_dots(const IdrState *__restrict__ S,
                                                           const double *__restrict__ t,
                                                           const double *__restrict__ r,
                                                           long long n, double *__restrict__ part,
                                                           int nps) {
  if (!idr_active(S, 1, -1)) return;
  __shared__ double sm[kIdrWaves][kIdrVals];
  double tr = 0.0, tt = 0.0, rr = 0.0;
#pragma unroll
  for (int u = 0; u < kIdrU; u++) {
    double t0, t1, r0, r1;
    idr_load2(t, idr_entry(u), n, t0, t1);
    idr_load2(r, idr_entry(u), n, r0, r1);
    tr += t0 * r0;
    tr += t1 * r1;
    tt += t0 * t0;
    tt += t1 * t1;
    rr += r0 * r0;
    rr += r1 * r1;
  }
  tr = idr_wave_sum(tr);
  tt = idr_wave_sum(tt);
  rr = idr_wave_sum(rr);
  if ((threadIdx.x & 63) == 0) {
    sm[threadIdx.x >> 6][0] = tr;
    sm[threadIdx.x >> 6][1] = tt;
    sm[threadIdx.x >> 6][2] = rr;
  }
  __syncthreads();
  idr_flush(sm, 3, part, nps);
}

// (e) second half (MODE 0): r -= omega t, x += omega v^, partials of ||r||^2 (value 0) and of
// P^T r (values 1 .. s).  MODE 1: the partials alone, of a residual the SpMV has just formed
// (the solve's start and the residual replacement, phase 2).
template <int MODE>
__global__ __launch_bounds__(kIdrBlock) void k_idr_om_update(const IdrState *__restrict__ S,
                                                             const double *__restrict__ t,
                                                             const double *__restrict__ vh,
                                                             double *__restrict__ r,
                                                             double *__restrict__ x,
                                                             const double *__restrict__ P,
                                                             long long ldp, long long n,
                                                             double *__restrict__ part, int nps) {
  if (!idr_active(S, MODE == 0 ? 1 : 2, -1)) return;
  __shared__ double sm[kIdrWaves][kIdrVals];
  const int s = S->s;
  double rv[2 * kIdrU];
#pragma unroll
  for (int u = 0; u < kIdrU; u++) idr_load2(r, idr_entry(u), n, rv[2 * u], rv[2 * u + 1]);
  if (MODE == 0) {
    const double om = S->omega;
#pragma unroll
    for (int u = 0; u < kIdrU; u++) {
      const long long e = idr_entry(u);
      double t0, t1, v0, v1, x0, x1;
      idr_load2(t, e, n, t0, t1);
      idr_load2(vh, e, n, v0, v1);
      idr_load2(x, e, n, x0, x1);
      rv[2 * u] -= om * t0;
      rv[2 * u + 1] -= om * t1;
      idr_store2(r, e, n, rv[2 * u], rv[2 * u + 1]);
      idr_store2(x, e, n, x0 + om * v0, x1 + om * v1);
    }
  }
  idr_norm2(rv, sm, 0);
  idr_pdots(P, ldp, n, s, rv, sm, 1);
  __syncthreads();
  idr_flush(sm, s + 1, part, nps);
}

// workgroup i sums value i's np partials (thread t takes t, t + 256, ... in order, then the fixed
// tree) into S->red[i].  phase < 0: ungated (the shadow matrix's orthonormalisation).
__global__ __launch_bounds__(kIdrBlock) void k_idr_colsum(IdrState *__restrict__ S, int phase,
                                                          int hk, const double *__restrict__ part,
                                                          int nps, int np) {
  if (phase >= 0 && !idr_active(S, phase, hk)) return;
  const int i = blockIdx.x;
  __shared__ double sm[kIdrWaves];
  double acc = 0.0;
  for (int t = threadIdx.x; t < np; t += kIdrBlock) acc += part[size_t(i) * nps + t];
  acc = idr_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sm[0];
#pragma unroll
    for (int q = 1; q < kIdrWaves; q++) s += sm[q];
    S->red[i] = s;
  }
}

// which: 0 step_a, 1 step_b, 2 omega, 3 omega_end, 4 begin (first = hk)
__global__ void k_idr_small(IdrState *S, double *hist, int which, int hk) {
  if (threadIdx.x != 0) return;
  if (which == 0)
    idr_step_a(S, hk);
  else if (which == 1)
    idr_step_b(S, hist, hk);
  else if (which == 2)
    idr_omega(S);
  else if (which == 3)
    idr_omega_end(S, hist);
  else
    idr_begin(S, hist, hk);
}

// ---- the shadow matrix -----------------------------------------------------------------------
__global__ __launch_bounds__(kIdrBlock) void k_idr_shadow_fill(int n_owned, int nf, int s,
                                                               const int *__restrict__ l2g,
                                                               double *__restrict__ P,
                                                               long long ldp) {
  const long long e = (long long)blockIdx.x * kIdrBlock + threadIdx.x;
  if (e >= (long long)n_owned * nf) return;
  const int i = int(e / nf), f = int(e - (long long)i * nf);
  const unsigned long long g = (unsigned long long)l2g[i];
  for (int j = 0; j < s; j++) P[size_t(j) * ldp + e] = idr_shadow_entry(g, unsigned(f), unsigned(j));
}

// partial of <a, b> (value 0)
__global__ __launch_bounds__(kIdrBlock) void k_idr_dot(const double *__restrict__ a,
                                                       const double *__restrict__ b, long long n,
                                                       double *__restrict__ part) {
  __shared__ double sm[kIdrWaves];
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < kIdrU; u++) {
    double a0, a1, b0, b1;
    idr_load2(a, idr_entry(u), n, a0, a1);
    idr_load2(b, idr_entry(u), n, b0, b1);
    acc += a0 * b0;
    acc += a1 * b1;
  }
  acc = idr_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sm[0];
#pragma unroll
    for (int q = 1; q < kIdrWaves; q++) s += sm[q];
    part[blockIdx.x] = s;
  }
}

// src == null: a *= 1 / sqrt(red[0]); else a -= red[0] * src
__global__ __launch_bounds__(kIdrBlock) void k_idr_mgs(const IdrState *__restrict__ S,
                                                       double *__restrict__ a,
                                                       const double *__restrict__ src,
                                                       long long n) {
  const double d = S->red[0];
  const double sc = src ? -d : 1.0 / sqrt(d);
#pragma unroll
  for (int u = 0; u < kIdrU; u++) {
    const long long e = idr_entry(u);
    double a0, a1;
    idr_load2(a, e, n, a0, a1);
    if (src) {
      double b0, b1;
      idr_load2(src, e, n, b0, b1);
      idr_store2(a, e, n, a0 + sc * b0, a1 + sc * b1);
    } else {
      idr_store2(a, e, n, a0 * sc, a1 * sc);
    }
  }
}

bool idr_geom_ok(long long ld, long long n) { return !(ld & 1) && ld >= n; }

}  // namespace

int idr_nparts(long long n) {
  const long long np = (n + kIdrSlice - 1) / kIdrSlice;
  return np > 0 ? int(np) : 1;
}

double *idr_red(IdrState *S) { return S->red; }

hipError_t launch_idr_v(const IdrState *S, int hk, const double *r, double *G, long long ldg,
                        long long n, double *v, hipStream_t st) {
  if (!idr_geom_ok(ldg, n)) return hipErrorInvalidValue;
  k_idr_comb<false><<<idr_nparts(n), kIdrBlock, 0, st>>>(S, hk, r, G, ldg, n, v);
  return hipGetLastError();
}

hipError_t launch_idr_u(const IdrState *S, int hk, const double *vh, double *U, long long ldu,
                        long long n, hipStream_t st) {
  if (!idr_geom_ok(ldu, n)) return hipErrorInvalidValue;
  k_idr_comb<true><<<idr_nparts(n), kIdrBlock, 0, st>>>(S, hk, vh, U, ldu, n, nullptr);
  return hipGetLastError();
}

hipError_t launch_idr_ptg(IdrState *S, int hk, int s, const double *G, long long ldg,
                          const double *P, long long n, double *part, int nps, hipStream_t st) {
  const int np = idr_nparts(n);
  if (np > nps || !idr_s_valid(s) || !idr_geom_ok(ldg, n)) return hipErrorInvalidValue;
  k_idr_ptg<<<np, kIdrBlock, 0, st>>>(S, hk, G, ldg, P, n, part, nps);
  k_idr_colsum<<<s, kIdrBlock, 0, st>>>(S, 0, hk, part, nps, np);
  return hipGetLastError();
}

hipError_t launch_idr_small(IdrState *S, double *hist, int which, int hk, hipStream_t st) {
  k_idr_small<<<1, 64, 0, st>>>(S, hist, which, hk);
  return hipGetLastError();
}

hipError_t launch_idr_update(IdrState *S, int hk, double *G, long long ldg, double *U,
                             long long ldu, double *r, double *x, long long n, double *part,
                             int nps, hipStream_t st) {
  const int np = idr_nparts(n);
  if (np > nps || !idr_geom_ok(ldg, n) || !idr_geom_ok(ldu, n)) return hipErrorInvalidValue;
  k_idr_update<<<np, kIdrBlock, 0, st>>>(S, hk, G, ldg, U, ldu, r, x, n, part, nps);
  k_idr_colsum<<<1, kIdrBlock, 0, st>>>(S, 0, hk, part, nps, np);
  return hipGetLastError();
}

hipError_t launch_idr_om_dots(IdrState *S, const double *t, const double *r, long long n,
                              double *part, int nps, hipStream_t st) {
  const int np = idr_nparts(n);
  if (np > nps) return hipErrorInvalidValue;
  k_idr_om_dots<<<np, kIdrBlock, 0, st>>>(S, t, r, n, part, nps);
  k_idr_colsum<<<3, kIdrBlock, 0, st>>>(S, 1, -1, part, nps, np);
  return hipGetLastError();
}

hipError_t launch_idr_om_update(IdrState *S, int s, const double *t, const double *vh, double *r,
                                double *x, const double *P, long long ldp, long long n,
                                double *part, int nps, hipStream_t st) {
  const int np = idr_nparts(n);
  if (np > nps || !idr_s_valid(s) || !idr_geom_ok(ldp, n)) return hipErrorInvalidValue;
  k_idr_om_update<0><<<np, kIdrBlock, 0, st>>>(S, t, vh, r, x, P, ldp, n, part, nps);
  k_idr_colsum<<<s + 1, kIdrBlock, 0, st>>>(S, 1, -1, part, nps, np);
  return hipGetLastError();
}

hipError_t launch_idr_resid_dots(IdrState *S, int s, double *r, const double *P, long long ldp,
                                 long long n, double *part, int nps, hipStream_t st) {
  const int np = idr_nparts(n);
  if (np > nps || !idr_s_valid(s) || !idr_geom_ok(ldp, n)) return hipErrorInvalidValue;
  k_idr_om_update<1><<<np, kIdrBlock, 0, st>>>(S, nullptr, nullptr, r, nullptr, P, ldp, n, part, nps);
  k_idr_colsum<<<s + 1, kIdrBlock, 0, st>>>(S, 2, -1, part, nps, np);
  return hipGetLastError();
}

hipError_t launch_idr_shadow_fill(int n_owned, int nf, int s, const int *l2g, double *P,
                                  long long ldp, hipStream_t st) {
  const long long n = (long long)n_owned * nf;
  if (!idr_s_valid(s) || !idr_geom_ok(ldp, n)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  k_idr_shadow_fill<<<unsigned((n + kIdrBlock - 1) / kIdrBlock), kIdrBlock, 0, st>>>(n_owned, nf, s,
                                                                                    l2g, P, ldp);
  return hipGetLastError();
}

hipError_t launch_idr_dot(IdrState *S, const double *a, const double *b, long long n, double *part,
                          int nps, hipStream_t st) {
  const int np = idr_nparts(n);
  if (np > nps) return hipErrorInvalidValue;
  k_idr_dot<<<np, kIdrBlock, 0, st>>>(a, b, n, part);
  k_idr_colsum<<<1, kIdrBlock, 0, st>>>(S, -1, -1, part, nps, np);
  return hipGetLastError();
}

hipError_t launch_idr_mgs(const IdrState *S, double *a, const double *src, long long n,
                          hipStream_t st) {
  k_idr_mgs<<<idr_nparts(n), kIdrBlock, 0, st>>>(S, a, src, n);
  return hipGetLastError();
}

}  // namespace pnp
