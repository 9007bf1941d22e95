// Restarted GMRES(m) / flexible GMRES: the multi-vector orthogonalisation kernels and the small
// dense kernels on the device-resident state block (gmres_small.h).  DESIGN.md 4.8.
//
// The basis V is (m + 1) vectors of ld doubles (ld even, >= n_local * nf: a basis vector is an
// SpMV input, so it carries its ghosts); the new direction w = A M^-1 V_j is written by the SpMV
// straight into V_{j+1}.  One Arnoldi step orthogonalises w against V_0 .. V_j twice (classical
// Gram-Schmidt applied twice, CGS2) in three launches of k_gm_orth over fixed 1,024-entry slices:
//   mode 0: partials of <V_i, w>, i = 0 .. j, and of <w, w>
//   mode 1: w -= sum red1[i] V_i, then partials of <V_i, w> for the second pass (row-local, so
//           the slice of w stays in registers; the basis slice is read a second time)
//   mode 2: w -= sum red2[i] V_i, then the partial of <w, w>: the new direction's norm
// Each is followed by k_gm_colsum (one workgroup per value sums that value's partials in a fixed
// order; no atomics, no ticket) and, with more than one rank, an allreduce of the summed block.
// Every kernel reads j and the phase / done flags from the state block and returns at once when
// its phase is not the current one, so the host enqueues steps without knowing when a cycle ended.
#include "gmres_small.h"
#include "kernels.h"

namespace pnp {

namespace {

constexpr int kGmBlock = 256;
constexpr int kGmU = 2;                           // 16-byte loads per thread and vector
constexpr int kGmSlice = kGmBlock * 2 * kGmU;     // entries per workgroup
constexpr int kGmWaves = kGmBlock / 64;
constexpr int kGmVals = kGmMaxRestart + 2;
constexpr int kGmJB = 4;                          // basis vectors per dot batch

__device__ __forceinline__ bool gm_active(const GmresState *S, int phase) {
  return !S->done && S->phase == phase;
}

// entries e, e + 1 of p (e even, p 16-byte aligned), zero past n
__device__ __forceinline__ void gm_load2(const double *__restrict__ p, long long e, long long n,
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
__device__ __forceinline__ void gm_store2(double *__restrict__ p, long long e, long long n,
                                          double a, double b) {
  if (e + 1 < n)
    *reinterpret_cast<double2 *>(p + e) = make_double2(a, b);
  else if (e < n)
    p[e] = a;
}

__device__ __forceinline__ double gm_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <int MODE>
__global__ __launch_bounds__(kGmBlock) void k_gm_orth(const GmresState *__restrict__ S,
                                                      double *__restrict__ V, long long ld,
                                                      long long n, double *__restrict__ part,
                                                      int nps) {
  if (!gm_active(S, 0)) return;
  const int j = S->j;
  double *__restrict__ w = V + size_t(j + 1) * ld;
  __shared__ double sm[kGmWaves][kGmVals];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long e[kGmU];
  double wv[2 * kGmU];
#pragma unroll
  for (int u = 0; u < kGmU; u++) {
    e[u] = (long long)blockIdx.x * kGmSlice + u * (2 * kGmBlock) + 2 * threadIdx.x;
    gm_load2(w, e[u], n, wv[2 * u], wv[2 * u + 1]);
  }
  if (MODE != 0) {  // w -= sum c_i V_i: one pass over the basis slice
    const double *__restrict__ c = MODE == 1 ? S->red1 : S->red2;
#pragma unroll 4
    for (int i = 0; i <= j; i++) {
      const double *__restrict__ vi = V + size_t(i) * ld;
      const double ci = c[i];
#pragma unroll
      for (int u = 0; u < kGmU; u++) {
        double a, b;
        gm_load2(vi, e[u], n, a, b);
        wv[2 * u] -= ci * a;
        wv[2 * u + 1] -= ci * b;
      }
    }
#pragma unroll
    for (int u = 0; u < kGmU; u++) gm_store2(w, e[u], n, wv[2 * u], wv[2 * u + 1]);
  }
  int nvals = 0;
  if (MODE != 2) {  // <V_i, w>, kGmJB basis vectors' loads in flight together
    for (int i0 = 0; i0 <= j; i0 += kGmJB) {
      double acc[kGmJB];
#pragma unroll
      for (int q = 0; q < kGmJB; q++) {
        acc[q] = 0.0;
        if (i0 + q <= j) {  // uniform
          const double *__restrict__ vi = V + size_t(i0 + q) * ld;
#pragma unroll
          for (int u = 0; u < kGmU; u++) {
            double a, b;
            gm_load2(vi, e[u], n, a, b);
            acc[q] += a * wv[2 * u];
            acc[q] += b * wv[2 * u + 1];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kGmJB; q++) {
        const double r = gm_wave_sum(acc[q]);
        if (lane == 0 && i0 + q <= j) sm[wave][i0 + q] = r;
      }
    }
    nvals = j + 1;
  }
  if (MODE != 1) {  // <w, w>
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 2 * kGmU; q++) acc += wv[q] * wv[q];
    acc = gm_wave_sum(acc);
    if (lane == 0) sm[wave][nvals] = acc;
    nvals += 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nvals; i += kGmBlock) {
    double s = sm[0][i];
#pragma unroll
    for (int q = 1; q < kGmWaves; q++) s += sm[q][i];
    part[size_t(i) * nps + blockIdx.x] = s;
  }
}

// ||a||^2 partials (value 0) over the same slices; the cycle end's residual norm
__global__ __launch_bounds__(kGmBlock) void k_gm_norm2(const GmresState *__restrict__ S,
                                                       const double *__restrict__ a, long long n,
                                                       double *__restrict__ part) {
  if (!gm_active(S, 1)) return;
  __shared__ double sm[kGmWaves];
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < kGmU; u++) {
    double x0, x1;
    gm_load2(a, (long long)blockIdx.x * kGmSlice + u * (2 * kGmBlock) + 2 * threadIdx.x, n, x0, x1);
    acc += x0 * x0;
    acc += x1 * x1;
  }
  acc = gm_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sm[0];
#pragma unroll
    for (int q = 1; q < kGmWaves; q++) s += sm[q];
    part[blockIdx.x] = s;
  }
}

// workgroup i sums value i's np partials (thread t takes t, t + 256, ... in order, then the fixed
// tree) into red1 (which 0: j + 2 values), red2 (1: j + 1), red3 (2: one, step; 3: one, cycle end)
__global__ __launch_bounds__(kGmBlock) void k_gm_colsum(GmresState *__restrict__ S,
                                                        const double *__restrict__ part, int nps,
                                                        int np, int which) {
  if (!gm_active(S, which == 3 ? 1 : 0)) return;
  const int nvals = which == 0 ? S->j + 2 : (which == 1 ? S->j + 1 : 1);
  const int i = blockIdx.x;
  if (i >= nvals) return;
  __shared__ double sm[kGmWaves];
  double acc = 0.0;
  for (int t = threadIdx.x; t < np; t += kGmBlock) acc += part[size_t(i) * nps + t];
  acc = gm_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sm[0];
#pragma unroll
    for (int q = 1; q < kGmWaves; q++) s += sm[q];
    (which == 0 ? S->red1 : (which == 1 ? S->red2 : S->red3))[i] = s;
  }
}

__global__ void k_gm_hess(GmresState *S, double *hist) {
  if (threadIdx.x == 0) gm_hess_column(S, hist);
}

__global__ void k_gm_backsub(GmresState *S) {
  if (threadIdx.x == 0 && gm_active(S, 1)) gm_backsub(S);
}

__global__ void k_gm_restart(GmresState *S, double *hist, int first) {
  if (threadIdx.x == 0) gm_restart(S, hist, first);
}

// after k_gm_hess: V_{j} *= scale (the column just completed; S->j already counts it);
// after k_gm_restart (src != null): V_0 = src * scale
__global__ __launch_bounds__(kGmBlock) void k_gm_scale(const GmresState *__restrict__ S,
                                                       double *V, long long ld, long long n,
                                                       const double *src) {
  if (src ? !S->fresh : !S->stepped) return;
  double *dst = src ? V : V + size_t(S->j) * ld;  // in place when src is null
  const double *from = src ? src : dst;
  const double sc = S->scale;
#pragma unroll
  for (int u = 0; u < kGmU; u++) {
    const long long e = (long long)blockIdx.x * kGmSlice + u * (2 * kGmBlock) + 2 * threadIdx.x;
    double a, b;
    gm_load2(from, e, n, a, b);
    gm_store2(dst, e, n, a * sc, b * sc);
  }
}

// cycle end: out = (add ? out : 0) + sum_{i < k} y_i B_i, k = S->j, one pass over the basis
__global__ __launch_bounds__(kGmBlock) void k_gm_combine(const GmresState *__restrict__ S,
                                                         const double *__restrict__ B,
                                                         long long ld, long long n,
                                                         double *__restrict__ out, int add) {
  if (!gm_active(S, 1)) return;
  const int k = S->j;
  long long e[kGmU];
  double acc[2 * kGmU];
#pragma unroll
  for (int u = 0; u < kGmU; u++) {
    e[u] = (long long)blockIdx.x * kGmSlice + u * (2 * kGmBlock) + 2 * threadIdx.x;
    acc[2 * u] = acc[2 * u + 1] = 0.0;
    if (add) gm_load2(out, e[u], n, acc[2 * u], acc[2 * u + 1]);
  }
#pragma unroll 4
  for (int i = 0; i < k; i++) {
    const double *__restrict__ bi = B + size_t(i) * ld;
    const double yi = S->y[i];
#pragma unroll
    for (int u = 0; u < kGmU; u++) {
      double a, b;
      gm_load2(bi, e[u], n, a, b);
      acc[2 * u] += yi * a;
      acc[2 * u + 1] += yi * b;
    }
  }
#pragma unroll
  for (int u = 0; u < kGmU; u++) gm_store2(out, e[u], n, acc[2 * u], acc[2 * u + 1]);
}

// cycle end: x += d
__global__ __launch_bounds__(kGmBlock) void k_gm_xpy(const GmresState *__restrict__ S,
                                                     double *__restrict__ x,
                                                     const double *__restrict__ d, long long n) {
  if (!gm_active(S, 1)) return;
#pragma unroll
  for (int u = 0; u < kGmU; u++) {
    const long long e = (long long)blockIdx.x * kGmSlice + u * (2 * kGmBlock) + 2 * threadIdx.x;
    double a, b, c, f;
    gm_load2(x, e, n, a, b);
    gm_load2(d, e, n, c, f);
    gm_store2(x, e, n, a + c, b + f);
  }
}

}  // namespace

int gmres_nparts(long long n) {
  const long long np = (n + kGmSlice - 1) / kGmSlice;
  return np > 0 ? int(np) : 1;
}

hipError_t launch_gmres_orth(int mode, GmresState *S, double *V, long long ld, long long n,
                             double *part, int nps, int jmax, hipStream_t s) {
  const int np = gmres_nparts(n);
  if (np > nps || jmax < 0 || jmax >= kGmMaxRestart || (ld & 1) || ld < n)
    return hipErrorInvalidValue;
  if (mode == 0) {
    k_gm_orth<0><<<np, kGmBlock, 0, s>>>(S, V, ld, n, part, nps);
    k_gm_colsum<<<jmax + 2, kGmBlock, 0, s>>>(S, part, nps, np, 0);
  } else if (mode == 1) {
    k_gm_orth<1><<<np, kGmBlock, 0, s>>>(S, V, ld, n, part, nps);
    k_gm_colsum<<<jmax + 1, kGmBlock, 0, s>>>(S, part, nps, np, 1);
  } else {
    k_gm_orth<2><<<np, kGmBlock, 0, s>>>(S, V, ld, n, part, nps);
    k_gm_colsum<<<1, kGmBlock, 0, s>>>(S, part, nps, np, 2);
  }
  return hipGetLastError();
}

hipError_t launch_gmres_hess(GmresState *S, double *hist, double *V, long long ld, long long n,
                             hipStream_t s) {
  k_gm_hess<<<1, 64, 0, s>>>(S, hist);
  k_gm_scale<<<gmres_nparts(n), kGmBlock, 0, s>>>(S, V, ld, n, nullptr);
  return hipGetLastError();
}

hipError_t launch_gmres_backsub(GmresState *S, hipStream_t s) {
  k_gm_backsub<<<1, 64, 0, s>>>(S);
  return hipGetLastError();
}

hipError_t launch_gmres_combine(const GmresState *S, const double *B, long long ld, long long n,
                                double *out, int add, hipStream_t s) {
  if ((ld & 1) || ld < n) return hipErrorInvalidValue;
  k_gm_combine<<<gmres_nparts(n), kGmBlock, 0, s>>>(S, B, ld, n, out, add);
  return hipGetLastError();
}

hipError_t launch_gmres_xpy(const GmresState *S, double *x, const double *d, long long n,
                            hipStream_t s) {
  k_gm_xpy<<<gmres_nparts(n), kGmBlock, 0, s>>>(S, x, d, n);
  return hipGetLastError();
}

hipError_t launch_gmres_norm2(GmresState *S, const double *a, long long n, double *part, int nps,
                              hipStream_t s) {
  const int np = gmres_nparts(n);
  if (np > nps) return hipErrorInvalidValue;
  k_gm_norm2<<<np, kGmBlock, 0, s>>>(S, a, n, part);
  k_gm_colsum<<<1, kGmBlock, 0, s>>>(S, part, nps, np, 3);
  return hipGetLastError();
}

hipError_t launch_gmres_restart(GmresState *S, double *hist, int first, double *V, long long ld,
                                long long n, const double *r, hipStream_t s) {
  k_gm_restart<<<1, 64, 0, s>>>(S, hist, first);
  k_gm_scale<<<gmres_nparts(n), kGmBlock, 0, s>>>(S, V, ld, n, r);
  return hipGetLastError();
}

}  // namespace pnp
