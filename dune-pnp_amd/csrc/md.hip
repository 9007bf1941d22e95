// The streaming kernels of the device-resident operator-split loop (pnp_md_run, md.cc): one
// thread per row, 256-thread workgroups, no atomics.  Scalar vectors in the internal layout.
#include "kernels.h"

namespace pnp {
namespace {

constexpr int kMdBlock = 256;

inline dim3 md_grid(int n) { return dim3((n + kMdBlock - 1) / kMdBlock); }

// StationaryLinearProblemSolver::apply's update x -= z on the owned rows
__global__ __launch_bounds__(kMdBlock) void k_md_sub(int n, const double *__restrict__ z,
                                                     double *__restrict__ x) {
  const int i = blockIdx.x * kMdBlock + threadIdx.x;
  if (i >= n) return;
  x[i] = x[i] - z[i];
}

// cvec = load + s r1 (r1 null: cvec = load).  Two roundings, the product and then the sum, as
// the host-driven loop makes them (r1 *= s, then load + c_extra): no fused multiply-add
__global__ __launch_bounds__(kMdBlock) void k_md_load(int n, const double *__restrict__ load,
                                                      double s, const double *__restrict__ r1,
                                                      double *__restrict__ cvec) {
  const int i = blockIdx.x * kMdBlock + threadIdx.x;
  if (i >= n) return;
  cvec[i] = r1 ? __dadd_rn(load[i], __dmul_rn(r1[i], s)) : load[i];
}

// phi, c+, c- -> the 3-field interleaved vector of the flux kernels (n rows: ghosts included)
__global__ __launch_bounds__(kMdBlock) void k_md_pack(int n, const double *__restrict__ phi,
                                                      const double *__restrict__ cp,
                                                      const double *__restrict__ cm,
                                                      double *__restrict__ x3) {
  const int i = blockIdx.x * kMdBlock + threadIdx.x;
  if (i >= n) return;
  x3[size_t(i) * 3] = phi[i];
  x3[size_t(i) * 3 + 1] = cp[i];
  x3[size_t(i) * 3 + 2] = cm[i];
}

// and back: the uploaded 3-field state into the three resident vectors
__global__ __launch_bounds__(kMdBlock) void k_md_unpack(int n, const double *__restrict__ x3,
                                                        double *__restrict__ phi,
                                                        double *__restrict__ cp,
                                                        double *__restrict__ cm) {
  const int i = blockIdx.x * kMdBlock + threadIdx.x;
  if (i >= n) return;
  phi[i] = x3[size_t(i) * 3];
  cp[i] = x3[size_t(i) * 3 + 1];
  cm[i] = x3[size_t(i) * 3 + 2];
}

}  // namespace

hipError_t launch_md_sub(int n, const double *z, double *x, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_md_sub, md_grid(n), dim3(kMdBlock), 0, s, n, z, x);
  return hipGetLastError();
}

hipError_t launch_md_load(int n, const double *load, double scale, const double *r1, double *cvec,
                          hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_md_load, md_grid(n), dim3(kMdBlock), 0, s, n, load, scale, r1, cvec);
  return hipGetLastError();
}

hipError_t launch_md_pack(int n, const double *phi, const double *cp, const double *cm, double *x3,
                          hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_md_pack, md_grid(n), dim3(kMdBlock), 0, s, n, phi, cp, cm, x3);
  return hipGetLastError();
}

hipError_t launch_md_unpack(int n, const double *x3, double *phi, double *cp, double *cm,
                            hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_md_unpack, md_grid(n), dim3(kMdBlock), 0, s, n, x3, phi, cp, cm);
  return hipGetLastError();
}

}  // namespace pnp
