// The scalar part of the Chebyshev polynomial preconditioner (PNP_PREC_CHEBYSHEV): option checks,
// the bounds and the recurrence's coefficients.  Plain C++ for the host (ctx.cc computes the
// coefficients and uploads them; the kernels of linalg.hip only read them) and for the host check
// program (tools/cheb_host_check.cc), which runs it under the host sanitizers.  DESIGN.md 4.13.
//
// With theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, T = D^-1 A:
//   r_0 = d, rho_0 = 1 / sigma, p_0 = D^-1 d / theta, z = p_0
//   i = 1 .. k-1:  r_i = r_{i-1} - A p_{i-1},  rho_i = 1 / (2 sigma - rho_{i-1}),
//                  p_i = a_i p_{i-1} + b_i D^-1 r_i,  z += p_i
//   a_i = rho_i rho_{i-1},  b_i = 2 rho_i / delta
#pragma once

#include <cmath>

namespace pnp {

constexpr int kChebMinSteps = 1;
constexpr int kChebMaxSteps = 16;
constexpr int kChebMaxEigIters = 100;
// the device buffer the kernels read: [0] = 1 / theta, [2 i - 1] = a_i, [2 i] = b_i, i = 1 .. k-1
constexpr int kChebCoefDoubles = 2 * kChebMaxSteps;

// pnp_cheb_opts' ranges: steps 1 .. 16, ratio > 1, iterations 1 .. 100, boost >= 1, lambda_max >= 0
// (each comparison written so that a NaN fails it)
inline bool cheb_opts_valid(int steps, double eig_ratio, int eig_iters, double eig_boost,
                            double lambda_max) {
  return steps >= kChebMinSteps && steps <= kChebMaxSteps && eig_ratio > 1.0 &&
         std::isfinite(eig_ratio) && eig_iters >= 1 && eig_iters <= kChebMaxEigIters &&
         eig_boost >= 1.0 && std::isfinite(eig_boost) && lambda_max >= 0.0 &&
         std::isfinite(lambda_max);
}

// lmax = the caller's bound if > 0, else boost x the estimate; lmin = lmax / ratio.  false when
// the result is not a pair of finite bounds lmax > lmin > 0 (a zero or non-finite estimate)
inline bool cheb_bounds(double lambda_user, double lambda_est, double eig_boost, double eig_ratio,
                        double &lmax, double &lmin) {
  lmax = lambda_user > 0.0 ? lambda_user : eig_boost * lambda_est;
  lmin = lmax / eig_ratio;
  return std::isfinite(lmax) && lmin > 0.0 && lmax > lmin;
}

// coef[0 .. kChebCoefDoubles): 1 / theta and the steps - 1 pairs (a_i, b_i); the rest zero
inline bool cheb_coefficients(int steps, double lmax, double lmin, double *coef) {
  for (int q = 0; q < kChebCoefDoubles; q++) coef[q] = 0.0;
  if (steps < kChebMinSteps || steps > kChebMaxSteps) return false;
  if (!(std::isfinite(lmax) && lmin > 0.0 && lmax > lmin)) return false;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
  coef[0] = 1.0 / theta;
  double rho = 1.0 / sigma;
  for (int i = 1; i < steps; i++) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    coef[2 * i - 1] = rho_new * rho;
    coef[2 * i] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
  return true;
}

}  // namespace pnp
