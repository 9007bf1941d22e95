// Host check of the Chebyshev preconditioner's scalar part (dune-pnp_amd/csrc/cheb_small.h): the
// option ranges, the bounds, and the coefficients -- the recurrence run with them on scalars must
// reproduce the Chebyshev residual polynomial 1 - lambda q(lambda) = T_k((theta - lambda) / delta)
// / T_k(sigma) and its bound 1 / T_k(sigma) on [lmin, lmax].
// Build and run under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I dune-pnp_amd/csrc tools/cheb_host_check.cc -o /tmp/cheb_host_check && /tmp/cheb_host_check
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cheb_small.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      fails++;                                                    \
    }                                                             \
  } while (0)

// T_k(x) by the three-term recurrence (any real x)
static double cheb_T(int k, double x) {
  double t0 = 1.0, t1 = x;
  if (k == 0) return t0;
  for (int i = 2; i <= k; i++) {
    const double t2 = 2.0 * x * t1 - t0;
    t0 = t1;
    t1 = t2;
  }
  return t1;
}

// z = q(lambda) d of the scalar "system" A = lambda, D = 1, by the kernels' recurrence
static double apply_scalar(int steps, const double *coef, double lambda, double d) {
  double r = d, p = d * coef[0], z = p;
  for (int i = 1; i < steps; i++) {
    r -= lambda * p;
    p = coef[2 * i - 1] * p + coef[2 * i] * r;
    z += p;
  }
  return z;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();
  // option ranges
  CHECK(pnp::cheb_opts_valid(3, 10.0, 20, 1.1, 0.0));
  CHECK(pnp::cheb_opts_valid(1, 1.0001, 1, 1.0, 2.5));
  CHECK(pnp::cheb_opts_valid(16, 1e6, 100, 4.0, 0.0));
  CHECK(!pnp::cheb_opts_valid(0, 10.0, 20, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(17, 10.0, 20, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, 1.0, 20, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, nan, 20, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, inf, 20, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, 10.0, 0, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, 10.0, 101, 1.1, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, 10.0, 20, 0.99, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, 10.0, 20, nan, 0.0));
  CHECK(!pnp::cheb_opts_valid(3, 10.0, 20, 1.1, -1.0));
  CHECK(!pnp::cheb_opts_valid(3, 10.0, 20, 1.1, nan));
  // bounds
  double lmax = 0, lmin = 0;
  CHECK(pnp::cheb_bounds(0.0, 2.0, 1.1, 10.0, lmax, lmin) && lmax == 1.1 * 2.0 &&
        lmin == lmax / 10.0);
  CHECK(pnp::cheb_bounds(2.5, 7.0, 1.1, 10.0, lmax, lmin) && lmax == 2.5 && lmin == 0.25);
  CHECK(!pnp::cheb_bounds(0.0, 0.0, 1.1, 10.0, lmax, lmin));
  CHECK(!pnp::cheb_bounds(0.0, nan, 1.1, 10.0, lmax, lmin));
  CHECK(!pnp::cheb_bounds(0.0, inf, 1.1, 10.0, lmax, lmin));
  // coefficients: refusals leave the buffer zero
  std::vector<double> coef(pnp::kChebCoefDoubles, 7.0);
  CHECK(!pnp::cheb_coefficients(0, 2.0, 0.2, coef.data()));
  CHECK(!pnp::cheb_coefficients(17, 2.0, 0.2, coef.data()));
  CHECK(!pnp::cheb_coefficients(3, 2.0, 2.0, coef.data()));
  CHECK(!pnp::cheb_coefficients(3, 2.0, 0.0, coef.data()));
  CHECK(!pnp::cheb_coefficients(3, nan, 0.2, coef.data()));
  for (double c : coef) CHECK(c == 0.0);
  // the recurrence against the closed form, every step count, several intervals
  const double ratios[] = {1.5, 10.0, 30.0, 1e3};
  const double tops[] = {0.7, 1.65 * 1.1, 2.5, 40.0};
  for (double ratio : ratios)
    for (double top : tops)
      for (int k = 1; k <= pnp::kChebMaxSteps; k++) {
        const double lo = top / ratio;
        CHECK(pnp::cheb_coefficients(k, top, lo, coef.data()));
        const double theta = 0.5 * (top + lo), delta = 0.5 * (top - lo), sigma = theta / delta;
        CHECK(std::fabs(coef[0] * theta - 1.0) <= 1e-15);
        for (int q = 2 * k - 1; q < pnp::kChebCoefDoubles; q++) CHECK(coef[q] == 0.0);
        const double tk = cheb_T(k, sigma);
        for (int s = 0; s <= 64; s++) {
          // inside the interval, and a little outside on both sides (the closed form holds there too)
          const double lam = lo * 0.5 + (top * 1.05 - lo * 0.5) * s / 64.0;
          const double z = apply_scalar(k, coef.data(), lam, 1.0);
          const double res = 1.0 - lam * z, want = cheb_T(k, (theta - lam) / delta) / tk;
          CHECK(std::fabs(res - want) <= 1e-9 * (1.0 + std::fabs(want)));
          // (1e-12: the rounding floor of 1 - lam z where 1 / T_k(sigma) is below it)
          if (lam >= lo && lam <= top) CHECK(std::fabs(res) <= (1.0 + 1e-9) / tk + 1e-12);
        }
      }
  // steps 1 is 1 / theta alone
  CHECK(pnp::cheb_coefficients(1, 2.0, 0.2, coef.data()));
  CHECK(std::fabs(apply_scalar(1, coef.data(), 1.0, 3.0) - 3.0 / 1.1) <= 1e-15);
  if (fails) {
    std::printf("cheb_host_check: %d check(s) failed\n", fails);
    return 1;
  }
  std::printf("cheb_host_check: ok\n");
  return 0;
}
