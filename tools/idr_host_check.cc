// Host check of the IDR(s) pieces that need no GPU (dune-pnp_amd/csrc/idr_small.h): the range of
// s, the shadow entries, the triangular solves, the M column, beta, omega, the stop, breakdown and
// residual-replacement logic, driven by a dense IDR(s) on small matrices whose vector work is done
// here in plain loops, in the order the kernels of idr.hip do it.
// Build and run under the host sanitizers:
//   make -C dune-pnp_amd idr_host_check
// With a file argument it solves the system in that file (n s reduction maxit, then A row-major,
// b, P column-major, whitespace-separated) and prints "done it replacements breakdown" and the
// history, one value per line: tests/test_idr_ref.py compares that with the numpy yardstick.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "idr_small.h"

using pnp::IdrState;
using pnp::kIdrMaxS;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      fails++;                                                    \
    }                                                             \
  } while (0)

struct Dense {
  int n;
  std::vector<double> a;  // row-major
  void mv(const double *x, double *y) const {
    for (int i = 0; i < n; i++) {
      double s = 0;
      for (int k = 0; k < n; k++) s += a[size_t(i) * n + k] * x[k];
      y[i] = s;
    }
  }
};

static double dot(const double *a, const double *b, int n) {
  double s = 0;
  for (int i = 0; i < n; i++) s += a[i] * b[i];
  return s;
}

// the shadow matrix as krylov.cc builds it: counter-based entries, modified Gram-Schmidt
static std::vector<double> shadow(int n, int s) {
  std::vector<double> P(size_t(n) * s);
  for (int j = 0; j < s; j++)
    for (int i = 0; i < n; i++) P[size_t(j) * n + i] = pnp::idr_shadow_entry(i, 0, j);
  for (int j = 0; j < s; j++) {
    double *pj = &P[size_t(j) * n];
    for (int i = 0; i < j; i++) {
      const double d = dot(&P[size_t(i) * n], pj, n);
      for (int q = 0; q < n; q++) pj[q] -= d * P[size_t(i) * n + q];
    }
    const double sc = 1.0 / std::sqrt(dot(pj, pj, n));
    for (int q = 0; q < n; q++) pj[q] *= sc;
  }
  return P;
}

// the host loop of krylov.cc idr() without a preconditioner, on the same state functions.  fake > 0:
// the recurrence's norm^2 is scaled by it (the residual-replacement path: the recurrence claims
// convergence early, the true residual disagrees).
static void solve(const Dense &A, const std::vector<double> &b, const std::vector<double> &P, int s,
                  double reduction, int maxit, IdrState &S, std::vector<double> &hist,
                  std::vector<double> &x, double fake = 0.0) {
  const int n = A.n;
  S = IdrState{};
  S.reduction = reduction;
  S.omega = 1.0;
  S.s = s;
  S.maxit = maxit;
  S.phase = 2;
  S.hcap = maxit;
  hist.assign(size_t(maxit) + 2, -1.0);
  x.assign(n, 0.0);
  std::vector<double> G(size_t(s) * n), U(size_t(s) * n), r(b), v(n), t(n);
  auto begin = [&](int first) {
    S.red[0] = dot(r.data(), r.data(), n);
    for (int i = 0; i < s; i++) S.red[1 + i] = dot(&P[size_t(i) * n], r.data(), n);
    std::fill(G.begin(), G.end(), 0.0);
    std::fill(U.begin(), U.end(), 0.0);
    pnp::idr_begin(&S, hist.data(), first);
  };
  begin(1);
  while (!S.done) {
    while (!S.done && S.phase != 2) {
      if (S.phase == 0) {
        const int k = S.k;
        double *gk = &G[size_t(k) * n], *uk = &U[size_t(k) * n];
        for (int q = 0; q < n; q++) {
          double a = r[q];
          for (int i = k; i < s; i++) a -= S.c[i] * G[size_t(i) * n + q];
          v[q] = a;
        }
        for (int q = 0; q < n; q++) {
          double a = S.omega * v[q];
          for (int i = k; i < s; i++) a += S.c[i] * U[size_t(i) * n + q];
          uk[q] = a;
        }
        A.mv(uk, gk);
        for (int i = 0; i < s; i++) S.red[i] = dot(&P[size_t(i) * n], gk, n);
        pnp::idr_step_a(&S, k);
        if (S.phase != 0) break;
        for (int q = 0; q < n; q++) {
          for (int i = 0; i < k; i++) {
            gk[q] -= S.alpha[i] * G[size_t(i) * n + q];
            uk[q] -= S.alpha[i] * U[size_t(i) * n + q];
          }
          r[q] -= S.beta * gk[q];
          x[q] += S.beta * uk[q];
        }
        S.red[0] = dot(r.data(), r.data(), n) * (fake > 0 ? fake : 1.0);
        pnp::idr_step_b(&S, hist.data(), k);
      } else {
        A.mv(r.data(), t.data());
        S.red[0] = dot(t.data(), r.data(), n);
        S.red[1] = dot(t.data(), t.data(), n);
        S.red[2] = dot(r.data(), r.data(), n);
        pnp::idr_omega(&S);
        if (S.phase != 1) break;
        for (int q = 0; q < n; q++) {
          x[q] += S.omega * r[q];
          r[q] -= S.omega * t[q];
        }
        S.red[0] = dot(r.data(), r.data(), n) * (fake > 0 ? fake : 1.0);
        for (int i = 0; i < s; i++) S.red[1 + i] = dot(&P[size_t(i) * n], r.data(), n);
        pnp::idr_omega_end(&S, hist.data());
      }
    }
    if (S.done) break;
    A.mv(x.data(), t.data());
    for (int i = 0; i < n; i++) r[i] = b[i] - t[i];
    begin(0);
  }
}

static double resnorm(const Dense &A, const std::vector<double> &b, const std::vector<double> &x) {
  std::vector<double> t(A.n);
  A.mv(x.data(), t.data());
  double s = 0;
  for (int i = 0; i < A.n; i++) s += (b[i] - t[i]) * (b[i] - t[i]);
  return std::sqrt(s);
}

static int solve_file(const char *path) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) return 2;
  int n = 0, s = 0, maxit = 0;
  double reduction = 0;
  if (std::fscanf(f, "%d %d %lf %d", &n, &s, &reduction, &maxit) != 4 || n < 1 || n > 4096 ||
      !pnp::idr_s_valid(s) || maxit < 0 || maxit > (1 << 20)) {
    std::fclose(f);
    return 2;
  }
  Dense A{n, std::vector<double>(size_t(n) * n)};
  std::vector<double> b(n), P(size_t(n) * s);
  bool ok = true;
  for (double &v : A.a) ok = ok && std::fscanf(f, "%lf", &v) == 1;
  for (double &v : b) ok = ok && std::fscanf(f, "%lf", &v) == 1;
  for (double &v : P) ok = ok && std::fscanf(f, "%lf", &v) == 1;
  std::fclose(f);
  if (!ok) return 2;
  auto S = std::make_unique<IdrState>();
  std::vector<double> hist, x;
  solve(A, b, P, s, reduction, maxit, *S, hist, x);
  std::printf("%d %d %d %d\n", S->done, S->it, S->replacements, S->breakdown);
  for (int k = 0; k <= S->it; k++) std::printf("%.17g\n", hist[size_t(k)]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1) return solve_file(argv[1]);
  CHECK(!pnp::idr_s_valid(0) && pnp::idr_s_valid(1) && pnp::idr_s_valid(4) && pnp::idr_s_valid(8) &&
        !pnp::idr_s_valid(9) && !pnp::idr_s_valid(-3));
  {  // shadow entries: inside (-1, 1), distinct across vertex, field and column, mean near 0
    double mean = 0, lo = 1, hi = -1;
    for (int g = 0; g < 4000; g++)
      for (int f = 0; f < 3; f++)
        for (int j = 0; j < 8; j++) {
          const double v = pnp::idr_shadow_entry(g, f, j);
          mean += v;
          lo = v < lo ? v : lo;
          hi = v > hi ? v : hi;
        }
    mean /= 4000.0 * 24;
    CHECK(lo > -1.0 && hi < 1.0 && lo < -0.999 && hi > 0.999 && std::fabs(mean) < 0.01);
    CHECK(pnp::idr_shadow_entry(5, 1, 2) != pnp::idr_shadow_entry(5, 2, 1));
    CHECK(pnp::idr_shadow_entry(0, 0, 0) != pnp::idr_shadow_entry(1, 0, 0));
    CHECK(pnp::idr_shadow_entry(1ull << 40, 2, 7) == pnp::idr_shadow_entry(1ull << 40, 2, 7));
  }
  auto S = std::make_unique<IdrState>();
  std::vector<double> hist, x;
  const int n = 150;
  Dense A{n, std::vector<double>(size_t(n) * n, 0.0)};
  std::vector<double> b(n);
  unsigned long long seed = 12345;
  auto rnd = [&] {
    seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
    return double(seed >> 11) / double(1ULL << 53) - 0.5;
  };
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < n; k++) A.a[size_t(i) * n + k] = 0.9 * rnd();
    A.a[size_t(i) * n + i] += 3.3 + 0.02 * i;
    b[i] = rnd();
  }
  double nb = std::sqrt(dot(b.data(), b.data(), n));
  for (int s = 1; s <= kIdrMaxS; s++) {
    const std::vector<double> P = shadow(n, s);
    for (int i = 0; i < s; i++)
      for (int j = 0; j <= i; j++)
        CHECK(std::fabs(dot(&P[size_t(i) * n], &P[size_t(j) * n], n) - (i == j)) < 1e-14);
    solve(A, b, P, s, 1e-10, 5000, *S, hist, x);
    CHECK(S->done == 1 && S->breakdown == 0);
    CHECK(resnorm(A, b, x) < 1.001e-10 * nb);
    CHECK(hist[0] == S->norm0 && hist[size_t(S->it)] == S->norm && hist[size_t(S->it) + 1] == -1.0);
    std::printf("s=%d: %d applications, %d cycles, %d replacements, |r|/|b| = %.3e\n", s, S->it,
                S->cycles, S->replacements, resnorm(A, b, x) / nb);
  }
  const std::vector<double> P4 = shadow(n, 4);
  // finite termination: n + n / s applications at the most in exact arithmetic
  {
    const int m = 24;
    Dense B{m, std::vector<double>(size_t(m) * m)};
    std::vector<double> c(m);
    for (int i = 0; i < m; i++) {
      for (int k = 0; k < m; k++) B.a[size_t(i) * m + k] = 0.9 * rnd();
      B.a[size_t(i) * m + i] += 4.0;
      c[i] = rnd();
    }
    solve(B, c, shadow(m, 4), 4, 1e-10, 200, *S, hist, x);
    CHECK(S->done == 1 && S->it <= m + m / 4 + 2);
  }
  // maxit smaller than s: unconverged after exactly maxit applications, the true norm reported
  solve(A, b, P4, 4, 1e-10, 3, *S, hist, x);
  CHECK(S->done == 3 && S->it == 3 && hist[3] >= 0 && hist[4] == -1.0);
  CHECK(std::fabs(hist[3] - resnorm(A, b, x)) <= 1e-12 * nb);
  // maxit in the middle of a later cycle
  solve(A, b, P4, 4, 1e-10, 12, *S, hist, x);
  CHECK(S->done == 3 && S->it == 12 && hist[12] >= 0 && hist[13] == -1.0);
  // zero right-hand side: converged at once
  solve(A, std::vector<double>(n, 0.0), P4, 4, 1e-8, 100, *S, hist, x);
  CHECK(S->done == 1 && S->it == 0 && hist[0] == 0.0 && hist[1] == -1.0);
  // maxit 0
  solve(A, b, P4, 4, 1e-8, 0, *S, hist, x);
  CHECK(S->done == 3 && S->it == 0);
  // residual replacement: a recurrence norm reported 1e6 times too small meets the test early,
  // the true residual does not, and the solve goes on from it; with the lie kept up it gives up
  // after kIdrMaxReplace replacements, unconverged and without a breakdown
  solve(A, b, P4, 4, 1e-10, 5000, *S, hist, x, 1e-12);
  CHECK(S->done == 3 && S->breakdown == 0 && S->replacements == pnp::kIdrMaxReplace);
  CHECK(resnorm(A, b, x) < 1e-3 * nb);  // every replacement still made progress
  // a history shorter than the solve: nothing is written past its capacity
  {
    *S = IdrState{};
    S->reduction = 1e-10, S->s = 2, S->maxit = 40, S->phase = 2, S->hcap = 2, S->omega = 1.0;
    std::vector<double> h3(3, -1.0);  // exactly hcap + 1 entries: ASan sees any write beyond
    S->red[0] = 4.0, S->red[1] = 1.0, S->red[2] = 0.5;
    pnp::idr_begin(S.get(), h3.data(), 1);
    CHECK(S->phase == 0 && S->k == 0 && h3[0] == 2.0);
    for (int cyc = 0; cyc < 2; cyc++) {
      for (int k = 0; k < 2; k++) {
        S->red[0] = k == 0 ? 1.0 : 0.25, S->red[1] = 0.5;
        pnp::idr_step_a(S.get(), k);
        S->red[0] = 3.0;
        pnp::idr_step_b(S.get(), h3.data(), k);
      }
      S->red[0] = 1.0, S->red[1] = 2.0, S->red[2] = 3.0;
      pnp::idr_omega(S.get());
      S->red[0] = 2.0, S->red[1] = 1.0, S->red[2] = 0.5;
      pnp::idr_omega_end(S.get(), h3.data());
    }
    CHECK(S->it == 6 && S->breakdown == 0 && h3[2] >= 0.0);
  }
  // a step enqueued for another k, or in another phase, changes nothing
  {
    solve(A, b, P4, 4, 1e-10, 2, *S, hist, x);
    IdrState before = *S;
    pnp::idr_step_a(S.get(), 1);
    pnp::idr_step_b(S.get(), hist.data(), 1);
    pnp::idr_omega(S.get());
    pnp::idr_omega_end(S.get(), hist.data());
    pnp::idr_begin(S.get(), hist.data(), 0);
    CHECK(S->it == before.it && S->done == before.done && S->norm == before.norm);
  }
  // singular operator (zero matrix): G_0 = 0, the pivot M[0,0] = 0 -> breakdown 6
  Dense Z{4, std::vector<double>(16, 0.0)};
  solve(Z, {1, 2, 3, 4}, shadow(4, 2), 2, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 2 && S->breakdown == 6 && S->it == 0);
  // a non-finite operator: breakdown 6, never a hang
  Dense Q{2, {1.0, 0.0, 0.0, 1.0 / 0.0}};
  solve(Q, {1, 1}, shadow(2, 1), 1, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 2 && S->breakdown == 6);
  // skew-symmetric: <t, r> = 0 in the omega step -> omega = 0 or 0/0 -> breakdown 6
  Dense K{2, {0.0, 1.0, -1.0, 0.0}};
  solve(K, {1, 0}, shadow(2, 1), 1, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 2 && S->breakdown == 6);
  // identity: one application converges, no breakdown
  Dense I{3, {1, 0, 0, 0, 1, 0, 0, 0, 1}};
  solve(I, {1, 2, 3}, shadow(3, 2), 2, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 1 && S->breakdown == 0 && S->it == 1);
  if (fails) {
    std::printf("%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("idr_host_check: ok\n");
  return 0;
}
