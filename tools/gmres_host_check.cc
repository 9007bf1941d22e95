// Host check of the GMRES pieces that need no GPU (dune-pnp_amd/csrc/gmres_small.h): the restart
// range, one Hessenberg column / Givens step, the back-substitution and the cycle logic, driven by
// a dense GMRES(m) on small matrices whose orthogonalisation is done here in plain loops.
// Build and run under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I dune-pnp_amd/csrc tools/gmres_host_check.cc -o /tmp/gmres_host_check && /tmp/gmres_host_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "gmres_small.h"

using pnp::GmresState;

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

// the host loop of krylov.cc gmres() without a preconditioner, on the same state functions
static void solve(const Dense &A, const std::vector<double> &b, int m, double reduction, int maxit,
                  GmresState &S, std::vector<double> &hist, std::vector<double> &x) {
  const int n = A.n;
  S = GmresState{};
  S.reduction = reduction;
  S.m = m;
  S.maxit = maxit;
  S.phase = 1;
  S.hcap = maxit;
  hist.assign(size_t(maxit) + 2, -1.0);
  x.assign(n, 0.0);
  std::vector<double> V(size_t(m + 1) * n), r(b), t(n);
  auto close = [&](int first) {
    double s = 0;
    for (int i = 0; i < n; i++) s += r[i] * r[i];
    S.red3[0] = s;
    pnp::gm_restart(&S, hist.data(), first);
    if (S.fresh)
      for (int i = 0; i < n; i++) V[i] = r[i] * S.scale;
  };
  close(1);
  while (!S.done) {
    while (!S.done && S.phase == 0) {
      const int j = S.j;
      double *w = &V[size_t(j + 1) * n];
      A.mv(&V[size_t(j) * n], w);
      double ww = 0;
      for (int i = 0; i < n; i++) ww += w[i] * w[i];
      S.red1[j + 1] = ww;
      for (int pass = 0; pass < 2; pass++) {
        double *red = pass == 0 ? S.red1 : S.red2;
        for (int c = 0; c <= j; c++) {
          double s = 0;
          for (int i = 0; i < n; i++) s += V[size_t(c) * n + i] * w[i];
          red[c] = s;
        }
        for (int c = 0; c <= j; c++)
          for (int i = 0; i < n; i++) w[i] -= red[c] * V[size_t(c) * n + i];
      }
      double s = 0;
      for (int i = 0; i < n; i++) s += w[i] * w[i];
      S.red3[0] = s;
      pnp::gm_hess_column(&S, hist.data());
      if (S.stepped)
        for (int i = 0; i < n; i++) V[size_t(S.j) * n + i] *= S.scale;
    }
    if (S.done) break;
    pnp::gm_backsub(&S);
    for (int c = 0; c < S.j; c++)
      for (int i = 0; i < n; i++) x[i] += S.y[c] * V[size_t(c) * n + i];
    A.mv(x.data(), t.data());
    for (int i = 0; i < n; i++) r[i] = b[i] - t[i];
    close(0);
  }
}

static double resnorm(const Dense &A, const std::vector<double> &b, const std::vector<double> &x) {
  std::vector<double> t(A.n);
  A.mv(x.data(), t.data());
  double s = 0;
  for (int i = 0; i < A.n; i++) s += (b[i] - t[i]) * (b[i] - t[i]);
  return std::sqrt(s);
}

int main() {
  CHECK(!pnp::gm_restart_valid(1) && pnp::gm_restart_valid(2) && pnp::gm_restart_valid(30) &&
        pnp::gm_restart_valid(128) && !pnp::gm_restart_valid(129) && !pnp::gm_restart_valid(-5));
  auto S = std::make_unique<GmresState>();
  std::vector<double> hist, x;
  // non-symmetric and dense; ~50 to 60 steps to 1e-10, so the short restarts run many cycles
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
  double nb = 0;
  for (double v : b) nb += v * v;
  nb = std::sqrt(nb);
  for (int m : {2, 5, 7, 30, 33, 128}) {
    solve(A, b, m, 1e-10, 5000, *S, hist, x);
    CHECK(S->done == 1 && S->breakdown == 0);
    CHECK(resnorm(A, b, x) < 1.001e-10 * nb);
    CHECK(hist[0] == S->norm0 && hist[size_t(S->it)] == S->norm && hist[size_t(S->it) + 1] == -1.0);
    bool mono = true;  // the estimates never grow inside a cycle
    for (int k = 1; k <= S->it; k++)
      if (k % m != 0 && k != S->it && (k - 1) % m != 0 && hist[k] > hist[k - 1]) mono = false;
    CHECK(mono);
    std::printf("m=%3d: %d iterations, %d cycles, |r|/|b| = %.3e\n", m, S->it, S->cycles,
                resnorm(A, b, x) / nb);
  }
  // maxit smaller than needed: stops unconverged after exactly maxit steps
  solve(A, b, 5, 1e-10, 12, *S, hist, x);
  CHECK(S->done == 3 && S->it == 12 && hist[12] >= 0 && hist[13] == -1.0);
  // zero right-hand side: converged at once
  solve(A, std::vector<double>(n, 0.0), 30, 1e-8, 100, *S, hist, x);
  CHECK(S->done == 1 && S->it == 0 && hist[0] == 0.0 && hist[1] == -1.0);
  // a history shorter than the solve: nothing is written past its capacity
  {
    *S = GmresState{};
    S->reduction = 1e-10, S->m = 5, S->maxit = 40, S->phase = 1, S->hcap = 3;
    std::vector<double> h4(4, -1.0);  // exactly hcap + 1 entries: ASan sees any write beyond
    S->red3[0] = 4.0;
    pnp::gm_restart(S.get(), h4.data(), 1);
    for (int k = 0; k < 5 && S->phase == 0; k++) {
      S->red1[0] = 0.5, S->red2[0] = 0.0;
      for (int i = 1; i <= S->j; i++) S->red1[i] = S->red2[i] = 0.0;
      S->red1[S->j + 1] = 1.0, S->red3[0] = 0.75;
      pnp::gm_hess_column(S.get(), h4.data());
    }
    CHECK(S->it == 5 && h4[3] >= 0.0);
    S->red3[0] = 1.0;
    pnp::gm_restart(S.get(), h4.data(), 0);
    CHECK(S->it == 5);
  }
  // maxit 0
  solve(A, b, 30, 1e-8, 0, *S, hist, x);
  CHECK(S->done == 3 && S->it == 0);
  // singular operator (zero matrix): the first column is zero -> breakdown 5
  Dense Z{4, std::vector<double>(16, 0.0)};
  solve(Z, {1, 2, 3, 4}, 3, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 2 && S->breakdown == 5 && S->it == 0);
  // nilpotent shift: A V_0 is orthogonal to V_0 with h_00 = 0 and the rotation still regular; then
  // the last column vanishes entirely -> breakdown 5, never a division by zero
  Dense N{3, {0, 0, 0, 1, 0, 0, 0, 1, 0}};
  solve(N, {1, 0, 0}, 3, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 2 && S->breakdown == 5);
  // identity: h_{1,0} = 0 with the stop test met is convergence, not breakdown
  Dense I{3, {1, 0, 0, 0, 1, 0, 0, 0, 1}};
  solve(I, {1, 2, 3}, 3, 1e-8, 10, *S, hist, x);
  CHECK(S->done == 1 && S->breakdown == 0 && S->it == 1);
  if (fails) {
    std::printf("%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("gmres_host_check: ok\n");
  return 0;
}
