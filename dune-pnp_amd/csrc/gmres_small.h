// The small dense part of restarted GMRES: the device-resident state block, one Hessenberg column
// (Givens rotations, residual estimate, stop test) and the back-substitution.  Plain C++ shared
// by the one-workgroup kernels of gmres.hip and by the host check program
// (tools/gmres_host_check.cc), which runs it under the host sanitizers.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PNP_GM_HD __host__ __device__
#else
#define PNP_GM_HD
#endif

namespace pnp {

constexpr int kGmMinRestart = 2;
constexpr int kGmMaxRestart = 128;
constexpr int kGmLd = kGmMaxRestart + 1;  // leading dimension of H (column-major)
constexpr int kGmHistCap = 1 << 20;       // steps whose residual norm pnp_solve_history keeps

inline bool gm_restart_valid(long long m) { return m >= kGmMinRestart && m <= kGmMaxRestart; }

// phase: 0 = Arnoldi steps run; 1 = the cycle is over (estimate met the test, restart length or
// maxit reached, breakdown) and the step kernels idle until the host enqueues the cycle end.
// done: 0 running, 1 converged, 2 breakdown, 3 maxit reached.
struct GmresState {
  double reduction, norm0, norm, scale;
  int m, maxit, j, it;
  int phase, done, breakdown, cycles;
  int stepped;  // the last k_gm_hess launch completed a column: the new vector is to be normalised
  int fresh;    // the last k_gm_restart launch opened a cycle: V_0 = r * scale is to be written
  int hcap;     // the history array holds entries 0 .. hcap; later steps are not recorded
  int pad;
  // everything above is the header the host polls
  double red1[kGmMaxRestart + 2];  // <V_i, w> i = 0..j, then <w, w>
  double red2[kGmMaxRestart + 2];  // second pass <V_i, w'>
  double red3[2];                  // ||w''||^2 (steps) / ||r||^2 (cycle end)
  double cs[kGmMaxRestart], sn[kGmMaxRestart], g[kGmMaxRestart + 1], y[kGmMaxRestart];
  double H[kGmLd * kGmMaxRestart];
};

PNP_GM_HD inline bool gm_finite(double v) { return v - v == 0.0; }

// Column j of the Hessenberg matrix from the two orthogonalisation passes: h_i = red1[i] + red2[i],
// h_{j+1} = sqrt(red3[0]).  Applies the previous rotations, forms the new one, updates g, appends
// |g_{j+1}| to the history and ends the cycle when the stop test, the restart length or maxit is
// reached.  A column that is zero or not finite, or a rotation of two zeros (singular A M^-1), is
// breakdown 5: the cycle ends with the columns before it.
PNP_GM_HD inline void gm_hess_column(GmresState *S, double *hist) {
  S->stepped = 0;
  if (S->done || S->phase != 0) return;
  const int j = S->j;
  double *h = S->H + size_t(j) * kGmLd;
  bool ok = gm_finite(S->red1[j + 1]) && S->red1[j + 1] > 0.0 && gm_finite(S->red3[0]);
  for (int i = 0; i <= j; i++) {
    h[i] = S->red1[i] + S->red2[i];
    ok = ok && gm_finite(h[i]);
  }
  const double hn = ok ? std::sqrt(S->red3[0]) : 0.0;
  h[j + 1] = hn;
  if (ok) {
    for (int i = 0; i < j; i++) {
      const double a = h[i], b = h[i + 1];
      h[i] = S->cs[i] * a + S->sn[i] * b;
      h[i + 1] = -S->sn[i] * a + S->cs[i] * b;
    }
    const double d = std::sqrt(h[j] * h[j] + hn * hn);
    ok = d > 0.0 && gm_finite(d);
    if (ok) {
      S->cs[j] = h[j] / d;
      S->sn[j] = hn / d;
      h[j] = d;
      h[j + 1] = 0.0;
      S->g[j + 1] = -S->sn[j] * S->g[j];
      S->g[j] = S->cs[j] * S->g[j];
    }
  }
  if (!ok) {
    S->breakdown = 5;
    S->phase = 1;
    return;
  }
  S->scale = hn > 0.0 ? 1.0 / hn : 0.0;
  S->stepped = 1;
  S->j = j + 1;
  S->it += 1;
  const double est = std::fabs(S->g[j + 1]);
  S->norm = est;
  if (S->it <= S->hcap) hist[S->it] = est;
  if (est < S->reduction * S->norm0 || S->j == S->m || S->it >= S->maxit || hn == 0.0) S->phase = 1;
}

// R y = g for the k = S->j columns of the cycle (R: the rotated H, upper triangular)
PNP_GM_HD inline void gm_backsub(GmresState *S) {
  const int k = S->j;
  for (int i = k - 1; i >= 0; i--) {
    double s = S->g[i];
    for (int c = i + 1; c < k; c++) s -= S->H[size_t(c) * kGmLd + i] * S->y[c];
    S->y[i] = s / S->H[size_t(i) * kGmLd + i];
  }
}

// After the cycle end's residual recompute (red3[0] = ||b - A x||^2): the true norm replaces the
// estimate in the history; stop, or open the next cycle.  first: the solve's start (x = 0).
PNP_GM_HD inline void gm_restart(GmresState *S, double *hist, int first) {
  S->fresh = 0;
  if (S->done || S->phase != 1) return;
  const double nr = std::sqrt(S->red3[0]);
  S->norm = nr;
  if (first) {
    S->norm0 = nr;
    S->it = 0;
  }
  if (S->it <= S->hcap) hist[S->it] = nr;
  if (first && !(nr >= 1e-30)) {
    S->done = gm_finite(nr) ? 1 : 2;
    if (S->done == 2) S->breakdown = 5;
    return;
  }
  if (S->breakdown || !gm_finite(nr)) {
    if (!S->breakdown) S->breakdown = 5;
    S->done = 2;
  } else if (nr < S->reduction * S->norm0) {
    S->done = 1;
  } else if (S->it >= S->maxit) {
    S->done = 3;
  } else {
    S->j = 0;
    S->g[0] = nr;
    S->scale = 1.0 / nr;
    S->phase = 0;
    S->cycles += 1;
    S->fresh = 1;
  }
}

}  // namespace pnp
