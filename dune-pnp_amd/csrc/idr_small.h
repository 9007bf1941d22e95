// The small dense part of IDR(s): the device-resident state block, the triangular solves on the
// s x s matrix M = P^T G, the scalar steps (beta, omega), the breakdown and stop tests.  Plain C++
// shared by the one-thread kernels of idr.hip and by the host check program
// (tools/idr_host_check.cc), which runs it under the host sanitizers.  DESIGN.md 4.10.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PNP_IDR_HD __host__ __device__
#else
#define PNP_IDR_HD
#endif

namespace pnp {

constexpr int kIdrMinS = 1;
constexpr int kIdrMaxS = 8;
constexpr int kIdrDefaultS = 4;
constexpr int kIdrMaxReplace = 8;        // residual replacements before the solve gives up
constexpr int kIdrHistCap = 1 << 20;     // applications whose residual norm pnp_solve_history keeps
constexpr double kIdrAngle = 0.7;        // omega's "maintaining the convergence" threshold
constexpr unsigned long long kIdrSeed = 0x1d72a5b3c4e6f809ull;  // of the shadow vectors

inline bool idr_s_valid(long long s) { return s >= kIdrMinS && s <= kIdrMaxS; }

// phase: 0 = step k of the dimension-reduction loop runs; 1 = the omega step runs; 2 = the
// recurrence is over (its norm met the test, maxit, breakdown) and every step kernel idles until
// the host has enqueued the true residual and idr_begin has judged it.
// done: 0 running, 1 converged, 2 breakdown, 3 unconverged (maxit or too many replacements).
struct IdrState {
  double reduction, norm0, norm, omega;
  int s, maxit, k, it;
  int phase, done, breakdown, cycles;
  int replacements, hcap, pad0, pad1;
  // everything above is the header the host polls
  double red[kIdrMaxS + 4];  // the current reduction's sums (after the allreduce)
  double beta;
  double M[kIdrMaxS * kIdrMaxS];  // row-major, lower triangular: column i is P^T G_i
  double f[kIdrMaxS], c[kIdrMaxS], alpha[kIdrMaxS];
};

PNP_IDR_HD inline bool idr_finite(double v) { return v - v == 0.0; }

// counter-based shadow entry in (-1, 1): splitmix64's finaliser over (global vertex, field,
// column, seed), so the matrix does not depend on row order, colouring or partition
PNP_IDR_HD inline double idr_shadow_entry(unsigned long long g, unsigned f, unsigned j) {
  unsigned long long z = kIdrSeed + 0x9e3779b97f4a7c15ull * (g * 64ull + f * 8ull + j + 1ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  // 53 bits -> [0, 1) -> (-1, 1); the half-ulp offset keeps both ends open
  return ((double)(z >> 11) + 0.5) * (2.0 / 9007199254740992.0) - 1.0;
}

// lower-triangular M[k:, k:] c[k:] = f[k:] (forward substitution); false when a pivot is zero or
// not finite
PNP_IDR_HD inline bool idr_solve_c(IdrState *S) {
  const int s = S->s, k = S->k;
  for (int i = k; i < s; i++) {
    double v = S->f[i];
    for (int j = k; j < i; j++) v -= S->M[i * kIdrMaxS + j] * S->c[j];
    const double d = S->M[i * kIdrMaxS + i];
    if (!(d != 0.0) || !idr_finite(d)) return false;
    S->c[i] = v / d;
  }
  return true;
}

PNP_IDR_HD inline void idr_end(IdrState *S, int breakdown) {
  if (breakdown) S->breakdown = breakdown;
  S->phase = 2;
}

// After red[0 .. s) = P^T (A U_k): alpha from M[:k, :k] alpha = q[:k], column k of M from
// q[k:] - M[k:, :k] alpha, beta = f_k / M[k, k].  Breakdown 6 on a zero or non-finite pivot.
PNP_IDR_HD inline void idr_step_a(IdrState *S, int hk) {
  if (S->done || S->phase != 0 || S->k != hk) return;
  const int s = S->s, k = S->k;
  const double *q = S->red;
  for (int i = 0; i < k; i++) {
    double v = q[i];
    for (int j = 0; j < i; j++) v -= S->M[i * kIdrMaxS + j] * S->alpha[j];
    S->alpha[i] = v / S->M[i * kIdrMaxS + i];  // pivots of earlier steps: tested then
  }
  for (int i = k; i < s; i++) {
    double v = q[i];
    for (int j = 0; j < k; j++) v -= S->M[i * kIdrMaxS + j] * S->alpha[j];
    S->M[i * kIdrMaxS + k] = v;
  }
  const double piv = S->M[k * kIdrMaxS + k];
  if (!(piv != 0.0) || !idr_finite(piv)) {
    idr_end(S, 6);
    return;
  }
  S->beta = S->f[k] / piv;
  if (!idr_finite(S->beta)) idr_end(S, 6);
}

// the recurrence's norm after an application: history, counters, the stop test
PNP_IDR_HD inline bool idr_record(IdrState *S, double *hist, double nr2) {
  const double nr = std::sqrt(nr2);
  S->norm = nr;
  S->it += 1;
  if (S->it <= S->hcap) hist[S->it] = nr;
  if (!idr_finite(nr)) {
    idr_end(S, 6);
    return false;
  }
  if (nr < S->reduction * S->norm0 || S->it >= S->maxit) {
    idr_end(S, 0);
    return false;
  }
  return true;
}

// After red[0] = ||r||^2 of the updated residual: f[:k+1] = 0, f[k+1:] -= beta M[k+1:, k], next k
// (or the omega step) and its c.
PNP_IDR_HD inline void idr_step_b(IdrState *S, double *hist, int hk) {
  if (S->done || S->phase != 0 || S->k != hk) return;
  const int s = S->s, k = S->k;
  if (!idr_record(S, hist, S->red[0])) return;
  for (int i = 0; i <= k; i++) S->f[i] = 0.0;
  for (int i = k + 1; i < s; i++) S->f[i] -= S->beta * S->M[i * kIdrMaxS + k];
  if (k + 1 == s) {
    S->phase = 1;
    return;
  }
  S->k = k + 1;
  if (!idr_solve_c(S)) idr_end(S, 6);
}

// After red[0 .. 3) = <t, r>, <t, t>, <r, r>: omega with the angle safeguard.  Breakdown 6 when
// omega is zero or not finite.
PNP_IDR_HD inline void idr_omega(IdrState *S) {
  if (S->done || S->phase != 1) return;
  const double tr = S->red[0], tt = S->red[1], rr = S->red[2];
  double om = tr / tt;
  const double rho = tr / (std::sqrt(tt) * std::sqrt(rr));
  const double ar = std::fabs(rho);
  if (ar < kIdrAngle) om *= kIdrAngle / ar;
  if (!(om != 0.0) || !idr_finite(om)) {
    idr_end(S, 6);
    return;
  }
  S->omega = om;
}

// After red[0] = ||r||^2, red[1 .. s] = P^T r of the omega step's residual: the next cycle
PNP_IDR_HD inline void idr_omega_end(IdrState *S, double *hist) {
  if (S->done || S->phase != 1) return;
  if (!idr_record(S, hist, S->red[0])) return;
  for (int i = 0; i < S->s; i++) S->f[i] = S->red[1 + i];
  S->k = 0;
  S->phase = 0;
  S->cycles += 1;
  if (!idr_solve_c(S)) idr_end(S, 6);
}

// After the true residual r = b - A x (red[0] = ||r||^2, red[1 .. s] = P^T r): the solve's start
// (first: x = 0, r = b), or the verdict on a recurrence that ended.  The true norm replaces the
// recurrence's in the history.  If the solve goes on, it does so from this residual with
// G = U = 0 (the host clears them), M = I, omega = 1: a residual replacement.
PNP_IDR_HD inline void idr_begin(IdrState *S, double *hist, int first) {
  if (S->done || S->phase != 2) return;
  const double nr = std::sqrt(S->red[0]);
  S->norm = nr;
  if (first) {
    S->norm0 = nr;
    S->it = 0;
  }
  if (S->it <= S->hcap) hist[S->it] = nr;
  if (first && !(nr >= 1e-30)) {
    S->done = idr_finite(nr) ? 1 : 2;
    if (S->done == 2) S->breakdown = 6;
    return;
  }
  if (S->breakdown || !idr_finite(nr)) {
    if (!S->breakdown) S->breakdown = 6;
    S->done = 2;
    return;
  }
  if (!first && nr < S->reduction * S->norm0) {
    S->done = 1;
    return;
  }
  if (S->it >= S->maxit || (!first && S->replacements >= kIdrMaxReplace)) {
    S->done = 3;
    return;
  }
  if (!first) S->replacements += 1;
  for (int i = 0; i < kIdrMaxS * kIdrMaxS; i++) S->M[i] = 0.0;
  for (int i = 0; i < kIdrMaxS; i++) {
    S->M[i * kIdrMaxS + i] = 1.0;
    S->f[i] = i < S->s ? S->red[1 + i] : 0.0;
    S->c[i] = S->alpha[i] = 0.0;
  }
  S->omega = 1.0;
  S->beta = 0.0;
  S->k = 0;
  S->phase = 0;
  S->cycles += 1;
  idr_solve_c(S);  // M = I
}

}  // namespace pnp
