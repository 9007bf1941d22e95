// Element arithmetic of the P1 operators, shared by the assembly (assemble.hip) and the matrix-free
// Jacobian application (jac_apply.hip): geometry and closed-form integrals of one fan element, and
// element(): its contributions to the residual and to the k-form blocks of row i.  Internal to the
// kernels' translation units (everything here is file-local).
#pragma once

#include "kernels.h"

namespace pnp {

namespace {

struct Geo {
  double gi0, gi1, gb0, gb1, gc0, gc1;  // physical gradients of the P1 basis at i, b, c
  double adet;
};

__device__ __forceinline__ void geometry(double xi, double yi, double xb, double yb, double xc,
                                         double yc, Geo &G) {
  double J00 = xb - xi, J01 = xc - xi, J10 = yb - yi, J11 = yc - yi;
  double det = J00 * J11 - J01 * J10;
  double id = 1.0 / det;
  G.gb0 = J11 * id;
  G.gb1 = -J01 * id;
  G.gc0 = -J10 * id;
  G.gc1 = J00 * id;
  G.gi0 = -G.gb0 - G.gc0;
  G.gi1 = -G.gb1 - G.gc1;
  G.adet = fabs(det);
}

// cylindrical/planar integrals of the P1 basis on the element (i, b, c):
//   W = int w, m_j = int w psi_j, M_ij = int w psi_i psi_j  (w = 2*PI*y or 1)
struct Ints {
  double W, mi, mb, mc, Mii, Mib, Mic;
};
__device__ __forceinline__ void integrals(const Geo &G, int cyl, double pi, double yi, double yb,
                                          double yc, Ints &I) {
  if (cyl) {
    double c = 2 * pi * G.adet;
    double Y = yi + yb + yc;
    I.W = c * Y * (1.0 / 6.0);
    I.mi = c * (Y + yi) * (1.0 / 24.0);
    I.mb = c * (Y + yb) * (1.0 / 24.0);
    I.mc = c * (Y + yc) * (1.0 / 24.0);
    I.Mii = c * (yi * (1.0 / 20.0) + (yb + yc) * (1.0 / 60.0));
    I.Mib = c * ((yi + yb) * (1.0 / 60.0) + yc * (1.0 / 120.0));
    I.Mic = c * ((yi + yc) * (1.0 / 60.0) + yb * (1.0 / 120.0));
  } else {
    I.W = G.adet * 0.5;
    I.mi = I.mb = I.mc = G.adet * (1.0 / 6.0);
    I.Mii = G.adet * (1.0 / 12.0);
    I.Mib = I.Mic = G.adet * (1.0 / 24.0);
  }
}

// order-2 (3-point) rule mass, (PnpTOperator, src/pnp_toperator.hh:26 / dune-geometry order 2);
// barycentric points (1/6, 2/3, 1/6) and permutations, weight 1/6 * |det| * (2 PI y)
__device__ __forceinline__ void mass_q2(const Geo &G, int cyl, double pi, double yi, double yb,
                                        double yc, double &Mii, double &Mib, double &Mic) {
  Mii = Mib = Mic = 0;
  const double a = 1.0 / 6.0, b = 2.0 / 3.0;
  const double P[3][3] = {{a, b, a}, {a, a, b}, {b, a, a}};
#pragma unroll
  for (int q = 0; q < 3; q++) {
    double f = (1.0 / 6.0) * G.adet;
    if (cyl) f *= (P[q][0] * yi + P[q][1] * yb + P[q][2] * yc) * 2 * pi;
    Mii += f * P[q][0] * P[q][0];
    Mib += f * P[q][0] * P[q][1];
    Mic += f * P[q][0] * P[q][2];
  }
}

template <int OP>
struct OpTraits {
  static constexpr int NF = (OP == OP_PNP || OP == OP_PNP_IE) ? 3 : 1;
  static constexpr int PAT = OP == OP_PNP ? kPatPnp : (OP == OP_PNP_IE ? kPatPnpIE : kPatScalar);
  static constexpr int NV = popc9(PAT);
  // independent coefficients of one block (i, j) while it accumulates over the fan:
  //   PNP: k0 = sum G_ij W, k1 = sum kappa M_ij, k2 = sum G_ij S+, k3 = sum G_ij S-,
  //        k4 = sum (grad phi . grad psi_i) m_j, (PNP_IE) k5 = sum tau M2_ij, scaled by dt;
  //   these are what the matrix stores (k-form, kernels.h expand_k)
  static constexpr int NK = nks_of(PAT);
};

// PBOperator: a vertex's e^{u/5} and e^{-u/5}, the factors element() builds the quadrature
// points' e^u from
__device__ __forceinline__ void pb_fifth(double u, double &e, double &ei) {
  e = exp(0.2 * u);
  ei = 1.0 / e;
}

// Contributions of element (i, b, c) to row i: residual res[NF], blocks (i,i), (i,b), (i,c).
// KC (PNP): the state-independent coefficients k0 and k1 are not accumulated (the
// assembly that leaves their stored planes alone, assemble.hip); the others are untouched.
template <int OP, int JAC, int KC = 0>
__device__ __forceinline__ void element(const AsmArgs &a, const Geo &G, double yi, double yb,
                                        double yc, const double *ui, const double *ub,
                                        const double *uc, double pi_, double pb_, double pc_,
                                        double qi, double qb, double qc, double *res, double *Bd,
                                        double *Bb, double *Bc) {
  const double PI = a.pi;
  double Gii = G.gi0 * G.gi0 + G.gi1 * G.gi1;
  double Gib = G.gb0 * G.gi0 + G.gb1 * G.gi1;
  double Gic = G.gc0 * G.gi0 + G.gc1 * G.gi1;
  if constexpr (OP == OP_PNP || OP == OP_PNP_IE) {
    Ints I;
    integrals(G, a.cylindrical, PI, yi, yb, yc, I);
    double gph0 = ui[0] * G.gi0 + ub[0] * G.gb0 + uc[0] * G.gc0;
    double gph1 = ui[0] * G.gi1 + ub[0] * G.gb1 + uc[0] * G.gc1;
    double gcp0 = ui[1] * G.gi0 + ub[1] * G.gb0 + uc[1] * G.gc0;
    double gcp1 = ui[1] * G.gi1 + ub[1] * G.gb1 + uc[1] * G.gc1;
    double gcm0 = ui[2] * G.gi0 + ub[2] * G.gb0 + uc[2] * G.gc0;
    double gcm1 = ui[2] * G.gi1 + ub[2] * G.gb1 + uc[2] * G.gc1;
    double gp = gph0 * G.gi0 + gph1 * G.gi1;
    double Sp = ui[1] * I.mi + ub[1] * I.mb + uc[1] * I.mc;
    double Sm = ui[2] * I.mi + ub[2] * I.mb + uc[2] * I.mc;
    double kap = 4 * PI * a.l_b;
    double sc = (OP == OP_PNP_IE) ? a.dt : 1.0;
    res[0] += sc * (gp * I.W + kap * ((ui[1] - ui[2]) * I.Mii + (ub[1] - ub[2]) * I.Mib +
                                      (uc[1] - uc[2]) * I.Mic));
    res[1] += sc * ((gcp0 * G.gi0 + gcp1 * G.gi1) * I.W - gp * Sp);
    res[2] += sc * ((gcm0 * G.gi0 + gcm1 * G.gi1) * I.W + gp * Sm);
    double M2ii = 0, M2ib = 0, M2ic = 0;
    if constexpr (OP == OP_PNP_IE) {
      mass_q2(G, a.cylindrical, PI, yi, yb, yc, M2ii, M2ib, M2ic);
      res[1] += a.tau * ((ui[1] + ui[2]) * M2ii + (ub[1] + ub[2]) * M2ib + (uc[1] + uc[2]) * M2ic);
    }
    if constexpr (JAC) {
      auto blk = [&](double *B, double Gij, double Mij, double mj, double M2ij) {
        if constexpr (!KC) {
          B[0] += sc * Gij * I.W;
          B[1] += sc * kap * Mij;
        }
        B[2] += sc * Gij * Sp;
        B[3] += sc * Gij * Sm;
        B[4] += sc * gp * mj;
        if constexpr (OP == OP_PNP_IE) B[5] += a.tau * M2ij;
      };
      blk(Bd, Gii, I.Mii, I.mi, M2ii);
      blk(Bb, Gib, I.Mib, I.mb, M2ib);
      blk(Bc, Gic, I.Mic, I.mc, M2ic);
    }
  } else if constexpr (OP == OP_PB) {
    // 4-point order-3 rule, barycentric (psi_i, psi_b, psi_c)
    const double P[4][3] = {{1.0 / 3, 1.0 / 3, 1.0 / 3}, {0.2, 0.6, 0.2}, {0.2, 0.2, 0.6},
                            {0.6, 0.2, 0.2}};
    const double w[4] = {0.5 * -27.0 / 48.0, 0.5 * 25.0 / 48.0, 0.5 * 25.0 / 48.0,
                         0.5 * 25.0 / 48.0};
    double gu0 = ui[0] * G.gi0 + ub[0] * G.gb0 + uc[0] * G.gc0;
    double gu1 = ui[0] * G.gi1 + ub[0] * G.gb1 + uc[0] * G.gc1;
    double gg = gu0 * G.gi0 + gu1 * G.gi1;
    double beta = 8 * PI * a.l_b * a.c0;
    // sinh and cosh at each point from e^u and e^-u (the library's sinh and cosh each cost about
    // two exps; the PB launch is issue-bound on them).  The walk passes each vertex's e^{u/5} and
    // e^{-u/5} (pi_, pb_, pc_ / qi, qb, qc), computed once per vertex of the fan: the three
    // off-centre points are fifths, (0.2, 0.6, 0.2) and its rotations, so there e^u is a product
    // of them; only the centroid takes an exp and a division of its own.  Errors: a few ulps of
    // e^|u|, absolute in the sinh term, against residual terms of at least that size.
    const double Eq = pi_ * pb_ * pc_, Iq = qi * qb * qc;
    const double eu[4] = {exp(P[0][0] * ui[0] + P[0][1] * ub[0] + P[0][2] * uc[0]), Eq * pb_ * pb_,
                          Eq * pc_ * pc_, Eq * pi_ * pi_};
    const double ei[4] = {1.0 / eu[0], Iq * qb * qb, Iq * qc * qc, Iq * qi * qi};
    double W = 0, Ri = 0, Jii = 0, Jib = 0, Jic = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      double f = w[q] * G.adet;
      if (a.cylindrical) f *= (P[q][0] * yi + P[q][1] * yb + P[q][2] * yc) * 2 * PI;
      W += f;
      Ri += f * (0.5 * (eu[q] - ei[q])) * P[q][0];
      if constexpr (JAC) {
        double ch = f * (0.5 * (eu[q] + ei[q])) * P[q][0];
        Jii += ch * P[q][0];
        Jib += ch * P[q][1];
        Jic += ch * P[q][2];
      }
    }
    res[0] += gg * W + beta * Ri;
    if constexpr (JAC) {
      Bd[0] += Gii * W + beta * Jii;
      Bb[0] += Gib * W + beta * Jib;
      Bc[0] += Gic * W + beta * Jic;
    }
  } else if constexpr (OP == OP_DIFF || OP == OP_DIFF_IE) {
    // DiffusionOperator: no cylindrical weight (quirk Q8); grad Phi of the frozen potential
    double W = G.adet * 0.5, m = G.adet * (1.0 / 6.0);
    double gu0 = ui[0] * G.gi0 + ub[0] * G.gb0 + uc[0] * G.gc0;
    double gu1 = ui[0] * G.gi1 + ub[0] * G.gb1 + uc[0] * G.gc1;
    double gP0 = pi_ * G.gi0 + pb_ * G.gb0 + pc_ * G.gc0;
    double gP1 = pi_ * G.gi1 + pb_ * G.gb1 + pc_ * G.gc1;
    double gpP = gP0 * G.gi0 + gP1 * G.gi1;
    double sc = (OP == OP_DIFF_IE) ? a.dt : 1.0;
    res[0] += sc * ((gu0 * G.gi0 + gu1 * G.gi1) * W + a.z * gpP * m * (ui[0] + ub[0] + uc[0]));
    double Mii = G.adet * (1.0 / 12.0), Mij = G.adet * (1.0 / 24.0);
    if constexpr (OP == OP_DIFF_IE) res[0] += ui[0] * Mii + (ub[0] + uc[0]) * Mij;
    if constexpr (JAC) {
      Bd[0] += sc * (Gii * W + a.z * gpP * m);
      Bb[0] += sc * (Gib * W + a.z * gpP * m);
      Bc[0] += sc * (Gic * W + a.z * gpP * m);
      if constexpr (OP == OP_DIFF_IE) {
        Bd[0] += Mii;
        Bb[0] += Mij;
        Bc[0] += Mij;
      }
    }
  } else {  // OP_POISSON: frozen c+ (aux0 -> pi_, ..) and c- (aux1 -> qi, ..)
    Ints I;
    integrals(G, a.cylindrical, PI, yi, yb, yc, I);
    double gu0 = ui[0] * G.gi0 + ub[0] * G.gb0 + uc[0] * G.gc0;
    double gu1 = ui[0] * G.gi1 + ub[0] * G.gb1 + uc[0] * G.gc1;
    double kap = a.l_b * 4 * PI;
    res[0] += (gu0 * G.gi0 + gu1 * G.gi1) * I.W +
              kap * ((qi - pi_) * I.Mii + (qb - pb_) * I.Mib + (qc - pc_) * I.Mic);
    if constexpr (JAC) {
      Bd[0] += Gii * I.W;
      Bb[0] += Gib * I.W;
      Bc[0] += Gic * I.W;
    }
  }
}

}  // namespace

}  // namespace pnp
