// Matrix-free Jacobian application on gfx950: y = J(x) z without a stored matrix.
//
// One thread per owned vertex row walks the row's fan exactly as the assembly does (assemble.hip:
// the same element<OP, 1> calls on the same operands in the same order, element.h), but where the
// assembly stores the finished k-form block of slot s (the pending block, the wrap-around block of
// a closed fan, the diagonal block), this kernel expands it (expand_k), applies the row's
// Dirichlet mask (mask_rows) and accumulates y_i += B z_col(s) in fp64.  So the blocks multiplied
// are the blocks the assembly would have stored, and a constrained row gives y_i[f] = z_i[f].
// The gather of a fan neighbour (coordinates, state, frozen fields) also brings its z record.
// The only global stores are y and the dot partials; no atomics.
//
// Fused dots and the residual form have launch_spmv's meaning (kernels.h); the partials are one
// group per workgroup, in workgroup order, summed inside the workgroup in a fixed order.
#include <hip/hip_ext.h>

#include "element.h"
#include "kernels.h"

namespace pnp {

namespace {

constexpr int kJaBlock = 256;

template <int NF>
__device__ __forceinline__ unsigned asm_row_mask(const AsmArgs &a, int row) {
  unsigned dm = 0;
#pragma unroll
  for (int f = 0; f < NF; f++) dm |= unsigned(a.dmask[size_t(row) * NF + f] != 0) << f;
  return dm;
}

// acc += B zj for the finished block K (k-form) of the row: the block the SpMV would multiply
template <int OP>
__device__ __forceinline__ void apply_block(const double *K, unsigned dm, bool diag,
                                            const double *zj, double *acc) {
  using T = OpTraits<OP>;
  constexpr int NF = T::NF, PAT = T::PAT, NV = T::NV;
  double B[NV];
  expand_k<PAT>(K, B);
  mask_rows<NF, PAT>(B, dm, diag);
#pragma unroll
  for (int f = 0; f < NF; f++)
#pragma unroll
    for (int g = 0; g < NF; g++) {
      const int v = pat_index(PAT, f, g);
      if (v >= 0) acc[f] += B[v] * zj[g];
    }
}

// the row's result: residual form, store, fused dots (mode as launch_spmv).  Every thread of the
// workgroup comes here (mode is uniform); the partials of workgroup b are partials[kd b .. kd b + kd)
template <int NF>
__device__ __forceinline__ void finish_row(bool live, int row, double (&acc)[NF], int mode,
                                           double *__restrict__ y, const double *__restrict__ w,
                                           const double *__restrict__ w2,
                                           double *__restrict__ partials) {
  double d[3] = {0, 0, 0};
  if (live) {
    if (mode == 3) {  // residual: y = w - J z
      double wr[NF];
      load_nf<NF>(w, size_t(row), wr);
#pragma unroll
      for (int f = 0; f < NF; f++) acc[f] = wr[f] - acc[f];
    }
    store_nf<NF>(y, size_t(row), acc);
    if (mode == 1 || mode == 2 || mode == 4) {
      double wr[NF];
      load_nf<NF>(w, size_t(row), wr);
#pragma unroll
      for (int f = 0; f < NF; f++) d[0] += acc[f] * wr[f];
    }
    if (mode == 2 || mode == 4) {
#pragma unroll
      for (int f = 0; f < NF; f++) d[1] += acc[f] * acc[f];
    }
    if (mode == 4) {
      double wr[NF];
      load_nf<NF>(w2, size_t(row), wr);
#pragma unroll
      for (int f = 0; f < NF; f++) d[2] += acc[f] * wr[f];
    }
  }
  if (mode == 1 || mode == 2 || mode == 4) {
    // fixed order: the xor tree inside each wave, then the four waves in order
    const int kd = mode == 4 ? 3 : mode;
    __shared__ double sh[kJaBlock / 64][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double v = d[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (int(threadIdx.x) < kd) {
      double t = 0;
      for (int i = 0; i < kJaBlock / 64; i++) t += sh[i][threadIdx.x];
      partials[size_t(kd) * blockIdx.x + threadIdx.x] = t;
    }
  }
}

// The pipelined walk of k_assemble (one element of gathers in flight).  FANR > 0: the row's column
// indices (fans of at most FANR - 1 neighbours) are loaded once into registers; FANR = 0: index
// loads in the walk, any fan length.  DIAG: only the diagonal block is kept and written, unmasked
// and in k-form, to dvals -- one slot per chunk, chunk c at dvals + 64 NK c in the layout of vin()
// (what launch_jacobi reads through a DevLayout whose chunk_off[c] = 64 c); z, y and the dots are
// not touched.
template <int OP, int MINW, int FANR, int DIAG>
__global__ __launch_bounds__(kJaBlock, MINW) void k_jac_apply(
    DevLayout L, AsmArgs a, const double *__restrict__ z, double *__restrict__ y, int mode,
    const double *__restrict__ w, const double *__restrict__ w2, double *__restrict__ partials,
    double *__restrict__ dvals) {
  using T = OpTraits<OP>;
  constexpr int NF = T::NF, NK = T::NK;
  constexpr bool AUX0 = OP == OP_DIFF || OP == OP_DIFF_IE || OP == OP_POISSON;
  constexpr bool AUX1 = OP == OP_POISSON;
  const int row0 = row_block(L, blockIdx.x, gridDim.x) * kJaBlock + threadIdx.x;
  const bool live = row0 < L.n_owned;
  if (DIAG && !live) return;
  const int row = live ? row0 : 0;
  const int chunk = row / kRows, lane = row % kRows;
  const int off = L.chunk_off[chunk];
  const uint64_t meta = L.rowmeta[row];
  const int len = live ? int(meta & 63) : 0;
  const bool closed = live && ((meta >> 6) & 1);
  const unsigned brk = unsigned(meta >> 8);  // fan-break bits, bit s: no element after slot s
  const int *__restrict__ cix = L.colidx + off + lane;

  const double2 pi2 = reinterpret_cast<const double2 *>(L.xy)[row];
  double ui[NF], zi[NF];
  load_nf<NF>(a.x, size_t(row), ui);
  if constexpr (!DIAG) load_nf<NF>(z, size_t(row), zi);
  double ai = 0, aq = 0;
  if constexpr (AUX0) ai = a.aux0[row];
  if constexpr (AUX1) aq = a.aux1[row];
  if constexpr (OP == OP_PB) pb_fifth(ui[0], ai, aq);  // element(): e^{u/5}, e^{-u/5} per vertex
  const unsigned dm = DIAG ? 0u : asm_row_mask<NF>(a, row);

  double R[NF], D[NK], P[NK], F[NK], acc[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) R[f] = acc[f] = 0;
#pragma unroll
  for (int v = 0; v < NK; v++) D[v] = P[v] = F[v] = 0;

  auto next_slot = [&](int s) { return (s + 1 < len) ? s + 1 : (closed ? 1 : -1); };
  auto load_nb = [&](int j, double2 &p, double (&u)[NF], double (&zz)[NF], double &a0,
                     double &a1) {
    p = reinterpret_cast<const double2 *>(L.xy)[j];
    load_nf<NF>(a.x, size_t(j), u);
    if constexpr (!DIAG) load_nf<NF>(z, size_t(j), zz);
    if constexpr (AUX0) a0 = a.aux0[j];
    if constexpr (AUX1) a1 = a.aux1[j];
  };
  double2 pc, pn;                          // coordinates of v_s (current) and v_t (next)
  double uc[NF], un[NF], zc[NF], zn[NF];   // their dofs and z records
  double z1[NF];                           // z of v_1 (the wrap-around block of a closed fan)
  double ac0 = 0, ac1 = 0, an0 = 0, an1 = 0;
  constexpr int NC = FANR > 0 ? FANR : 1;
  int cj[NC];
  if constexpr (FANR > 0) {
#pragma unroll
    for (int k = 1; k < FANR; k++) cj[k] = cix[(k < len ? k : 0) * kRows];  // past the fan: the row
  }
  auto col = [&](int k) -> int {
    if constexpr (FANR > 0)
      return cj[k];
    else
      return cix[k * kRows];
  };
  load_nb(col(1), pc, uc, zc, ac0, ac1);
#pragma unroll
  for (int f = 0; f < NF; f++) z1[f] = DIAG ? 0.0 : zc[f];
  if constexpr (OP == OP_PB) pb_fifth(uc[0], ac0, ac1);
  {
    const int t1 = next_slot(1);
    if (t1 > 0) load_nb(t1 == 1 ? col(1) : col(2), pn, un, zn, an0, an1);
  }
  int jn = -1;  // FANR = 0: column index of the slot needed two elements ahead
  if constexpr (FANR == 0) {
    const int t2 = next_slot(1) > 0 ? next_slot(next_slot(1)) : -1;
    if (t2 > 0 && next_slot(1) != 1) jn = cix[t2 * kRows];
  }
  for (int s = 1; s < len; ++s) {
    const int t = next_slot(s);
    // prefetch the data of the slot the next element needs, and the index after that
    const int tn = (t > 0 && t != 1) ? next_slot(t) : -1;
    double2 pp = pn;
    double up[NF], zp[NF];
    double ap0 = 0, ap1 = 0;
    if (tn > 0) {
      if constexpr (FANR > 0) {
        load_nb(tn == 1 ? col(1) : col(s + 2), pp, up, zp, ap0, ap1);  // tn is s + 2 or a wrap to 1
      } else {
        load_nb(jn, pp, up, zp, ap0, ap1);
        const int tnn = tn != 1 ? next_slot(tn) : -1;
        jn = tnn > 0 ? cix[tnn * kRows] : -1;
      }
    }
    const bool elem = t > 0 && !((brk >> s) & 1);
    if constexpr (OP == OP_PB)
      if (t > 0) pb_fifth(un[0], an0, an1);
    if (elem) {
      Geo G;
      geometry(pi2.x, pi2.y, pc.x, pc.y, pn.x, pn.y, G);
      double Ct[NK];
#pragma unroll
      for (int v = 0; v < NK; v++) Ct[v] = 0;
      // P (pending block of slot s) receives this element's (i, v_s) contribution directly
      element<OP, 1>(a, G, pi2.y, pc.y, pn.y, ui, uc, un, ai, ac0, an0, aq, ac1, an1, R, D, P, Ct);
      if (s == 1 && closed) {
#pragma unroll
        for (int v = 0; v < NK; v++) F[v] = P[v];
      } else if constexpr (!DIAG) {
        apply_block<OP>(P, dm, false, zc, acc);
      }
#pragma unroll
      for (int v = 0; v < NK; v++) P[v] = Ct[v];
    } else {
      if constexpr (!DIAG) apply_block<OP>(P, dm, false, zc, acc);
#pragma unroll
      for (int v = 0; v < NK; v++) P[v] = 0;
    }
    // rotate: v_t becomes the current neighbour, the prefetched one the next
    pc = pn;
#pragma unroll
    for (int f = 0; f < NF; f++) {
      uc[f] = un[f];
      zc[f] = zn[f];
    }
    ac0 = an0;
    ac1 = an1;
    if (tn > 0) {
      pn = pp;
#pragma unroll
      for (int f = 0; f < NF; f++) {
        un[f] = up[f];
        zn[f] = zp[f];
      }
      an0 = ap0;
      an1 = ap1;
    }
  }
  if constexpr (DIAG) {
    store_vals<NK>(dvals + size_t(chunk) * kRows * NK, lane, D);
  } else {
    if (closed) {
#pragma unroll
      for (int v = 0; v < NK; v++) F[v] += P[v];
      apply_block<OP>(F, dm, false, z1, acc);
    }
    apply_block<OP>(D, dm, true, zi, acc);
    finish_row<NF>(live, row, acc, mode, y, w, w2, partials);
  }
}

}  // namespace

// Fans up to 8 neighbours (max_slots <= 9, all meshes seen) and up to 11 (max_slots <= 12): the
// pipelined walk with the column indices in registers (9 or 12 of them); longer fans: index loads
// in the walk (launch_assemble's dispatch).  A gather-all walk (k_assemble_ga's, all neighbours in
// registers before the walk: PNP 224 VGPRs, 2 waves per SIMD) was measured slower, 53.8 against
// 50.5 us per application at config 3, and is not built.
hipError_t launch_jac_apply(const DevLayout &L, const AsmArgs &a, const double *z, double *y,
                            int mode, const double *w, double *partials, int *nparts,
                            hipStream_t s, const double *w2, hipEvent_t t0, hipEvent_t t1) {
  if (L.blkcount < 0) {  // an empty block subset (e.g. a rank without interior blocks)
    if (nparts) *nparts = 0;
    return hipSuccess;
  }
  if (mode < 0 || mode > 4) return hipErrorInvalidValue;
  const dim3 grid(L.blkcount > 0 ? L.blkcount : (L.n_owned + kJaBlock - 1) / kJaBlock),
      block(kJaBlock);
  if (nparts) *nparts = int(grid.x);
  if (L.n_owned == 0) return hipSuccess;
  const int fanr = L.max_slots <= 9 ? 9 : (L.max_slots <= 12 ? 12 : 0);
#define PNP_JA_CASE(OPK)                                                                         \
  case OPK:                                                                                      \
    if (fanr == 9)                                                                               \
      hipExtLaunchKernelGGL((k_jac_apply<OPK, 2, 9, 0>), grid, block, 0, s, t0, t1, 0, L, a, z,  \
                            y, mode, w, w2, partials, (double *)nullptr);                        \
    else if (fanr == 12)                                                                         \
      hipExtLaunchKernelGGL((k_jac_apply<OPK, 2, 12, 0>), grid, block, 0, s, t0, t1, 0, L, a, z, \
                            y, mode, w, w2, partials, (double *)nullptr);                        \
    else                                                                                         \
      hipExtLaunchKernelGGL((k_jac_apply<OPK, 2, 0, 0>), grid, block, 0, s, t0, t1, 0, L, a, z,  \
                            y, mode, w, w2, partials, (double *)nullptr);                        \
    break;
  switch (a.kind) {
    PNP_JA_CASE(OP_PNP)
    PNP_JA_CASE(OP_PNP_IE)
    PNP_JA_CASE(OP_PB)
    PNP_JA_CASE(OP_DIFF)
    PNP_JA_CASE(OP_DIFF_IE)
    PNP_JA_CASE(OP_POISSON)
  default:
    return hipErrorInvalidValue;
  }
#undef PNP_JA_CASE
  return hipGetLastError();
}

// The diagonal blocks alone (the walk keeping only D), for the Jacobi preconditioner without SELL
// values: dvals holds 64 NK nchunks doubles, see k_jac_apply's DIAG form.  Once per linearisation
// point, so one form for every fan length (index loads in the walk).
hipError_t launch_jac_diag(const DevLayout &L, const AsmArgs &a, double *dvals, hipStream_t s) {
  if (L.n_owned == 0) return hipSuccess;
  const dim3 grid((L.n_owned + kJaBlock - 1) / kJaBlock), block(kJaBlock);
  DevLayout all = L;  // every row once, whatever block subset L lists
  all.blkmap = nullptr;
  all.blkcount = 0;
#define PNP_JD_CASE(OPK)                                                                      \
  case OPK:                                                                                   \
    hipLaunchKernelGGL((k_jac_apply<OPK, 2, 0, 1>), grid, block, 0, s, all, a,                \
                       (const double *)nullptr, (double *)nullptr, 0, (const double *)nullptr, \
                       (const double *)nullptr, (double *)nullptr, dvals);                    \
    break;
  switch (a.kind) {
    PNP_JD_CASE(OP_PNP)
    PNP_JD_CASE(OP_PNP_IE)
    PNP_JD_CASE(OP_PB)
    PNP_JD_CASE(OP_DIFF)
    PNP_JD_CASE(OP_DIFF_IE)
    PNP_JD_CASE(OP_POISSON)
  default:
    return hipErrorInvalidValue;
  }
#undef PNP_JD_CASE
  return hipGetLastError();
}

}  // namespace pnp
