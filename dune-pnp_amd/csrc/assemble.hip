// Residual + Jacobian assembly on gfx950: owner-computes, atomic-free, one thread per vertex row.
//
// The reference assembles element by element (PDELab GridOperator over alpha_volume, e.g.
// src/pnp_operator.hh:46-195) and differentiates by forward differences (NumericalJacobianVolume,
// 10 residual evaluations per PNP element), scatter-adding 81 values per element into a BCRS
// matrix.  Here each thread owns one vertex row i and walks the CCW fan of triangles around i
// (mesh.cc build_fans): element (i, v_s, v_{s+1}) contributes to row i's diagonal block, to
// block (i, v_s) and to block (i, v_{s+1}).  Block (i, v_s) only ever receives contributions
// from the two fan elements on either side of edge (i, v_s), which are consecutive in the walk,
// so it is complete after step s: it is kept in registers ("pending"), finished, and stored
// exactly once.  Slot s of the SELL row is the s-th fan neighbour, so at step s every lane of a
// wave stores slot s: all block stores are coalesced 512-byte lines and there are no atomics.
//
// Element integrals are the closed forms of the reference's order-3 quadrature where that rule
// is exact (PnpOperator / PoissonOperator integrands are polynomials of degree <= 3, also with
// the cylindrical 2*PI*y weight); PBOperator (sinh) and the PnpTOperator mass (a cubic under the
// order-2 rule, src/pnp_toperator.hh:26) use the reference's quadrature points explicitly.
#include <cstdlib>

#include <hip/hip_ext.h>

#include "element.h"
#include "kernels.h"

namespace pnp {

namespace {

// store one block's coefficients (k-form, OpTraits::NK values, unmasked: the Dirichlet rows are
// applied by the consumers, see kernels.h expand_k / mask_rows)
// KC (PNP): the slot's first 16-B record (k0, k1: geometry and l_b only) already holds this
// operator's values and is left alone; records 1.. are written -- (k2, k3) as one dwordx4 and
// k4.  Kc[0] and Kc[1] are not read.  The record is 1 KiB per 64-row slot, whole 128-B lines.
template <int OP, int KC = 0>
__device__ __forceinline__ void store_block(double *__restrict__ vc, int lane, int s,
                                            const double *Kc) {
  constexpr int NK = OpTraits<OP>::NK;
  static_assert(!KC || OP == OP_PNP, "constant planes: the PNP operator only");
  constexpr int Q0 = KC ? 2 : 0;
  // non-temporal: the blocks are read back only by later kernels (SpMV, split), which stream
  // them non-temporally too; plain stores allocate the 207 MB in the caches and evict the
  // gathered x / xy / column indices.  94 -> 77 us at config 3 (profiles/r01/ab_asm_nt_stores.log)
#ifdef ASM_STORE_PLAIN  // A/B build flag: plain (allocating) block stores
  store_vals<NK, Q0>(vc + size_t(s) * NK * kRows, lane, Kc);
#else
  store_vals_nt<NK, Q0>(vc + size_t(s) * NK * kRows, lane, Kc);
#endif
}

// r = mask(R + cvec) of one row.  fl = the row's flag byte (AsmArgs::rowflag): the constant load is
// zero except on flux-boundary rows (and on every row of an implicit Euler operator), so only
// flagged rows read cvec; the others add the +0.0 the load would have returned (the add stays:
// -0.0 + 0.0 = +0.0).  The mask is the flag's low bits.
template <int NF>
__device__ __forceinline__ void residual_tail(const AsmArgs &a, int row, unsigned fl,
                                              const double (&R)[NF]) {
  double cv[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) cv[f] = 0.0;
  if (fl & kRowFlagLoad) {
#pragma unroll
    for (int f = 0; f < NF; f++) cv[f] = a.cvec[size_t(row) * NF + f];
  }
#pragma unroll
  for (int f = 0; f < NF; f++) {
    const double rv = R[f] + cv[f];
    a.r[size_t(row) * NF + f] = ((fl >> f) & 1) ? 0.0 : rv;
  }
}

// One thread per owned vertex row.  JAC = 0: residual only (Newton line search).
// FANR > 0: the row's column indices (fans of at most FANR - 1 neighbours) are loaded once into
// registers, so the fan walk issues no dependent index loads.  On gfx9-family ISAs vmcnt counts
// loads and stores in issue order: an index load issued behind an element's SELL block stores
// could not be consumed before those stores drained (the FANR = 0 path waits vmcnt(0) per
// element).
// (Non-temporal loads of the once-read row streams -- fan metadata, column indices, constant
// load, mask -- and a non-temporal residual store: 77 -> 96 us, profiles/r01/ab_asm_nt_row_streams.log)
template <int OP, int JAC, int MINW, int FANR>
__global__ __launch_bounds__(256, MINW) void k_assemble(DevLayout L, AsmArgs a) {
  using T = OpTraits<OP>;
  constexpr int NF = T::NF, NK = T::NK;
  const int row = xcd_block(blockIdx.x, gridDim.x, L.xcd_remap) * blockDim.x + threadIdx.x;
  if (row >= L.n_owned) return;
  const int chunk = row / kRows, lane = row % kRows;
  const int off = L.chunk_off[chunk];
  const uint64_t meta = L.rowmeta[row];
  const int len = int(meta & 63);
  const bool closed = (meta >> 6) & 1;
  const unsigned brk = unsigned(meta >> 8);  // fan-break bits, bit s: no element after slot s
  const int *__restrict__ cix = L.colidx + off + lane;
  double *__restrict__ vc = a.vals + size_t(off) * NK;  // chunk base (k-form), see vin()

  const double2 pi2 = reinterpret_cast<const double2 *>(L.xy)[row];
  double ui[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) ui[f] = a.x[size_t(row) * NF + f];
  double ai = 0, aq = 0;
  if constexpr (OP == OP_DIFF || OP == OP_DIFF_IE || OP == OP_POISSON) ai = a.aux0[row];
  if constexpr (OP == OP_POISSON) aq = a.aux1[row];
  if constexpr (OP == OP_PB) pb_fifth(ui[0], ai, aq);  // element(): e^{u/5}, e^{-u/5} per vertex

  double R[NF], D[NK], P[NK], F[NK];  // block coefficients, see OpTraits::NK
#pragma unroll
  for (int f = 0; f < NF; f++) R[f] = 0;
#pragma unroll
  for (int v = 0; v < NK; v++) D[v] = P[v] = F[v] = 0;

  // Software-pipelined fan walk.  Element s is (i, v_s, v_t) with t = s+1 (or 1 when a closed
  // fan wraps); consecutive elements share v_{s+1}, so each neighbour's data (coordinates, NF
  // dofs, frozen fields) is gathered once, one element ahead, and its column index two ahead.
  auto next_slot = [&](int s) { return (s + 1 < len) ? s + 1 : (closed ? 1 : -1); };
  auto load_nb = [&](int j, double2 &p, double (&u)[NF], double &a0, double &a1) {
    p = reinterpret_cast<const double2 *>(L.xy)[j];
    load_nf<NF>(a.x, size_t(j), u);
    if constexpr (OP == OP_DIFF || OP == OP_DIFF_IE || OP == OP_POISSON) a0 = a.aux0[j];
    if constexpr (OP == OP_POISSON) a1 = a.aux1[j];
  };
  double2 pc, pn;               // coordinates of v_s (current) and v_t (next)
  double uc[NF], un[NF];        // dofs of v_s, v_t
  double ac0 = 0, ac1 = 0, an0 = 0, an1 = 0;
  constexpr int NC = FANR > 0 ? FANR : 1;
  int cj[NC];
  if constexpr (FANR > 0) {
#pragma unroll
    // branch-free: past the fan, slot 0 (the diagonal, column = row) is read instead, so all
    // index loads issue back to back (guarded loads were serialised by the register allocator)
    for (int k = 1; k < FANR; k++) cj[k] = cix[(k < len ? k : 0) * kRows];
  }
  // column of slot k (FANR path: k is the wave-uniform s + c, or 1 after a wrap)
  auto col = [&](int k) -> int {
    if constexpr (FANR > 0)
      return cj[k];
    else
      return cix[k * kRows];
  };
  load_nb(col(1), pc, uc, ac0, ac1);
  if constexpr (OP == OP_PB) pb_fifth(uc[0], ac0, ac1);
  {
    const int t1 = next_slot(1);
    if (t1 > 0) load_nb(t1 == 1 ? col(1) : col(2), pn, un, an0, an1);
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
    double up[NF];
    double ap0 = 0, ap1 = 0;
    if (tn > 0) {
      if constexpr (FANR > 0) {
        load_nb(tn == 1 ? col(1) : col(s + 2), pp, up, ap0, ap1);  // tn is s + 2 or a wrap to 1
      } else {
        load_nb(jn, pp, up, ap0, ap1);
        const int tnn = tn != 1 ? next_slot(tn) : -1;
        jn = tnn > 0 ? cix[tnn * kRows] : -1;
      }
    }
    const bool elem = t > 0 && !((brk >> s) & 1);
    // v_t's e^{u/5} for this element and, rotated into v_s, the next one
    if constexpr (OP == OP_PB)
      if (t > 0) pb_fifth(un[0], an0, an1);
    if (elem) {
      Geo G;
      geometry(pi2.x, pi2.y, pc.x, pc.y, pn.x, pn.y, G);
      double Ct[NK];
#pragma unroll
      for (int v = 0; v < NK; v++) Ct[v] = 0;
      // P (pending block of slot s) receives this element's (i, v_s) contribution directly
      element<OP, JAC>(a, G, pi2.y, pc.y, pn.y, ui, uc, un, ai, ac0, an0, aq, ac1, an1, R, D, P,
                       Ct);
      if constexpr (JAC) {
        if (s == 1 && closed) {
#pragma unroll
          for (int v = 0; v < NK; v++) F[v] = P[v];
        } else {
          store_block<OP>(vc, lane, s, P);
        }
#pragma unroll
        for (int v = 0; v < NK; v++) P[v] = Ct[v];
      }
    } else if constexpr (JAC) {
      store_block<OP>(vc, lane, s, P);
#pragma unroll
      for (int v = 0; v < NK; v++) P[v] = 0;
    }
    // rotate: v_t becomes the current neighbour, the prefetched one the next
    pc = pn;
#pragma unroll
    for (int f = 0; f < NF; f++) uc[f] = un[f];
    ac0 = an0;
    ac1 = an1;
    if (tn > 0) {
      pn = pp;
#pragma unroll
      for (int f = 0; f < NF; f++) un[f] = up[f];
      an0 = ap0;
      an1 = ap1;
    }
  }
  if constexpr (JAC) {
    if (closed) {
#pragma unroll
      for (int v = 0; v < NK; v++) F[v] += P[v];
      store_block<OP>(vc, lane, 1, F);
    }
    store_block<OP>(vc, lane, 0, D);
  }
  residual_tail<NF>(a, row, a.rowflag[row], R);
}

// Gather-all variant (GA): every neighbour's data (coordinates, NF dofs, frozen fields) of the
// row's fan is loaded into registers before the walk, so the gathers of the whole fan are in
// flight together (one memory round trip per row instead of one per element; the pipelined walk
// above keeps ~1 element of loads in flight), and the block stores of the walk never sit in front
// of a load the walk still waits for.  Same element() calls with the same operands in the same
// order as k_assemble (the compiler's FMA contraction may still differ in the last bit).  Fans of
// at most FANR - 1 neighbours.  Rows come in the spatial block order (row_block, DevLayout::
// blkmap), so an XCD's rows share the neighbours they gather in its L2.  Config 3: pipelined walk
// 76.5 us; gather-all at 2 waves/SIMD (180 VGPRs) 72.2 us, with the block map 58.5 us; slots 1-5
// first and 6-8 after element 4 (SPLIT 6) fits 3 waves in 160 VGPRs: 54.5 us
// (profiles/r01/ab_asm_gather_all.log, ab_blkmap_gather_all.log, ab_asm_ga_split_blkmap.log).
// SPLIT < FANR: only slots 1 .. SPLIT-1 are gathered up front; the rest are issued after element
// SPLIT-2, when the first elements' neighbour registers are free again (fewer live VGPRs).
// LDSG: the fan neighbours' coordinates, dofs and frozen fields come from LDS, where the
// workgroup first gathered them once per distinct column of its 256 rows (DevLayout::uptr /
// ulist / lidx, as the LDS-staged SpMV): half the scattered gathers of the direct walk.
#ifndef ASM_SU
#define ASM_SU 4  // staged list entries per thread issued together (build-flag A/B knob)
#endif
template <int OP>
__host__ __device__ constexpr int asm_lds_rec() {  // doubles per staged column
  return 2 + OpTraits<OP>::NF + (OP == OP_DIFF || OP == OP_DIFF_IE || OP == OP_POISSON) +
         (OP == OP_POISSON);
}
// KC (PNP, JAC): the block coefficients k0 / k1 depend on the mesh and l_b only, so the planes
// an earlier full assembly of this operator stored are still right (AsmArgs::kconst, kept by the
// context): this instantiation neither accumulates nor stores them (store_block), 82.5 of the
// 207 MB write stream at config 3.  k2.. and the residual are computed as without KC, bitwise.
// 148 VGPRs, no spill, 3 waves per SIMD; at 4 waves (128 VGPRs) it spills 33-36 VGPRs and runs
// 74 us warm against 44.  PNP_IE has the same planes (scaled by dt), but there the compiler
// contracts k2..k4 differently without the k0 / k1 accumulators (one ulp in a few blocks), so it
// keeps writing every plane.
template <int OP>
constexpr int asm_kc() {  // 1: the operator's blocks have state-independent planes
  return OP == OP_PNP;
}
// PIPE (PNP_ASM_PIPE=1; off by default): a persistent grid of G workgroups (G a multiple of 8,
// so a workgroup stays on its XCD's spatial slice); workgroup b walks the logical 256-row tiles
// b, b + G, ... of row_block().  Every wave is on its own (no barrier, atomic or flag).  While a wave walks tile t,
// the per-row inputs of its 64 rows of the next tile -- 8 column indices, the two rowmeta dwords
// and the flag byte's dword -- are on their way into the wave's own kPipeDw * 256 bytes of LDS by
// LDS-DMA, issued once the wave has read tile t's values out of that region (one buffer per wave).
// The wave-uniform block map entries and chunk offsets run two tiles ahead in scalar registers.
// At the top of a tile the wave reads its indices from LDS and issues its own xy / x loads and
// the slot 1 .. SPLIT-1 gathers together: one exposed round trip per tile instead of four in
// sequence (blkmap, chunk_off, rowmeta + indices, gathers).  The walk itself is the same code:
// 166 VGPRs, no spill, the direct walk's fp64 instruction multiset, bitwise its results.
// Measured at config 3 it is slower, 44.1 us warm against 39.6, at every grid size: the wait for
// the DMA loads is a wait for the previous tile's stores too (vmcnt retires in issue order), and
// a resident grid walks 4 tiles where dynamic dispatch balances to 3.75.
constexpr int kPipeDw = 11;  // dwords per lane of the prefetch region
template <class P>
__device__ __forceinline__ void lds_dma4(const P *src, uint32_t *dst_wave) {
  // 4 bytes per lane from src (per lane) to dst_wave (wave-uniform) + 4 * lane
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void *)(src),
      (__attribute__((address_space(3))) void *)(dst_wave), 4, 0, 0);
}
// a wave-uniform load of layout data that no kernel writes: from the constant address space, so
// it is a scalar load whatever the kernel stores in between
__device__ __forceinline__ int const_ld(const int *p, int i) {
  return ((const __attribute__((address_space(4))) int *)(p))[i];
}
__device__ __forceinline__ int row_block_const(const DevLayout &L, int b, int nwg) {  // row_block
  return L.blkmap ? const_ld(L.blkmap, xcd_block(b, nwg, 1)) : xcd_block(b, nwg, L.xcd_remap);
}
// REG (PNP_ASM_REGULAR=1, the default; OP_PNP, the direct constant-planes Jacobian walk): a wave
// whose live rows are all closed six-neighbour fans without a break (rowmeta: len 7, closed, no
// break bit -- a wave vote, so the branch is scalar) walks its six elements (i,v1,v2) .. (i,v5,v6),
// (i,v6,v1) with static slots: no s < len / has_next / closed / brk tests and no wrap selects, 6
// index loads and 6 gathers instead of 8 and 8 (slots 7 and 8 of such a row re-read the row
// itself).  All of them and the flag byte are issued before the first store, so no later wait
// drains the block stores, and a wave without a flagged row ends without waiting for them.  The
// geometry() / element() calls, their operands and their order, the F / P / D handling and the
// store order are the general walk's for such a row, and the fp64 instruction multiset is that of
// the general walk unrolled for six neighbours (tools/isa_regs.py with -DASM_REGULAR_CHECK) plus
// the adds of a second residual tail: the same bits.  Every other wave falls through to the
// general walk below.  160 VGPRs, no spill.  The full-write instantiation (KC = 0, once per
// operator) has ten more accumulator registers live and spills with it (11 VGPRs): it keeps the
// general walk for every wave.
template <int OP>
constexpr int asm_reg() {  // 1: the operator has the regular walk
  return OP == OP_PNP;
}
constexpr int kRegSlots = 7;  // slots of a regular row: the diagonal and six neighbours
template <int OP, int JAC, int MINW, int FANR, int SPLIT = FANR, int STAGE = 0, int LDSG = 0,
          int KC = 0, int PIPE = 0, int REG = 0>
__global__ __launch_bounds__(256, MINW) void k_assemble_ga(DevLayout L, AsmArgs a) {
  using T = OpTraits<OP>;
  constexpr int NF = T::NF, NK = T::NK, NS = FANR;
  constexpr bool AUX0 = OP == OP_DIFF || OP == OP_DIFF_IE || OP == OP_POISSON;
  constexpr bool AUX1 = OP == OP_POISSON;
  constexpr int RW = asm_lds_rec<OP>();
  static_assert(!PIPE || (JAC && FANR == 9 && !STAGE && !LDSG), "PIPE: the direct Jacobian walk");
  static_assert(!REG || (OP == OP_PNP && JAC && KC && FANR == 9 && !STAGE && !LDSG && !PIPE),
                "REG: OP_PNP, the direct constant-planes Jacobian walk");
  extern __shared__ double srec[];  // LDSG: [cnt][RW] = x, y, dofs, aux0, aux1
  __shared__ uint32_t pfb[PIPE ? 4 * kPipeDw * kRows : 1];  // PIPE: the waves' prefetch regions
  // PIPE, wave-uniform: the 256-row blocks of this and the next two tiles (-1: none), this and
  // the next tile's chunk offset and the next one's slot count
  const int ntiles = (L.n_owned + 255) / 256, G = gridDim.x;
  const int wv = PIPE ? __builtin_amdgcn_readfirstlane(int(threadIdx.x) / kRows) : 0;
  const int ln = int(threadIdx.x) % kRows;
  uint32_t *const pw = pfb + (PIPE ? wv * kPipeDw * kRows : 0);
  int tile = blockIdx.x, b0 = -1, b1 = -1, b2 = -1, o0 = 0, o1 = 0, c1 = 0;
  auto tile_blk = [&](int t) { return t < ntiles ? row_block_const(L, t, ntiles) : -1; };
  // chunk of the wave's rows in block b (-1: b is no block, or the wave's rows are past the end)
  auto wave_chunk = [&](int b) {
    return (b >= 0 && b * 256 + wv * kRows < L.n_owned) ? b * 4 + wv : -1;
  };
  auto prefetch = [&](int b, int off, int clen) {  // all lanes; rows past the end read row n - 1
    if (wave_chunk(b) < 0) return;
    const int r0 = b * 256 + wv * kRows;
    const int *cix = L.colidx + off + ln;
#pragma unroll
    for (int k = 1; k < NS; k++)  // past the chunk's slots: slot 0 (padding slots hold the row)
      lds_dma4(cix + (k < clen ? k : 0) * kRows, pw + (k - 1) * kRows);
    const uint32_t *m =
        reinterpret_cast<const uint32_t *>(L.rowmeta + min(r0 + ln, L.n_owned - 1));
    lds_dma4(m, pw + 8 * kRows);
    lds_dma4(m + 1, pw + 9 * kRows);
    lds_dma4(reinterpret_cast<const uint32_t *>(a.rowflag + r0) + (ln >> 2), pw + 10 * kRows);
  };
  if constexpr (PIPE) {
    if (tile >= ntiles) return;
    b0 = tile_blk(tile);
    b1 = tile_blk(tile + G);
    b2 = tile_blk(tile + 2 * G);
    int c0 = 0;
    if (wave_chunk(b0) >= 0) {
      o0 = const_ld(L.chunk_off, wave_chunk(b0));
      c0 = const_ld(L.chunk_len, wave_chunk(b0));
    }
    if (wave_chunk(b1) >= 0) {
      o1 = const_ld(L.chunk_off, wave_chunk(b1));
      c1 = const_ld(L.chunk_len, wave_chunk(b1));
    }
    prefetch(b0, o0, c0);
  }
  int o2 = 0, c2 = 0, b3 = -1;  // PIPE: the scalars of tile + 2 G, tile + 3 G, loaded mid-tile
  const auto advance = [&]() {   // PIPE: on to the workgroup's next tile
    tile += G;
    b0 = b1, o0 = o1;
    b1 = b2, o1 = o2, c1 = c2;
    b2 = b3;
    return b0 >= 0;
  };
  do {
    const int blk = PIPE ? b0 : row_block(L, blockIdx.x, gridDim.x);
    const int row0 = blk * blockDim.x + threadIdx.x;
    const bool live = row0 < L.n_owned;
    if (!PIPE && !LDSG && !live) return;
    // the row's own loads first (LDSG: they are in flight while the workgroup stages the
    // neighbour records, instead of after its barrier)
    const int row = live ? row0 : 0;
    const int chunk = row / kRows, lane = row % kRows;
    if constexpr (REG) {
      const uint64_t meta = L.rowmeta[row];
      const bool regular =
          int(meta & 63) == kRegSlots && ((meta >> 6) & 1) && (meta >> 8) == 0;
      if (__all(regular)) {  // dead lanes have returned: a vote of the live rows
        // every row of the chunk has its seven slots: no bound on the index loads
        const int off = L.chunk_off[chunk];
        const int *__restrict__ cix = L.colidx + off + lane;
        int cr[kRegSlots];
#pragma unroll
        for (int k = 1; k < kRegSlots; k++) cr[k] = cix[k * kRows];
        const unsigned fl = a.rowflag[row];
        const double2 pi2 = reinterpret_cast<const double2 *>(L.xy)[row];
        double ui[NF];
        load_nf<NF>(a.x, size_t(row), ui);
        double2 pn[kRegSlots];
        double un[kRegSlots][NF];
        auto gather = [&](int k) {
          pn[k] = reinterpret_cast<const double2 *>(L.xy)[cr[k]];
          load_nf<NF>(a.x, size_t(cr[k]), un[k]);
        };
        // slot 6 is gathered in element 2, just ahead of the first store, when element 2's
        // temporaries are dead: with all six up front, or slot 6 before element 2, the kernel spills
#pragma unroll
        for (int k = 1; k < kRegSlots - 1; k++) gather(k);
        double *__restrict__ vc = a.vals + size_t(off) * NK;
        double R[NF], D[NK], P[NK], F[NK];
#pragma unroll
        for (int f = 0; f < NF; f++) R[f] = 0;
#pragma unroll
        for (int v = 0; v < NK; v++) D[v] = P[v] = F[v] = 0;
#pragma unroll
        for (int s = 1; s < kRegSlots; s++) {
          const int t = s + 1 < kRegSlots ? s + 1 : 1;  // static: the fan wraps after slot 6
          // Each element works on copies of its two neighbours that went through an empty asm,
          // v_t's first, then v_s's.  The copies make every element's arithmetic independent of
          // its neighbours', as in the general walk, where v_t comes through a per-lane select:
          // otherwise the compiler shares y_c / 120 and (y_i + y_c) / 60 with the next element's
          // y_b terms, and a product with a second use is fused the other way round.  The order
          // makes v_t's values the older ones, as the general walk's statements do: the compiler
          // orders the two products of Mib and Mic by the age of their inputs and fuses the first.
          // Either way Mib and Mic, and with them one residual entry in a hundred, came out an ulp
          // off the general walk's.
          double2 pt = pn[t], ps = pn[s];
          double ut[NF], us[NF];
          asm volatile("" : "+v"(pt.x), "+v"(pt.y));
#pragma unroll
          for (int f = 0; f < NF; f++) {
            ut[f] = un[t][f];
            asm volatile("" : "+v"(ut[f]));
          }
          asm volatile("" : "+v"(ps.x), "+v"(ps.y));
#pragma unroll
          for (int f = 0; f < NF; f++) {
            us[f] = un[s][f];
            asm volatile("" : "+v"(us[f]));
          }
          Geo G;
          geometry(pi2.x, pi2.y, ps.x, ps.y, pt.x, pt.y, G);
          double Ct[NK];
#pragma unroll
          for (int v = 0; v < NK; v++) Ct[v] = 0;
          element<OP, JAC, KC>(a, G, pi2.y, ps.y, pt.y, ui, us, ut, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, R,
                               D, P, Ct);
          if (s == 1) {
#pragma unroll
            for (int v = 0; v < NK; v++) F[v] = P[v];
          } else {
            if (s == 2) gather(kRegSlots - 1);
            store_block<OP, KC>(vc, lane, s, P);
          }
#pragma unroll
          for (int v = 0; v < NK; v++) P[v] = Ct[v];
          // R and D are read only after the last element, and without the general walk's
          // branches the compiler sinks all six elements' contributions to them down there,
          // keeping every element's geometry alive (59 VGPRs spilled); an empty asm that names
          // the running sums keeps each addition in its element
#pragma unroll
          for (int f = 0; f < NF; f++) asm volatile("" : "+v"(R[f]));
#pragma unroll
          for (int v = 2; v < NK; v++) asm volatile("" : "+v"(D[v]));  // KC: k2 ..
        }
#pragma unroll
        for (int v = 0; v < NK; v++) F[v] += P[v];
        store_block<OP, KC>(vc, lane, 1, F);
        store_block<OP, KC>(vc, lane, 0, D);
        // Only a wave with a flagged row reads cvec.  The others get a tail of their own with no
        // load in it, hence no wait at its top for the wave's block stores (the compiler waits
        // vmcnt(0) where the two paths of the per-lane load join).
        if (__any(fl & kRowFlagLoad))
          residual_tail<NF>(a, row, fl, R);
        else
          residual_tail<NF>(a, row, fl & ~unsigned(kRowFlagLoad), R);
        return;
      }
#ifdef ASM_REGULAR_CHECK  // ISA check build: the regular walk alone (tools/isa_regs.py)
      return;
#endif
    }
    int cj[NS];  // the fan's columns (LDSG: their positions in the staged list)
    uint64_t meta_pf = 0;
    unsigned fl_pf = 0;
    if constexpr (PIPE) {
      // The compiler orders neither the DMA loads before these LDS reads nor the reads before the
      // next DMA loads (seen in the ISA), so both waits are explicit: the tile's DMA loads have
      // landed (vmcnt counts in issue order: so have the previous tile's stores) ...
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = 1; k < NS; k++) cj[k] = int(pw[(k - 1) * kRows + ln]);
      meta_pf = uint64_t(pw[8 * kRows + ln]) | (uint64_t(pw[9 * kRows + ln]) << 32);
      fl_pf = (pw[10 * kRows + ln] >> (8 * (ln & 3))) & 0xffu;
      // ... and the region is read out before the next tile's loads may write it; then the scalars
      // of the tile after that
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      prefetch(b1, o1, c1);
      o2 = c2 = 0;
      if (wave_chunk(b2) >= 0) {
        o2 = const_ld(L.chunk_off, wave_chunk(b2));
        c2 = const_ld(L.chunk_len, wave_chunk(b2));
      }
      b3 = tile_blk(tile + 3 * G);
      if (!live) continue;
    }
    const int off = PIPE ? o0 : L.chunk_off[chunk];
    const uint64_t meta = PIPE ? meta_pf : L.rowmeta[row];
    const int len = int(meta & 63);
    const bool closed = (meta >> 6) & 1;
    const unsigned brk = unsigned(meta >> 8);  // fan-break bits, bit s: no element after slot s
    double *__restrict__ vc = a.vals + size_t(off) * NK;  // chunk base (k-form), see vin()

    if constexpr (PIPE) {
      // cj came from the prefetch region above
    } else if constexpr (LDSG) {
      const uint16_t *__restrict__ lix = L.lidx + off + lane;
#pragma unroll
      for (int k = 1; k < NS; k++) {  // past the fan: entry 0 (slot 0's own row is not staged)
        const int t = lix[(k < len ? k : 0) * kRows];
        cj[k] = k < len ? t : 0;
      }
    } else {
      const int *__restrict__ cix = L.colidx + off + lane;
#pragma unroll
      // past the fan: the row
      for (int k = 1; k < NS; k++) cj[k] = cix[(k < len ? k : 0) * kRows];
    }
    const double2 pi2 = reinterpret_cast<const double2 *>(L.xy)[row];
    double ui[NF];
    load_nf<NF>(a.x, size_t(row), ui);
    double ai = 0, aq = 0;
    if constexpr (AUX0) ai = a.aux0[row];
    if constexpr (AUX1) aq = a.aux1[row];
    if constexpr (OP == OP_PB) pb_fifth(ui[0], ai, aq);  // element(): e^{u/5}, e^{-u/5} per vertex
    if constexpr (LDSG) {
      const int u0 = L.uptr[blk], cnt = L.uown[blk];  // the fan neighbours (own rows come after)
      // up to ASM_SU list entries per thread: their list loads, then their gathers, then the LDS
      // stores (two round trips, not two per entry; ~1,000 distinct columns per block at config 3)
      constexpr int kSU = ASM_SU;
      int jj[kSU];
#pragma unroll
      for (int u = 0; u < kSU; u++) {
        const int k = int(threadIdx.x) + u * 256;
        jj[u] = k < cnt ? L.ulist[u0 + k] : -1;
      }
      double t[kSU][RW];
#pragma unroll
      for (int u = 0; u < kSU; u++)
        if (jj[u] >= 0) {
          const double2 p = reinterpret_cast<const double2 *>(L.xy)[jj[u]];
          t[u][0] = p.x;
          t[u][1] = p.y;
          double uu[NF];
          load_nf<NF>(a.x, size_t(jj[u]), uu);
#pragma unroll
          for (int f = 0; f < NF; f++) t[u][2 + f] = uu[f];
          if constexpr (AUX0) t[u][2 + NF] = a.aux0[jj[u]];
          if constexpr (AUX1) t[u][3 + NF] = a.aux1[jj[u]];
        }
#pragma unroll
      for (int u = 0; u < kSU; u++)
        if (jj[u] >= 0)
#pragma unroll
          for (int w = 0; w < RW; w++) srec[size_t(int(threadIdx.x) + u * 256) * RW + w] = t[u][w];
      for (int k = int(threadIdx.x) + kSU * 256; k < cnt; k += blockDim.x) {
        const int j = L.ulist[u0 + k];
        const double2 p = reinterpret_cast<const double2 *>(L.xy)[j];
        double u[NF];
        load_nf<NF>(a.x, size_t(j), u);
        double *r = srec + size_t(k) * RW;
        r[0] = p.x;
        r[1] = p.y;
#pragma unroll
        for (int f = 0; f < NF; f++) r[2 + f] = u[f];
        if constexpr (AUX0) r[2 + NF] = a.aux0[j];
        if constexpr (AUX1) r[3 + NF] = a.aux1[j];
      }
      __syncthreads();
      if (!live) return;
    }
    double2 pn[NS];
    double un[NS][NF], a0[NS], a1[NS];
    auto gather = [&](int k) {
      if constexpr (LDSG) {
        const double *r = srec + size_t(cj[k]) * RW;
        pn[k] = make_double2(r[0], r[1]);
#pragma unroll
        for (int f = 0; f < NF; f++) un[k][f] = r[2 + f];
        a0[k] = AUX0 ? r[2 + NF] : 0.0;
        a1[k] = AUX1 ? r[3 + NF] : 0.0;
      } else {
        pn[k] = reinterpret_cast<const double2 *>(L.xy)[cj[k]];
        load_nf<NF>(a.x, size_t(cj[k]), un[k]);
        a0[k] = AUX0 ? a.aux0[cj[k]] : 0.0;
        a1[k] = AUX1 ? a.aux1[cj[k]] : 0.0;
      }
    };
#pragma unroll
    for (int k = 1; k < SPLIT; k++) gather(k);
    // PB: slot k's e^{u/5} goes to a0[k] / a1[k] when element k - 1 needs it (slot 1: up front)
    if constexpr (OP == OP_PB) pb_fifth(un[1][0], a0[1], a1[1]);

    double R[NF], D[NK], P[NK], F[NK];
#pragma unroll
    for (int f = 0; f < NF; f++) R[f] = 0;
#pragma unroll
    for (int v = 0; v < NK; v++) D[v] = P[v] = F[v] = 0;
    // STAGE: blocks finished before the second-half gathers are issued (slots 1 .. SPLIT-3) wait
    // in LDS and go out right after those gathers: vmcnt retires loads and stores in issue order,
    // so a gather issued behind a store also waits for the store (A/B knob PNP_ASM_GA=6)
    constexpr int NSTG = (STAGE && JAC && SPLIT < NS && SPLIT > 3) ? SPLIT - 3 : 0;
    __shared__ double stg[NSTG > 0 ? NSTG * NK * 256 : 1];
    unsigned staged = 0;
    auto put = [&](int s, const double *Kc) {
      if (NSTG > 0 && s <= NSTG) {
#pragma unroll
        for (int v = 0; v < NK; v++) stg[((s - 1) * NK + v) * 256 + threadIdx.x] = Kc[v];
        staged |= 1u << s;
      } else {
        store_block<OP, KC>(vc, lane, s, Kc);
      }
    };
#pragma unroll
    for (int s = 1; s < NS; s++) {
      if (SPLIT < NS && s == (SPLIT > 2 ? SPLIT - 2 : 1)) {
#pragma unroll
        for (int k = SPLIT; k < NS; k++) gather(k);
        if constexpr (NSTG > 0) {
#pragma unroll
          for (int q = 1; q <= NSTG; q++)
            if ((staged >> q) & 1) {
              double K[NK];
#pragma unroll
              for (int v = 0; v < NK; v++) K[v] = stg[((q - 1) * NK + v) * 256 + threadIdx.x];
              store_block<OP, KC>(vc, lane, q, K);
            }
        }
      }
      if (s < len) {
        const bool has_next = s + 1 < len;
        const int sn = (s + 1 < NS) ? s + 1 : 1;  // static slot of v_{s+1}
        const bool elem = (has_next || closed) && !((brk >> s) & 1);
        if constexpr (OP == OP_PB)
          if (has_next) pb_fifth(un[sn][0], a0[sn], a1[sn]);
        if (elem) {
          // v_t = v_{s+1}, or v_1 when a closed fan wraps
          const double2 pt = has_next ? pn[sn] : pn[1];
          double ut[NF];
#pragma unroll
          for (int f = 0; f < NF; f++) ut[f] = has_next ? un[sn][f] : un[1][f];
          const double at0 = has_next ? a0[sn] : a0[1], at1 = has_next ? a1[sn] : a1[1];
          Geo G;
          geometry(pi2.x, pi2.y, pn[s].x, pn[s].y, pt.x, pt.y, G);
          double Ct[NK];
#pragma unroll
          for (int v = 0; v < NK; v++) Ct[v] = 0;
          element<OP, JAC, KC>(a, G, pi2.y, pn[s].y, pt.y, ui, un[s], ut, ai, a0[s], at0, aq,
                               a1[s], at1, R, D, P, Ct);
          if constexpr (JAC) {
            if (s == 1 && closed) {
#pragma unroll
              for (int v = 0; v < NK; v++) F[v] = P[v];
            } else {
              put(s, P);
            }
#pragma unroll
            for (int v = 0; v < NK; v++) P[v] = Ct[v];
          }
        } else if constexpr (JAC) {
          put(s, P);
#pragma unroll
          for (int v = 0; v < NK; v++) P[v] = 0;
        }
      }
    }
    if constexpr (JAC) {
      if (closed) {
#pragma unroll
        for (int v = 0; v < NK; v++) F[v] += P[v];
        store_block<OP, KC>(vc, lane, 1, F);
      }
      store_block<OP, KC>(vc, lane, 0, D);
    }
    residual_tail<NF>(a, row, PIPE ? fl_pf : unsigned(a.rowflag[row]), R);
  } while (PIPE && advance());
}

#ifdef ASM_REGULAR_CHECK
// ISA check build: the general walk unrolled for six neighbours, whose fp64 instruction multiset
// the regular walk (alone in its kernels under this flag) must show
template __global__ void k_assemble_ga<OP_PNP, 1, 3, 7, 7, 0, 0, 1>(DevLayout, AsmArgs);
#endif

// cvec[row] -= M(x_old)[row]: PnpTOperator (tau * (c+ + c-) into the c+ row, Q2) or the
// DiffusionTOperator mass, for the implicit Euler residual M(u) - M(u_old) + dt R(u).
template <int OP>
__global__ __launch_bounds__(256) void k_mass_apply(DevLayout L, double tau, double pi, int cyl,
                                                    const double *__restrict__ xo,
                                                    double *__restrict__ cvec) {
  constexpr int NF = OpTraits<OP>::NF;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= L.n_owned) return;
  const int chunk = row / kRows, lane = row % kRows;
  const int off = L.chunk_off[chunk];
  const uint64_t meta = L.rowmeta[row];
  const int len = int(meta & 63);
  const bool closed = (meta >> 6) & 1;
  const int *cix = L.colidx + off + lane;
  const double2 pi2 = reinterpret_cast<const double2 *>(L.xy)[row];
  double acc = 0;
  for (int s = 1; s < len; ++s) {
    const int t = (s + 1 < len) ? s + 1 : (closed ? 1 : -1);
    if (t < 0 || ((meta >> (8 + s)) & 1)) continue;
    const int b = cix[s * kRows], c = cix[t * kRows];
    const double2 pb2 = reinterpret_cast<const double2 *>(L.xy)[b];
    const double2 pc2 = reinterpret_cast<const double2 *>(L.xy)[c];
    Geo G;
    geometry(pi2.x, pi2.y, pb2.x, pb2.y, pc2.x, pc2.y, G);
    if constexpr (OP == OP_PNP_IE) {
      double Mii, Mib, Mic;
      mass_q2(G, cyl, pi, pi2.y, pb2.y, pc2.y, Mii, Mib, Mic);
      acc += tau * ((xo[size_t(row) * 3 + 1] + xo[size_t(row) * 3 + 2]) * Mii +
                    (xo[size_t(b) * 3 + 1] + xo[size_t(b) * 3 + 2]) * Mib +
                    (xo[size_t(c) * 3 + 1] + xo[size_t(c) * 3 + 2]) * Mic);
    } else {
      acc += xo[row] * G.adet * (1.0 / 12.0) + (xo[b] + xo[c]) * G.adet * (1.0 / 24.0);
    }
  }
  if constexpr (OP == OP_PNP_IE)
    cvec[size_t(row) * NF + 1] -= acc;
  else
    cvec[row] -= acc;
}

// Ion-current observable (calcIonFlux, src/ionFlux.hh:8-96): one thread per boundary segment
// handled by this rank; seg = {a, c, o, group} local vertices (segment a-c, opposite vertex o of
// its element).  out[2k] = ip contribution, out[2k+1] = im contribution (summed on the host in
// segment order, so the result does not depend on the launch).
__global__ __launch_bounds__(256) void k_ion_flux(int ns, const int4 *__restrict__ seg,
                                                  const double *__restrict__ xy,
                                                  const double *__restrict__ x, int cyl,
                                                  double pi, double *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ns) return;
  const int4 q = seg[k];
  const double2 pa = reinterpret_cast<const double2 *>(xy)[q.x];
  const double2 pc = reinterpret_cast<const double2 *>(xy)[q.y];
  const double2 po = reinterpret_cast<const double2 *>(xy)[q.z];
  Geo G;  // vertex order (a, c, o): gi = grad psi_a, gb = grad psi_c, gc = grad psi_o
  geometry(pa.x, pa.y, pc.x, pc.y, po.x, po.y, G);
  double gf[3][2];
#pragma unroll
  for (int f = 0; f < 3; f++) {
    const double ua = x[size_t(q.x) * 3 + f], uc = x[size_t(q.y) * 3 + f],
                 uo = x[size_t(q.z) * 3 + f];
    gf[f][0] = ua * G.gi0 + uc * G.gb0 + uo * G.gc0;
    gf[f][1] = ua * G.gi1 + uc * G.gb1 + uo * G.gc1;
  }
  const double cp = 0.5 * (x[size_t(q.x) * 3 + 1] + x[size_t(q.y) * 3 + 1]);
  const double cm = 0.5 * (x[size_t(q.x) * 3 + 2] + x[size_t(q.y) * 3 + 2]);
  const double tx = pc.x - pa.x, ty = pc.y - pa.y;
  const double len = sqrt(tx * tx + ty * ty);
  double factor = len;
  if (cyl) factor *= 2 * pi * (0.5 * (pa.y + pc.y));
  double nx = ty / len, ny = -tx / len;
  if (nx * (po.x - pa.x) + ny * (po.y - pa.y) > 0) {
    nx = -nx;
    ny = -ny;
  }
  const double gp0 = factor * gf[0][0] * cp, gp1 = factor * gf[0][1] * cp;
  out[2 * size_t(k)] = (-factor * gf[1][0] + gp0) * nx + (-factor * gf[1][1] + gp1) * ny;
  const double r = cm / cp;
  out[2 * size_t(k) + 1] =
      (-factor * gf[2][0] - gp0 * r) * nx + (-factor * gf[2][1] - gp1 * r) * ny;
}

}  // namespace

hipError_t launch_ion_flux(int ns, const int4 *seg, const double *xy, const double *x, int cyl,
                           double pi, double *out, hipStream_t s) {
  if (ns == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ion_flux, dim3((ns + 255) / 256), dim3(256), 0, s, ns, seg, xy, x, cyl, pi,
                     out);
  return hipGetLastError();
}

// t0 / t1 (may be null): events the launch itself records at the kernel's start and end
// (hipExtLaunchKernelGGL), so the library's timers see the kernel's own duration -- an event pair
// recorded around the launch adds the dispatch of two markers (~5 us at config 3 in situ, against
// the kernel trace: 75.7 vs 69.6 us, gpurun_out r6final1 / profiles/r06/asm_regimes_config3.json)
// PNP_ASM_PIPE's default: off.  At config 3 the pipelined walk measured 44.1 us per warm launch
// against 39.6 for the direct walk (parent commit: 42.4), at every grid from one tile per
// workgroup to the resident grid (profiles/asm_pipe/)
constexpr bool kAsmPipeDefault = false;
// PNP_ASM_REGULAR's default (profiles/asm_regular/)
constexpr bool kAsmRegularDefault = true;

// The pipelined walk's launch (operators with constant planes: OP_PNP).  Grid: the workgroups
// resident at once (occupancy x CUs) rounded down to a multiple of 8, at most one per tile, at
// most cap (> 0).  Returns 1 when it launched.
template <int OP>
static int launch_pipe(const DevLayout &L, const AsmArgs &a, int cap, hipStream_t s, hipEvent_t t0,
                       hipEvent_t t1) {
  if constexpr (asm_kc<OP>()) {
    const auto kern = k_assemble_ga<OP, 1, 3, 9, 6, 0, 0, 1, 1>;
    static const int resident = [&] {
      int dev = 0, cus = 0, per_cu = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0) != hipSuccess)
        return 0;
      return per_cu * cus;
    }();
    const int ntiles = (L.n_owned + 255) / 256;
    int g = resident >= 8 ? resident / 8 * 8 : 8;
    if (g > ntiles) g = ntiles;
    if (cap > 0 && g > cap) g = cap;
    hipExtLaunchKernelGGL(kern, dim3(g), dim3(256), 0, s, t0, t1, 0, L, a);
    return 1;
  } else {
    return 0;
  }
}

hipError_t launch_assemble(const DevLayout &L, const AsmArgs &a, hipStream_t s, hipEvent_t t0,
                           hipEvent_t t1, int *pipelined) {
  if (pipelined) *pipelined = 0;
  if (L.n_owned == 0) return hipSuccess;
  dim3 grid((L.n_owned + 255) / 256), block(256);
  // occupancy variant (A/B knob, PNP_ASM_WAVES=3|4): 4 waves/SIMD caps the fused PNP kernel at
  // 128 VGPRs (a few bytes of spill), 3 lets it keep ~134 without spilling
  static const int waves = [] {
    const char *e = getenv("PNP_ASM_WAVES");
    return (e && atoi(e) == 4) ? 4 : 3;
  }();
  // fans up to 11 neighbours keep their column indices in registers (all meshes seen: <= 8)
  static const bool fanr_ok = [] {  // A/B knob: PNP_ASM_FANR=0 forces the index-load path
    const char *e = getenv("PNP_ASM_FANR");
    return !(e && atoi(e) == 0);
  }();
  // A/B knob PNP_ASM_GA: 0 = the pipelined walk (k_assemble), 1 = gather-all at 3 waves/SIMD
  // (spills), 2 = gather-all at 2 waves, 3 / 4 / 5 = gather slots 1-4 / 1-5 / 1-2 first and the
  // rest two elements later at 3 waves; 4 is the default (profiles/r01/ab_asm_ga_*.log)
  static const int ga = [] {
    const char *e = getenv("PNP_ASM_GA");
    return e ? atoi(e) : 4;
  }();
  // column indices in registers: FANR - 1 >= the longest fan (max_slots - 1; 8 on all meshes
  // seen), 12 as the general case, 0 (index loads in the walk) beyond
  const int fanr = !fanr_ok ? 0 : (L.max_slots <= 9 ? 9 : (L.max_slots <= 12 ? 12 : 0));
  // LDS-staged neighbour data (A/B knob PNP_ASM_LDS=1), when the layout has the lists and a
  // workgroup's records fit 53 KiB (3 workgroups per CU at the kernel's 3 waves per SIMD).
  // Measured at config 3, with the row's own loads issued before the staging barrier: warm
  // 53.5 -> 60-63 us, cache-cold 87 -> 77.7 us (profiles/r02/ab_asm_lds2.log): the barrier costs
  // more than the halved gathers save while the inputs sit in the Infinity Cache, and less when
  // they come from HBM.  Off by default (the back-to-back assembly is the benchmark's number).
  // Well past the Infinity Cache every launch is cache-cold, so the Jacobian assembly takes the
  // LDS-staged walk there by default: its k-form write stream (~7 blocks per row on triangle
  // meshes) larger than twice the 256 MiB Infinity Cache.  Config 5 (828 MB): 344.8 -> 319.5 us
  // (profiles/r02/ab_cfg5_lds.log); config 2 (311 MB, still partly cache-resident back to back):
  // 79 -> 84 us, so the direct walk below 512 MiB (ab_cfg2_lds.log).  PNP_ASM_LDS=0 / 1 forces
  // either walk.
  static const int lds_env = [] {
    const char *e = getenv("PNP_ASM_LDS");
    return e ? (atoi(e) == 1 ? 1 : 0) : -1;
  }();
  // The Jacobian assembly inside Newton follows a BiCGSTAB solve, whose matrix and vector streams
  // have replaced the assembly's inputs in the caches: such a launch (a.cold, set by the context
  // after a solve) is cache-cold at any size and takes the LDS-staged walk too (config 3 in situ:
  // profiles/r03/ab_asm_cold_hint.log); PNP_ASM_COLD_HINT=0 ignores the hint (A/B)
  static const bool cold_hint = [] {
    const char *e = getenv("PNP_ASM_COLD_HINT");
    return !(e && e[0] == '0');
  }();
  const auto lds_walk = [&](int nk) {
    return lds_env == 1 ||
           (lds_env < 0 && (size_t(L.n_owned) * 7 * size_t(nk) * 8 > (size_t(512) << 20) ||
                            (cold_hint && a.cold)));
  };
  // The persistent, prefetching walk (k_assemble_ga<..., PIPE = 1>) in place of the direct
  // constant-planes walk: PNP_ASM_PIPE=1 (0, the default: the direct walk; read once per
  // process).  The cold / in-situ launches keep the LDS-staged walk.  PNP_ASM_PIPE_GRID=n caps
  // its grid at n workgroups (A/B and test knob: any n >= 1 is correct).
  static const bool pipe_on = [] {
    const char *e = getenv("PNP_ASM_PIPE");
    return e ? atoi(e) != 0 : kAsmPipeDefault;
  }();
  static const int pipe_cap = [] {
    const char *e = getenv("PNP_ASM_PIPE_GRID");
    return (e && atoi(e) >= 1) ? atoi(e) : 0;
  }();
  // The regular walk inside the direct constant-planes OP_PNP walk (k_assemble_ga<..., REG = 1>):
  // PNP_ASM_REGULAR=0/1, read once per process.
  static const bool regular_on = [] {
    const char *e = getenv("PNP_ASM_REGULAR");
    return e ? atoi(e) != 0 : kAsmRegularDefault;
  }();
  int piped = 0;
#define PNP_ASM_CASE(OPK)                                                          \
  case OPK:                                                                        \
    if (!fanr && a.jac)                                                            \
      hipExtLaunchKernelGGL((k_assemble<OPK, 1, 3, 0>), grid, block, 0, s, t0, t1, 0, L, a);     \
    else if (!fanr)                                                                \
      hipExtLaunchKernelGGL((k_assemble<OPK, 0, 4, 0>), grid, block, 0, s, t0, t1, 0, L, a);     \
    else if (!a.jac && fanr == 9 && ga && lds_env == 1 && L.uown &&                 \
             size_t(L.unmax) * asm_lds_rec<OPK>() * 8 <= 53 * 1024)                    \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 0, 3, 9, 9, 0, 1>), grid, block,         \
                         size_t(L.unmax) * asm_lds_rec<OPK>() * 8, s, t0, t1, 0, L, a);             \
    else if (!a.jac && fanr == 9 && ga)                                            \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 0, 3, 9>), grid, block, 0, s, t0, t1, 0, L, a);  \
    else if (!a.jac)                                                               \
      hipExtLaunchKernelGGL((k_assemble<OPK, 0, 4, 12>), grid, block, 0, s, t0, t1, 0, L, a);    \
    else if (ga == 1 && fanr == 9)                                                 \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9>), grid, block, 0, s, t0, t1, 0, L, a);  \
    else if (ga == 2 && fanr == 9)                                                 \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 2, 9>), grid, block, 0, s, t0, t1, 0, L, a);  \
    else if (ga == 3 && fanr == 9)                                                 \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 5>), grid, block, 0, s, t0, t1, 0, L, a); \
    else if (ga == 4 && fanr == 9 && asm_kc<OPK>() && a.kconst &&                   \
             lds_walk(OpTraits<OPK>::NK) && L.uown &&                               \
             size_t(L.unmax) * asm_lds_rec<OPK>() * 8 <= 53 * 1024)                    \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 6, 0, 1, asm_kc<OPK>()>), grid,  \
                         block, size_t(L.unmax) * asm_lds_rec<OPK>() * 8, s, t0, t1, 0, L, a); \
    else if (ga == 4 && fanr == 9 && asm_kc<OPK>() && a.kconst && pipe_on)         \
      piped = launch_pipe<OPK>(L, a, pipe_cap, s, t0, t1);                         \
    else if (ga == 4 && fanr == 9 && asm_kc<OPK>() && a.kconst && regular_on)      \
      hipExtLaunchKernelGGL(                                                       \
          (k_assemble_ga<OPK, 1, 3, 9, 6, 0, 0, asm_kc<OPK>(), 0, asm_reg<OPK>()>), grid, block, \
          0, s, t0, t1, 0, L, a);                                                  \
    else if (ga == 4 && fanr == 9 && asm_kc<OPK>() && a.kconst)                    \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 6, 0, 0, asm_kc<OPK>()>), grid,  \
                         block, 0, s, t0, t1, 0, L, a);                             \
    else if (ga == 4 && fanr == 9 && lds_walk(OpTraits<OPK>::NK) && L.uown &&       \
             size_t(L.unmax) * asm_lds_rec<OPK>() * 8 <= 53 * 1024)                    \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 6, 0, 1>), grid, block,         \
                         size_t(L.unmax) * asm_lds_rec<OPK>() * 8, s, t0, t1, 0, L, a);             \
    else if (ga == 4 && fanr == 9)                                                 \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 6>), grid, block, 0, s, t0, t1, 0, L, a); \
    else if (ga == 5 && fanr == 9)                                                 \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 3>), grid, block, 0, s, t0, t1, 0, L, a); \
    else if (ga == 6 && fanr == 9)                                                 \
      hipExtLaunchKernelGGL((k_assemble_ga<OPK, 1, 3, 9, 6, 1>), grid, block, 0, s, t0, t1, 0, L, a); \
    else if (fanr == 12)                                                           \
      hipExtLaunchKernelGGL((k_assemble<OPK, 1, 3, 12>), grid, block, 0, s, t0, t1, 0, L, a);    \
    else if (waves == 3)                                                           \
      hipExtLaunchKernelGGL((k_assemble<OPK, 1, 3, 9>), grid, block, 0, s, t0, t1, 0, L, a);     \
    else                                                                           \
      hipExtLaunchKernelGGL((k_assemble<OPK, 1, 4, 9>), grid, block, 0, s, t0, t1, 0, L, a);     \
    break;
  switch (a.kind) {
    PNP_ASM_CASE(OP_PNP)
    PNP_ASM_CASE(OP_PNP_IE)
    PNP_ASM_CASE(OP_PB)
    PNP_ASM_CASE(OP_DIFF)
    PNP_ASM_CASE(OP_DIFF_IE)
    PNP_ASM_CASE(OP_POISSON)
  default:
    return hipErrorInvalidValue;
  }
#undef PNP_ASM_CASE
  if (pipelined) *pipelined = piped;
  return hipGetLastError();
}

hipError_t launch_mass_apply(const DevLayout &L, int kind, double tau, double pi, int cylindrical,
                             const double *x_old, double *cvec, hipStream_t s) {
  if (L.n_owned == 0) return hipSuccess;
  dim3 grid((L.n_owned + 255) / 256), block(256);
  if (kind == OP_PNP_IE)
    hipLaunchKernelGGL(k_mass_apply<OP_PNP_IE>, grid, block, 0, s, L, tau, pi, cylindrical, x_old,
                       cvec);
  else if (kind == OP_DIFF_IE)
    hipLaunchKernelGGL(k_mass_apply<OP_DIFF_IE>, grid, block, 0, s, L, tau, pi, cylindrical,
                       x_old, cvec);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace pnp
