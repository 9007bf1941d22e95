// What the device layout (kernels.h DevLayout) holds beyond the LocalLayout itself, derived on the
// host: pure functions of (LocalLayout, knobs), shared by the context (ctx.cc: derive, upload) and
// the GPU-free pnp_layout_derived.  No HIP here.  Element types are those of the device buffers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "mesh.h"
#include "pk.h"

namespace pnp {

// The environment's A/B switches of the derivation, read once per context (from_env)
struct LayoutKnobs {
  bool split_sort = true;     // PNP_SPLIT_SORT: lanes longest-first inside a colour segment
  bool blkmap = true;         // PNP_BLKMAP: spatial block order
  bool spmv_lds = true;       // PNP_SPMV_LDS: the SpMV's per-block column lists
  bool list_own_last = true;  // PNP_LIST_OWN_LAST: a block's own-row-only columns last in them
  bool halo_overlap = true;   // PNP_HALO_OVERLAP: interior / boundary block split (multi-rank)
  int xcd_remap = 0;          // PNP_XCD_REMAP (DevLayout::xcd_remap; measured: off)
  static LayoutKnobs from_env();
};

// Triangular split of the owned-column pattern (DevLayout l* / u*): position p = 64 ch + lane
// holds row rowL(p) in L and rowU(p) in U; *src = row << 6 | slot of the SELL entry, -1 padding
struct SplitLayout {
  std::vector<uint8_t> lperm, uperm, lpinv, upinv, llen, ulen, ldl;
  std::vector<int> lchunk_len, lchunk_off, lcolidx, lsrc, uchunk_len, uchunk_off, ucolidx, usrc;
  int64_t lslots_live = 0, uslots_live = 0;
  int rowL(int pos) const { return 64 * (pos / 64) + lperm[pos]; }
  int rowU(int pos) const { return 64 * (pos / 64) + uperm[pos]; }
};
void derive_split(const LocalLayout &L, const LayoutKnobs &K, SplitLayout &S);

// LDS-staged sweep lists (DevLayout lsx_* / usx_*), per 256-position block of each colour.
// usable = false (everything empty) when they do not fit: >= 0xFFFF entries in a block, more than
// 256 colours, or a list longer than 64 KiB / 24 B.  posrow*: the row at each split position
struct SweepLists {
  bool usable = false;
  std::vector<int> lptr, llist, uptr, ulist;
  std::vector<uint16_t> lidx, uidx;
  int sx_max = 0;
  std::vector<int> posrowL, posrowU;
};
void derive_sweep_lists(const LocalLayout &L, const SplitLayout &S, SweepLists &X);

// row-contiguous block offsets and columns of the owned rows (fused ILU(0) factorisation)
struct RowLists {
  std::vector<int> rowoff, rowcol;
};
void derive_row_lists(const LocalLayout &L, RowLists &R);

// spatial order of the 256-row blocks (DevLayout::blkmap); empty: identity (knob off, no rows)
void derive_blkmap(const LocalLayout &L, const LayoutKnobs &K, std::vector<int> &blkmap);

// P1 ion-flux segments of this rank, in global segment order (the layout of an int4)
struct FluxSeg {
  int a, c, opp, group;  // local vertices of the segment, the opposite vertex, physical group
};
struct FluxSegs {
  std::vector<FluxSeg> segs;
  std::vector<int> group;
};
bool derive_flux_segments(const Mesh &mg, const LocalLayout &L, FluxSegs &F, std::string &err);

// LDS-staged SpMV lists (DevLayout uptr / ulist / lidx / uown), per 256-row block.  usable = false
// (everything empty) when the knob is off, a block has more than 65535 distinct columns, or a list
// is longer than 64 KiB / 24 B
struct SpmvLists {
  bool usable = false;
  std::vector<int> uptr, ulist, uown;
  std::vector<uint16_t> lidx;
  int umax = 0, unmax = 0;
};
void derive_spmv_lists(const LocalLayout &L, const LayoutKnobs &K, SpmvLists &U);

// halo-overlapped SpMV: the blocks without / with a ghost column, each in blkmap's order
struct BlockSplit {
  bool usable = false;  // knob on and rows owned
  std::vector<int> interior, boundary;
};
void derive_block_split(const LocalLayout &L, const LayoutKnobs &K, const std::vector<int> &blkmap,
                        BlockSplit &B);

struct DerivedLayout {
  SplitLayout split;
  SweepLists sweep;
  RowLists rows;
  std::vector<int> blkmap;
  FluxSegs flux;
  SpmvLists spmv;
  BlockSplit halo;
};
// every block above, in the order the context uploads them
bool derive_layout(const Mesh &m, const LocalLayout &L, const LayoutKnobs &K, DerivedLayout &D,
                   std::string &err);

// What the context reads after creation (ilu_flow_build, pk_build, pnp_get_info); the matrix-sized
// arrays are not kept
struct KeptLayout {
  std::vector<int> posrowL, posrowU;                      // empty unless the sweep lists are usable
  std::vector<int> lsx_ptr, lsx_list, usx_ptr, usx_list;  // likewise
  std::vector<int> blkmap;
  int64_t lslots_live = 0, uslots_live = 0;
};
KeptLayout keep_layout(DerivedLayout &&D);

// The host front half of pnp_create_pk and pnp_layout_build_pk: on entry `mesh` is the validated
// triangle mesh; for degree > 1 it moves to tmesh and mesh becomes the node mesh of the P_k space.
// Then fans (or the node adjacency), RCB partition, the empty-part check and the local layout.
// Every rank computes the same partition, so all of them fail here alike
bool build_host_layout(Mesh &mesh, int degree, int rank, int nranks, Mesh &tmesh, PkSpace &pks,
                       Fans &fans, LocalLayout &L, std::string &err);

}  // namespace pnp
