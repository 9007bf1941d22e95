// Host derivation of the device layout (layout_derive.h): index computation only, no device.
#include "layout_derive.h"

#include <algorithm>
#include <cstdlib>
#include <unordered_map>

namespace pnp {

LayoutKnobs LayoutKnobs::from_env() {
  LayoutKnobs K;
  K.split_sort = [] {
    const char *e = getenv("PNP_SPLIT_SORT");
    return !(e && e[0] == '0');
  }();
  if (const char *e = getenv("PNP_BLKMAP")) K.blkmap = !(atoi(e) == 0);
  if (const char *ev = getenv("PNP_SPMV_LDS")) K.spmv_lds = !(atoi(ev) == 0);
  K.list_own_last = [] {
    const char *e = getenv("PNP_LIST_OWN_LAST");
    return !(e && e[0] == '0');
  }();
  if (const char *ev = getenv("PNP_HALO_OVERLAP")) K.halo_overlap = !(atoi(ev) == 0);
  {
    const char *e = getenv("PNP_XCD_REMAP");
    K.xcd_remap = (e && atoi(e) == 1) ? 1 : 0;  // measured: off for assembly / SpMV
  }
  return K;
}

// triangular split of the owned-column pattern (DevLayout l*/u*).  Lane order (PNP_SPLIT_SORT,
// default on): inside each 64-row chunk, and inside each colour's segment of it, the rows are
// stored longest-first in each of L and U, so a slot plane's padding is a tail of lanes that
// issue no loads (config 3: 17.8 % of the split slots are padding); position p = 64 ch + lane
// holds row 64 ch + lperm[p] in L and 64 ch + uperm[p] in U.  A row's own arithmetic and slot
// order are unchanged, so every result is bitwise the identity order's.
void derive_split(const LocalLayout &L, const LayoutKnobs &K, SplitLayout &S) {
  const int no = L.n_owned, npos = 64 * L.nchunks;
  std::vector<int> nlr(npos, 0), nur(npos, 1);
  for (int row = 0; row < no; row++) {
    const int ch = row / 64, ln = row % 64, len = int(L.rowmeta[row] & 63);
    for (int sl = 1; sl < len; sl++) {
      const int j = L.colidx[size_t(L.chunk_off[ch]) + 64 * sl + ln];
      // ghost and same-colour columns are outside the sweeps (mesh.cc absorb_top)
      if (j >= no || j == row || L.rowcolor[j] == L.rowcolor[row]) continue;
      (j < row ? nlr[row] : nur[row])++;
    }
  }
  std::vector<uint8_t> &lperm = S.lperm, &uperm = S.uperm, &lpinv = S.lpinv, &upinv = S.upinv,
                       &llen8 = S.llen, &ulen8 = S.ulen, &ldl = S.ldl;
  lperm.assign(npos, 0), uperm.assign(npos, 0), lpinv.assign(npos, 0), upinv.assign(npos, 0);
  llen8.assign(npos, 0), ulen8.assign(npos, 0), ldl.assign(npos, 0);
  const bool sort_lanes = K.split_sort;
  for (int ch = 0; ch < L.nchunks; ch++) {
    for (int ln = 0; ln < 64; ln++) lperm[64 * ch + ln] = uperm[64 * ch + ln] = uint8_t(ln);
    for (int a0 = 64 * ch; a0 < std::min(no, 64 * ch + 64);) {  // colour segments
      int a1 = a0 + 1;
      while (a1 < std::min(no, 64 * ch + 64) && L.rowcolor[a1] == L.rowcolor[a0]) a1++;
      if (sort_lanes) {
        std::vector<int> ord(a1 - a0);
        for (int k = 0; k < a1 - a0; k++) ord[k] = a0 + k;
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return nlr[x] > nlr[y]; });
        for (int k = 0; k < a1 - a0; k++) lperm[a0 + k] = uint8_t(ord[k] - 64 * ch);
        for (int k = 0; k < a1 - a0; k++) ord[k] = a0 + k;
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return nur[x] > nur[y]; });
        for (int k = 0; k < a1 - a0; k++) uperm[a0 + k] = uint8_t(ord[k] - 64 * ch);
      }
      a0 = a1;
    }
  }
  auto rowL = [&](int pos) { return 64 * (pos / 64) + lperm[pos]; };
  auto rowU = [&](int pos) { return 64 * (pos / 64) + uperm[pos]; };
  for (int pos = 0; pos < npos; pos++) {
    lpinv[rowL(pos)] = uint8_t(pos % 64);
    upinv[rowU(pos)] = uint8_t(pos % 64);
  }
  S.lslots_live = S.uslots_live = 0;
  for (int pos = 0; pos < npos; pos++) {
    llen8[pos] = uint8_t(nlr[rowL(pos)]);
    ulen8[pos] = uint8_t(nur[rowU(pos)]);
    ldl[pos] = upinv[rowL(pos)];
    if (rowL(pos) < no) S.lslots_live += nlr[rowL(pos)];
    if (rowU(pos) < no) S.uslots_live += nur[rowU(pos)];
  }
  std::vector<int> &lcl = S.lchunk_len, &lco = S.lchunk_off, &ucl = S.uchunk_len,
                   &uco = S.uchunk_off;
  lcl.assign(L.nchunks, 0), lco.assign(L.nchunks + 1, 0), ucl.assign(L.nchunks, 0),
      uco.assign(L.nchunks + 1, 0);
  for (int ch = 0; ch < L.nchunks; ch++) {
    int ml = 0, mu = 1;
    for (int row = 64 * ch; row < std::min(no, 64 * ch + 64); row++) {
      ml = std::max(ml, nlr[row]);
      mu = std::max(mu, nur[row]);
    }
    lcl[ch] = ml;
    ucl[ch] = mu;
    lco[ch + 1] = lco[ch] + 64 * ml;
    uco[ch + 1] = uco[ch] + 64 * mu;
  }
  std::vector<int> &lcol = S.lcolidx, &lsrc = S.lsrc, &ucol = S.ucolidx, &usrc = S.usrc;
  lcol.assign(lco[L.nchunks], 0), lsrc.assign(lco[L.nchunks], -1), ucol.assign(uco[L.nchunks], 0),
      usrc.assign(uco[L.nchunks], -1);
  for (int ch = 0; ch < L.nchunks; ch++)
    for (int ln = 0; ln < 64; ln++) {
      const int p = 64 * ch + ln, rl = rowL(p), ru = rowU(p);
      for (int sl = 0; sl < lcl[ch]; sl++) lcol[size_t(lco[ch]) + 64 * sl + ln] = rl;
      for (int sl = 0; sl < ucl[ch]; sl++) ucol[size_t(uco[ch]) + 64 * sl + ln] = ru;
      if (p >= no) continue;
      for (int side = 0; side < 2; side++) {  // 0: L at this position (row rl), 1: U (row ru)
        const int row = side ? ru : rl, rch = row / 64, rln = row % 64;
        const int len = int(L.rowmeta[row] & 63);
        int kl = 0, ku = 1;
        if (side) usrc[size_t(uco[ch]) + ln] = row << 6;  // slot 0: the diagonal block
        for (int sl = 1; sl < len; sl++) {
          const int j = L.colidx[size_t(L.chunk_off[rch]) + 64 * sl + rln];
          if (j >= no || j == row || L.rowcolor[j] == L.rowcolor[row]) continue;
          if (j < row) {
            if (!side) {
              lcol[size_t(lco[ch]) + 64 * kl + ln] = j;
              lsrc[size_t(lco[ch]) + 64 * kl + ln] = row << 6 | sl;
            }
            kl++;
          } else {
            if (side) {
              ucol[size_t(uco[ch]) + 64 * ku + ln] = j;
              usrc[size_t(uco[ch]) + 64 * ku + ln] = row << 6 | sl;
            }
            ku++;
          }
        }
      }
    }
}

// LDS-staged sweep lists (DevLayout lsx_* / usx_*): per colour, per 256-row block of the
// colour, the distinct rows its L / U split slots couple to; per split position its list
// position (0xFFFF for padding and the U diagonal slot)
void derive_sweep_lists(const LocalLayout &L, const SplitLayout &S, SweepLists &X) {
  const int npos = 64 * L.nchunks;
  auto rowL = [&](int pos) { return S.rowL(pos); };
  auto rowU = [&](int pos) { return S.rowU(pos); };
  const int nc = int(L.color_ptr.size()) - 1;
  auto lists = [&](const std::vector<int> &cl, const std::vector<int> &co,
                   const std::vector<int> &cc, int s0, auto rowat, std::vector<int> &ptr,
                   std::vector<int> &lst, std::vector<uint16_t> &idx) -> bool {
    idx.assign(cc.size(), 0xFFFF);
    ptr.assign(1, 0);
    lst.clear();
    std::vector<int> cols;
    for (int c = 0; c < nc; c++) {
      const int a = L.color_ptr[c], b = L.color_ptr[c + 1];
      for (int r0 = a; r0 < b; r0 += 256) {
        const int r1 = std::min(b, r0 + 256);
        cols.clear();
        for (int p = r0; p < r1; p++) {  // positions; the row at p is rowat(p)
          const int ch = p / 64, ln = p % 64, row = rowat(p);
          for (int sl = s0; sl < cl[ch]; sl++) {
            const int j = cc[size_t(co[ch]) + 64 * sl + ln];
            if (j != row) cols.push_back(j);
          }
        }
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        if (cols.size() >= 0xFFFF) return false;
        for (int p = r0; p < r1; p++) {
          const int ch = p / 64, ln = p % 64, row = rowat(p);
          for (int sl = s0; sl < cl[ch]; sl++) {
            const size_t pos = size_t(co[ch]) + 64 * sl + ln;
            if (cc[pos] != row)
              idx[pos] = uint16_t(std::lower_bound(cols.begin(), cols.end(), cc[pos]) - cols.begin());
          }
        }
        lst.insert(lst.end(), cols.begin(), cols.end());
        ptr.push_back(int(lst.size()));
      }
    }
    return true;
  };
  std::vector<int> &lp = X.lptr, &ll = X.llist, &up2 = X.uptr, &ul = X.ulist;
  std::vector<uint16_t> &li = X.lidx, &ui = X.uidx;
  const bool ok = lists(S.lchunk_len, S.lchunk_off, S.lcolidx, 0, rowL, lp, ll, li) &&
                  lists(S.uchunk_len, S.uchunk_off, S.ucolidx, 1, rowU, up2, ul, ui);
  int mx = 0;
  for (size_t k = 0; ok && k + 1 < lp.size(); k++) mx = std::max(mx, lp[k + 1] - lp[k]);
  for (size_t k = 0; ok && k + 1 < up2.size(); k++) mx = std::max(mx, up2[k + 1] - up2[k]);
  if (ok && nc <= 256 && size_t(mx) * 3 * 8 <= 64 * 1024) {
    X.usable = true;
    X.sx_max = mx;
    // for the one-launch ILU(0) application's dependency lists (ilu_flow_build)
    X.posrowL.resize(npos);
    X.posrowU.resize(npos);
    for (int pos = 0; pos < npos; pos++) {
      X.posrowL[pos] = rowL(pos);
      X.posrowU[pos] = rowU(pos);
    }
  } else {
    X = SweepLists();
  }
}

// row-contiguous block offsets and columns of the owned rows (fused ILU(0) factorisation)
void derive_row_lists(const LocalLayout &L, RowLists &R) {
  std::vector<int> &ro = R.rowoff, &rcol = R.rowcol;
  ro.assign(L.n_owned + 1, 0), rcol.clear();
  rcol.reserve(size_t(L.nblocks));
  for (int i = 0; i < L.n_owned; i++) {
    const int ch = i / kChunk, ln = i % kChunk, len = meta_len(L.rowmeta[i]);
    for (int sl = 0; sl < len; sl++)
      rcol.push_back(L.colidx[size_t(L.chunk_off[ch]) + 64 * size_t(sl) + ln]);
    ro[i + 1] = ro[i] + len;
  }
}

// spatial block order (DevLayout::blkmap) for the whole-matrix kernels (assembly, SpMV):
// each XCD takes one spatial slice of every colour, so the neighbour gathers of its rows
// share its L2.  With the gather-all assembly it pays 72.7 -> 58.8 us (the pipelined walk
// was latency-bound and did not see it; SpMV and sweeps neutral,
// profiles/r01/ab_blkmap_gather_all.log).  PNP_BLKMAP=0 turns it off (A/B)
void derive_blkmap(const LocalLayout &L, const LayoutKnobs &K, std::vector<int> &blkmap) {
  blkmap.clear();
  if (K.blkmap && L.n_owned > 0) {
    int nblk = (L.n_owned + 255) / 256;
    std::vector<double> key(nblk);
    for (int b = 0; b < nblk; b++) {
      int r = 256 * b, cc = L.rowcolor[r];
      double lo = L.color_ptr[cc], hi = L.color_ptr[cc + 1];
      key[b] = (r - lo) / std::max(1.0, hi - lo);
    }
    std::vector<int> order(nblk);
    for (int b = 0; b < nblk; b++) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
    blkmap = std::move(order);
  }
}

// boundary segments for the ion-flux observable
bool derive_flux_segments(const Mesh &mg, const LocalLayout &L, FluxSegs &F, std::string &err) {
  auto ekey = [](int a, int b) {
    if (a > b) std::swap(a, b);
    return (long long)a << 32 | (unsigned)b;
  };
  std::unordered_map<long long, int> opp;
  opp.reserve(size_t(mg.nb) * 2);
  for (int b = 0; b < mg.nb; b++) opp[ekey(mg.bseg[2 * b], mg.bseg[2 * b + 1])] = -1;
  for (int e = 0; e < mg.nt; e++)
    for (int k = 0; k < 3; k++) {
      auto it = opp.find(ekey(mg.tri[3 * e + k], mg.tri[3 * e + (k + 1) % 3]));
      if (it != opp.end() && it->second < 0) it->second = mg.tri[3 * e + (k + 2) % 3];
    }
  std::vector<FluxSeg> &segs = F.segs;
  segs.clear(), F.group.clear();
  for (int b = 0; b < mg.nb; b++) {
    const int a = mg.bseg[2 * b], cc = mg.bseg[2 * b + 1], lo = L.g2l[std::min(a, cc)];
    if (lo < 0 || lo >= L.n_owned) continue;  // another rank's segment
    const int o = opp[ekey(a, cc)];
    const int la = L.g2l[a], lc = L.g2l[cc], lop = o >= 0 ? L.g2l[o] : -1;
    if (la < 0 || lc < 0 || lop < 0) {
      err = "ion flux: the element of a boundary segment is not local";
      return false;
    }
    segs.push_back(FluxSeg{la, lc, lop, mg.bgroup[b]});
    F.group.push_back(mg.bgroup[b]);
  }
  return true;
}

// per 256-row block: its distinct columns, and per slot the column's position among them
void derive_spmv_lists(const LocalLayout &L, const LayoutKnobs &K, SpmvLists &U) {
  U = SpmvLists();
  if (K.spmv_lds) {
    const int nblk = (L.n_owned + 255) / 256;
    std::vector<int> uptr(nblk + 1, 0), ulist;
    std::vector<uint16_t> lidx(size_t(L.nslots), 0);
    std::vector<int> cols, uown(nblk, 0);
    int umax = 0, unmax = 0;
    bool fits = true;
    const bool own_last = K.list_own_last;
    for (int b = 0; b < nblk && fits; b++) {
      cols.clear();
      const int r1 = std::min(L.n_owned, 256 * b + 256);
      for (int i = 256 * b; i < r1; i++) {
        const int ch = i / kChunk, ln = i % kChunk;
        for (int sl = 0; sl < L.chunk_len[ch]; sl++)
          cols.push_back(L.colidx[size_t(L.chunk_off[ch]) + 64 * size_t(sl) + ln]);
      }
      std::sort(cols.begin(), cols.end());
      cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
      if (cols.size() > 65535) fits = false;
      umax = std::max(umax, int(cols.size()));
      // columns that are only a row's own slot 0 last (PNP_LIST_OWN_LAST, default): the assembly
      // walk stages only the first uown[b] entries, the columns of slots >= 1 (fan neighbours; a
      // block's rows are mostly of one colour, so its own rows are rarely among them); the SpMV
      // stages all
      std::vector<int> npos(cols.size());
      int nn = 0;
      if (own_last) {
        std::vector<char> nb(cols.size(), 0);
        for (int i = 256 * b; i < r1; i++) {
          const int ch = i / kChunk, ln = i % kChunk;
          for (int sl = 1; sl < L.chunk_len[ch]; sl++) {
            const int j = L.colidx[size_t(L.chunk_off[ch]) + 64 * size_t(sl) + ln];
            if (j != i) nb[std::lower_bound(cols.begin(), cols.end(), j) - cols.begin()] = 1;
          }
        }
        for (size_t k = 0; k < cols.size(); k++)
          if (nb[k]) npos[k] = nn++;
        int no = nn;
        for (size_t k = 0; k < cols.size(); k++)
          if (!nb[k]) npos[k] = no++;
      } else {
        for (size_t k = 0; k < cols.size(); k++) npos[k] = int(k);
        nn = int(cols.size());
      }
      uown[b] = nn;
      unmax = std::max(unmax, nn);
      for (int i = 256 * b; i < r1; i++) {
        const int ch = i / kChunk, ln = i % kChunk;
        for (int sl = 0; sl < L.chunk_len[ch]; sl++) {
          const size_t pos = size_t(L.chunk_off[ch]) + 64 * size_t(sl) + ln;
          lidx[pos] = uint16_t(npos[std::lower_bound(cols.begin(), cols.end(), L.colidx[pos]) - cols.begin()]);
        }
      }
      std::vector<int> reord(cols.size());
      for (size_t k = 0; k < cols.size(); k++) reord[npos[k]] = cols[k];
      ulist.insert(ulist.end(), reord.begin(), reord.end());
      uptr[b + 1] = int(ulist.size());
    }
    if (fits && size_t(umax) * 3 * 8 <= 64 * 1024) {
      U.usable = true;
      U.uptr = std::move(uptr);
      U.ulist = std::move(ulist);
      U.lidx = std::move(lidx);
      U.umax = umax;
      U.uown = std::move(uown);
      U.unmax = unmax;
    }
  }
}

// halo-overlapped SpMV: interior / boundary 256-row blocks
void derive_block_split(const LocalLayout &L, const LayoutKnobs &K, const std::vector<int> &blkmap,
                        BlockSplit &B) {
  B = BlockSplit();
  if (K.halo_overlap && L.n_owned > 0) {
    const int nblk = (L.n_owned + 255) / 256;
    std::vector<int> order(nblk);
    if (!blkmap.empty()) {
      order = blkmap;
    } else {
      for (int b = 0; b < nblk; b++) order[b] = b;
    }
    std::vector<int> &bi = B.interior, &bb = B.boundary;
    for (int b : order) {
      bool bnd = false;
      for (int i = 256 * b; i < std::min(L.n_owned, 256 * b + 256) && !bnd; i++) {
        const int ch = i / kChunk, ln = i % kChunk, len = meta_len(L.rowmeta[i]);
        for (int sl = 1; sl < len && !bnd; sl++)
          bnd = L.colidx[size_t(L.chunk_off[ch]) + 64 * size_t(sl) + ln] >= L.n_owned;
      }
      (bnd ? bb : bi).push_back(b);
    }
    B.usable = true;
  }
}

bool derive_layout(const Mesh &m, const LocalLayout &L, const LayoutKnobs &K, DerivedLayout &D,
                   std::string &err) {
  derive_split(L, K, D.split);
  derive_sweep_lists(L, D.split, D.sweep);
  derive_row_lists(L, D.rows);
  derive_blkmap(L, K, D.blkmap);
  if (!derive_flux_segments(m, L, D.flux, err)) return false;
  derive_spmv_lists(L, K, D.spmv);
  derive_block_split(L, K, D.blkmap, D.halo);
  return true;
}

KeptLayout keep_layout(DerivedLayout &&D) {
  KeptLayout H;
  H.posrowL = std::move(D.sweep.posrowL);
  H.posrowU = std::move(D.sweep.posrowU);
  H.lsx_ptr = std::move(D.sweep.lptr);
  H.lsx_list = std::move(D.sweep.llist);
  H.usx_ptr = std::move(D.sweep.uptr);
  H.usx_list = std::move(D.sweep.ulist);
  H.blkmap = std::move(D.blkmap);
  H.lslots_live = D.split.lslots_live;
  H.uslots_live = D.split.uslots_live;
  return H;
}

bool build_host_layout(Mesh &mesh, int degree, int rank, int nranks, Mesh &tmesh, PkSpace &pks,
                       Fans &fans, LocalLayout &L, std::string &err) {
  if (degree > 1) {  // the layout is built on the node graph of the P_k space
    if (!validate(mesh, err) || !build_pk_space(mesh, degree, pks, err)) return false;
    tmesh = std::move(mesh);
    mesh = pk_node_mesh(pks);
    if (!pk_adjacency(tmesh, pks, fans, err)) return false;
  } else if (!build_fans(mesh, fans, err)) {
    return false;
  }
  std::vector<int> part;
  rcb_partition(mesh, nranks, part);
  {  // every rank computes the same partition: all of them fail here, before any collective or
     // group barrier, when one part is empty (more ranks than vertices)
    std::vector<int> cnt(nranks, 0);
    for (int p : part) cnt[p]++;
    for (int r = 0; r < nranks; r++)
      if (cnt[r] == 0) {
        err = "partition: rank " + std::to_string(r) + " of " + std::to_string(nranks) +
              " owns no vertices (the mesh has " + std::to_string(mesh.nv) + ")";
        return false;
      }
  }
  return build_local_layout(mesh, fans, part, rank, nranks, L, err);
}

}  // namespace pnp
