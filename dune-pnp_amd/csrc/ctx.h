// The context behind the C ABI (include/pnp_capi.h): its data, the small accessors and the
// declarations of the member functions defined in ctx.cc (everything but the linear solvers),
// krylov.cc (the linear solvers) and md.cc (the operator-split time loop).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <queue>
#include <random>
#include <chrono>
#include <condition_variable>
#include <map>
#include <unordered_map>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pnp_capi.h"
#include "amg.h"
#include "cheb_small.h"
#include "gmres_small.h"
#include "idr_small.h"
#include "kernels.h"
#include "layout_derive.h"
#include "mesh.h"
#include "pk.h"

template <typename T>
struct DBuf {
  T *p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc(&p, sizeof(T) * count);
    if (e == hipSuccess) e = hipMemset(p, 0, sizeof(T) * count);  // no reliance on fresh pages
    // the memset runs on the null stream, which does not order against the context's
    // non-blocking streams: finish it before a kernel there writes the buffer (seen as zeroed
    // FD element matrices with 8 in-process ranks competing for the GPU)
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DBuf() { release(); }
};

enum TimerCat { T_ASM = 0, T_SPMV, T_PREC, T_BLAS, T_HALO, T_ALLRED, T_FACT, T_NCAT };

inline double now_s() {
  using namespace std::chrono;
  return duration<double>(steady_clock::now().time_since_epoch()).count();
}

struct pnp_mesh_buf {
  pnp::Mesh m;
};

// In-process communicator for tests on one GPU (pnp_comm::local_group): ranks are contexts in
// one process, each driven by its own host thread.  Collectives are host barriers plus
// device-to-device copies; every call synchronises, which is fine for correctness tests.
struct LocalGroup {
  int size = 0;
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  long generation = 0;
  std::vector<pnp_ctx *> members;
  std::vector<std::vector<double>> host;  // per-rank published host values (allreduce)
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    long gen = generation;
    if (++arrived == size) {
      arrived = 0;
      generation++;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != gen; });
    }
  }
};
extern std::mutex g_groups_m;
extern std::map<std::string, std::shared_ptr<LocalGroup>> g_groups;

struct pnp_ctx {
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  int rank = 0, nranks = 1;
  // the multi-rank code path (reduce -> allreduce -> derive, halo-split SpMV, two-reduction
  // BiCGSTAB): more than one rank, or one rank with an RCCL communicator of its own (a pnp_comm of
  // size 1 with an RCCL id -- the N > 1 path on one GPU, every allreduce a real ncclAllReduce)
  bool dist = false;
  ncclComm_t comm = nullptr;
  std::shared_ptr<LocalGroup> lg;  // test transport instead of RCCL
  pnp_host_transport ht{};         // host-staged transport (pnp_comm.host), if ht.exchange
  double *h_send = nullptr, *h_recv = nullptr, *h_red = nullptr;  // its pinned staging buffers
  size_t h_red_n = 0;
  bool host_tr() const { return ht.exchange != nullptr; }

  // P_k, k > 1 (pnp_create_pk): `mesh` is the node mesh (nv = Lagrange nodes, no elements) the
  // partition, layout and external vectors are built on; tmesh the triangle mesh, pks the space
  int degree = 1;
  pnp::Mesh mesh, tmesh;
  pnp::PkSpace pks;
  pnp::PkDev pkd;
  DBuf<int> pk_enode, pk_ioff, pk_icnt, pk_inc;
  DBuf<uint32_t> pk_islot;
  DBuf<double> pk_eres, pk_ejac;
  DBuf<int> pk_blk_short, pk_blk_long;
  pnp::Params params;
  pnp::Fans fans;
  pnp::LocalLayout L;
  pnp::DevLayout dl;

  DBuf<int> d_chunk_len, d_chunk_off, d_colidx, d_l2g, d_send_idx, d_color_idx;
  DBuf<uint8_t> d_rowcolor;
  DBuf<uint64_t> d_rowmeta;
  DBuf<int> d_uptr, d_ulist;   // LDS-staged SpMV lists (PNP_SPMV_LDS, DevLayout::uptr)
  DBuf<int> d_uown;            // per block: list entries before its own rows (DevLayout::uown)
  DBuf<int> d_lsx_ptr, d_lsx_list, d_usx_ptr, d_usx_list;  // LDS-staged sweeps (DevLayout lsx_*)
  DBuf<uint16_t> d_lsx_idx, d_usx_idx;
  DBuf<uint8_t> d_lperm, d_uperm, d_lpinv, d_upinv, d_llen, d_ulen, d_ldl;  // split lane order
  DBuf<uint16_t> d_lidx;
  DBuf<double> d_xy;

  // operator
  int kind = -1, nf = 0, pat = 0, nvb = 0, nks = 0;  // nvb: block pattern size, nks: stored
  std::vector<uint8_t> hmask;  // Dirichlet mask of the current operator, owned rows x nf
  pnp::AsmArgs aa{};

  // ---- what the context holds of the current operator's Jacobian --------------
  // The flags, and the only functions that write them: the transitions below, and for each derived
  // object the function that computes it.
  //   assembled       a Jacobian of the current operator is held.  Every reader of the flags down
  //                   to amg_valid sits behind it.  Set by jacobian_stored / seq_jacobian_stored,
  //                   cleared by jacobian_drop (and by md_run after a failed solve)
  //   mf_lin          it is held as a linearisation point (PNP_OPT_MATRIX_FREE, or on a P_k context
  //                   pnp_pk_matfree_set): jacobian_stored(mf)
  //   vals_stale      ... and vals does not hold its values yet: jacobian_stored(mf) sets,
  //                   ensure_values clears; mf_settle and jacobian_drop clear both
  //   mf_diag_valid   mf_diag holds its diagonal blocks: jacobi_prepare sets, every transition clears
  //   csr_vals_valid  csr_val holds it: set by csr_values, and by seq_jacobian_stored (the
  //                   reference-order Jacobian lives there only); cleared by jacobian_stored,
  //                   jacobian_drop and a new csr_structure
  //   lu_valid        lu (fused factorisation: lvals / uvals) holds its ILU(0) factors: ilu_factor
  //                   sets; derived_drop and ilu_factors_drop clear
  //   split_of        what lvals / uvals hold of it: 0 nothing, 1 the matrix (SSOR), 2 the factors.
  //                   split and ilu_factor set; derived_drop clears, ilu_factors_drop clears a 2
  //   amg_valid       the AMG's coarse values come from it: amg_setup sets; derived_drop and
  //                   amg_values_drop (pnp_amg_configure) clear
  //   cheb_valid      cheb_coef holds the Chebyshev coefficients for its bounds (estimated from it,
  //                   or the caller's) and the configured steps: cheb_prepare sets; derived_drop and
  //                   pnp_cheb_configure clear
  // and of the operator itself:
  //   vals_const_valid  vals holds the PNP k-form's state-independent planes for the operator set
  //                   now: set by a P1 analytic assembly that wrote every plane (asm_wrote), cleared
  //                   by whatever else zeroes or writes vals (op_activate, set_fd, the FD and P_k
  //                   Jacobians, a failed launch).  About the contents of vals, not about a derived
  //                   object: jacobian_drop leaves it alone
  //   seq_op_valid    the reference-order copies of the operator are on the device: seq_prepare sets,
  //                   op_activate clears
  bool assembled = false, mf_lin = false, vals_stale = false, mf_diag_valid = false;
  bool csr_vals_valid = false, lu_valid = false, amg_valid = false, cheb_valid = false;
  int split_of = 0;
  bool vals_const_valid = false, seq_op_valid = false;
  // what is computed from the stored Jacobian's values
  void derived_drop() {
    lu_valid = false;
    split_of = 0;
    amg_valid = false;
    cheb_valid = false;
  }
  void amg_values_drop() { amg_valid = false; }
  // the factors are recomputed (another factorisation path or precision); a split matrix stays
  void ilu_factors_drop() {
    if (split_of == 2) split_of = 0;
    lu_valid = false;
  }
  // assemble() now holds a Jacobian: in vals, or (mf) as a linearisation point
  void jacobian_stored(bool mf) {
    assembled = true;
    derived_drop();
    csr_vals_valid = false;
    mf_lin = vals_stale = mf;
    mf_diag_valid = false;
  }
  // seq_jacobian() now holds one, in the CSR view only.  The mf_* flags stay: they describe the
  // k-form Jacobian pnp_assemble_state may have stored in this mode, which
  // pnp_bicgstab_iterations goes on applying
  void seq_jacobian_stored() {
    assembled = true;
    derived_drop();
    csr_vals_valid = true;
  }
  // no Jacobian is held: another operator, value layout or arithmetic order comes next
  void jacobian_drop() {
    assembled = false;
    derived_drop();
    csr_vals_valid = false;
    mf_lin = vals_stale = mf_diag_valid = false;
  }
  // PNP_OPT_MATRIX_FREE off: the current Jacobian goes on as an assembled one -- its values, if
  // nobody needed them yet
  int mf_settle() {
    if (int rc = ensure_values()) return rc;
    mf_lin = mf_diag_valid = false;
    return PNP_OK;
  }
  // the current operator: fields, block pattern of the analytic Jacobian
  static int nfields_of(int kind) {
    return (kind == PNP_OP_PNP || kind == PNP_OP_PNP_IMPLICIT_EULER) ? 3 : 1;
  }
  static int base_pat(int kind) {
    return kind == PNP_OP_PNP ? pnp::kPatPnp
                              : (kind == PNP_OP_PNP_IMPLICIT_EULER ? pnp::kPatPnpIE : pnp::kPatScalar);
  }
  // `kind` becomes the current operator (pnp_set_operator, md_activate; ctx.cc): pattern, no
  // Jacobian, vals zeroed on the stream, the AsmArgs on the context's operator buffers -- which
  // the caller fills (mask, row flags, load, frozen fields), with the reference-order copies
  int op_activate(int kind, double dt, double z);
  // the P1 assembly's flag byte per owned row, whole SELL chunks (ctx.cc)
  std::vector<uint8_t> row_flags(int nfk, bool ie, const std::vector<uint8_t> &lmask,
                                 const std::vector<double> &lload, const double *c_extra) const;

  DBuf<double> vals, lu;  // matrix and its ILU(0) factors
  // triangular split storage (DevLayout l*/u*): lvals/uvals hold either the matrix (SSOR) or the
  // ILU(0) factors; split_of says which is current
  DBuf<int> d_lchunk_len, d_lchunk_off, d_lcolidx, d_lsrc, d_uchunk_len, d_uchunk_off, d_ucolidx,
      d_usrc;
  DBuf<double> lvals, uvals, tsgs;
  // ILU(0) factors in the split storage in single precision (PNP_OPT_ILU_F32, default 1; the
  // sweeps compute in fp64, the matrix, SpMV, SSOR and every vector stay fp64).  Measured at
  // config 3: ILU(0) apply 119 -> 95 us, BiCGSTAB 428 -> 389 us/it, Newton 9,295 -> 9,177
  // iterations (profiles/r02/ab_ilu_f32.log)
  // 2 (the default since round 5): bfloat16 factors for block systems (linalg.hip bf16s: 14 B per
  // PNP block instead of 28 -- 16 B until ILU_BF16_B7; ILU(0) apply 66.3 -> 58.6 us, BiCGSTAB 0.285 -> 0.270 ms per
  // iteration at config 3, Newton counts inside their last-bit spread); scalar
  // systems (PB, Poisson, diffusion: one value per block, 2 B saved per slot) keep f32, where the
  // PB Newton at config 1 took 13 % more iterations with bf16
  // 3 (opt-in): the bf16 factors of 2, and the forward sweep's intermediate y = L^-1 d kept in
  // single precision (ilu_y32: 12 B per PNP row written, re-read by the backward sweep and gathered
  // by the forward one, instead of 24): apply 56.3 -> 54.5 us at config 3, but the rounding makes
  // the preconditioner nonlinear (2-5e-8 relative per application), which BiCGSTAB's short
  // recurrences do not tolerate: 408 -> 710 iterations on a config-5 solve, the config-5 Newton
  // and the config-4 AMG steps stall, so not the default.  The dataflow form (PNP_OPT_ILU_FLOW) keeps y in fp64 and runs
  // 3 as 2
  int ilu_f32 = [] {
    const char *e = std::getenv("PNP_ILU_F32");
    const int v = e ? std::atoi(e) : 2;
    return (v >= 0 && v <= 3) ? v : 2;
  }();
  int ilu_eff() const { return (ilu_f32 >= 2 && nf == 1) ? 1 : ilu_f32; }
  // the factors' storage: 0 fp64, 1 f32, 2 bf16 (the kernels' f32 argument)
  int ilu_fac() const { return ilu_eff() == 3 ? 2 : ilu_eff(); }
  int f32_now() const { return split_of == 2 ? ilu_fac() : 0; }
  // the single-precision forward intermediate of the colour launches, or null
  DBuf<float> ilu_y32buf;
  float *ilu_y32() const {
    return (split_of == 2 && ilu_eff() == 3 && !ilu_flow_opt) ? ilu_y32buf.p : nullptr;
  }
  int ilu_fused = 1;  // PNP_OPT_ILU_FUSED_FACTOR
  int amg_fallback = 0;  // PNP_OPT_AMG_FALLBACK
  int ilu_retry = 1;     // PNP_OPT_ILU_RETRY
  int twored_opt = [] {  // PNP_OPT_BICG_TWORED: -1 auto (on with more than one rank), 0, 1
    const char *ev = std::getenv("PNP_BICG_TWORED");
    return ev ? (std::atoi(ev) != 0 ? 1 : 0) : -1;
  }();
  DBuf<int> d_blkmap;
  DBuf<int> d_rowoff, d_rowcol;  // row-contiguous block offsets / columns (fused ILU(0) factor)
  // halo-overlapped SpMV (multi-GPU): 256-row blocks without / with ghost columns, each in the
  // spatial order of blkmap; the halo runs on cstream while the interior blocks compute
  DBuf<int> d_blk_int, d_blk_bnd;
  int n_blk_int = 0, n_blk_bnd = 0;
  bool split_spmv = false;
  pnp::DevLayout sub_layout(bool interior) const {
    pnp::DevLayout d = dl;
    d.blkmap = interior ? d_blk_int.p : d_blk_bnd.p;
    const int n = interior ? n_blk_int : n_blk_bnd;
    d.blkcount = n > 0 ? n : -1;  // -1: no block (launch nothing)
    return d;
  }
  hipStream_t cstream = nullptr;
  hipEvent_t ev_ready = nullptr, ev_halo = nullptr;
  DBuf<double> scrub;  // pnp_cache_scrub (cache-cold benchmark timings)
  // forward-difference Jacobian (PNP_JAC_FD, fd_jacobian.hip): local elements, per-row block
  // contribution lists, element matrices; built on first use
  bool fd_built = false, fd_mode = false;
  int fd_opt = 0;  // PNP_OPT_JAC_FD: every Jacobian assembly (Newton's too) by forward differences
  int fd_ne = 0;
  DBuf<int> fd_etri, fd_cdata;
  DBuf<long long> fd_rptr;
  DBuf<double> fd_jel;
  // device CSR view (pnp_jacobian_csr_device): structure per block pattern, values per request
  int csr_pat = -1, csr_nf = 0;
  long long csr_nnz = 0;
  DBuf<int> csr_rowptr, csr_col, csr_src;
  DBuf<unsigned char> csr_vidx;
  DBuf<double> csr_val;
  // natural-order SSOR (PNP_PREC_SSOR_NATURAL, ssor_natural.hip): level schedules of the forward
  // and backward sweeps over the external-layout rows with each level's rows as an ELL over the
  // CSR (pnp::NatSweep; built with the CSR structure), and external-layout work vectors
  struct NatDir {
    std::vector<int> lptr;
    std::vector<long long> eoff;
    DBuf<int4> info;
    DBuf<int> ecol;
    // the tail as chains (PNP_NAT_CHAIN): lane-group row lists, rows, padded entries
    bool chain_ok = false;
    int chain_groups = 0, chain_wpad = 0;
    DBuf<int> cgptr, cecode;
    DBuf<int4> crec;
    pnp::NatFlow::Chains chains() const {
      pnp::NatFlow::Chains c;
      if (!chain_ok) return c;
      c.ngroups = chain_groups;
      c.wpad = chain_wpad;
      c.gptr = cgptr.p;
      c.rec = crec.p;
      c.ecode = cecode.p;
      return c;
    }
    pnp::NatSweep view() const {
      pnp::NatSweep w;
      w.nlev = int(lptr.size()) - 1;
      w.lptr = lptr.data();
      w.eoff = eoff.data();
      w.info = info.p;
      w.ecol = ecol.p;
      return w;
    }
  };
  NatDir nat_f, nat_b;
  DBuf<double> nat_d, nat_v, nat_vf;  // external layout: d (level launches), vb, vf
  DBuf<double> nat_di, nat_vi;        // internal layout temporaries (reference-order mode)
  // the one-launch dataflow sweep (launch_ssor_natural_flow): units, forward units first
  std::vector<int4> nat_units;
  DBuf<int4> d_nat_units;
  int nat_units_f = 0, nat_tail_f = 0, nat_tail_b = 0, nat_max_width = 0;
  bool nat_units_ok = false;
  DBuf<unsigned> nat_abort;  // [0]: set by a sweep whose operand wait timed out (sticky)
  DBuf<int> csr_diag;        // index of each CSR-view row's diagonal entry
  // ILU(0) application as one dataflow launch (PNP_OPT_ILU_FLOW, linalg.hip k_ilu0_flow): per
  // c_first (0: every colour in the launch, 1: colour 0's forward step done by the update kernel)
  // the unit table and dependency lists, built on first use from the staging lists (host copies
  // kept from the layout build: rows at each L / U split position, lsx / usx lists)
  int ilu_flow_opt = [] {
    const char *e = std::getenv("PNP_ILU_FLOW");
    return (e && std::atoi(e) != 0) ? 1 : 0;
  }();
  // what stays on the host of the derived layout (layout_derive.h): those copies, blkmap
  // (pk_build) and the live-slot counts (pnp_info)
  pnp::KeptLayout hl;
  struct IluFlowDev {
    bool built = false, ok = false;
    pnp::IluFlow F;
    DBuf<int> dep_ptr, dep_list;
    DBuf<unsigned> flags;
  };
  IluFlowDev ilu_flow[2];
  DBuf<unsigned> ilu_flow_abort;
  bool ilu_flow_used = false;  // a flow launch ran since the last check
  long long ilu_flow_n = 0;    // flow launches issued (pnp_info; a graph capture counts once)
  // ---- reference-order mode (PNP_OPT_SEQ_ORDER, seq_order.hip) -----------------------------
  int seq_opt = 0;
  bool seq_built = false;
  DBuf<int> seq_tri, seq_vptr, seq_vinc;
  DBuf<double> seq_xy;
  // the operator's data as the reference holds it: constrained rows (external layout), frozen
  // fields, x_old, implicit-Euler dt / valency (host copies taken by pnp_set_operator)
  std::vector<uint8_t> seq_mask_h;
  std::vector<double> seq_phi_h, seq_cp_h, seq_cm_h, seq_xold_h;
  double seq_dt = 0, seq_z = 0;
  bool seq_cextra = false;
  DBuf<unsigned char> seq_mask;
  DBuf<int> seq_bptr;
  DBuf<double> seq_bval, seq_phi, seq_cp, seq_cm, seq_xold;
  DBuf<double> seq_rl, seq_rlt, seq_rlo, seq_jl, seq_jlt, seq_vec, seq_dotv;
  int nat_pat = -1, nat_nf = 0;
  // ion-current observable (pnp_ion_flux): boundary segments handled by this rank (the owner of
  // the segment's lower global vertex), {a, c, opposite vertex, group} in local indices, in
  // global segment order
  DBuf<int4> d_fseg;
  std::vector<int> fseg_group;
  DBuf<double> fluxout, fluxx, fluxred;
  DBuf<uint8_t> dmask;
  // AsmArgs::rowflag of the operator set now: a byte per owned row, whole SELL chunks (padding 0)
  DBuf<uint8_t> rowflag;
  std::vector<uint8_t> hrowflag;  // its owned rows on the host (pnp_asm_row_flags)
  DBuf<double> cvec, aux0, aux1;
  bool after_solve = false;  // a linear solve ran since the last Jacobian assembly (AsmArgs::cold)
  // ---- matrix-free Jacobian application (PNP_OPT_MATRIX_FREE, jac_apply.hip) ----
  // With the option on, a Jacobian "assembly" of a P1 analytic operator records the linearisation
  // point (mf_x: the state with ghosts; mf_aa: the operator's arguments at that moment) and leaves
  // the SELL values stale; halo_spmv and pnp_jacobian_apply compute J z from the point, and the
  // consumers of vals (SSOR / ILU(0) / AMG set-up, the CSR view, the export) first run the
  // ordinary assembly at the point (ensure_values).
  // P_k contexts (degree 2, 3) have a switch of their own, pnp_pk_matfree_set (pk_mf_opt; mf_opt
  // stays 0 there, PNP_OPT_MATRIX_FREE = 1 being refused): the same record and flags, the two-pass
  // kernels of pk_assemble.hip (launch_pk_jac_apply / launch_pk_jac_diag) in place of the fan walk,
  // and halo_spmv unsplit (the element pass reads ghosts of the vector).
  int mf_opt = 0, pk_mf_opt = 0;
  bool mf_on() const { return degree == 1 ? mf_opt != 0 : pk_mf_opt != 0; }
  pnp::AsmArgs mf_aa{};
  DBuf<double> mf_x, mf_r;  // the point; the residual ensure_values' fused assembly also writes
  // Jacobi without SELL values: the diagonal blocks alone, one slot per chunk (launch_jac_diag),
  // read by launch_jacobi through a layout whose chunk_off[c] = 64 c
  DBuf<double> mf_diag;
  DBuf<int> mf_choff;
  long long mf_applies = 0, value_assemblies = 0;  // pnp_matfree_info
  // ---- state-independent planes of the PNP k-form (PNP_OPT_ASM_REUSE_CONST) ----
  // k0 / k1 of every PNP block depend on the mesh and the parameters only.  While vals_const_valid
  // holds, the PNP Jacobian assembly leaves those planes alone (AsmArgs::kconst).
  int asm_reuse_opt = [] {  // the environment variable PNP_ASM_REUSE_CONST=0/1 sets the default
    const char *e = std::getenv("PNP_ASM_REUSE_CONST");
    return (e && std::atoi(e) == 0) ? 0 : 1;
  }();
  // pnp_asm_info; asm_piped: launches of the persistent, prefetching walk (PNP_ASM_PIPE)
  long long asm_full = 0, asm_reused = 0, asm_piped = 0;
  // (the variant exists for the gather-all walk only: layouts with a fan of more than 8 neighbours
  // take launch_assemble's longer-fan walks, which write every plane and count as full writes)
  bool asm_kconst() const {
    return asm_reuse_opt && vals_const_valid && degree == 1 && !fd_mode && kind == PNP_OP_PNP &&
           dl.max_slots <= 9;
  }
  void asm_wrote(bool kc, bool full);

  // aggregation AMG (PNP_PREC_AMG, amg.h): the pattern hierarchy is built once per context (it
  // depends on the layout only), the coarse values after every assembly
  pnp_amg_opts amg_opts{PNP_PREC_SSOR, pnp::kAmgMaxCoarse, 12, 0.8, 2, -1};
  bool amg_symmetric = true;  // set per solve: CG needs the symmetric V-cycle
  std::vector<pnp::AmgLevelHost> amg_h;
  struct AmgDev {
    int nb = 0;
    DBuf<int> rp, col, dpos, mptr, mem, agg, csrc;
    DBuf<long long> cptr;
    DBuf<double> v, dinv, b, x, x2;
    DBuf<float> vf;  // single-precision values for the V-cycle's sweeps (amg_f32; null: fp64)
  };
  // PNP_AMG_F32 (default 1): the coarse levels' sweeps and residuals read single-precision block
  // values, and the coarsest solve a single-precision copy of its inverse (the arithmetic, the
  // Galerkin products, the diagonal inverses and the LU / inverse themselves stay fp64), as the
  // ILU(0) factors do; 0 keeps fp64 (A/B)
  static bool amg_f32() {
    static const bool v = [] {
      const char *e = std::getenv("PNP_AMG_F32");
      return !(e && e[0] == '0');
    }();
    return v;
  }
  std::vector<std::unique_ptr<AmgDev>> amg_d;  // amg_d[k] = level k + 1
  bool amg_built = false;
  int amg_nf = 0;
  double amg_setup_ms = 0;
  DBuf<double> amg_ainv, amg_x0, amg_t, amg_y, amg_r, amg_z;
  DBuf<float> amg_ainv_f;  // amg_f32(): the inverse in single precision, rows padded to amg_ld
  int amg_ld = 0;
  DBuf<int> amg_ipiv, amg_info;
  rocblas_handle blas = nullptr;  // rocSOLVER getrf/getri of the AMG's coarsest level

  // ---- Chebyshev polynomial preconditioner (PNP_PREC_CHEBYSHEV) ----------------
  // cheb_p: the double-buffered direction with its ghosts (zeroed once; the stand-alone form
  // exchanges them per step, the AMG's rank-local form keeps them zero); cheb_r: the recurrence's
  // residual; cheb_t: A p of the unfused step; cheb_coef: the coefficients the kernels read
  // (cheb_small.h), rewritten by cheb_prepare, so that a captured graph outlives a new Jacobian
  pnp_cheb_opts cheb_opts{3, 10.0, 20, 1.1, 0.0};
  DBuf<double> cheb_r, cheb_t, cheb_p[2], cheb_coef;
  double cheb_hcoef[pnp::kChebCoefDoubles] = {0};
  double cheb_lest = 0, cheb_lmax = 0, cheb_lmin = 0;  // the bounds last used (pnp_cheb_info)
  bool cheb_ghosts_dirty = false;  // a stand-alone application has written the ghosts of cheb_p
  long long cheb_applies = 0, cheb_estimates = 0, cheb_fused = 0, cheb_unfused = 0;
  int cheb_estimate(double &lest);
  int cheb_prepare();
  // local: the owned x owned operator without a halo (inside amg_apply), else the global one
  int cheb_apply(const double *d, double *vout, bool local);

  // vectors (sized n_local * 3)
  DBuf<double> x, r, rs, z, rt, p, v, t, y, y2, b, prevu, ext, sendbuf, partials, partials2;
  DBuf<double> redmw;  // the multi-workgroup reduction's ticket and slice sums (main stream only)
  std::vector<int> newton_its;        // pnp_newton_history: linear iterations per Newton step
  std::vector<double> newton_defects; // and the defect after each step
  DBuf<pnp::Scalars> S;
  pnp::Scalars *hS = nullptr;  // pinned host mirror
  // restarted GMRES / FGMRES (gmres()): basis V, preconditioned basis Z (flexible only), the
  // orthogonalisation's partials, the device state block and history; allocated on first use
  int gm_restart = 30;  // PNP_OPT_GMRES_RESTART
  DBuf<double> gm_V, gm_Z, gm_part, gm_hist;
  DBuf<pnp::GmresState> gm_S;
  std::vector<double> gm_history;  // the last GMRES / FGMRES / IDR solve's (pnp_solve_history)
  // IDR(s) (idr()): the n x s arrays G (owned rows), U (with ghosts) and the shadow matrix P, the
  // reductions' partials, the device state block and history; allocated on first use
  int idr_s = pnp::kIdrDefaultS;  // PNP_OPT_IDR_S
  int idr_P_s = 0, idr_P_nf = 0;  // what idr_P was generated for (0: not generated)
  DBuf<double> idr_G, idr_U, idr_P, idr_part, idr_hist;
  DBuf<pnp::IdrState> idr_S;
  long long idr_replacements = 0;  // residual replacements since the context was created

  // timers / debugging
  bool timing = false;
  bool debug_trace = [] {
    const char *e = std::getenv("PNP_DEBUG_BICGSTAB");
    return e && std::atoi(e) != 0;
  }();
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending[T_NCAT];
  std::vector<hipEvent_t> ev_pool;
  double t_ms[T_NCAT] = {0};
  long long t_n[T_NCAT] = {0};

  ~pnp_ctx();

  // ---- hipGraph replay of BiCGSTAB iteration blocks (PNP_OPT_GRAPH) ------------------------------
  // -1 auto: on for up to 131,072 owned rows (launch-bound sizes), 0 off, 1 on
  int graph_opt = [] {
    const char *e = std::getenv("PNP_GRAPH");
    return e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
  }();
  bool use_graphs() const {
    return graph_opt == 1 || (graph_opt < 0 && L.n_owned <= (1 << 17) && !profiled());
  }
  static bool profiled();
  struct GraphKey {
    int count, prec, fuse, nf, pat, f32, flow;
    int mf;  // the operator application: 0 the SpMV, 1 matrix-free, 2 matrix-free with the SELL
             // values stale (Jacobi then reads the diagonal blocks of jacobi_prepare())
    const void *zout, *dmask;
    long long epoch;
    bool operator==(const GraphKey &o) const {
      return count == o.count && prec == o.prec && fuse == o.fuse && nf == o.nf && pat == o.pat &&
             f32 == o.f32 && flow == o.flow && mf == o.mf && zout == o.zout && dmask == o.dmask &&
             epoch == o.epoch;
    }
  };
  // kernel arguments captured in a graph stay valid while the buffers and the layout do: anything
  // that changes an operator, an option or a buffer bumps the epoch
  long long graph_epoch = 0;
  bool graphs_failed = false;  // a capture / instantiation failed: eager launches from then on
  struct GraphSlot {
    GraphKey key;
    hipGraphExec_t exec = nullptr;
  };
  std::vector<GraphSlot> graph_cache;
  // the natural-order SSOR's level launches (ssor_natural.hip: ~2 x 131 levels per field sweep
  // at pore_pnp k=3) replayed as one graph: their arguments are context buffers only
  hipGraphExec_t nat_exec = nullptr;
  bool nat_graph_failed = false;
  void nat_graph_clear() {
    if (nat_exec) hipGraphExecDestroy(nat_exec);
    nat_exec = nullptr;
    nat_graph_failed = false;
  }
  void graphs_clear();
  // replay the launches `issue` makes on the stream as a graph (captured on first use of `key`)
  // *captured = false when the failure happened before any launch ran (capture / instantiate):
  // the caller can then run the same iterations eagerly
  template <typename F>
  int graph_run(const GraphKey &key, F &&issue, bool *captured = nullptr) {
    if (captured) *captured = true;
    for (auto &g : graph_cache)
      if (g.key == key) {
        hipError_t e = hipGraphLaunch(g.exec, stream);
        return e == hipSuccess ? PNP_OK : hipfail(e, "graph launch");
      }
    if (captured) *captured = false;
    hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return hipfail(e, "graph capture");
    const int rc = issue();
    hipGraph_t graph = nullptr;
    hipError_t e2 = hipStreamEndCapture(stream, &graph);
    if (rc) {
      if (graph) hipGraphDestroy(graph);
      return rc;
    }
    if (e2 != hipSuccess) return hipfail(e2, "graph capture");
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) return hipfail(e, "graph instantiate");
    if (captured) *captured = true;
    if (graph_cache.size() >= 8) {
      hipGraphExecDestroy(graph_cache.front().exec);
      graph_cache.erase(graph_cache.begin());
    }
    graph_cache.push_back({key, exec});
    e = hipGraphLaunch(exec, stream);
    return e == hipSuccess ? PNP_OK : hipfail(e, "graph launch");
  }

  int fail(int code, const std::string &msg) {
    err = msg;
    return code;
  }
  int hipfail(hipError_t e, const char *what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return PNP_E_HIP;
  }

  hipEvent_t ev_get();
  hipEvent_t tb(int cat) {
    if (!timing) return nullptr;
    hipEvent_t e = ev_get();
    hipEventRecord(e, stream);
    (void)cat;
    return e;
  }
  void te(int cat, hipEvent_t start) {
    if (!timing || !start) return;
    hipEvent_t e = ev_get();
    hipEventRecord(e, stream);
    ev_pending[cat].push_back({start, e});
    t_n[cat]++;
  }
  void timers_flush();

  // ---- helpers ------------------------------------------------------------------------------
  long long nown() const { return (long long)L.n_owned * nf; }

  int halo(double *vec, int nfv) { return halo_on(vec, nfv, stream); }

  int halo_on(double *vec, int nfv, hipStream_t hs);

  // the operator application on the rows of Lr (dl or one of its block subsets): the SpMV on the
  // SELL values, or, with the Jacobian held as a linearisation point, the matrix-free kernel
  hipError_t apply_op(const pnp::DevLayout &Lr, const double *vin, double *yout, int mode,
                      const double *w, double *parts, int *nparts, hipStream_t s,
                      const double *w2 = nullptr, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    if (mf_lin && degree > 1)
      return pnp::launch_pk_jac_apply(Lr, mf_aa, pkd, vin, yout, mode, w, parts, nparts, s, w2, t0,
                                      t1);
    if (mf_lin)
      return pnp::launch_jac_apply(Lr, mf_aa, vin, yout, mode, w, parts, nparts, s, w2, t0, t1);
    return pnp::launch_spmv(Lr, nf, pat, vals.p, vin, yout, mode, w, parts, nparts, s, w2, t0, t1);
  }

  int halo_spmv(double *vin, double *yout, int mode, const double *w, const double *w2, int *nsp);
  int halo_host(double *vec, int nfv);
  int halo_local(double *vec, int nfv);
  int allreduce_dev(double *d, int k);
  int allreduce_red(int k);
  int reduce_derive(int np, int k, int stage, bool from2 = false);
  int reduce_derive2(int npa, int ka, int npb, int kb, int stage);
  int norm(const double *vec, double &out);
  int upload_ext(const double *host, int nfv, double *dev, bool with_ghosts, bool devptr = false);
  int download_ext(const double *dev, int nfv, double *host, bool devptr = false);
  int assemble(const double *xdev, int jac);
  int mf_record(const double *xdev);
  int ensure_values();
  int jacobi_prepare();
  int csr_structure();
  int csr_values();

  // v = SSOR_natural^{-1} d on internal-layout owned rows (ssor_natural.hip); csr_values() first
  // (internal layout, owned rows; d == vout allowed: the result is gathered into vout after both
  // sweeps)
  hipError_t ssor_natural(const double *d, double *vout) { return nat_sweep(d, vout); }
  bool use_nat_flow() const;
  int nat_flow_opt = -1;  // PNP_OPT_NAT_FLOW: -1 auto (use_nat_flow), 0 level launches, 1 dataflow
  // the dataflow's progress needs its whole grid resident: checked once per schedule on the device
  // (pnp::ssor_natural_flow_resident) before the first dataflow application; 0 keeps the level
  // launches (the same results bit for bit).  -1 not yet checked
  int nat_resident = -1;
  DBuf<unsigned> nat_probe;
  int nat_probe_run();
  long long nat_flow_n = 0, nat_level_n = 0;  // applications per schedule (pnp_info)
  hipError_t nat_sweep(const double *d, double *vout);
  pnp::NatFlow nat_flow_view() const;
  hipError_t ssor_natural_flow(const double *d, double *vout);
  int nat_check();
  int ilu_flow_build(int c_first, IluFlowDev &D);
  int ilu_apply(const double *d, double *vout, int c_first, const char *what,
                hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
  int ilu_flow_check();
  // the level launches: one graph replay (captured on first use; PNP_NAT_GRAPH=0: eager), or eager
  // when the stream is itself being captured (a BiCGSTAB block graph then holds them), with more
  // than one rank, or after a failed capture
  // (on the context's external-layout nat_d / nat_v, so that the captured level graph's arguments
  // stay valid whatever vectors the caller passes)
  hipError_t ssor_natural_levels(const double *d, double *vout) {
    const int nv = mesh.nv;
    hipError_t e = pnp::launch_scatter_ext(L.n_owned, nf, nv, d_l2g.p, d, nat_d.p, stream);
    if (e == hipSuccess) e = ssor_natural_levels_fixed();
    if (e == hipSuccess) e = pnp::launch_gather_ext(L.n_owned, nf, nv, d_l2g.p, nat_v.p, vout, stream);
    return e;
  }
  hipError_t ssor_natural_levels_fixed();
  int set_fd(bool on);
  // the steps of pnp_create_pk, in order (ctx.cc)
  int create(const pnp_mesh *mesh_in, const pnp_params *pp, int degree_in, int device_in,
             const pnp_comm *comm_in);
  int create_host(const pnp_mesh *mesh_in, const pnp_params *pp, int degree_in,
                  const pnp_comm *comm_in);
  int create_device(int device_in, const pnp_comm *comm_in);
  int upload_layout(const pnp::DerivedLayout &D, const pnp::LayoutKnobs &K);
  int alloc_vectors();
  int create_halo_stream(const pnp_comm *comm_in);
  int create_host_transport(const pnp_comm *comm_in);
  int join_local_group(const pnp_comm *comm_in);
  int pk_build();
  int fd_build();
  int ilu_factor();
  int split(int which);

  // a host vector to a device buffer of (at least min_count) as many records.  upload leaves an
  // empty vector's buffer null; upv gives it one zeroed element, for readers that take the pointer
  template <typename T, typename U>
  int upload(DBuf<T> &d, const std::vector<U> &h, const char *what, size_t min_count = 0) {
    static_assert(sizeof(T) == sizeof(U), "upload: record size");
    hipError_t e = d.alloc(std::max(min_count, h.size()));
    if (e == hipSuccess && !h.empty())
      e = hipMemcpy(d.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice);
    return e == hipSuccess ? PNP_OK : hipfail(e, what);
  }
  template <typename T>
  int upv(DBuf<T> &d, const std::vector<T> &h, const char *what) {
    return upload(d, h, what, 1);
  }

  // ---- aggregation AMG ------------------------------------------------------------------------
  int amg_setup();

  // block-Jacobi sweeps on coarse level k + 1 (amg_d[k]): the configured count; PNP_AMG_DEEP_SWEEPS
  // (A/B, environment) overrides it below level 1, where the kernels sit at the launch floor
  int amg_sweeps(int k) const {
    static const int deep = [] {
      const char *e = std::getenv("PNP_AMG_DEEP_SWEEPS");
      return e ? std::atoi(e) : 0;
    }();
    return (k >= 1 && deep >= 1) ? deep : amg_opts.coarse_sweeps;
  }

  int amg_apply(const double *d, double *vout);
  // ---- the linear solvers (krylov.cc) and what they share --------------------------------------
  int prec_prepare(int prec);
  int solve_start(const double *bdev, double *zout);
  int state_upload(void *dev, const void *init, size_t bytes, const char *what);
  int poll(void *host, const void *dev, size_t bytes, const char *what);
  int allred_timed(double *d, int k);
  int solve_checks(int prec);
  void solve_result(pnp_solve_result &res, int done, int breakdown, int it, double it_half,
                    double norm0, double norm, double t_start);
  int history_download(const double *dev, int count);
  int smoother(int prec, const double *d, double *vout, bool in_amg = false);
  int precond(int prec, const double *d, double *vout);
  int bicgstab(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res,
               int fixed);
  int cg(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res);
  int gmres_alloc(bool flexible);
  void gmres_free();
  int gmres(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res,
            bool flexible);
  long long idr_ld(bool ghosts) const;
  void idr_free();
  int idr_shadow_build();
  int idr_alloc();
  int idr(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res);

  // ---- the operator-split time loop (pnp_md_run, md.cc) -------------------------
  // what pnp_set_operator computes from the mesh and the parameters alone (ctx.cc)
  void op_static(int kind, int field, double dt, std::vector<uint8_t> &mask,
                 std::vector<uint8_t> &lmask, std::vector<double> &lload) const;
  int ion_flux_dev(const double *xd, int nsurf, double *ip, double *im);
  // one operator of the loop: its static part, computed once per run and kept on the device
  struct MdOp {
    int kind = -1, field = 0;
    double z = 0;
    std::vector<uint8_t> gmask;         // every node, global order
    std::vector<uint8_t> hmask, hflag;  // owned rows; whole SELL chunks (as rowflag)
    DBuf<uint8_t> mask, flag;
    DBuf<double> load;                  // owned rows
  };
  struct MdRun;  // the run's resident state (md.cc)
  int md_op_build(MdOp &op, int kind, int field, double z);
  int md_activate(const MdOp &op, double dt, const double *a0, const double *a1);
  int md_cvec(const MdOp &op, double s, const double *r1, const double *xold);
  int md_residual_of(const MdOp &op, const double *xdev);
  int md_linear_problem(MdRun &R, double *xvec, bool jac, double reduction, bool diffusion);
  int md_alexander2(MdRun &R, double *cvecx, const MdOp &ie, const MdOp &sp);
  int md_poisson(MdRun &R);
  int md_run(double *u, const pnp_md_opts &o, int nsurf, int cap, double *t_out, double *ip,
             double *im, pnp_md_result &res, bool devptr);

  // ---- reference-order mode (PNP_OPT_SEQ_ORDER) ------------------------------------------------
  // The reference's single-rank arithmetic in its order (seq_order.hip): element-order assembly
  // into the CSR view, ISTL's sequential mv / dot / updates, the scalar recurrences here in double.
  // External-layout vectors throughout.  P1, one rank.
  bool seq_on() const { return seq_opt && degree == 1 && !dist; }
  int nseq() const { return nf * mesh.nv; }
  enum { SQ_X = 0, SQ_R, SQ_Z, SQ_PREVU, SQ_P, SQ_V, SQ_T, SQ_Y, SQ_RT, SQ_B, SQ_N };
  double *sq(int k) { return seq_vec.p + size_t(k) * size_t(3 * mesh.nv); }

  int seq_build();
  int seq_prepare();
  pnp::SeqMesh seq_mesh() const;
  pnp::SeqOp seq_op() const;
  int seq_residual(const double *x, double *r);
  int seq_jacobian(const double *x, bool fd);
  double seq_dot(const double *a, const double *b, int &rc);
  int seq_prec(int prec, const double *d, double *v);
  int seq_bicgstab(int prec, double reduction, int maxit, double *x, double *b,
                   pnp_solve_result &res);
  int seq_cg(int prec, double reduction, int maxit, double *x, double *b, pnp_solve_result &res);
  int seq_krylov(const pnp_solve_opts &o, double *x, double *b, pnp_solve_result &res);
  int krylov(const double *bdev, double *zout, const pnp_solve_opts &o, pnp_solve_result &res);
};
