// linsys.h -- device-resident Jacobi-PCG on the reduced KKT system
//     (R_x + P + A' R_y^{-1} A) x = r_x + A' R_y^{-1} r_y ,  y = R_y^{-1}(A x - r_y)
// i.e. the algorithm of reference linsys/cpu/indirect/private.c:133-324, with
// every vector in HBM and the loop controlled from the device.
#pragma once
#include "spmv.h"
#include "scs_host.h"
#include "spmv_wave.h"
#include "spmm.h"

namespace scsamd {

int selected_device(); // device chosen by scs_amd_set_device (HIP's current device is per host thread)

// Control block of one PCG solve, lives in device memory; the host reads it back
// once per enqueued batch of iterations (cg_pace=0) or not at all (cg_pace=1: the progress word below).
struct CgCtl {
  real ztr[2];   // z'r, double-buffered by iteration parity
  real norm_r;   // ||r||_inf after the last completed iteration
  real tol;      // tolerance of this solve
  real rhs_norm; // ||b||_inf over n+m on entry
  int zero_rhs;  // ||b||_inf <= 1e-12: solution is 0, everything else is skipped
  int cg_done;   // converged (or breakdown): remaining iteration kernels return
  int iters;     // PCG iterations performed (reference counting, private.c:203,216)
  int max_its;   // 10 n (private.c:307): the device stops there even if more iterations were enqueued
  unsigned seq;  // sequence number of this solve (k_rhs_prep): tags every progress word the solve publishes
};

// Progress word of a paced solve: ONE aligned 64-bit word in pinned, host-coherent, device-mapped memory that the lane which
// writes CgCtl::iters / cg_done also stores, so the host learns "stopped, after how many iterations" from one load without
// stopping the stream.  bits 63..32: sequence number of the solve (a word left by the previous solve never matches);
// bits 31..1: iterations done (max_its < 2^31); bit 0: done.
typedef unsigned long long cg_word;
__host__ __device__ inline cg_word cg_word_pack(unsigned seq, int iters, int done) {
  return ((cg_word)seq << 32) | ((cg_word)(unsigned)iters << 1) | (cg_word)(done ? 1 : 0);
}

// Control block of a block solve (linsys_multi.h): what CgCtl holds, per column, plus one word that says every column has stopped.
struct CgCtlM {
  real ztr[2][MULTI_W_MAX];
  real norm_r[MULTI_W_MAX], tol[MULTI_W_MAX], rhs_norm[MULTI_W_MAX];
  int zero_rhs[MULTI_W_MAX]; // also set for the padding columns
  int done[MULTI_W_MAX];     // this column has stopped: frozen from here on
  int iters[MULTI_W_MAX];
  int max_its;
  int all_done; // every column has stopped: iteration kernels enqueued past this point return at once
};

// Buffers of the block solves, in the block layout of spmm.h at the largest width W used so far: 7 n W + 2 m W values
// (6 n W + 2 m W without P).  Allocated at the first block call, reused, freed with the workspace.
struct MultiWork {
  int width = 0;    // width the buffers were allocated for (0: not allocated)
  int last_its = 16;
  DevBuf<real> bx, by;      // right-hand side / solution: n W, m W
  DevBuf<real> s, r, z, p;  // n W each
  DevBuf<real> gt;          // (n + m) W: Gp (n W) and tmp (m W) during a solve; the column-major staging of the host block around it
  DevBuf<real> Pp;          // n W, only with P
  DevBuf<real> part_pgp, part_ztr, part_max; // per-workgroup, per-column reduction partials
  DevBuf<CgCtlM> ctl;
  PinnedBuf<CgCtlM> hctl;
  // per-column R (scs_amd_solve_lin_sys_multi_r): R_x, R_y and the Jacobi preconditioner of every column, 2 n W + m W values more.
  // Allocated at the first per-column call only (ensure_multi_r): a caller who never makes one allocates what is listed above.
  int rwidth = 0;           // width these three were allocated for (0: not allocated)
  DevBuf<real> rxb, ryb, Mb; // n W, m W, n W
  // per-column values (scs_amd_linsys_set_values_multi): the values of every column's A and P on the workspace's pattern, blocks of
  // nnz x W' in the block layout at the layout width W' of the last set call's `vcols` columns (W' <= vwidth); padding columns 0.
  // Allocated by the first set call only, rebuilt when a set call needs a wider block (ensure_multi_values).
  int vwidth = 0;           // width the value blocks were allocated for (0: not allocated)
  int vcols = 0;            // columns of the set call in force (0: none)
  DevBuf<real> vA, vAt;     // nnz(A) vwidth each: CSR(A) order, CSC order
  DevBuf<real> vP, vPdiag;  // nnz(full P) vwidth, n vwidth; only with P
  DevBuf<real> vstage;      // one column of the caller's values on its way into the blocks: max(nnz(A), nnz(upper P))
};

// ONE linear system split by rows of A over several devices (the operator split is
// linsys/cpu/indirect/private.c:106-119).  A workspace created on the row slab A_r with diag_r = [R_x / N ; R_y of the slab]
// applies ITS term of G = R_x + A' R_y^-1 A = sum_r (R_x / N + A_r' R_r^-1 A_r); `allreduce` sums (or takes the maximum of)
// an n-vector over the N ranks IN PLACE, enqueued on the workspace's stream -- the PCG loop stays device controlled, the host
// reads one control block per batch of iterations as in the unsplit solve.  Everything of length n is replicated on every rank
// and computed redundantly (identical bits after the all-reduce), so alpha / beta / the stop test need no second collective.
struct ShardHook {
  void *ctx = nullptr;
  int world = 1, rank = 0;
  int (*allreduce)(void *ctx, real *buf, size_t count, int op /* 0 sum, 1 max */, hipStream_t st) = nullptr; // 0 = ok
};

// The operator of a block solve or block product: what differs from column to column, as blocks in device memory in the layout of
// spmm.h.  All null = the workspace's shared rx / ry / M and values.  A new per-column quantity is a field here, a line of check()
// and an argument of the constructors below.
struct MultiOp {
  // every column under its own diag_r: R_x (n x W), R_y (m x W) and the preconditioner built from them by precond_multi_blocks
  // (n x W); padding columns hold ordinary finite values (1).  A block product reads rx / ry only.
  const real *rx = nullptr, *ry = nullptr, *Minv = nullptr;
  // every column its own values of A (CSR order), A' (CSC order) and the symmetric P, value blocks of nnz x W (MultiWork::vA ...);
  // vP and vPdiag with P only; Minv is then built by precond_multi_blocks from vAt and vPdiag
  const real *vA = nullptr, *vAt = nullptr, *vP = nullptr, *vPdiag = nullptr;

  bool percol() const { return rx != nullptr; } // the per-column instantiations: the workspace's rx, ry, M are not read
  bool vcol() const { return vA != nullptr; }   // the per-value instantiations: the workspace's A.val, At.val, P.val are not read
  // the rule of a solve, stated once: R is all three or none; values are all or none, vP / vPdiag exactly with P; values need R
  void check(bool has_P) const {
    if (percol() != (ry != nullptr) || percol() != (Minv != nullptr)) throw HipError("scs_amd: per-column R needs rx, ry and Minv together");
    if (vcol() != (vAt != nullptr) || (vcol() && has_P) != (vP != nullptr) || (vcol() && has_P) != (vPdiag != nullptr))
      throw HipError("scs_amd: per-column values need vA, vAt and, with P, vP");
    if (vcol() && !percol()) throw HipError("scs_amd: per-column values run under per-column R");
  }
  static MultiOp shared() { return MultiOp(); }
  static MultiOp r_blocks(const real *rx, const real *ry, const real *Minv) {
    MultiOp o;
    o.rx = rx, o.ry = ry, o.Minv = Minv;
    return o;
  }
  // the x and y rows of one l x W block [R_x rows | R_y rows | ...], as a family holds its R (nw = n W)
  static MultiOp r_rows(const real *R, size_t nw, const real *Minv) { return r_blocks(R, R + nw, Minv); }
  // the workspace's own R blocks and, with `values`, the value blocks of its last set call
  static MultiOp of_work(const MultiWork &mw, bool values, bool has_P) {
    MultiOp o = r_blocks(mw.rxb.p, mw.ryb.p, mw.Mb.p);
    if (values) o.vA = mw.vA.p, o.vAt = mw.vAt.p, o.vP = has_P ? mw.vP.p : nullptr, o.vPdiag = has_P ? mw.vPdiag.p : nullptr;
    return o;
  }
  // this op's values under the x and y rows of another R block (a block product under a caller's R): no preconditioner goes
  // with that R, so Minv is null and the result serves products only -- check() refuses it for a solve
  MultiOp with_r_rows(const real *R, size_t nw) const {
    MultiOp o = *this;
    o.rx = R, o.ry = R + nw, o.Minv = nullptr;
    return o;
  }
};

// What a block solve works on when the caller holds the blocks (LinSys::solve_multi_blocks), all in device memory, in the layout
// of spmm.h.  warm_part != null: the tolerance of column k is formed on the device, as solve_dev forms it, as
//     max(1e-12, 0.2 * min(tolv[k], max(column k of warm_part[0 .. warm_cnt)) * warm_scale))      (reference src/scs.c:745-762)
// from warm_cnt x W per-workgroup partials of |s|_inf; otherwise tolv[k] is used as given.  pre_stopped != null: W ints, a non-zero
// entry marks a column that is stopped on entry -- its lanes load and store nothing, it costs no iteration and counts none.
struct MultiRhs {
  real *bx = nullptr, *by = nullptr; // n x W, m x W: [r_x; r_y] -> [x; y] in place
  const real *s = nullptr;           // n x W warm start, or null
  const real *warm_part = nullptr;
  int warm_cnt = 0;
  real warm_scale = 0;
  // non-null: W host values, column k takes warm_scale_col[k] where the others take warm_scale (columns that stand at different
  // iterations of their own solves: scs_amd_solve_family_stream); passed to the kernel by value, not read after the call returns
  const real *warm_scale_col = nullptr;
  const int *pre_stopped = nullptr;
  MultiOp op; // the system of every column; default: the workspace's shared R and values
  MultiRhs() = default;
  MultiRhs(real *bx_, real *by_, const real *s_, const MultiOp &op_) : bx(bx_), by(by_), s(s_), op(op_) {}
};

struct LinSys {
  int n = 0, m = 0;
  ShardHook *shard = nullptr;   // non-null: this workspace holds one row slab (set_shard)
  long long n_allreduce = 0;
  EventTimer ar_timer;          // sampled all-reduce times (profiling)
  void set_shard(ShardHook *h); // call right after init(), before the first set_diag_r_*
  void shard_allreduce(real *buf, size_t count, int op);
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool has_P = false;
  bool use_fused = false; // whole solve in one workgroup (small systems)
  int nt_mode = 0;        // non-temporal policy of the update kernel's streams (SCS_AMD_VEC_NT; 0 = default policy; bit 2: two chunks per lane in flight)
  int dir_mode = 0;       // k_cg_direction: bit 0 non-temporal z reads, bit 1 non-temporal p stores, bit 2 two chunks per lane (SCS_AMD_DIR_MODE)
  bool use_cg2 = false;   // two launches per CG iteration (n <= CG2_N_MAX): k_cg2_a + transposed product
  bool use_cg3 = false;   // three launches per CG iteration (round 5): the stop test, alpha, beta, x, r, z, p in ONE vector kernel (k_cg3_update)

  CsrDev At; // CSR(A') == CSC(A): n rows, gathers an m-vector
  CsrDev A;  // CSR(A): m rows, gathers an n-vector
  CsrDev P;  // full symmetric CSR of P (n x n), optional
  DevBuf<real> Pdiag; // sum of stored diagonal entries of P per column

  DevBuf<real> rx, ry;               // R_x (n), R_y (m)
  DevBuf<real> M, p, r, Gp, z, Pp;   // n each
  DevBuf<real> p2, r2;               // second direction / residual buffers of the two-launch path (p_j, r_j in {p, p2}[j & 1])
  DevBuf<real> tmp;                  // m
  DevBuf<real> partA, partB;         // reduction partials
  DevBuf<real> partC, partD;         // use_cg3: partials of z'Gp and Gp'MGp
  DevBuf<CgCtl> ctl;
  PinnedBuf<CgCtl> hctl;
  // paced enqueue (cg_pace): the progress word, the sequence number of the last solve, how many quanta the
  // host may run ahead of the published iteration count, and what scs_amd_get_cg_pacing reports
  PinnedBuf<cg_word> prog;
  cg_word *prog_dev = nullptr; // device view of `prog`; null = nothing is published (cg_pace=0, row-sharded workspaces)
  unsigned cg_seq = 0;
  bool cg_pace = true;
  int cg_lead = 4;
  long long n_enq_its = 0, n_syncs = 0; // CG iterations enqueued (a graph counts CG_GRAPH_ITERS); blocking waits inside solve_dev
  cg_word progress_word() const;
  bool wait_word(cg_word seen, double iter_us);
  // options read once in init (options.h: "read when a workspace is created")
  bool opt_debug = false;
  const char *opt_trace_file = nullptr; // interned by options.h: stays valid
  int vec_cap = 0;                      // cap on the grid of the vector kernels (vec_max_grid)
  int vec_grid(long long len) const;

  // staging for the host-pointer boundary (B1)
  DevBuf<real> b_stage, s_stage, dr_stage;

  // HIP graph of CG_GRAPH_ITERS iterations (4 kernels each, constant arguments: everything that
  // changes lives in the control block) for systems whose kernels are shorter than a launch
  hipGraphExec_t cg_graph = nullptr;
  real *cg_x = nullptr; // solution vector of the current / captured solve
  bool cg_graph_tried = false, use_graph = false;
  void enqueue_cg_iteration(int q);
  void enqueue_cg2_iteration(long long it);
  void enqueue_cg3_iteration(long long it);
  bool build_cg_graph();
  // statistics / profiling
  long long tot_cg_its = 0, n_solves = 0, n_matvecs = 0, n_spmv = 0, n_graph_launches = 0;
  int last_its = 16;
  bool profiling = false;
  EventTimer spmv_timer, cg_timer;
  long long spmv_sample_ctr = 0;

  LinSys() = default;
  ~LinSys();
  LinSys(const LinSys &) = delete;

  // A, P: host CSC as handed over by the reference (normalized data).
  // `pat` (optional): an already-built pattern transpose of A_csc
  // with pat->dev.valid the matrices are adopted from HBM (device equilibration) instead of uploaded (round 5)
  void init(const CscView *A_csc, const CscView *P_csc, hipStream_t s, CsrPattern *pat = nullptr);
  // diag_r = [R_x (n); R_y (m)] : host or device source
  void set_diag_r_host(const real *diag_r);
  void set_diag_r_dev(const real *diag_r_dev);
  // Solve in place on device memory: b = [r_x; r_y] -> [x; y].  s: warm start
  // (device, length n) or nullptr.  If warm_part != nullptr the tolerance is
  // formed on the device as
  //     tol = max(1e-12, 0.2 * min(tol, max(warm_part[0..warm_cnt)) * warm_scale))
  // (reference src/scs.c:745-762), otherwise `tol` is used as given.
  // Returns the PCG iteration count (>= 0).
  int solve_dev(real *b, const real *s, real tol, const real *warm_part = nullptr,
                int warm_cnt = 0, real warm_scale = 0);
  // y_out(n) = (R_x + P + A' R_y^-1 A) x  -- exposed for tests / roofline runs
  void mat_vec_dev(const real *x, real *y_out, real *dot_partials);
  // plain products for the residual computation (reference src/scs.c:559,581)
  void mul_A(const real *x_n, real *y_m);  // y = A x
  void mul_At(const real *y_m, real *x_n); // x = A' y
  void mul_P(const real *x_n, real *y_n);  // y = P x (full symmetric)
  // ---- blocks of right-hand sides (linsys_multi.h) ----
  MultiWork *multi = nullptr; // owned
  void ensure_multi(int W);
  void ensure_multi_r(int W); // ensure_multi plus the three R blocks of MultiWork
  // dcol: e.d is a block (rows x W), one divisor / multiplier per column (EPI_DIV, EPI_GP, EPI_NEGDIV)
  // vals: the matrix's values per column, an nnz x W block in mat's entry order (null: mat's own, shared by the columns)
  void launch_spmm(int W, int epi, const CsrDev &mat, const real *X, real *Y, const EpiArgs &e, const int *cskip, const int *allskip,
                   bool dcol = false, const real *vals = nullptr);
  // Y = G X under op (its rx / ry and vA / vAt / vP; Minv is not read), skipping the columns of cskip / everything under allskip
  void mat_vec_multi_dev(int W, const MultiOp &op, const real *X, real *Y, real *dot_partials, const int *cskip, const int *allskip);
  void precond_multi_blocks(int W, const MultiOp &op, real *Minv); // Minv from op's rx / ry and, with values, its vAt / vPdiag
  // value blocks of the per-value solves (MultiWork::vA ...; scs_amd_linsys_set_values_multi)
  void ensure_multi_values(int W);
  void set_multi_values(int K, int W, const real *AX, size_t ldax, const real *PX, size_t ldpx);
  void free_multi_values();
  void solve_multi_blocks(int K, int W, const MultiRhs &a, const real *tolv, int *iters_out);
  // ---- new values on the pattern given to init (scs_amd_linsys_update_values, include/scs_amd.h) ----
  // Position maps, device resident, built by the first update that needs them and freed with the workspace:
  //   upd_rpos  nnz(A) x sizeof(eoff)            CSC position of every CSR(A) entry (the pattern transpose, formed on the device)
  //   upd_fsrc  nnz(full P) x sizeof(eoff)       position in the upper triangle of every entry of the symmetric P
  //   upd_pux   nnz(upper P) x sizeof(real)      where the caller's Px lands before the gather
  // The wave layouts keep no map: the builder that made them runs again on the refreshed CSR copy (wave_refresh_values).
  DevBuf<eoff> upd_rpos, upd_fsrc;
  DevBuf<real> upd_pux;
  long long nnzP_up = 0; // entries of the upper triangle handed to init
  void ensure_update_maps(bool need_A, bool need_P);
  // Ax / Px: HOST arrays in the CSC order of init's A / P (either may be null); every value copy, the layouts and the preconditioner
  // follow; returns with the stream idle
  void update_values(const real *Ax, const real *Px);
  long long matvec_bytes() const { return A.algorithmic_bytes() + At.algorithmic_bytes(); }
  void harvest_timers();
  void get_cg_pacing(long long out[4]) const; // scs_amd_get_cg_pacing (include/scs_amd.h)

private:
  void build_preconditioner();
  void launch_spmv(int epi, const CsrDev &mat, const real *x, real *y, const EpiArgs &e,
                   const int *skip);
};

} // namespace scsamd
