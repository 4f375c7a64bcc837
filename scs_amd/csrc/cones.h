// cones.h -- device-resident projection onto K = zero x pos x box x SOC^q x PSD^s
// (reference src/cones.c:1340-1394 `proj_cone`, wrapped by the Moreau identity of
// src/cones.c:1552-1596 `proj_dual_cone`).
#pragma once
#include "common.h"

namespace scsamd {

typedef scs_float real;

struct BigPsd; // psd_big.h

// block projections (cones_multi.h): state and staging at one width, per column position; nothing of it is shared with the
// single-vector path
struct ConeMulti {
  ~ConeMulti();
  int width = 0;
  DevBuf<real> s;              // m x W: the saved input of the Moreau wrapper
  DevBuf<real> cols;           // W columns of length m, column major: what the single-vector device code of the box and PSD cones works on
  DevBuf<real> xblk;           // m x W: the block of the host-pointer entry (allocated by it)
  DevBuf<real> tile_part;      // per (tile, column)
  DevBuf<real> big_coef;       // per (big cone, column): [head, tail multiplier]
  DevBuf<real> box_t;          // W Newton warm starts
  DevBuf<real> ry_cols;        // W columns of length m, column major: the box rows of a per-column r_y (set_multi_ry allocates it)
  DevBuf<int> psd_off, psd_k;  // tables of the LDS kernel, replicated per column
  DevBuf<real> psd_vprev, psd_tscratch; // per (column, block)
  std::vector<BigPsd *> big;   // per column: blocks beyond the LDS path
  long long psd_calls = 0;     // block projections since the last cold start
};

struct ConeDev {
  ~ConeDev();
  ConeDev() = default;
  ConeDev(const ConeDev &) = delete;
  ConeDev &operator=(const ConeDev &) = delete;
  int m = 0;
  hipStream_t stream = nullptr;
  // layout (row offsets into the length-m cone vector)
  int z = 0, l = 0, bsize = 0, box_off = 0;
  // box cone
  DevBuf<real> bl, bu;      // bsize-1 each (already D-normalised, +-inf applied)
  DevBuf<real> box_t;       // [0] Newton warm start (reference c->box_t_warm_start)
  int psd_pipe = 1;         // step of k_psd_jacobi for orders <= 72 (option psd_pipe, read in init): 0 two-phase, 1 look-ahead, 2 signal form
  bool box_multi = false;   // large box: Newton steps as chip-wide launches (k_box_step), else one workgroup (k_box)
  DevBuf<real> box_part, box_ctl;
  // second-order cones
  int n_tiny = 0;           // cones with q <= SOC_TINY_MAX: one lane per cone
  DevBuf<int> tiny_off, tiny_len;
  int n_big = 0, n_tiles = 0; // remaining cones: tiled three-pass reduction
  DevBuf<int> big_off, big_len, big_tile0; // per big cone (+1 sentinel in big_tile0)
  DevBuf<int> tile_cone, tile_off, tile_len;
  DevBuf<real> tile_part;   // per-tile sum of squares of the tail
  DevBuf<real> big_coef;    // per big cone: [head, tail multiplier]
  // PSD cones
  int n_psd = 0, psd_kmax = 0, psd_lds_kmax = 0, psd_row0 = 0; // psd_row0: first row of the PSD blocks (they end at exp_off)
  DevBuf<int> psd_off, psd_k;
  BigPsd *psd_big = nullptr; // blocks of order > PSD_LDS_KMAX: chip-wide Jacobi steps
  DevBuf<real> psd_vprev;   // per block: eigenbasis of the previous projection (warm start of the LDS kernel, every order it handles)
  DevBuf<real> psd_tscratch; // per block: T = A Vp of the warm start when three matrices do not fit LDS (orders 73..92)
  long long psd_calls = 0;  // projections since the last cold start
  void reset_warm_start();
  // exponential (primal, dual) and power cones: 3 rows each, after the PSD blocks
  int ep = 0, ed = 0, psize = 0, exp_off = 0;
  DevBuf<real> pow_a;       // psize power-cone parameters (negative = dual cone)
  DevBuf<int> status;       // [0] = PSD block projections that hit the Jacobi sweep cap since the last take_status()
  PinnedBuf<int> hstatus;   // its host copy (pinned: take_status runs at every residual evaluation)
  int take_status(hipStream_t st);

  // host staging for the B1' boundary
  DevBuf<real> x_stage, s_stage, r_stage;

  void init(const ScsCone *k, int m, const real *D_host, hipStream_t s);
  void upload_box_bounds(const ScsCone *k, const real *D_host); // bl / bu (allocated) from the cone's bounds and D
  // the host half of it: hl / hu (bsize - 1 each) from the cone's bounds and the box rows Db of D (bsize values; null: as given)
  static void box_bounds_host(const ScsCone *k, const real *Db, real *hl, real *hu);
  void update_scaling(const ScsCone *k, const real *D_host);    // a new D on the same cone: bounds again, every warm start as after init
  // cw (device, length m) <- Proj_K(cw), projection under the diag(r_y)^-1 metric
  // (only the box cone looks at r_y; nullptr = Euclidean).
  void proj_primal(real *cw, const real *r_y);
  void proj_exp_pow(real *cw);
  // x (device, length m) <- Proj_{K*}^{R}(x) via Moreau; `scratch` is a length-m
  // device buffer that receives the saved input.
  void proj_dual(real *x, real *scratch, const real *r_y);
  // the same for a block of K vectors in the m x W block layout (cones_multi.h), in place; columns K .. W - 1 become zero
  ConeMulti *multi = nullptr;
  void ensure_multi(int W);
  void proj_dual_multi(real *X, int W, int K, const real *r_y);
  // the same without the Moreau wrapper: Proj_K per column.  own_ry: every column under its own r_y (only the box cone reads it),
  // column k's slice of the copy that set_multi_ry keeps; r_y is then not read
  // bl_cols / bu_cols (both or neither): every column under its own normalised box bounds (its own D), column k's bsize - 1 values at
  // k * (bsize - 1); null: the cone's own bl / bu in every column
  void proj_primal_multi(real *X, int W, int K, const real *r_y, bool own_ry = false, const real *bl_cols = nullptr,
                         const real *bu_cols = nullptr);
  // keeps a column-major copy of the box rows of the m x W block Ry; to be called again when Ry changes
  void set_multi_ry(const real *Ry, int W);
  void reset_multi_cold();                                       // box Newton starts and eigenbases of the block state: cold
  void reset_multi_box_start(int k);                             // the per-column half of it: column position k's box Newton start
  // launches shared by the two paths
  void launch_box(real *tx, real *t_warm, const real *rb, const real *lo = nullptr, const real *hi = nullptr); // lo / hi null: bl / bu
  void launch_psd_lds(real *cw, int nblocks, const int *off, const int *kk, real *tscratch, real *vprev, int warm);
  int rows() const { return m; }
};

// validation shared by scs_init and scs_amd_cone_init; returns <0 when the cone
// description is inconsistent with m or uses a cone this backend does not carry.
int validate_cone(const ScsCone *k, int m, bool verbose);
long long cone_total_rows(const ScsCone *k);

} // namespace scsamd
