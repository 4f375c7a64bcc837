// linsys_multi.h -- K independent Jacobi-PCG solves of the reduced KKT system in lock step on one workspace (part of
// linsys.hip: included there, behind the single-vector solve whose helpers it uses).
//
// Column k computes what LinSys::solve_dev computes for that column alone: the recurrence of reference
// linsys/cpu/indirect/private.c:133-217 and the wrapper :284-324, with its OWN alpha, beta, z'r, |r|_inf, tolerance, stop
// tests, breakdown exit, iteration cap and zero short-circuit.  Nothing couples the columns (this is not block CG): every
// reduction runs over the lanes and workgroup partials of one column only, in an order that does not depend on the column's
// position, so the bits of a column do not depend on its neighbours.  A column that has stopped is frozen: its lanes return
// before they load anything, its x is not touched again and it counts no more iterations.  When every column has stopped the
// all_done word is set, and iteration kernels that were enqueued past that point return at their first instruction.
//
// One plain form of the iteration (the four kernels of linsys.hip's header comment, on blocks):
//   csr_block<DIV>  tmp = R_y^-1 (A p)            csr_block<GP>  Gp = R_x p + P p + A' tmp, partials of p'Gp per column
//   k_m_cg_update   alpha; x, r, z; partials      k_m_cg_direction  stop tests; beta; p; control block
// Buffers (MultiWork, linsys.h): 7 n W + 2 m W values at the largest width used (6 n W + 2 m W without P), allocated at the
// first block call, reused, freed with the workspace.
//
// What differs from column to column is one value, MultiOp (linsys.h), which MultiRhs carries and mat_vec_multi_dev,
// precond_multi_blocks and solve_multi_blocks take; MultiOp::check states once which of its fields go together.
//
// Per-column R (MultiOp::rx / ry / Minv): column k runs under its own diag_r_k = [R_x,k; R_y,k] and its own Jacobi preconditioner
// (k_m_precond), i.e. it computes what scs_update_lin_sys_diag_r(diag_r_k) followed by the single solve computes.  R_x, R_y and
// M^-1 are then blocks in the block layout and the kernels that read them run in their per-column instantiation (the DCOL form of
// csr_block_kernel, PERCOL of k_m_rhs_prep / k_m_cg_init / k_m_cg_update); A and P are still read once per product for all
// columns.  The workspace's own rx, ry, M, captured graph and single-vector state are neither read nor written.  Three more blocks
// (2 n W + m W values), allocated at the first per-column call only.
//
// Per-column values (MultiOp::vA / vAt / vP / vPdiag): K systems on one pattern, column k with its own values of A and P, i.e. it
// computes what scs_amd_linsys_update_values(values k) followed by the per-column-R solve computes.  The values are blocks of
// nnz x W in the block layout (the VCOL form of csr_block_kernel and k_m_precond, spmm.h); the row pointers and indices are the
// workspace's and are read once per product for all columns.  Always under per-column R: a caller without an R of their own gets
// the workspace's replicated into the R blocks.  The workspace's A.val, At.val, P.val, Pdiag, rx, ry, M, layouts, captured graph
// and single-vector state are neither read for the columns nor written.  Allocated by the first set call only.
//
// Host side: the instantiation of each kernel is chosen in one place -- spmm_built and launch_spmm_epi for csr_block_kernel,
// launch_rhs_prep / launch_cg_init / launch_cg_update for the vector kernels with a per-column form -- and solve_multi_blocks
// reads as the algorithm.  The width switch is MULTI_DISPATCH (common.h).
#pragma once

namespace scsamd {

struct TolArgs {
  real t[MULTI_W_MAX];
};

// column-major (len x K, leading dimension len) <-> block layout; padding columns become `fill` (0 for vectors; 1 for the R
// blocks of a per-column solve, so that a padding column is an ordinary finite column)
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_to_block(const real *__restrict__ src, real *dx, int n, real *dy, int m, int K, real fill) {
  const int len = n + m;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) {
    real *d = i < n ? dx + (size_t)i * W : dy + (size_t)(i - n) * W;
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = k < K ? src[(size_t)k * len + i] : fill;
  }
}
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_from_block(real *dst, const real *__restrict__ sx, int n, const real *__restrict__ sy, int m, int K) {
  const int len = n + m;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) {
    const real *s = i < n ? sx + (size_t)i * W : sy + (size_t)(i - n) * W;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < K) dst[(size_t)k * len + i] = s[k];
  }
}

// private.c:50-82 per column: the Jacobi preconditioner of column k under its own R_x,k / R_y,k, on blocks (rx, M: n x W; ry:
// m x W).  Rows of CSR(A') with the lane mapping of the block product: W consecutive lanes serve one row, lane k column k; the
// lanes of a row read the same val / idx (one broadcast read serves the W columns) and gather W contiguous values of ry.  Every
// lane evaluates k_precond's expression in k_precond's order -- start from rx, the entries in index order, pdiag last, one
// reciprocal -- so column k holds the bits k_precond gives for diag_r_k.  Rows are summed sequentially per lane, long ones too:
// the kernel runs once per solve, not once per iteration.
// VCOL: every column its own values (ValBlk, spmm.h) -- a lane reads its own value of A', the W lanes of a row W contiguous ones,
// and pdiag is an n x W block; the expression and its order are the same.
template <int W, bool VCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_precond(CsrView At, const real *__restrict__ rx, const real *__restrict__ ry,
                                                            const real *__restrict__ pdiag, real *M, ValBlk<VCOL> vb) {
  const size_t total = (size_t)At.rows * W;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < total; f += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(f / W), col = (int)(f & (W - 1));
    real acc = rx[f];
    for (eoff k = At.ptr[i]; k < At.ptr[i + 1]; ++k) {
      const real a = blk_val<W>(vb, At.val, k, col);
      acc += a * a / ry[(size_t)At.idx[k] * W + col];
    }
    if (pdiag) acc += pdiag[VCOL ? f : (size_t)i];
    M[f] = (real)1 / acc;
  }
}

// One column of new values into a value block through a position map: dst[k * W + col] = src[map[k]] (map null: src[k]).  The
// maps are those of LinSys::ensure_update_maps -- upd_rpos for CSR(A), upd_fsrc for the symmetric P; CSC(A) is CSR(A') and takes
// the caller's order as it is.  One launch per column: the source is the one column that is staged at a time.
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_upd_gather_block(const real *__restrict__ src, const eoff *__restrict__ map,
                                                                     real *__restrict__ dst, long long len, int col) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < len; k += (long long)gridDim.x * blockDim.x)
    dst[(size_t)k * W + col] = src[map ? map[k] : (eoff)k];
}

// k_upd_pdiag on a value block of the symmetric P: pd[j * W + col] = the stored diagonal entries of row j in their stored order,
// column by column (the lane mapping of k_m_precond)
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_upd_pdiag(CsrView P, ValBlk<true> vb, real *__restrict__ pd) {
  const size_t total = (size_t)P.rows * W;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < total; f += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(f / W), col = (int)(f & (W - 1));
    real s = 0;
    for (eoff k = P.ptr[j]; k < P.ptr[j + 1]; ++k)
      if (P.idx[k] == j) s += vb.v[(size_t)(k - vb.bias) * W + col];
    pd[f] = s;
  }
}

// the workspace's R_x / R_y in every column of a block (a caller of the per-value solve who brings no R of their own)
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_replicate(const real *__restrict__ src, real *__restrict__ dst, size_t len) {
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < len * W; f += (size_t)gridDim.x * blockDim.x) dst[f] = src[f / W];
}

// |[r_x; r_y]|_inf per column (private.c:296)
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_absmax(const real *__restrict__ bx, size_t nx, const real *__restrict__ by, size_t ny, real *part) {
  __shared__ real red[4 * W];
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (size_t)gridDim.x * blockDim.x; // gs % W == 0
  real mx = 0;
  for (size_t f = gtid; f < nx; f += gs) {
    const real a = absval(bx[f]);
    mx = a > mx ? a : mx;
  }
  for (size_t f = gtid; f < ny; f += gs) {
    const real a = absval(by[f]);
    mx = a > mx ? a : mx;
  }
  mx = block_col_max<W>(mx, red);
  if (threadIdx.x < W) part[(size_t)blockIdx.x * W + threadIdx.x] = mx;
}

// block 0 of a control kernel: every column stopped?
__device__ __forceinline__ void set_all_done(CgCtlM *ctl, int W, bool col_done) {
  if (threadIdx.x < 64) {
    const unsigned long long live = __ballot((int)threadIdx.x < W && !col_done);
    if (threadIdx.x == 0) ctl->all_done = live == 0 ? 1 : 0;
  }
}

// private.c:296-303 per column: zero short-circuit, tmp = R_y^-1 r_y; arms the control block.  Padding columns count as zero.
// `warm_part` (or null): per-workgroup, per-column |warm start|_inf partials; with it the tolerance of column k is formed here as
// solve_dev forms it (src/scs.c:745-762), tol.t[k] being the cap.  `pre` (W ints, or null): columns that are stopped on entry --
// nothing of theirs is read or written, here or by any later kernel of the solve, and they count no iteration.
// PERCOL: ry is an m x W block (every column its own R_y) instead of one vector of m.
// WS: the type of warm_scale -- `real`, one factor for the block, or TolArgs, column k its own factor warm_scale.t[k]
// (MultiRhs::warm_scale_col), in the same expression: equal factors give the scalar form's bits.
__device__ __forceinline__ real warm_scale_of(real s, int) { return s; }
__device__ __forceinline__ real warm_scale_of(const TolArgs &s, int col) { return s.t[col]; }
template <int W, bool PERCOL = false, typename WS = real>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_rhs_prep(real *bx, real *by, const real *__restrict__ ry, real *tmp, int n, int m,
                                                             const real *part, int pcount, CgCtlM *ctl, TolArgs tol, int K, int max_its,
                                                             const real *warm_part, int warm_cnt, WS warm_scale, const int *pre) {
  __shared__ real red[4 * W];
  const real nb = reduce_partials_col_max<W>(part, pcount, red);
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (size_t)gridDim.x * blockDim.x;
  const int col = threadIdx.x & (W - 1);
  const bool stopped = pre && pre[col];
  const bool zero = stopped || col >= K || nb <= (real)1e-12;
  real t = col < K ? tol.t[col] : (real)0;
  if (warm_part) {
    const real nw = reduce_partials_col_max<W>(warm_part, warm_cnt, red) * warm_scale_of(warm_scale, col);
    t = t < nw ? t : nw;
    t = (real)0.2 * t;                     // CG_TOL_FACTOR, include/glbopts.h:250
    t = t > (real)1e-12 ? t : (real)1e-12; // CG_BEST_TOL, glbopts.h:247
  }
  if (stopped) {
  } else if (zero) {
    for (size_t f = gtid; f < (size_t)n * W; f += gs) bx[f] = 0;
    for (size_t f = gtid; f < (size_t)m * W; f += gs) {
      by[f] = 0;
      tmp[f] = 0;
    }
  } else {
    for (size_t f = gtid; f < (size_t)m * W; f += gs) tmp[f] = by[f] / ry[PERCOL ? f : f / W];
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < W) {
      ctl->zero_rhs[col] = zero ? 1 : 0;
      ctl->done[col] = zero ? 1 : 0;
      ctl->iters[col] = 0;
      ctl->tol[col] = col < K ? t : (real)0;
      ctl->rhs_norm[col] = nb;
      ctl->norm_r[col] = 0;
      ctl->ztr[0][col] = 0;
      ctl->ztr[1][col] = 0;
    }
    if (threadIdx.x == 0) ctl->max_its = max_its;
    set_all_done(ctl, W, zero);
  }
}

// private.c:145-172 per column.  PERCOL: M is an n x W block (every column its own preconditioner) instead of one vector of n.
template <int W, bool PERCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cg_init(real *x, const real *__restrict__ s, real *r, real *z, const real *__restrict__ M, int n,
                                                            real *part_ztr, real *part_max, const CgCtlM *ctl) {
  __shared__ real red[4 * W];
  if (ctl->all_done) return;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (size_t)gridDim.x * blockDim.x;
  const int col = threadIdx.x & (W - 1);
  real ztr = 0, mx = 0;
  if (!ctl->zero_rhs[col]) {
    for (size_t f = gtid; f < (size_t)n * W; f += gs) {
      real ri;
      if (s) {
        ri = x[f] - r[f]; // r held G s; r = b - G s
        x[f] = s[f];
      } else {
        ri = x[f];
        x[f] = 0;
      }
      r[f] = ri;
      const real zi = ri * M[PERCOL ? f : f / W];
      z[f] = zi;
      ztr += zi * ri;
      const real a = absval(ri);
      mx = a > mx ? a : mx;
    }
  }
  ztr = block_col_sum<W>(ztr, red);
  mx = block_col_max<W>(mx, red);
  if (threadIdx.x < W) {
    part_ztr[(size_t)blockIdx.x * W + threadIdx.x] = ztr;
    part_max[(size_t)blockIdx.x * W + threadIdx.x] = mx;
  }
}

// private.c:163 early-out with max(tol, 1e-12) per column; p = z
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cg_start(real *p, const real *__restrict__ z, int n, const real *part_ztr, const real *part_max,
                                                             int pcount, CgCtlM *ctl) {
  __shared__ real red[4 * W];
  if (ctl->all_done) return;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (size_t)gridDim.x * blockDim.x;
  const int col = threadIdx.x & (W - 1);
  const int zero = ctl->zero_rhs[col];
  const real tol = ctl->tol[col];
  const real ztr = reduce_partials_col_sum<W>(part_ztr, pcount, red);
  const real nr = reduce_partials_col_max<W>(part_max, pcount, red);
  const real thr = tol > (real)1e-12 ? tol : (real)1e-12;
  const bool conv = nr < thr;
  if (!zero && !conv)
    for (size_t f = gtid; f < (size_t)n * W; f += gs) p[f] = z[f];
  if (blockIdx.x == 0) {
    if (threadIdx.x < W && !zero) {
      ctl->ztr[0][col] = ztr;
      ctl->norm_r[col] = nr;
      if (conv) ctl->done[col] = 1;
    }
    set_all_done(ctl, W, zero || conv);
  }
}

// private.c:181-197 per column; PERCOL as in k_m_cg_init
template <int W, bool PERCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cg_update(real *x, real *r, real *z, const real *__restrict__ p, const real *__restrict__ Gp,
                                                              const real *__restrict__ M, int n, const real *part_pgp, int cnt_pgp,
                                                              real *part_ztr, real *part_max, const CgCtlM *ctl, int parity) {
  __shared__ real red[4 * W];
  if (ctl->all_done) return;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (size_t)gridDim.x * blockDim.x;
  const int col = threadIdx.x & (W - 1);
  const int done = ctl->done[col];
  const real ztr_in = ctl->ztr[parity][col];
  const real pgp = reduce_partials_col_sum<W>(part_pgp, cnt_pgp, red);
  real ztr = 0, mx = 0;
  if (!done) {
    const real alpha = ztr_in / pgp;
    for (size_t f = gtid; f < (size_t)n * W; f += gs) {
      x[f] += alpha * p[f];
      const real ri = r[f] + (-alpha) * Gp[f];
      r[f] = ri;
      const real zi = ri * M[PERCOL ? f : f / W];
      z[f] = zi;
      ztr += zi * ri;
      const real a = absval(ri);
      mx = a > mx ? a : mx;
    }
  }
  ztr = block_col_sum<W>(ztr, red);
  mx = block_col_max<W>(mx, red);
  if (threadIdx.x < W) {
    part_ztr[(size_t)blockIdx.x * W + threadIdx.x] = ztr;
    part_max[(size_t)blockIdx.x * W + threadIdx.x] = mx;
  }
}

// private.c:202-214 per column
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cg_direction(real *p, const real *__restrict__ z, int n, const real *part_ztr,
                                                                 const real *part_max, int pcount, CgCtlM *ctl, int parity) {
  __shared__ real red[4 * W];
  if (ctl->all_done) return;
  const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (size_t)gridDim.x * blockDim.x;
  const int col = threadIdx.x & (W - 1);
  const int done = ctl->done[col];
  const real ztr_prev = ctl->ztr[parity][col], tol = ctl->tol[col];
  const int its = ctl->iters[col], max_its = ctl->max_its;
  const real ztr = reduce_partials_col_sum<W>(part_ztr, pcount, red);
  const real nr = reduce_partials_col_max<W>(part_max, pcount, red);
  const bool conv = nr < tol;
  const bool brk = !conv && ztr_prev == (real)0;
  if (!done && !conv && !brk) {
    const real beta = ztr / ztr_prev;
    for (size_t f = gtid; f < (size_t)n * W; f += gs) p[f] = z[f] + beta * p[f];
  }
  if (blockIdx.x == 0) {
    bool stop = done != 0;
    if (threadIdx.x < W && !done) {
      const int it2 = brk ? its : its + 1; // converged at i -> i + 1; breakdown returns i (private.c:203,216)
      ctl->ztr[parity ^ 1][col] = ztr;
      ctl->norm_r[col] = nr;
      ctl->iters[col] = it2;
      stop = conv || brk || it2 >= max_its;
      if (stop) ctl->done[col] = 1;
    }
    set_all_done(ctl, W, stop);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The instantiations of csr_block_kernel that are built, 13 per width: shared values take a shared d with every epilogue (5) and a
// per-column d where the epilogue has a d (3); per-column values take a per-column d exactly where there is a d (5).  The launch
// below names a kernel under this predicate only, so a combination outside it cannot be built by accident: it is refused at run time.
constexpr bool epi_has_d(int epi) { return epi == EPI_DIV || epi == EPI_GP || epi == EPI_NEGDIV; }
constexpr bool spmm_built(int epi, bool dcol, bool vcol) { return vcol ? dcol == epi_has_d(epi) : !dcol || epi_has_d(epi); }

struct SpmmArgs {
  int g;
  hipStream_t st;
  CsrView v;
  const real *X;
  real *Y;
  EpiArgs e;
  const int *cskip, *allskip;
  const real *vals;
  eoff bias;
};
template <bool VCOL>
static ValBlk<VCOL> val_blk(const real *vals, eoff bias) {
  if constexpr (VCOL) return ValBlk<true>{vals, bias};
  else return ValBlk<false>{};
}
template <int W, int EPI, bool DCOL, bool VCOL>
static void launch_spmm_as(const SpmmArgs &a) {
  if constexpr (spmm_built(EPI, DCOL, VCOL)) {
    hipLaunchKernelGGL((csr_block_kernel<W, EPI, DCOL, VCOL>), dim3(a.g), dim3(SCSAMD_BLOCK), 0, a.st, a.v, a.X, a.Y, a.e, a.cskip, a.allskip,
                       val_blk<VCOL>(a.vals, a.bias));
  } else {
    throw HipError(VCOL ? "scs_amd: per-column values run under per-column R" : "scs_amd: this block-product epilogue has no per-column form");
  }
}
template <int W, bool DCOL, bool VCOL>
static void launch_spmm_epi(int epi, const SpmmArgs &a) {
  switch (epi) {
  case EPI_PLAIN: return launch_spmm_as<W, EPI_PLAIN, DCOL, VCOL>(a);
  case EPI_DIV: return launch_spmm_as<W, EPI_DIV, DCOL, VCOL>(a);
  case EPI_GP: return launch_spmm_as<W, EPI_GP, DCOL, VCOL>(a);
  case EPI_ACC: return launch_spmm_as<W, EPI_ACC, DCOL, VCOL>(a);
  case EPI_NEGDIV: return launch_spmm_as<W, EPI_NEGDIV, DCOL, VCOL>(a);
  default: throw HipError("scs_amd: bad block-product epilogue");
  }
}
void LinSys::launch_spmm(int W, int epi, const CsrDev &mat, const real *X, real *Y, const EpiArgs &e, const int *cskip, const int *allskip,
                         bool dcol, const real *vals) {
  SpmmArgs a{spmm_grid(mat.rows, W), stream, mat.view(), X, Y, e, cskip, allskip, vals, (eoff)mat.bias};
  if (vals) a.v.val = nullptr; // the pattern only: the values are the block's
  MULTI_DISPATCH(W, MULTI_FLAG(dcol, DCOL, MULTI_FLAG(vals != nullptr, VCOL, (launch_spmm_epi<MW, DCOL, VCOL>(epi, a)))));
  n_spmv++;
}

void LinSys::ensure_multi(int W) {
  if (shard) throw HipError("scs_amd: block solves are not available on a row-sharded workspace");
  if (!multi) multi = new MultiWork();
  MultiWork &mw = *multi;
  if (mw.width >= W) return;
  mw.width = 0; // a failed allocation below leaves a state that is built again at the next call
  const size_t nw = (size_t)n * W, mwid = (size_t)m * W;
  mw.bx.alloc(nw);
  mw.by.alloc(mwid);
  mw.s.alloc(nw);
  mw.r.alloc(nw);
  mw.z.alloc(nw);
  mw.p.alloc(nw);
  mw.gt.alloc(nw + mwid);
  if (has_P) mw.Pp.alloc(nw);
  mw.part_pgp.alloc((size_t)SPMM_MAX_GRID * MULTI_W_MAX);
  mw.part_ztr.alloc((size_t)PART_CAP / 2 * MULTI_W_MAX);
  mw.part_max.alloc((size_t)PART_CAP / 2 * MULTI_W_MAX);
  if (!mw.ctl.p) mw.ctl.alloc(1);
  if (!mw.hctl.p) mw.hctl.alloc(1);
  mw.width = W;
}

// The R blocks of the per-column solves at width W (2 n W + m W values): allocated by the first per-column call, so a caller who
// never makes one holds what ensure_multi allocates and nothing more; freed with the workspace.
void LinSys::ensure_multi_r(int W) {
  ensure_multi(W);
  MultiWork &mw = *multi;
  if (mw.rwidth >= W) return;
  mw.rwidth = 0;
  mw.rxb.alloc((size_t)n * W);
  mw.ryb.alloc((size_t)m * W);
  mw.Mb.alloc((size_t)n * W);
  mw.rwidth = W;
}

// The value blocks of the per-value solves (scs_amd_linsys_set_values_multi): 2 nnz(A) W + nnz(full P) W + n W values and one
// staged column.  Allocated by the first set call only, rebuilt when a set call needs a wider block, freed with the workspace or
// by free_multi_values.  A failed allocation leaves the workspace usable with no value blocks (vwidth = 0).
void LinSys::free_multi_values() {
  if (!multi) return;
  MultiWork &mw = *multi;
  mw.vwidth = 0;
  mw.vcols = 0;
  mw.vA.release();
  mw.vAt.release();
  mw.vP.release();
  mw.vPdiag.release();
  mw.vstage.release();
}
void LinSys::ensure_multi_values(int W) {
  ensure_multi_r(W);
  MultiWork &mw = *multi;
  if (mw.vwidth >= W) return;
  free_multi_values();
  try {
    mw.vA.alloc((size_t)At.nnz * W);
    mw.vAt.alloc((size_t)At.nnz * W);
    if (has_P) {
      mw.vP.alloc((size_t)P.nnz * W);
      mw.vPdiag.alloc((size_t)n * W);
    }
    mw.vstage.alloc((size_t)std::max<long long>(At.nnz, has_P ? nnzP_up : 0));
  } catch (...) {
    free_multi_values();
    throw;
  }
  mw.vwidth = W;
}

// K columns of values, host arrays in the CSC order of init's A / upper P (AX: nnz(A) x K, PX: nnz(upper P) x K, column-major),
// into the value blocks at the layout width W of K columns; padding columns 0.  One column is staged at a time (the staging is
// reused in stream order) and scattered into each block by k_m_upd_gather_block through the maps of ensure_update_maps.  Returns
// with the stream idle: the caller's arrays may be pageable and reused.
void LinSys::set_multi_values(int K, int W, const real *AX, size_t ldax, const real *PX, size_t ldpx) {
  ensure_update_maps(true, has_P);
  ensure_multi_values(W);
  MultiWork &mw = *multi;
  mw.vcols = 0; // a failure below leaves no set in force
  const long long nza = At.nnz, nzp = has_P ? P.nnz : 0;
  if (nza > 0) {
    HIP_CHECK(hipMemsetAsync(mw.vA.p, 0, (size_t)nza * W * sizeof(real), stream));
    HIP_CHECK(hipMemsetAsync(mw.vAt.p, 0, (size_t)nza * W * sizeof(real), stream));
  }
  if (nzp > 0) HIP_CHECK(hipMemsetAsync(mw.vP.p, 0, (size_t)nzp * W * sizeof(real), stream));
  for (int k = 0; k < K; ++k) {
    if (nza > 0) {
      mw.vstage.upload(AX + (size_t)k * ldax, (size_t)nza, stream);
      MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_upd_gather_block<MW>, dim3(upd_grid(nza)), dim3(SCSAMD_BLOCK), 0, stream,
                                           (const real *)mw.vstage.p, (const eoff *)nullptr, mw.vAt.p, nza, k));
      MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_upd_gather_block<MW>, dim3(upd_grid(nza)), dim3(SCSAMD_BLOCK), 0, stream,
                                           (const real *)mw.vstage.p, (const eoff *)upd_rpos.p, mw.vA.p, nza, k));
    }
    if (nzp > 0) {
      mw.vstage.upload(PX + (size_t)k * ldpx, (size_t)nnzP_up, stream);
      MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_upd_gather_block<MW>, dim3(upd_grid(nzp)), dim3(SCSAMD_BLOCK), 0, stream,
                                           (const real *)mw.vstage.p, (const eoff *)upd_fsrc.p, mw.vP.p, nzp, k));
    }
  }
  if (has_P) {
    CsrView pv = P.view();
    pv.val = nullptr;
    const ValBlk<true> vb{mw.vP.p, (eoff)P.bias};
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_upd_pdiag<MW>, dim3(vec_grid((long long)n * W)), dim3(SCSAMD_BLOCK), 0, stream, pv, vb, mw.vPdiag.p));
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
  mw.vcols = K;
}

// Minv(n x W) = the Jacobi preconditioner of every column under its own rx (n x W) / ry (m x W): k_precond per column.
// vAt (with vPdiag when there is a P): every column under its own values too; the workspace's At.val and Pdiag are not read.
void LinSys::precond_multi_blocks(int W, const MultiOp &op, real *Minv) {
  CsrView v = At.view();
  if (op.vcol()) v.val = nullptr;
  const real *pd = !has_P ? nullptr : op.vcol() ? op.vPdiag : Pdiag.p;
  const int g = vec_grid((long long)n * W);
  MULTI_DISPATCH(W, MULTI_FLAG(op.vcol(), VCOL, hipLaunchKernelGGL((k_m_precond<MW, VCOL>), dim3(g), dim3(SCSAMD_BLOCK), 0, stream, v, op.rx,
                                                                   op.ry, pd, Minv, val_blk<VCOL>(op.vAt, (eoff)At.bias))));
}

// G X on blocks (private.c:106-119 per column) under op; dot_partials as in launch_spmm's EPI_GP
void LinSys::mat_vec_multi_dev(int W, const MultiOp &op, const real *X, real *Y, real *dot_partials, const int *cskip, const int *allskip) {
  MultiWork &mw = *multi;
  real *tmpb = mw.gt.p + (size_t)n * mw.width;
  const bool percol = op.percol();
  EpiArgs e1{percol ? op.ry : ry.p, nullptr, nullptr, nullptr};
  launch_spmm(W, EPI_DIV, A, X, tmpb, e1, cskip, allskip, percol, op.vA);
  if (has_P) {
    EpiArgs ep{nullptr, nullptr, nullptr, nullptr};
    launch_spmm(W, EPI_PLAIN, P, X, mw.Pp.p, ep, cskip, allskip, false, op.vP);
  }
  EpiArgs e2{percol ? op.rx : rx.p, X, has_P ? mw.Pp.p : nullptr, dot_partials};
  launch_spmm(W, EPI_GP, At, tmpb, Y, e2, cskip, allskip, percol, op.vAt);
  n_matvecs++;
}

// The launchers of the vector kernels that have per-column forms: op.percol() and, for k_m_rhs_prep, "one warm-scale per column"
// become the template arguments; R_y and the preconditioner are op's blocks or the workspace's vectors accordingly.
template <typename WS>
static void launch_rhs_prep_ws(LinSys &ls, int W, int K, const MultiRhs &a, real *tmp, const TolArgs &ta, int max_its, int g, WS ws) {
  MultiWork &mw = *ls.multi;
  const real *ry = a.op.percol() ? a.op.ry : ls.ry.p;
  MULTI_DISPATCH(W, MULTI_FLAG(a.op.percol(), PERCOL,
                               hipLaunchKernelGGL((k_m_rhs_prep<MW, PERCOL, WS>), dim3(g), dim3(SCSAMD_BLOCK), 0, ls.stream, a.bx, a.by, ry,
                                                  tmp, ls.n, ls.m, mw.part_max.p, g, mw.ctl.p, ta, K, max_its,
                                                  a.warm_part, a.warm_cnt, ws, a.pre_stopped)));
}
static void launch_rhs_prep(LinSys &ls, int W, int K, const MultiRhs &a, real *tmp, const TolArgs &ta, int max_its, int g) {
  if (!a.warm_scale_col) return launch_rhs_prep_ws(ls, W, K, a, tmp, ta, max_its, g, a.warm_scale);
  TolArgs ws{}; // every column its own factor of the warm-start term
  for (int k = 0; k < W; ++k) ws.t[k] = a.warm_scale_col[k];
  launch_rhs_prep_ws(ls, W, K, a, tmp, ta, max_its, g, ws);
}
static void launch_cg_init(LinSys &ls, int W, const MultiRhs &a, int g) {
  MultiWork &mw = *ls.multi;
  const real *Minv = a.op.percol() ? a.op.Minv : ls.M.p;
  MULTI_DISPATCH(W, MULTI_FLAG(a.op.percol(), PERCOL,
                               hipLaunchKernelGGL((k_m_cg_init<MW, PERCOL>), dim3(g), dim3(SCSAMD_BLOCK), 0, ls.stream, a.bx, a.s, mw.r.p, mw.z.p,
                                                  Minv, ls.n, mw.part_ztr.p, mw.part_max.p, mw.ctl.p)));
}
static void launch_cg_update(LinSys &ls, int W, const MultiRhs &a, const real *Gp, int g, int cnt_pgp, int parity) {
  MultiWork &mw = *ls.multi;
  const real *Minv = a.op.percol() ? a.op.Minv : ls.M.p;
  MULTI_DISPATCH(W, MULTI_FLAG(a.op.percol(), PERCOL,
                               hipLaunchKernelGGL((k_m_cg_update<MW, PERCOL>), dim3(g), dim3(SCSAMD_BLOCK), 0, ls.stream, a.bx, mw.r.p, mw.z.p,
                                                  mw.p.p, Gp, Minv, ls.n, mw.part_pgp.p, cnt_pgp, mw.part_ztr.p, mw.part_max.p, mw.ctl.p,
                                                  parity)));
}

// K columns (2 <= K <= W) on blocks the caller holds (a.bx: n x W, a.by: m x W, a.s: n x W or null): [r_x; r_y] -> [x; y] in place,
// with the options of MultiRhs and under the operator a.op (linsys.h).  The steps are those of private.c:284-324 per column:
// |b|_inf, the zero test and tmp = R_y^-1 r_y, b_x += A' tmp, r = G s when warm, the first residual, p = z, the iteration in
// batches, y.
void LinSys::solve_multi_blocks(int K, int W, const MultiRhs &a, const real *tolv, int *iters_out) {
  MultiWork &mw = *multi;
  const bool warm = a.s != nullptr;
  const MultiOp &op = a.op;
  op.check(has_P);
  const bool percol = op.percol();
  real *const bx = a.bx, *const by = a.by;
  const int gv = vec_grid((long long)n * W), gnm = vec_grid(((long long)n + m) * W);
  CgCtlM *c = mw.ctl.p;
  real *Gp = mw.gt.p, *tmpb = mw.gt.p + (size_t)n * mw.width;
  const int *zero = c->zero_rhs, *done = c->done, *all = &c->all_done;
  const int max_its = (int)std::min<long long>(10LL * n, 2147483647LL); // private.c:307
  TolArgs ta{};
  for (int k = 0; k < K; ++k) ta.t[k] = tolv[k];
  const size_t nx = (size_t)n * W, ny = (size_t)m * W;
  const long long mv0 = n_matvecs;
  const EpiArgs none{nullptr, nullptr, nullptr, nullptr}, by_ry{percol ? op.ry : ry.p, nullptr, nullptr, nullptr};

  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_absmax<MW>, dim3(gnm), dim3(SCSAMD_BLOCK), 0, stream, bx, nx, by, ny, mw.part_max.p));
  launch_rhs_prep(*this, W, K, a, tmpb, ta, max_its, gnm);
  launch_spmm(W, EPI_ACC, At, tmpb, bx, none, zero, all, false, op.vAt);           // b_x += A' R_y^-1 r_y   (private.c:305)
  if (warm) mat_vec_multi_dev(W, op, a.s, mw.r.p, nullptr, zero, all);             // r = G s  (private.c:153)
  launch_cg_init(*this, W, a, gv);
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_cg_start<MW>, dim3(gv), dim3(SCSAMD_BLOCK), 0, stream, mw.p.p, mw.z.p, n, mw.part_ztr.p,
                                       mw.part_max.p, gv, c));
  // iteration batches: one control record read per batch, as solve_dev does with cg_pace=0 (every column's own count has to be
  // read back after the solve anyway, and the all-stopped word would need a maximum over the columns to pace by: left on batches)
  const int gp = spmm_grid(At.rows, W);
  long long it = 0;
  int batch = std::max(4, std::min(mw.last_its + 1, 4096));
  for (;;) {
    int nb = (int)std::min<long long>(batch, (long long)max_its - it);
    if (nb < 1) nb = 1;
    for (int j = 0; j < nb; ++j) {
      const int q = (int)((it + j) & 1);
      mat_vec_multi_dev(W, op, mw.p.p, Gp, mw.part_pgp.p, done, all);
      launch_cg_update(*this, W, a, Gp, gv, gp, q);
      MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_cg_direction<MW>, dim3(gv), dim3(SCSAMD_BLOCK), 0, stream, mw.p.p, mw.z.p, n, mw.part_ztr.p,
                                           mw.part_max.p, gv, c, q));
    }
    it += nb;
    HIP_CHECK(hipMemcpyAsync(mw.hctl.p, c, sizeof(CgCtlM), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (mw.hctl.p->all_done || it >= max_its) break;
    batch = std::max(4, std::min(mw.last_its / 4 + 1, 1024));
  }
  launch_spmm(W, EPI_NEGDIV, A, bx, by, by_ry, zero, nullptr, percol, op.vA); // y = R_y^-1 (A x - r_y)   (private.c:313-317)
  HIP_CHECK(hipGetLastError());
  int most = 0;
  for (int k = 0; k < K; ++k) {
    const int its = mw.hctl.p->iters[k];
    if (iters_out) iters_out[k] = its;
    tot_cg_its += its;
    most = std::max(most, its);
  }
  mw.last_its = most;
  n_solves += K;
  n_matvecs = mv0 + most + (warm ? 1 : 0); // a block product counts once; products enqueued past the last stop did nothing
}

} // namespace scsamd
