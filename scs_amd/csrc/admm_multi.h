// admm_multi.h -- a family of problems that share A, P and the cones, solved in ONE device-resident ADMM loop on one workspace
// (part of admm.hip: included there, behind the single-vector loop whose helpers it uses).
//
// Column k is the map of reference src/scs.c:1356-1455 applied to problem k alone: its own tau, kappa, root_plus, scales of
// normalize_b_c, g = (R + M)^-1 [c_k; -b_k], residuals, CG tolerance schedule (:745-762), convergence test, status and ScsInfo.
// The columns share A, P, D, E, the cone description and -- in scs_amd_solve_family -- diag_r, and nothing else.  Every per-column reduction (|v|, the dots of
// root_plus, the norms and inner products of populate_residuals) runs over the lanes and workgroup partials of one column only --
// the fixed butterfly over the lanes of a column, the waves in wave order, one partial per workgroup and column re-reduced in
// index order -- so within one width the bits of a column depend neither on its neighbours nor on its position.  No floating-point
// atomics.
//
// Layout: the block layout of spmm.h / linsys_multi.h / cones_multi.h -- row-major, element (i, k) at i * W + k, W in {2, 4, 8, 16}.
// A block of l = n + m + 1 rows is [x rows | y rows | the tau row], so its x and y parts ARE the n x W and m x W blocks the block
// solve and the block projection take: nothing is copied between the steps of an iteration.  Lane t serves column t % W of row t / W.
//
// Control: a per-column record on the device (FamCtl: scales and the frozen flag) next to the block solve's CgCtlM.  Convergence is
// tested where the single solve tests it (i % CONVERGED_INTERVAL == 0), for all running columns in one block residual evaluation
// and one read-back of NQ x W scalars.  A column whose test fires at iteration i is frozen there (info.iter = i, exactly where
// the single loop breaks): from then on its u, v, rsk are not written, its lanes load and store nothing in the glue kernels, the
// block products (cskip of csr_block_kernel) and the block solve (pre_stopped of MultiRhs), and its slot of the cone block is
// scratch.  Padding columns k >= K are frozen from the start and hold zeros.
//
// Two entries, one loop.  scs_amd_solve_family: the columns share the workspace's diag_r (the instantiations with PERCOL / PC =
// false).  scs_amd_solve_family_scaled: column k runs under its own diag_r_k, built from its own scale, in an l x W block R whose x
// and y rows are the rx / ry blocks of the per-column block solve (MultiRhs::rx / ry / Minv, linsys_multi.h); the glue kernels read
// R[f] where the shared form reads R[f / W], in the same expressions, so equal scales give the shared form's bits.  With
// adaptive_scale the column runs update_scale (admm.hip, :1164-1241) on its own residuals where the single loop runs it -- at a
// check, after the convergence test, before the dual update.  For the columns whose scale changed (FamCtl::upd), in this order:
// their R (k_f_set_diag_r), the preconditioners (precond_multi_blocks) and the box cone's copy of r_y, their g (rebuilt and solved
// cold to CG_BEST_TOL with every other column stopped on entry), their v (k_f_remap_v).  Of a column that did not update not one
// bit is read or written by this, and a frozen column never updates.
//
// Refused: acceleration_lookback (the Anderson memory is per problem) and log_csv_filename; by scs_amd_solve_family also
// adaptive_scale (a scale update changes diag_r, which its columns share).
#pragma once

namespace scsamd {

struct FamCtl {
  real ps[MULTI_W_MAX], ds[MULTI_W_MAX]; // primal_scale / dual_scale of normalize_b_c, per column
  int frozen[MULTI_W_MAX];               // non-zero: the column has finished (or is padding): nothing of it is read or written
  // scs_amd_solve_family_scaled only: the column's own scale, and the columns whose scale has just been set (upd) or not (keep, the
  // complement: what a block solve takes as pre_stopped).  Read by the kernels of a scale update and by nothing else.
  real scale[MULTI_W_MAX];
  int upd[MULTI_W_MAX], keep[MULTI_W_MAX];
};

// ----------------------------------------------------------------------------
// glue kernels on blocks: the kernels of admm.hip with lane -> (row t / W, column t % W)
// ----------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_sumsq_partial(const real *__restrict__ v, int len, real *part, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  const size_t tot = (size_t)len * W, gs = (size_t)gridDim.x * blockDim.x; // gs % W == 0: a lane stays in its column
  real s = 0;
  if (!ctl->frozen[col])
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) s += v[f] * v[f];
  s = block_col_sum<W>(s, red);
  if (threadIdx.x < W) part[(size_t)blockIdx.x * W + threadIdx.x] = s;
}

// k_prep_linsys per column: normalize_v, u_t = [R_x v; -R_y v; v_tau], warm = u_x + tau g_x with its |.|_inf partials
// PERCOL (here and in the three kernels below that read R): R is an l x W block, every column its own diag_r, instead of one vector
// of l -- R[f] where the shared form reads R[f / W], in the same expression: equal scales give the shared form's bits.
template <int W, bool PERCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_prep_linsys(real *v, real *u_t, const real *__restrict__ u, const real *__restrict__ g,
                                                                const real *__restrict__ R, real *warm, int n, int l, const real *nrm_part,
                                                                int nrm_cnt, real *warm_part, int do_normalize, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  const bool on = !ctl->frozen[col];
  real factor = 1;
  if (do_normalize) {
    const real nrm = sqrt(reduce_partials_col_sum<W>(nrm_part, nrm_cnt, red));
    if (nrm != (real)0) factor = sqrt((real)l) * (real)1. / nrm;
  }
  real mx = 0;
  if (on) {
    const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x;
    const real tau = u[(size_t)(l - 1) * W + col];
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
      const int i = (int)(f / W);
      real vi = v[f];
      if (do_normalize) {
        vi *= factor;
        v[f] = vi;
      }
      real ut;
      if (i < n) {
        ut = vi * R[PERCOL ? f : (size_t)i];
        const real w = u[f] + tau * g[f];
        warm[f] = w;
        const real a = absval(w);
        mx = a > mx ? a : mx;
      } else if (i < l - 1) {
        ut = -vi * R[PERCOL ? f : (size_t)i];
      } else {
        ut = vi;
      }
      u_t[f] = ut;
    }
  }
  mx = block_col_max<W>(mx, red);
  if (threadIdx.x < W) warm_part[(size_t)blockIdx.x * W + threadIdx.x] = mx;
}

// the five R-weighted dots of root_plus per column -> part[(q * stride + workgroup) * W + column]
template <int W, bool PERCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_root_plus_partial(const real *__restrict__ p, const real *__restrict__ mu,
                                                                      const real *__restrict__ g, const real *__restrict__ R, int nm,
                                                                      real *part, int stride, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  real gg = 0, mug = 0, pg = 0, pp = 0, pmu = 0;
  if (!ctl->frozen[col]) {
    const size_t tot = (size_t)nm * W, gs = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
      const real ri = R[PERCOL ? f : f / W], gi = g[f], pi = p[f], mui = mu[f];
      gg += gi * gi * ri;
      mug += mui * gi * ri;
      pg += pi * gi * ri;
      pp += pi * pi * ri;
      pmu += pi * mui * ri;
    }
  }
  gg = block_col_sum<W>(gg, red);
  mug = block_col_sum<W>(mug, red);
  pg = block_col_sum<W>(pg, red);
  pp = block_col_sum<W>(pp, red);
  pmu = block_col_sum<W>(pmu, red);
  if (threadIdx.x < W) {
    const size_t o = (size_t)blockIdx.x * W + threadIdx.x, sw = (size_t)stride * W;
    part[0 * sw + o] = gg;
    part[1 * sw + o] = mug;
    part[2 * sw + o] = pg;
    part[3 * sw + o] = pp;
    part[4 * sw + o] = pmu;
  }
}

// k_post_linsys per column: tau~, u_t -= tau~ g, u = 2 u_t - v, cw = -R_y (2 u_t - v)_y
template <int W, bool PERCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_post_linsys(real *u_t, real *u, const real *__restrict__ v, const real *__restrict__ g,
                                                                const real *__restrict__ R, real *cw, int n, int l, const real *part, int cnt,
                                                                int stride, int feasible_iter, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  const bool on = !ctl->frozen[col];
  real tau_t = 1;
  if (!feasible_iter) {
    const size_t sw = (size_t)stride * W;
    const real gg = reduce_partials_col_sum<W>(part + 0 * sw, cnt, red);
    const real mug = reduce_partials_col_sum<W>(part + 1 * sw, cnt, red);
    const real pg = reduce_partials_col_sum<W>(part + 2 * sw, cnt, red);
    const real pp = reduce_partials_col_sum<W>(part + 3 * sw, cnt, red);
    const real pmu = reduce_partials_col_sum<W>(part + 4 * sw, cnt, red);
    if (on) {
      const real tau_scale = R[PERCOL ? (size_t)(l - 1) * W + col : (size_t)(l - 1)], eta = v[(size_t)(l - 1) * W + col];
      tau_t = root_plus_from_coeffs(tau_scale + gg, mug - 2 * pg - eta * tau_scale, pp - pmu);
    }
  }
  if (!on) return;
  const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x, nw = (size_t)n * W;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const int i = (int)(f / W);
    if (i < l - 1) {
      const real ut = u_t[f] + g[f] * (-tau_t);
      u_t[f] = ut;
      const real uu = 2 * ut - v[f];
      u[f] = uu;
      if (i >= n) cw[f - nw] = uu * (-R[PERCOL ? f : (size_t)i]);
    } else {
      u_t[f] = tau_t;
      const real uu = 2 * tau_t - v[f];
      u[f] = feasible_iter ? (real)1 : (uu > (real)0 ? uu : (real)0); // :804-808
    }
  }
}

// k_post_cone per column: the Moreau post of the cone part, rsk = R (v + u - 2 u_t) and, with alpha > 0, v += alpha (u - u_t)
template <int W, bool PERCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_post_cone(real *u, const real *__restrict__ u_t, real *v, real *rsk,
                                                              const real *__restrict__ R, const real *__restrict__ cw, int n, int l,
                                                              real alpha, const FamCtl *ctl) {
  if (ctl->frozen[threadIdx.x & (W - 1)]) return;
  const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x, nw = (size_t)n * W;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const int i = (int)(f / W);
    real ui = u[f];
    const real ri = R[PERCOL ? f : (size_t)i];
    if (i >= n && i < l - 1) {
      ui = cw[f - nw] / ri + ui;
      u[f] = ui;
    }
    const real vi = v[f], ut = u_t[f];
    rsk[f] = (vi + ui - 2 * ut) * ri;
    if (alpha > (real)0) v[f] = vi + alpha * (ui - ut);
  }
}

template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_dual_update(real *v, const real *__restrict__ u, const real *__restrict__ u_t, int l,
                                                                real alpha, const FamCtl *ctl) {
  if (ctl->frozen[threadIdx.x & (W - 1)]) return;
  const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) v[f] += alpha * (u[f] - u_t[f]);
}

// g = [c; -b] per column; skip (W ints): the columns that are left as they are
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_build_g(real *g, const real *__restrict__ c, const real *__restrict__ b, int n, int m,
                                                            const int *skip) {
  if (skip[threadIdx.x & (W - 1)]) return;
  const size_t tot = (size_t)(n + m) * W, gs = (size_t)gridDim.x * blockDim.x, nw = (size_t)n * W;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) g[f] = f < nw ? c[f] : -b[f - nw];
}

// ---- the kernels of a per-column scale (scs_amd_solve_family_scaled) ---------------------------------------------------------
// k_set_diag_r on the l x W block, for the columns in ctl->upd only: diag_r_k = [rho_x; 1/(1000 scale_k) on the zero cone,
// 1/scale_k elsewhere; TAU_FACTOR], in k_set_diag_r's expressions.  Padding columns (>= K) get R = 1, as the block solve's
// per-column entry gives them: ordinary finite columns.
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_set_diag_r(real *R, int n, int m, int z, real rho_x, int K, const FamCtl *ctl) {
  const int col = threadIdx.x & (W - 1);
  if (!ctl->upd[col]) return;
  const real scale = ctl->scale[col];
  const int l = n + m + 1;
  const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const int i = (int)(f / W);
    real r;
    if (col >= K) r = (real)1;
    else if (i < n) r = rho_x;
    else if (i < n + z) r = (real)1.0 / ((real)1000. * scale);
    else if (i < l - 1) r = (real)1.0 / scale;
    else r = (real)TAU_FACTOR;
    R[f] = r;
  }
}

// k_remap_v on blocks, for the columns in ctl->upd only: v = rsk / R + 2 u_t - u after a scale update (:1236-1238)
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_remap_v(real *v, const real *__restrict__ rsk, const real *__restrict__ R,
                                                            const real *__restrict__ u_t, const real *__restrict__ u, int l,
                                                            const FamCtl *ctl) {
  if (!ctl->upd[threadIdx.x & (W - 1)]) return;
  const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) v[f] = rsk[f] / R[f] + 2 * u_t[f] - u[f];
}

// ---- residuals per column: the quantities Q_* of admm.hip -> part[(q * stride + workgroup) * W + column] --------------------
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_resid_primal(const real *__restrict__ ax, const real *__restrict__ s,
                                                                 const real *__restrict__ y, const real *__restrict__ b,
                                                                 const real *__restrict__ D, const real *tau_row, int m, real *part,
                                                                 int stride, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  real q_pri = 0, q_axs = 0, q_ax = 0, o_pri = 0, o_axs = 0, o_ax = 0, o_s = 0, n_s = 0, bty = 0;
  if (!ctl->frozen[col]) {
    const real tau = absval(tau_row[col]), ds = ctl->ds[col], inv_ds = (real)1.0 / ds;
    const size_t tot = (size_t)m * W, gs = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
      const real axi = ax[f], si = s[f], bi = b[f], Di = D[f / W];
      const real axs = axi + si;
      const real pri = axs - tau * bi;
      const real fo = inv_ds / Di;
      real a;
      a = absval(pri); q_pri = a > q_pri ? a : q_pri;
      a = absval(axs); q_axs = a > q_axs ? a : q_axs;
      a = absval(axi); q_ax = a > q_ax ? a : q_ax;
      a = absval(pri * fo); o_pri = a > o_pri ? a : o_pri;
      a = absval(axs * fo); o_axs = a > o_axs ? a : o_axs;
      a = absval(axi * fo); o_ax = a > o_ax ? a : o_ax;
      a = absval(si / (Di * ds)); o_s = a > o_s ? a : o_s;
      a = absval(si); n_s = a > n_s ? a : n_s;
      bty += y[f] * bi;
    }
  }
  q_pri = block_col_max<W>(q_pri, red); q_axs = block_col_max<W>(q_axs, red); q_ax = block_col_max<W>(q_ax, red);
  o_pri = block_col_max<W>(o_pri, red); o_axs = block_col_max<W>(o_axs, red); o_ax = block_col_max<W>(o_ax, red);
  o_s = block_col_max<W>(o_s, red); n_s = block_col_max<W>(n_s, red);
  bty = block_col_sum<W>(bty, red);
  if (threadIdx.x < W) {
    const size_t o = (size_t)blockIdx.x * W + threadIdx.x, sw = (size_t)stride * W;
    part[Q_PRI_N * sw + o] = q_pri; part[Q_AXS_N * sw + o] = q_axs; part[Q_AX_N * sw + o] = q_ax;
    part[Q_PRI_O * sw + o] = o_pri; part[Q_AXS_O * sw + o] = o_axs; part[Q_AX_O * sw + o] = o_ax;
    part[Q_S_O * sw + o] = o_s; part[Q_S_N * sw + o] = n_s; part[Q_BTY * sw + o] = bty;
  }
}

template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_resid_dual(const real *px, const real *__restrict__ aty, const real *__restrict__ x,
                                                               const real *__restrict__ c, const real *__restrict__ E, const real *tau_row,
                                                               int n, real *part, int stride, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  real q_d = 0, q_px = 0, q_aty = 0, o_d = 0, o_px = 0, o_aty = 0, ctx = 0, xpx = 0;
  if (!ctl->frozen[col]) {
    const real tau = absval(tau_row[col]), inv_ps = (real)1.0 / ctl->ps[col];
    const size_t tot = (size_t)n * W, gs = (size_t)gridDim.x * blockDim.x;
    for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
      const real pxi = px ? px[f] : (real)0, ai = aty[f], xi = x[f], ci = c[f];
      const real dual = pxi + ai + tau * ci;
      const real fo = inv_ps / E[f / W];
      real a;
      a = absval(dual); q_d = a > q_d ? a : q_d;
      a = absval(pxi); q_px = a > q_px ? a : q_px;
      a = absval(ai); q_aty = a > q_aty ? a : q_aty;
      a = absval(dual * fo); o_d = a > o_d ? a : o_d;
      a = absval(pxi * fo); o_px = a > o_px ? a : o_px;
      a = absval(ai * fo); o_aty = a > o_aty ? a : o_aty;
      ctx += xi * ci;
      xpx += pxi * xi;
    }
  }
  q_d = block_col_max<W>(q_d, red); q_px = block_col_max<W>(q_px, red); q_aty = block_col_max<W>(q_aty, red);
  o_d = block_col_max<W>(o_d, red); o_px = block_col_max<W>(o_px, red); o_aty = block_col_max<W>(o_aty, red);
  ctx = block_col_sum<W>(ctx, red); xpx = block_col_sum<W>(xpx, red);
  if (threadIdx.x < W) {
    const size_t o = (size_t)blockIdx.x * W + threadIdx.x, sw = (size_t)stride * W;
    part[Q_DUAL_N * sw + o] = q_d; part[Q_PX_N * sw + o] = q_px; part[Q_ATY_N * sw + o] = q_aty;
    part[Q_DUAL_O * sw + o] = o_d; part[Q_PX_O * sw + o] = o_px; part[Q_ATY_O * sw + o] = o_aty;
    part[Q_CTX * sw + o] = ctx; part[Q_XPX * sw + o] = xpx;
  }
}

// one workgroup: out[q * W + column]
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_resid_final(const real *part, int stride, int cnt_m, int cnt_n, const real *tau_row,
                                                                const real *kap_row, real *out, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const size_t sw = (size_t)stride * W;
  for (int q = 0; q < Q_TAU; ++q) {
    const bool primal = q < Q_DUAL_N;
    const int cnt = primal ? cnt_m : cnt_n;
    const bool is_sum = q == Q_BTY || q == Q_CTX || q == Q_XPX;
    const real r = is_sum ? reduce_partials_col_sum<W>(part + q * sw, cnt, red) : reduce_partials_col_max<W>(part + q * sw, cnt, red);
    if (threadIdx.x < W) out[q * W + threadIdx.x] = r;
  }
  if (threadIdx.x < W && !ctl->frozen[threadIdx.x]) {
    out[Q_TAU * W + threadIdx.x] = absval(tau_row[threadIdx.x]);
    out[Q_KAP * W + threadIdx.x] = absval(kap_row[threadIdx.x]);
  }
}

} // namespace scsamd

// ============================================================================
// host control: solve_begin / solve_steps / populate_residuals / has_converged / finalize per column
// ============================================================================
#define FAM_DISPATCH(W_, CALL)                                                                                         \
  do {                                                                                                                 \
    switch (W_) {                                                                                                      \
    case 2: { constexpr int MW = 2; CALL; } break;                                                                     \
    case 4: { constexpr int MW = 4; CALL; } break;                                                                     \
    case 8: { constexpr int MW = 8; CALL; } break;                                                                     \
    case 16: { constexpr int MW = 16; CALL; } break;                                                                   \
    default: throw HipError("scs_amd: bad block width");                                                               \
    }                                                                                                                  \
  } while (0)

// Family state: belongs to scs_amd_solve_family only.  Blocks at the largest width used so far (a narrower chunk uses the front
// of each buffer at its own width), allocated at the first call, freed with the workspace.
struct FamilyWork {
  int width = 0;
  DevBuf<real> u, u_t, v, rsk; // l x W iterates
  DevBuf<real> g;              // (n + m) x W
  DevBuf<real> cw, warm;       // m x W cone block, n x W warm start of the block solve
  DevBuf<real> ax, aty, px;    // residual blocks
  DevBuf<real> b, c;           // per-column normalised data
  DevBuf<real> part, qout;     // reduction partials, NQ x W reduced scalars
  PinnedBuf<real> hq;
  DevBuf<FamCtl> ctl;
  PinnedBuf<FamCtl> hctl;
  std::vector<real> hblk, hblk2, col_x, col_y, col_s; // host staging
  // scs_amd_solve_family_scaled only, allocated at its first call (family_ensure_r): every column its own diag_r
  int rwidth = 0;
  DevBuf<real> R;    // l x W: [R_x rows | R_y rows | the tau row]; its x and y parts are the rx / ry blocks MultiRhs takes
  DevBuf<real> Minv; // n x W: the Jacobi preconditioner of every column under its own R (precond_multi_blocks)
};
static void family_free(FamilyWork *f) { delete f; }

// what the single solve keeps in the workspace for its one problem, per column
struct FamCol {
  Resid r_n, r_o;
  real ps = 1, ds = 1, nm_b_orig = 0, nm_c_orig = 0;
  int status = SCS_UNFINISHED, iter = 0;
  bool frozen = false;
  // the scaled entry: the column's own scale and the state of its update_scale
  real scale = 0, sum_log_scale_factor = 0;
  int last_scale_update_iter = 0, n_log_scale_factor = 0, scale_updates = 0;
  bool upd = false; // the scale has just been set: the next control record names the column in FamCtl::upd
};

static void family_ensure(ScsWork *w, int W) {
  if (!w->fam) w->fam = new FamilyWork();
  FamilyWork &f = *w->fam;
  if (f.width >= W) return;
  f.width = 0; // a failed allocation below leaves a state that is built again at the next call
  const size_t n = w->n, m = w->m, l = w->l;
  for (DevBuf<real> *b : {&f.u, &f.u_t, &f.v, &f.rsk}) b->alloc(l * W);
  f.g.alloc((n + m) * W);
  f.cw.alloc(m * W);
  f.warm.alloc(n * W);
  f.ax.alloc(m * W);
  f.aty.alloc(n * W);
  if (w->has_P) f.px.alloc(n * W);
  f.b.alloc(m * W);
  f.c.alloc(n * W);
  if (!f.part.p) f.part.alloc((size_t)NQ * PSTRIDE * MULTI_W_MAX);
  if (!f.qout.p) f.qout.alloc((size_t)NQ * MULTI_W_MAX);
  if (!f.hq.p) f.hq.alloc((size_t)NQ * MULTI_W_MAX);
  if (!f.ctl.p) f.ctl.alloc(1);
  if (!f.hctl.p) f.hctl.alloc(1);
  f.width = W;
}

// the R blocks of the scaled entry at width W (l W + n W values more): a caller who never makes a scaled call does not hold them
static void family_ensure_r(ScsWork *w, int W) {
  FamilyWork &f = *w->fam;
  if (f.rwidth >= W) return;
  f.rwidth = 0;
  f.R.alloc((size_t)w->l * W);
  f.Minv.alloc((size_t)w->n * W);
  f.rwidth = W;
}

// the message for a setting the entry refuses, or null (host only).  scaled: scs_amd_solve_family_scaled, where every column has its
// own diag_r and adaptive_scale is served
static const char *family_refusal(const ScsWork *w, bool scaled = false) {
  if (w->stgs.adaptive_scale && !scaled) return "scs_amd_solve_family requires adaptive_scale == 0: a scale update changes diag_r, which the problems of a family share";
  if (w->stgs.acceleration_lookback) return "scs_amd_solve_family requires acceleration_lookback == 0: Anderson acceleration is per problem";
  if (!w->log_csv_name.empty()) return "scs_amd_solve_family requires log_csv_filename == NULL: the per-iteration log describes one problem";
  return nullptr;
}

// one residual evaluation for all running columns, one read-back (populate_residuals on blocks)
static void family_residuals(ScsWork *w, int W, int K, FamCol *cols, int iter) {
  FamilyWork &f = *w->fam;
  const int n = w->n, m = w->m, l = w->l;
  hipStream_t st = w->stream;
  const size_t nw = (size_t)n * W;
  const real *x = f.u.p, *y = f.u.p + nw, *s = f.rsk.p + nw;
  const real *tau_row = f.u.p + (size_t)(l - 1) * W, *kap_row = f.rsk.p + (size_t)(l - 1) * W;
  const int *frozen = f.ctl.p->frozen;
  const EpiArgs e{nullptr, nullptr, nullptr, nullptr};
  w->ls.launch_spmm(W, EPI_PLAIN, w->ls.A, x, f.ax.p, e, frozen, nullptr);
  w->ls.launch_spmm(W, EPI_PLAIN, w->ls.At, y, f.aty.p, e, frozen, nullptr);
  if (w->has_P) w->ls.launch_spmm(W, EPI_PLAIN, w->ls.P, x, f.px.p, e, frozen, nullptr);
  const int gm = glue_grid((long long)m * W), gn = glue_grid((long long)n * W);
  FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_resid_primal<MW>, dim3(gm), dim3(SCSAMD_BLOCK), 0, st, f.ax.p, s, y, f.b.p, w->D.p, tau_row, m,
                                     f.part.p, PSTRIDE, f.ctl.p));
  FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_resid_dual<MW>, dim3(gn), dim3(SCSAMD_BLOCK), 0, st, w->has_P ? f.px.p : (const real *)nullptr,
                                     f.aty.p, x, f.c.p, w->E.p, tau_row, n, f.part.p, PSTRIDE, f.ctl.p));
  FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_resid_final<MW>, dim3(1), dim3(SCSAMD_BLOCK), 0, st, f.part.p, PSTRIDE, gm, gn, tau_row, kap_row,
                                     f.qout.p, f.ctl.p));
  HIP_CHECK(hipMemcpyAsync(f.hq.p, f.qout.p, (size_t)NQ * W * sizeof(real), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  w->cone_timer.harvest(); // stream is idle here
  if (w->cone.n_psd > 0) w->psd_unconverged += w->cone.take_status(st);
  for (int k = 0; k < K; ++k)
    if (!cols[k].frozen)
      fill_residuals(cols[k].r_n, cols[k].r_o, f.hq.p + k, W, iter, w->has_P, w->stgs.normalize != 0, cols[k].ps, cols[k].ds);
}

// pad_upd: the padding columns count as just set too (the first record of a scaled chunk: their R becomes 1)
static void family_upload_ctl(ScsWork *w, int W, int K, const FamCol *cols, int pad_upd = 0) {
  FamilyWork &f = *w->fam;
  for (int k = 0; k < MULTI_W_MAX; ++k) {
    f.hctl.p->ps[k] = k < K ? cols[k].ps : (real)1;
    f.hctl.p->ds[k] = k < K ? cols[k].ds : (real)1;
    f.hctl.p->frozen[k] = k < K && !cols[k].frozen ? 0 : 1;
    f.hctl.p->scale[k] = k < K ? cols[k].scale : (real)1;
    f.hctl.p->upd[k] = k < K ? (cols[k].upd ? 1 : 0) : pad_upd;
    f.hctl.p->keep[k] = f.hctl.p->upd[k] ? 0 : 1;
  }
  // the pinned record is rewritten only after a synchronisation of the stream (every caller has just waited on it)
  HIP_CHECK(hipMemcpyAsync(f.ctl.p, f.hctl.p, sizeof(FamCtl), hipMemcpyHostToDevice, w->stream));
}

// K (1 <= K <= W) problems as one block of width W.  B / Cc: column-major host data of this chunk.  Returns SCS_SIGINT when
// interrupted (the unfinished columns are then filled by fail_out), 0 otherwise; throws on a HIP failure.
// PC = false: scs_amd_solve_family, the columns share the workspace's diag_r.  PC = true: scs_amd_solve_family_scaled, column k
// runs under its own diag_r_k from scales[k] (null: the workspace's stgs.scale in every column) and, with adaptive_scale, under its
// own update_scale; the workspace's diag_r and the linear system's rx / ry / M are not read.
template <bool PC>
static int family_chunk(ScsWork *w, int K, int W, const real *B, size_t ldb, const real *Cc, size_t ldc, const real *scales,
                        ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  const int n = w->n, m = w->m, l = w->l;
  hipStream_t st = w->stream;
  const size_t nw = (size_t)n * W, mw = (size_t)m * W, lw = (size_t)l * W;
  family_ensure(w, W);
  if (PC) family_ensure_r(w, W);
  w->ls.ensure_multi(W);
  w->cone.ensure_multi(W);
  w->cone.reset_multi_cold(); // every family solve starts its eigenbases and box Newton starts cold: reruns are bit-identical
  FamilyWork &f = *w->fam;
  const real *const R = PC ? f.R.p : w->diag_r.p; // l x W block / one vector of l
  const int gl = glue_grid((long long)l * W), gnm = glue_grid((long long)(n + m) * W);
  const double t0 = now_ms();
  double t_lin = 0;
  w->cone_timer.total_ms = 0;
  w->cone_timer.samples = 0;
  const bool nrm = w->stgs.normalize != 0;
  const Reorder &ro = w->reord;
  FamCol cols[MULTI_W_MAX];

  // ---- scs_update per column (:1287-1325): renumber, norms of the data as given, normalize_b_c with the column's own sigma
  f.hblk.assign(mw, (real)0);
  f.hblk2.assign(nw, (real)0);
  f.col_y.resize(m);
  f.col_x.resize(n);
  f.col_s.resize(m);
  for (int k = 0; k < K; ++k) {
    const real *bk = B + (size_t)k * ldb, *ck = Cc + (size_t)k * ldc;
    real *b = f.col_y.data(), *c = f.col_x.data();
    for (int i = 0; i < m; ++i) b[i] = ro.active ? bk[ro.row_new2old[i]] : bk[i];
    for (int j = 0; j < n; ++j) c[j] = ro.active ? ck[ro.col_new2old[j]] : ck[j];
    real nb = 0, nc = 0;
    for (int i = 0; i < m; ++i) nb = std::max(nb, (real)std::fabs(b[i]));
    for (int j = 0; j < n; ++j) nc = std::max(nc, (real)std::fabs(c[j]));
    cols[k].nm_b_orig = nb;
    cols[k].nm_c_orig = nc;
    if (nrm) cols[k].ps = cols[k].ds = normalize_b_c_sigma(w->scal, b, c);
    for (int i = 0; i < m; ++i) f.hblk[(size_t)i * W + k] = b[i];
    for (int j = 0; j < n; ++j) f.hblk2[(size_t)j * W + k] = c[j];
  }
  f.b.upload(f.hblk.data(), mw, st);
  f.c.upload(f.hblk2.data(), nw, st);
  for (int k = 0; k < K; ++k) {
    cols[k].scale = PC && scales ? scales[k] : w->stgs.scale;
    cols[k].upd = PC;
  }
  family_upload_ctl(w, W, K, cols, PC ? 1 : 0);
  // the R of every column (padding: 1), its preconditioner and the box cone's copy of its r_y
  auto apply_scales = [&]() {
    FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_set_diag_r<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.R.p, n, m, (int)w->k.z, w->stgs.rho_x, K,
                                       f.ctl.p));
    w->ls.precond_multi_blocks(W, f.R.p, f.R.p + nw, f.Minv.p);
    w->cone.set_multi_ry(f.R.p + nw, W);
  };
  if (PC) apply_scales();
  for (int k = 0; k < K; ++k) cols[k].upd = false;
  HIP_CHECK(hipStreamSynchronize(st)); // the staging vectors are reused below

  // ---- solve_begin per column: warm / cold start (:660-687)
  f.hblk.assign(lw, (real)0);
  if (warm_start) {
    std::vector<real> hr(PC ? lw : (size_t)l); // PC: the R block, element (i, k) at i * W + k
    if (PC) f.R.download(hr.data(), lw, st);
    else w->diag_r.download(hr.data(), l, st);
    HIP_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) {
      const ScsSolution &sol = sols[k];
      if (!sol.x || !sol.y || !sol.s) continue;
      real *x = f.col_x.data(), *y = f.col_y.data(), *s = f.col_s.data();
      for (int j = 0; j < n; ++j) x[j] = ro.active ? sol.x[ro.col_new2old[j]] : sol.x[j];
      for (int i = 0; i < m; ++i) {
        y[i] = ro.active ? sol.y[ro.row_new2old[i]] : sol.y[i];
        s[i] = ro.active ? sol.s[ro.row_new2old[i]] : sol.s[i];
      }
      if (nrm) { // normalize_sol (src/normalize.c:64-76) with the column's scales
        for (int j = 0; j < n; ++j) x[j] /= (w->scal.E[j] / cols[k].ds);
        for (int i = 0; i < m; ++i) {
          y[i] /= (w->scal.D[i] / cols[k].ps);
          s[i] *= (w->scal.D[i] * cols[k].ds);
        }
      }
      for (int j = 0; j < n; ++j) f.hblk[(size_t)j * W + k] = x[j] != x[j] ? (real)0 : x[j];
      for (int i = 0; i < m; ++i) {
        const real t = y[i] + s[i] / hr[PC ? (size_t)(n + i) * W + k : (size_t)(n + i)]; // the column's own R_y
        f.hblk[(size_t)(n + i) * W + k] = t != t ? (real)0 : t;
      }
    }
  }
  for (int k = 0; k < K; ++k) f.hblk[(size_t)(l - 1) * W + k] = 1;
  f.v.upload(f.hblk.data(), lw, st);
  HIP_CHECK(hipMemsetAsync(f.u.p, 0, lw * sizeof(real), st));
  HIP_CHECK(hipMemsetAsync(f.u_t.p, 0, lw * sizeof(real), st));
  HIP_CHECK(hipMemsetAsync(f.rsk.p, 0, lw * sizeof(real), st));
  HIP_CHECK(hipMemsetAsync(f.cw.p, 0, mw * sizeof(real), st));
  HIP_CHECK(hipMemsetAsync(f.g.p, 0, (nw + mw) * sizeof(real), st));
  HIP_CHECK(hipStreamSynchronize(st));

  // ---- update_work_cache per column: g = (R + M)^-1 [c; -b] to CG_BEST_TOL (:1118-1128)
  const int *frozen = f.ctl.p->frozen;
  real tolv[MULTI_W_MAX];
  // `skip` (W ints on the device): the columns whose g stays as it is -- not one bit of theirs is read or written
  auto update_g = [&](const int *skip) {
    FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_build_g<MW>, dim3(gnm), dim3(SCSAMD_BLOCK), 0, st, f.g.p, f.c.p, f.b.p, n, m, skip));
    for (int k = 0; k < MULTI_W_MAX; ++k) tolv[k] = (real)CG_BEST_TOL;
    MultiRhs a;
    a.bx = f.g.p;
    a.by = f.g.p + nw;
    a.pre_stopped = skip;
    if (PC) a.rx = f.R.p, a.ry = f.R.p + nw, a.Minv = f.Minv.p;
    w->ls.solve_multi_blocks(K, W, a, tolv, nullptr);
  };
  update_g(frozen);

  // ---- the loop of src/scs.c:1356-1455 on blocks
  real *part = f.part.p, *nrm_part = f.part.p + (size_t)8 * PSTRIDE * W, *warm_part = f.part.p + (size_t)9 * PSTRIDE * W;
  const int max_iters = (int)w->stgs.max_iters;
  int time_limit_reached = 0, running = K, i = 0;
  bool sigint = false;
  for (; i < max_iters && running > 0; ++i) {
    const int do_norm = i >= FEASIBLE_ITERS;
    if (do_norm) FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_sumsq_partial<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, l, nrm_part, f.ctl.p));
    FAM_DISPATCH(W, hipLaunchKernelGGL((k_f_prep_linsys<MW, PC>), dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, f.u_t.p, f.u.p, f.g.p, R,
                                       f.warm.p, n, l, nrm_part, gl, warm_part, do_norm, f.ctl.p));
    { // the linear system (:763), every column on its own tolerance schedule (:745-762)
      const double tl = now_ms();
      MultiRhs a;
      a.bx = f.u_t.p;
      a.by = f.u_t.p + nw;
      a.s = f.warm.p;
      a.pre_stopped = frozen;
      if (PC) a.rx = f.R.p, a.ry = f.R.p + nw, a.Minv = f.Minv.p;
      if (w->cg_tol_override > 0) {
        for (int k = 0; k < K; ++k) tolv[k] = (real)w->cg_tol_override;
      } else {
        for (int k = 0; k < K; ++k) tolv[k] = std::min(cols[k].r_n.nm_ax_s_btau, cols[k].r_n.nm_px_aty_ctau);
        a.warm_part = warm_part;
        a.warm_cnt = gl;
        a.warm_scale = (real)1.0 / std::pow((real)i + 1, (real)CG_RATE);
      }
      w->ls.solve_multi_blocks(K, W, a, tolv, nullptr);
      t_lin += now_ms() - tl;
    }
    const int feas = i < FEASIBLE_ITERS;
    if (!feas)
      FAM_DISPATCH(W, hipLaunchKernelGGL((k_f_root_plus_partial<MW, PC>), dim3(gnm), dim3(SCSAMD_BLOCK), 0, st, f.u_t.p, f.v.p, f.g.p, R,
                                         n + m, part, PSTRIDE, f.ctl.p));
    FAM_DISPATCH(W, hipLaunchKernelGGL((k_f_post_linsys<MW, PC>), dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.u_t.p, f.u.p, f.v.p, f.g.p, R,
                                       f.cw.p, n, l, part, gnm, PSTRIDE, feas, f.ctl.p));
    int cslot = -1;
    if (w->cone_timer.used < 500) cslot = w->cone_timer.start(st);
    if (PC) w->cone.proj_primal_multi(f.cw.p, W, K, nullptr, true); // the box cone under the column's own r_y
    else w->cone.proj_primal_multi(f.cw.p, W, K, w->diag_r.p + n);
    w->cone_timer.stop(cslot, st);
    w->cone_projs++;
    const bool check = i % CONVERGED_INTERVAL == 0;
    FAM_DISPATCH(W, hipLaunchKernelGGL((k_f_post_cone<MW, PC>), dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.u.p, f.u_t.p, f.v.p, f.rsk.p, R,
                                       f.cw.p, n, l, check ? (real)0 : w->stgs.alpha, f.ctl.p));
    if (!check) continue;
    if (interrupted()) { // :1400-1403
      sigint = true;
      break;
    }
    family_residuals(w, W, K, cols, i);
    bool changed = false;
    for (int k = 0; k < K; ++k) {
      if (cols[k].frozen) continue;
      if ((cols[k].status = has_converged(cols[k].r_o, w->stgs, cols[k].nm_b_orig, cols[k].nm_c_orig)) != 0) {
        cols[k].frozen = changed = true; // like the single loop's break: the converged iteration is not counted, v is not updated
        cols[k].iter = i;
        --running;
      }
    }
    if (running == 0) {
      if (changed) family_upload_ctl(w, W, K, cols);
      break;
    }
    const bool timed_out = w->stgs.time_limit_secs && now_ms() - t0 > 1000. * w->stgs.time_limit_secs;
    // update_scale per running column, where the single loop runs it: after the convergence test, before the dual update (:1410-1412)
    bool rescaled = false;
    if (PC && w->stgs.adaptive_scale && !timed_out)
      for (int k = 0; k < K; ++k) {
        FamCol &c = cols[k];
        if (c.frozen) continue;
        real new_scale;
        if (scale_update_due(c.r_o, c.nm_b_orig, c.nm_c_orig, c.scale, i, c.sum_log_scale_factor, c.n_log_scale_factor,
                             c.last_scale_update_iter, &new_scale)) {
          c.scale_updates++;
          c.scale = new_scale;
          c.upd = rescaled = true;
        }
      }
    if (changed || rescaled) family_upload_ctl(w, W, K, cols); // one record: the pinned copy is rewritten after the next wait only
    if (timed_out) {
      time_limit_reached = 1;
      break;
    }
    if (rescaled) { // update_scale's device half for the columns in upd; of the others not one bit changes
      apply_scales();
      update_g(f.ctl.p->keep);
      FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_remap_v<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, f.rsk.p, f.R.p, f.u_t.p, f.u.p, l, f.ctl.p));
      for (int k = 0; k < K; ++k) cols[k].upd = false;
    }
    FAM_DISPATCH(W, hipLaunchKernelGGL(k_f_dual_update<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, f.u.p, f.u_t.p, l, w->stgs.alpha,
                                       f.ctl.p));
  }
  HIP_CHECK(hipStreamSynchronize(st));

  // ---- solve_end / finalize per column
  if (!sigint) {
    bool stale = false;
    for (int k = 0; k < K; ++k)
      if (!cols[k].frozen) {
        cols[k].iter = i;
        stale = stale || cols[k].r_n.last_iter != i;
      }
    if (stale) family_residuals(w, W, K, cols, i);
  }
  f.hblk.resize(lw);
  f.hblk2.resize(mw);
  f.u.download(f.hblk.data(), lw, st);
  HIP_CHECK(hipMemcpyAsync(f.hblk2.data(), f.rsk.p + nw, mw * sizeof(real), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  w->cone_timer.harvest();
  const double solve_ms = now_ms() - t0;
  const double cone_ms = w->cone_timer.samples ? w->cone_timer.total_ms * ((double)std::max(i, 1) / (double)w->cone_timer.samples) : 0.0;
  for (int k = 0; k < K; ++k) {
    ScsSolution *sol = &sols[k];
    ScsInfo *info = &infos[k];
    if (sigint && !cols[k].frozen) {
      fail_out(w, m, n, sol, info, SCS_SIGINT, "interrupted", "interrupted");
      continue;
    }
    if (!sol->x) sol->x = (real *)calloc(n, sizeof(real));
    if (!sol->y) sol->y = (real *)calloc(m, sizeof(real));
    if (!sol->s) sol->s = (real *)calloc(m, sizeof(real));
    real *x = f.col_x.data(), *y = f.col_y.data(), *s = f.col_s.data();
    for (int j = 0; j < n; ++j) x[j] = f.hblk[(size_t)j * W + k];
    for (int r = 0; r < m; ++r) {
      y[r] = f.hblk[(size_t)(n + r) * W + k];
      s[r] = f.hblk2[(size_t)r * W + k];
    }
    if (nrm) { // un_normalize_sol (src/normalize.c:78-91) with the column's scales
      for (int j = 0; j < n; ++j) x[j] *= (w->scal.E[j] / cols[k].ds);
      for (int r = 0; r < m; ++r) {
        y[r] *= (w->scal.D[r] / cols[k].ps);
        s[r] /= (w->scal.D[r] * cols[k].ds);
      }
    }
    for (int j = 0; j < n; ++j) sol->x[ro.active ? ro.col_new2old[j] : j] = x[j];
    for (int r = 0; r < m; ++r) {
      sol->y[ro.active ? ro.row_new2old[r] : r] = y[r];
      sol->s[ro.active ? ro.row_new2old[r] : r] = s[r];
    }
    memset(info, 0, sizeof *info);
    strcpy(info->lin_sys_solver, scs_get_lin_sys_method());
    info->status_val = cols[k].status;
    info->iter = cols[k].iter;
    info->setup_time = (real)w->setup_time;
    info->scale = PC ? cols[k].scale : w->stgs.scale;
    info->scale_updates = cols[k].scale_updates;
    info->aa_stats.last_aa_norm = (real)NAN;
    const LoopEnd e{max_iters, time_limit_reached, false};
    finalize_status(cols[k].r_o, n, m, e, sol, info);
    info->solve_time = (real)solve_ms;
    info->lin_sys_time = (real)t_lin;
    info->cone_time = (real)cone_ms;
    if (w->stgs.verbose) print_summary_row(cols[k].r_o, cols[k].iter, PC ? cols[k].scale : w->stgs.scale, (solve_ms + w->setup_time) / 1e3);
  }
  return sigint ? SCS_SIGINT : 0;
}

// the body of the two entries.  PC / scales: as in family_chunk; `name`: the entry, for the messages
template <bool PC>
static scs_int family_solve(const char *name, ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                            const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  if (!w || !B || !Cc || !sols || !infos || nprob < 1) {
    printf("ERROR: %s: missing ScsWork, B, Cc, ScsSolution or ScsInfo input, or nprob < 1\n", name);
    return SCS_FAILED;
  }
  if ((long long)ldb < (long long)w->m || (long long)ldc < (long long)w->n) {
    printf("ERROR: %s: ldb < m or ldc < n\n", name);
    return SCS_FAILED;
  }
  if (const char *why = family_refusal(w, PC)) {
    printf("ERROR: %s\n", why);
    return SCS_FAILED;
  }
  if (PC && scales)
    for (scs_int k = 0; k < nprob; ++k)
      if (!std::isfinite((double)scales[k]) || !(scales[k] > 0)) {
        printf("ERROR: %s: scales[%li] must be a positive finite number\n", name, (long)k);
        return SCS_FAILED;
      }
  if (w->stale) { // the last scs_amd_update_matrix failed half way
    for (scs_int k = 0; k < nprob; ++k)
      fail_out(w, w->m, w->n, &sols[k], &infos[k], SCS_FAILED, "the last scs_amd_update_matrix failed: update again before solving", "failure");
    return SCS_FAILED;
  }
  InterruptListener listener;
  scs_int done = 0; // columns already returned
  try {
    HIP_CHECK(hipSetDevice(w->device));
    if (w->stgs.verbose) print_header(w);
    bool sigint = false;
    for (; done < nprob; done += MULTI_W_MAX) { // chunks of at most 16 problems
      const int K = (int)std::min<scs_int>(MULTI_W_MAX, nprob - done);
      if (sigint) {
        for (int k = 0; k < K; ++k) fail_out(w, w->m, w->n, &sols[done + k], &infos[done + k], SCS_SIGINT, "interrupted", "interrupted");
        continue;
      }
      const int W = std::max(2, multi_width(K)); // one problem runs as a block of width 2: it stays off the single-solve state
      sigint = family_chunk<PC>(w, K, W, B + (size_t)done * (size_t)ldb, (size_t)ldb, Cc + (size_t)done * (size_t)ldc, (size_t)ldc,
                                PC && scales ? scales + done : nullptr, sols + done, infos + done, warm_start) == SCS_SIGINT;
    }
    if (w->stgs.verbose) print_rule();
  } catch (const std::exception &ex) {
    fprintf(stderr, "%s\n", ex.what());
    (void)hipStreamSynchronize(w->stream); // nothing of this call may still be reading or writing
    const std::string msg = std::string("HIP error in ") + name;
    for (scs_int k = 0; k < nprob; ++k) fail_out(w, w->m, w->n, &sols[k], &infos[k], SCS_FAILED, msg.c_str(), "failure");
    return SCS_FAILED;
  }
  return 0;
}

extern "C" {

const char *scs_amd_solve_family_refusal(const ScsWork *w) { return w ? family_refusal(w) : nullptr; }

scs_int scs_amd_solve_family(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                             ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  return family_solve<false>("scs_amd_solve_family", w, nprob, B, ldb, Cc, ldc, nullptr, sols, infos, warm_start);
}

// every column under its own scale, fixed (adaptive_scale == 0: a scale sweep) or adapted by its own update_scale
const char *scs_amd_solve_family_scaled_refusal(const ScsWork *w) { return w ? family_refusal(w, true) : nullptr; }

scs_int scs_amd_solve_family_scaled(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                    const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  return family_solve<true>("scs_amd_solve_family_scaled", w, nprob, B, ldb, Cc, ldc, scales, sols, infos, warm_start);
}

} // extern "C"
