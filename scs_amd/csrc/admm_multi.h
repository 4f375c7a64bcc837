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
// Two entries, one loop.  The loop is, on the device, the glue kernels below, each stated once with its forms as template flags, and,
// on the host, family_iterate -- the one place that launches an iteration -- with family_begin (the state of a loop, FamLoop),
// family_scale_due / family_rescale (update_scale) and family_fetch_ry / family_warm (the warm start) around it; the form of a call is
// a runtime value (FamForm) that becomes the kernels' flags where they are launched.  family_chunk and family_stream_run keep only what
// differs on purpose: how columns are loaded and returned, and when a column ends.
// scs_amd_solve_family: the columns share the workspace's diag_r (the instantiations with PERCOL = false, FamForm::own_r =
// false).  scs_amd_solve_family_scaled: column k runs under its own diag_r_k, built from its own scale, in an l x W block R whose x
// and y rows are the rx / ry blocks of the per-column block solve (MultiOp::rx / ry / Minv, linsys.h); the glue kernels read
// R[f] where the shared form reads R[f / W], in the same expressions, so equal scales give the shared form's bits.  With
// adaptive_scale the column runs update_scale (admm.hip, :1164-1241) on its own residuals where the single loop runs it -- at a
// check, after the convergence test, before the dual update.  For the columns whose scale changed (FamCtl::upd), in this order:
// their R (k_f_set_diag_r), the preconditioners (precond_multi_blocks) and the box cone's copy of r_y, their g (rebuilt and solved
// cold to CG_BEST_TOL with every other column stopped on entry), their v (k_f_remap_v).  Of a column that did not update not one
// bit is read or written by this, and a frozen column never updates.
//
// Refused: acceleration_lookback (the Anderson memory is per problem) and log_csv_filename; by scs_amd_solve_family also
// adaptive_scale (a scale update changes diag_r, which its columns share).
//
// A third entry, the same loop with a phase per column.  scs_amd_solve_family_stream takes a queue of any length through the W
// slots of ONE block: a column that has ended gives its slot to the next problem while its neighbours run on, where the two entries
// above cut the queue into chunks that each wait for their slowest column.  The schedule (part of the contract; the tests replay it):
//   * one global iteration index i = 0, 1, 2, ...; a problem that starts at global iteration s runs its local iteration j = i - s, and
//     everything the loop derives from the iteration index it derives per column from j: the feasible first iteration
//     (j < FEASIBLE_ITERS: tau = 1, u_tau = 1) and the normalisation of v (j >= FEASIBLE_ITERS) -- masks of columns in the PHASED
//     instantiations of k_f_prep_linsys / k_f_post_linsys; the warm-start term 1 / (j + 1)^CG_RATE of the CG tolerance -- one factor
//     per column (MultiRhs::warm_scale_col, k_m_rhs_prep's WS = TolArgs); the iteration passed to fill_residuals, has_converged and
//     scale_update_due; info.iter;
//   * problems 0 .. min(W, nprob) - 1 start at s = 0 in slots 0, 1, ...;
//   * a column ends at the bottom of global iteration i when j % CONVERGED_INTERVAL == 0 and its test fires (iter = j, as the chunk
//     loop freezes it), when j + 1 == max_iters (iter = max_iters; its residuals are evaluated then, for that column alone, as the
//     chunk loop evaluates them after its last iteration), or when at a check its own time limit -- counted from the moment its
//     column started running -- has passed;
//   * its result is taken out (k_f_col_out: its x, y, s in one contiguous record, not the l x W blocks) and returned at once; the
//     lowest free slot takes the next problem of the queue, in index order (k_f_col_in: its b, c, v and zeros in its u, u_t, rsk, cw,
//     warm, g; its g from family_update_g with every other column skipped; with own scales its R, preconditioner and box r_y through the
//     FamCtl::upd path of a scale update);
//   * THAT PROBLEM STARTS AT THE SMALLEST MULTIPLE OF CONVERGED_INTERVAL GREATER THAN i, so every start is a multiple of 25: all
//     running columns reach their checks in the same global iterations, one residual evaluation and one read-back serve all of
//     them, and the tests of i % 25 in the loop stay global (k_f_post_cone's alpha among them).  The price is up to 24 block
//     iterations in which the refilled slot is loaded but still frozen (it becomes a running column, frozen 1 -> 0, at the top of
//     its start iteration: one wait and one control record, at most once per 25 iterations); a check phase per slot would cost up
//     to W residual evaluations and synchronisations per 25 iterations and a per-column alpha instead;
//   * the call ends when the queue is empty and every slot is free.  Iterations in which no column runs are not executed.
// A refilled slot starts its box Newton iteration at 1 again (ConeDev::reset_multi_box_start, at its activation: while it waits its
// part of the cone block is scratch like a frozen column's).  The other cones carried here keep no state between projections, and
// PSD blocks are refused: the LDS eigensolver's warm flag is one per launch and its cold-restart counter belongs to the width.
// Every problem that passes through a stream has, bit for bit, what the entry of the same form returns for it in a call of the
// same width: the guarantee above (no dependence on neighbours or position) is what makes that an exact yardstick.
//
// A fourth entry, the scaled loop for problems that share the pattern and the cones but not the VALUES of A and P.
// scs_amd_family_set_values runs scs_init's value-dependent half once per column (scs_amd_update_matrix's code on scratch copies: the
// internal numbering, the equilibration, D_k / E_k, the box cone's bounds) and stores the equilibrated values in the linear system's
// value blocks; scs_amd_solve_family_values is family_chunk in the form {own_r, own_vals}, where the products, the preconditioner, D / E
// in the residuals, the Scaling of the host steps and the box bounds are the column's own (DCOL).  Column k is, bit for bit, column k of
// the scaled entry on a workspace brought to values k by scs_amd_update_matrix.  At most 16 problems, no stream form.
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
// PHASED (here and in k_f_post_linsys; scs_amd_solve_family_stream): the columns stand at different iterations of their own solves,
// so the flag the loop derives from the iteration index -- do_normalize here, feasible_iter there -- is a mask, bit k for column k,
// and a column whose bit equals the scalar form's flag runs the scalar form's expressions in the scalar form's order.
template <int W, bool PERCOL = false, bool PHASED = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_prep_linsys(real *v, real *u_t, const real *__restrict__ u, const real *__restrict__ g,
                                                                const real *__restrict__ R, real *warm, int n, int l, const real *nrm_part,
                                                                int nrm_cnt, real *warm_part, int do_normalize, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  const bool on = !ctl->frozen[col];
  real factor = 1;
  if (do_normalize) { // uniform over the workgroup: the reduction below synchronises it
    const real nrm = sqrt(reduce_partials_col_sum<W>(nrm_part, nrm_cnt, red));
    if (PHASED) do_normalize = (do_normalize >> col) & 1;
    if (do_normalize && nrm != (real)0) factor = sqrt((real)l) * (real)1. / nrm;
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
// PHASED: feasible_iter is a mask of the columns in their first iteration; `part` holds the dots of every running column (those of
// a column in its first iteration are not used)
template <int W, bool PERCOL = false, bool PHASED = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_post_linsys(real *u_t, real *u, const real *__restrict__ v, const real *__restrict__ g,
                                                                const real *__restrict__ R, real *cw, int n, int l, const real *part, int cnt,
                                                                int stride, int feasible_iter, const FamCtl *ctl) {
  __shared__ real red[4 * W];
  const int col = threadIdx.x & (W - 1);
  const bool on = !ctl->frozen[col];
  real tau_t = 1;
  if (PHASED || !feasible_iter) { // uniform over the workgroup: the reductions below synchronise it
    const size_t sw = (size_t)stride * W;
    const real gg = reduce_partials_col_sum<W>(part + 0 * sw, cnt, red);
    const real mug = reduce_partials_col_sum<W>(part + 1 * sw, cnt, red);
    const real pg = reduce_partials_col_sum<W>(part + 2 * sw, cnt, red);
    const real pp = reduce_partials_col_sum<W>(part + 3 * sw, cnt, red);
    const real pmu = reduce_partials_col_sum<W>(part + 4 * sw, cnt, red);
    if (PHASED) feasible_iter = (feasible_iter >> col) & 1;
    if (on && !feasible_iter) {
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

// ---- one column in, one column out (scs_amd_solve_family_stream) --------------------------------------------------------------
// The columns named in `mask` (bit k: column k) are written from a column-major staging buffer: column k's record is the
// `rec` = m + n + l values [b (m) | c (n) | v (l)] at stage + k * rec -- its normalised data and its start (warm or cold, tau row 1).
// Its u, u_t, rsk, cw, warm and g become zero, as solve_begin leaves them.  Of a column outside the mask nothing is read or written.
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_col_in(const real *__restrict__ stage, unsigned mask, real *b, real *c, real *v,
                                                           real *u, real *u_t, real *rsk, real *cw, real *warm, real *g, int n, int m) {
  const int col = threadIdx.x & (W - 1);
  if (!((mask >> col) & 1u)) return;
  const int l = n + m + 1;
  const real *sb = stage + (size_t)col * ((size_t)m + n + l), *sc = sb + m, *sv = sc + n;
  const size_t tot = (size_t)l * W, gs = (size_t)gridDim.x * blockDim.x, nw = (size_t)n * W; // gs % W == 0: a lane stays in its column
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const int i = (int)(f / W);
    v[f] = sv[i];
    u[f] = 0;
    u_t[f] = 0;
    rsk[f] = 0;
    if (i < n) {
      c[f] = sc[i];
      warm[f] = 0;
      g[f] = 0;
    } else if (i < l - 1) {
      b[f - nw] = sb[i - n];
      cw[f - nw] = 0;
      g[f] = 0;
    }
  }
}

// The result of the columns named in `mask`: column k's x and y rows of u and s rows of rsk -> the contiguous record of n + 2 m
// values [x | y | s] at out + k * (n + 2 m), which is what the host downloads of a finished column.
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_f_col_out(real *out, unsigned mask, const real *__restrict__ u, const real *__restrict__ rsk,
                                                            int n, int m) {
  const int col = threadIdx.x & (W - 1);
  if (!((mask >> col) & 1u)) return;
  real *o = out + (size_t)col * ((size_t)n + 2 * (size_t)m);
  const size_t tot = (size_t)(n + m) * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const size_t i = f / W;
    o[i] = u[f];
    if (i >= (size_t)n) o[i + m] = rsk[f];
  }
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
// DCOL (here and in k_f_resid_dual; scs_amd_solve_family_values): D / E are m x W / n x W blocks, every column its own equilibration,
// instead of one vector -- D[f] where the shared form reads D[f / W], in the same expressions.
template <int W, bool DCOL = false>
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
      const real axi = ax[f], si = s[f], bi = b[f], Di = D[DCOL ? f : f / W];
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

template <int W, bool DCOL = false>
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
      const real fo = inv_ps / E[DCOL ? f : f / W];
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
// Family state: what the family entries keep on a workspace, and nothing else reads.  Blocks at the largest width used so far (a
// narrower chunk uses the front of each buffer at its own width), allocated at the first call of any entry, freed with the workspace;
// the parts that only one form needs are allocated at that form's first call (below).
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
  DevBuf<real> R;    // l x W: [R_x rows | R_y rows | the tau row]; its x and y parts are the rx / ry blocks of MultiOp::r_rows
  DevBuf<real> Minv; // n x W: the Jacobi preconditioner of every column under its own R (precond_multi_blocks)
  // scs_amd_solve_family_stream only, allocated at its first call (family_ensure_stream): the records of k_f_col_in / k_f_col_out,
  // column k's at k * (m + n + l) / k * (n + 2 m), with their host copies, and the counters of the last stream call
  int swidth = 0;
  DevBuf<real> stage, outb;
  std::vector<real> hstage, hout;
  long long counters[6] = {0, 0, 0, 0, 0, 0};
  // scs_amd_solve_family_values only, allocated by scs_amd_family_set_values: what scs_init derives from the values, per column.
  // The equilibrated values themselves are the linear system's value blocks (MultiWork::vA ...), which nothing else can reach on a
  // ScsWork: scs_amd_linsys_set_values_multi takes a ScsLinSysWork.
  int vwidth = 0;            // width the four blocks below were allocated for (0: not allocated)
  int vcols = 0, vlayout = 0; // columns and layout width of the set call in force (0: none)
  DevBuf<real> vD, vE;       // m x W, n x W: D_k, E_k; padding columns 1
  DevBuf<real> vbl, vbu;     // the box cone's normalised bounds, column k's bsize - 1 values at k * (bsize - 1); only with a box cone
  std::vector<Scaling> vscal; // every column's D, E on the host (its primal / dual scale belongs to a solve: FamCol::ps / ds)
  void free_values() {
    vwidth = vcols = vlayout = 0;
    for (DevBuf<real> *b : {&vD, &vE, &vbl, &vbu}) b->release();
    vscal = std::vector<Scaling>();
  }
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
  // the stream entry, where the record belongs to a slot and is reset when the slot is filled: the problem of the queue the slot
  // holds (-1: none), the global iteration at which it starts (its local iteration is the global one minus this; 0 in a chunk),
  // whether it is loaded but has not started yet, how it ended, and its own clocks
  int prob = -1, start = 0;
  bool pending = false;
  int time_limit_reached = 0;
  double t0 = 0, t_lin0 = 0;
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

// the records of the stream entry at width W (W (l + 2 n + 3 m) values more: a record of m + n + l in, one of n + 2 m out, per column)
static void family_ensure_stream(ScsWork *w, int W) {
  FamilyWork &f = *w->fam;
  if (f.swidth >= W) return;
  f.swidth = 0;
  const size_t n = w->n, m = w->m, l = w->l;
  f.stage.alloc((m + n + l) * W);
  f.outb.alloc((n + 2 * m) * W);
  f.swidth = W;
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
// iter: the global iteration; column k is told its own, iter - cols[k].start.  only: the columns whose records are filled
// vc: every column under its own values and its own D / E (the blocks of scs_amd_family_set_values)
static void family_residuals(ScsWork *w, int W, int K, FamCol *cols, int iter, unsigned only = ~0u, bool vc = false) {
  FamilyWork &f = *w->fam;
  const int n = w->n, m = w->m, l = w->l;
  hipStream_t st = w->stream;
  const size_t nw = (size_t)n * W;
  const real *x = f.u.p, *y = f.u.p + nw, *s = f.rsk.p + nw;
  const real *tau_row = f.u.p + (size_t)(l - 1) * W, *kap_row = f.rsk.p + (size_t)(l - 1) * W;
  const int *frozen = f.ctl.p->frozen;
  const EpiArgs e{nullptr, nullptr, nullptr, nullptr};
  const MultiOp vals = vc ? MultiOp::of_work(*w->ls.multi, true, w->has_P) : MultiOp::shared(); // the value blocks only: no R in a residual
  w->ls.launch_spmm(W, EPI_PLAIN, w->ls.A, x, f.ax.p, e, frozen, nullptr, false, vals.vA);
  w->ls.launch_spmm(W, EPI_PLAIN, w->ls.At, y, f.aty.p, e, frozen, nullptr, false, vals.vAt);
  if (w->has_P) w->ls.launch_spmm(W, EPI_PLAIN, w->ls.P, x, f.px.p, e, frozen, nullptr, false, vals.vP);
  const int gm = glue_grid((long long)m * W), gn = glue_grid((long long)n * W);
  MULTI_DISPATCH(W, MULTI_FLAG(vc, DCOL, hipLaunchKernelGGL((k_f_resid_primal<MW, DCOL>), dim3(gm), dim3(SCSAMD_BLOCK), 0, st, f.ax.p, s, y, f.b.p,
                                                            vc ? f.vD.p : w->D.p, tau_row, m, f.part.p, PSTRIDE, f.ctl.p)));
  MULTI_DISPATCH(W, MULTI_FLAG(vc, DCOL, hipLaunchKernelGGL((k_f_resid_dual<MW, DCOL>), dim3(gn), dim3(SCSAMD_BLOCK), 0, st,
                                                            w->has_P ? f.px.p : (const real *)nullptr, f.aty.p, x, f.c.p,
                                                            vc ? f.vE.p : w->E.p, tau_row, n, f.part.p, PSTRIDE, f.ctl.p)));
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_resid_final<MW>, dim3(1), dim3(SCSAMD_BLOCK), 0, st, f.part.p, PSTRIDE, gm, gn, tau_row, kap_row,
                                       f.qout.p, f.ctl.p));
  HIP_CHECK(hipMemcpyAsync(f.hq.p, f.qout.p, (size_t)NQ * W * sizeof(real), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  w->cone_timer.harvest(); // stream is idle here
  if (w->cone.n_psd > 0) w->psd_unconverged += w->cone.take_status(st);
  for (int k = 0; k < K; ++k)
    if (!cols[k].frozen && ((only >> k) & 1u))
      fill_residuals(cols[k].r_n, cols[k].r_o, f.hq.p + k, W, iter - cols[k].start, w->has_P, w->stgs.normalize != 0, cols[k].ps, cols[k].ds);
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
  // the pinned record is rewritten only after a synchronisation of the stream (every caller has just waited on it; the stream
  // loop's activation of a loaded slot at the top of an iteration waits for exactly that)
  HIP_CHECK(hipMemcpyAsync(f.ctl.p, f.hctl.p, sizeof(FamCtl), hipMemcpyHostToDevice, w->stream));
}

// ---- the host arithmetic of one problem, shared by the chunk loop and the stream loop (staging: f.col_x / col_y / col_s) -----
// scs_update (:1287-1325): renumber, the norms of the data as given, normalize_b_c with the problem's own sigma.  Leaves b in
// f.col_y and c in f.col_x, in the internal numbering, and the problem's scales and norms in col.  sc: the D, E the problem's
// matrices were equilibrated with -- the workspace's, or the column's own (scs_amd_solve_family_values); here and in the two below.
static void family_stage_data(ScsWork *w, const Scaling &sc, const real *bk, const real *ck, FamCol &col) {
  FamilyWork &f = *w->fam;
  const int n = w->n, m = w->m;
  const Reorder &ro = w->reord;
  f.col_y.resize(m);
  f.col_x.resize(n);
  f.col_s.resize(m);
  real *b = f.col_y.data(), *c = f.col_x.data();
  for (int i = 0; i < m; ++i) b[i] = ro.active ? bk[ro.row_new2old[i]] : bk[i];
  for (int j = 0; j < n; ++j) c[j] = ro.active ? ck[ro.col_new2old[j]] : ck[j];
  real nb = 0, nc = 0;
  for (int i = 0; i < m; ++i) nb = std::max(nb, (real)std::fabs(b[i]));
  for (int j = 0; j < n; ++j) nc = std::max(nc, (real)std::fabs(c[j]));
  col.nm_b_orig = nb;
  col.nm_c_orig = nc;
  if (w->stgs.normalize) col.ps = col.ds = normalize_b_c_sigma(sc, b, c);
}

// solve_begin's warm start (:660-687): v = [x; y + s / R_y] from the caller's (x, y, s), normalised with the problem's scales.
// ry, ry_stride: the problem's own R_y, row i at ry[i * ry_stride].  Leaves the x part in f.col_x and the y part in f.col_y; false
// (nothing written) when the caller gave no start for this problem.
static bool family_stage_warm(ScsWork *w, const Scaling &sc, const ScsSolution &sol, const FamCol &col, const real *ry, size_t ry_stride) {
  if (!sol.x || !sol.y || !sol.s) return false;
  FamilyWork &f = *w->fam;
  const int n = w->n, m = w->m;
  const Reorder &ro = w->reord;
  real *x = f.col_x.data(), *y = f.col_y.data(), *s = f.col_s.data();
  for (int j = 0; j < n; ++j) x[j] = ro.active ? sol.x[ro.col_new2old[j]] : sol.x[j];
  for (int i = 0; i < m; ++i) {
    y[i] = ro.active ? sol.y[ro.row_new2old[i]] : sol.y[i];
    s[i] = ro.active ? sol.s[ro.row_new2old[i]] : sol.s[i];
  }
  if (w->stgs.normalize) normalize_sol_scaled(sc, col.ps, col.ds, x, y, s); // src/normalize.c:64-76 with the problem's scales
  for (int j = 0; j < n; ++j) x[j] = x[j] != x[j] ? (real)0 : x[j];
  for (int i = 0; i < m; ++i) {
    const real t = y[i] + s[i] / ry[(size_t)i * ry_stride];
    y[i] = t != t ? (real)0 : t;
  }
  return true;
}

// solve_end / finalize: the problem's normalised (x, y, s) in f.col_x / col_y / col_s, in the internal numbering -> sol and info
static void family_return(ScsWork *w, const Scaling &sc, const FamCol &col, bool own_scale, int time_limit_reached, double solve_ms, double lin_ms,
                          double cone_ms, ScsSolution *sol, ScsInfo *info) {
  FamilyWork &f = *w->fam;
  const int n = w->n, m = w->m;
  const Reorder &ro = w->reord;
  if (!sol->x) sol->x = (real *)calloc(n, sizeof(real));
  if (!sol->y) sol->y = (real *)calloc(m, sizeof(real));
  if (!sol->s) sol->s = (real *)calloc(m, sizeof(real));
  real *x = f.col_x.data(), *y = f.col_y.data(), *s = f.col_s.data();
  if (w->stgs.normalize) un_normalize_sol_scaled(sc, col.ps, col.ds, x, y, s); // src/normalize.c:78-91 with the problem's scales
  for (int j = 0; j < n; ++j) sol->x[ro.active ? ro.col_new2old[j] : j] = x[j];
  for (int r = 0; r < m; ++r) {
    sol->y[ro.active ? ro.row_new2old[r] : r] = y[r];
    sol->s[ro.active ? ro.row_new2old[r] : r] = s[r];
  }
  memset(info, 0, sizeof *info);
  strcpy(info->lin_sys_solver, scs_get_lin_sys_method());
  info->status_val = col.status;
  info->iter = col.iter;
  info->setup_time = (real)w->setup_time;
  info->scale = own_scale ? col.scale : w->stgs.scale;
  info->scale_updates = col.scale_updates;
  info->aa_stats.last_aa_norm = (real)NAN;
  const LoopEnd e{(int)w->stgs.max_iters, time_limit_reached, false};
  finalize_status(col.r_o, n, m, e, sol, info);
  info->solve_time = (real)solve_ms;
  info->lin_sys_time = (real)lin_ms;
  info->cone_time = (real)cone_ms;
  if (w->stgs.verbose) print_summary_row(col.r_o, col.iter, own_scale ? col.scale : w->stgs.scale, (solve_ms + w->setup_time) / 1e3);
}

// the operator of a family's block solves: with own scales the x and y rows of f.R and f.Minv, else the workspace's shared R;
// vc: under them the linear system's value blocks, every column its own A and P
static MultiOp family_op(const ScsWork *w, int W, bool own_r, bool vc = false) {
  if (!own_r) return MultiOp::shared();
  MultiOp o = vc ? MultiOp::of_work(*w->ls.multi, true, w->has_P) : MultiOp::shared();
  o.rx = w->fam->R.p, o.ry = w->fam->R.p + (size_t)w->n * W, o.Minv = w->fam->Minv.p;
  return o;
}

// the R of every column (padding: 1) from the scales of the control record, its preconditioner and the box cone's copy of its r_y
static void family_apply_scales(ScsWork *w, int W, int K, bool vc = false) {
  FamilyWork &f = *w->fam;
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_set_diag_r<MW>, dim3(glue_grid((long long)w->l * W)), dim3(SCSAMD_BLOCK), 0, w->stream, f.R.p, w->n,
                                         w->m, (int)w->k.z, w->stgs.rho_x, K, f.ctl.p));
  w->ls.precond_multi_blocks(W, family_op(w, W, true, vc), f.Minv.p);
  w->cone.set_multi_ry(f.R.p + (size_t)w->n * W, W);
}

// update_work_cache per column: g = (R + M)^-1 [c; -b] to CG_BEST_TOL (:1118-1128).  `skip` (W ints on the device): the columns
// whose g stays as it is -- not one bit of theirs is read or written
static void family_update_g(ScsWork *w, int W, int K, bool own_r, const int *skip, bool vc = false) {
  FamilyWork &f = *w->fam;
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_build_g<MW>, dim3(glue_grid((long long)(w->n + w->m) * W)), dim3(SCSAMD_BLOCK), 0, w->stream, f.g.p,
                                         f.c.p, f.b.p, w->n, w->m, skip));
  real tolv[MULTI_W_MAX];
  for (int k = 0; k < MULTI_W_MAX; ++k) tolv[k] = (real)CG_BEST_TOL;
  MultiRhs a(f.g.p, f.g.p + (size_t)w->n * W, nullptr, family_op(w, W, own_r, vc));
  a.pre_stopped = skip;
  w->ls.solve_multi_blocks(K, W, a, tolv, nullptr);
}

// ---- the form of a call, and what every entry hands to the loops after its own checks ----------------------------------------
// own_r = false: scs_amd_solve_family, the columns share the workspace's diag_r.  own_r = true: scs_amd_solve_family_scaled, column k
// runs under its own diag_r_k from scales[k] (null: the workspace's stgs.scale in every column) and, with adaptive_scale, under its
// own update_scale; the workspace's diag_r and the linear system's rx / ry / M are not read.
// own_vals (with own_r only): scs_amd_solve_family_values, column k under its own A_k and P_k as well -- the blocks of the set call in
// force (FamilyWork::vD ..., the linear system's value blocks) stand where the shared form reads the workspace's values, D, E, scal
// and box bounds, which are then not read.
// The kernels' PERCOL / DCOL arguments are these flags, made constants where a kernel is launched (MULTI_FLAG).
struct FamForm {
  bool own_r, own_vals;
};

struct FamCall {
  FamForm form;
  scs_int nprob;
  const real *B, *Cc; // column-major host data, problem p at B + p * ldb / Cc + p * ldc
  size_t ldb, ldc;
  const real *scales; // own_r: the problems' initial scales, or null
  ScsSolution *sols;
  ScsInfo *infos;
  scs_int warm_start;
  int stream; // scs_amd_solve_family_stream: the width of its block; 0: the call is cut into chunks
  int width;  // of every chunk (scs_amd_solve_family_values: the set call's layout); 0: chosen from the chunk's size
};

// ---- THE ONE LOOP: family_begin, family_iterate, family_scale_due / family_rescale, family_ry ---------------------------------
// What a chunk and a stream have in common, built once per chunk or stream by family_begin.
struct FamLoop {
  ScsWork *w;
  int W, K; // the block's width; columns in use (K .. W - 1 are padding: frozen and zero throughout)
  FamForm form;
  bool phased, adapt; // the stream: every column its own local iteration; the columns run update_scale
  const real *R;      // own_r: the l x W block; else the workspace's vector of l
  int gl, gnm;        // grids over l x W and (n + m) x W
  real *part, *nrm_part, *warm_part;
  const int *frozen; // FamCtl::frozen on the device
  FamCol cols[MULTI_W_MAX];
  double t_lin = 0;
  std::vector<real> hr; // R_y on the host, for the warm starts (family_ry)
};

static void family_begin(FamLoop &c, ScsWork *w, int W, int K, FamForm form, bool stream) {
  family_ensure(w, W);
  if (form.own_r) family_ensure_r(w, W);
  if (stream) family_ensure_stream(w, W);
  w->ls.ensure_multi(W);
  w->cone.ensure_multi(W);
  w->cone.reset_multi_cold(); // every family solve starts its eigenbases and box Newton starts cold: reruns are bit-identical
  FamilyWork &f = *w->fam;
  c.w = w, c.W = W, c.K = K, c.form = form, c.phased = stream;
  c.adapt = form.own_r && w->stgs.adaptive_scale;
  c.R = form.own_r ? f.R.p : w->diag_r.p;
  c.gl = glue_grid((long long)w->l * W), c.gnm = glue_grid((long long)(w->n + w->m) * W);
  c.part = f.part.p, c.nrm_part = f.part.p + (size_t)8 * PSTRIDE * W, c.warm_part = f.part.p + (size_t)9 * PSTRIDE * W;
  c.frozen = f.ctl.p->frozen;
  w->cone_timer.total_ms = 0;
  w->cone_timer.samples = 0;
}

// One iteration of src/scs.c:1356-1455 on the block, from the norm of v to the Moreau post of the cone step; true at a check
// (i % CONVERGED_INTERVAL == 0: v is then left to the caller's dual update).  i: the global iteration; column k stands at its local
// iteration i - cols[k].start.  What the loop derives from the iteration index -- the feasible first iteration, the normalisation
// of v, the warm-start term of the CG tolerance -- it derives per column: in a stream (phased) as masks of columns and one factor per
// column, in a chunk, whose columns all stand at i, in the scalar form of the same kernels.
static bool family_iterate(FamLoop &c, int i) {
  ScsWork *w = c.w;
  FamilyWork &f = *w->fam;
  const int W = c.W, K = c.K, n = w->n, m = w->m, l = w->l, gl = c.gl, gnm = c.gnm;
  const real *const R = c.R;
  hipStream_t st = w->stream;
  int first = 0, norm = 0; // bit k: column k runs its feasible first iteration / normalises v
  real tolv[MULTI_W_MAX], wsc[MULTI_W_MAX];
  for (int k = 0; k < MULTI_W_MAX; ++k) tolv[k] = 0, wsc[k] = 1;
  for (int k = 0; k < K; ++k) {
    if (w->cg_tol_override > 0) tolv[k] = (real)w->cg_tol_override;
    if (c.cols[k].frozen) continue;
    const int j = i - c.cols[k].start;
    (j < FEASIBLE_ITERS ? first : norm) |= 1 << k;
    if (w->cg_tol_override > 0) continue;
    tolv[k] = std::min(c.cols[k].r_n.nm_ax_s_btau, c.cols[k].r_n.nm_px_aty_ctau); // its own tolerance schedule (:745-762)
    wsc[k] = (real)1.0 / std::pow((real)j + 1, (real)CG_RATE);
  }
  if (!c.phased) first = first != 0, norm = norm != 0; // one iteration for all: do_normalize / feasible_iter as the single loop has them
  if (norm) MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_sumsq_partial<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, l, c.nrm_part, f.ctl.p));
  MULTI_DISPATCH(W, MULTI_FLAG(c.form.own_r, PERCOL, MULTI_FLAG(c.phased, PHASED,
                    hipLaunchKernelGGL((k_f_prep_linsys<MW, PERCOL, PHASED>), dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, f.u_t.p, f.u.p, f.g.p, R,
                                       f.warm.p, n, l, c.nrm_part, gl, c.warm_part, norm, f.ctl.p))));
  { // the linear system (:763)
    const double tl = now_ms();
    MultiRhs a(f.u_t.p, f.u_t.p + (size_t)n * W, f.warm.p, family_op(w, W, c.form.own_r, c.form.own_vals));
    a.pre_stopped = c.frozen;
    if (!(w->cg_tol_override > 0)) {
      a.warm_part = c.warm_part;
      a.warm_cnt = gl;
      if (c.phased) a.warm_scale_col = wsc;
      else a.warm_scale = (real)1.0 / std::pow((real)i + 1, (real)CG_RATE);
    }
    w->ls.solve_multi_blocks(K, W, a, tolv, nullptr);
    c.t_lin += now_ms() - tl;
  }
  if (norm)
    MULTI_DISPATCH(W, MULTI_FLAG(c.form.own_r, PERCOL,
                      hipLaunchKernelGGL((k_f_root_plus_partial<MW, PERCOL>), dim3(gnm), dim3(SCSAMD_BLOCK), 0, st, f.u_t.p, f.v.p, f.g.p, R,
                                         n + m, c.part, PSTRIDE, f.ctl.p)));
  MULTI_DISPATCH(W, MULTI_FLAG(c.form.own_r, PERCOL, MULTI_FLAG(c.phased, PHASED,
                    hipLaunchKernelGGL((k_f_post_linsys<MW, PERCOL, PHASED>), dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.u_t.p, f.u.p, f.v.p, f.g.p, R,
                                       f.cw.p, n, l, c.part, gnm, PSTRIDE, first, f.ctl.p))));
  int cslot = -1;
  if (w->cone_timer.used < 500) cslot = w->cone_timer.start(st);
  if (c.form.own_vals) w->cone.proj_primal_multi(f.cw.p, W, K, nullptr, true, f.vbl.p, f.vbu.p); // and between the column's own bounds
  else if (c.form.own_r) w->cone.proj_primal_multi(f.cw.p, W, K, nullptr, true); // the box cone under the column's own r_y
  else w->cone.proj_primal_multi(f.cw.p, W, K, w->diag_r.p + n);
  w->cone_timer.stop(cslot, st);
  w->cone_projs++;
  const bool check = i % CONVERGED_INTERVAL == 0; // a stream's starts are multiples of CONVERGED_INTERVAL: all columns check together
  MULTI_DISPATCH(W, MULTI_FLAG(c.form.own_r, PERCOL,
                    hipLaunchKernelGGL((k_f_post_cone<MW, PERCOL>), dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.u.p, f.u_t.p, f.v.p, f.rsk.p, R,
                                       f.cw.p, n, l, check ? (real)0 : w->stgs.alpha, f.ctl.p)));
  return check;
}

// update_scale's host half for a running column at its local iteration j (admm.hip, :1164-1241): true when its scale has changed --
// the next control record then names the column in FamCtl::upd
static bool family_scale_due(FamCol &c, int j) {
  real new_scale;
  if (!scale_update_due(c.r_o, c.nm_b_orig, c.nm_c_orig, c.scale, j, c.sum_log_scale_factor, c.n_log_scale_factor, c.last_scale_update_iter,
                        &new_scale))
    return false;
  c.scale_updates++;
  c.scale = new_scale;
  return c.upd = true;
}

// update_scale's device half for the columns in upd, after the control record that names them; of the others not one bit changes
static void family_rescale(FamLoop &c) {
  ScsWork *w = c.w;
  FamilyWork &f = *w->fam;
  family_apply_scales(w, c.W, c.K, c.form.own_vals);
  family_update_g(w, c.W, c.K, c.form.own_r, f.ctl.p->keep, c.form.own_vals);
  MULTI_DISPATCH(c.W, hipLaunchKernelGGL(k_f_remap_v<MW>, dim3(c.gl), dim3(SCSAMD_BLOCK), 0, w->stream, f.v.p, f.rsk.p, f.R.p, f.u_t.p, f.u.p,
                                         w->l, f.ctl.p));
  for (int k = 0; k < c.K; ++k) c.cols[k].upd = false;
}

// The host copy of R_y for the warm starts, after columns have been set: the R block, downloaded every time (the new columns' rows
// have just been written), or the shared diag_r, downloaded once per loop
static void family_fetch_ry(FamLoop &c) {
  ScsWork *w = c.w;
  if (!c.form.own_r && !c.hr.empty()) return;
  const size_t lw = (size_t)w->l * c.W;
  c.hr.resize(c.form.own_r ? lw : (size_t)w->l);
  if (c.form.own_r) w->fam->R.download(c.hr.data(), lw, w->stream); // element (i, k) at i * W + k
  else w->diag_r.download(c.hr.data(), w->l, w->stream);
  HIP_CHECK(hipStreamSynchronize(w->stream));
}

// solve_begin's warm start of column k from sol, under the column's own R_y (family_stage_warm)
static bool family_warm(FamLoop &c, int k, const ScsSolution &sol) {
  ScsWork *w = c.w;
  const real *ry = c.form.own_r ? c.hr.data() + (size_t)w->n * c.W + k : c.hr.data() + w->n;
  return family_stage_warm(w, c.form.own_vals ? w->fam->vscal[k] : w->scal, sol, c.cols[k], ry, c.form.own_r ? c.W : 1);
}

static scs_int family_fail_all(ScsWork *w, scs_int nprob, ScsSolution *sols, ScsInfo *infos, scs_int status_val, const char *msg,
                               const char *status) {
  for (scs_int k = 0; k < nprob; ++k) fail_out(w, w->m, w->n, &sols[k], &infos[k], status_val, msg, status);
  return status_val;
}

// Problems off .. off + K - 1 of the call (1 <= K <= W) as one block of width W.  Returns SCS_SIGINT when interrupted (the
// unfinished columns are then filled by fail_out), 0 otherwise; throws on a HIP failure.
static int family_chunk(ScsWork *w, int K, int W, const FamCall &q, scs_int off) {
  const int n = w->n, m = w->m, l = w->l;
  hipStream_t st = w->stream;
  const size_t nw = (size_t)n * W, mw = (size_t)m * W, lw = (size_t)l * W;
  const bool PC = q.form.own_r, VC = q.form.own_vals;
  FamLoop c;
  family_begin(c, w, W, K, q.form, false);
  FamilyWork &f = *w->fam;
  FamCol *cols = c.cols;
  ScsSolution *sols = q.sols + off;
  const double t0 = now_ms();

  // ---- scs_update per column (:1287-1325): renumber, norms of the data as given, normalize_b_c with the column's own sigma
  f.hblk.assign(mw, (real)0);
  f.hblk2.assign(nw, (real)0);
  for (int k = 0; k < K; ++k) {
    family_stage_data(w, VC ? f.vscal[k] : w->scal, q.B + (size_t)(off + k) * q.ldb, q.Cc + (size_t)(off + k) * q.ldc, cols[k]);
    for (int i = 0; i < m; ++i) f.hblk[(size_t)i * W + k] = f.col_y[i];
    for (int j = 0; j < n; ++j) f.hblk2[(size_t)j * W + k] = f.col_x[j];
  }
  f.b.upload(f.hblk.data(), mw, st);
  f.c.upload(f.hblk2.data(), nw, st);
  for (int k = 0; k < K; ++k) {
    cols[k].scale = PC && q.scales ? q.scales[off + k] : w->stgs.scale;
    cols[k].upd = PC;
  }
  family_upload_ctl(w, W, K, cols, PC ? 1 : 0);
  if (PC) family_apply_scales(w, W, K, VC);
  for (int k = 0; k < K; ++k) cols[k].upd = false;
  HIP_CHECK(hipStreamSynchronize(st)); // the staging vectors are reused below

  // ---- solve_begin per column: warm / cold start (:660-687)
  f.hblk.assign(lw, (real)0);
  if (q.warm_start) {
    family_fetch_ry(c);
    for (int k = 0; k < K; ++k) {
      if (!family_warm(c, k, sols[k])) continue;
      for (int j = 0; j < n; ++j) f.hblk[(size_t)j * W + k] = f.col_x[j];
      for (int i = 0; i < m; ++i) f.hblk[(size_t)(n + i) * W + k] = f.col_y[i];
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
  family_update_g(w, W, K, PC, c.frozen, VC);

  // ---- the loop of src/scs.c:1356-1455 on blocks
  const int max_iters = (int)w->stgs.max_iters;
  int time_limit_reached = 0, running = K, i = 0;
  bool sigint = false;
  for (; i < max_iters && running > 0; ++i) {
    if (!family_iterate(c, i)) continue;
    if (interrupted()) { // :1400-1403
      sigint = true;
      break;
    }
    family_residuals(w, W, K, cols, i, ~0u, VC);
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
    if (c.adapt && !timed_out)
      for (int k = 0; k < K; ++k)
        if (!cols[k].frozen && family_scale_due(cols[k], i)) rescaled = true;
    if (changed || rescaled) family_upload_ctl(w, W, K, cols); // one record: the pinned copy is rewritten after the next wait only
    if (timed_out) {
      time_limit_reached = 1;
      break;
    }
    if (rescaled) family_rescale(c);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_dual_update<MW>, dim3(c.gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, f.u.p, f.u_t.p, l, w->stgs.alpha,
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
    if (stale) family_residuals(w, W, K, cols, i, ~0u, VC);
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
    ScsInfo *info = &q.infos[off + k];
    if (sigint && !cols[k].frozen) {
      fail_out(w, m, n, &sols[k], info, SCS_SIGINT, "interrupted", "interrupted");
      continue;
    }
    real *x = f.col_x.data(), *y = f.col_y.data(), *s = f.col_s.data();
    for (int j = 0; j < n; ++j) x[j] = f.hblk[(size_t)j * W + k];
    for (int r = 0; r < m; ++r) {
      y[r] = f.hblk[(size_t)(n + r) * W + k];
      s[r] = f.hblk2[(size_t)r * W + k];
    }
    family_return(w, VC ? f.vscal[k] : w->scal, cols[k], PC, time_limit_reached, solve_ms, c.t_lin, cone_ms, &sols[k], info);
  }
  return sigint ? SCS_SIGINT : 0;
}

// ============================================================================
// scs_amd_solve_family_stream: a queue of problems through the W slots of one block (the schedule: the header comment)
// ============================================================================
static const char *family_stream_refusal(const ScsWork *w, bool own_scale) {
  if (const char *why = family_refusal(w, own_scale)) return why;
  if (w->k.ssize + w->k.cssize > 0)
    return "scs_amd_solve_family_stream requires cones without PSD blocks (ssize + cssize == 0): the warm start and the cold-restart counter of "
           "the LDS eigensolver belong to the width, not to a slot; use scs_amd_solve_family or scs_amd_solve_family_scaled";
  return nullptr;
}

// The queue q through the q.stream slots of one block: the schedule around family_iterate.  returned[p] != 0: problem p has its
// result in q.sols[p] / q.infos[p].  Throws on a HIP failure; true when interrupted (the problems not yet returned are then left to
// the caller).
static bool family_stream_run(ScsWork *w, const FamCall &q, std::vector<char> &returned) {
  const int n = w->n, m = w->m, l = w->l, W = q.stream, nprob = (int)q.nprob;
  hipStream_t st = w->stream;
  const bool PC = q.form.own_r;
  const int K = std::min(W, nprob); // slots in use
  FamLoop lp;
  family_begin(lp, w, W, K, q.form, true);
  FamilyWork &f = *w->fam;
  long long *cnt = f.counters;
  for (int t = 0; t < 6; ++t) cnt[t] = 0;
  cnt[5] = W;
  const int gl = lp.gl, gnm = lp.gnm;
  const size_t rec_in = (size_t)m + n + l, rec_out = (size_t)n + 2 * (size_t)m;
  f.hstage.assign(rec_in * W, (real)0);
  f.hout.assign(rec_out * W, (real)0);
  FamCol *cols = lp.cols;
  for (int k = 0; k < MULTI_W_MAX; ++k) cols[k].frozen = true; // an empty slot
  const int max_iters = (int)w->stgs.max_iters;
  int next = 0, busy = 0, running = 0; // the queue's head; slots that hold a problem; slots whose column runs

  // The lowest free slots take the next problems of the queue, which start at global iteration `start`.  The stream is idle on
  // entry (the control record is rewritten) and has been waited on after the staging upload on return (family_update_g waits).
  auto fill = [&](int start, bool first) {
    unsigned mask = 0;
    for (int k = 0; k < K && next < nprob; ++k) {
      if (cols[k].prob >= 0) continue;
      FamCol &c = cols[k] = FamCol();
      c.prob = next++;
      c.start = start;
      c.frozen = c.pending = !first; // the first columns run from iteration 0: nothing to wait for
      c.upd = true;                  // its R (PC) and its g are built below, with every other column left as it is
      c.scale = PC && q.scales ? q.scales[c.prob] : w->stgs.scale;
      family_stage_data(w, w->scal, q.B + (size_t)c.prob * q.ldb, q.Cc + (size_t)c.prob * q.ldc, c);
      real *rec = f.hstage.data() + (size_t)k * rec_in;
      std::copy(f.col_y.begin(), f.col_y.end(), rec);
      std::copy(f.col_x.begin(), f.col_x.end(), rec + m);
      std::fill(rec + m + n, rec + rec_in, (real)0);
      rec[rec_in - 1] = 1; // the tau row of v
      mask |= 1u << k;
      ++busy;
      if (first) {
        ++running;
        c.t0 = now_ms();
      } else {
        ++cnt[3];
      }
    }
    if (!mask) return;
    family_upload_ctl(w, W, K, cols, first && PC ? 1 : 0);
    if (PC) family_apply_scales(w, W, K);
    if (q.warm_start) { // solve_begin per problem, under its own R_y
      family_fetch_ry(lp);
      for (int k = 0; k < K; ++k) {
        if (!((mask >> k) & 1u)) continue;
        if (!family_warm(lp, k, q.sols[cols[k].prob])) continue;
        real *v = f.hstage.data() + (size_t)k * rec_in + m + n;
        std::copy(f.col_x.begin(), f.col_x.end(), v);
        std::copy(f.col_y.begin(), f.col_y.end(), v + n);
      }
    }
    for (int k = 0; k < K; ++k)
      if ((mask >> k) & 1u) HIP_CHECK(hipMemcpyAsync(f.stage.p + (size_t)k * rec_in, f.hstage.data() + (size_t)k * rec_in, rec_in * sizeof(real),
                                                     hipMemcpyHostToDevice, st));
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_col_in<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.stage.p, mask, f.b.p, f.c.p, f.v.p, f.u.p,
                                         f.u_t.p, f.rsk.p, f.cw.p, f.warm.p, f.g.p, n, m));
    family_update_g(w, W, K, PC, first ? lp.frozen : f.ctl.p->keep); // update_work_cache for the new columns alone (:1118-1128)
    for (int k = 0; k < K; ++k) cols[k].upd = false;
  };

  // The columns in `mask` have ended: their (x, y, s) out of the blocks, their results to the caller, their slots free.
  auto take_out = [&](unsigned mask) {
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_col_out<MW>, dim3(gnm), dim3(SCSAMD_BLOCK), 0, st, f.outb.p, mask, f.u.p, f.rsk.p, n, m));
    for (int k = 0; k < K; ++k)
      if ((mask >> k) & 1u) HIP_CHECK(hipMemcpyAsync(f.hout.data() + (size_t)k * rec_out, f.outb.p + (size_t)k * rec_out, rec_out * sizeof(real),
                                                     hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    w->cone_timer.harvest();
    const double t1 = now_ms();
    const double cone_iter_ms = w->cone_timer.samples ? w->cone_timer.total_ms / (double)w->cone_timer.samples : 0.0; // sampled mean
    for (int k = 0; k < K; ++k) {
      if (!((mask >> k) & 1u)) continue;
      FamCol &c = cols[k];
      const real *rec = f.hout.data() + (size_t)k * rec_out;
      std::copy(rec, rec + n, f.col_x.begin());
      std::copy(rec + n, rec + n + m, f.col_y.begin());
      std::copy(rec + n + m, rec + rec_out, f.col_s.begin());
      family_return(w, w->scal, c, PC, c.time_limit_reached, t1 - c.t0, lp.t_lin - c.t_lin0, cone_iter_ms * std::max(c.iter, 1),
                    &q.sols[c.prob], &q.infos[c.prob]);
      returned[c.prob] = 1;
      c.prob = -1;
      --busy;
    }
  };

  fill(0, true);
  bool sigint = false;
  int i = 0, last = -1;
  for (;; ++i) {
    { // a loaded slot becomes a running column at the top of its start iteration: one wait, one control record
      bool due = false;
      for (int k = 0; k < K; ++k) due = due || (cols[k].pending && cols[k].start == i);
      if (due) {
        HIP_CHECK(hipStreamSynchronize(st));
        for (int k = 0; k < K; ++k) {
          FamCol &c = cols[k];
          if (!c.pending || c.start != i) continue;
          c.pending = c.frozen = false;
          c.t0 = now_ms();
          c.t_lin0 = lp.t_lin;
          w->cone.reset_multi_box_start(k); // the slot projected scratch while it waited
          ++running;
        }
        family_upload_ctl(w, W, K, cols);
      }
    }
    if (running == 0) {
      if (busy == 0) break; // the queue is empty and every slot is free
      int s = 2147483647;
      for (int k = 0; k < K; ++k)
        if (cols[k].pending) s = std::min(s, cols[k].start);
      i = s - 1; // nothing runs until then
      continue;
    }
    last = i;
    cnt[1] += running;
    unsigned ended = 0;
    if (family_iterate(lp, i)) {
      if (interrupted()) {
        sigint = true;
        break;
      }
      family_residuals(w, W, K, cols, i);
      ++cnt[4];
      bool changed = false, rescaled = false;
      const double tnow = now_ms();
      for (int k = 0; k < K; ++k) {
        FamCol &c = cols[k];
        if (c.frozen) continue;
        c.status = has_converged(c.r_o, w->stgs, c.nm_b_orig, c.nm_c_orig);
        if (c.status == 0 && w->stgs.time_limit_secs && tnow - c.t0 > 1000. * w->stgs.time_limit_secs) c.time_limit_reached = 1;
        if (c.status != 0 || c.time_limit_reached) { // as the chunk loop's break: the iteration is not counted, v is not updated
          c.frozen = changed = true;
          c.iter = i - c.start;
          ended |= 1u << k;
          --running;
        } else if (lp.adapt && family_scale_due(c, i - c.start)) {
          rescaled = true;
        }
      }
      if (changed || rescaled) family_upload_ctl(w, W, K, cols); // the stream has been waited on and nothing has been enqueued since
      if (rescaled) family_rescale(lp);
      if (running > 0)
        MULTI_DISPATCH(W, hipLaunchKernelGGL(k_f_dual_update<MW>, dim3(gl), dim3(SCSAMD_BLOCK), 0, st, f.v.p, f.u.p, f.u_t.p, l, w->stgs.alpha,
                                             f.ctl.p));
    }
    unsigned capped = 0; // the column's last iteration: its residuals as they stand after it, as the chunk loop's after its last
    for (int k = 0; k < K; ++k)
      if (!cols[k].frozen && i - cols[k].start + 1 == max_iters) capped |= 1u << k;
    if (capped) {
      family_residuals(w, W, K, cols, i + 1, capped);
      ++cnt[4];
      for (int k = 0; k < K; ++k)
        if ((capped >> k) & 1u) {
          cols[k].frozen = true;
          cols[k].iter = max_iters;
          --running;
        }
      family_upload_ctl(w, W, K, cols);
      ended |= capped;
    }
    if (ended) {
      take_out(ended);
      fill((i / CONVERGED_INTERVAL + 1) * CONVERGED_INTERVAL, false);
    }
  }
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipGetLastError());
  w->cone_timer.harvest();
  cnt[0] = last + 1;
  cnt[2] = cnt[0] * W - cnt[1];
  return sigint;
}

// ============================================================================
// the entries: every one its own checks, messages and record of a refusal, then family_run
// ============================================================================
// the first of the scales that is not a positive finite number, or -1 (none given: -1)
static scs_int family_bad_scale(const scs_float *scales, scs_int nprob) {
  for (scs_int k = 0; scales && k < nprob; ++k)
    if (!std::isfinite((double)scales[k]) || !(scales[k] > 0)) return k;
  return -1;
}

static scs_int family_fail_stale(ScsWork *w, const FamCall &q) { // the last scs_amd_update_matrix failed half way
  return family_fail_all(w, q.nprob, q.sols, q.infos, SCS_FAILED, "the last scs_amd_update_matrix failed: update again before solving", "failure");
}

// A checked call of the entry `name`: the queue through a stream, or cut into chunks of at most 16 problems.  A HIP failure fails
// every problem of the call; an interrupt fails the problems that have not been returned.
static scs_int family_run(const char *name, ScsWork *w, const FamCall &q) {
  InterruptListener listener;
  std::vector<char> returned(q.stream ? (size_t)q.nprob : 0, 0);
  try {
    HIP_CHECK(hipSetDevice(w->device));
    if (w->stgs.verbose) print_header(w);
    if (q.stream) {
      if (family_stream_run(w, q, returned)) {
        (void)hipStreamSynchronize(w->stream);
        for (scs_int k = 0; k < q.nprob; ++k)
          if (!returned[k]) fail_out(w, w->m, w->n, &q.sols[k], &q.infos[k], SCS_SIGINT, "interrupted", "interrupted");
      }
    } else {
      bool sigint = false;
      for (scs_int done = 0; done < q.nprob; done += MULTI_W_MAX) { // done: problems already returned
        const int K = (int)std::min<scs_int>(MULTI_W_MAX, q.nprob - done);
        const int W = q.width ? q.width : std::max(2, multi_width(K)); // one problem runs as a block of width 2: it stays off the single-solve state
        if (sigint) family_fail_all(w, K, q.sols + done, q.infos + done, SCS_SIGINT, "interrupted", "interrupted");
        else sigint = family_chunk(w, K, W, q, done) == SCS_SIGINT;
      }
    }
    if (w->stgs.verbose) print_rule();
  } catch (const std::exception &ex) {
    fprintf(stderr, "%s\n", ex.what());
    (void)hipStreamSynchronize(w->stream); // nothing of this call may still be reading or writing
    const std::string msg = std::string("HIP error in ") + name;
    return family_fail_all(w, q.nprob, q.sols, q.infos, SCS_FAILED, msg.c_str(), "failure");
  }
  return 0;
}

// the body of scs_amd_solve_family and scs_amd_solve_family_scaled; `name`: the entry, for the messages
static scs_int family_solve(const char *name, bool own_r, ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc,
                            scs_int ldc, const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  if (!w || !B || !Cc || !sols || !infos || nprob < 1) {
    printf("ERROR: %s: missing ScsWork, B, Cc, ScsSolution or ScsInfo input, or nprob < 1\n", name);
    return SCS_FAILED;
  }
  if ((long long)ldb < (long long)w->m || (long long)ldc < (long long)w->n) {
    printf("ERROR: %s: ldb < m or ldc < n\n", name);
    return SCS_FAILED;
  }
  if (const char *why = family_refusal(w, own_r)) {
    printf("ERROR: %s\n", why);
    return SCS_FAILED;
  }
  if (!own_r) scales = nullptr;
  if (const scs_int k = family_bad_scale(scales, nprob); k >= 0) {
    printf("ERROR: %s: scales[%li] must be a positive finite number\n", name, (long)k);
    return SCS_FAILED;
  }
  const FamCall q{{own_r, false}, nprob, B, Cc, (size_t)ldb, (size_t)ldc, scales, sols, infos, warm_start, 0, 0};
  if (w->stale) return family_fail_stale(w, q);
  return family_run(name, w, q);
}

extern "C" scs_int scs_amd_solve_family_stream(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                               scs_int own_scale, const scs_float *scales, scs_int width, ScsSolution *sols, ScsInfo *infos,
                                               scs_int warm_start) {
  const char *name = "scs_amd_solve_family_stream";
  if (!w || !B || !Cc || !sols || !infos || nprob < 1) {
    printf("ERROR: %s: missing ScsWork, B, Cc, ScsSolution or ScsInfo input, or nprob < 1\n", name);
    return SCS_FAILED;
  }
  if (width != 0 && width != 2 && width != 4 && width != 8 && width != 16) { // before the workspace is looked at
    printf("ERROR: %s: width must be 0 (chosen from nprob), 2, 4, 8 or 16\n", name);
    return SCS_FAILED;
  }
  w->stream_arg_refusal = nullptr;
  auto refuse = [&](const char *why) {
    w->stream_arg_refusal = why;
    printf("ERROR: %s\n", why);
    return (scs_int)SCS_FAILED;
  };
  if ((long long)ldb < (long long)w->m || (long long)ldc < (long long)w->n) return refuse("scs_amd_solve_family_stream: ldb < m or ldc < n");
  if (const char *why = family_stream_refusal(w, own_scale != 0)) {
    printf("ERROR: %s\n", why);
    return SCS_FAILED;
  }
  if (!own_scale && scales)
    return refuse("scs_amd_solve_family_stream: scales must be NULL with own_scale == 0: the problems then share the workspace's scale");
  if (family_bad_scale(scales, nprob) >= 0) return refuse("scs_amd_solve_family_stream: every one of the scales must be a positive finite number");
  const int W = width ? (int)width : std::max(2, multi_width(std::min<scs_int>(nprob, MULTI_W_MAX)));
  const FamCall q{{own_scale != 0, false}, nprob, B, Cc, (size_t)ldb, (size_t)ldc, scales, sols, infos, warm_start, W, 0};
  if (w->stale) return family_fail_stale(w, q);
  if ((long long)nprob > 2147483647LL) return refuse("scs_amd_solve_family_stream: nprob exceeds 2^31 - 1");
  return family_run(name, w, q);
}

// ============================================================================
// scs_amd_family_set_values / scs_amd_solve_family_values: a family that shares the pattern and the cones but not the values of A, P
// ============================================================================
// The set call is scs_init's value-dependent half per column, on scratch copies of the host matrices: values into the internal
// numbering and equilibration exactly as scs_amd_update_matrix takes them, so column k's D_k, E_k and equilibrated values are, bit
// for bit, those of a workspace brought to values k.  The solve call is one chunk in the form {own_r, own_vals}: the loop of the scaled
// entry with every input that follows the values -- the products, the preconditioner, D / E in the residuals, the Scaling of the host steps, the
// box cone's bounds -- taken from the column's own.  Nothing of the workspace's own problem is read for a column or written.
static scs_int family_values_refuse(ScsWork *w, const char *why) {
  if (w) w->values_arg_refusal = why;
  printf("ERROR: %s\n", why);
  return SCS_FAILED;
}

extern "C" scs_int scs_amd_family_set_values(ScsWork *w, scs_int nprob, const scs_float *AX, scs_int ldax, const scs_float *PX, scs_int ldpx) {
  if (!w || !AX) return family_values_refuse(w, "scs_amd_family_set_values: w and AX must be given");
  w->values_arg_refusal = nullptr;
  if (const char *why = family_refusal(w, true)) {
    printf("ERROR: %s\n", why);
    return SCS_FAILED;
  }
  if ((PX != nullptr) != w->has_P) return family_values_refuse(w, "scs_amd_family_set_values: PX must be given exactly when the workspace has a P");
  if (nprob < 1 || nprob > MULTI_W_MAX) return family_values_refuse(w, "scs_amd_family_set_values: nprob must be 1 .. 16 (set and solve in groups)");
  const size_t nzA = w->A.x.size(), nzP = w->has_P ? w->P.x.size() : 0;
  if ((long long)ldax < (long long)nzA || (PX && (long long)ldpx < (long long)nzP))
    return family_values_refuse(w, "scs_amd_family_set_values: a leading dimension is shorter than its column");
  for (scs_int k = 0; k < nprob; ++k)
    if (!all_finite(AX + (size_t)k * (size_t)ldax, nzA) || (PX && !all_finite(PX + (size_t)k * (size_t)ldpx, nzP)))
      return family_values_refuse(w, "scs_amd_family_set_values: a matrix value is not finite");
  if (w->stale) return family_values_refuse(w, "scs_amd_family_set_values: the last scs_amd_update_matrix failed: update again first");
  if (w->ls.shard) return family_values_refuse(w, "scs_amd_family_set_values: a row-sharded workspace takes no values per column");
  const int K = (int)nprob, W = std::max(2, multi_width(K)), n = w->n, m = w->m;
  const int nb = w->k.bsize > 1 ? (int)w->k.bsize - 1 : 0; // bounds of the box cone
  try {
    HIP_CHECK(hipSetDevice(w->device));
    if (!w->fam) w->fam = new FamilyWork();
    FamilyWork &f = *w->fam;
    f.vcols = 0; // a failure below leaves no set in force
    if (f.vwidth < W) {
      f.free_values();
      f.vD.alloc((size_t)m * W);
      f.vE.alloc((size_t)n * W);
      if (nb) {
        f.vbl.alloc((size_t)nb * W);
        f.vbu.alloc((size_t)nb * W);
      }
      f.vwidth = W;
    }
    f.vscal.assign((size_t)K, Scaling());
    const bool norm = w->stgs.normalize != 0;
    HostCsc A2 = w->A, P2; // scratch: the workspace's own copies, D, E and scal stay as they are
    if (w->has_P) P2 = w->P;
    std::vector<real> ax(nzA * K), px(nzP * K), hD((size_t)m * W, (real)1), hE((size_t)n * W, (real)1), hbl((size_t)nb * W, (real)0),
        hbu((size_t)nb * W, (real)0);
    for (int k = 0; k < K; ++k) {
      const real *a = AX + (size_t)k * (size_t)ldax, *p = PX ? PX + (size_t)k * (size_t)ldpx : nullptr;
      if (norm && w->has_P) { // as scs_amd_update_matrix: P switches the renumbering off, the caller's order is the internal one
        std::copy(a, a + nzA, A2.x.begin());
        std::copy(p, p + nzP, P2.x.begin());
      } else {
        permute_values(w->reord, a, nzA, A2.x.data());
        if (p) std::copy(p, p + nzP, P2.x.begin());
      }
      Scaling &sc = f.vscal[k];
      if (norm) {
        if (w->dev_eq) equilibrate_dev(w->has_P ? &P2 : nullptr, A2, &w->k, sc, w->stream, nullptr);
        else equilibrate(w->has_P ? &P2 : nullptr, A2, &w->k, sc);
      } else {
        sc.D.assign(m, (real)1);
        sc.E.assign(n, (real)1);
      }
      std::copy(A2.x.begin(), A2.x.end(), ax.begin() + (size_t)k * nzA);
      if (w->has_P) std::copy(P2.x.begin(), P2.x.end(), px.begin() + (size_t)k * nzP);
      for (int i = 0; i < m; ++i) hD[(size_t)i * W + k] = sc.D[i];
      for (int j = 0; j < n; ++j) hE[(size_t)j * W + k] = sc.E[j];
      if (nb) ConeDev::box_bounds_host(&w->k, norm ? sc.D.data() + w->cone.box_off : nullptr, hbl.data() + (size_t)k * nb, hbu.data() + (size_t)k * nb);
    }
    w->ls.set_multi_values(K, W, ax.data(), nzA, w->has_P ? px.data() : nullptr, nzP);
    f.vD.upload(hD.data(), hD.size(), w->stream);
    f.vE.upload(hE.data(), hE.size(), w->stream);
    if (nb) {
      f.vbl.upload(hbl.data(), hbl.size(), w->stream);
      f.vbu.upload(hbu.data(), hbu.size(), w->stream);
    }
    HIP_CHECK(hipStreamSynchronize(w->stream)); // the host blocks end here; the call returns with the stream idle
    f.vcols = K;
    f.vlayout = W;
  } catch (const std::exception &ex) {
    fprintf(stderr, "%s\n", ex.what());
    (void)hipStreamSynchronize(w->stream);
    if (w->fam) w->fam->free_values(); // the workspace stays usable, with no values set
    w->ls.free_multi_values();
    return family_values_refuse(w, "scs_amd_family_set_values: HIP error or failed allocation: no values are set");
  }
  return 0;
}

extern "C" {

scs_int scs_amd_solve_family_values(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                    const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  if (!w || !B || !Cc || !sols || !infos)
    return family_values_refuse(w, "scs_amd_solve_family_values: missing ScsWork, B, Cc, ScsSolution or ScsInfo input");
  w->values_arg_refusal = nullptr;
  if (const char *why = family_refusal(w, true)) {
    printf("ERROR: %s\n", why);
    return SCS_FAILED;
  }
  if (nprob < 1 || nprob > MULTI_W_MAX) return family_values_refuse(w, "scs_amd_solve_family_values: nprob must be 1 .. 16 (set and solve in groups)");
  if ((long long)ldb < (long long)w->m || (long long)ldc < (long long)w->n) return family_values_refuse(w, "scs_amd_solve_family_values: ldb < m or ldc < n");
  if (family_bad_scale(scales, nprob) >= 0)
    return family_values_refuse(w, "scs_amd_solve_family_values: every one of the scales must be a positive finite number");
  if (w->stale) return family_values_refuse(w, "scs_amd_solve_family_values: the last scs_amd_update_matrix failed: update again before solving");
  const FamilyWork *fv = w->fam;
  if (!fv || fv->vcols == 0 || !w->ls.multi || w->ls.multi->vcols != fv->vcols)
    return family_values_refuse(w, "scs_amd_solve_family_values: no values are set (scs_amd_family_set_values)");
  if (fv->vcols != (int)nprob) return family_values_refuse(w, "scs_amd_solve_family_values: nprob differs from the set call's");
  return family_run("scs_amd_solve_family_values", w,
                    FamCall{{true, true}, nprob, B, Cc, (size_t)ldb, (size_t)ldc, scales, sols, infos, warm_start, 0, fv->vlayout});
}

void scs_amd_family_free_values(ScsWork *w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  (void)hipStreamSynchronize(w->stream);
  if (w->fam) w->fam->free_values();
  w->ls.free_multi_values();
}

// host only: the normalised bounds scs_init and the set call keep for a box cone whose rows are scaled by Db (bsize values; NULL:
// the bounds as given, the normalize == 0 case) -- bl / bu receive bsize - 1 values each
scs_int scs_amd_box_bounds(const ScsCone *k, const scs_float *Db, scs_float *bl, scs_float *bu) {
  if (!k || k->bsize < 1 || (k->bsize > 1 && (!k->bl || !k->bu || !bl || !bu))) return -1;
  ConeDev::box_bounds_host(k, Db, bl, bu);
  return 0;
}

// the setting the two entries refuse, else the arguments the last call of either was refused for (until a call is accepted)
const char *scs_amd_solve_family_values_refusal(const ScsWork *w) {
  if (!w) return nullptr;
  if (const char *why = family_refusal(w, true)) return why;
  return w->values_arg_refusal;
}

const char *scs_amd_solve_family_stream_refusal(const ScsWork *w, scs_int own_scale) {
  if (!w) return nullptr;
  if (const char *why = family_stream_refusal(w, own_scale != 0)) return why;
  return w->stream_arg_refusal; // the arguments the last call was refused for, until a call is accepted
}

void scs_amd_family_stream_get_counters(const ScsWork *w, long long out[6]) {
  for (int q = 0; q < 6; ++q) out[q] = w && w->fam ? w->fam->counters[q] : 0;
}

const char *scs_amd_solve_family_refusal(const ScsWork *w) { return w ? family_refusal(w) : nullptr; }

scs_int scs_amd_solve_family(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                             ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  return family_solve("scs_amd_solve_family", false, w, nprob, B, ldb, Cc, ldc, nullptr, sols, infos, warm_start);
}

// every column under its own scale, fixed (adaptive_scale == 0: a scale sweep) or adapted by its own update_scale
const char *scs_amd_solve_family_scaled_refusal(const ScsWork *w) { return w ? family_refusal(w, true) : nullptr; }

scs_int scs_amd_solve_family_scaled(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                    const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  return family_solve("scs_amd_solve_family_scaled", true, w, nprob, B, ldb, Cc, ldc, scales, sols, infos, warm_start);
}

} // extern "C"
