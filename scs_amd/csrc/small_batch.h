// small_batch.h -- scs_amd_small_*: a batch of SMALL problems that share A, P, the cone and the settings, every problem solved
// from its first iteration to its convergence test inside ONE kernel by ONE workgroup, its whole state in LDS.
// Included at the end of admm.hip: the host side turns the kernel's reduced scalars into ScsInfo with the functions finalize uses
// (fill_residuals, finalize_status), and refuses with the validation of scs_init.
//
// The iteration is the loop of src/scs.c:1356-1455 with adaptive_scale = 0 and acceleration_lookback = 0, the steps in the order
// of solve_steps above.  What differs from the single solve is the linear system: the scale never changes, so the reduced matrix
//   H = R_x + P + A' R_y^-1 A      (n x n, dense, n <= SB_MAX_N)
// is assembled and factored once at init (Cholesky in long double on the host) and every solve is exact:
//   x = H^-1 (r_x + A' R_y^-1 r_y),  y = R_y^-1 (A x - r_y)        (the elimination of linsys/cpu/indirect/private.c)
// with H^-1 applied as a dense product and one step of refinement against the KKT operator [R_x + P, A'; A, -R_y] (lin_solve
// below): no chain of n dependent steps, and the cond(H) eps that a dense inverse loses is repaired (tests/test_small_batch_gpu.py,
// the ill-conditioned case: refinement against H itself, whose residual carries an error of |H| |x| eps, does not repair it).
// A and A' are read in padded-row (ELL) form, entry k of all rows adjacent, so a workgroup's lanes read consecutive addresses; the
// matrices are shared by all workgroups and stay in L2.
//
// Determinism: a workgroup owns a problem; every sum is taken in an order fixed by (n, m, the pattern, the block size) alone -- per-thread partial
// sums over a fixed index range, combined by wave shuffles and a fixed loop over the workgroup's waves.  No floating-point atomics.  The
// only atomic is the integer counter problems are taken from, so a problem's bits depend neither on the grid, on nprob, on its
// index nor on its neighbours.  Every loop is bounded by max_iters, n, m, the row widths or the cone sizes.
//
// scs_amd_small_set_values / scs_amd_small_solve_values: the same batch with every problem's OWN values of A and P on the pattern
// of init.  The host equilibrates every problem and writes its values into the problem's own padded rows and dense P; H is then
// per problem, and the problem's workgroup assembles, factors and inverts it in working precision before the first iteration
// (sb_factor, k_small_batch<true, .>).  k_small_batch<false, .> is the shared kernel, unchanged.
//
// The host half (from struct ScsAmdSmall down) says each thing once.  small_kernel names the four instantiations, and the occupancy
// query and the launch both take the kernel from it; small_grid_default is the default grid of either entry's kernel; small_ry is
// the host's R_y of a row and small_equilibrate a problem's D, E (the identity with normalize = 0), for init and the set call alike;
// the kernel's argument is filled once, by small_device_init, with what is the object's, and a launch sets what is the chunk's.
// small_solve is a frame -- the listener, the try / catch, the chunk loop with SIGINT between launches, the counters -- around
// small_solve_accepts (the checks, arguments before state), small_stage (one problem's scs_update and warm start), small_launch
// and small_return (one problem's finalize).  (Un)normalisation with a problem's own sigma is normalize_sol_scaled /
// un_normalize_sol_scaled of equilibrate.cpp, as in the family solve.  The SIGINT path and the catch path have no test: they were
// kept by reading.
#include <cstdarg>
#include <memory>
#include <type_traits>

namespace scsamd {

// Two instantiations of one kernel.  NARROW: 4 waves, one per SIMD, two workgroups per CU; n <= SB_NARROW_N and
// n + m + 1 <= SB_NARROW_L.  WIDE: 16 waves, four per SIMD, one workgroup with the whole LDS of its CU; every other accepted size.
constexpr int SB_BLOCK = 256, SB_BLOCK_WIDE = 1024;
constexpr int SB_NARROW_N = 128, SB_NARROW_L = 1024;
constexpr int SB_MAX_N = 512;   // H, H^-1 and P are dense n x n; one thread per entry of an n-vector and two per dense output
constexpr int SB_MAX_L = 2304;  // n + m + 1: 6 l + 2 m + 3 n + BLOCK + 16 values of LDS, 159 856 B of the CU's 160 KiB at (512, 1791)
constexpr int SB_QS = NQ;       // stride of a problem's reduced scalars (Q_* above)
constexpr int SB_CHUNK = 32768; // problems per launch: SIGINT is looked at between launches
constexpr int SB_SERIAL_Q = 16; // second-order cones up to this size are projected by one thread, larger ones by one wave

struct SbArgs {
  int n, m, l, z, nl, qsize, has_P, normalize, max_iters, wA, wAt, nprob, warm;
  real rho_x, scale, alpha, eps_abs, eps_rel, eps_infeas;
  const real *Av, *Atv, *Hinv, *Pd, *D, *E;    // ELL values of A (m rows) and A' (n rows); dense n x n; equilibration
  const int *Ai, *Ati, *qoff, *qlen;            // ELL column indices; start (in y) and size of every second-order cone
  const real *Bn, *Cn, *V0, *scal;              // per problem: normalised b (m), c (n), warm v (l), [sigma, |b|_inf, |c|_inf]
  real *xys, *q;                                // per problem: normalised x, y, s (n + 2 m); reduced scalars (SB_QS)
  int *it;                                      // per problem: iter, status_val
  int *counter;                                 // the next problem index
};
// own values (scs_amd_small_solve_values): Av, Atv, Pd, D, E hold one block per problem, at strides m wA, n wAt, n^2, m, n, and
// Hinv is not read: every workgroup factors its problem's H into its own slab of 2 n^2 values (slab + 2 n^2 blockIdx.x)
struct SbArgsOwn : SbArgs {
  real *slab;
};

// scr (block values) and red (a slot per wave, 8 at the least)
static size_t sb_lds_values(int n, int m, int block) {
  return 6 * (size_t)(n + m + 1) + 2 * (size_t)m + 3 * (size_t)n + block + std::max(8, block / 64);
}

// out[j] = sum_{k < W} val[k * cols + j] * x[SPARSE ? idx[k * cols + j] : k],  j < cols; x, out and scr (BLOCK values) in LDS.
// cols <= BLOCK / 2: BLOCK / cols threads share an output, each a fixed range of k, combined in index order.  Barrier on exit.
template <bool SPARSE, int BLOCK>
__device__ __forceinline__ void sb_mv(const real *__restrict__ val, const int *__restrict__ idx, int W, int cols, const real *x,
                                      real *out, real *scr) {
  const int t = threadIdx.x;
  if (cols > BLOCK / 2) {
    for (int j = t; j < cols; j += BLOCK) {
      real s = 0;
#pragma unroll 4
      for (int k = 0; k < W; ++k) s += val[(size_t)k * cols + j] * x[SPARSE ? idx[(size_t)k * cols + j] : k];
      out[j] = s;
    }
    __syncthreads();
  } else {
    const int nc = BLOCK / cols, c = t / cols, j = t - c * cols, per = (W + nc - 1) / nc;
    if (c < nc) {
      const int k0 = c * per, k1 = min(W, k0 + per);
      real s = 0;
#pragma unroll 4
      for (int k = k0; k < k1; ++k) s += val[(size_t)k * cols + j] * x[SPARSE ? idx[(size_t)k * cols + j] : k];
      scr[c * cols + j] = s;
    }
    __syncthreads();
    if (t < cols) {
      real s = scr[t];
      for (int cc = 1; cc < nc; ++cc) s += scr[cc * cols + t];
      out[t] = s;
    }
    __syncthreads();
  }
}

// The per-problem factor of the own-values kernel, run by the problem's workgroup before its first iteration.  S0, S1: the
// workgroup's slab in HBM, n x n each; w_m (m), o_n, e_n (n) and scr (BLOCK): LDS.  On return S0 = H^-1, or false when a pivot of
// the Cholesky factor is not positive and finite (the same value is read by every thread, so the workgroup returns as one).
//   1. H = rho_x I + P + A' R_y^-1 A, row i as (A' (R_y^-1 (A e_i)) + P e_i) + rho_x e_i: the two products of the iteration
//      (sb_mv), so every element's sum is taken in the order of the padded rows, fixed by the pattern alone.  No atomics.
//   2. H = L L', right-looking: column j is scaled by one pass (kept in scr), the trailing lower triangle updated by all threads.
//   3. X = L^-1 by forward substitution, thread c its column c (it reads only what it wrote itself); H^-1 = X' X, element (a, b)
//      and (b, a) from the same products in the same order, so the inverse is symmetric to the bit.
// Every loop is bounded by n, m or the row widths.
template <int BLOCK>
__device__ __forceinline__ bool sb_factor(const real *__restrict__ Av, const int *__restrict__ Ai, int wA, const real *__restrict__ Atv,
                                          const int *__restrict__ Ati, int wAt, const real *__restrict__ Pd, int n, int m, int z,
                                          real rho_x, real rz, real rc, real *S0, real *S1, real *w_m, real *o_n, real *e_n, real *scr) {
  const int t = threadIdx.x;
  for (int i = 0; i < n; ++i) {
    if (t < n) e_n[t] = t == i ? (real)1 : (real)0;
    __syncthreads();
    sb_mv<true, BLOCK>(Av, Ai, wA, m, e_n, w_m, scr);
    for (int r = t; r < m; r += BLOCK) w_m[r] = w_m[r] / (r < z ? rz : rc);
    __syncthreads();
    sb_mv<true, BLOCK>(Atv, Ati, wAt, n, w_m, o_n, scr);
    if (t < n) {
      real h = o_n[t];
      if (Pd) h += Pd[(size_t)i * n + t];
      if (t == i) h += rho_x;
      S0[(size_t)i * n + t] = h;
    }
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const real d = S0[(size_t)j * n + j];
    if (!(d > (real)0) || !isfinite(d)) return false;
    const real rd = sqrt(d);
    const int cnt = n - 1 - j;
    if (t < cnt) {
      const size_t e = (size_t)(j + 1 + t) * n + j;
      const real v = S0[e] / rd;
      scr[t] = v;
      S0[e] = v;
    }
    __syncthreads(); // every thread has read the pivot
    if (t == 0) S0[(size_t)j * n + j] = rd;
    for (int e = t; e < cnt * cnt; e += BLOCK) {
      const int ii = e / cnt, kk = e - ii * cnt;
      if (kk <= ii) S0[(size_t)(j + 1 + ii) * n + (j + 1 + kk)] -= scr[ii] * scr[kk];
    }
    __syncthreads();
  }
  // n of the workgroup's threads work here, each a chain of O(n^2) reads of what it wrote itself: the serial part of the factor.  The
  // whole factor was measured at 0.6 - 2.8 % of a values solve at (n, m) = (128, 384) (profiles/small_values.md), so it is left simple
  if (t < n) {
    for (int i = 0; i < n; ++i) {
      real x = 0;
      if (i >= t) {
        x = i == t ? (real)1 : (real)0;
        for (int k = t; k < i; ++k) x -= S0[(size_t)i * n + k] * S1[(size_t)k * n + t];
        x /= S0[(size_t)i * n + i];
      }
      S1[(size_t)i * n + t] = x;
    }
  }
  __syncthreads();
  for (int e = t; e < n * n; e += BLOCK) {
    const int r = e / n, c = e - r * n;
    real h = 0;
    for (int i = max(r, c); i < n; ++i) h += S1[(size_t)i * n + r] * S1[(size_t)i * n + c];
    S0[e] = h;
  }
  __syncthreads();
  return true;
}

__device__ __forceinline__ real sb_safediv(real x, real y) { return y < (real)DIV_EPS_TOL ? x / (real)DIV_EPS_TOL : x / y; }

// fill_residuals + compute_residuals_scalars + has_converged above on the reduced scalars q (the un-normalised side is what the
// test reads); sg = the problem's primal_scale = dual_scale
__device__ int sb_has_converged(const real *q, const SbArgs &a, real sg, real nm_b, real nm_c) {
  const real tau = q[Q_TAU];
  real bty_tau = q[Q_BTY], ctx_tau = q[Q_CTX];
  const real xpx_tau = a.has_P ? q[Q_XPX] : (real)0;
  real bty = sb_safediv(bty_tau, tau), ctx = sb_safediv(ctx_tau, tau), xpx = sb_safediv(xpx_tau, tau * tau);
  real gap = fabs(xpx + ctx + bty);
  real pd = 1;
  real nm_pri = q[Q_PRI_N], nm_axs = q[Q_AXS_N], nm_ax = q[Q_AX_N], nm_s = q[Q_S_N];
  real nm_dual = q[Q_DUAL_N], nm_px = q[Q_PX_N], nm_aty = q[Q_ATY_N];
  if (a.normalize) {
    pd = sg * sg;
    bty_tau /= pd; ctx_tau /= pd; xpx /= pd; ctx /= pd; bty /= pd; gap /= pd;
    nm_pri = q[Q_PRI_O]; nm_axs = q[Q_AXS_O]; nm_ax = q[Q_AX_O]; nm_s = q[Q_S_O];
    nm_dual = q[Q_DUAL_O]; nm_px = q[Q_PX_O]; nm_aty = q[Q_ATY_O];
  }
  const real tol = (real)INFEAS_NEGATIVITY_TOL / pd;
  const real res_pri = sb_safediv(nm_pri, tau), res_dual = sb_safediv(nm_dual, tau);
  real res_unbdd_a = (real)NAN, res_unbdd_p = (real)NAN, res_infeas = (real)NAN;
  if (ctx_tau < -tol) {
    res_unbdd_a = sb_safediv(nm_axs, -ctx_tau);
    res_unbdd_p = sb_safediv(nm_px, -ctx_tau);
  }
  if (bty_tau < -tol) res_infeas = sb_safediv(nm_aty, -bty_tau);
  if (tau > (real)0) {
    const real grl = fmax(fmax(fabs(xpx), fabs(ctx)), fabs(bty));
    const real prl = fmax(fmax(nm_b * tau, nm_s), nm_ax) / tau;
    const real drl = fmax(fmax(nm_c * tau, nm_px), nm_aty) / tau;
    if (res_pri < a.eps_abs + a.eps_rel * prl && res_dual < a.eps_abs + a.eps_rel * drl && gap < a.eps_abs + a.eps_rel * grl)
      return SCS_SOLVED;
  }
  if (res_unbdd_a < a.eps_infeas && res_unbdd_p < a.eps_infeas) return SCS_UNBOUNDED;
  if (res_infeas < a.eps_infeas) return SCS_INFEASIBLE;
  return 0;
}

// BLOCK = 256: two waves per SIMD, so that two workgroups share a CU at the narrow limits.  BLOCK = 1024: four waves per SIMD, one
// workgroup per CU.  OWN = false: the matrices and H^-1 are the object's, shared by all problems.  OWN = true: the problem's own
// values, and H^-1 from the factor the workgroup runs first (sb_factor).
template <bool OWN, int BLOCK>
__global__ __launch_bounds__(BLOCK, BLOCK == SB_BLOCK ? 2 : 1) void k_small_batch(const std::conditional_t<OWN, SbArgsOwn, SbArgs> a) {
  extern __shared__ __align__(16) unsigned char sb_lds_raw[];
  __shared__ int next_p;
  const int n = a.n, m = a.m, l = a.l, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  real *u = reinterpret_cast<real *>(sb_lds_raw), *u_t = u + l, *v = u_t + l, *rsk = v + l, *g = rsk + l, *cb = g + l; // cb = [c; b]
  real *sm1 = cb + l, *sm2 = sm1 + m, *sn1 = sm2 + m, *sn2 = sn1 + n, *sn3 = sn2 + n, *scr = sn3 + n, *red = scr + BLOCK;
  const real rz = (real)1.0 / ((real)1000. * a.scale), rc = (real)1.0 / a.scale; // k_set_diag_r
  auto R = [&](int i) -> real { return i < n ? a.rho_x : (i < n + a.z ? rz : (i < l - 1 ? rc : (real)TAU_FACTOR)); };
  const real *Av = a.Av, *Atv = a.Atv, *Hinv = a.Hinv, *Pd = a.Pd, *D = a.D, *E = a.E; // OWN: set per problem below
  // r[0 .. n + m) <- (R + M)^-1 r, exactly (the header comment); r in LDS
  auto lin_solve = [&](real *r) {
    for (int i = t; i < m; i += BLOCK) sm1[i] = r[n + i] / R(n + i);
    __syncthreads();
    sb_mv<true, BLOCK>(Atv, a.Ati, a.wAt, n, sm1, sn1, scr);
    if (t < n) sn1[t] += r[t];
    __syncthreads();
    sb_mv<false, BLOCK>(Hinv, nullptr, n, n, sn1, sn2, scr); // x0
    // one step of refinement against the KKT operator: y0 = R_y^-1 (A x0 - r_y), rho = r_x - (R_x + P) x0 - A' y0, x = x0 + H^-1 rho.
    // The residual is formed from terms of the size of the data, not of |H| |x|: the error of H^-1 along an eigenvector of H of
    // eigenvalue near rho_x (entries of H^-1 near 1 / rho_x) is seen and removed
    sb_mv<true, BLOCK>(Av, a.Ai, a.wA, m, sn2, sm1, scr);
    for (int i = t; i < m; i += BLOCK) sm1[i] = (sm1[i] - r[n + i]) / R(n + i);
    __syncthreads();
    sb_mv<true, BLOCK>(Atv, a.Ati, a.wAt, n, sm1, sn3, scr);
    if (a.has_P) sb_mv<false, BLOCK>(Pd, nullptr, n, n, sn2, sn1, scr);
    if (t < n) sn3[t] = ((r[t] - a.rho_x * sn2[t]) - (a.has_P ? sn1[t] : (real)0)) - sn3[t];
    __syncthreads();
    sb_mv<false, BLOCK>(Hinv, nullptr, n, n, sn3, sn1, scr);
    if (t < n) r[t] = sn2[t] + sn1[t];
    __syncthreads();
    sb_mv<true, BLOCK>(Av, a.Ai, a.wA, m, r, sm1, scr);
    for (int i = t; i < m; i += BLOCK) r[n + i] = (sm1[i] - r[n + i]) / R(n + i);
    __syncthreads();
  };
  for (int taken = 0; taken < a.nprob; ++taken) { // a workgroup takes at most nprob problems
    __syncthreads();
    if (t == 0) next_p = atomicAdd(a.counter, 1);
    __syncthreads();
    const int p = next_p;
    if (p >= a.nprob) break;
    if constexpr (OWN) {
      Av = a.Av + (size_t)p * m * a.wA;
      Atv = a.Atv + (size_t)p * n * a.wAt;
      if (a.has_P) Pd = a.Pd + (size_t)p * n * n;
      D = a.D + (size_t)p * m;
      E = a.E + (size_t)p * n;
      real *slab = a.slab + (size_t)blockIdx.x * 2 * n * n;
      Hinv = slab;
      // the state vectors are not live yet: the factor's scratch is sm1, sn1, sn2 and scr
      if (!sb_factor<BLOCK>(Av, a.Ai, a.wA, Atv, a.Ati, a.wAt, a.has_P ? Pd : nullptr, n, m, a.z, a.rho_x, rz, rc, slab, slab + (size_t)n * n,
                     sm1, sn1, sn2, scr)) {
        if (t == 0) { // H is not positive definite: this problem alone fails
          a.it[2 * (size_t)p] = -1;
          a.it[2 * (size_t)p + 1] = SCS_FAILED;
        }
        continue;
      }
    }
    const real sg = a.scal[3 * (size_t)p], nm_b = a.scal[3 * (size_t)p + 1], nm_c = a.scal[3 * (size_t)p + 2];
    for (int i = t; i < l; i += BLOCK) {
      real h = 0;
      if (i < n) h = a.Cn[(size_t)p * n + i];
      else if (i < l - 1) h = a.Bn[(size_t)p * m + (i - n)];
      cb[i] = h;
      g[i] = i < n ? h : -h; // k_build_g
      v[i] = a.warm ? a.V0[(size_t)p * l + i] : (i == l - 1 ? (real)1 : (real)0);
      u[i] = 0;
      u_t[i] = 0;
      rsk[i] = 0;
    }
    __syncthreads();
    lin_solve(g); // update_work_cache
    real q[Q_COUNT];
    int status = 0, iter = 0;
    for (int it = 0;; ++it) {
      const bool last = it >= a.max_iters; // past the loop: the residuals of the final iterate (finalize)
      if (!last) {
        // ---- normalize_v, u_t = [R_x v; -R_y v; v_tau]
        if (it >= FEASIBLE_ITERS) {
          real s = 0;
          for (int i = t; i < l; i += BLOCK) s += v[i] * v[i];
          const real nrm = sqrt(block_sum(s, red));
          if (nrm != (real)0) {
            const real f = sqrt((real)l) * (real)1. / nrm;
            for (int i = t; i < l; i += BLOCK) v[i] *= f;
          }
        }
        for (int i = t; i < l; i += BLOCK) u_t[i] = i < n ? v[i] * R(i) : (i < l - 1 ? -v[i] * R(i) : v[i]);
        __syncthreads();
        lin_solve(u_t);
        // ---- root_plus
        real tau_t = 1;
        if (it >= FEASIBLE_ITERS) {
          real gg = 0, mug = 0, pg = 0, pp = 0, pmu = 0;
          for (int i = t; i < l - 1; i += BLOCK) {
            const real ri = R(i), gi = g[i], pi = u_t[i], mui = v[i];
            gg += gi * gi * ri;
            mug += mui * gi * ri;
            pg += pi * gi * ri;
            pp += pi * pi * ri;
            pmu += pi * mui * ri;
          }
          gg = block_sum(gg, red);
          mug = block_sum(mug, red);
          pg = block_sum(pg, red);
          pp = block_sum(pp, red);
          pmu = block_sum(pmu, red);
          const real ts = (real)TAU_FACTOR, eta = v[l - 1];
          tau_t = root_plus_from_coeffs(ts + gg, mug - 2 * pg - eta * ts, pp - pmu);
        }
        // ---- u_t -= tau~ g, u = 2 u_t - v, Moreau pre-scaling (sm2 = -R_y u_y)
        __syncthreads();
        for (int i = t; i < l; i += BLOCK) {
          if (i < l - 1) {
            const real ut = u_t[i] + g[i] * (-tau_t);
            u_t[i] = ut;
            const real uu = 2 * ut - v[i];
            u[i] = uu;
            if (i >= n) sm2[i - n] = i < n + a.z ? (real)0 : (i < n + a.z + a.nl ? fmax(uu * (-rc), (real)0) : uu * (-rc));
          } else {
            u_t[i] = tau_t;
            const real uu = 2 * tau_t - v[i];
            u[i] = it < FEASIBLE_ITERS ? (real)1 : (uu > (real)0 ? uu : (real)0);
          }
        }
        __syncthreads();
        // ---- second-order cones (proj_soc, src/cones.c:1250-1279)
        for (int ci = t; ci < a.qsize; ci += BLOCK) {
          const int len = a.qlen[ci];
          if (len > SB_SERIAL_Q || len <= 0) continue;
          real *x = sm2 + a.qoff[ci];
          if (len == 1) {
            x[0] = fmax(x[0], (real)0);
            continue;
          }
          const real v1 = x[0];
          real s;
          if (len == 2) s = fabs(x[1]);
          else {
            s = 0;
            for (int k = 1; k < len; ++k) s += x[k] * x[k];
            s = sqrt(s);
          }
          if (s <= v1) continue;
          if (s <= -v1) {
            for (int k = 0; k < len; ++k) x[k] = 0;
          } else {
            const real al = (s + v1) / (real)2.0, f = al / s;
            x[0] = al;
            for (int k = 1; k < len; ++k) x[k] *= f;
          }
        }
        for (int ci = wave; ci < a.qsize; ci += BLOCK / 64) {
          const int len = a.qlen[ci];
          if (len <= SB_SERIAL_Q) continue;
          real *x = sm2 + a.qoff[ci];
          real s = 0;
          for (int k = 1 + lane; k < len; k += 64) s += x[k] * x[k];
          s = sqrt(__shfl(wave_sum(s), 0, 64));
          const real v1 = x[0];
          if (s <= v1) continue;
          if (s <= -v1) {
            for (int k = lane; k < len; k += 64) x[k] = 0;
          } else {
            const real al = (s + v1) / (real)2.0, f = al / s;
            for (int k = 1 + lane; k < len; k += 64) x[k] *= f;
            if (lane == 0) x[0] = al;
          }
        }
        __syncthreads();
        // ---- Moreau post, rsk = R (v + u - 2 u_t)
        for (int i = t; i < l; i += BLOCK) {
          real ui = u[i];
          const real ri = R(i);
          if (i >= n && i < l - 1) {
            ui = sm2[i - n] / ri + ui;
            u[i] = ui;
          }
          rsk[i] = (v[i] + ui - 2 * u_t[i]) * ri;
        }
        __syncthreads();
      }
      if (last || it % CONVERGED_INTERVAL == 0) {
        // ---- populate_residual_struct (:535-607): the quantities of k_resid_primal / k_resid_dual
        const real *x = u, *y = u + n, *s = rsk + n;
        sb_mv<true, BLOCK>(Av, a.Ai, a.wA, m, x, sm1, scr);     // ax
        sb_mv<true, BLOCK>(Atv, a.Ati, a.wAt, n, y, sn1, scr);  // aty
        if (a.has_P) sb_mv<false, BLOCK>(Pd, nullptr, n, n, x, sn2, scr); // px
        const real tau = absval(u[l - 1]);
        const real ds = sg, inv_ds = (real)1.0 / sg, inv_ps = (real)1.0 / sg;
        {
          real q_pri = 0, q_axs = 0, q_ax = 0, o_pri = 0, o_axs = 0, o_ax = 0, o_s = 0, n_s = 0, bty = 0;
          for (int i = t; i < m; i += BLOCK) {
            const real axi = sm1[i], si = s[i], bi = cb[n + i], Di = D[i];
            const real axs = axi + si, pri = axs - tau * bi, f = inv_ds / Di;
            q_pri = fmax(q_pri, absval(pri)); q_axs = fmax(q_axs, absval(axs)); q_ax = fmax(q_ax, absval(axi));
            o_pri = fmax(o_pri, absval(pri * f)); o_axs = fmax(o_axs, absval(axs * f)); o_ax = fmax(o_ax, absval(axi * f));
            o_s = fmax(o_s, absval(si / (Di * ds))); n_s = fmax(n_s, absval(si));
            bty += y[i] * bi;
          }
          q[Q_PRI_N] = block_max(q_pri, red); q[Q_AXS_N] = block_max(q_axs, red); q[Q_AX_N] = block_max(q_ax, red);
          q[Q_PRI_O] = block_max(o_pri, red); q[Q_AXS_O] = block_max(o_axs, red); q[Q_AX_O] = block_max(o_ax, red);
          q[Q_S_O] = block_max(o_s, red); q[Q_S_N] = block_max(n_s, red); q[Q_BTY] = block_sum(bty, red);
        }
        {
          real q_d = 0, q_px = 0, q_aty = 0, o_d = 0, o_px = 0, o_aty = 0, ctx = 0, xpx = 0;
          for (int j = t; j < n; j += BLOCK) {
            const real pxi = a.has_P ? sn2[j] : (real)0, ai = sn1[j], xi = x[j], ci = cb[j];
            const real dual = pxi + ai + tau * ci, f = inv_ps / E[j];
            q_d = fmax(q_d, absval(dual)); q_px = fmax(q_px, absval(pxi)); q_aty = fmax(q_aty, absval(ai));
            o_d = fmax(o_d, absval(dual * f)); o_px = fmax(o_px, absval(pxi * f)); o_aty = fmax(o_aty, absval(ai * f));
            ctx += xi * ci;
            xpx += pxi * xi;
          }
          q[Q_DUAL_N] = block_max(q_d, red); q[Q_PX_N] = block_max(q_px, red); q[Q_ATY_N] = block_max(q_aty, red);
          q[Q_DUAL_O] = block_max(o_d, red); q[Q_PX_O] = block_max(o_px, red); q[Q_ATY_O] = block_max(o_aty, red);
          q[Q_CTX] = block_sum(ctx, red); q[Q_XPX] = block_sum(xpx, red);
        }
        q[Q_TAU] = tau;
        q[Q_KAP] = absval(rsk[l - 1]);
        iter = it;
        if (last) break;
        status = sb_has_converged(q, a, sg, nm_b, nm_c);
        if (status != 0) break; // like the reference, the converged iteration is not counted
      }
      // ---- dual update
      for (int i = t; i < l; i += BLOCK) v[i] += a.alpha * (u[i] - u_t[i]);
      __syncthreads();
    }
    // ---- the problem's result: normalised x, y, s and the reduced scalars
    real *o = a.xys + (size_t)p * (n + 2 * (size_t)m);
    for (int i = t; i < n + m; i += BLOCK) o[i] = u[i];
    for (int i = t; i < m; i += BLOCK) o[n + m + i] = rsk[n + i];
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < Q_COUNT; ++k) a.q[(size_t)p * SB_QS + k] = q[k];
      a.it[2 * (size_t)p] = iter;
      a.it[2 * (size_t)p + 1] = status;
    }
  }
}

} // namespace scsamd

struct ScsAmdSmall {
  int n = 0, m = 0, l = 0, device = 0, wA = 0, wAt = 0;
  bool has_P = false;
  ScsSettings stgs;
  ScsCone k;
  std::vector<scs_int> cq;
  Scaling scal;
  hipStream_t stream = nullptr;
  DevBuf<real> Av, Atv, Hinv, Pd, D, E;
  DevBuf<int> Ai, Ati, qoff, qlen, counter;
  // staging of a launch, grown to the largest chunk seen
  size_t cap = 0;
  bool cap_warm = false;
  DevBuf<real> dB, dC, dV, dS, dXYS, dQ;
  DevBuf<int> dIt;
  std::vector<real> hB, hC, hV, hS, hXYS, hQ, hWs; // hWs: the s of one problem's warm start (m)
  std::vector<int> hIt;
  SbArgsOwn args{}; // what is the object's, filled once by small_device_init; a chunk copies it and sets what is its own
  int grid_user = 0, grid_default = 1, wg_per_cu = 0;
  int block = SB_BLOCK; // the instantiation, chosen once at init: SB_BLOCK (narrow) or SB_BLOCK_WIDE
  size_t lds_bytes = 0;
  long long counters[4] = {0, 0, 0, 0};
  double setup_time = 0;
  bool on_device = false; // small_device_init has run
  std::vector<real> h_av, h_atv, h_Hinv, h_Pd; // what it uploads, kept on the host until then
  std::vector<int> h_ai, h_ati, h_qoff, h_qlen;
  // own values per problem (scs_amd_small_set_values).  The pattern of init and, built at the first set call, the position maps:
  // CSC entry of A -> its slot in the padded rows of A and of A', upper-P entry -> its dense position (the mirror is the transpose)
  HostCsc patA, patP;
  std::vector<size_t> mapA, mapAt, mapP;
  long long vals_nprob = 0; // 0: no values set
  DevBuf<real> vAv, vAtv, vPd, vD, vE, slab; // one block per problem; the slab: 2 n^2 per workgroup of the largest grid seen
  std::vector<Scaling> vscal;                // D_p, E_p on the host: normalize_b_c, the warm start and the way out
  size_t slab_grid = 0;
  int grid_default_own = 0; // 0: the own-values kernel has not been set up
  ~ScsAmdSmall() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
};

static thread_local std::string g_small_refusal;
static thread_local bool g_small_refused = false;
// says why a call is not served; false, so that a check of the arguments reads `return small_refuse(...)`
static bool small_refuse(const char *fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_small_refusal = buf;
  g_small_refused = true;
  printf("ERROR: scs_amd_small: %s\n", buf);
  return false;
}

// H^-1 and the full symmetric P, dense n x n, from the equilibrated A (CSC) and P (upper triangle, CSC); false when H is not
// positive definite to working precision
static bool small_factor(const HostCsc &A, const HostCsc *P, const std::vector<real> &Ry, real rho_x, std::vector<real> &Hinv,
                         std::vector<real> &Pd) {
  const int n = A.n;
  std::vector<long double> h((size_t)n * n, 0.0L);
  Pd.assign((size_t)n * n, (real)0);
  if (P)
    for (int j = 0; j < n; ++j)
      for (eoff e = P->p[j]; e < P->p[j + 1]; ++e) {
        const int i = P->i[e];
        Pd[(size_t)i * n + j] = P->x[e];
        Pd[(size_t)j * n + i] = P->x[e];
      }
  for (size_t e = 0; e < (size_t)n * n; ++e) h[e] = Pd[e];
  for (int j = 0; j < n; ++j) h[(size_t)j * n + j] += rho_x;
  { // A' R_y^-1 A, row by row of A: gather the rows first
    std::vector<std::vector<std::pair<int, real>>> rows(A.m);
    for (int j = 0; j < n; ++j)
      for (eoff e = A.p[j]; e < A.p[j + 1]; ++e) rows[A.i[e]].push_back({j, A.x[e]});
    for (int i = 0; i < A.m; ++i)
      for (const auto &p1 : rows[i])
        for (const auto &p2 : rows[i]) h[(size_t)p1.first * n + p2.first] += (long double)p1.second * p2.second / Ry[i];
  }
  std::vector<long double> L(h); // Cholesky, lower triangle
  for (int j = 0; j < n; ++j) {
    long double d = L[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(d > 0)) return false;
    d = sqrtl(d);
    L[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      long double s = L[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      L[(size_t)i * n + j] = s / d;
    }
  }
  Hinv.resize((size_t)n * n);
  std::vector<long double> col(n);
  for (int c = 0; c < n; ++c) { // H^-1 e_c
    for (int i = 0; i < n; ++i) {
      long double s = i == c ? 1.0L : 0.0L;
      for (int k = 0; k < i; ++k) s -= L[(size_t)i * n + k] * col[k];
      col[i] = s / L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      long double s = col[i];
      for (int k = i + 1; k < n; ++k) s -= L[(size_t)k * n + i] * col[k];
      col[i] = s / L[(size_t)i * n + i];
    }
    for (int i = 0; i < n; ++i) Hinv[(size_t)c * n + i] = (real)col[i];
  }
  for (int i = 0; i < n; ++i) // H^-1 is symmetric: store it so
    for (int j = i + 1; j < n; ++j) Hinv[(size_t)i * n + j] = Hinv[(size_t)j * n + i] = (real)0.5 * (Hinv[(size_t)i * n + j] + Hinv[(size_t)j * n + i]);
  return true;
}

// padded rows: entry k of row r at [k * rows + r]; padding is (0, column 0).  by_row: the rows of A (else its columns: the rows of A')
static int small_ell(const HostCsc &A, bool by_row, std::vector<real> &val, std::vector<int> &idx) {
  const int rows = by_row ? A.m : A.n;
  std::vector<int> cnt(rows, 0);
  for (int j = 0; j < A.n; ++j)
    for (eoff e = A.p[j]; e < A.p[j + 1]; ++e) cnt[by_row ? A.i[e] : j]++;
  int W = 1;
  for (int r = 0; r < rows; ++r) W = std::max(W, cnt[r]);
  val.assign((size_t)W * rows, (real)0);
  idx.assign((size_t)W * rows, 0);
  std::fill(cnt.begin(), cnt.end(), 0);
  for (int j = 0; j < A.n; ++j)
    for (eoff e = A.p[j]; e < A.p[j + 1]; ++e) {
      const int r = by_row ? A.i[e] : j, c = by_row ? j : A.i[e], k = cnt[r]++;
      val[(size_t)k * rows + r] = A.x[e];
      idx[(size_t)k * rows + r] = c;
    }
  return W;
}

// the instantiation an object runs: k_small_batch<own, s->block>
static const void *small_kernel(const ScsAmdSmall *s, bool own) {
  if (s->block == SB_BLOCK)
    return own ? reinterpret_cast<const void *>(k_small_batch<true, SB_BLOCK>) : reinterpret_cast<const void *>(k_small_batch<false, SB_BLOCK>);
  return own ? reinterpret_cast<const void *>(k_small_batch<true, SB_BLOCK_WIDE>)
             : reinterpret_cast<const void *>(k_small_batch<false, SB_BLOCK_WIDE>);
}

// The default grid of an instantiation, what the chip holds of it at once: its dynamic LDS is set, and the workgroups a CU then
// holds times the CUs.  0 workgroups is an error, not a grid of one (the wide kernel asks for nearly the whole CU: a build whose
// static LDS leaves less room must say so).  Throws HipError.
static int small_grid_default(ScsAmdSmall *s, bool own) {
  const void *kp = small_kernel(s, own);
  HIP_CHECK(hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->lds_bytes));
  int per_cu = 0, cus = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kp, s->block, s->lds_bytes));
  if (per_cu < 1)
    throw HipError("scs_amd_small: no workgroup of " + std::to_string(s->block) + " threads with " + std::to_string(s->lds_bytes) +
                   " B of LDS fits a CU of this device");
  if (!own) s->wg_per_cu = per_cu; // scs_amd_small_get_occupancy reports the shared kernel
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
  return std::max(1, cus) * per_cu;
}

// the host's R_y of row i (the kernel's R lambda on rows n .. n + m): 1 / (1000 scale) on the zero cone, 1 / scale elsewhere
static real small_ry(const ScsAmdSmall *s, int i) {
  return i < s->k.z ? (real)1.0 / ((real)1000. * s->stgs.scale) : (real)1.0 / s->stgs.scale;
}

// D, E of one problem's matrices, which are equilibrated in place (the host passes of scs_init); normalize = 0: the identity
static void small_equilibrate(const ScsAmdSmall *s, HostCsc *P, HostCsc &A, Scaling &sc) {
  if (s->stgs.normalize) {
    equilibrate(P, A, &s->k, sc);
  } else {
    sc.D.assign(s->m, (real)1);
    sc.E.assign(s->n, (real)1);
  }
}

static void small_ensure(ScsAmdSmall *s, size_t chunk, bool warm) {
  if (chunk > s->cap) {
    const size_t n = s->n, m = s->m;
    s->dB.alloc(chunk * m);
    s->dC.alloc(chunk * n);
    s->dS.alloc(chunk * 3);
    s->dXYS.alloc(chunk * (n + 2 * m));
    s->dQ.alloc(chunk * SB_QS);
    s->dIt.alloc(chunk * 2);
    s->cap = chunk;
    s->cap_warm = false;
  }
  if (warm && !s->cap_warm) {
    s->dV.alloc(s->cap * (size_t)s->l);
    s->cap_warm = true;
  }
  const size_t n = s->n, m = s->m; // the host side of the staging: vectors keep their capacity
  s->hB.resize(chunk * m);
  s->hC.resize(chunk * n);
  s->hS.resize(chunk * 3);
  s->hXYS.resize(chunk * (n + 2 * m));
  s->hQ.resize(chunk * SB_QS);
  s->hIt.resize(chunk * 2);
  s->hWs.resize(m);
  if (warm) s->hV.resize(chunk * (size_t)s->l);
}

// the device side of an object, created by its first accepted solve (init is host work only: a refusal, and a machine without a
// device, are known before any device call).  Throws HipError.
static void small_device_init(ScsAmdSmall *s) {
  if (s->on_device) return;
  const double t0 = now_ms();
  const int n = s->n, m = s->m;
  if (scs_amd_device_count() <= 0) throw HipError("scs_amd: no HIP device visible -- this backend has no CPU fallback");
  s->device = selected_device();
  HIP_CHECK(hipSetDevice(s->device));
  if (!s->stream) HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  auto up = [&](auto &b, const auto &h) {
    b.alloc(h.size());
    b.upload(h.data(), h.size(), st);
  };
  up(s->Av, s->h_av);
  up(s->Atv, s->h_atv);
  up(s->Hinv, s->h_Hinv);
  up(s->Pd, s->h_Pd);
  up(s->D, s->scal.D);
  up(s->E, s->scal.E);
  up(s->Ai, s->h_ai);
  up(s->Ati, s->h_ati);
  up(s->qoff, s->h_qoff);
  up(s->qlen, s->h_qlen);
  s->counter.alloc(1);
  HIP_CHECK(hipStreamSynchronize(st));
  s->lds_bytes = sb_lds_values(n, m, s->block) * sizeof(real);
  s->grid_default = small_grid_default(s, false);
  SbArgsOwn &a = s->args; // the chunk's part (nprob, warm, the staging, the own-values blocks and the slab) is set by small_launch
  a.n = n; a.m = m; a.l = s->l; a.z = (int)s->k.z; a.nl = (int)s->k.l; a.qsize = (int)s->k.qsize; a.has_P = s->has_P ? 1 : 0;
  a.normalize = s->stgs.normalize ? 1 : 0; a.max_iters = (int)s->stgs.max_iters; a.wA = s->wA; a.wAt = s->wAt;
  a.rho_x = s->stgs.rho_x; a.scale = s->stgs.scale; a.alpha = s->stgs.alpha; a.eps_abs = s->stgs.eps_abs; a.eps_rel = s->stgs.eps_rel;
  a.eps_infeas = s->stgs.eps_infeas;
  a.Av = s->Av.p; a.Atv = s->Atv.p; a.Hinv = s->Hinv.p; a.Pd = s->Pd.p; a.D = s->D.p; a.E = s->E.p;
  a.Ai = s->Ai.p; a.Ati = s->Ati.p; a.qoff = s->qoff.p; a.qlen = s->qlen.p;
  a.counter = s->counter.p;
  s->on_device = true;
  for (std::vector<real> *v : {&s->h_av, &s->h_atv, &s->h_Hinv, &s->h_Pd}) std::vector<real>().swap(*v);
  for (std::vector<int> *v : {&s->h_ai, &s->h_ati, &s->h_qoff, &s->h_qlen}) std::vector<int>().swap(*v);
  s->setup_time += now_ms() - t0;
}

extern "C" {

void scs_amd_small_limits(scs_int out[2]) {
  if (!out) return;
  out[0] = SB_MAX_N;
  out[1] = SB_MAX_L;
}

const char *scs_amd_small_refusal(void) { return g_small_refused ? g_small_refusal.c_str() : nullptr; }

ScsAmdSmall *scs_amd_small_init(const ScsData *d, const ScsCone *k, const ScsSettings *stgs) {
  g_small_refused = false;
  if (!d || !k || !stgs) {
    small_refuse("missing ScsData, ScsCone or ScsSettings (a NULL argument)");
    return nullptr;
  }
  if (!d->A || !d->b || !d->c || d->m <= 0 || d->n <= 0) {
    small_refuse("A, b or c missing (a NULL argument), or m or n not positive");
    return nullptr;
  }
  if (k->bsize) { small_refuse("a box cone (bsize != 0) is not served"); return nullptr; }
  if (k->ssize) { small_refuse("a PSD cone (ssize != 0) is not served"); return nullptr; }
  if (k->cssize) { small_refuse("a complex PSD cone (cssize != 0) is not served"); return nullptr; }
  if (k->ep || k->ed) { small_refuse("an exponential cone (ep / ed != 0) is not served"); return nullptr; }
  if (k->psize) { small_refuse("a power cone (psize != 0) is not served"); return nullptr; }
  if (stgs->adaptive_scale) { small_refuse("adaptive_scale != 0 is not served (the factor of H belongs to one scale)"); return nullptr; }
  if (stgs->acceleration_lookback) { small_refuse("acceleration_lookback != 0 is not served"); return nullptr; }
  if (stgs->time_limit_secs != 0) { small_refuse("time_limit_secs != 0 is not served (the kernel reads no clock)"); return nullptr; }
  if (stgs->log_csv_filename) { small_refuse("log_csv_filename is not served"); return nullptr; }
  if (stgs->write_data_filename) { small_refuse("write_data_filename is not served"); return nullptr; }
  if ((long long)d->n > SB_MAX_N) {
    small_refuse("size over the limit: n = %lld > %d", (long long)d->n, SB_MAX_N);
    return nullptr;
  }
  if ((long long)d->n + (long long)d->m + 1 > SB_MAX_L) {
    small_refuse("size over the limit: n + m + 1 = %lld > %d", (long long)d->n + (long long)d->m + 1, SB_MAX_L);
    return nullptr;
  }
  if ((d->A->x && d->A->p && d->A->p[d->n] > 0 && !all_finite(d->A->x, (size_t)d->A->p[d->n])) ||
      (d->P && d->P->x && d->P->p && d->P->p[d->n] > 0 && !all_finite(d->P->x, (size_t)d->P->p[d->n]))) {
    small_refuse("non-finite values in A or P");
    return nullptr;
  }
  if (validate_problem(d, k, stgs) < 0) {
    small_refuse("the problem does not pass the validation of scs_init (its message is above)");
    return nullptr;
  }
  const double t0 = now_ms();
  std::unique_ptr<ScsAmdSmall> s(new ScsAmdSmall());
  const int n = s->n = (int)d->n, m = s->m = (int)d->m;
  s->l = n + m + 1;
  s->block = n <= SB_NARROW_N && s->l <= SB_NARROW_L ? SB_BLOCK : SB_BLOCK_WIDE; // both entries, for the object's life
  s->stgs = *stgs;
  s->stgs.write_data_filename = s->stgs.log_csv_filename = nullptr;
  s->k = *k;
  if (k->qsize) s->cq.assign(k->q, k->q + k->qsize);
  s->k.q = s->cq.data();
  s->has_P = d->P != nullptr;
  // ---- host: equilibrate (the host passes of scs_init), diag_r, H, its factor, the padded rows
  HostCsc A, P;
  A.copy_from(d->A);
  if (s->has_P) P.copy_from(d->P);
  s->patA = A; // the pattern scs_amd_small_set_values writes values on
  if (s->has_P) s->patP = P;
  small_equilibrate(s.get(), s->has_P ? &P : nullptr, A, s->scal);
  std::vector<real> Ry(m), Hinv, Pd, av, atv;
  std::vector<int> ai, ati, qoff, qlen;
  for (int i = 0; i < m; ++i) Ry[i] = small_ry(s.get(), i);
  if (!small_factor(A, s->has_P ? &P : nullptr, Ry, stgs->rho_x, Hinv, Pd)) {
    small_refuse("the reduced matrix R_x + P + A' R_y^-1 A is not positive definite (P must be positive semidefinite)");
    return nullptr;
  }
  s->wA = small_ell(A, true, av, ai);
  s->wAt = small_ell(A, false, atv, ati);
  {
    int off = (int)(k->z + k->l);
    for (scs_int c = 0; c < k->qsize; ++c) {
      qoff.push_back(off);
      qlen.push_back((int)k->q[c]);
      off += (int)k->q[c];
    }
    if (qoff.empty()) { // never read (qsize = 0); keeps the upload below uniform
      qoff.push_back(0);
      qlen.push_back(0);
    }
  }
  s->h_av.swap(av); s->h_atv.swap(atv); s->h_Hinv.swap(Hinv); s->h_Pd.swap(Pd);
  s->h_ai.swap(ai); s->h_ati.swap(ati); s->h_qoff.swap(qoff); s->h_qlen.swap(qlen);
  s->setup_time = now_ms() - t0;
  return s.release();
}

scs_int scs_amd_small_set_grid(ScsAmdSmall *s, scs_int workgroups) {
  if (!s || workgroups < 0 || (long long)workgroups > 1048576) return -1;
  s->grid_user = (int)workgroups;
  return 0;
}

void scs_amd_small_get_counters(const ScsAmdSmall *s, long long out[4]) {
  if (!s || !out) return;
  for (int i = 0; i < 4; ++i) out[i] = s->counters[i];
}

// out[0] workgroups per CU the kernel's LDS allows, out[1] LDS bytes per workgroup, out[2] the default grid, out[3] setup time in
// microseconds (0 and 1 are 0 before the first solve); out[4] the threads of a workgroup of the object's instantiation, 256 (narrow)
// or 1024 (wide), known from init on
void scs_amd_small_get_occupancy(const ScsAmdSmall *s, long long out[5]) {
  if (!s || !out) return;
  out[0] = s->wg_per_cu;
  out[1] = (long long)s->lds_bytes;
  out[2] = s->grid_default;
  out[3] = (long long)(s->setup_time * 1e3);
  out[4] = s->block;
}

// ---- the steps of small_solve: the checks of a call, one problem's way in, a chunk's launch, one problem's way out ------------
// false, with the refusal said, when the call is not served
static bool small_solve_accepts(const ScsAmdSmall *s, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                const ScsSolution *sols, const ScsInfo *infos, bool own) {
  if (!s || !B || !Cc || !sols || !infos) return small_refuse("missing ScsAmdSmall, B, Cc, ScsSolution or ScsInfo (a NULL argument)");
  if (nprob < 1) return small_refuse("nprob < 1");
  const int n = s->n, m = s->m;
  if ((long long)ldb < m || (long long)ldc < n) return small_refuse("short leading dimension: ldb < m or ldc < n");
  for (scs_int p = 0; p < nprob; ++p) {
    if (!all_finite(B + (size_t)p * (size_t)ldb, (size_t)m) || !all_finite(Cc + (size_t)p * (size_t)ldc, (size_t)n))
      return small_refuse("non-finite values in B or Cc (problem %lld)", (long long)p);
    if (!sols[p].x || !sols[p].y || !sols[p].s) return small_refuse("sols[%lld].x, y or s is NULL (a NULL argument)", (long long)p);
  }
  // what depends on the object's state comes last: the checks of the arguments above need no accepted set call
  if (own && s->vals_nprob == 0) return small_refuse("no values are set (scs_amd_small_set_values comes first)");
  if (own && (long long)nprob != s->vals_nprob)
    return small_refuse("nprob = %lld, but the values were set for %lld problems", (long long)nprob, s->vals_nprob);
  return true;
}

// scs_update (:1287-1325) and, with warm, the warm start (:660-687) of the problem in slot p of the chunk's staging: the norms of
// (b, c) as given, b and c normalised with the problem's own sigma, v = [x; y + s / R_y; 1] from the caller's normalised (x, y, s).
// sc: the D, E the problem's matrices were equilibrated with -- the object's, or the problem's own; in small_return too.
static void small_stage(ScsAmdSmall *s, int p, const Scaling &sc, const scs_float *bk, const scs_float *ck, const ScsSolution &sol, bool warm) {
  const int n = s->n, m = s->m, l = s->l;
  const bool norm = s->stgs.normalize != 0;
  real *b = s->hB.data() + (size_t)p * m, *c = s->hC.data() + (size_t)p * n;
  std::copy(bk, bk + m, b);
  std::copy(ck, ck + n, c);
  real nb = 0, nc = 0, sg = 1;
  for (int i = 0; i < m; ++i) nb = std::max(nb, (real)std::fabs(b[i]));
  for (int j = 0; j < n; ++j) nc = std::max(nc, (real)std::fabs(c[j]));
  if (norm) sg = normalize_b_c_sigma(sc, b, c);
  s->hS[3 * (size_t)p] = sg;
  s->hS[3 * (size_t)p + 1] = nb;
  s->hS[3 * (size_t)p + 2] = nc;
  if (!warm) return;
  real *v = s->hV.data() + (size_t)p * l, *x = v, *y = v + n, *sv = s->hWs.data();
  std::copy(sol.x, sol.x + n, x);
  std::copy(sol.y, sol.y + m, y);
  std::copy(sol.s, sol.s + m, sv);
  if (norm) normalize_sol_scaled(sc, sg, sg, x, y, sv);
  for (int j = 0; j < n; ++j) x[j] = x[j] != x[j] ? (real)0 : x[j];
  for (int i = 0; i < m; ++i) {
    const real tt = y[i] + sv[i] / small_ry(s, i);
    y[i] = tt != tt ? (real)0 : tt;
  }
  v[l - 1] = 1;
}

// The chunk of K staged problems, the first of them problem `done` of the call: the staging goes up, one launch of the object's
// instantiation on min(K, the grid) workgroups, the results come down; returns with the stream idle.  Returns the grid.  Throws
// HipError.
static int small_launch(ScsAmdSmall *s, int K, size_t done, bool warm, bool own) {
  const size_t n = s->n, m = s->m, l = s->l, ow = n + 2 * m;
  hipStream_t st = s->stream;
  s->dB.upload(s->hB.data(), (size_t)K * m, st);
  s->dC.upload(s->hC.data(), (size_t)K * n, st);
  s->dS.upload(s->hS.data(), (size_t)K * 3, st);
  if (warm) s->dV.upload(s->hV.data(), (size_t)K * l, st);
  HIP_CHECK(hipMemsetAsync(s->counter.p, 0, sizeof(int), st));
  SbArgsOwn a = s->args;
  a.nprob = K; a.warm = warm ? 1 : 0;
  a.Bn = s->dB.p; a.Cn = s->dC.p; a.V0 = warm ? s->dV.p : nullptr; a.scal = s->dS.p;
  a.xys = s->dXYS.p; a.q = s->dQ.p; a.it = s->dIt.p;
  const int grid = std::min(K, s->grid_user > 0 ? s->grid_user : (own ? s->grid_default_own : s->grid_default));
  if (own) {
    a.Av = s->vAv.p + done * m * s->wA; a.Atv = s->vAtv.p + done * n * s->wAt; a.Hinv = nullptr;
    a.Pd = s->has_P ? s->vPd.p + done * n * n : nullptr; a.D = s->vD.p + done * m; a.E = s->vE.p + done * n;
    if ((size_t)grid > s->slab_grid) { // the slab follows the grid, not the number of problems
      s->slab_grid = 0;
      s->slab.alloc((size_t)grid * 2 * n * n);
      s->slab_grid = (size_t)grid;
    }
    a.slab = s->slab.p;
  }
  // the shared kernel's parameter is an SbArgs: the base of the struct filled above
  void *arg[] = {own ? static_cast<void *>(&a) : static_cast<void *>(static_cast<SbArgs *>(&a))};
  (void)hipLaunchKernel(small_kernel(s, own), dim3(grid), dim3(s->block), arg, s->lds_bytes, st);
  HIP_CHECK(hipGetLastError());
  s->dXYS.download(s->hXYS.data(), (size_t)K * ow, st);
  s->dQ.download(s->hQ.data(), (size_t)K * SB_QS, st);
  s->dIt.download(s->hIt.data(), (size_t)K * 2, st);
  HIP_CHECK(hipStreamSynchronize(st));
  return grid;
}

// finalize (:825-969) of the problem in slot p of the chunk that came down: its (x, y, s) un-normalised into sol, its reduced
// scalars into info; the failed pivot of the device factor fails this problem alone
static void small_return(ScsAmdSmall *s, int p, const Scaling &sc, bool own, double chunk_ms, double t_call, ScsSolution *sol, ScsInfo *info) {
  const int n = s->n, m = s->m;
  const bool norm = s->stgs.normalize != 0;
  if (own && s->hIt[2 * (size_t)p + 1] == SCS_FAILED) { // the device factor's pivot test: this problem alone
    memset(info, 0, sizeof *info);
    fail_out(nullptr, m, n, sol, info, SCS_FAILED, "the reduced matrix R_x + P + A' R_y^-1 A of this problem is not positive definite",
             "failure");
    return;
  }
  const real sg = s->hS[3 * (size_t)p];
  const real *o = s->hXYS.data() + (size_t)p * ((size_t)n + 2 * (size_t)m);
  std::copy(o, o + n, sol->x);
  std::copy(o + n, o + n + m, sol->y);
  std::copy(o + n + m, o + n + 2 * (size_t)m, sol->s);
  if (norm) un_normalize_sol_scaled(sc, sg, sg, sol->x, sol->y, sol->s);
  Resid r_n, r_o;
  const int iter = s->hIt[2 * (size_t)p];
  fill_residuals(r_n, r_o, s->hQ.data() + (size_t)p * SB_QS, 1, iter, s->has_P, norm, sg, sg);
  memset(info, 0, sizeof *info);
  strcpy(info->lin_sys_solver, "dense-direct-small-batch-hip-gfx950");
  info->status_val = s->hIt[2 * (size_t)p + 1];
  info->iter = iter;
  info->setup_time = (real)s->setup_time;
  info->scale = s->stgs.scale;
  info->aa_stats.last_aa_norm = (real)NAN;
  const LoopEnd e{(int)s->stgs.max_iters, 0, false};
  finalize_status(r_o, n, m, e, sol, info);
  info->solve_time = (real)chunk_ms; // the launch's wall time, the same in every problem of it
  s->counters[3] += iter;
  if (s->stgs.verbose) print_summary_row(r_o, iter, s->stgs.scale, (now_ms() - t_call + s->setup_time) / 1e3);
}

// scs_amd_small_solve (own = false) and scs_amd_small_solve_values (own = true: the values, D and E of the last set call): the
// frame around the steps above -- the listener, the chunk loop with SIGINT looked at between launches, the counters, and the
// failure of every problem on a HIP error
static scs_int small_solve(ScsAmdSmall *s, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                           ScsSolution *sols, ScsInfo *infos, scs_int warm_start, bool own) {
  g_small_refused = false;
  if (!small_solve_accepts(s, nprob, B, ldb, Cc, ldc, sols, infos, own)) return SCS_FAILED;
  const int n = s->n, m = s->m;
  InterruptListener listener;
  const double t_call = now_ms();
  const bool warm = warm_start != 0;
  try {
    small_device_init(s);
    HIP_CHECK(hipSetDevice(s->device));
    bool sigint = false;
    for (scs_int done = 0; done < nprob; done += SB_CHUNK) {
      const int K = (int)std::min<scs_int>(SB_CHUNK, nprob - done);
      if (sigint || interrupted()) { // honoured between launches only
        sigint = true;
        for (int p = 0; p < K; ++p) fail_out(nullptr, m, n, &sols[done + p], &infos[done + p], SCS_SIGINT, "interrupted", "interrupted");
        continue;
      }
      const double t0 = now_ms();
      small_ensure(s, (size_t)K, warm);
      // problem p of the chunk is problem done + p of the call: its column of B and Cc, its sols / infos and, own values, its D and E
      auto scaling = [&](int p) -> const Scaling & { return own ? s->vscal[(size_t)done + p] : s->scal; };
      for (int p = 0; p < K; ++p)
        small_stage(s, p, scaling(p), B + (size_t)(done + p) * (size_t)ldb, Cc + (size_t)(done + p) * (size_t)ldc, sols[done + p], warm);
      const int grid = small_launch(s, K, (size_t)done, warm, own);
      const double chunk_ms = now_ms() - t0;
      s->counters[0] += 1;
      s->counters[1] += grid;
      s->counters[2] += K;
      for (int p = 0; p < K; ++p) small_return(s, p, scaling(p), own, chunk_ms, t_call, &sols[done + p], &infos[done + p]);
    }
  } catch (const std::exception &ex) {
    fprintf(stderr, "%s\n", ex.what());
    if (s->stream) (void)hipStreamSynchronize(s->stream); // nothing of this call may still be reading or writing
    for (scs_int p = 0; p < nprob; ++p) fail_out(nullptr, m, n, &sols[p], &infos[p], SCS_FAILED, "HIP error in scs_amd_small_solve", "failure");
    return SCS_FAILED;
  }
  return 0;
}

scs_int scs_amd_small_solve(ScsAmdSmall *s, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                            ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  return small_solve(s, nprob, B, ldb, Cc, ldc, sols, infos, warm_start, false);
}

scs_int scs_amd_small_solve_values(ScsAmdSmall *s, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                   ScsSolution *sols, ScsInfo *infos, scs_int warm_start) {
  return small_solve(s, nprob, B, ldb, Cc, ldc, sols, infos, warm_start, true);
}

void scs_amd_small_free_values(ScsAmdSmall *s) {
  if (!s) return;
  if (s->on_device) (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (DevBuf<real> *b : {&s->vAv, &s->vAtv, &s->vPd, &s->vD, &s->vE, &s->slab}) b->release();
  std::vector<Scaling>().swap(s->vscal);
  s->slab_grid = 0;
  s->vals_nprob = 0;
}

// the checks of scs_amd_small_set_values: false, with the refusal said, when the call is not served
static bool small_set_accepts(const ScsAmdSmall *s, scs_int nprob, const scs_float *AX, scs_int ldax, const scs_float *PX, scs_int ldpx) {
  if (!s || !AX) return small_refuse("missing ScsAmdSmall or AX (a NULL argument)");
  if (PX && !s->has_P) return small_refuse("PX given, but the object was built without a P");
  if (!PX && s->has_P) return small_refuse("PX missing (a NULL argument): the object was built with a P");
  if (nprob < 1) return small_refuse("nprob < 1");
  const size_t nzA = (size_t)s->patA.p[s->n], nzP = s->has_P ? (size_t)s->patP.p[s->n] : 0;
  if ((long long)ldax < (long long)nzA || (s->has_P && (long long)ldpx < (long long)nzP))
    return small_refuse("short leading dimension: ldax < nnz(A) = %lld or ldpx < nnz(P) = %lld", (long long)nzA, (long long)nzP);
  for (scs_int p = 0; p < nprob; ++p)
    if ((nzA && !all_finite(AX + (size_t)p * (size_t)ldax, nzA)) || (nzP && !all_finite(PX + (size_t)p * (size_t)ldpx, nzP)))
      return small_refuse("non-finite values in AX or PX (problem %lld)", (long long)p);
  return true;
}

scs_int scs_amd_small_set_values(ScsAmdSmall *s, scs_int nprob, const scs_float *AX, scs_int ldax, const scs_float *PX, scs_int ldpx) {
  g_small_refused = false;
  if (!small_set_accepts(s, nprob, AX, ldax, PX, ldpx)) return SCS_FAILED;
  const int n = s->n, m = s->m;
  const size_t nzA = (size_t)s->patA.p[n], nzP = s->has_P ? (size_t)s->patP.p[n] : 0;
  scs_amd_small_free_values(s); // a second set call replaces the values; a failure below leaves none
  try {
    small_device_init(s);
    HIP_CHECK(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    if (s->grid_default_own == 0) s->grid_default_own = small_grid_default(s, true); // the own-values kernel, set up by the first set call
    const size_t wA = s->wA, wAt = s->wAt, szA = (size_t)m * wA, szAt = (size_t)n * wAt, szP = s->has_P ? (size_t)n * n : 0;
    if (s->mapA.size() != nzA || s->mapAt.size() != nzA) { // the slots small_ell gives the entries, in its order
      s->mapA.resize(nzA);
      s->mapAt.resize(nzA);
      std::vector<int> cr(m, 0);
      for (int j = 0; j < n; ++j)
        for (eoff e = s->patA.p[j]; e < s->patA.p[j + 1]; ++e) {
          const int r = s->patA.i[e];
          s->mapA[e] = (size_t)(cr[r]++) * m + r;
          s->mapAt[e] = (size_t)(e - s->patA.p[j]) * n + j;
        }
      s->mapP.resize(nzP);
      for (int j = 0; j < n && s->has_P; ++j)
        for (eoff e = s->patP.p[j]; e < s->patP.p[j + 1]; ++e) s->mapP[e] = (size_t)s->patP.i[e] * n + j;
    }
    const size_t K = (size_t)nprob;
    s->vAv.alloc(K * szA);
    s->vAtv.alloc(K * szAt);
    if (s->has_P) s->vPd.alloc(K * szP);
    s->vD.alloc(K * m);
    s->vE.alloc(K * n);
    s->vscal.resize(K);
    // staged in blocks of problems of about 32 MB; the padding of the rows and the zeros of P are written once
    const size_t per = szA + szAt + szP + m + n, blk = std::max<size_t>(1, std::min<size_t>(K, ((size_t)4 << 20) / per));
    std::vector<real> hAv(blk * szA, (real)0), hAtv(blk * szAt, (real)0), hPd(blk * szP, (real)0), hD(blk * m), hE(blk * n);
    HostCsc A = s->patA, P;
    if (s->has_P) P = s->patP;
    for (size_t p0 = 0; p0 < K; p0 += blk) {
      const size_t kb = std::min(blk, K - p0);
      for (size_t q = 0; q < kb; ++q) {
        const size_t p = p0 + q;
        Scaling &sc = s->vscal[p];
        std::copy(AX + p * (size_t)ldax, AX + p * (size_t)ldax + nzA, A.x.begin());
        if (s->has_P) std::copy(PX + p * (size_t)ldpx, PX + p * (size_t)ldpx + nzP, P.x.begin());
        small_equilibrate(s, s->has_P ? &P : nullptr, A, sc);
        real *av = hAv.data() + q * szA, *atv = hAtv.data() + q * szAt, *pd = hPd.data() + q * szP;
        for (size_t e = 0; e < nzA; ++e) {
          av[s->mapA[e]] = A.x[e];
          atv[s->mapAt[e]] = A.x[e];
        }
        for (size_t e = 0; e < nzP; ++e) {
          const size_t ij = s->mapP[e], i = ij / n, j = ij - i * n;
          pd[ij] = P.x[e];
          pd[j * n + i] = P.x[e];
        }
        std::copy(sc.D.begin(), sc.D.end(), hD.begin() + q * m);
        std::copy(sc.E.begin(), sc.E.end(), hE.begin() + q * n);
      }
      HIP_CHECK(hipMemcpyAsync(s->vAv.p + p0 * szA, hAv.data(), kb * szA * sizeof(real), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(s->vAtv.p + p0 * szAt, hAtv.data(), kb * szAt * sizeof(real), hipMemcpyHostToDevice, st));
      if (s->has_P) HIP_CHECK(hipMemcpyAsync(s->vPd.p + p0 * szP, hPd.data(), kb * szP * sizeof(real), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(s->vD.p + p0 * m, hD.data(), kb * m * sizeof(real), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipMemcpyAsync(s->vE.p + p0 * n, hE.data(), kb * n * sizeof(real), hipMemcpyHostToDevice, st));
      HIP_CHECK(hipStreamSynchronize(st)); // the staging is written again by the next block
    }
    s->vals_nprob = (long long)nprob;
  } catch (const std::exception &ex) {
    fprintf(stderr, "%s\n", ex.what());
    scs_amd_small_free_values(s);
    fprintf(stderr, "scs_amd_small_set_values: HIP error or failed allocation: no values are set\n");
    return SCS_FAILED;
  }
  return 0;
}

void scs_amd_small_finish(ScsAmdSmall *s) {
  if (!s) return;
  if (s->on_device) (void)hipSetDevice(s->device);
  delete s;
}

} // extern "C"
