// aa_multi.h -- K independent Anderson accelerations in lock step (included at the end of aa_dev.hip).
//
// Column k computes what aa_dev_apply / aa_dev_safeguard compute for that column alone (reference src/aa.c:236-967); nothing
// couples the columns.  What they share is the launches and the read-backs: for reflector step j every column that is solving
// and has len_k > j takes its pivot and reflector scalars from ONE read-back, and every sweep kernel is enqueued ONCE with
// blockIdx.y = column and the per-column arguments (pivot, tau, scale, beta, column set) passed by value.  A column that seeds,
// fills its memory below min_len, is skipped or has run out of reflectors has n == 0 in that launch and returns at once.
//
// Where each piece lives.  The host side of a column -- counters, norms, AaStats, pivot choice with norm downdating, reflector
// scalars, and everything from the top rows of its panel to gamma and the accept / reject decision -- is AaPanelCol of
// aa_small.h, the same object the single-vector path derives from; for K == 1 the object holds a complete AaDev and runs that
// path itself.  The four panel passes (build, dots, w, update) are the __device__ bodies of aa_dev.hip behind entry points
// that pick their column's pointers and arguments out of AamArgs / AamBuild.  This file adds the kernels that touch the block
// layout, the device-side second reduction level, the lock-step sweep and the C ABI.
//
// Layout.  F and X arrive in the block layout of the other block entries (row-major, element (i, k) at i * W + k).  The state of a
// column -- S, D, Y, x, f, g, g_prev, x_work and its QR panel -- stays contiguous per column exactly as AaDev lays it out, because
// the sweeps address a different panel column per problem (its pivot, its ring slot).  The kernels that touch F / X (ingest =
// seed + update, combine, the safeguard's restore) transpose one tile of AAM_TILE rows through LDS: the block side is read and
// written contiguously over (i, k), the per-column side in runs of 64 consecutive rows per wave.
//
// Determinism.  Every reduction is two-level with a fixed order: one partial per workgroup, then one wave per value sums the
// partials on the device (k_aam_reduce), so a read-back carries one number per (column, panel column).  Grids depend on dim (and
// the object's width) only; the bits of a column depend neither on the other columns nor on its position.
#pragma once

namespace scsamd {

constexpr int AAM_KMAX = 16;  // widest block (MULTI_W_MAX of spmm.h)
constexpr int AAM_TILE = 128; // rows per transposition tile
constexpr int AAM_SMALL = 4 * AA_BATCH; // per (column, batch): w | row-k entry | row-lo entry | sum of squares

// width of the device layout for nrhs columns (multi_width of spmm.h): 1 for one column, 0 outside 1 .. 16
inline int aa_multi_width(long long nrhs) {
  if (nrhs < 1 || nrhs > AAM_KMAX) return 0;
  int w = 1;
  while (w < nrhs) w <<= 1;
  return w;
}

struct AamCol { // one column's share of a sweep launch; n == 0: nothing to do
  int n, apply, piv, set_beta;
  real tau, vscale, beta;
  int col[AA_BATCH];
};
struct AamArgs {
  AamCol c[AAM_KMAX];
};
struct AamSel { // column sets of the kernels that touch F / X, and one integer per column (ring slot, len)
  unsigned m0, m1;
  int v[AAM_KMAX];
};
struct AamBuild {
  int len[AAM_KMAX];
  real sqrt_r[AAM_KMAX];
};

// ---- kernels that touch the block layout ---------------------------------------------
// m0 = columns that seed (aa.c:293-307), m1 = columns that update (aa.c:340-391, ring slot v[k]).
// part: [AAM_KMAX][3][gridDim.x] sums of squares of the new S column, Y column, g.
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_ingest(const real *__restrict__ Xb, const real *__restrict__ Fb, int W, int wsh, long dim, AamSel sel,
             real *__restrict__ ax, real *__restrict__ af, real *__restrict__ g, real *__restrict__ g_prev,
             real *__restrict__ x_work, size_t vs, real *__restrict__ S, real *__restrict__ D, real *__restrict__ Y, size_t ms,
             real *__restrict__ part) {
  __shared__ real lx[AAM_TILE * (AAM_KMAX + 1)], lf[AAM_TILE * (AAM_KMAX + 1)];
  __shared__ real sh[SCSAMD_BLOCK / 64][3][AAM_KMAX / 2];
  const unsigned act = sel.m0 | sel.m1;
  const int P = W + 1, r = threadIdx.x & (AAM_TILE - 1), h = threadIdx.x >> 7;
  real acc[3][AAM_KMAX / 2];
#pragma unroll
  for (int c = 0; c < AAM_KMAX / 2; ++c) acc[0][c] = acc[1][c] = acc[2][c] = 0;
  const long ntiles = (dim + AAM_TILE - 1) / AAM_TILE;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long row0 = t * AAM_TILE;
    const int rows = (int)(dim - row0 < AAM_TILE ? dim - row0 : AAM_TILE);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * W; e += blockDim.x) {
      const int i = e >> wsh, k = e & (W - 1);
      if ((act >> k) & 1u) {
        lx[i * P + k] = Xb[(size_t)row0 * W + e];
        lf[i * P + k] = Fb[(size_t)row0 * W + e];
      }
    }
    __syncthreads();
    if (r < rows) {
#pragma unroll
      for (int c = 0; c < AAM_KMAX / 2; ++c) {
        const int k = 2 * c + h;
        if (k < W && ((act >> k) & 1u)) {
          const real xi = lx[r * P + k], fi = lf[r * P + k];
          const size_t o = (size_t)k * vs + row0 + r;
          if ((sel.m0 >> k) & 1u) {
            ax[o] = xi;
            af[o] = fi;
            g_prev[o] = xi - fi;
          } else {
            const size_t oc = (size_t)k * ms + (size_t)sel.v[k] * dim + row0 + r;
            const real s = xi - ax[o], d = fi - af[o], gi = xi - fi, y = gi - g_prev[o];
            S[oc] = s;
            D[oc] = d;
            Y[oc] = y;
            g[o] = gi;
            g_prev[o] = gi;
            ax[o] = xi;
            af[o] = fi;
            if (x_work) x_work[o] = xi;
            acc[0][c] += s * s;
            acc[1][c] += y * y;
            acc[2][c] += gi * gi;
          }
        }
      }
    }
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int c = 0; c < AAM_KMAX / 2; ++c) {
      const real s = wave_sum(acc[q][c]);
      if (l == 0) sh[w][q][c] = s;
    }
  __syncthreads();
  if (threadIdx.x < 3 * AAM_KMAX) { // waves 0, 1 hold the even columns, waves 2, 3 the odd ones
    const int q = threadIdx.x / AAM_KMAX, k = threadIdx.x % AAM_KMAX, hh = k & 1, c = k >> 1;
    part[((size_t)k * 3 + q) * gridDim.x + blockIdx.x] = sh[2 * hh][q][c] + sh[2 * hh + 1][q][c];
  }
}

// columns of m1 (v[k] = len): f -= D gamma; with relaxation: x_work -= S gamma, f = relax f + (1-relax) x_work
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_combine(real *__restrict__ Fb, int W, int wsh, long dim, AamSel sel, const real *__restrict__ gamma, int mem,
              const real *__restrict__ D, const real *__restrict__ S, size_t ms, real *__restrict__ x_work, size_t vs,
              real relaxation) {
  __shared__ real lf[AAM_TILE * (AAM_KMAX + 1)];
  const int P = W + 1, r = threadIdx.x & (AAM_TILE - 1), h = threadIdx.x >> 7;
  const long ntiles = (dim + AAM_TILE - 1) / AAM_TILE;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long row0 = t * AAM_TILE;
    const int rows = (int)(dim - row0 < AAM_TILE ? dim - row0 : AAM_TILE);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * W; e += blockDim.x) {
      const int i = e >> wsh, k = e & (W - 1);
      if ((sel.m1 >> k) & 1u) lf[i * P + k] = Fb[(size_t)row0 * W + e];
    }
    __syncthreads();
    if (r < rows) {
      for (int k = h; k < W; k += 2) {
        if (!((sel.m1 >> k) & 1u)) continue;
        const int len = sel.v[k];
        const real *gk = gamma + (size_t)k * mem;
        const size_t oc = (size_t)k * ms + row0 + r;
        real fi = lf[r * P + k];
        for (int j = 0; j < len; ++j) {
          const real gj = gk[j];
          if (gj != 0) fi -= D[oc + (size_t)j * dim] * gj;
        }
        if (x_work) {
          const size_t o = (size_t)k * vs + row0 + r;
          real xw = x_work[o];
          for (int j = 0; j < len; ++j) {
            const real gj = gk[j];
            if (gj != 0) xw -= S[oc + (size_t)j * dim] * gj;
          }
          x_work[o] = xw;
          fi = relaxation * fi + ((real)1. - relaxation) * xw;
        }
        lf[r * P + k] = fi;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * W; e += blockDim.x) {
      const int i = e >> wsh, k = e & (W - 1);
      if ((sel.m1 >> k) & 1u) Fb[(size_t)row0 * W + e] = lf[i * P + k];
    }
  }
}

// Both operands are in the block layout: no transposition.  gridDim.x * blockDim.x is a multiple of W, so a thread serves one
// column; part[k][wg] = sum over that workgroup's share of (x - f)^2 of column k (columns of m1 only).
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_diff_sumsq(const real *__restrict__ Xb, const real *__restrict__ Fb, int W, long dim, unsigned m1,
                 real *__restrict__ part) {
  __shared__ real sh[SCSAMD_BLOCK / 64][AAM_KMAX];
  const int k = threadIdx.x & (W - 1);
  const size_t n = (size_t)dim * W;
  real s = 0;
  if ((m1 >> k) & 1u)
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
      const real d = Xb[e] - Fb[e];
      s += d * d;
    }
  for (int o = 32; o >= W; o >>= 1) s += __shfl_down(s, o, 64); // lanes 0 .. W-1: the wave's sum of their column
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l < W) sh[w][l] = s;
  __syncthreads();
  if ((int)threadIdx.x < W) {
    real v = sh[0][threadIdx.x];
    for (int i = 1; i < SCSAMD_BLOCK / 64; ++i) v += sh[i][threadIdx.x];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = v;
  }
}

// safeguard rejection (aa.c:885-893): columns of m1 get f_new = f, x_new = x back
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_restore(real *__restrict__ Fb, real *__restrict__ Xb, int W, int wsh, long dim, unsigned m1,
              const real *__restrict__ af, const real *__restrict__ ax, size_t vs) {
  __shared__ real lx[AAM_TILE * (AAM_KMAX + 1)], lf[AAM_TILE * (AAM_KMAX + 1)];
  const int P = W + 1, r = threadIdx.x & (AAM_TILE - 1), h = threadIdx.x >> 7;
  const long ntiles = (dim + AAM_TILE - 1) / AAM_TILE;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long row0 = t * AAM_TILE;
    const int rows = (int)(dim - row0 < AAM_TILE ? dim - row0 : AAM_TILE);
    __syncthreads();
    if (r < rows)
      for (int k = h; k < W; k += 2)
        if ((m1 >> k) & 1u) {
          const size_t o = (size_t)k * vs + row0 + r;
          lf[r * P + k] = af[o];
          lx[r * P + k] = ax[o];
        }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * W; e += blockDim.x) {
      const int i = e >> wsh, k = e & (W - 1);
      if ((m1 >> k) & 1u) {
        Fb[(size_t)row0 * W + e] = lf[i * P + k];
        Xb[(size_t)row0 * W + e] = lx[i * P + k];
      }
    }
  }
}

// ---- the panel passes of aa_dev.hip, one column per blockIdx.y (build: blockIdx.z): entry points that resolve --------
// ---- their column's pointers and arguments and run the same bodies ------------------------------------------------
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_build(real *__restrict__ Q, size_t qs, long ld, long dim, long aug, int mem, int type1, AamBuild bd,
            const real *__restrict__ S, const real *__restrict__ Y, size_t ms, const real *__restrict__ g, size_t vs) {
  const int p = blockIdx.z, len = bd.len[p], cy = blockIdx.y;
  if (len == 0 || cy >= len + (type1 ? len : 0) + 1) return;
  aa_build_body(Q + (size_t)p * qs, ld, dim, aug, mem, len, type1, cy, (type1 ? S : Y) + (size_t)p * ms, Y + (size_t)p * ms,
                g + (size_t)p * vs, bd.sqrt_r[p]);
}

// part[p][c][wg] = sum_{i >= lo} Q_p[piv][i] * Q_p[col_c][i]
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_dots(const real *__restrict__ Qall, size_t qs, long ld, long aug, long lo, AamArgs a, real *__restrict__ part,
           size_t ps) {
  const int p = blockIdx.y, n = a.c[p].n;
  if (n == 0 || !a.c[p].apply) return;
  int col[AA_BATCH]; // out of the kernarg once (its offset depends on p), not once per row
#pragma unroll
  for (int c = 0; c < AA_BATCH; ++c) col[c] = a.c[p].col[c];
  qr_dots_body(Qall + (size_t)p * qs, ld, aug, lo, a.c[p].piv, n, col, part + (size_t)p * ps);
}

// one workgroup per column; small[p]: w | row-k entry
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_w(real *__restrict__ Qall, size_t qs, long ld, long k, AamArgs a, const real *__restrict__ part, size_t ps, int nparts,
        real *__restrict__ small, size_t ss) {
  const int p = blockIdx.y, n = a.c[p].n;
  if (n == 0 || !a.c[p].apply) return;
  real *sm = small + (size_t)p * ss;
  qr_w_body(Qall + (size_t)p * qs, ld, k, a.c[p].piv, a.c[p].tau, a.c[p].vscale, a.c[p].beta, a.c[p].set_beta, n, a.c[p].col,
            part + (size_t)p * ps, nparts, sm, sm + AA_BATCH);
}

// small[p][2 AA_BATCH + c] = x at row lo, part_ss[p][c][wg] = sum of squares over rows > lo
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_update(real *__restrict__ Qall, size_t qs, long ld, long aug, long lo, AamArgs a, real *__restrict__ part_ss, size_t ps,
             real *__restrict__ small, size_t ss) {
  const int p = blockIdx.y, n = a.c[p].n;
  if (n == 0) return;
  real *sm = small + (size_t)p * ss;
  int col[AA_BATCH];
#pragma unroll
  for (int c = 0; c < AA_BATCH; ++c) col[c] = a.c[p].col[c];
  qr_update_body(Qall + (size_t)p * qs, ld, aug, lo, a.c[p].piv, a.c[p].vscale, a.c[p].apply, n, col, sm, part_ss + (size_t)p * ps,
                 sm + 2 * AA_BATCH);
}

// second level of every reduction: one wave per value.  Value e (group q = e / grp, member c = e % grp) is the sum of the G
// partials at part[q * istride + c * G] and goes to out[q * ostride + c]; nothing but these values leaves the device.
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aam_reduce(const real *__restrict__ part, int G, int nent, int grp, size_t istride, size_t ostride,
             real *__restrict__ out) {
  const int e = blockIdx.x * (SCSAMD_BLOCK / 64) + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (e >= nent) return;
  const int q = e / grp, c = e % grp;
  const real *pp = part + (size_t)q * istride + (size_t)c * G;
  real s = 0;
  for (int i = l; i < G; i += 64) s += pp[i];
  s = wave_sum(s);
  if (l == 0) out[(size_t)q * ostride + c] = s;
}

// top len rows of every panel column of every solving column: out[p][col][mem]
__global__ void __launch_bounds__(64)
k_aam_top(const real *__restrict__ Q, size_t qs, long ld, int mem, AamBuild bd, real *__restrict__ out) {
  const int p = blockIdx.y, col = blockIdx.x, len = bd.len[p];
  for (int r = threadIdx.x; r < len; r += blockDim.x)
    out[((size_t)p * gridDim.x + col) * mem + r] = Q[(size_t)p * qs + (size_t)col * ld + r];
}

// ---- state -------------------------------------------------------------------------
struct AamStep { // one column's share of a lock-step sweep, host side
  bool on = false, apply = false;
  std::vector<int> cols;
  int n_stat = 0, piv = 0;
  real tau = 0, vscale = 0, beta = 0;
};

struct AaMulti {
  int K = 0, W = 0, wsh = 0, type1 = 1, mem = 0, ncols = 0, MB = 1;
  long dim = 0, aug = 0, ld = 0;
  real relaxation = 1;
  hipStream_t st = nullptr;
  int G = 1, gt = 1, gd = 1; // grids: panel passes, tile kernels, the safeguard's difference
  size_t vs = 0, ms = 0, qs = 0;
  // K == 1: col[0] is a complete AaDev on `st` (the single-vector path itself).  K > 1: col[k] is the host side of column k
  // (aa_small.h); the device side is below, column k at k * stride.
  std::vector<AaPanelCol *> col;
  AaDev *one() const { return static_cast<AaDev *>(col[0]); }
  DevBuf<real> x, f, g, g_prev, x_work, Y, S, D, Q;
  DevBuf<real> part;  // [K][2 MB][AA_BATCH][G] dot partials, then sum-of-squares partials; reused as [KMAX][3][gt] and [KMAX][gd]
  DevBuf<real> small; // [K][MB][AAM_SMALL]
  DevBuf<real> red, gamma, top;
  PinnedBuf<real> h, hg;
  bool idle = true;
  long long cnt[4] = {0, 0, 0, 0}; // block applies, syncs in applies, syncs in safeguards, kernel launches
  int sync_slot = 1;
  std::vector<AamStep> step;
  // staging of the host entries (created at their first use)
  DevBuf<real> Fb, Xb;
  std::vector<real> hF, hX;
  real *part_dot(int b) { return part.p + (size_t)b * AA_BATCH * G; }
  real *part_ss(int b) { return part.p + (size_t)(MB + b) * AA_BATCH * G; }
  size_t part_stride() const { return (size_t)2 * MB * AA_BATCH * G; }
};

#define AAM_LAUNCH(m, kern, grid, block, ...)                                                                                    \
  do {                                                                                                                           \
    hipLaunchKernelGGL(kern, grid, block, 0, (m)->st, __VA_ARGS__);                                                              \
    (m)->cnt[3]++;                                                                                                               \
    (m)->idle = false;                                                                                                           \
  } while (0)

static void aam_sync(AaMulti *m) {
  HIP_CHECK(hipStreamSynchronize(m->st));
  m->cnt[m->sync_slot]++;
  m->idle = true;
}

void aa_multi_finish(AaMulti *m) {
  if (!m) return;
  if (m->st) (void)hipStreamSynchronize(m->st);
  if (m->K == 1 && !m->col.empty()) aa_dev_finish(m->one());
  else
    for (AaPanelCol *a : m->col) delete a;
  hipStream_t st = m->st;
  delete m;
  if (st) (void)hipStreamDestroy(st);
}

AaMulti *aa_multi_init(int dim, int nrhs, int mem, int min_len, int type1, real regularization, real relaxation,
                       real safeguard_factor, real max_weight_norm, int ir_max_steps) {
  const int W = aa_multi_width(nrhs);
  const int memc = std::min(mem, dim);
  if (W == 0 || !aa_params_ok(dim, mem, min_len, regularization, relaxation, safeguard_factor, max_weight_norm, ir_max_steps))
    return nullptr;
  AaMulti *m = new AaMulti();
  try {
    HIP_CHECK(hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking));
    m->K = nrhs;
    m->W = W;
    while ((1 << m->wsh) < W) m->wsh++;
    m->type1 = type1;
    m->dim = dim;
    m->mem = memc;
    m->relaxation = relaxation;
    if (nrhs == 1) {
      AaDev *a = aa_dev_init(dim, mem, min_len, type1, regularization, relaxation, safeguard_factor, max_weight_norm,
                             ir_max_steps, m->st);
      if (!a) throw HipError("aa_dev_init failed");
      m->col.push_back(a);
      return m;
    }
    for (int k = 0; k < nrhs; ++k) {
      m->col.push_back(new AaPanelCol());
      m->col[k]->init(dim, mem, min_len, type1, regularization, relaxation, safeguard_factor, max_weight_norm, ir_max_steps);
      m->col[k]->init_panel();
    }
    m->ncols = m->col[0]->ncols();
    m->step.resize(nrhs);
    if (memc <= 0) return m;
    const size_t K = (size_t)nrhs, d = (size_t)dim, mm = (size_t)memc;
    m->aug = dim + memc;
    m->ld = (m->aug + 7) & ~7L;
    m->G = std::max(1, std::min(AA_GRID, ceil_div(m->aug, SCSAMD_BLOCK)));
    m->gt = std::max(1, std::min(AA_GRID, ceil_div(dim, AAM_TILE)));
    m->gd = std::max(1, std::min(AA_GRID, ceil_div((long long)dim * W, SCSAMD_BLOCK)));
    m->MB = ceil_div(m->ncols, AA_BATCH);
    m->vs = (d + 15) & ~(size_t)15;
    m->ms = (d * mm + 15) & ~(size_t)15;
    m->qs = (size_t)m->ld * m->ncols;
    m->x.alloc(K * m->vs); m->f.alloc(K * m->vs); m->g.alloc(K * m->vs); m->g_prev.alloc(K * m->vs);
    if (relaxation != (real)1.0) m->x_work.alloc(K * m->vs);
    m->Y.alloc(K * m->ms); m->S.alloc(K * m->ms); m->D.alloc(K * m->ms);
    m->Q.alloc(K * m->qs);
    m->part.alloc(std::max(K * m->part_stride(), (size_t)AAM_KMAX * 3 * std::max(m->gt, m->gd)));
    m->small.alloc(K * m->MB * AAM_SMALL);
    m->red.alloc((size_t)AAM_KMAX * 3);
    m->gamma.alloc(K * mm);
    m->top.alloc(K * m->ncols * mm);
    m->h.alloc(std::max(std::max(K * m->MB * AAM_SMALL, K * m->ncols * mm), (size_t)AAM_KMAX * 3));
    m->hg.alloc(K * mm);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    aa_multi_finish(m);
    return nullptr;
  }
  return m;
}

// ---- the lock-step sweep ------------------------------------------------------------
// Statistics pass and / or reflector application for every column with step[p].on, as sweep() of aa_dev.hip does it for one:
// afterwards E / SS (and CK when a reflector was applied) of each column hold, per physical panel column, the row-lo entry, the
// sum of squares below it and the updated row-k entry.  One read-back whatever the number of columns; none when no column
// has pivot candidates left.
static void aam_sweep(AaMulti *m, long k) {
  const long lo = k + 1;
  const int K = m->K, G = m->G;
  int nb = 0, nbs = 0;
  for (int p = 0; p < K; ++p) {
    const AamStep &s = m->step[p];
    if (!s.on) continue;
    nb = std::max(nb, ceil_div((long long)s.cols.size(), AA_BATCH));
    nbs = std::max(nbs, ceil_div(s.n_stat, AA_BATCH));
  }
  const size_t ps = m->part_stride(), ss = (size_t)m->MB * AAM_SMALL;
  for (int b = 0; b < nb; ++b) {
    AamArgs A;
    memset(&A, 0, sizeof A);
    bool any_apply = false, any = false;
    for (int p = 0; p < K; ++p) {
      const AamStep &s = m->step[p];
      const int first = b * AA_BATCH;
      if (!s.on || first >= (int)s.cols.size()) continue;
      if (!s.apply && first >= s.n_stat) continue;
      AamCol &c = A.c[p];
      c.n = std::min(AA_BATCH, (int)s.cols.size() - first);
      for (int i = 0; i < c.n; ++i) c.col[i] = s.cols[first + i];
      c.apply = s.apply ? 1 : 0;
      c.piv = s.piv;
      c.set_beta = b == 0 ? 1 : 0;
      c.tau = s.tau;
      c.vscale = s.vscale;
      c.beta = s.beta;
      any = true;
      any_apply = any_apply || s.apply;
    }
    if (any_apply) {
      AAM_LAUNCH(m, k_aam_dots, dim3(G, K), dim3(SCSAMD_BLOCK), m->Q.p, m->qs, m->ld, m->aug, lo, A, m->part_dot(b), ps);
      AAM_LAUNCH(m, k_aam_w, dim3(1, K), dim3(SCSAMD_BLOCK), m->Q.p, m->qs, m->ld, k, A, m->part_dot(b), ps, G,
                 m->small.p + (size_t)b * AAM_SMALL, ss);
    }
    if (any)
      AAM_LAUNCH(m, k_aam_update, dim3(G, K), dim3(SCSAMD_BLOCK), m->Q.p, m->qs, m->ld, m->aug, lo, A, m->part_ss(b), ps,
                 m->small.p + (size_t)b * AAM_SMALL, ss);
  }
  HIP_CHECK(hipGetLastError());
  if (nbs == 0) return;
  // sums of squares: part_ss [p][b][c][G] -> small[p][b][3 AA_BATCH + c], one launch per batch that has pivot candidates
  for (int b = 0; b < nbs; ++b)
    AAM_LAUNCH(m, k_aam_reduce, dim3(ceil_div((long long)K * AA_BATCH, SCSAMD_BLOCK / 64)), dim3(SCSAMD_BLOCK), m->part_ss(b),
               G, K * AA_BATCH, AA_BATCH, ps, ss, m->small.p + (size_t)b * AAM_SMALL + 3 * AA_BATCH);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(m->h.p, m->small.p, (size_t)K * ss * sizeof(real), hipMemcpyDeviceToHost, m->st));
  aam_sync(m);
  for (int p = 0; p < K; ++p) {
    const AamStep &s = m->step[p];
    if (!s.on) continue;
    AaPanelCol *a = m->col[p];
    for (int i = 0; i < s.n_stat; ++i) {
      const int b = i / AA_BATCH, c = i % AA_BATCH, col = s.cols[i];
      const real *sm = m->h.p + (size_t)p * ss + (size_t)b * AAM_SMALL;
      if (s.apply) a->CK[col] = sm[AA_BATCH + c];
      else a->CK[col] = a->E[col]; // row k untouched: it is the row-lo entry of the previous pass
      a->E[col] = sm[2 * AA_BATCH + c];
      a->SS[col] = sm[3 * AA_BATCH + c];
    }
  }
}

// solve (aa.c:422-655) of every column with len[p] > 0, in lock step; aa_norm[p] as aa_dev_solve returns it
static void aam_solve(AaMulti *m, real *Fb, const int *len, real *aa_norm) {
  const int K = m->K, mem = m->mem;
  AamBuild bd;
  memset(&bd, 0, sizeof bd);
  std::vector<real> reg(K, 0);
  int maxlen = 0;
  for (int p = 0; p < K; ++p) {
    if (len[p] <= 0) continue;
    const real r = m->col[p]->regularization_r();
    reg[p] = r;
    bd.len[p] = len[p];
    bd.sqrt_r[p] = r > 0 ? std::sqrt(r) : (real)0;
    maxlen = std::max(maxlen, len[p]);
  }
  AAM_LAUNCH(m, k_aam_build, dim3(m->G, (m->type1 ? 2 : 1) * maxlen + 1, K), dim3(SCSAMD_BLOCK), m->Q.p, m->qs, m->ld, m->dim,
             m->aug, mem, m->type1, bd, m->S.p, m->Y.p, m->ms, m->g.p, m->vs);
  // initial statistics of the pivot candidates
  for (int p = 0; p < K; ++p) {
    AamStep &s = m->step[p];
    s = AamStep();
    if (len[p] <= 0) continue;
    s.on = true;
    for (int j = 0; j < len[p]; ++j) s.cols.push_back(j);
    s.n_stat = len[p];
  }
  aam_sweep(m, -1);
  for (int p = 0; p < K; ++p) m->col[p]->pivot_begin(len[p]);
  for (int k = 0; k < maxlen; ++k) {
    for (int p = 0; p < K; ++p) {
      AamStep &s = m->step[p];
      s.on = len[p] > k;
      if (!s.on) continue;
      AaPanelCol *a = m->col[p];
      const int ln = len[p];
      const Reflector h = a->pivot_step(k, ln);
      s.cols.clear();
      for (int j = k + 1; j < ln; ++j) s.cols.push_back(a->jpvt[j]);
      s.n_stat = (int)s.cols.size();
      if (a->type1) // carried (never pivoted) columns: B then c
        for (int j = 0; j < ln; ++j) s.cols.push_back(mem + j);
      s.cols.push_back(a->col_c());
      s.piv = a->jpvt[k];
      s.apply = h.tau != 0;
      s.tau = h.tau;
      s.vscale = h.scale;
      s.beta = h.beta;
    }
    aam_sweep(m, k);
    for (int p = 0; p < K; ++p)
      if (len[p] > k) m->col[p]->pivot_downdate(k, len[p]);
  }
  // top rows of every panel column: R, W = top of Q'[Y_piv; ..], c_top
  const size_t tsz = (size_t)m->ncols * mem;
  AAM_LAUNCH(m, k_aam_top, dim3(m->ncols, K), dim3(64), m->Q.p, m->qs, m->ld, mem, bd, m->top.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(m->h.p, m->top.p, (size_t)K * tsz * sizeof(real), hipMemcpyDeviceToHost, m->st));
  aam_sync(m);
  AamSel sel;
  memset(&sel, 0, sizeof sel);
  for (int p = 0; p < K; ++p) {
    if (len[p] <= 0) continue;
    AaPanelCol *a = m->col[p];
    for (int c = 0; c < m->ncols; ++c)
      for (int rr = 0; rr < len[p]; ++rr) a->top[(size_t)c * mem + rr] = m->h.p[(size_t)p * tsz + (size_t)c * mem + rr];
    aa_norm[p] = a->solve_from_top(len[p], reg[p]);
    if (aa_norm[p] >= 0) {
      a->success = 1;
      sel.m1 |= 1u << p;
      sel.v[p] = len[p];
      memcpy(m->hg.p + (size_t)p * mem, a->gamma.data(), (size_t)len[p] * sizeof(real));
    }
  }
  if (!sel.m1) return;
  HIP_CHECK(hipMemcpyAsync(m->gamma.p, m->hg.p, (size_t)K * mem * sizeof(real), hipMemcpyHostToDevice, m->st));
  AAM_LAUNCH(m, k_aam_combine, dim3(m->gt), dim3(SCSAMD_BLOCK), Fb, m->W, m->wsh, m->dim, sel, m->gamma.p, mem, m->D.p, m->S.p,
             m->ms, m->x_work.p /* null unless relaxation != 1 */, m->vs, m->relaxation);
  HIP_CHECK(hipGetLastError());
}

// Fb, Xb: device pointers in the block layout; aa_apply (aa.c:822-854) of every column that is not skipped
static void aam_apply(AaMulti *m, real *Fb, const real *Xb, const int *skip, real *aa_norm) {
  const int K = m->K, mem = m->mem;
  m->sync_slot = 1;
  m->cnt[0]++;
  for (int p = 0; p < K; ++p) aa_norm[p] = 0;
  if (mem <= 0) return;
  AamSel sel;
  memset(&sel, 0, sizeof sel);
  for (int p = 0; p < K; ++p) {
    if (skip[p]) continue;
    AaPanelCol *a = m->col[p];
    a->success = 0;
    if (a->iter == 0) {
      sel.m0 |= 1u << p;
    } else {
      sel.m1 |= 1u << p;
      sel.v[p] = (a->iter - 1) % mem;
    }
  }
  if (!(sel.m0 | sel.m1)) return;
  // init_accel_params (aa.c:293-307) and update_accel_params (aa.c:340-391) in one launch
  AAM_LAUNCH(m, k_aam_ingest, dim3(m->gt), dim3(SCSAMD_BLOCK), Xb, Fb, m->W, m->wsh, m->dim, sel, m->x.p, m->f.p, m->g.p,
             m->g_prev.p, m->x_work.p, m->vs, m->S.p, m->D.p, m->Y.p, m->ms, m->part.p);
  HIP_CHECK(hipGetLastError());
  std::vector<int> len(K, 0);
  bool any_solve = false;
  if (sel.m1) {
    AAM_LAUNCH(m, k_aam_reduce, dim3(ceil_div(3 * K, SCSAMD_BLOCK / 64)), dim3(SCSAMD_BLOCK), m->part.p, m->gt, 3 * K, 3,
               (size_t)3 * m->gt, (size_t)3, m->red.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(m->h.p, m->red.p, (size_t)3 * K * sizeof(real), hipMemcpyDeviceToHost, m->st));
    aam_sync(m);
    for (int p = 0; p < K; ++p) {
      if (!((sel.m1 >> p) & 1u)) continue;
      AaPanelCol *a = m->col[p];
      const int idx = sel.v[p];
      a->nrm_s_col[idx] = std::sqrt(m->h.p[3 * p]);
      a->nrm_y_col[idx] = std::sqrt(m->h.p[3 * p + 1]);
      a->norm_g = std::sqrt(m->h.p[3 * p + 2]);
      if (a->iter >= a->min_len) {
        len[p] = std::min(a->iter, mem);
        any_solve = true;
      }
    }
  }
  if (any_solve) aam_solve(m, Fb, len.data(), aa_norm);
  for (int p = 0; p < K; ++p) {
    if (skip[p]) continue;
    AaPanelCol *a = m->col[p];
    if (aa_norm[p] > 0) a->st.n_accept++;
    a->iter++;
  }
  if (!m->idle) aam_sync(m); // also: the gamma upload has been consumed
}

// aa_safeguard (aa.c:856-899) of every column that is not skipped and whose last apply succeeded
static void aam_safeguard(AaMulti *m, real *Fb, real *Xb, const int *skip, int *rejected) {
  const int K = m->K;
  m->sync_slot = 2;
  unsigned test = 0, rej = 0;
  for (int p = 0; p < K; ++p) {
    rejected[p] = 0;
    AaPanelCol *a = m->col[p];
    if (skip[p] || m->mem <= 0 || !a->success) continue;
    a->success = 0;
    test |= 1u << p;
  }
  if (!test) return;
  AAM_LAUNCH(m, k_aam_diff_sumsq, dim3(m->gd), dim3(SCSAMD_BLOCK), Xb, Fb, m->W, m->dim, test, m->part.p);
  AAM_LAUNCH(m, k_aam_reduce, dim3(ceil_div(K, SCSAMD_BLOCK / 64)), dim3(SCSAMD_BLOCK), m->part.p, m->gd, K, K, (size_t)0,
             (size_t)0, m->red.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(m->h.p, m->red.p, (size_t)K * sizeof(real), hipMemcpyDeviceToHost, m->st));
  aam_sync(m);
  for (int p = 0; p < K; ++p) {
    if (!((test >> p) & 1u)) continue;
    AaPanelCol *a = m->col[p];
    const real nd = std::sqrt(m->h.p[p]);
    if (nd > a->safeguard_factor * a->norm_g) {
      rej |= 1u << p;
      rejected[p] = -1;
      a->st.n_safeguard_reject++;
      a->reset();
    }
  }
  if (!rej) return;
  AAM_LAUNCH(m, k_aam_restore, dim3(m->gt), dim3(SCSAMD_BLOCK), Fb, Xb, m->W, m->wsh, m->dim, rej, m->f.p, m->x.p, m->vs);
  HIP_CHECK(hipGetLastError());
  aam_sync(m);
}

} // namespace scsamd

// ---- C ABI (include/scs_amd.h) ----------------------------------------------------------
using namespace scsamd;
struct SCS_AMD_AA_MULTI {
  AaMulti *m = nullptr;
};
namespace {
// after a HIP failure: drain what was enqueued and start every column from an empty memory
void aam_fail(AaMulti *m, const std::exception &e) {
  fprintf(stderr, "%s\n", e.what());
  (void)hipStreamSynchronize(m->st);
  m->idle = true;
  for (AaPanelCol *a : m->col) a->reset();
}
void aam_flags(const AaMulti *m, const scs_int *skip, int *out) {
  for (int p = 0; p < m->K; ++p) out[p] = (skip && skip[p]) ? 1 : 0;
}
// the single-vector path itself, on the object's stream
void aam_apply_one(AaMulti *m, real *F_dev, const real *X_dev, const int *sk, scs_float *aa_norm) {
  m->cnt[0]++;
  aa_norm[0] = sk[0] ? (scs_float)0 : aa_dev_apply(F_dev, X_dev, m->one());
  HIP_CHECK(hipStreamSynchronize(m->st));
}
void aam_safeguard_one(AaMulti *m, real *F_dev, real *X_dev, const int *sk, scs_int *rejected) {
  rejected[0] = sk[0] ? 0 : (scs_int)aa_dev_safeguard(F_dev, X_dev, m->one());
  HIP_CHECK(hipStreamSynchronize(m->st));
}
void aam_stage(AaMulti *m) {
  const size_t n = (size_t)m->dim * m->W;
  if (m->Fb.p) return;
  m->hF.assign(n, 0);
  m->hX.assign(n, 0);
  m->Fb.alloc(n);
  m->Xb.alloc(n);
}
// host columns (column-major) <-> the block layout, columns that are not skipped only
void aam_pack(const AaMulti *m, const int *sk, const scs_float *src, scs_int lds, std::vector<real> &blk) {
  for (int p = 0; p < m->K; ++p)
    if (!sk[p])
      for (long i = 0; i < m->dim; ++i) blk[(size_t)i * m->W + p] = src[(size_t)p * lds + i];
}
void aam_unpack(const AaMulti *m, const int *sk, const std::vector<real> &blk, scs_float *dst, scs_int ldd) {
  for (int p = 0; p < m->K; ++p)
    if (!sk[p])
      for (long i = 0; i < m->dim; ++i) dst[(size_t)p * ldd + i] = blk[(size_t)i * m->W + p];
}
} // namespace

extern "C" {
scs_int scs_amd_aa_multi_width(scs_int nrhs) { return (scs_int)aa_multi_width((long long)nrhs); }

ScsAmdAaMulti *scs_amd_aa_multi_init(scs_int dim, scs_int nrhs, scs_int mem, scs_int min_len, scs_int type1,
                                     scs_float regularization, scs_float relaxation, scs_float safeguard_factor,
                                     scs_float max_weight_norm, scs_int ir_max_steps) {
  if (dim <= 0 || dim > 0x7fffffffLL - 64 || aa_multi_width((long long)nrhs) == 0 || mem < 0 || mem > 0xffff) return nullptr;
  ScsAmdAaMulti *h = nullptr;
  try {
    h = new ScsAmdAaMulti();
    h->m = aa_multi_init((int)dim, (int)nrhs, (int)mem, (int)min_len, (int)type1, regularization, relaxation, safeguard_factor,
                         max_weight_norm, (int)ir_max_steps);
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
  }
  if (h && !h->m) {
    delete h;
    h = nullptr;
  }
  return h;
}

scs_int scs_amd_aa_multi_apply_dev(ScsAmdAaMulti *a, scs_float *F_dev, const scs_float *X_dev, const scs_int *skip,
                                   scs_float *aa_norm) {
  if (!a || !a->m || !F_dev || !X_dev || !aa_norm) return -1;
  AaMulti *m = a->m;
  int sk[AAM_KMAX];
  aam_flags(m, skip, sk);
  try {
    if (m->K == 1) aam_apply_one(m, F_dev, X_dev, sk, aa_norm);
    else aam_apply(m, F_dev, X_dev, sk, aa_norm);
    return 0;
  } catch (const std::exception &e) {
    aam_fail(m, e);
    return -1;
  }
}

scs_int scs_amd_aa_multi_safeguard_dev(ScsAmdAaMulti *a, scs_float *F_dev, scs_float *X_dev, const scs_int *skip,
                                       scs_int *rejected) {
  if (!a || !a->m || !F_dev || !X_dev || !rejected) return -1;
  AaMulti *m = a->m;
  int sk[AAM_KMAX], rj[AAM_KMAX];
  aam_flags(m, skip, sk);
  try {
    if (m->K == 1) {
      aam_safeguard_one(m, F_dev, X_dev, sk, rejected);
    } else {
      aam_safeguard(m, F_dev, X_dev, sk, rj);
      for (int p = 0; p < m->K; ++p) rejected[p] = rj[p];
    }
    return 0;
  } catch (const std::exception &e) {
    aam_fail(m, e);
    return -1;
  }
}

scs_int scs_amd_aa_multi_apply(ScsAmdAaMulti *a, scs_float *F, scs_int ldf, const scs_float *X, scs_int ldx,
                               const scs_int *skip, scs_float *aa_norm) {
  if (!a || !a->m || !F || !X || !aa_norm || ldf < a->m->dim || ldx < a->m->dim) return -1;
  AaMulti *m = a->m;
  int sk[AAM_KMAX];
  aam_flags(m, skip, sk);
  try {
    aam_stage(m);
    const size_t n = (size_t)m->dim * m->W;
    aam_pack(m, sk, F, ldf, m->hF);
    aam_pack(m, sk, X, ldx, m->hX);
    m->Fb.upload(m->hF.data(), n, m->st);
    m->Xb.upload(m->hX.data(), n, m->st);
    HIP_CHECK(hipStreamSynchronize(m->st));
    if (m->K == 1) aam_apply_one(m, m->Fb.p, m->Xb.p, sk, aa_norm);
    else aam_apply(m, m->Fb.p, m->Xb.p, sk, aa_norm);
    m->Fb.download(m->hF.data(), n, m->st);
    HIP_CHECK(hipStreamSynchronize(m->st));
    aam_unpack(m, sk, m->hF, F, ldf);
    return 0;
  } catch (const std::exception &e) {
    aam_fail(m, e);
    return -1;
  }
}

scs_int scs_amd_aa_multi_safeguard(ScsAmdAaMulti *a, scs_float *F_new, scs_int ldf, scs_float *X_new, scs_int ldx,
                                   const scs_int *skip, scs_int *rejected) {
  if (!a || !a->m || !F_new || !X_new || !rejected || ldf < a->m->dim || ldx < a->m->dim) return -1;
  AaMulti *m = a->m;
  int sk[AAM_KMAX], rj[AAM_KMAX];
  aam_flags(m, skip, sk);
  try {
    aam_stage(m);
    const size_t n = (size_t)m->dim * m->W;
    aam_pack(m, sk, F_new, ldf, m->hF);
    aam_pack(m, sk, X_new, ldx, m->hX);
    m->Fb.upload(m->hF.data(), n, m->st);
    m->Xb.upload(m->hX.data(), n, m->st);
    HIP_CHECK(hipStreamSynchronize(m->st));
    if (m->K == 1) {
      aam_safeguard_one(m, m->Fb.p, m->Xb.p, sk, rejected);
      rj[0] = (int)rejected[0];
    } else {
      aam_safeguard(m, m->Fb.p, m->Xb.p, sk, rj);
      for (int p = 0; p < m->K; ++p) rejected[p] = rj[p];
    }
    bool any = false;
    for (int p = 0; p < m->K; ++p) {
      sk[p] = rj[p] == 0; // only a rejected column changed
      any = any || rj[p] != 0;
    }
    if (any) {
      m->Fb.download(m->hF.data(), n, m->st);
      m->Xb.download(m->hX.data(), n, m->st);
      HIP_CHECK(hipStreamSynchronize(m->st));
      aam_unpack(m, sk, m->hF, F_new, ldf);
      aam_unpack(m, sk, m->hX, X_new, ldx);
    }
    return 0;
  } catch (const std::exception &e) {
    aam_fail(m, e);
    return -1;
  }
}

void scs_amd_aa_multi_reset(ScsAmdAaMulti *a, scs_int col) {
  if (!a || !a->m) return;
  for (int p = 0; p < a->m->K; ++p)
    if (col < 0 || col == p) a->m->col[p]->reset();
}
void scs_amd_aa_multi_get_stats(const ScsAmdAaMulti *a, scs_int col, AaStats *out) {
  if (!a || !a->m || !out || col < 0 || col >= a->m->K) return;
  a->m->col[col]->stats(out);
}
void scs_amd_aa_multi_get_counters(const ScsAmdAaMulti *a, long long out[4]) {
  if (!a || !a->m || !out) return;
  for (int i = 0; i < 4; ++i) out[i] = a->m->cnt[i];
}
void scs_amd_aa_multi_finish(ScsAmdAaMulti *a) {
  if (!a) return;
  aa_multi_finish(a->m);
  delete a;
}
}
