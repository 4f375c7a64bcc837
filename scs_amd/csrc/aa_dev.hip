// aa_dev.hip -- device-resident Anderson acceleration of the ADMM fixed-point map
// (SURVEY.md 8f item 1).  Same algorithm and the same host-side decisions as the
// host version (aa_host.cpp, restating reference src/aa.c:236-967), but every
// O(dim) operation runs on the GPU and v / v_prev never leave HBM:
//
//   update_accel_params (aa.c:340-391)   one fused kernel: S, D, Y columns, g, the
//                                        x/f/g_prev copies and three sums of squares
//   solve (aa.c:422-655)                 column-pivoted Householder QR of [A; sqrt(r) I]
//                                        as a left-looking sweep over a tall-skinny
//                                        panel that ALSO carries [Y; sqrt(r) I] (type-I)
//                                        and [g; 0]: reflector k is applied to every
//                                        remaining column in one "dots" pass and one
//                                        "update" pass, so Q'[g;0] and Q'[Y;..] fall out
//                                        of the factorisation instead of being separate
//                                        ormqr sweeps.  Columns are never swapped in
//                                        memory (pivoting permutes indices), the
//                                        reflectors are never stored (nothing reads
//                                        them afterwards).
//   f -= D gamma, relaxation (:393-410)  one kernel
//   safeguard (aa.c:856-899)             one reduction, two D2D copies on rejection
//
// The host keeps what is O(mem^2): pivot choice with LAPACK-style norm downdating,
// reflector scalars, rank truncation, the mem x mem solve with iterative refinement and
// the accept / reject decision.  All of that is AaPanelCol of aa_small.h, which the block
// form (aa_multi.h) uses as well; this file adds the device buffers, the kernels and the
// sweep that feeds one small read-back per reflector to those decisions.  Each panel pass
// (build, dots, w, update) is one __device__ body with two entry points: the one here
// takes its arguments directly, the k_aam_* one of aa_multi.h resolves them per column.
// Reductions are two-level with fixed order (deterministic run to run); they are not
// the host's summation order, so device and host AA agree to rounding, not bitwise.
#include "aa_small.h"

namespace scsamd {

constexpr int AA_BATCH = 16; // columns carried per launch
constexpr int AA_GRID = 512; // workgroups per tall-skinny pass (= partials per column)

struct ColSet {
  int n;
  int col[AA_BATCH];
};

// ---- kernels ---------------------------------------------------------------------
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aa_seed(const real *__restrict__ x, const real *__restrict__ f, real *__restrict__ ax, real *__restrict__ af,
          real *__restrict__ g_prev, long dim) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += (long)gridDim.x * blockDim.x) {
    const real xi = x[i], fi = f[i];
    ax[i] = xi;
    af[i] = fi;
    g_prev[i] = xi - fi;
  }
}

// part: [3][gridDim.x] sums of squares of the new S column, Y column, g
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aa_update(const real *__restrict__ x, const real *__restrict__ f, real *__restrict__ ax, real *__restrict__ af,
            real *__restrict__ g, real *__restrict__ g_prev, real *__restrict__ sc, real *__restrict__ dc,
            real *__restrict__ yc, real *__restrict__ x_work, long dim, real *__restrict__ part) {
  __shared__ real sh[SCSAMD_BLOCK / 64];
  real ss = 0, sy = 0, sg = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += (long)gridDim.x * blockDim.x) {
    const real xi = x[i], fi = f[i];
    const real s = xi - ax[i], d = fi - af[i], gi = xi - fi, y = gi - g_prev[i];
    sc[i] = s;
    dc[i] = d;
    yc[i] = y;
    g[i] = gi;
    g_prev[i] = gi;
    ax[i] = xi;
    af[i] = fi;
    if (x_work) x_work[i] = xi;
    ss += s * s;
    sy += y * y;
    sg += gi * gi;
  }
  ss = block_sum(ss, sh);
  sy = block_sum(sy, sh);
  sg = block_sum(sg, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = ss;
    part[gridDim.x + blockIdx.x] = sy;
    part[2 * gridDim.x + blockIdx.x] = sg;
  }
}

// Panel columns: [0, mem) = [A_j; sqrt(r) e_j], [mem, 2 mem) = [Y_j; sqrt(r) e_j] (type-I
// only), last = [g; 0].  cy picks the column: 0..len-1: A, len..2len-1: B (type1), last: c
__device__ __forceinline__ void aa_build_body(real *__restrict__ Q, long ld, long dim, long aug, int mem, int len,
                                              int type1, int cy, const real *__restrict__ A_src,
                                              const real *__restrict__ Y, const real *__restrict__ g, real sqrt_r) {
  const real *src;
  int phys, unit;
  if (cy < len) {
    src = A_src + (size_t)cy * dim;
    phys = cy;
    unit = cy;
  } else if (type1 && cy < 2 * len) {
    src = Y + (size_t)(cy - len) * dim;
    phys = mem + (cy - len);
    unit = cy - len;
  } else {
    src = g;
    phys = type1 ? 2 * mem : mem;
    unit = -1;
  }
  real *dst = Q + (size_t)phys * ld;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < aug; i += (long)gridDim.x * blockDim.x) {
    real v;
    if (i < dim) v = src[i];
    else v = (unit >= 0 && i - dim == unit) ? sqrt_r : (real)0;
    dst[i] = v;
  }
}
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aa_build(real *__restrict__ Q, long ld, long dim, long aug, int mem, int len, int type1,
           const real *__restrict__ A_src, const real *__restrict__ Y, const real *__restrict__ g, real sqrt_r) {
  aa_build_body(Q, ld, dim, aug, mem, len, type1, blockIdx.y, A_src, Y, g, sqrt_r);
}

// part[c][wg] = sum_{i >= lo} Q[piv][i] * Q[col_c][i]
__device__ __forceinline__ void qr_dots_body(const real *__restrict__ Q, long ld, long aug, long lo, int piv, int n,
                                             const int *col, real *__restrict__ part) {
  __shared__ real sh[SCSAMD_BLOCK / 64][AA_BATCH];
  real acc[AA_BATCH];
#pragma unroll
  for (int c = 0; c < AA_BATCH; ++c) acc[c] = 0;
  const real *vp = Q + (size_t)piv * ld;
  for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < aug; i += (long)gridDim.x * blockDim.x) {
    const real v = vp[i];
#pragma unroll
    for (int c = 0; c < AA_BATCH; ++c)
      if (c < n) acc[c] += v * Q[(size_t)col[c] * ld + i];
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < AA_BATCH; ++c) {
    if (c < n) {
      const real s = wave_sum(acc[c]);
      if (l == 0) sh[w][c] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n) {
    real s = sh[0][threadIdx.x];
    for (int k = 1; k < SCSAMD_BLOCK / 64; ++k) s += sh[k][threadIdx.x];
    part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
  }
}
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_qr_dots(const real *__restrict__ Q, long ld, long aug, long lo, int piv, ColSet cs, real *__restrict__ part) {
  qr_dots_body(Q, ld, aug, lo, piv, cs.n, cs.col, part);
}

// one workgroup: w_c = tau (Q[col_c][k] + vscale * dot_c); Q[col_c][k] -= w_c; the new
// row-k entries go to info_ck (pivot norm downdating); R_kk = beta into the pivot column.
__device__ __forceinline__ void qr_w_body(real *__restrict__ Q, long ld, long k, int piv, real tau, real vscale, real beta,
                                          int set_beta, int n, const int *col, const real *__restrict__ part, int nparts,
                                          real *__restrict__ W, real *__restrict__ info_ck) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int c = w; c < n; c += SCSAMD_BLOCK / 64) {
    real s = 0;
    for (int i = l; i < nparts; i += 64) s += part[(size_t)c * nparts + i];
    s = wave_sum(s);
    if (l == 0) {
      real *e = Q + (size_t)col[c] * ld + k;
      const real ck = *e;
      const real wc = tau * (ck + vscale * s);
      *e = ck - wc;
      W[c] = wc;
      info_ck[c] = ck - wc;
    }
  }
  if (set_beta && threadIdx.x == 0) Q[(size_t)piv * ld + k] = beta;
}
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_qr_w(real *__restrict__ Q, long ld, long k, int piv, real tau, real vscale, real beta, int set_beta, ColSet cs,
       const real *__restrict__ part, int nparts, real *__restrict__ W, real *__restrict__ info_ck) {
  qr_w_body(Q, ld, k, piv, tau, vscale, beta, set_beta, cs.n, cs.col, part, nparts, W, info_ck);
}

// rows i >= lo of every column in the set: x -= W_c * vscale * Q[piv][i] (if do_update);
// statistics for the next pivot step: elem[c] = x at row lo, part_ss[c][wg] = sum of
// squares over rows > lo.
__device__ __forceinline__ void qr_update_body(real *__restrict__ Q, long ld, long aug, long lo, int piv, real vscale,
                                               int do_update, int n, const int *col, const real *__restrict__ W,
                                               real *__restrict__ part_ss, real *__restrict__ elem) {
  __shared__ real sh[SCSAMD_BLOCK / 64][AA_BATCH];
  real ss[AA_BATCH], wv[AA_BATCH];
#pragma unroll
  for (int c = 0; c < AA_BATCH; ++c) {
    ss[c] = 0;
    wv[c] = (do_update && c < n) ? W[c] : (real)0;
  }
  const real *vp = Q + (size_t)piv * ld;
  for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < aug; i += (long)gridDim.x * blockDim.x) {
    const real v = do_update ? vscale * vp[i] : (real)0;
#pragma unroll
    for (int c = 0; c < AA_BATCH; ++c) {
      if (c < n) {
        real *e = Q + (size_t)col[c] * ld + i;
        real x = *e;
        if (do_update) {
          x -= wv[c] * v;
          *e = x;
        }
        if (i > lo) ss[c] += x * x;
        else elem[c] = x;
      }
    }
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < AA_BATCH; ++c) {
    if (c < n) {
      const real s = wave_sum(ss[c]);
      if (l == 0) sh[w][c] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n) {
    real s = sh[0][threadIdx.x];
    for (int k = 1; k < SCSAMD_BLOCK / 64; ++k) s += sh[k][threadIdx.x];
    part_ss[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
  }
}
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_qr_update(real *__restrict__ Q, long ld, long aug, long lo, int piv, real vscale, int do_update, ColSet cs,
            const real *__restrict__ W, real *__restrict__ part_ss, real *__restrict__ elem) {
  qr_update_body(Q, ld, aug, lo, piv, vscale, do_update, cs.n, cs.col, W, part_ss, elem);
}

// f -= D gamma; with relaxation: x_work -= S gamma, f = relax f + (1-relax) x_work
__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aa_combine(real *__restrict__ f, const real *__restrict__ D, const real *__restrict__ S,
             real *__restrict__ x_work, const real *__restrict__ gamma, int len, long dim, real relaxation) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += (long)gridDim.x * blockDim.x) {
    real fi = f[i];
    for (int j = 0; j < len; ++j) {
      const real gj = gamma[j];
      if (gj != 0) fi -= D[(size_t)j * dim + i] * gj;
    }
    if (x_work) {
      real xw = x_work[i];
      for (int j = 0; j < len; ++j) {
        const real gj = gamma[j];
        if (gj != 0) xw -= S[(size_t)j * dim + i] * gj;
      }
      x_work[i] = xw;
      fi = relaxation * fi + ((real)1. - relaxation) * xw;
    }
    f[i] = fi;
  }
}

__global__ void __launch_bounds__(SCSAMD_BLOCK)
k_aa_diff_sumsq(const real *__restrict__ a, const real *__restrict__ b, long dim, real *__restrict__ part) {
  __shared__ real sh[SCSAMD_BLOCK / 64];
  real s = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < dim; i += (long)gridDim.x * blockDim.x) {
    const real d = a[i] - b[i];
    s += d * d;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- state -------------------------------------------------------------------------
struct AaDev : AaPanelCol {
  long dim = 0, aug = 0, ld = 0;
  hipStream_t stream = nullptr;
  int grid = 1;
  DevBuf<real> x, f, g, g_prev, x_work, Y, S, D, Q;
  DevBuf<real> part;  // [2 * max_batches][AA_BATCH][grid] partial sums
  DevBuf<real> small; // per batch: W[AA_BATCH] | ck[AA_BATCH] | elem[AA_BATCH]; then gamma[mem]
  PinnedBuf<real> h;  // read-back area
  int max_batches = 1;
  // offsets inside `small`
  real *Wd(int b) { return small.p + (size_t)b * 3 * AA_BATCH; }
  real *ckd(int b) { return Wd(b) + AA_BATCH; }
  real *elemd(int b) { return Wd(b) + 2 * AA_BATCH; }
  real *gammad() { return small.p + (size_t)max_batches * 3 * AA_BATCH; }
  real *part_dot(int b) { return part.p + (size_t)b * AA_BATCH * grid; }
  real *part_ss(int b) { return part.p + (size_t)(max_batches + b) * AA_BATCH * grid; }
};

AaDev *aa_dev_init(int dim, int mem, int min_len, int type1, real regularization, real relaxation,
                   real safeguard_factor, real max_weight_norm, int ir_max_steps, hipStream_t st) {
  if (!aa_params_ok(dim, mem, min_len, regularization, relaxation, safeguard_factor, max_weight_norm, ir_max_steps))
    return nullptr;
  AaDev *a = new AaDev();
  a->dim = dim;
  a->stream = st;
  try {
    a->init(dim, mem, min_len, type1, regularization, relaxation, safeguard_factor, max_weight_norm, ir_max_steps);
    if (a->mem <= 0) return a;
    a->init_panel();
    const size_t d = (size_t)dim, m = (size_t)a->mem;
    const int ncols = a->ncols();
    a->aug = dim + a->mem;
    a->ld = (a->aug + 7) & ~7L;
    a->grid = std::max(1, std::min(AA_GRID, ceil_div(a->aug, SCSAMD_BLOCK)));
    a->max_batches = ceil_div(ncols, AA_BATCH);
    a->x.alloc(d); a->f.alloc(d); a->g.alloc(d); a->g_prev.alloc(d);
    if (relaxation != (real)1.0) a->x_work.alloc(d);
    a->Y.alloc(d * m); a->S.alloc(d * m); a->D.alloc(d * m);
    a->Q.alloc((size_t)a->ld * ncols);
    a->part.alloc((size_t)2 * a->max_batches * AA_BATCH * a->grid + 3 * a->grid);
    a->small.alloc((size_t)a->max_batches * 3 * AA_BATCH + m);
    a->h.alloc(std::max((size_t)a->max_batches * (3 * AA_BATCH + (size_t)AA_BATCH * a->grid) + 3 * a->grid,
                        (size_t)ncols * m));
  } catch (const std::exception &e) {
    printf("Failed to allocate memory for AA (%s).\n", e.what());
    delete a;
    return nullptr;
  }
  return a;
}

void aa_dev_reset(AaDev *a) {
  if (a) a->reset();
}
void aa_dev_finish(AaDev *a) { delete a; }
void aa_dev_stats(const AaDev *a, AaStats *out) { a->stats(out); }

// ---- the panel sweep ---------------------------------------------------------------
static std::vector<ColSet> make_batches(const std::vector<int> &cols) {
  std::vector<ColSet> out;
  for (size_t i = 0; i < cols.size(); i += AA_BATCH) {
    ColSet cs;
    cs.n = (int)std::min((size_t)AA_BATCH, cols.size() - i);
    for (int c = 0; c < AA_BATCH; ++c) cs.col[c] = c < cs.n ? cols[i + c] : 0;
    out.push_back(cs);
  }
  return out;
}

// Statistics pass and/or reflector application over `cols`; afterwards E/SS (and CK when
// a reflector was applied) hold, per physical column, the row-lo entry, the sum of
// squares below it and the updated row-k entry.  `n_stat` = how many leading entries of
// `cols` the host needs back (the pivot candidates).
static void sweep(AaDev *a, const std::vector<int> &cols, int n_stat, long k, int piv, bool apply, real tau,
                  real vscale, real beta) {
  const std::vector<ColSet> bs = make_batches(cols);
  const long lo = k + 1;
  const int G = a->grid;
  for (size_t b = 0; b < bs.size(); ++b) {
    if (apply) {
      hipLaunchKernelGGL(k_qr_dots, dim3(G), dim3(SCSAMD_BLOCK), 0, a->stream, a->Q.p, a->ld, a->aug, lo, piv, bs[b],
                         a->part_dot((int)b));
      hipLaunchKernelGGL(k_qr_w, dim3(1), dim3(SCSAMD_BLOCK), 0, a->stream, a->Q.p, a->ld, k, piv, tau, vscale, beta,
                         b == 0 ? 1 : 0, bs[b], a->part_dot((int)b), G, a->Wd((int)b), a->ckd((int)b));
    }
    const bool need_stats = (int)(b * AA_BATCH) < n_stat;
    if (apply || need_stats)
      hipLaunchKernelGGL(k_qr_update, dim3(G), dim3(SCSAMD_BLOCK), 0, a->stream, a->Q.p, a->ld, a->aug, lo, piv, vscale,
                         apply ? 1 : 0, bs[b], a->Wd((int)b), a->part_ss((int)b), a->elemd((int)b));
  }
  HIP_CHECK(hipGetLastError());
  if (n_stat <= 0) return;
  const int nb = ceil_div(n_stat, AA_BATCH);
  real *h_small = a->h.p, *h_ss = a->h.p + (size_t)a->max_batches * 3 * AA_BATCH;
  HIP_CHECK(hipMemcpyAsync(h_small, a->small.p, (size_t)nb * 3 * AA_BATCH * sizeof(real), hipMemcpyDeviceToHost,
                           a->stream));
  HIP_CHECK(hipMemcpyAsync(h_ss, a->part_ss(0), (size_t)nb * AA_BATCH * G * sizeof(real), hipMemcpyDeviceToHost,
                           a->stream));
  HIP_CHECK(hipStreamSynchronize(a->stream));
  for (int i = 0; i < n_stat; ++i) {
    const int b = i / AA_BATCH, c = i % AA_BATCH, col = cols[i];
    const real *sm = h_small + (size_t)b * 3 * AA_BATCH;
    if (apply) a->CK[col] = sm[AA_BATCH + c];
    else a->CK[col] = a->E[col]; // row k untouched: it is the row-lo entry of the previous pass
    real s = 0;
    const real *ps = h_ss + ((size_t)b * AA_BATCH + c) * G;
    for (int w = 0; w < G; ++w) s += ps[w];
    a->E[col] = sm[2 * AA_BATCH + c];
    a->SS[col] = s;
  }
}

static real aa_dev_solve(real *f, AaDev *a, int len) {
  const long dim = a->dim;
  const int mem = a->mem;
  const real *A_src = a->type1 ? a->S.p : a->Y.p;
  const real r = a->regularization_r();
  const real sqrt_r = r > 0 ? std::sqrt(r) : (real)0;
  const int ncarry = (a->type1 ? len : 0) + 1;
  hipLaunchKernelGGL(k_aa_build, dim3(a->grid, len + ncarry), dim3(SCSAMD_BLOCK), 0, a->stream, a->Q.p, a->ld, dim,
                     a->aug, mem, len, a->type1, A_src, a->Y.p, a->g.p, sqrt_r);
  // carried (never pivoted) columns: B then c
  std::vector<int> carried;
  if (a->type1)
    for (int j = 0; j < len; ++j) carried.push_back(mem + j);
  carried.push_back(a->col_c());
  // initial statistics of the pivot candidates
  std::vector<int> cols;
  for (int j = 0; j < len; ++j) cols.push_back(j);
  sweep(a, cols, len, -1, 0, false, 0, 0, 0);
  a->pivot_begin(len);
  for (int k = 0; k < len; ++k) {
    const Reflector h = a->pivot_step(k, len);
    cols.clear();
    for (int j = k + 1; j < len; ++j) cols.push_back(a->jpvt[j]);
    const int n_stat = (int)cols.size();
    for (int c : carried) cols.push_back(c);
    sweep(a, cols, n_stat, k, a->jpvt[k], h.tau != 0, h.tau, h.scale, h.beta);
    a->pivot_downdate(k, len);
  }
  // top len rows of every panel column: R, W = top of Q'[Y_piv; ..], c_top
  const int ncols = a->ncols();
  HIP_CHECK(hipMemcpy2DAsync(a->h.p, (size_t)mem * sizeof(real), a->Q.p, (size_t)a->ld * sizeof(real),
                             (size_t)len * sizeof(real), ncols, hipMemcpyDeviceToHost, a->stream));
  HIP_CHECK(hipStreamSynchronize(a->stream));
  memcpy(a->top.data(), a->h.p, (size_t)ncols * mem * sizeof(real));
  const real aa_norm = a->solve_from_top(len, r);
  if (aa_norm < 0) return aa_norm;
  HIP_CHECK(hipMemcpyAsync(a->gammad(), a->gamma.data(), (size_t)len * sizeof(real), hipMemcpyHostToDevice, a->stream));
  const int g1 = std::max(1, std::min(4096, ceil_div(dim, SCSAMD_BLOCK)));
  hipLaunchKernelGGL(k_aa_combine, dim3(g1), dim3(SCSAMD_BLOCK), 0, a->stream, f, a->D.p, a->S.p,
                     a->x_work.p /* null unless relaxation != 1 */, a->gammad(), len, dim, a->relaxation);
  HIP_CHECK(hipGetLastError());
  // gamma lives in pageable host memory: make sure the copy has consumed it
  HIP_CHECK(hipStreamSynchronize(a->stream));
  a->success = 1;
  return aa_norm;
}

// f, x: device pointers (length dim) on the AA stream
real aa_dev_apply(real *f, const real *x, AaDev *a) { // aa.c:822-854
  real aa_norm = 0;
  const int len = std::min(a->iter, a->mem);
  const long dim = a->dim;
  a->success = 0;
  if (a->mem <= 0) return aa_norm;
  const int g1 = std::max(1, std::min(4096, ceil_div(dim, SCSAMD_BLOCK)));
  if (a->iter == 0) { // init_accel_params, aa.c:293-307
    hipLaunchKernelGGL(k_aa_seed, dim3(g1), dim3(SCSAMD_BLOCK), 0, a->stream, x, f, a->x.p, a->f.p, a->g_prev.p, dim);
    HIP_CHECK(hipGetLastError());
    a->iter++;
    return aa_norm;
  }
  { // update_accel_params, aa.c:340-391
    const int idx = (a->iter - 1) % a->mem;
    const int G = a->grid;
    real *p3 = a->part.p + (size_t)2 * a->max_batches * AA_BATCH * G;
    hipLaunchKernelGGL(k_aa_update, dim3(G), dim3(SCSAMD_BLOCK), 0, a->stream, x, f, a->x.p, a->f.p, a->g.p,
                       a->g_prev.p, a->S.p + (size_t)idx * dim, a->D.p + (size_t)idx * dim,
                       a->Y.p + (size_t)idx * dim, a->x_work.p, dim, p3);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(a->h.p, p3, (size_t)3 * G * sizeof(real), hipMemcpyDeviceToHost, a->stream));
    HIP_CHECK(hipStreamSynchronize(a->stream));
    real s3[3] = {0, 0, 0};
    for (int q = 0; q < 3; ++q)
      for (int w = 0; w < G; ++w) s3[q] += a->h.p[(size_t)q * G + w];
    a->nrm_s_col[idx] = std::sqrt(s3[0]);
    a->nrm_y_col[idx] = std::sqrt(s3[1]);
    a->norm_g = std::sqrt(s3[2]);
  }
  if (a->iter >= a->min_len) {
    aa_norm = aa_dev_solve(f, a, len);
    if (aa_norm > 0) a->st.n_accept++;
  }
  a->iter++;
  return aa_norm;
}

int aa_dev_safeguard(real *f_new, real *x_new, AaDev *a) { // aa.c:856-899
  if (a->mem <= 0 || !a->success) return 0;
  a->success = 0;
  const long dim = a->dim;
  const int G = a->grid;
  real *p3 = a->part.p + (size_t)2 * a->max_batches * AA_BATCH * G;
  hipLaunchKernelGGL(k_aa_diff_sumsq, dim3(G), dim3(SCSAMD_BLOCK), 0, a->stream, x_new, f_new, dim, p3);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(a->h.p, p3, (size_t)G * sizeof(real), hipMemcpyDeviceToHost, a->stream));
  HIP_CHECK(hipStreamSynchronize(a->stream));
  real s = 0;
  for (int w = 0; w < G; ++w) s += a->h.p[w];
  const real nd = std::sqrt(s);
  if (nd > a->safeguard_factor * a->norm_g) {
    HIP_CHECK(hipMemcpyAsync(f_new, a->f.p, dim * sizeof(real), hipMemcpyDeviceToDevice, a->stream));
    HIP_CHECK(hipMemcpyAsync(x_new, a->x.p, dim * sizeof(real), hipMemcpyDeviceToDevice, a->stream));
    a->st.n_safeguard_reject++;
    aa_dev_reset(a);
    return -1;
  }
  return 0;
}

} // namespace scsamd

// ---- C ABI: the device AA behind host pointers, so a test can pin it against the
// reference's aa_apply on the same sequences (vectors are staged through HBM per call;
// inside scs_solve the iterates are already resident) ---------------------------------
using namespace scsamd;
namespace {
struct AaDevHandle {
  AaDev *a = nullptr;
  hipStream_t st = nullptr;
  DevBuf<real> f, x;
  long dim = 0;
};
} // namespace
extern "C" {
void *scs_amd_aa_dev_init(scs_int dim, scs_int mem, scs_int min_len, scs_int type1, scs_float regularization,
                          scs_float relaxation, scs_float safeguard_factor, scs_float max_weight_norm,
                          scs_int ir_max_steps) {
  AaDevHandle *h = nullptr;
  try {
    h = new AaDevHandle();
    HIP_CHECK(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
    h->a = aa_dev_init(dim, mem, min_len, type1, regularization, relaxation, safeguard_factor, max_weight_norm,
                       ir_max_steps, h->st);
    if (!h->a) throw HipError("aa_dev_init failed");
    h->dim = dim;
    h->f.alloc(dim);
    h->x.alloc(dim);
    return h;
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    if (h) {
      if (h->a) aa_dev_finish(h->a);
      if (h->st) (void)hipStreamDestroy(h->st);
      delete h;
    }
    return nullptr;
  }
}
scs_float scs_amd_aa_dev_apply(scs_float *f, const scs_float *x, void *hv) {
  AaDevHandle *h = (AaDevHandle *)hv;
  try {
    h->f.upload(f, h->dim, h->st);
    h->x.upload(x, h->dim, h->st);
    const real nrm = aa_dev_apply(h->f.p, h->x.p, h->a);
    h->f.download(f, h->dim, h->st);
    HIP_CHECK(hipStreamSynchronize(h->st));
    return nrm;
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return (scs_float)NAN;
  }
}
scs_int scs_amd_aa_dev_safeguard(scs_float *f_new, scs_float *x_new, void *hv) {
  AaDevHandle *h = (AaDevHandle *)hv;
  try {
    h->f.upload(f_new, h->dim, h->st);
    h->x.upload(x_new, h->dim, h->st);
    const int rc = aa_dev_safeguard(h->f.p, h->x.p, h->a);
    h->f.download(f_new, h->dim, h->st);
    h->x.download(x_new, h->dim, h->st);
    HIP_CHECK(hipStreamSynchronize(h->st));
    return rc;
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    return -2;
  }
}
void scs_amd_aa_dev_reset(void *hv) { aa_dev_reset(((AaDevHandle *)hv)->a); }
void scs_amd_aa_dev_get_stats(const void *hv, AaStats *out) { aa_dev_stats(((const AaDevHandle *)hv)->a, out); }
void scs_amd_aa_dev_finish(void *hv) {
  AaDevHandle *h = (AaDevHandle *)hv;
  if (!h) return;
  if (h->st) (void)hipStreamSynchronize(h->st);
  if (h->a) aa_dev_finish(h->a);
  h->f.release();
  h->x.release();
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
}
}

#include "aa_multi.h"
