// cones_multi.h -- the dual-cone projection of K vectors at once on one workspace (part of cones.hip: included there, behind
// the single-vector projection whose kernels and helpers it uses).
//
// Column k computes what ConeDev::proj_dual computes for that column alone: the Moreau wrapper of reference src/cones.c:1552-1596
// around proj_cone (:1340-1394).  The columns share the cone description and r_y and nothing else: every reduction runs over the
// lanes and partials of one column only, in an order that does not depend on the column's position, so the bits of a column do
// not depend on its neighbours.  No floating-point atomics.
//
// Layout: the block layout of spmm.h / linsys_multi.h -- row-major, element (i, k) at i * W + k, W the smallest of {2, 4, 8, 16}
// that is >= K -- so a block passes between the block solve and this projection as it is.  Padding columns k >= K are set to
// zero by the first pass and stay zero (the projection of 0 is 0 for every cone carried here).
//
// Native on the interleaved block, launch for launch what the single-vector path issues (lane -> (row or cone l / W, column l % W),
// the W lanes of a group touch W contiguous values):
//   k_m_moreau_pre / k_m_moreau_post   k_m_zero_pos   k_m_soc_tiny   k_m_exp_pow
//   k_m_soc_tile_partial / k_m_soc_finalize / k_m_soc_tile_apply: a workgroup takes a tile of SOC_TILE rows x W columns; the lanes of
//     a column are combined by __shfl_xor at strides 32 .. W (the butterfly of csr_block_kernel), the waves in wave order, and the
//     per-tile partials of a column are re-reduced in tile order by one lane.
// Through a column-major copy of the rows concerned (k_m_rows_to_cols / k_m_cols_to_rows) and the single-vector device code:
//   PSD blocks of order <= PSD_LDS_KMAX: the blocks of ALL columns in one launch of k_psd_jacobi (offset tables replicated per
//     column, eigenbasis and warm-start scratch per (column, block));
//   the box cone and PSD blocks beyond the LDS path: column after column, each on the state of its column position.
// Carried state (Newton start of the box cone, eigenbases, the cold-restart counter) belongs to the column position at one width;
// a change of width starts cold.  Nothing here reads or writes the state of the single-vector path.
//
// A column under its own r_y (proj_primal_multi's own_ry, for scs_amd_solve_family_scaled): only the box cone reads r_y inside the
// projection, so set_multi_ry keeps a column-major copy of the box rows of an m x W block of r_y's and launch_box gets column k's
// slice of it.  The public scs_amd_cone_proj_dual_multi keeps its one shared r_y: its Moreau passes would need the block as well,
// and no caller asks for it.
#pragma once

namespace scsamd {

constexpr int CONE_W_MAX = 16; // widest block (MULTI_W_MAX of spmm.h)

// width of the device layout for nrhs columns (multi_width of spmm.h): 1 for one column, 0 outside 1 .. 16
inline int cone_multi_width(long long nrhs) {
  if (nrhs < 1 || nrhs > CONE_W_MAX) return 0;
  int w = 1;
  while (w < nrhs) w <<= 1;
  return w;
}

// sum over the lanes of a workgroup that serve the same column (lane l: column l % W): fixed butterfly inside a wave, then the
// waves in wave order.  `sh` holds (blockDim.x / 64) * W entries; every lane of a column receives the same bits.
template <int W, typename T> __device__ __forceinline__ T cone_col_sum(T v, T *sh) {
#pragma unroll
  for (int o = 32; o >= W; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6, col = l & (W - 1);
  __syncthreads();
  if (l < W) sh[w * W + l] = v;
  __syncthreads();
  T s = sh[col];
  for (int i = 1; i < nw; ++i) s += sh[i * W + col];
  return s;
}

// ---- Moreau pre / post (cones.c:1567-1593) on the block; padding columns become zero ----------------------------------------
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_moreau_pre(real *x, real *s, const real *__restrict__ ry, int m, int K) {
  const size_t tot = (size_t)m * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const real xi = (int)(f & (W - 1)) < K ? x[f] : (real)0;
    s[f] = xi;
    x[f] = ry ? xi * (-ry[f / W]) : -xi;
  }
}
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_moreau_post(real *x, const real *__restrict__ s, const real *__restrict__ ry, int m, int K) {
  const size_t tot = (size_t)m * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const real v = ry ? x[f] / ry[f / W] + s[f] : x[f] + s[f];
    x[f] = (int)(f & (W - 1)) < K ? v : (real)0;
  }
}

// zero cone -> 0, nonnegative orthant -> max(x, 0)   (cones.c:1349-1359)
template <int W> __global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_zero_pos(real *x, int z, int l) {
  const size_t tot = (size_t)(z + l) * W, zw = (size_t)z * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    if (f < zw) x[f] = 0;
    else {
      const real v = x[f];
      x[f] = v > (real)0 ? v : (real)0;
    }
  }
}

// ---- second-order cones ---------------------------------------------------------------------------------------------------------
// one lane per (tiny cone, column); case analysis and summation order of proj_soc (cones.c:1250-1279), as k_soc_tiny
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_soc_tiny(real *x, const int *__restrict__ off, const int *__restrict__ len, int ncones) {
  const size_t tot = (size_t)ncones * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const int c = (int)(f / W);
    real *xc = x + (size_t)off[c] * W + (f & (W - 1)); // entry j of the cone at xc[j * W]
    const int q = len[c];
    if (q <= 0) continue;
    if (q == 1) {
      xc[0] = xc[0] > (real)0 ? xc[0] : (real)0;
      continue;
    }
    const real v1 = xc[0];
    real s;
    if (q == 2) s = absval(xc[W]);
    else {
      real ss = 0;
      for (int j = 1; j < q; ++j) ss += xc[(size_t)j * W] * xc[(size_t)j * W];
      s = sqrt(ss);
    }
    real head, mult;
    soc_decide(v1, s, head, mult);
    if (mult == (real)1 && head == v1) continue;
    xc[0] = head;
    if (mult == (real)0)
      for (int j = 1; j < q; ++j) xc[(size_t)j * W] = 0;
    else
      for (int j = 1; j < q; ++j) xc[(size_t)j * W] *= mult;
  }
}

// pass 1: per (tile, column) the sum of squares of the tail entries -> part[t * W + col]
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_soc_tile_partial(const real *__restrict__ x, const int *__restrict__ tile_off,
                                                                     const int *__restrict__ tile_len, const int *__restrict__ tile_cone,
                                                                     const int *__restrict__ big_off, real *part, int ntiles) {
  __shared__ real red[(SCSAMD_BLOCK / SCSAMD_WAVE) * W];
  const int col = threadIdx.x & (W - 1), r0 = threadIdx.x / W;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int o = tile_off[t], n = tile_len[t];
    const int head = big_off[tile_cone[t]];
    real ss = 0;
    for (int j = r0; j < n; j += SCSAMD_BLOCK / W) { // consecutive lanes, consecutive addresses
      const real v = x[(size_t)(o + j) * W + col];
      if (o + j != head) ss += v * v;
    }
    ss = cone_col_sum<W>(ss, red);
    if (threadIdx.x < W) part[(size_t)t * W + threadIdx.x] = ss;
  }
}
// pass 2: one lane per (cone, column); the cone's tiles in index order -> coef[(2 c) * W + col] = head, [(2 c + 1) * W + col] = multiplier
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_soc_finalize(const real *__restrict__ x, const int *__restrict__ big_off,
                                                                 const int *__restrict__ big_tile0, const real *__restrict__ part, real *coef,
                                                                 int ncones) {
  const size_t tot = (size_t)ncones * W, gs = (size_t)gridDim.x * blockDim.x;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < tot; f += gs) {
    const int c = (int)(f / W), col = (int)(f & (W - 1));
    real ss = 0;
    for (int t = big_tile0[c]; t < big_tile0[c + 1]; ++t) ss += part[(size_t)t * W + col];
    const real s = sqrt(ss), v1 = x[(size_t)big_off[c] * W + col];
    real head, mult;
    soc_decide(v1, s, head, mult);
    coef[(size_t)(2 * c) * W + col] = head;
    coef[(size_t)(2 * c + 1) * W + col] = mult;
  }
}
// pass 3: apply
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_soc_tile_apply(real *x, const int *__restrict__ tile_off, const int *__restrict__ tile_len,
                                                                   const int *__restrict__ tile_cone, const int *__restrict__ big_off,
                                                                   const real *__restrict__ coef, int ntiles) {
  const int col = threadIdx.x & (W - 1), r0 = threadIdx.x / W;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int o = tile_off[t], n = tile_len[t], c = tile_cone[t];
    const int head = big_off[c];
    const real hv = coef[(size_t)(2 * c) * W + col], mult = coef[(size_t)(2 * c + 1) * W + col];
    if (mult == (real)1) continue; // this column is inside the cone: untouched (head == v1)
    for (int j = r0; j < n; j += SCSAMD_BLOCK / W) {
      const size_t f = (size_t)(o + j) * W + col;
      if (o + j == head) x[f] = hv;
      else x[f] = mult == (real)0 ? (real)0 : x[f] * mult;
    }
  }
}

// ---- exponential, dual exponential and power cones: one lane per (cone, column), the per-lane arithmetic of k_exp_pow ---------
// x: the block at the first exp/pow row.  Whole waves stay in the loop (the root searches of cones_exp_pow.h vote over the wave;
// a lane that is done is frozen by its own predicate, so its bits do not depend on the lanes beside it).
template <int W>
__global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_exp_pow(real *x, int ep, int ed, int psize, const real *__restrict__ pw) {
  const size_t tot = (size_t)(ep + ed + psize) * W, gs = (size_t)gridDim.x * blockDim.x;
  const size_t rounded = (tot + SCSAMD_BLOCK - 1) / SCSAMD_BLOCK * SCSAMD_BLOCK;
  for (size_t f = (size_t)blockIdx.x * blockDim.x + threadIdx.x; f < rounded; f += gs) {
    const bool have = f < tot;
    const int c = have ? (int)(f / W) : 0;
    real *xc = x + (size_t)3 * c * W + (f & (W - 1));
    Triple v{(real)0, (real)0, (real)0};
    if (have) v = Triple{xc[0], xc[W], xc[2 * W]};
    const bool is_exp = have && c < ep + ed, is_pow = have && !is_exp;
    Triple out = v;
    if (XP_ANY(is_exp)) {
      const Triple r = xp::project_exp(v, is_exp, is_exp && c >= ep);
      if (is_exp) out = r;
    }
    if (XP_ANY(is_pow)) {
      const xreal a_raw = is_pow ? pw[c - ep - ed] : (xreal)0.5;
      const bool dualp = a_raw < 0; // dual power cone: Moreau, v + Proj_K(-v) (cones.c:1427-1441)
      const xreal a = dualp ? -a_raw : a_raw;
      const Triple in{dualp ? -v.u : v.u, dualp ? -v.w : v.w, dualp ? -v.t : v.t};
      const Triple r = xp::project_pow(in, a, is_pow);
      if (is_pow) {
        out.u = dualp ? v.u + r.u : r.u;
        out.w = dualp ? v.w + r.w : r.w;
        out.t = dualp ? v.t + r.t : r.t;
      }
    }
    if (have) {
      xc[0] = out.u;
      xc[W] = out.w;
      xc[2 * W] = out.t;
    }
  }
}

// ---- rows [r0, r1) of the block <-> W columns of length m, column major (the layout the single-vector device code works on) ----
// A workgroup moves a tile of CONE_TR rows x W columns through LDS, so that both sides are unit stride: on the block side lane t
// touches element t of the tile (row t / W, column t % W), on the column side lane t touches row t % CONE_TR of column t / CONE_TR.
constexpr int CONE_TR = 64;
template <int W> __global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_rows_to_cols(const real *__restrict__ X, real *cols, int m, int r0, int r1) {
  __shared__ real tile[CONE_TR * (W + 1)];
  const int ntiles = (r1 - r0 + CONE_TR - 1) / CONE_TR;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int i0 = r0 + t * CONE_TR, nr = r1 - i0 < CONE_TR ? r1 - i0 : CONE_TR;
    for (int e = threadIdx.x; e < nr * W; e += SCSAMD_BLOCK) tile[(e / W) * (W + 1) + (e & (W - 1))] = X[(size_t)i0 * W + e];
    __syncthreads();
    for (int e = threadIdx.x; e < CONE_TR * W; e += SCSAMD_BLOCK) {
      const int k = e / CONE_TR, r = e & (CONE_TR - 1);
      if (r < nr) cols[(size_t)k * m + i0 + r] = tile[r * (W + 1) + k];
    }
    __syncthreads();
  }
}
template <int W> __global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cols_to_rows(real *X, const real *__restrict__ cols, int m, int r0, int r1) {
  __shared__ real tile[CONE_TR * (W + 1)];
  const int ntiles = (r1 - r0 + CONE_TR - 1) / CONE_TR;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int i0 = r0 + t * CONE_TR, nr = r1 - i0 < CONE_TR ? r1 - i0 : CONE_TR;
    for (int e = threadIdx.x; e < CONE_TR * W; e += SCSAMD_BLOCK) {
      const int k = e / CONE_TR, r = e & (CONE_TR - 1);
      if (r < nr) tile[r * (W + 1) + k] = cols[(size_t)k * m + i0 + r];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nr * W; e += SCSAMD_BLOCK) X[(size_t)i0 * W + e] = tile[(e / W) * (W + 1) + (e & (W - 1))];
    __syncthreads();
  }
}
// host entry: K columns of length m, column major with leading dimension m <-> the block; padding columns become zero
template <int W> __global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cone_to_block(const real *__restrict__ src, real *X, int m, int K) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    real *d = X + (size_t)i * W;
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = k < K ? src[(size_t)k * m + i] : (real)0;
  }
}
template <int W> __global__ __launch_bounds__(SCSAMD_BLOCK) void k_m_cone_from_block(real *dst, const real *__restrict__ X, int m, int K) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const real *s = X + (size_t)i * W;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (k < K) dst[(size_t)k * m + i] = s[k];
  }
}

// ---- host side (the width switch is MULTI_DISPATCH, common.h) -------------------------------------------------------------------
ConeMulti::~ConeMulti() {
  for (BigPsd *b : big) delete b;
}

// state and staging of block projections at width W: built at the first block call, rebuilt (cold) when the width changes
void ConeDev::ensure_multi(int W) {
  if (multi && multi->width == W) return;
  if ((long long)m * W > 2147483647LL) throw HipError("scs_amd: block of cone vectors exceeds 32-bit device indexing");
  delete multi;
  multi = nullptr;
  ConeMulti *mc = new ConeMulti();
  try {
    const size_t mw = (size_t)m * W;
    mc->s.alloc(mw ? mw : 1);
    mc->cols.alloc(mw ? mw : 1);
    mc->tile_part.alloc(n_tiles ? (size_t)n_tiles * W : 1);
    mc->big_coef.alloc(n_big ? 2 * (size_t)n_big * W : 2);
    std::vector<real> ones(W, (real)1); // cones.c:1560
    mc->box_t.alloc(W);
    mc->box_t.upload(ones.data(), W, stream);
    if (n_psd) {
      // the offset tables of k_psd_jacobi, replicated per column: block j of column k starts at k * m + psd_off[j] of the column copy
      std::vector<int> ho(n_psd), hk(n_psd), mo((size_t)n_psd * W), mk((size_t)n_psd * W);
      HIP_CHECK(hipMemcpyAsync(ho.data(), psd_off.p, n_psd * sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipMemcpyAsync(hk.data(), psd_k.p, n_psd * sizeof(int), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      for (int k = 0; k < W; ++k)
        for (int j = 0; j < n_psd; ++j) {
          mo[(size_t)k * n_psd + j] = k * m + ho[j];
          mk[(size_t)k * n_psd + j] = hk[j];
        }
      mc->psd_off.alloc(mo.size());
      mc->psd_k.alloc(mk.size());
      mc->psd_off.upload(mo.data(), mo.size(), stream);
      mc->psd_k.upload(mk.data(), mk.size(), stream);
      if (psd_vprev.p) { // the warm start of the LDS kernel, as the single-vector path sized and gated it (ConeDev::init)
        const size_t per_cone = (size_t)((psd_lds_kmax + 1) & ~1) * (((psd_lds_kmax + 1) & ~1) | 1);
        mc->psd_vprev.alloc((size_t)W * n_psd * per_cone);
        if (psd_tscratch.p) mc->psd_tscratch.alloc((size_t)W * n_psd * per_cone);
      }
      if (psd_big)
        for (int k = 0; k < W; ++k) {
          mc->big.push_back(new BigPsd);
          mc->big.back()->init(hk, PSD_LDS_KMAX, stream);
        }
    }
    HIP_CHECK(hipStreamSynchronize(stream)); // the tables above are read from host vectors that end here
  } catch (...) {
    delete mc;
    throw;
  }
  mc->width = W;
  multi = mc;
}

// X (device, m x W block) <- its K columns projected onto the dual cone under the r_y metric; columns K .. W - 1 <- 0
void ConeDev::proj_dual_multi(real *X, int W, int K, const real *r_y) {
  ensure_multi(W);
  ConeMulti &mc = *multi;
  const int g = small_grid((long long)m * W);
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_moreau_pre<MW>, dim3(g), dim3(SCSAMD_BLOCK), 0, stream, X, mc.s.p, r_y, m, K));
  proj_primal_multi(X, W, K, r_y);
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_moreau_post<MW>, dim3(g), dim3(SCSAMD_BLOCK), 0, stream, X, mc.s.p, r_y, m, K));
}

// the block state back to what ensure_multi leaves: every column position starts its box Newton iteration and its eigenbases cold
void ConeDev::reset_multi_cold() {
  if (!multi) return;
  ConeMulti &mc = *multi;
  const std::vector<real> ones(mc.width, (real)1); // cones.c:1560
  mc.box_t.upload(ones.data(), mc.width, stream);
  HIP_CHECK(hipStreamSynchronize(stream)); // `ones` ends here
  mc.psd_calls = 0;
  for (BigPsd *b : mc.big) b->reset_warm_start();
}

// Column position k alone starts its box Newton iteration at 1 again (cones.c:1560): a position that takes another problem while
// its neighbours run on (scs_amd_solve_family_stream).  The other cones carried here keep nothing between projections except the
// PSD eigenbases, whose cold-restart counter belongs to the width: a caller with PSD blocks uses reset_multi_cold.
void ConeDev::reset_multi_box_start(int k) {
  if (!multi || bsize <= 0 || k < 0 || k >= multi->width) return;
  static const real one = 1; // static: the copy may run after this returns
  HIP_CHECK(hipMemcpyAsync(multi->box_t.p + k, &one, sizeof(real), hipMemcpyHostToDevice, stream));
}

// Ry (device, m x W block: every column its own r_y) -> the column-major copy of its box rows that launch_box takes a column of.
// The copy lives with the block state of width W: a change of width (ensure_multi) drops it.
void ConeDev::set_multi_ry(const real *Ry, int W) {
  ensure_multi(W);
  if (bsize <= 0) return;
  ConeMulti &mc = *multi;
  if (!mc.ry_cols.p) mc.ry_cols.alloc((size_t)m * W);
  const int gb = std::max(1, std::min(2048, (bsize + CONE_TR - 1) / CONE_TR));
  MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_rows_to_cols<MW>, dim3(gb), dim3(SCSAMD_BLOCK), 0, stream, Ry, mc.ry_cols.p, m, box_off, box_off + bsize));
}

// X (device, m x W block) <- Proj_K of its columns (proj_cone, cones.c:1340-1394, per column), without the Moreau wrapper: what
// proj_primal is to proj_dual.  The elementwise and second-order passes run over all W columns; the box cone and the PSD blocks beyond
// the LDS path over columns 0 .. K - 1.  Padding columns that hold zeros keep them.
void ConeDev::proj_primal_multi(real *X, int W, int K, const real *r_y, bool own_ry, const real *bl_cols, const real *bu_cols) {
  ensure_multi(W);
  ConeMulti &mc = *multi;
  if (own_ry && bsize > 0 && !mc.ry_cols.p) throw HipError("scs_amd: per-column r_y of the box cone has not been set");
  if (z + l > 0)
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_zero_pos<MW>, dim3(small_grid((long long)(z + l) * W)), dim3(SCSAMD_BLOCK), 0, stream, X, z, l));
  if (bsize > 0) { // column after column on the column position's Newton start
    const int gb = std::max(1, std::min(2048, (bsize + CONE_TR - 1) / CONE_TR));
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_rows_to_cols<MW>, dim3(gb), dim3(SCSAMD_BLOCK), 0, stream, X, mc.cols.p, m, box_off, box_off + bsize));
    const real *rb = r_y ? r_y + box_off : (const real *)nullptr;
    const size_t nb = bsize > 1 ? (size_t)bsize - 1 : 0; // a column's bounds
    for (int k = 0; k < K; ++k)
      launch_box(mc.cols.p + (size_t)k * m + box_off, mc.box_t.p + k, own_ry ? mc.ry_cols.p + (size_t)k * m + box_off : rb,
                 bl_cols ? bl_cols + k * nb : nullptr, bl_cols ? bu_cols + k * nb : nullptr);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_cols_to_rows<MW>, dim3(gb), dim3(SCSAMD_BLOCK), 0, stream, X, mc.cols.p, m, box_off, box_off + bsize));
  }
  if (n_tiny)
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_soc_tiny<MW>, dim3(small_grid((long long)n_tiny * W)), dim3(SCSAMD_BLOCK), 0, stream, X, tiny_off.p,
                                         tiny_len.p, n_tiny));
  if (n_big) {
    const int gt = std::min(n_tiles, 8192);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_soc_tile_partial<MW>, dim3(gt), dim3(SCSAMD_BLOCK), 0, stream, X, tile_off.p, tile_len.p,
                                         tile_cone.p, big_off.p, mc.tile_part.p, n_tiles));
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_soc_finalize<MW>, dim3(small_grid((long long)n_big * W)), dim3(SCSAMD_BLOCK), 0, stream, X,
                                         big_off.p, big_tile0.p, mc.tile_part.p, mc.big_coef.p, n_big));
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_soc_tile_apply<MW>, dim3(gt), dim3(SCSAMD_BLOCK), 0, stream, X, tile_off.p, tile_len.p,
                                         tile_cone.p, big_off.p, mc.big_coef.p, n_tiles));
  }
  if (n_psd) {
    const int p0 = psd_row0, gp = std::max(1, std::min(2048, (exp_off - psd_row0 + CONE_TR - 1) / CONE_TR));
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_rows_to_cols<MW>, dim3(gp), dim3(SCSAMD_BLOCK), 0, stream, X, mc.cols.p, m, p0, exp_off));
    // the LDS kernel over the blocks of all W columns in ONE launch (a padding column holds zero blocks: no sweeps)
    const int warm = mc.psd_vprev.p != nullptr && (mc.psd_calls % PSD_WARM_RESET) != 0;
    ++mc.psd_calls;
    launch_psd_lds(mc.cols.p, n_psd * W, mc.psd_off.p, mc.psd_k.p, mc.psd_tscratch.p, mc.psd_vprev.p, warm);
    for (size_t k = 0; k < mc.big.size() && (int)k < K; ++k) mc.big[k]->project(mc.cols.p + k * m, psd_off.p, psd_k.p, status.p, stream);
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_cols_to_rows<MW>, dim3(gp), dim3(SCSAMD_BLOCK), 0, stream, X, mc.cols.p, m, p0, exp_off));
  }
  if (ep + ed + psize > 0)
    MULTI_DISPATCH(W, hipLaunchKernelGGL(k_m_exp_pow<MW>, dim3(small_grid((long long)(ep + ed + psize) * W)), dim3(SCSAMD_BLOCK), 0, stream,
                                         X + (size_t)exp_off * W, ep, ed, psize, pow_a.p));
}

} // namespace scsamd
