// spmm.h -- CSR products on a BLOCK of vectors (several right-hand sides of one KKT system), CDNA4.
//
// Generalises SCS(accum_by_atrans) (reference linsys/scs_matrix.c:161-186) from one vector to K: column k of the result is the
// product the single-vector kernels of spmv.h compute for column k alone.  The single-vector row gather uses 8 bytes of every
// 128-byte line it fetches; with the K vectors interleaved, one gathered row index brings K contiguous values, and the entry
// values and indices of the matrix are read once for K products.
//
// Layout of a block of `len` rows and K columns: row-major, element (i, k) at i * W + k, where the width W is the smallest of
// {2, 4, 8, 16} that is >= K (multi_width).  Padding columns k >= K are ordinary columns to the products.
//
// Lane mapping: a 64-lane wave is G = 64 / W groups of W lanes; lane l serves column l % W in group l / W.
//   * short rows (<= SPMM_LONG_ROW entries, i.e. all of them on the usual SCS matrices: 5 - 10 per row on the headline one):
//     a wave owns G consecutive rows per pass, one per group.  Their entries are contiguous in the CSR arrays: the wave reads
//     them once, coalesced, into LDS (up to 16 G entries; measured on the headline matrix against every group reading its own
//     val / idx from memory: 343 / 394 / 440 / 528 us per block product at W = 2 / 4 / 8 / 16 against 405 / 416 / 445 / 628).  The W lanes
//     of a group then read the SAME val / idx from LDS (a broadcast) and gather X[idx * W + k]: W contiguous values, 64 bytes
//     at W = 8 in fp64.  Each lane sums its row in index order -- the order of the reference's scalar loop -- so no cross-lane
//     traffic is needed and the row sums of a column do not depend on W.  Rows whose entries do not fit the stage are read
//     by their lanes directly;
//   * long rows: the whole wave takes one row, group g sums entries g, g + G, g + 2 G, ... and the G partial sums are combined
//     with __shfl_xor at strides W, 2 W, ..., 32 (a fixed tree; every lane of a column ends with the same bits).
// Waves stride over the rows (grid capped at SPMM_MAX_GRID workgroups), so empty rows, the last partial wave and matrices of
// any number of rows need no special case.  The matrices are the plain CSR arrays of the workspace (CsrView): no new layout.
//
// Per-column masks: `cskip` (W ints, or null) switches single columns off -- their lanes load nothing and store nothing (a
// stopped column of the block PCG costs no gather); `allskip` (one int, or null) ends the kernel at once.
//
// Values per column (VCOL): K systems that share the pattern but not the values.  `ptr` and `idx` are still the workspace's arrays,
// read once for all columns; the values are a block of nnz x W in the block layout, value (t, col) of stored entry t at
// (t - bias) * W + col (ValBlk).  Lane `col` of a group reads its own value, so the W lanes of a group read W contiguous values
// (64 bytes at W = 8 in fp64, a full line at W = 16) next to the W contiguous values they gather; only the indices are staged in
// LDS.  The sums keep the order and the multiply-add expression of the shared form: a column that holds the workspace's values has
// the shared form's bits.
#pragma once
#include "spmv.h"

namespace scsamd {

constexpr int MULTI_W_MAX = 16;    // widest block
constexpr int SPMM_LONG_ROW = 128; // rows longer than this are summed by the whole wave
constexpr int SPMM_STAGE_PER_ROW = 16; // a wave stages its G rows' entries in LDS when they are at most 16 G (24 KB per workgroup at W = 2 in fp64, 3 KB at W = 16)
constexpr int SPMM_MAX_GRID = 2048; // 8 workgroups of 4 waves per CU: the gathers are latency bound, occupancy hides it

// width of the device layout for nrhs columns; 1 for one column (the single-vector path), 0 outside 1 .. 16
inline int multi_width(long long nrhs) {
  if (nrhs < 1 || nrhs > MULTI_W_MAX) return 0;
  int w = 1;
  while (w < nrhs) w <<= 1;
  return w;
}

inline int spmm_grid(int rows, int W) {
  const long long waves = ((long long)rows + 64 / W - 1) / (64 / W);
  long long g = (waves + SCSAMD_BLOCK / SCSAMD_WAVE - 1) / (SCSAMD_BLOCK / SCSAMD_WAVE);
  if (g < 1) g = 1;
  return (int)(g < SPMM_MAX_GRID ? g : SPMM_MAX_GRID);
}

#ifdef __HIPCC__
// sum over the lanes of a wave that serve the same column (fixed butterfly; every such lane receives the same bits)
template <int W, typename T> __device__ __forceinline__ T col_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= W; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int W, typename T> __device__ __forceinline__ T col_wave_max(T v) {
#pragma unroll
  for (int o = 32; o >= W; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
// the same over a workgroup: `sh` holds (blockDim.x / 64) * W entries; waves are added in wave order
template <int W, typename T> __device__ __forceinline__ T block_col_sum(T v, T *sh) {
  v = col_wave_sum<W>(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6, col = l & (W - 1);
  __syncthreads();
  if (l < W) sh[w * W + l] = v;
  __syncthreads();
  T s = sh[col];
  for (int i = 1; i < nw; ++i) s += sh[i * W + col];
  return s;
}
template <int W, typename T> __device__ __forceinline__ T block_col_max(T v, T *sh) {
  v = col_wave_max<W>(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6, col = l & (W - 1);
  __syncthreads();
  if (l < W) sh[w * W + l] = v;
  __syncthreads();
  T s = sh[col];
  for (int i = 1; i < nw; ++i) s = sh[i * W + col] > s ? sh[i * W + col] : s;
  return s;
}

// consumer side of the two-level reduction, per column: `part` holds count x W entries, entry (b, k) at b * W + k
template <int W> __device__ __forceinline__ real reduce_partials_col_sum(const real *part, int count, real *sh) {
  real s = 0;
  for (int i = threadIdx.x; i < count * W; i += SCSAMD_BLOCK) s += part[i]; // SCSAMD_BLOCK % W == 0: a thread stays in its column
  return block_col_sum<W>(s, sh);
}
template <int W> __device__ __forceinline__ real reduce_partials_col_max(const real *part, int count, real *sh) {
  real s = 0;
  for (int i = threadIdx.x; i < count * W; i += SCSAMD_BLOCK) {
    const real v = part[i];
    s = v > s ? v : s;
  }
  return block_col_max<W>(s, sh);
}

// epilogues of spmv.h on element (r, col) of a block.  DCOL = false: d (R_x / R_y) is shared by the columns, one value per row.
// DCOL = true: every column has its own, d is a block in the block layout and element (r, col) is d[o] -- the W lanes of a group
// read W contiguous values.  The choice is a template parameter: the shared form carries no test for the other.
// The values of a product: shared by the columns (A.val of the CsrView; nothing more is carried) or one per column.  v: the nnz x W
// value block; bias: what the stored entry positions carry over the plain ones (CsrDev::bias, the DLONG test hook) -- the block is
// indexed by the plain position.  The choice is a template parameter, as for DCOL.
template <bool VCOL> struct ValBlk {};
template <> struct ValBlk<true> {
  const real *v;
  eoff bias;
};
template <int W> __device__ __forceinline__ real blk_val(const ValBlk<false> &, const real *val, eoff t, int) { return val[t]; }
template <int W> __device__ __forceinline__ real blk_val(const ValBlk<true> &vb, const real *, eoff t, int col) {
  return vb.v[(size_t)(t - vb.bias) * W + col];
}

template <int EPI, int W>
__device__ __forceinline__ real epi_init_blk(const EpiArgs &e, const real *y, size_t o) {
  if (EPI == EPI_GP) return e.y0 ? e.y0[o] : (real)0;
  if (EPI == EPI_ACC) return y[o];
  if (EPI == EPI_NEGDIV) return -y[o];
  return (real)0;
}
template <int EPI, int W, bool DCOL>
__device__ __forceinline__ void epi_apply_blk(const EpiArgs &e, real *y, int r, size_t o, real acc, real &dot) {
  real out = acc;
  if (EPI == EPI_DIV || EPI == EPI_NEGDIV) out = acc / (DCOL ? e.d[o] : e.d[r]);
  if (EPI == EPI_GP) {
    const real xr = e.xin[o];
    out = acc + (DCOL ? e.d[o] : e.d[r]) * xr;
    dot += xr * out;
  }
  y[o] = out;
}

// Y(rows x W) (op)= A X(cols x W).  EPI_GP: e.partial[blockIdx.x * W + k] receives the workgroup's part of column k's xin . y.
// DCOL (EPI_DIV, EPI_GP, EPI_NEGDIV): e.d is a rows x W block, one divisor / multiplier per column (epi_apply_blk).
// VCOL: every column its own values of the matrix, vb.v (ValBlk); A.val is not read and no value is staged in LDS.
template <int W, int EPI, bool DCOL = false, bool VCOL = false>
__global__ __launch_bounds__(SCSAMD_BLOCK) void csr_block_kernel(CsrView A, const real *__restrict__ X, real *Y, EpiArgs e,
                                                                 const int *cskip, const int *allskip, ValBlk<VCOL> vb) {
  constexpr int G = SCSAMD_WAVE / W;
  constexpr int STAGE = SPMM_STAGE_PER_ROW * G; // entries a wave stages per pass
  __shared__ real red[(SCSAMD_BLOCK / SCSAMD_WAVE) * W];
  __shared__ real sval_all[SCSAMD_BLOCK / SCSAMD_WAVE][VCOL ? 1 : STAGE]; // VCOL: never referenced, so no LDS is allocated for it
  __shared__ int sidx_all[SCSAMD_BLOCK / SCSAMD_WAVE][STAGE];
  real *sval = sval_all[threadIdx.x >> 6];
  int *sidx = sidx_all[threadIdx.x >> 6];
  (void)sval;
  if (allskip && *allskip) return; // the same word for every lane of the grid
  const int lane = threadIdx.x & 63, col = lane & (W - 1), g = lane / W;
  const bool on = !(cskip && cskip[col]);
  const int nwaves = gridDim.x * (SCSAMD_BLOCK / SCSAMD_WAVE);
  const int wave = blockIdx.x * (SCSAMD_BLOCK / SCSAMD_WAVE) + (threadIdx.x >> 6);
  real dot = 0;
  for (long long base = (long long)wave * G; base < A.rows; base += (long long)nwaves * G) { // wave-uniform trip count
    const long long rl = base + g;
    const int r = (int)rl;
    const bool valid = rl < A.rows;
    const bool has = on && valid;
    eoff a = 0, z = 0;
    if (valid) {
      a = A.ptr[r];
      z = A.ptr[r + 1];
    }
    const bool lng = z - a > SPMM_LONG_ROW;
    // the entries of the wave's G rows are contiguous: [a0, zend)
    const long long left = (long long)A.rows - 1 - base;
    const int glast = left < G - 1 ? (int)left : G - 1;
    const eoff a0 = __shfl(a, 0, 64), zend = __shfl(z, glast * W, 64);
    const bool staged = __ballot(valid && lng) == 0 && zend - a0 <= STAGE; // the same for every lane of the wave
    if (staged) {
      // one coalesced read of the entries into LDS; per lane the separate val / idx reads of G rows would cost the address
      // path of the vector memory as much as the gathers themselves
      const int cnt = (int)(zend - a0);
      for (int t = lane; t < cnt; t += SCSAMD_WAVE) {
        sidx[t] = A.idx[a0 + t];
        if constexpr (!VCOL) sval[t] = A.val[a0 + t];
      }
      __builtin_amdgcn_wave_barrier(); // LDS operations of one wave complete in issue order: no workgroup barrier is needed
      if (has) {
        const size_t o = (size_t)r * W + col;
        real acc = epi_init_blk<EPI, W>(e, Y, o);
        int k = (int)(a - a0);
        const int kz = (int)(z - a0);
        // four gathers in flight per lane; the sum keeps index order.  (Eight in flight with the slots past the row's end
        // predicated off measured slower at W >= 8, 480 against 440 us at W = 8: the latency of a lane's chain is not what
        // bounds the product; profiles/multi_rhs.md.)
        if constexpr (VCOL) {
          // the lane's own values: W contiguous ones per entry over the lanes of the group, four value loads in flight beside
          // the four gathers
          const real *vrow = vb.v + (size_t)(a0 - vb.bias) * W + col;
          for (; k + 4 <= kz; k += 4) {
            const int i0 = sidx[k], i1 = sidx[k + 1], i2 = sidx[k + 2], i3 = sidx[k + 3];
            const real v0 = vrow[(size_t)k * W], v1 = vrow[(size_t)(k + 1) * W], v2 = vrow[(size_t)(k + 2) * W],
                       v3 = vrow[(size_t)(k + 3) * W];
            const real x0 = X[(size_t)i0 * W + col], x1 = X[(size_t)i1 * W + col], x2 = X[(size_t)i2 * W + col],
                       x3 = X[(size_t)i3 * W + col];
            acc += v0 * x0;
            acc += v1 * x1;
            acc += v2 * x2;
            acc += v3 * x3;
          }
          for (; k < kz; ++k) acc += vrow[(size_t)k * W] * X[(size_t)sidx[k] * W + col];
        } else {
          for (; k + 4 <= kz; k += 4) {
            const int i0 = sidx[k], i1 = sidx[k + 1], i2 = sidx[k + 2], i3 = sidx[k + 3];
            const real x0 = X[(size_t)i0 * W + col], x1 = X[(size_t)i1 * W + col], x2 = X[(size_t)i2 * W + col],
                       x3 = X[(size_t)i3 * W + col];
            acc += sval[k] * x0;
            acc += sval[k + 1] * x1;
            acc += sval[k + 2] * x2;
            acc += sval[k + 3] * x3;
          }
          for (; k < kz; ++k) acc += sval[k] * X[(size_t)sidx[k] * W + col];
        }
        epi_apply_blk<EPI, W, DCOL>(e, Y, r, o, acc, dot);
      }
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    // rows too long to stage (or a long row among them): every lane reads its row's entries itself
    if (has && !lng) {
      const size_t o = (size_t)r * W + col;
      real acc = epi_init_blk<EPI, W>(e, Y, o);
      eoff k = a;
      for (; k + 4 <= z; k += 4) {
        const int i0 = A.idx[k], i1 = A.idx[k + 1], i2 = A.idx[k + 2], i3 = A.idx[k + 3];
        const real v0 = blk_val<W>(vb, A.val, k, col), v1 = blk_val<W>(vb, A.val, k + 1, col), v2 = blk_val<W>(vb, A.val, k + 2, col),
                   v3 = blk_val<W>(vb, A.val, k + 3, col);
        const real x0 = X[(size_t)i0 * W + col], x1 = X[(size_t)i1 * W + col], x2 = X[(size_t)i2 * W + col],
                   x3 = X[(size_t)i3 * W + col];
        acc += v0 * x0;
        acc += v1 * x1;
        acc += v2 * x2;
        acc += v3 * x3;
      }
      for (; k < z; ++k) acc += blk_val<W>(vb, A.val, k, col) * X[(size_t)A.idx[k] * W + col];
      epi_apply_blk<EPI, W, DCOL>(e, Y, r, o, acc, dot);
    }
    // long rows of this pass, one after the other, by the whole wave
    unsigned long long todo = __ballot(has && lng);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1; // a lane that holds the row's bounds
      const int gl = src / W;
      const eoff al = __shfl(a, src, 64), zl = __shfl(z, src, 64);
      real part = 0;
      if (on)
        for (eoff k = al + g; k < zl; k += G) part += blk_val<W>(vb, A.val, k, col) * X[(size_t)A.idx[k] * W + col];
      part = col_wave_sum<W>(part);
      if (on && g == gl) {
        const int rr = (int)(base + gl);
        const size_t o = (size_t)rr * W + col;
        epi_apply_blk<EPI, W, DCOL>(e, Y, rr, o, epi_init_blk<EPI, W>(e, Y, o) + part, dot);
      }
      todo &= ~((((unsigned long long)1 << W) - 1) << (gl * W));
    }
  }
  if (EPI == EPI_GP && e.partial) {
    dot = block_col_sum<W>(dot, red);
    if (threadIdx.x < W) e.partial[(size_t)blockIdx.x * W + threadIdx.x] = dot;
  }
}
#endif // __HIPCC__

} // namespace scsamd
