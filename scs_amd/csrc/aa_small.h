// aa_small.h -- the host core of Anderson acceleration: everything that is O(mem^2) or a
// decision, stated once for the host AA (aa_host.cpp), the device AA (aa_dev.hip) and the
// block form (aa_multi.h).  Those three differ in who does the O(dim) work and in where the
// top rows of the factored panel come from; what is here does not know which of them calls.
//   aa_params_ok        the parameter check of aa_init (reference src/aa.c:657-700)
//   AaCol               per-column host state with init / reset (:934-967) / stats, the
//                       regularisation r (:253-270), rank truncation at len*eps*|R11| and
//                       the tail of solve (:505-655): reduced solve (type-I: LU of the top
//                       block of Q'[Y_piv; ..]; type-II: R u = c) with iterative refinement,
//                       scatter into gamma, weight cap, rejection counters, return value
//   householder         reflector scalars from (alpha, xnorm)
//   pivot_to_front, downdate_norm   dgeqp3's pivot choice and norm downdating on index arrays
//   AaPanelCol          AaCol plus the pivoting state of the two device paths, whose panel
//                       columns are never swapped in memory (E / SS / CK per physical column)
//   nrm2, frob_from_cols (:236-251), lu_factor / lu_solve (gesv / getrs :505-552),
//   upper_solve (trsv :556-585)
#pragma once
#include "scs_host.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace scsamd {

static inline real nrm2(const real *x, long n) { // scaled 2-norm (overflow safe, like BLAS nrm2)
  real scale = 0, ssq = 1;
  for (long i = 0; i < n; ++i) {
    if (x[i] != 0) {
      const real a = std::fabs(x[i]);
      if (scale < a) {
        ssq = 1 + ssq * (scale / a) * (scale / a);
        scale = a;
      } else {
        ssq += (a / scale) * (a / scale);
      }
    }
  }
  return scale * std::sqrt(ssq);
}

static inline real frob_from_cols(const std::vector<real> &c) { // aa.c:236-251
  real m = 0;
  for (real v : c) m = std::max(m, v);
  if (m == 0) return 0;
  real s = 0;
  for (real v : c) s += (v / m) * (v / m);
  return m * std::sqrt(s);
}

// LU with partial pivoting of the r x r matrix W (column major, leading dim ld); 0 on success
static inline int lu_factor(real *W, int r, int ld, int *ipiv) {
  for (int k = 0; k < r; ++k) {
    int p = k;
    for (int i = k + 1; i < r; ++i)
      if (std::fabs(W[i + (size_t)k * ld]) > std::fabs(W[p + (size_t)k * ld])) p = i;
    ipiv[k] = p;
    if (W[p + (size_t)k * ld] == 0) return k + 1;
    if (p != k)
      for (int j = 0; j < r; ++j) std::swap(W[k + (size_t)j * ld], W[p + (size_t)j * ld]);
    const real d = (real)1 / W[k + (size_t)k * ld];
    for (int i = k + 1; i < r; ++i) W[i + (size_t)k * ld] *= d;
    for (int j = k + 1; j < r; ++j) {
      const real wkj = W[k + (size_t)j * ld];
      for (int i = k + 1; i < r; ++i) W[i + (size_t)j * ld] -= W[i + (size_t)k * ld] * wkj;
    }
  }
  return 0;
}
static inline void lu_solve(const real *W, int r, int ld, const int *ipiv, real *b) {
  for (int k = 0; k < r; ++k)
    if (ipiv[k] != k) std::swap(b[k], b[ipiv[k]]);
  for (int k = 0; k < r; ++k)
    for (int i = k + 1; i < r; ++i) b[i] -= W[i + (size_t)k * ld] * b[k];
  for (int k = r - 1; k >= 0; --k) {
    b[k] /= W[k + (size_t)k * ld];
    for (int i = 0; i < k; ++i) b[i] -= W[i + (size_t)k * ld] * b[k];
  }
}
static inline void upper_solve(const real *R, long ld, int r, real *b) { // R u = b
  for (int k = r - 1; k >= 0; --k) {
    b[k] /= R[k + (size_t)k * ld];
    for (int i = 0; i < k; ++i) b[i] -= R[i + (size_t)k * ld] * b[k];
  }
}

constexpr real AA_EPS = (real)(sizeof(real) == 8 ? DBL_EPSILON : FLT_EPSILON);

static inline bool aa_params_ok(int dim, int mem, int min_len, real regularization, real relaxation,
                                real safeguard_factor, real max_weight_norm, int ir_max_steps) {
  if (dim <= 0 || mem < 0 || !std::isfinite((double)regularization) || relaxation < 0 || relaxation > 2 ||
      safeguard_factor < 0 || max_weight_norm <= 0 || ir_max_steps < 0 || (std::min(mem, dim) > 0 && min_len < 1)) {
    printf("Invalid AA parameters.\n");
    return false;
  }
  return true;
}

// Reflector H = I - tau [1; v][1; v]' taking [alpha; x] to [beta; 0], v = scale * x (dlarfg)
struct Reflector {
  real beta, tau, scale;
};
static inline Reflector householder(real alpha, real xnorm) {
  if (xnorm == 0) return {alpha, 0, 0};
  const real beta = -std::copysign(std::hypot(alpha, xnorm), alpha);
  return {beta, (beta - alpha) / beta, (real)1 / (alpha - beta)};
}

// dgeqp3: the candidate with the largest remaining norm goes to position k; returns where it was
static inline int pivot_to_front(int k, int len, int *jpvt, real *cn, real *cn0) {
  int piv = k;
  for (int j = k + 1; j < len; ++j)
    if (cn[j] > cn[piv]) piv = j;
  if (piv != k) {
    std::swap(jpvt[k], jpvt[piv]);
    cn[piv] = cn[k];
    cn0[piv] = cn0[k];
  }
  return piv;
}

// dgeqp3's norm downdating of a trailing column whose row-k entry became ck.  Returns true
// when cancellation has eaten the estimate: the caller then sets cn = cn0 = the norm of what
// is left of the column, computed its own way.
static inline bool downdate_norm(real ck, real &cn, real cn0) {
  if (cn == 0) return false;
  real t = std::fabs(ck) / cn;
  t = std::max((real)0, (1 + t) * (1 - t));
  const real t2 = t * (cn / cn0) * (cn / cn0);
  const real tol3z = std::sqrt(AA_EPS);
  if (t2 <= tol3z) return true;
  cn *= std::sqrt(t);
  return false;
}

// One column's host state, whichever side does the O(dim) work.
struct AaCol {
  int type1 = 1, mem = 0, min_len = 0, iter = 0, success = 0, ir_max_steps = 0;
  real relaxation = 1, regularization = 0, safeguard_factor = 1, max_weight_norm = 0;
  real norm_g = 0;
  std::vector<real> nrm_s_col, nrm_y_col;
  AaStats st;
  // solve scratch, mem-sized: Rm = R of the pivoted columns, W = top of Q'[Y_piv; ..] (type-I), both with leading dim mem
  std::vector<real> W, W_orig, Rm, gamma, gamma_red, c_top, ir_res, tau;
  std::vector<int> jpvt, ipiv;

  int ncols() const { return (type1 ? 2 : 1) * mem + 1; } // panel columns: A, [Y], c
  int col_c() const { return type1 ? 2 * mem : mem; }

  // parameters as checked by aa_params_ok; may throw std::bad_alloc
  void init(int dim, int mem_, int min_len_, int type1_, real regularization_, real relaxation_, real safeguard_factor_,
            real max_weight_norm_, int ir_max_steps_) {
    type1 = type1_;
    mem = std::min(mem_, dim);
    min_len = mem > 0 ? std::min(min_len_, mem) : 0;
    regularization = regularization_;
    relaxation = relaxation_;
    safeguard_factor = safeguard_factor_;
    max_weight_norm = max_weight_norm_;
    ir_max_steps = ir_max_steps_;
    memset(&st, 0, sizeof st);
    st.last_aa_norm = (real)NAN;
    const size_t m = (size_t)mem;
    nrm_s_col.assign(m, 0); nrm_y_col.assign(m, 0);
    W.assign(m * m, 0); W_orig.assign(m * m, 0); Rm.assign(m * m, 0);
    gamma.assign(m, 0); gamma_red.assign(m, 0); c_top.assign(m, 0); ir_res.assign(m, 0); tau.assign(m, 0);
    jpvt.assign(m, 0); ipiv.assign(m, 0);
  }
  void reset() { // aa.c:934-967
    iter = 0;
    success = 0;
    norm_g = 0;
    std::fill(nrm_s_col.begin(), nrm_s_col.end(), (real)0);
    std::fill(nrm_y_col.begin(), nrm_y_col.end(), (real)0);
  }
  void stats(AaStats *out) const {
    *out = st;
    out->iter = iter;
  }
  real regularization_r() const { // aa.c:253-270
    if (regularization > 0) {
      const real ny = frob_from_cols(nrm_y_col);
      const real na = type1 ? frob_from_cols(nrm_s_col) : ny;
      return regularization * na * ny;
    }
    return regularization < 0 ? -regularization : (real)0;
  }
  // rank of R (in Rm) truncated at len * eps * |R11|
  int find_rank(int len) const {
    int rank = 0;
    const real r11 = std::fabs(Rm[0]);
    if (r11 > 0) {
      const real tol = r11 * (real)len * AA_EPS;
      for (rank = 0; rank < len; ++rank)
        if (std::fabs(Rm[rank + (size_t)rank * mem]) < tol) break;
    }
    return rank;
  }
  // The tail of solve (aa.c:505-655).  In: jpvt, Rm, rank = find_rank(len) and, for the leading rank rows, c_top = top of
  // Q'[g; 0] and (type-I) W.  Out: gamma; the returned aa_norm is negative exactly when the step is rejected, and then
  // the column has been reset.  Applying gamma and setting `success` is the caller's.
  real solve_small(int len, int rank, real r) {
    int info = rank == 0 ? 1 : 0;
    if (info == 0) {
      memcpy(gamma_red.data(), c_top.data(), rank * sizeof(real));
      if (type1) {
        for (int i = 0; i < rank; ++i) memcpy(&W_orig[(size_t)i * mem], &W[(size_t)i * mem], rank * sizeof(real));
        info = lu_factor(W.data(), rank, mem, ipiv.data());
        if (info == 0) lu_solve(W.data(), rank, mem, ipiv.data(), gamma_red.data());
      } else {
        upper_solve(Rm.data(), mem, rank, gamma_red.data());
      }
      real prev = 0;
      for (int k = 0; info == 0 && k < ir_max_steps; ++k) { // iterative refinement, aa.c:530-552, :566-585
        for (int i = 0; i < rank; ++i) {
          if (type1) {
            real s = c_top[i];
            for (int j = 0; j < rank; ++j) s -= W_orig[i + (size_t)j * mem] * gamma_red[j];
            ir_res[i] = s;
          } else {
            real s = 0;
            for (int j = i; j < rank; ++j) s += Rm[i + (size_t)j * mem] * gamma_red[j];
            ir_res[i] = c_top[i] - s;
          }
        }
        if (type1) lu_solve(W.data(), rank, mem, ipiv.data(), ir_res.data());
        else upper_solve(Rm.data(), mem, rank, ir_res.data());
        const real dn = nrm2(ir_res.data(), rank);
        for (int i = 0; i < rank; ++i) gamma_red[i] += ir_res[i];
        if (k > 0 && dn >= (real)0.5 * prev) break;
        prev = dn;
      }
      if (info == 0) {
        for (int i = 0; i < len; ++i) gamma[i] = 0;
        for (int i = 0; i < rank; ++i) gamma[jpvt[i]] = gamma_red[i];
      }
    }
    real aa_norm = info == 0 ? nrm2(gamma.data(), len) : (real)-1.0;
    st.last_rank = rank;
    st.last_regularization = r;
    st.last_aa_norm = (info == 0 && std::isfinite((double)aa_norm)) ? aa_norm : (real)NAN;
    if (info != 0 || !std::isfinite((double)aa_norm) || aa_norm >= max_weight_norm) {
      if (rank == 0) st.n_reject_rank0++;
      else if (info != 0) st.n_reject_lapack++;
      else if (!std::isfinite((double)aa_norm)) st.n_reject_nonfinite++;
      else st.n_reject_weight_cap++;
      reset();
      if (!std::isfinite((double)aa_norm)) aa_norm = -1.0;
      return aa_norm < 0 ? aa_norm : -aa_norm;
    }
    return aa_norm;
  }
};

// AaCol plus the pivoting state of a panel whose columns stay where they are: the device reports, per physical panel
// column, E = the entry at the row below the last reflector, SS = the sum of squares below that, CK = the entry at the
// reflector's own row after it was applied; `top` receives the leading rows of every panel column, top[col * mem + row].
struct AaPanelCol : AaCol {
  std::vector<real> cn, cn0, E, SS, CK, top;
  void init_panel() {
    const size_t m = (size_t)mem, nc = (size_t)ncols();
    cn.assign(m, 0); cn0.assign(m, 0);
    E.assign(nc, 0); SS.assign(nc, 0); CK.assign(nc, 0);
    top.assign(nc * m, 0);
  }
  real remaining_norm(int col) const { return std::sqrt(E[col] * E[col] + SS[col]); }
  void pivot_begin(int len) { // after the first statistics pass
    for (int j = 0; j < len; ++j) {
      jpvt[j] = j;
      cn[j] = cn0[j] = remaining_norm(j);
    }
  }
  // step k: chooses the pivot (its physical column is jpvt[k] afterwards) and gives its reflector
  Reflector pivot_step(int k, int len) {
    pivot_to_front(k, len, jpvt.data(), cn.data(), cn0.data());
    const int P = jpvt[k];
    const Reflector h = householder(E[P], std::sqrt(SS[P]));
    tau[k] = h.tau;
    return h;
  }
  void pivot_downdate(int k, int len) { // after the sweep of step k
    for (int j = k + 1; j < len; ++j)
      if (downdate_norm(CK[jpvt[j]], cn[j], cn0[j])) cn[j] = cn0[j] = remaining_norm(jpvt[j]);
  }
  // from `top` of a finished factorisation to gamma: the hand-over to solve_small
  real solve_from_top(int len, real r) {
    for (int j = 0; j < len; ++j)
      for (int i = 0; i <= j; ++i) Rm[i + (size_t)j * mem] = top[(size_t)jpvt[j] * mem + i];
    const int rank = find_rank(len);
    for (int i = 0; i < rank; ++i) {
      c_top[i] = top[(size_t)col_c() * mem + i];
      if (type1) memcpy(&W[(size_t)i * mem], &top[(size_t)(mem + jpvt[i]) * mem], rank * sizeof(real));
    }
    return solve_small(len, rank, r);
  }
};

} // namespace scsamd
