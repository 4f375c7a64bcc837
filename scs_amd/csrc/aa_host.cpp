// aa_host.cpp -- host-side Anderson acceleration of the ADMM fixed-point map.
//
// Stays on the host by design (BASELINE.json north_star); the driver ships v and
// v_prev over PCIe only on the iterations that call in here.  Restates the
// algorithm of reference src/aa.c without LAPACK:
//   aa_init :657-820, aa_apply :822-854, aa_safeguard :856-899, aa_reset :934-967
//   update_accel_params :340-391  (S, D, Y columns; g = x - f; cached column norms)
//   solve :422-655  pivoted QR of [A; sqrt(r) I] (A = S type-I, Y type-II), rank
//                   truncation, Q'[g;0] and (type-I) Q'[Y_piv; sqrt(r) e_piv] by the
//                   first `rank` reflectors, then f -= D gamma and relaxation.
// This file holds the O(dim) work: the Householder QR with column pivoting on columns
// that are swapped in memory (geqp3), the reflector application (ormqr), the loops over
// S and D.  The parameter check, the per-column state, r, the reflector scalars, the
// pivot and downdating rules and everything from the top rows of the factored panel to
// gamma (the reduced solve, the accept / reject decision and its counters) are in
// aa_small.h, shared with the device paths.
#include "scs_host.h"
#include "aa_small.h"

namespace scsamd {

struct AaHost : AaCol {
  int dim = 0;
  std::vector<real> x, f, g, g_prev, Y, S, D;
  std::vector<real> A_aug, B_aug, c_aug, work, x_work, colnrm, colnrm0;
};

AaHost *aa_host_init(int dim, int mem, int min_len, int type1, real regularization, real relaxation,
                     real safeguard_factor, real max_weight_norm, int ir_max_steps) {
  if (!aa_params_ok(dim, mem, min_len, regularization, relaxation, safeguard_factor, max_weight_norm, ir_max_steps))
    return nullptr;
  AaHost *a = new AaHost();
  try {
    a->init(dim, mem, min_len, type1, regularization, relaxation, safeguard_factor, max_weight_norm, ir_max_steps);
    a->dim = dim;
    if (a->mem <= 0) return a;
    const size_t d = (size_t)dim, m = (size_t)a->mem, aug = d + m;
    a->x.assign(d, 0); a->f.assign(d, 0); a->g.assign(d, 0); a->g_prev.assign(d, 0);
    a->Y.assign(d * m, 0); a->S.assign(d * m, 0); a->D.assign(d * m, 0);
    a->A_aug.assign(aug * m, 0); a->c_aug.assign(aug, 0);
    a->colnrm.assign(m, 0); a->colnrm0.assign(m, 0);
    if (type1) a->B_aug.assign(aug * m, 0);
    a->work.assign(d, 0);
    if (relaxation != (real)1.0) a->x_work.assign(d, 0);
  } catch (const std::bad_alloc &) {
    printf("Failed to allocate memory for AA.\n");
    delete a;
    return nullptr;
  }
  return a;
}

void aa_host_reset(AaHost *a) {
  if (a) a->reset();
}
void aa_host_finish(AaHost *a) { delete a; }
void aa_host_stats(const AaHost *a, AaStats *out) { a->stats(out); }

// ---- dense kernels on tall-skinny column-major matrices ------------------------------
// Householder QR with column pivoting of the rows x len matrix A (leading dim = rows).
// On exit R is in the upper triangle, reflector k is [1; A[k+1:, k]] with scalar tau[k],
// jpvt[k] = original index of the column now in position k.
static void qr_pivoted(real *A, long rows, int len, int *jpvt, real *tau, real *cn, real *cn0) {
  for (int j = 0; j < len; ++j) {
    jpvt[j] = j;
    cn[j] = cn0[j] = nrm2(A + (size_t)j * rows, rows);
  }
  for (int k = 0; k < len; ++k) {
    real *v = A + (size_t)k * rows;
    const int piv = pivot_to_front(k, len, jpvt, cn, cn0);
    if (piv != k) std::swap_ranges(v, v + rows, A + (size_t)piv * rows);
    const real xnorm = nrm2(v + k + 1, rows - k - 1);
    const Reflector h = householder(v[k], xnorm);
    tau[k] = h.tau;
    if (xnorm != 0) {
      for (long i = k + 1; i < rows; ++i) v[i] *= h.scale;
      v[k] = h.beta;
    }
    for (int j = k + 1; j < len; ++j) { // apply H_k to the trailing columns, downdate norms
      real *c = A + (size_t)j * rows;
      if (tau[k] != 0) {
        real w = c[k];
        for (long i = k + 1; i < rows; ++i) w += v[i] * c[i];
        w *= tau[k];
        c[k] -= w;
        for (long i = k + 1; i < rows; ++i) c[i] -= w * v[i];
      }
      if (downdate_norm(c[k], cn[j], cn0[j])) cn[j] = cn0[j] = nrm2(c + k + 1, rows - k - 1);
    }
  }
}

// c <- H_{nref-1} ... H_0 c  (= Q' c restricted to the first nref reflectors)
static void apply_qt(const real *A, long rows, int nref, const real *tau, real *c) {
  for (int k = 0; k < nref; ++k) {
    if (tau[k] == 0) continue;
    const real *v = A + (size_t)k * rows;
    real w = c[k];
    for (long i = k + 1; i < rows; ++i) w += v[i] * c[i];
    w *= tau[k];
    c[k] -= w;
    for (long i = k + 1; i < rows; ++i) c[i] -= w * v[i];
  }
}

// ---- the acceleration step -----------------------------------------------------------
static real aa_solve(real *f, AaHost *a, int len) {
  const long dim = a->dim, aug = dim + a->mem;
  const int mem = a->mem;
  const real *A_src = a->type1 ? a->S.data() : a->Y.data();
  const real r = a->regularization_r();
  const real sqrt_r = r > 0 ? std::sqrt(r) : (real)0;
  // [A; sqrt(r) I] column by column (aa.c:272-291)
  for (int i = 0; i < len; ++i) {
    real *col = a->A_aug.data() + (size_t)i * aug;
    memcpy(col, A_src + (size_t)i * dim, dim * sizeof(real));
    memset(col + dim, 0, mem * sizeof(real));
    col[dim + i] = sqrt_r;
  }
  qr_pivoted(a->A_aug.data(), aug, len, a->jpvt.data(), a->tau.data(), a->colnrm.data(), a->colnrm0.data());
  for (int j = 0; j < len; ++j) memcpy(&a->Rm[(size_t)j * mem], a->A_aug.data() + (size_t)j * aug, (j + 1) * sizeof(real));
  const int rank = a->find_rank(len);
  if (rank > 0) { // only the first `rank` reflectors reach c and the Y columns
    memcpy(a->c_aug.data(), a->g.data(), dim * sizeof(real));
    memset(a->c_aug.data() + dim, 0, mem * sizeof(real));
    apply_qt(a->A_aug.data(), aug, rank, a->tau.data(), a->c_aug.data());
    memcpy(a->c_top.data(), a->c_aug.data(), rank * sizeof(real));
    for (int i = 0; a->type1 && i < rank; ++i) {
      const int piv = a->jpvt[i];
      real *col = a->B_aug.data() + (size_t)i * aug;
      memcpy(col, a->Y.data() + (size_t)piv * dim, dim * sizeof(real));
      memset(col + dim, 0, mem * sizeof(real));
      col[dim + piv] = sqrt_r;
      apply_qt(a->A_aug.data(), aug, rank, a->tau.data(), col);
      memcpy(&a->W[(size_t)i * mem], col, rank * sizeof(real));
    }
  }
  const real aa_norm = a->solve_small(len, rank, r);
  if (aa_norm < 0) return aa_norm;
  const real *gamma = a->gamma.data();
  // f -= D gamma
  for (int j = 0; j < len; ++j) {
    const real gj = gamma[j];
    if (gj == 0) continue;
    const real *dc = a->D.data() + (size_t)j * dim;
    for (long i = 0; i < dim; ++i) f[i] -= dc[i] * gj;
  }
  if (a->relaxation != (real)1.0) { // aa.c:393-410
    for (int j = 0; j < len; ++j) {
      const real gj = gamma[j];
      const real *sc = a->S.data() + (size_t)j * dim;
      for (long i = 0; i < dim; ++i) a->x_work[i] -= sc[i] * gj;
    }
    const real om = (real)1. - a->relaxation;
    for (long i = 0; i < dim; ++i) f[i] = a->relaxation * f[i] + om * a->x_work[i];
  }
  a->success = 1;
  return aa_norm;
}

real aa_host_apply(real *f, const real *x, AaHost *a) { // aa.c:822-854
  real aa_norm = 0;
  const int len = std::min(a->iter, a->mem);
  const long dim = a->dim;
  a->success = 0;
  if (a->mem <= 0) return aa_norm;
  if (a->iter == 0) { // seed (init_accel_params, aa.c:293-307)
    memcpy(a->x.data(), x, dim * sizeof(real));
    memcpy(a->f.data(), f, dim * sizeof(real));
    for (long i = 0; i < dim; ++i) a->g_prev[i] = x[i] - f[i];
    a->iter++;
    return aa_norm;
  }
  { // update_accel_params, aa.c:340-391
    const int idx = (a->iter - 1) % a->mem;
    real *sc = a->S.data() + (size_t)idx * dim, *dc = a->D.data() + (size_t)idx * dim,
         *yc = a->Y.data() + (size_t)idx * dim;
    for (long i = 0; i < dim; ++i) {
      sc[i] = x[i] - a->x[i];
      dc[i] = f[i] - a->f[i];
      const real gi = x[i] - f[i];
      a->g[i] = gi;
      yc[i] = gi - a->g_prev[i];
    }
    a->nrm_s_col[idx] = nrm2(sc, dim);
    a->nrm_y_col[idx] = nrm2(yc, dim);
    memcpy(a->x.data(), x, dim * sizeof(real));
    memcpy(a->f.data(), f, dim * sizeof(real));
    memcpy(a->g_prev.data(), a->g.data(), dim * sizeof(real));
    if (!a->x_work.empty()) memcpy(a->x_work.data(), x, dim * sizeof(real));
    a->norm_g = nrm2(a->g.data(), dim);
  }
  if (a->iter >= a->min_len) {
    aa_norm = aa_solve(f, a, len);
    if (aa_norm > 0) a->st.n_accept++;
  }
  a->iter++;
  return aa_norm;
}

int aa_host_safeguard(real *f_new, real *x_new, AaHost *a) { // aa.c:856-899
  if (a->mem <= 0 || !a->success) return 0;
  a->success = 0;
  const long dim = a->dim;
  for (long i = 0; i < dim; ++i) a->work[i] = x_new[i] - f_new[i];
  const real nd = nrm2(a->work.data(), dim);
  if (nd > a->safeguard_factor * a->norm_g) {
    memcpy(f_new, a->f.data(), dim * sizeof(real));
    memcpy(x_new, a->x.data(), dim * sizeof(real));
    a->st.n_safeguard_reject++;
    aa_host_reset(a);
    return -1;
  }
  return 0;
}

} // namespace scsamd

// ---- C ABI exposure of the host AA (so the CPU test-suite can pin it against the
// reference's aa_init/aa_apply/aa_safeguard without a GPU) --------------------------------
using namespace scsamd;
extern "C" {
void *scs_amd_aa_init(scs_int dim, scs_int mem, scs_int min_len, scs_int type1, scs_float regularization,
                      scs_float relaxation, scs_float safeguard_factor, scs_float max_weight_norm,
                      scs_int ir_max_steps) {
  return aa_host_init(dim, mem, min_len, type1, regularization, relaxation, safeguard_factor, max_weight_norm,
                      ir_max_steps);
}
scs_float scs_amd_aa_apply(scs_float *f, const scs_float *x, void *a) { return aa_host_apply(f, x, (AaHost *)a); }
scs_int scs_amd_aa_safeguard(scs_float *f_new, scs_float *x_new, void *a) {
  return aa_host_safeguard(f_new, x_new, (AaHost *)a);
}
void scs_amd_aa_reset(void *a) { aa_host_reset((AaHost *)a); }
void scs_amd_aa_finish(void *a) { aa_host_finish((AaHost *)a); }
void scs_amd_aa_get_stats(const void *a, AaStats *out) { aa_host_stats((const AaHost *)a, out); }
}
