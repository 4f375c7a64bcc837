/*
 * scs_amd.h -- C ABI of the MI355X-native ADMM hot path for SCS.
 *
 * One shared library (scs_amd/lib/libscsamd.so, fp64; libscsamd_f32.so when
 * built with -DSFLOAT) exports three concentric boundaries.  Every entry point
 * below is bound exactly as the reference (cvxgrp/scs v3.2.11) binds the one it
 * replaces; citations are <file>:<line> relative to the reference tree.
 *
 *   B2  whole-solve API             reference include/scs.h:271-338
 *         scs_init  scs_update  scs_solve  scs_finish  scs
 *         scs_set_default_settings  scs_version
 *       The iterate vectors live in HBM for the whole scs_solve; the host only
 *       sees scalars (residual norms, tau, CG counts) and, every
 *       acceleration_interval iterations, the vector v for Anderson
 *       acceleration (host side by design).
 *
 *   B1  linear-system plugin        reference include/linsys.h:25-71
 *         scs_init_lin_sys_work  scs_solve_lin_sys  scs_update_lin_sys_diag_r
 *         scs_free_lin_sys_work  scs_get_lin_sys_method
 *       Host pointers in/out, identical contract to linsys/cpu/indirect
 *       (private.c:221-349): `b` is overwritten by [x; y], `s` may be NULL,
 *       0 == success, NULL on init failure.  These five symbols are also
 *       exported by scs_amd/lib/libscsamd_linsys.so (besides scs_amd_* helpers,
 *       nothing else in it), which is what a reference build links instead of
 *       linsys/<backend>/private.o.  Beside them, on DEVICE pointers, the pieces
 *       of `mat_vec` (private.c:106-119) for a caller that splits one system by
 *       rows of A across GPUs: scs_amd_linsys_mat_vec_dev / _mul_a_dev /
 *       _mul_at_dev / _sync (declared with the instrumentation below).
 *
 *   B1' cone projection             reference include/cones.h:80-90
 *         scs_amd_cone_init  scs_amd_cone_proj_dual  scs_amd_cone_finish
 *       (the reference has no plugin API for cones; INTEGRATION.md shows the
 *       three-line shim that maps _scs_proj_dual_cone onto these).
 *
 * Plain C types only: pointers, sizes, the structs below.  No HIP or torch type
 * crosses this boundary.  Struct layouts are ABI facts of the reference and are
 * restated field-for-field (include/scs.h:47-244, include/aa_stats.h:21-42,
 * include/scs_types.h:13-32).  scs_int is 32-bit by default and 64-bit when the
 * header is compiled with -DDLONG, exactly like the reference's own switch; the
 * matching library is libscsamd_dlong.so (same entry points, 64-bit indices and
 * sizes at this boundary; on the device row / column indices stay 32-bit --
 * m + n + 1 < 2^31, refused loudly otherwise -- and entry positions are 64-bit
 * in that build, so nnz(A) >= 2^31 is accepted).
 */
#ifndef SCS_AMD_H
#define SCS_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- primitive types (reference include/scs_types.h:13-32) ------------- */
#ifdef DLONG
typedef long long scs_int; /* reference -DDLONG, include/scs_types.h:13-20 */
#else
typedef int scs_int;
#endif
#ifndef SFLOAT
typedef double scs_float;
#else
typedef float scs_float;
#endif

/* ---- exit flags (reference include/scs.h:33-42) ------------------------ */
#define SCS_INFEASIBLE_INACCURATE (-7)
#define SCS_UNBOUNDED_INACCURATE (-6)
#define SCS_SIGINT (-5)
#define SCS_FAILED (-4)
#define SCS_INDETERMINATE (-3)
#define SCS_INFEASIBLE (-2)
#define SCS_UNBOUNDED (-1)
#define SCS_UNFINISHED (0)
#define SCS_SOLVED (1)
#define SCS_SOLVED_INACCURATE (2)

/* ---- opaque workspaces -------------------------------------------------- */
typedef struct SCS_WORK ScsWork;                /* B2 */
typedef struct SCS_LIN_SYS_WORK ScsLinSysWork;  /* B1 */
typedef struct SCS_AMD_CONE_WORK ScsAmdConeWork; /* B1' */

/* ---- data structs ------------------------------------------------------- */
/* CSC, zero based (reference include/scs.h:47-58). */
typedef struct {
  scs_float *x; /* values, nnz                */
  scs_int *i;   /* row indices, nnz           */
  scs_int *p;   /* column pointers, n + 1     */
  scs_int m;    /* rows                       */
  scs_int n;    /* columns                    */
} ScsMatrix;

/* reference include/scs.h:61-101 */
typedef struct {
  scs_int normalize;
  scs_float scale;
  scs_int adaptive_scale;
  scs_float rho_x;
  scs_int max_iters;
  scs_float eps_abs;
  scs_float eps_rel;
  scs_float eps_infeas;
  scs_float alpha;
  scs_float time_limit_secs;
  scs_int verbose;
  scs_int warm_start;
  scs_int acceleration_lookback;
  scs_int acceleration_interval;
  scs_int acceleration_type_1;
  scs_float acceleration_regularization;
  scs_float acceleration_relaxation;
  const char *write_data_filename;
  const char *log_csv_filename;
} ScsSettings;

/* reference include/scs.h:104-119 */
typedef struct {
  scs_int m;
  scs_int n;
  ScsMatrix *A; /* m x n                               */
  ScsMatrix *P; /* n x n upper triangle, or NULL       */
  scs_float *b; /* m                                   */
  scs_float *c; /* n                                   */
} ScsData;

/* reference include/scs.h:122-172 (spectral-cone members are compiled out of
 * the default reference build, scs.mk:195, and are not part of this ABI). */
typedef struct {
  scs_int z;      /* zero cone rows                                  */
  scs_int l;      /* nonnegative orthant rows                        */
  scs_float *bu;  /* box upper bounds, bsize - 1                     */
  scs_float *bl;  /* box lower bounds, bsize - 1                     */
  scs_int bsize;  /* box cone length including t                     */
  scs_int *q;     /* second-order cone sizes                         */
  scs_int qsize;
  scs_int *s;     /* PSD cone matrix dimensions                      */
  scs_int ssize;
  scs_int *cs;    /* complex PSD cone matrix dimensions              */
  scs_int cssize;
  scs_int ep;     /* primal exponential cones (3 rows each)          */
  scs_int ed;     /* dual exponential cones                          */
  scs_float *p;   /* power cone parameters in [-1,1], <0 = dual cone  */
  scs_int psize;
} ScsCone;

/* reference include/scs.h:180-187 */
typedef struct {
  scs_float *x;
  scs_float *y;
  scs_float *s;
} ScsSolution;

/* reference include/aa_stats.h:21-42 */
typedef struct {
  scs_int iter;
  scs_int n_accept;
  scs_int n_reject_lapack;
  scs_int n_reject_rank0;
  scs_int n_reject_nonfinite;
  scs_int n_reject_weight_cap;
  scs_int n_safeguard_reject;
  scs_int last_rank;
  scs_float last_aa_norm;
  scs_float last_regularization;
} AaStats;

/* reference include/scs.h:190-244 */
typedef struct {
  scs_int iter;
  char status[128];
  char lin_sys_solver[128];
  scs_int status_val;
  scs_int scale_updates;
  scs_float pobj;
  scs_float dobj;
  scs_float res_pri;
  scs_float res_dual;
  scs_float gap;
  scs_float res_infeas;
  scs_float res_unbdd_a;
  scs_float res_unbdd_p;
  scs_float setup_time; /* ms */
  scs_float solve_time; /* ms */
  scs_float scale;
  scs_float comp_slack;
  scs_int rejected_accel_steps;
  scs_int accepted_accel_steps;
  AaStats aa_stats;
  scs_float lin_sys_time; /* ms */
  scs_float cone_time;    /* ms */
  scs_float accel_time;   /* ms */
} ScsInfo;

/* ======================= B2: whole-solve API ============================== */
/* replaces src/scs.c:1245 (scs_init)   -- validates, deep-copies, equilibrates
 * on the host, then uploads A (both orientations), b, c, D, E once. */
ScsWork *scs_init(const ScsData *d, const ScsCone *k, const ScsSettings *stgs);
/* replaces src/scs.c:1287 */
scs_int scs_update(ScsWork *w, scs_float *b, scs_float *c);
/* Extension (not in the reference; OSQP / Clarabel users know it as update_A / update_P): NEW VALUES of A and / or P on the pattern
 * given to scs_init -- scs_init's value-dependent half again, without its pattern-dependent half (the numbering of reorder.h, the
 * pattern transposes, the row units of the wave layouts, every kernel choice: all of them read the pattern only and stay as taken).
 * Ax, Px: host arrays in the CALLER's order, the CSC arrays of d->A / d->P as given to scs_init (P: upper triangle); either may be
 * NULL (that matrix keeps its values); both NULL is a no-op returning 0.
 * After a successful call the workspace is in the state scs_init would have produced on the same pattern, cones and settings with the
 * new values and the b, c most recently set (scs_init or scs_update): a solve returns the bits a fresh workspace returns.  In detail:
 * the renumbering decided at init is kept and the values follow the entry permutation recorded with it (host, nnz entry positions,
 * only when the renumbering is active); the equilibration runs again from the new raw values, through the passes scs_init took (host
 * or device: bit-identical); D, E, primal_scale, dual_scale are replaced and b, c normalised again from the originals; every value copy
 * of the linear system, the layouts and the preconditioner follow (scs_amd_linsys_update_values); stgs.scale goes back to the value
 * given to scs_init -- an adapted scale does not carry over -- and diag_r with it; the box cone's normalised bounds are rebuilt and the
 * warm starts of the box and PSD projections (single and block) are cold again; both Anderson memories start empty, as before every
 * solve.  The family state of scs_amd_solve_family caches nothing that depends on the values.  With P the workspace also keeps the
 * raw values of both matrices on the host (the one an update does not name is equilibrated again from them).
 * -1 before any device call, the workspace untouched: w NULL, Px on a workspace without P, a non-finite value.  -1 on a HIP failure
 * (message on stderr): the workspace is then STALE -- scs_solve and scs_amd_solve_family return SCS_FAILED, NaN-filled, until an
 * update succeeds.  info.setup_time of the next solve is this call's time, as after scs_update.  Returns with the stream idle. */
scs_int scs_amd_update_matrix(ScsWork *w, const scs_float *Ax, const scs_float *Px);
/* replaces src/scs.c:1327 -- the device-resident ADMM loop */
scs_int scs_solve(ScsWork *w, ScsSolution *sol, ScsInfo *info,
                  scs_int warm_start);
/* replaces src/scs.c:1486 */
void scs_finish(ScsWork *w);
/* replaces src/scs.c:1538 */
scs_int scs(const ScsData *d, const ScsCone *k, const ScsSettings *stgs,
            ScsSolution *sol, ScsInfo *info);
/* replaces src/util.c:158 */
void scs_set_default_settings(ScsSettings *stgs);
/* replaces src/scs_version.c */
const char *scs_version(void);

/* ======================= B1: linear-system plugin ========================= */
/* replaces linsys/cpu/indirect/private.c:225 (callers src/scs.c:1092) */
ScsLinSysWork *scs_init_lin_sys_work(const ScsMatrix *A, const ScsMatrix *P,
                                     const scs_float *diag_r);
/* replaces private.c:284 (callers src/scs.c:763,1127) */
scs_int scs_solve_lin_sys(ScsLinSysWork *w, scs_float *b, const scs_float *s,
                          scs_float tol);
/* replaces private.c:327 (caller src/scs.c:1220) */
scs_int scs_update_lin_sys_diag_r(ScsLinSysWork *w,
                                  const scs_float *new_diag_r);
/* Extension: new values for the matrices of a live workspace, in the CSC order of the A (and P, upper triangle) handed to
 * scs_init_lin_sys_work; the pattern is the one given then.  Ax or Px may be NULL (that matrix keeps its values).
 * Afterwards the workspace cannot be told from one scs_init_lin_sys_work created on the new values: CSC(A) as given, CSR(A), the value
 * arrays of the wave-owned-rows layouts (plain, lockstep, wide: whichever was built), the symmetric P and its diagonal sums, the Jacobi
 * preconditioner under the diag_r in force; every decision taken at init (kernel choice, captured graphs, pacing) stays as taken, and
 * the block entries and small-system paths read the same arrays.  The values are uploaded once and gathered on the device through
 * position maps that the FIRST update builds and the workspace frees: nnz(A) entry positions (CSR position -> CSC position, formed on the
 * device from the two patterns in HBM), and with P nnz(full P) entry positions + nnz(upper P) values of staging (the map of P is replayed
 * once on the host from the symmetric copy, which requires the P given at init to have been an upper triangle).  Entry positions are
 * 4 bytes, 8 in the DLONG build.  The layouts store no map: the builder that made a layout runs again on the refreshed CSR copy -- the
 * device builder, or the HOST builder (one download and one pass) for a layout it made (a unit beyond 8192 entries, wr_build=host) --
 * so their bytes equal a fresh build's.  No other host pass over the entries than the finiteness check.
 * 0 on success; -1 on bad arguments (w NULL, a row-sharded workspace, Px given for a workspace without P, a non-finite value --
 * checked before any device call, the workspace untouched) or on a HIP failure (message on stderr).  Returns with the stream idle. */
scs_int scs_amd_linsys_update_values(ScsLinSysWork *w, const scs_float *Ax, const scs_float *Px);
/* replaces private.c:333 (caller src/scs.c:1493) */
void scs_free_lin_sys_work(ScsLinSysWork *w);
/* replaces private.c:221 (callers src/scs.c:127,1346) */
const char *scs_get_lin_sys_method(void);

/* ======================= B1': cone projection ============================= */
/* replaces src/cones.c:1498 (_scs_init_cone).  `k` is read, never mutated: the
 * box bounds are copied and the lazy D-normalisation of cones.c:1161-1177 is
 * applied to the copy when D != NULL.  D may be NULL (un-normalised cones). */
ScsAmdConeWork *scs_amd_cone_init(const ScsCone *k, scs_int m,
                                  const scs_float *D);
/* replaces src/cones.c:1552 (_scs_proj_dual_cone): x (host, length m) is
 * overwritten by its projection onto the DUAL cone under the r_y metric;
 * r_y may be NULL (Euclidean).  Returns <0 on failure, like the reference. */
scs_int scs_amd_cone_proj_dual(ScsAmdConeWork *c, scs_float *x,
                               const scs_float *r_y);
/* replaces src/cones.c:338 (_scs_finish_cone) */
void scs_amd_cone_finish(ScsAmdConeWork *c);
/* ---- blocks of vectors: K projections at once (the cone half of an iteration over a family of problems that share the cones) ----
 * Column k of a block projection is what scs_amd_cone_proj_dual(c, X[:, k], r_y) computes -- the Moreau wrapper of
 * src/cones.c:1552-1596 around proj_cone (:1340-1394) -- for every cone scs_amd_cone_init accepts, to the projection's own
 * accuracy (not bit for bit: the reduction trees of the second-order cones differ).  The columns share the cone description and
 * r_y and nothing else: on a freshly initialised workspace the bits of a column do not depend on the other columns, nor, within
 * one width, on its position; two runs on the same inputs return the same bits (no floating-point atomics).
 * Device layout: that of the block solve (scs_amd_solve_lin_sys_multi) -- row-major, element (i, k) at i * W + k,
 * W = scs_amd_cone_multi_width(nrhs).  All W columns are written; columns nrhs .. W - 1 come back zero.
 * Carried state (the box cone's Newton start, src/cones.c:1560; each PSD block's eigenbasis; the periodic cold restart) belongs
 * to the column position and passes from one block call to the next of the same width; a change of width starts cold.  Block
 * calls neither read nor write the state of the single-vector path.  Block state and staging are allocated at the first block
 * call and freed by scs_amd_cone_finish.  One column (nrhs == 1) IS the single-vector path, bit for bit. */
/* width of the device layout for nrhs columns (2, 4, 8 or 16; 1 for nrhs == 1; 0 if nrhs < 1 or > 16) */
scs_int scs_amd_cone_multi_width(scs_int nrhs);
/* K projections of scs_amd_cone_proj_dual (src/cones.c:1552) on one workspace.  X: host, column-major, nrhs columns of length
 * m, leading dimension ldx >= m; each column is overwritten by its projection onto the dual cone under the r_y metric; rows
 * between m and ldx are not touched.  r_y: host, length m, shared by all columns, or NULL.  More than 16 columns are served in
 * chunks of at most 16 (a last chunk of one column as a block of width 2: it stays off the single-vector state).
 * 0 on success; 1 when a PSD block of any column hit the Jacobi sweep cap (as scs_amd_cone_proj_dual: reported, not fatal,
 * src/cones.c:1031); -1 on bad arguments (checked before any device call; X untouched) or on a HIP failure (message on
 * stderr; the workspace stays usable). */
scs_int scs_amd_cone_proj_dual_multi(ScsAmdConeWork *c, scs_int nrhs, scs_float *X, scs_int ldx,
                                     const scs_float *r_y);
/* the same on DEVICE pointers, in place, under the stream contract of scs_amd_linsys_*_dev: the work is enqueued on the
 * workspace's private stream; the caller synchronises its own work before the call and calls scs_amd_cone_sync before it reads
 * the result.  x_dev: m values; X_dev: m * W values in the device layout; r_y_dev: m values or NULL.  -1 for nrhs outside
 * 1 .. 16; nrhs == 1 is the single-vector entry.  PSD blocks that hit the sweep cap are counted on the device and reported by
 * the next host-pointer projection. */
scs_int scs_amd_cone_proj_dual_dev(ScsAmdConeWork *c, scs_float *x_dev, const scs_float *r_y_dev);
scs_int scs_amd_cone_proj_dual_multi_dev(ScsAmdConeWork *c, scs_int nrhs, scs_float *X_dev,
                                         const scs_float *r_y_dev);
scs_int scs_amd_cone_sync(ScsAmdConeWork *c);

/* ======================= instrumentation ================================== */
/* Not in the reference (its `tot_cg_its`, private.h:28, is never surfaced).
 * Counters accumulate per workspace since init / since the last reset.  Kernel
 * times come from HIP events recorded on the library's own stream. */
typedef struct {
  long long cg_iters;        /* PCG iterations, all solves                   */
  long long lin_sys_solves;  /* scs_solve_lin_sys calls                      */
  long long mat_vecs;        /* applications of R_x + P + A' R_y^-1 A        */
  long long spmv_launches;   /* CSR SpMV kernel launches (both orientations) */
  double spmv_ms;            /* summed HIP-event time of those launches      */
  double cg_ms;              /* summed HIP-event time of whole PCG solves    */
  double cone_ms;            /* summed HIP-event time of cone projections    */
  long long cone_projs;
  long long nnz;             /* nnz(A)                                       */
  long long spmv_bytes;      /* algorithmic bytes of ONE mat_vec (2 SpMV)    */
  long long psd_unconverged; /* PSD block projections whose Jacobi eigensolve hit the sweep cap (the
                              * reference's LAPACK info > 0 case: reported, not fatal, src/cones.c:1031) */
} ScsAmdStats;

void scs_amd_linsys_get_stats(const ScsLinSysWork *w, ScsAmdStats *out);
/* How the host fed the PCG loop of this workspace since it was created (option cg_pace):
 *   out[0]  CG iterations enqueued, counted in iterations: a quantum is one iteration (its launches) or one replayed graph of 8
 *   out[1]  CG iterations the device executed (ScsAmdStats.cg_iters); out[0] - out[1] was enqueued past convergence
 *   out[2]  blocking synchronisations inside the linear solves (0 with cg_pace=1 unless `debug` / `trace_file` ask for more)
 *   out[3]  linear solves
 * Plain host counters: no device call, no synchronisation.  Block solves (scs_amd_solve_lin_sys_multi) count in out[1] and out[3] only. */
void scs_amd_linsys_get_cg_pacing(const ScsLinSysWork *w, long long out[4]);
void scs_amd_get_cg_pacing(const ScsWork *w, long long out[4]);
void scs_amd_linsys_set_profiling(ScsLinSysWork *w, scs_int on);
/* Pieces of the operator of linsys/cpu/indirect/private.c:106-119 (`mat_vec`) on DEVICE pointers, for a caller that splits
 * ONE linear system by rows of A across GPUs (scs_amd/shard.py): the workspace is created by
 * scs_init_lin_sys_work on a row slab A_r (m_r x n) with diag_r = [R_x / ranks ; R_y of the slab], so that the sum over
 * ranks of mat_vec is R_x x + A' R_y^-1 A x.  Work is enqueued on the workspace's stream; _sync waits for it.
 *   mat_vec_dev   y(n)   = diag_r[0..n) .* x + A_r' R_r^-1 A_r x
 *   mul_a_dev     y(m_r) = A_r x           (src/scs.c:559 uses the same product for the residuals)
 *   mul_at_dev    x(n)   = A_r' y
 * CONTRACT (the entries take no lengths and no stream):
 *   - buffers: x / y are device pointers on the workspace's device (the one selected by scs_amd_set_device when the workspace
 *     was created) holding at least n resp. m_r scs_float of THIS library's precision; they are not validated;
 *   - ordering: the work is enqueued on the workspace's PRIVATE non-blocking stream, which has no implicit ordering with any
 *     stream of the caller (e.g. torch's current stream).  The caller must (1) make its writes to the input visible before the
 *     call -- synchronise its own stream (or the device) first -- and (2) call scs_amd_linsys_sync(w) before it reads the
 *     output or reuses the input; entries issued back to back on one workspace run in issue order;
 *   - threads: one host thread per workspace at a time (as for the five plugin functions, include/linsys.h).            */
scs_int scs_amd_linsys_mat_vec_dev(ScsLinSysWork *w, const scs_float *x_dev, scs_float *y_dev);
scs_int scs_amd_linsys_mul_a_dev(ScsLinSysWork *w, const scs_float *x_dev, scs_float *y_dev);
scs_int scs_amd_linsys_mul_at_dev(ScsLinSysWork *w, const scs_float *y_dev, scs_float *x_dev);
scs_int scs_amd_linsys_sync(ScsLinSysWork *w);
/* ---- blocks of right-hand sides: K solves of one KKT system at once (families of problems that share A, P and the cones) ----
 * Column k of a block solve is what scs_solve_lin_sys(w, B[:, k], S[:, k], tol[k]) computes: the recurrence of
 * linsys/cpu/indirect/private.c:133-217 (`pcg`) under the wrapper of :284-324, applied to that column alone -- its own alpha,
 * beta, z'r, |r|_inf and tolerance, the strict `norm_r < tol` stop test, the max(tol, 1e-12) test before the first iteration
 * (:163), the z'r == 0 breakdown exit, the cap of 10 n iterations (:307) and the zero short-circuit (:296-299); iterations are
 * counted as the reference counts them (:203, :216).  The columns run in lock step on the device but share nothing except the
 * workspace's A, P and diag_r: this is K independent conjugate-gradient solves, not block CG, and the bits of a column do not
 * depend on the other columns of the block nor on its position in it.  A column that has stopped is frozen while the others go
 * on.  Deterministic: two calls on the same inputs return the same bits.
 * Device layout of a block of K columns: row-major, element (i, k) at i * W + k, W = scs_amd_linsys_multi_width(K) = the smallest
 * of {2, 4, 8, 16} that is >= K; padding columns are zero.  One column goes to the single-vector path (bit-identical to
 * scs_solve_lin_sys); more than 16 are served in chunks of at most 16.  The block buffers (7 n W + 2 m W values at the largest W
 * used; 6 n W + 2 m W without P) are allocated at the first block call and freed by scs_free_lin_sys_work.
 * scs_update_lin_sys_diag_r applies to block solves as to single ones.  Row-sharded systems (ScsAmdShard) have no block entry.
 * ScsAmdStats: a block solve adds every column's iterations to cg_iters, one per column to lin_sys_solves, and one per block
 * product that did work to mat_vecs (the largest iteration count of the block, plus one for a warm start). */
/* K solves of scs_solve_lin_sys (private.c:284-324) on one workspace.  B: host, column-major, nrhs columns of
 * length n + m, leading dimension ldb >= n + m; column k in: [r_x; r_y], out: [x; y].
 * S: warm starts, n x nrhs, leading dimension lds >= n, or NULL (all cold).
 * tol: nrhs tolerances.  iters: nrhs PCG iteration counts on return, or NULL.
 * 0 on success; -1 on bad arguments (checked before any device call) or on a HIP failure (message on stderr; the workspace
 * stays usable). */
scs_int scs_amd_solve_lin_sys_multi(ScsLinSysWork *w, scs_int nrhs, scs_float *B, scs_int ldb,
                                    const scs_float *S, scs_int lds, const scs_float *tol,
                                    scs_int *iters);
/* width of the device layout for nrhs columns (2, 4, 8 or 16; 1 for nrhs == 1; 0 if nrhs < 1 or > 16) */
scs_int scs_amd_linsys_multi_width(scs_int nrhs);
/* the operator pieces of scs_amd_linsys_mat_vec_dev / _mul_a_dev / _mul_at_dev (private.c:106-119; linsys/scs_matrix.c:161-186)
 * on blocks in the device layout (row-major, width = scs_amd_linsys_multi_width(nrhs)); same stream contract.  All `width`
 * columns of the output are written (a padding column holds the product of the input's padding column).  -1 for nrhs outside
 * 1 .. 16; nrhs == 1 is the single-vector entry. */
scs_int scs_amd_linsys_mat_vec_multi_dev(ScsLinSysWork *w, scs_int nrhs, const scs_float *X_dev, scs_float *Y_dev);
scs_int scs_amd_linsys_mul_a_multi_dev(ScsLinSysWork *w, scs_int nrhs, const scs_float *X_dev, scs_float *Y_dev);
scs_int scs_amd_linsys_mul_at_multi_dev(ScsLinSysWork *w, scs_int nrhs, const scs_float *Y_dev, scs_float *X_dev);
/* ---- every column of a block under its own diag_r ----
 * The block solve above shares the workspace's diag_r = [R_x; R_y] among its columns.  Here column k has its own R_x,k, R_y,k and
 * its own Jacobi preconditioner: it computes what scs_update_lin_sys_diag_r(w, DR[:, k]) followed by
 * scs_solve_lin_sys(w, B[:, k], S[:, k], tol[k]) computes (private.c:50-82, :106-119, :133-217, :284-327), while A and P are still
 * read once per product for all columns -- a sweep over rho, scale or regularisation as one block.  Everything said above about
 * independence, frozen columns, determinism and the statistics holds; with every column's R equal to the workspace's diag_r the
 * call returns the bits and the iteration counts of scs_amd_solve_lin_sys_multi.  Three more blocks (2 n W + m W values) are
 * allocated at the first per-column call and freed by scs_free_lin_sys_work; a caller who never makes one allocates nothing
 * more than before. */
/* K solves, column k under its own diag_r.  DR: host, column-major, (n + m) x nrhs, lddr >= n + m, column k = [R_x,k; R_y,k],
 * every used entry finite and > 0; not modified.  Everything else as scs_amd_solve_lin_sys_multi.  The workspace's own diag_r is
 * neither used nor changed.  More than 16 columns in chunks of at most 16; ONE column runs as a block of width 2 (it stays off
 * the single-vector state).  -1 before any device call, B untouched: w / DR / B / tol NULL, nrhs < 1, lddr or ldb < n + m,
 * lds < n with S, a non-finite or non-positive entry of DR, a row-sharded workspace.  -1 on a HIP failure with the stream
 * drained (the convention of scs_amd_solve_lin_sys_multi); the workspace stays usable. */
scs_int scs_amd_solve_lin_sys_multi_r(ScsLinSysWork *w, scs_int nrhs, const scs_float *DR, scs_int lddr,
                                      scs_float *B, scs_int ldb, const scs_float *S, scs_int lds,
                                      const scs_float *tol, scs_int *iters);
/* Y = R_x,k .* x_k + P x_k + A' R_y,k^-1 A x_k per column, on device blocks, the stream contract of
 * scs_amd_linsys_mat_vec_multi_dev.  R_dev: (n + m) x W row-major, rows 0 .. n-1 = R_x, rows n .. n+m-1 = R_y; all W columns
 * are read as ordinary columns (the caller fills padding columns, e.g. with 1).  -1 for nrhs outside 1 .. 16 (1 runs at W = 2). */
scs_int scs_amd_linsys_mat_vec_multi_r_dev(ScsLinSysWork *w, scs_int nrhs, const scs_float *R_dev,
                                           const scs_float *X_dev, scs_float *Y_dev);
/* ---- every column of a block with its own values of A and P ----
 * The blocks above read one A and one P for all columns.  Here the K systems share the PATTERN given to scs_init_lin_sys_work and
 * nothing else: column k has its own values of A and P (and its own diag_r), and computes what
 *     scs_amd_linsys_update_values(w, AX[:, k], PX[:, k]); scs_update_lin_sys_diag_r(w, DR[:, k]);
 *     scs_solve_lin_sys(w, B[:, k], S[:, k], tol[k])
 * computes (private.c:50-82, :106-119, :133-217, :284-327) -- time-varying dynamics, scenario-dependent coefficients, a sweep over
 * a coefficient as one block.  The row pointers and indices are read once per product for all columns; the values are stored as
 * blocks of nnz x W in the block layout, so the W lanes that gather W contiguous values of the vector also read W contiguous
 * values of the matrix.  Bit for bit, column k is column k of scs_amd_solve_lin_sys_multi_r at the same nrhs on a workspace
 * brought to values k by scs_amd_linsys_update_values; with every column holding the workspace's own values the call returns the
 * bits and iteration counts of scs_amd_solve_lin_sys_multi_r (DR given) or scs_amd_solve_lin_sys_multi (DR NULL).  Independence,
 * frozen columns, determinism and the statistics as above.
 * Memory: (2 nnz(A) + nnz(full P) + n) W values and one staged column, allocated by the FIRST set call only (with the R blocks of
 * scs_amd_solve_lin_sys_multi_r and the position maps of scs_amd_linsys_update_values), rebuilt when a set call needs a wider
 * block, released by scs_amd_linsys_free_values_multi or scs_free_lin_sys_work; an allocation failure leaves the workspace usable
 * without value blocks.  The workspace's own values, layouts, diag_r, preconditioner, captured graph and single-vector state are
 * neither read for the columns nor written: scs_solve_lin_sys, _multi and _multi_r return the bits they returned before, and
 * scs_amd_linsys_update_values / scs_update_lin_sys_diag_r on the same workspace neither read nor change the stored blocks.
 * Refusals, all before any device call, message on stderr, -1, the workspace, the stored blocks and B untouched: w / AX / B / tol
 * NULL; PX given without P or missing with P; nrhs < 1 or > 16 (no chunking: set and solve in groups); a short leading
 * dimension; a non-finite value in AX or PX; a non-finite or non-positive value in DR; a row-sharded workspace; a solve or a
 * product before a set call or with another nrhs than the set call's.  -1 on a HIP failure with the stream drained. */
/* stores the values of nrhs (1..16) systems on the pattern given to scs_init_lin_sys_work: AX column-major nnz(A) x nrhs in the CSC
 * order of init's A, PX nnz(upper P) x nrhs (NULL iff the workspace has no P); host arrays, not modified.  Replaces the values of
 * an earlier set call.  Returns with the stream idle (the arrays may be pageable and reused). */
scs_int scs_amd_linsys_set_values_multi(ScsLinSysWork *w, scs_int nrhs, const scs_float *AX, scs_int ldax, const scs_float *PX, scs_int ldpx);
/* column k: scs_amd_linsys_update_values(AX[:,k], PX[:,k]); scs_update_lin_sys_diag_r(DR[:,k]); scs_solve_lin_sys(B[:,k], S[:,k], tol[k]).
 * DR may be NULL (the workspace's diag_r in every column); the rest as scs_amd_solve_lin_sys_multi_r; nrhs must equal the set call's.
 * ONE column runs as a block of width 2. */
scs_int scs_amd_solve_lin_sys_multi_v(ScsLinSysWork *w, scs_int nrhs, const scs_float *DR, scs_int lddr, scs_float *B, scs_int ldb,
                                      const scs_float *S, scs_int lds, const scs_float *tol, scs_int *iters);
/* Y(:,k) = (R_x,k + P_k + A_k' R_y,k^-1 A_k) X(:,k) on device blocks, as scs_amd_linsys_mat_vec_multi_r_dev (R_dev NULL: the
 * workspace's diag_r in every column) */
scs_int scs_amd_linsys_mat_vec_multi_v_dev(ScsLinSysWork *w, scs_int nrhs, const scs_float *R_dev, const scs_float *X_dev, scs_float *Y_dev);
void scs_amd_linsys_free_values_multi(ScsLinSysWork *w);   /* releases the value blocks; NULL-safe */
/* the SpMV kernel these entries (and scs_solve_lin_sys) run for A (which = 0) / A' (which = 1): the strings of
 * scs_amd_get_spmv_kernel_name.  Returns the length needed. */
scs_int scs_amd_linsys_spmv_kernel_name(const ScsLinSysWork *w, scs_int which, char *buf, scs_int cap);
void scs_amd_get_stats(const ScsWork *w, ScsAmdStats *out);
void scs_amd_set_profiling(ScsWork *w, scs_int on);
/* scs_solve split in three so a harness can time / inspect an exact range of ADMM
 * iterations (bench.py's timed region, trajectory tests):
 *   scs_amd_solve_begin(w, sol_or_NULL, warm)   == everything scs_solve does before
 *                                                  the loop (src/scs.c:1341-1354)
 *   scs_amd_solve_steps(w, k)                   runs up to k more iterations, returns
 *                                                  the iteration counter, stream idle
 *   scs_amd_solve_end(w, sol, info)             == finalize + timings (:1457-1484)   */
scs_int scs_amd_solve_begin(ScsWork *w, const ScsSolution *sol, scs_int warm_start);
scs_int scs_amd_solve_steps(ScsWork *w, scs_int steps);
scs_int scs_amd_solve_converged(const ScsWork *w);
scs_int scs_amd_solve_end(ScsWork *w, ScsSolution *sol, ScsInfo *info);
/* test hook: every per-iteration linear solve uses this tolerance instead of the
 * schedule of src/scs.c:745-762 (0 restores the schedule) */
void scs_amd_set_cg_tol_override(ScsWork *w, double tol);
/* ---- a family of problems: the same A, P and cones with nprob different (b, c), solved in ONE device-resident ADMM loop ----
 * K solves of scs_update(w, B[:,k], Cc[:,k]); scs_solve(w, &sols[k], &infos[k], warm_start)  (src/scs.c:1287-1325, :1327-1484)
 * on one workspace, on blocks: the block solve (scs_amd_solve_lin_sys_multi) and the block projection
 * (scs_amd_cone_proj_dual_multi) are the two halves of its iteration, in their device layout (row-major, element (i, k) at
 * i * W + k, W in {2, 4, 8, 16}).
 * Column k is the reference's ADMM map (src/scs.c:1356-1455) applied to problem k alone: its own tau, kappa, root_plus,
 * primal_scale / dual_scale (normalize_b_c per column), g = (R + M)^-1 [c_k; -b_k], residuals, CG tolerance schedule
 * (:745-762, from that column's own norms), convergence test, status, certificates and ScsInfo.  The columns share A, P, D, E,
 * diag_r and the cones and nothing else.  Not bit for bit the single solve (the reduction trees differ); within one width the
 * bits of a column depend neither on the other columns nor on its position, and two calls on the same inputs return the same
 * bits (no floating-point atomics; every family solve starts its PSD eigenbases and box Newton starts cold).
 * Convergence is tested where the single solve tests it (every 25 iterations), for all running columns in one block residual
 * evaluation.  A column whose test fires at iteration i is frozen there with info.iter = i, exactly as the single loop breaks:
 * from then on nothing of it is read or written, and it costs no linear-solve iteration.  The loop ends when every column is
 * frozen, at max_iters, at time_limit_secs (one clock per chunk) or on SIGINT (every column not yet finished: SCS_SIGINT).
 * B: host, column-major, m x nprob, leading dimension ldb >= m.  Cc: host, column-major, n x nprob, ldc >= n.  sols, infos: nprob
 * of each; sols[k].x / y / s are caller-allocated (n, m, m) and, with warm_start != 0, hold the warm start of column k as
 * scs_solve takes it (src/scs.c:660-687).  More than 16 problems are served in chunks of at most 16 (a chunk of one problem as
 * a block of width 2: it stays off the single-solve state).
 * Requires adaptive_scale == 0 (a scale update changes diag_r, which the columns share), acceleration_lookback == 0 and
 * log_csv_filename == NULL: otherwise the call is refused before any device call with a message that names the setting
 * (scs_amd_solve_family_refusal returns that message, or NULL).  Refused settings and bad arguments (w, B, Cc, sols or infos
 * NULL, nprob < 1, ldb < m, ldc < n) return SCS_FAILED with sols / infos untouched.
 * Family state (block iterates, residual blocks, per-column b, c, scales) belongs to this entry: allocated at the first call at
 * the largest width used, freed by scs_finish.  The workspace's own problem and single-solve state (b, c, scales, iterates,
 * cone and PCG state of the single-vector path) are neither read nor written: a scs_solve after a family call returns the
 * bits it returns without it.  scs_amd_set_cg_tol_override applies per column.  infos[k].solve_time, lin_sys_time and cone_time
 * are the chunk's wall times, the same in every column of a chunk; scale_updates and the acceleration fields are 0.  verbose
 * prints the header once and one summary line per column, no iteration table.
 * Returns 0 when every column ended with a status the single solve would have returned; SCS_FAILED on a HIP failure (message on
 * stderr, every column NaN-filled with status SCS_FAILED, the workspace stays usable). */
scs_int scs_amd_solve_family(ScsWork *w, scs_int nprob,
                             const scs_float *B, scs_int ldb,   /* host, column-major, m x nprob, ldb >= m */
                             const scs_float *Cc, scs_int ldc,  /* host, column-major, n x nprob, ldc >= n */
                             ScsSolution *sols, ScsInfo *infos, /* nprob of each; sols[k].x/y/s caller-allocated */
                             scs_int warm_start);
const char *scs_amd_solve_family_refusal(const ScsWork *w);
/* ---- the same with a scale per problem, fixed or adaptive ----
 * scs_amd_solve_family with one difference: the columns do not share diag_r.  Column k runs under its own
 *   diag_r_k = [rho_x ; 1/(1000 scale_k) on the zero cone, 1/scale_k elsewhere ; TAU_FACTOR]   (src/scs.c:971-980)
 * in every step that reads R: the block solve (its own R_x, R_y and Jacobi preconditioner, scs_amd_solve_lin_sys_multi_r), the
 * glue of the iteration, the box cone's Newton iteration and the warm start (v_y = y + s / R_y,k).
 * scales: nprob initial scales (host), or NULL for the workspace's stgs.scale in every column.  Every entry must be finite and
 * > 0: otherwise SCS_FAILED before any device call, sols / infos untouched.
 * adaptive_scale != 0: column k runs update_scale (src/scs.c:1164-1241) on its own residuals, with its own running sums and its
 * own last update, where the single solve runs it -- at a convergence check, after the test, before the dual update.  A column
 * whose scale changes gets its R, its preconditioner, its g = (R + M)^-1 [c_k; -b_k] (a cold solve to 1e-12 in which every other
 * column is stopped on entry) and its v = rsk / R + 2 u_t - u anew; of a column whose scale did not change not one bit is read
 * or written by that.  A frozen column never updates.  adaptive_scale == 0: the scales stay as given -- a scale sweep.
 * With equal scales and adaptive_scale == 0 a column holds the bits scs_amd_solve_family gives on a workspace of that scale.
 * infos[k].scale and infos[k].scale_updates are the column's own.  The workspace's stgs.scale, diag_r, the linear system's
 * rx / ry / M, its captured graph and the single-solve state are neither read for the columns nor written: scs_solve and
 * scs_amd_solve_family return the same bits before and after.  acceleration_lookback != 0 and log_csv_filename are refused as
 * in scs_amd_solve_family (scs_amd_solve_family_scaled_refusal: that message, or NULL).  Holds one l x W and one n x W block
 * more than scs_amd_solve_family (the R of every column and its preconditioner), allocated at the first scaled call.
 * Everything else -- arguments, chunks, freezing, statuses, failure convention -- as in scs_amd_solve_family. */
scs_int scs_amd_solve_family_scaled(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                    const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start);
const char *scs_amd_solve_family_scaled_refusal(const ScsWork *w);
/* ---- a queue of problems through one block: the finished columns are refilled ----
 * scs_amd_solve_family (own_scale == 0; scales must be NULL, adaptive_scale is refused) or scs_amd_solve_family_scaled
 * (own_scale != 0; scales: nprob initial scales or NULL) for ANY nprob >= 1, through one block of `width` columns (2, 4, 8 or 16;
 * 0: max(2, the block width of min(nprob, 16) columns)): a column that has ended gives its slot to the next problem of the queue
 * while its neighbours run on, where the two entries above cut the queue into chunks that each wait for their slowest column.
 * The schedule (part of the contract):
 *  - one global iteration index i = 0, 1, 2, ...; a problem that starts at global iteration s runs its local iteration j = i - s,
 *    and everything the loop derives from the iteration index it derives, per column, from j: the feasible first iteration, the
 *    normalisation of v, the warm-start term 1 / (j + 1)^1.5 of the CG tolerance, the iteration of the residuals, of the
 *    convergence test and of update_scale, and info.iter;
 *  - problems 0 .. min(width, nprob) - 1 start at s = 0 in slots 0, 1, ...;
 *  - a column ends at the bottom of global iteration i when j % 25 == 0 and its convergence test fires (iter = j), when
 *    j + 1 == max_iters (iter = max_iters, its residuals evaluated after that iteration), or when at a check its own
 *    time_limit_secs, counted from the moment its column started running, has passed;
 *  - its result is then taken out and returned to sols[p] / infos[p] at once, and the lowest free slot takes the next problem of
 *    the queue, in index order, which starts at the smallest multiple of 25 greater than i -- so all running columns reach their
 *    checks in the same global iterations and one residual evaluation and one read-back serve all of them; the price is up to 24
 *    block iterations in which the refilled slot does not run yet;
 *  - the call ends when the queue is empty and every slot is free.
 * The promise: for every problem p, (x, y, s), status_val, iter, scale, scale_updates and the residual and objective fields of
 * ScsInfo are, bit for bit, what scs_amd_solve_family / scs_amd_solve_family_scaled returns for it in a call of the same width,
 * whatever its place in the queue, the slot it gets and what its neighbours do.  With nprob <= width no slot is refilled.
 * Refused (scs_amd_solve_family_stream_refusal(w, own_scale): the message, or NULL): what the entry of the chosen form refuses,
 * and cones with PSD or complex PSD blocks (ssize + cssize > 0: the eigensolver's warm start and cold-restart counter belong to
 * the width, not to a slot -- use the two entries above).  Refused arguments that depend on the workspace -- ldb < m, ldc < n,
 * scales with own_scale == 0, a scale that is not finite and > 0 -- are reported by the same function until a call on the
 * workspace is accepted.  Every refusal, and w, B, Cc, sols or infos NULL, nprob < 1 or a width outside {0, 2, 4, 8, 16} (checked
 * before the workspace is looked at), returns SCS_FAILED with a message before any device call, with sols / infos untouched.
 * infos[p].solve_time runs from the activation of p's column to its return; lin_sys_time is the block solves' wall time in
 * between, cone_time the sampled mean of a block projection times p's iterations.  verbose prints one summary row per problem as
 * it finishes.  SIGINT: the problems that run or have not started get SCS_SIGINT, the finished ones keep their results.  A HIP
 * failure fails every problem of the call, those already returned included; the workspace stays usable.  The state of scs_solve
 * and of the two entries above is not disturbed.  Holds W (l + 2 n + 3 m) values (the records of a column in and a column out) more than they do, from its first call on.
 * scs_amd_family_stream_get_counters, for the last stream call on the workspace: out[0] block iterations (the last global i that
 * ran, + 1), out[1] slot-iterations in which a column ran (a problem that converged with iter = j counts j + 1, one that ended at
 * the cap max_iters), out[2] slot-iterations in which a slot held no running column (out[0] * width - out[1]), out[3] refills,
 * out[4] residual evaluations, out[5] the width used. */
scs_int scs_amd_solve_family_stream(ScsWork *w, scs_int nprob,
                                    const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                    scs_int own_scale, const scs_float *scales, scs_int width,
                                    ScsSolution *sols, ScsInfo *infos, scs_int warm_start);
const char *scs_amd_solve_family_stream_refusal(const ScsWork *w, scs_int own_scale);
void scs_amd_family_stream_get_counters(const ScsWork *w, long long out[6]);
/* ---- a family that shares the pattern and the cones but not the VALUES of A and P ----
 * scs_amd_solve_family_scaled with one more difference: column k has its own A_k and P_k on the pattern given to scs_init (time-
 * varying dynamics, scenario coefficients, a sweep over a coefficient).  Two calls, set once and solve any number of times:
 * scs_amd_family_set_values: AX is nnz(A) x nprob, PX nnz(upper P) x nprob (given exactly when the workspace has a P), column-major
 * host arrays with leading dimensions ldax / ldpx, every column in the CSC order of the d->A / d->P given to scs_init, as for
 * scs_amd_update_matrix.  1 <= nprob <= 16 (no chunks: set and solve in groups, as scs_amd_linsys_set_values_multi).  Per column it
 * runs scs_init's value-dependent half on scratch copies: the internal numbering, the equilibration passes scs_init took (so its own
 * D_k, E_k), the box cone's normalised bounds, and the equilibrated values into the linear system's value blocks.  One column at a
 * time; returns with the stream idle.  The workspace's own problem -- its values, D, E, scales, diag_r, preconditioner, captured
 * graph, cone state -- is neither read for the columns nor written.
 * scs_amd_solve_family_values: B, Cc, scales, sols, infos, warm_start as in scs_amd_solve_family_scaled (scales NULL: stgs.scale
 * in every column; adaptive_scale is served per column), nprob that of the set call.  The contract:
 *  - column k is scs_amd_update_matrix(w, AX[:,k], PX[:,k]); scs_update(w, B[:,k], Cc[:,k]); scs_solve(...) on a workspace at the
 *    column's starting scale;
 *  - bit for bit, column k is column k of scs_amd_solve_family_scaled, at the same nprob, on a workspace brought to values k by
 *    scs_amd_update_matrix: (x, y, s), status_val, iter, scale, scale_updates and the residual and objective fields;
 *  - with the workspace's own values in every column the call returns the bits of scs_amd_solve_family_scaled;
 *  - a column depends neither on its neighbours' values nor on its position;
 *  - scs_solve and the other family entries return the same bits before and after either call.
 * Refused with SCS_FAILED before any device call, sols / infos untouched, the message from scs_amd_solve_family_values_refusal
 * (which serves both calls; NULL when the last call was accepted): acceleration_lookback != 0 or log_csv_filename; a NULL among w,
 * AX, B, Cc, sols, infos; PX given without a P or missing with one; nprob outside 1 .. 16; a short leading dimension; a matrix
 * value that is not finite; a scale that is not finite and > 0; a solve before a set call or with another nprob than the set
 * call's; a workspace that is stale after a failed scs_amd_update_matrix.  A scs_amd_update_matrix on the workspace leaves the
 * stored blocks in force, as scs_amd_linsys_update_values does for the linear system's blocks.
 * Memory: the value blocks of scs_amd_linsys_set_values_multi (2 nnz(A) W + nnz(full P) W + n W) plus (m + n) W for D / E,
 * 2 (bsize - 1) W for the box bounds and nprob host copies of D, E; allocated by the first set call only, released by
 * scs_amd_family_free_values (NULL-safe) or scs_finish; a failed allocation leaves the workspace usable with no values set.
 * Host memory while the set call runs, released when it returns: scratch copies of A and P (their patterns and one column of
 * values), the equilibrated values of all columns (nprob (nnz(A) + nnz(upper P)) values, handed to the value blocks in one go) and
 * the (m + n) W host images of the D / E blocks.  The value blocks are those scs_amd_linsys_set_values_multi fills on a
 * ScsLinSysWork; a ScsWork hands out no ScsLinSysWork, so on it only the set call above writes them.
 * Not served: the stream entry, more than 16 columns in a call, Anderson acceleration, a row-sharded system.
 * scs_amd_box_bounds is a TEST / DIAGNOSTIC entry, not part of the solver interface: host only, it returns the normalised bounds
 * scs_init and the set call keep for a box cone whose bsize rows are scaled by Db (NULL: as given), so that arithmetic can be
 * checked without a device. */
scs_int scs_amd_family_set_values(ScsWork *w, scs_int nprob, const scs_float *AX, scs_int ldax, const scs_float *PX, scs_int ldpx);
scs_int scs_amd_solve_family_values(ScsWork *w, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                    const scs_float *scales, ScsSolution *sols, ScsInfo *infos, scs_int warm_start);
void scs_amd_family_free_values(ScsWork *w);
const char *scs_amd_solve_family_values_refusal(const ScsWork *w);
scs_int scs_amd_box_bounds(const ScsCone *k, const scs_float *Db, scs_float *bl, scs_float *bu);
/* What scs_init decided about its internal numbering (scs_amd/csrc/reorder.h: variables, the rows of the zero / nonnegative
 * cones and -- round 6 -- the rows behind the first one of a second-order cone may be renumbered so that the gathers of the CSR products of linsys/scs_matrix.c:161-186 share cache lines; callers never see
 * it -- b, c, warm starts and the returned (x, y, s) are mapped at this boundary).  out[0] = 1 if renumbered, out[1], out[2] =
 * distinct 128-byte lines per gathered entry of the A / A' product as given, out[3], out[4] = after, out[5] = seconds spent. */
void scs_amd_get_reorder_info(const ScsWork *w, double *out);
/* how scs_init laid out A (out[0..2]) and A' (out[3..5]): wave-owned-rows layout built (0 / 1), built on the device (0 / 1),
 * distinct 128-byte lines per gathered entry (scs_amd/csrc/spmv_wave.h, spmv_wave_build.h) */
void scs_amd_get_layout_info(const ScsWork *w, double *out);
/* the SpMV kernel scs_init chose for A (which = 0) / A' (which = 1): the template's name as rocprofv3 lists it, e.g.
 * "csr_wave_lockstep_kernel<EPI,16,4>", "csr_wave_kernel<EPI,0>", "csr_stream_kernel<EPI>".  Returns the length needed. */
scs_int scs_amd_get_spmv_kernel_name(const ScsWork *w, scs_int which, char *buf, scs_int cap);
/* Test hook, host code only: the renumbering decision scs_init would take for this matrix and cone (no device needed).
 * col_new2old (n) and row_new2old (m) receive new index -> caller's index (identity when nothing is kept); info (6 doubles, may be
 * NULL) as scs_amd_get_reorder_info.  Returns 1 if a renumbering is kept, 0 if not, < 0 on error. */
scs_int scs_amd_plan_reorder(const ScsMatrix *A, const ScsCone *k, scs_int *col_new2old, scs_int *row_new2old, double *info);
/* The same plus the ENTRY permutation scs_amd_update_matrix follows: entry o of the renumbered matrix A[row_new2old][:, col_new2old]
 * (row indices sorted inside every column) is entry entry_new2old[o] (nnz of them) of A's arrays; the identity when nothing is kept.
 * info (7 doubles, may be NULL): the six above, then 1 if the renumbered matrix was built beside the measurement of the candidate,
 * 0 if afterwards -- the two ways scs_init comes by it; both record the same permutation. */
scs_int scs_amd_plan_reorder_entries(const ScsMatrix *A, const ScsCone *k, scs_int *col_new2old, scs_int *row_new2old,
                                     scs_int *entry_new2old, double *info);
/* measurement hook: recompute the residuals after every ADMM iteration, where the reference does when
 * `log_csv_filename` is set (src/scs.c:1449-1454).  Those norms feed the next iteration's CG tolerance
 * (src/scs.c:745-762): a logged reference run follows a tighter schedule than an unlogged one, and this puts
 * the solve on that schedule without writing a log (bench.py times the CPU window's schedule with it). */
void scs_amd_set_residuals_every_iter(ScsWork *w, scs_int on);
/* ---- a batch of SMALL problems that share A, P, the cone and the settings: one workgroup per problem, one launch ----
 * The contract of scs_amd_solve_family -- problem p is scs_update(w, B[:,p], Cc[:,p]); scs_solve(...) on a workspace with
 * adaptive_scale = 0 and acceleration_lookback = 0 -- for problems small enough that a problem's whole state fits in one
 * workgroup's LDS, for ANY nprob >= 1, and with EXACT linear solves: the scale is fixed, so H = R_x + P + A' R_y^-1 A (n x n,
 * dense) is factored once at init and applied as a dense inverse with one step of refinement (scs_amd/csrc/small_batch.h).  A
 * workgroup runs a problem from its first iteration to its convergence test (every 25 iterations; solved, infeasible, unbounded,
 * or max_iters with the "inaccurate" statuses) inside one kernel and then takes the next problem from a counter; the host is
 * not involved until the launch has ended.  A batch may mix all of these outcomes.  Equilibration (done once, at init, by the
 * host passes of scs_init), normalize_b_c per problem, the feasible first iteration, the normalisation of v, root_plus, alpha,
 * rho_x, scale, the residuals, the three tests, `iter` and the warm start are the reference's (src/scs.c).
 * Bits: every reduction has a fixed order and the only atomic is the integer problem counter, so a problem's (x, y, s) and
 * ScsInfo depend neither on nprob, on its index, on its neighbours, on the grid nor on the run.  They are not the bits of
 * scs_solve (exact against iterative solves: the iteration counts differ too).
 * scs_amd_small_init: d, k, stgs as scs_init takes them (d->b and d->c must be present and are not used).  Served: cones z, l and
 * q of any sizes (1 and 2 included), P present or absent, normalize 0 or 1, any scale, rho_x, alpha, eps_*, max_iters; sizes up
 * to scs_amd_small_limits: out[0] = the largest n (512), out[1] = the largest n + m + 1 (2304).  One of two instantiations of the
 * kernel is chosen once, at init, for both solve entries: n <= 128 and n + m + 1 <= 1024 run the NARROW one (256 threads, two
 * workgroups per CU), every other accepted size the WIDE one (1024 threads, one workgroup with the whole LDS of its CU); the
 * bits of a problem within the narrow limits are those it always had.  Not served, and named in the refusal: box,
 * PSD, complex PSD, exponential and power cones; adaptive_scale, acceleration_lookback and time_limit_secs != 0;
 * log_csv_filename and write_data_filename; a size over a limit; a NULL argument; non-finite values in A or P; a problem
 * scs_init's validation rejects; a reduced matrix that is not positive definite (an indefinite P).  A refused init returns NULL;
 * scs_amd_small_refusal returns the message of the last refused init / solve of the calling thread, NULL when that thread's last
 * init / solve was not refused.  Init is host work only (equilibration, H and its factor, the padded rows); the device side of
 * the object is created by its first accepted solve, so every refusal -- of init and of solve -- comes before any device call,
 * and a machine without a device shows in that solve (SCS_FAILED, the failure convention below).
 * scs_amd_small_solve: B, ldb, Cc, ldc, sols, infos, warm_start as in scs_amd_solve_family; sols[p].x / y / s must be allocated
 * by the caller.  Refused with SCS_FAILED before any device call, sols / infos untouched: a NULL argument (a NULL sols[p].x / y /
 * s included), nprob < 1, ldb < m or ldc < n, non-finite values in B or Cc.  Returns 0 otherwise; infos[p].status_val is the
 * problem's own status.  infos[p].solve_time is the wall time of the launch the problem ran in (at most 32768 problems per
 * launch), lin_sys_time, cone_time and the acceleration fields are 0, scale_updates is 0.  verbose: one summary row per problem
 * after its launch, as scs_amd_solve_family_stream prints them; no header.
 * A HIP failure fails every problem of the call (NaN-filled, SCS_FAILED, message on stderr) and leaves the object usable.  A
 * SIGINT is honoured BETWEEN LAUNCHES ONLY: a launch that has started runs to its end (at most max_iters iterations per problem);
 * the problems of the launches not yet started get SCS_SIGINT.
 * scs_amd_small_set_grid: the number of workgroups of the following launches (0: the default, what the chip holds at once:
 * CUs x workgroups per CU by the kernel's LDS; never more than the problems of the launch); returns 0, or -1 on a bad argument.
 * scs_amd_small_get_counters, summed over the object's life: out[0] launches, out[1] workgroups launched, out[2] problems,
 * out[3] iterations (the sum of infos[p].iter).  scs_amd_small_get_occupancy: out[0] workgroups per CU, out[1] LDS bytes per
 * workgroup, out[2] the default grid (what the device side sets: out[0] and out[1] are 0 before the first accepted solve), out[3] the setup time of init in
 * microseconds, out[4] the threads of a workgroup of the object's instantiation: 256 (narrow) or 1024 (wide), known from init on.
 * Memory: the padded rows of A and A', three dense n x n matrices, and per problem of the largest launch 2 (n + 2 m) + 27 values
 * (+ n + m + 1 once a call has warm-started), in HBM; 6 (n + m + 1) + 2 m + 3 n values of LDS per workgroup plus 264 (narrow) or
 * 1040 (wide).
 * One caller thread per object; several GPUs are not used. */
typedef struct ScsAmdSmall ScsAmdSmall;
ScsAmdSmall *scs_amd_small_init(const ScsData *d, const ScsCone *k, const ScsSettings *stgs);
const char *scs_amd_small_refusal(void);
void scs_amd_small_limits(scs_int out[2]);
scs_int scs_amd_small_solve(ScsAmdSmall *s, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                            ScsSolution *sols, ScsInfo *infos, scs_int warm_start);
scs_int scs_amd_small_set_grid(ScsAmdSmall *s, scs_int workgroups);
void scs_amd_small_get_counters(const ScsAmdSmall *s, long long out[4]);
void scs_amd_small_get_occupancy(const ScsAmdSmall *s, long long out[5]);
void scs_amd_small_finish(ScsAmdSmall *s);
/* ---- the same batch with OWN VALUES of A and P per problem, on the pattern the object was built with ----
 * scs_amd_small_set_values: AX is nnz(A) x nprob and PX nnz(upper P) x nprob (given exactly when the object was built with a P),
 * column-major with leading dimensions ldax / ldpx, every column in the CSC order of the d->A / d->P handed to
 * scs_amd_small_init, as for scs_amd_update_matrix; the pattern is the one of init, explicit zeros included.  Any nprob >= 1.
 * Per problem the host checks the values, runs the equilibration of scs_init on them (normalize = 1; D = E = 1 otherwise), keeps
 * D_p, E_p and writes the equilibrated values into the problem's blocks in HBM.  One set call serves any number of solve calls;
 * a second set call replaces the values; scs_amd_small_free_values releases them (NULL-safe; scs_amd_small_finish does it too).
 * scs_amd_small_solve_values: the arguments of scs_amd_small_solve; nprob is the set call's.  Problem p is
 * scs_amd_small_init on (A_p, P_p) followed by scs_amd_small_solve of (b_p, c_p): the same iteration, equilibration,
 * normalize_b_c, tests, statuses and warm start, launches of at most 32768 problems, and linear solves exact in the same sense.
 * NOT BIT FOR BIT that pair: scs_amd_small_init factors H in long double on the host; here the problem's workgroup assembles
 * H_p = R_x + P_p + A_p' R_y^-1 A_p, factors it (Cholesky) and inverts it in WORKING PRECISION on the device before the problem's
 * first iteration, and the refinement step of every solve repairs what that loses.  The two agree in iter and status_val, and in
 * ScsInfo and (x, y, s) to about 1e-6 relative (tests/test_small_values_gpu.py).  A problem's bits depend neither on nprob, on its
 * index, on its neighbours, on the grid nor on the run: every sum of the factor is taken in an order the pattern fixes, without
 * floating-point atomics.  scs_amd_small_solve stays usable on the same object before and after, with the bits it always had.
 * Refused with SCS_FAILED before any device call, sols / infos untouched, the message in scs_amd_small_refusal: a NULL among s,
 * AX, B, Cc, sols, infos or sols[p].x / y / s; PX given without a P, or missing with one; nprob < 1; ldax < nnz(A), ldpx < nnz(P),
 * ldb < m or ldc < n; a non-finite value in AX, PX, B or Cc (the message names the problem); a solve before a set call, or with
 * another nprob than the set call's.
 * A problem whose H_p is not positive definite (an indefinite P_p) is found by the device factor's pivot test (> 0 and finite):
 * that problem alone returns status_val = SCS_FAILED with NaN-filled x, y, s; the call returns 0 and its neighbours are untouched.
 * A HIP failure or a failed allocation in the set call returns SCS_FAILED (message on stderr, no refusal) and leaves the object
 * usable with no values set.
 * Memory, in HBM: per problem of the set call m wA + n wAt values (wA, wAt: the longest row of A and of A'), n^2 for P when
 * present, and m + n for D, E; per workgroup of the largest grid launched a slab of 2 n^2 values for the factor (it follows the
 * grid, not nprob); the per-problem staging of scs_amd_small_solve.  On the host D_p, E_p (m + n values per problem). */
scs_int scs_amd_small_set_values(ScsAmdSmall *s, scs_int nprob, const scs_float *AX, scs_int ldax, const scs_float *PX, scs_int ldpx);
scs_int scs_amd_small_solve_values(ScsAmdSmall *s, scs_int nprob, const scs_float *B, scs_int ldb, const scs_float *Cc, scs_int ldc,
                                   ScsSolution *sols, ScsInfo *infos, scs_int warm_start);
void scs_amd_small_free_values(ScsAmdSmall *s);
/* ---- B1', drop-in form: the reference's internal cone interface -------------------
 * The nine symbols of include/cones.h:80-90 (prefix `_scs_` = glbopts.h's SCS(x)), exported
 * by libscsamd_cones.so so that a reference build links it IN PLACE OF src/cones.o (the
 * reference has no plugin API for cones).  Same argument meaning and return conventions:
 * init returns NULL on failure, proj_dual_cone returns <0 on failure (the reference then
 * aborts with SCS_FAILED, src/scs.c:1389), deep_copy_cone returns 1 on success,
 * get_cone_header returns a malloc'd string the caller frees.  Vectors are HOST pointers
 * (x of length m is projected in place).  `struct SCS_CONE_WORK` is opaque here; the
 * reference only looks inside it under USE_SPECTRAL_CONES, which this backend does not
 * carry.  The device side is created at the first projection (that is when the caller says,
 * through `scal`, whether box bounds are normalised by D: src/cones.c:1557-1565). */
typedef struct SCS_CONE_WORK ScsConeWork;
typedef struct { /* reference include/scs_work.h:24-29 */
  scs_float *D, *E;
  scs_int m, n;
  scs_float primal_scale, dual_scale;
} ScsScaling;
ScsConeWork *_scs_init_cone(ScsCone *k, scs_int m);                      /* src/cones.c:1498 */
scs_int _scs_proj_dual_cone(scs_float *x, ScsConeWork *c, const ScsScaling *scal,
                            scs_float *r_y);                             /* src/cones.c:1552 */
void _scs_finish_cone(ScsConeWork *c);                                   /* src/cones.c:284  */
void _scs_set_r_y(const ScsConeWork *c, scs_float scale, scs_float *r_y);/* src/cones.c:349  */
void _scs_enforce_cone_boundaries(const ScsConeWork *c, scs_float *vec,
                                  scs_float (*f)(const scs_float *, scs_int)); /* :366 */
scs_int _scs_validate_cones(const ScsData *d, const ScsCone *k);         /* src/cones.c:583  */
char *_scs_get_cone_header(const ScsCone *k);                            /* src/cones.c:565  */
scs_int _scs_deep_copy_cone(ScsCone *dest, const ScsCone *src);          /* src/cones.c:154  */
void _scs_free_cone(ScsCone *k);                                         /* src/cones.c:122  */

/* Test hook: the data equilibration scs_init performs (linsys/scs_matrix.c:433-496, 25 Ruiz
 * + 1 L2 pass) on caller-owned CSC arrays.  A->x (and P->x, P may be NULL) are overwritten
 * with the equilibrated values, D (m) and E (n) receive the scalings.  where = 0: host
 * code, 1: the device kernels (bit-identical by construction).  0 on success. */
scs_int scs_amd_equilibrate(ScsMatrix *A, ScsMatrix *P, const ScsCone *k, scs_float *D, scs_float *E,
                            scs_int where);
/* Problem files in the reference's binary layout (src/rw.c:574-705): replaces
 * _scs_write_data / _scs_read_data; a file written by either side is read by the other.
 * `write_data_filename` in ScsSettings makes scs_init write one (src/scs.c:1272-1275).
 * scs_amd_read_data allocates with malloc; release with scs_amd_free_data. */
scs_int scs_amd_write_data(const ScsData *d, const ScsCone *k, const ScsSettings *stgs, const char *filename);
scs_int scs_amd_read_data(const char *filename, ScsData **d, ScsCone **k, ScsSettings **stgs);
void scs_amd_free_data(ScsData *d, ScsCone *k, ScsSettings *stgs);
/* Host-side Anderson acceleration, as used inside scs_solve; same contract as the
 * reference's aa_init / aa_apply / aa_safeguard / aa_reset / aa_finish
 * (include/aa.h:66-143).  Pure host code (exposed so it can be tested without a GPU). */
void *scs_amd_aa_init(scs_int dim, scs_int mem, scs_int min_len, scs_int type1,
                      scs_float regularization, scs_float relaxation,
                      scs_float safeguard_factor, scs_float max_weight_norm,
                      scs_int ir_max_steps);
scs_float scs_amd_aa_apply(scs_float *f, const scs_float *x, void *a);
scs_int scs_amd_aa_safeguard(scs_float *f_new, scs_float *x_new, void *a);
void scs_amd_aa_reset(void *a);
void scs_amd_aa_finish(void *a);
void scs_amd_aa_get_stats(const void *a, AaStats *out);
/* Device-resident Anderson acceleration (what scs_solve uses once n+m+1 >= 32768; the option
 * `aa` = host|dev of scs_amd_set_option forces either): same contract again, replacing aa_init / aa_apply /
 * aa_safeguard / aa_reset / aa_finish of include/aa.h:66-143.  These wrappers take HOST
 * pointers and stage them through HBM so the device path can be pinned against the
 * reference's AA on identical sequences; inside scs_solve the iterates never leave HBM.
 * init returns NULL on bad parameters or any HIP failure; apply returns NaN on a HIP failure. */
void *scs_amd_aa_dev_init(scs_int dim, scs_int mem, scs_int min_len, scs_int type1,
                          scs_float regularization, scs_float relaxation,
                          scs_float safeguard_factor, scs_float max_weight_norm,
                          scs_int ir_max_steps);
scs_float scs_amd_aa_dev_apply(scs_float *f, const scs_float *x, void *a);
scs_int scs_amd_aa_dev_safeguard(scs_float *f_new, scs_float *x_new, void *a);
void scs_amd_aa_dev_reset(void *a);
void scs_amd_aa_dev_finish(void *a);
void scs_amd_aa_dev_get_stats(const void *a, AaStats *out);
/* ---- A block of accelerations at once -------------------------------------------------------------------------------------
 * K = nrhs independent accelerations (1 <= nrhs <= 16) that share their kernels and their read-backs: column k computes what
 * scs_amd_aa_dev_apply / _safeguard compute for that column alone -- its own iteration count, ring slot, memory length, success
 * flag, norms and AaStats; nothing couples the columns -- but every kernel of the reflector sweep is enqueued once for all
 * columns and every host decision of one reflector step is taken from one read-back.  The host synchronisations of one block
 * apply are at most max_k len_k + 4 whatever K is (scs_amd/csrc/aa_multi.h).  Columns may be in different phases in one call:
 * seeding after a reset or a rejection, filling their memory, solving with memories of different lengths.
 * The object has a fixed width W = scs_amd_aa_multi_width(nrhs) in {2, 4, 8, 16} (1 for nrhs == 1, 0 if nrhs < 1 or > 16); there
 * is no chunking beyond 16 columns.  init arguments as scs_amd_aa_dev_init, shared by the columns; NULL on bad arguments or a
 * HIP failure.
 *   Host entries (apply, safeguard): F / X are column-major, nrhs columns of length dim with leading dimension >= dim; rows
 *     beyond dim are not touched.  They stage the columns through HBM (staging buffers are created at the first such call).
 *   Device entries (_dev): F_dev / X_dev are device pointers in the block layout of the other block entries, row-major with
 *     element (i, k) at i * W + k; columns nrhs .. W-1 are neither read nor written.  The caller synchronises its own work before
 *     the call; the call returns with the object's private stream idle (the algorithm reads scalars back anyway).
 *   skip: nrhs flags, or NULL.  Nothing of a skipped column is read or written, its state does not move, aa_norm[k] = 0 and
 *     rejected[k] = 0 (the frozen columns of a family solve).
 *   aa_norm[k]: what aa_apply returns for column k -- 0 while seeding or filling, negative on a rejected solve, positive when
 *     the step was applied (F updated in place).
 *   rejected[k]: 0 or -1, as aa_safeguard returns (-1: F_new / X_new of that column were put back to the last accepted pair and
 *     the column restarts from an empty memory).  A column whose last apply did not succeed is not tested.
 *   nrhs == 1 is the single-vector device path, bit for bit (of the counters only out[0] moves then).  For nrhs > 1 the result
 *     agrees with it to rounding amplified by the least-squares solve, not bit for bit: the sums are ordered differently.  Within
 *     one width the bits of a column depend neither on the other columns nor on its position, and a run repeats bit for bit.
 *   Return: 0 on success; -1 on bad arguments (checked before any device call, F untouched); -1 on a HIP failure (message on
 *     stderr, every column reset, F unspecified, the object stays usable).
 *   reset: col < 0 resets every column.  get_stats: the AaStats of one column.
 *   get_counters: out[0] = block applies, out[1] = host synchronisations inside applies, out[2] = host synchronisations inside
 *     safeguards, out[3] = kernel launches.
 *   Memory, all allocated at init and freed at finish: per column (3 mem + (type1 ? 2 : 1) mem + 1) vectors of dim (S, D, Y and
 *     the QR panel) plus five work vectors (x, f, g, g_prev, and x_work when relaxation != 1).  At dim = 3e6, lookback 10, type I
 *     that is about 1.2 GB per column. */
typedef struct SCS_AMD_AA_MULTI ScsAmdAaMulti;
scs_int scs_amd_aa_multi_width(scs_int nrhs);
ScsAmdAaMulti *scs_amd_aa_multi_init(scs_int dim, scs_int nrhs, scs_int mem, scs_int min_len, scs_int type1,
                                     scs_float regularization, scs_float relaxation, scs_float safeguard_factor,
                                     scs_float max_weight_norm, scs_int ir_max_steps);
scs_int scs_amd_aa_multi_apply(ScsAmdAaMulti *a, scs_float *F, scs_int ldf, const scs_float *X, scs_int ldx,
                               const scs_int *skip, scs_float *aa_norm);
scs_int scs_amd_aa_multi_safeguard(ScsAmdAaMulti *a, scs_float *F_new, scs_int ldf, scs_float *X_new, scs_int ldx,
                                   const scs_int *skip, scs_int *rejected);
scs_int scs_amd_aa_multi_apply_dev(ScsAmdAaMulti *a, scs_float *F_dev, const scs_float *X_dev,
                                   const scs_int *skip, scs_float *aa_norm);
scs_int scs_amd_aa_multi_safeguard_dev(ScsAmdAaMulti *a, scs_float *F_dev, scs_float *X_dev,
                                       const scs_int *skip, scs_int *rejected);
void scs_amd_aa_multi_reset(ScsAmdAaMulti *a, scs_int col);
void scs_amd_aa_multi_get_stats(const ScsAmdAaMulti *a, scs_int col, AaStats *out);
void scs_amd_aa_multi_get_counters(const ScsAmdAaMulti *a, long long out[4]);
void scs_amd_aa_multi_finish(ScsAmdAaMulti *a);
/* ---- ONE linear system split by rows of A across GPUs, native form -------------------------------------------
 * The operator of linsys/cpu/indirect/private.c:106-119 is a sum over row slabs: G = R_x + A' R_y^-1 A = sum_r (R_x / N + A_r' R_r^-1 A_r).
 * Rank r creates a workspace on ITS slab (rows [r0, r1) of A, all n columns, CSC) with diag_r_local = [R_x / N (n) ; R_y of the
 * slab (m_r)]; the PCG of private.c:133-217 then runs device-controlled on every rank with ONE all-reduce of an n-vector per
 * iteration, enqueued on the solver's stream (RCCL, opened with dlopen at the first call: no link-time dependency), and the O(n)
 * part replicated.  All calls on a group of workspaces are collective (every rank calls them in the same order).
 *   scs_amd_shard_unique_id     rank 0 fills 128 opaque bytes; the launcher hands them to every rank (file, socket, ...)
 *   scs_amd_shard_init_rccl     one process per GPU (device = scs_amd_set_device); NULL on failure
 *   scs_amd_shard_solve         b_local = [r_x (n, the same on every rank) ; r_y of the slab] -> [x ; y of the slab], in place;
 *                               s = warm start (n) or NULL; tolerance / return value as scs_solve_lin_sys
 *   scs_amd_shard_group_create / _init_threads / _group_free: a TEST DOUBLE of the collective -- the ranks are host threads of one
 *                               process sharing one GPU -- so that the N = 2 algebra runs on a single-GPU box (RCCL refuses two
 *                               ranks on one device); at most 8 ranks
 *   scs_amd_shard_get_stats     out[0] PCG iterations, out[1] all-reduces enqueued, out[2] all-reduces timed, out[3] their mean us
 *                               (HIP events on the solver's stream; scs_amd_shard_set_profiling(h, 1) switches the sampling on),
 *                               out[4] solves                                                                                     */
typedef struct SCS_AMD_SHARD ScsAmdShard;
scs_int scs_amd_shard_unique_id(char *out128);
ScsAmdShard *scs_amd_shard_init_rccl(const ScsMatrix *A_slab, const scs_float *diag_r_local, scs_int world, scs_int rank, const char *id128);
void *scs_amd_shard_group_create(scs_int world);
void scs_amd_shard_group_free(void *group);
ScsAmdShard *scs_amd_shard_init_threads(const ScsMatrix *A_slab, const scs_float *diag_r_local, void *group, scs_int rank);
scs_int scs_amd_shard_solve(ScsAmdShard *h, scs_float *b_local, const scs_float *s, scs_float tol);
scs_int scs_amd_shard_update_diag_r(ScsAmdShard *h, const scs_float *diag_r_local);
void scs_amd_shard_get_stats(ScsAmdShard *h, double *out);
void scs_amd_shard_set_profiling(ScsAmdShard *h, scs_int on);
void scs_amd_shard_free(ScsAmdShard *h);
/* Test hook for the failure convention (src/scs.c:361-371, :1381-1384, include/linsys.h:25-71): the k-th HIP runtime call
 * the library checks from now on is reported as failed although it succeeded (k <= 0 disarms; SCS_AMD_FAIL_AT=k in the
 * environment arms it at load).  What must follow: scs_init / scs_init_lin_sys_work return NULL with nothing leaked,
 * scs_solve returns SCS_FAILED with a NaN-filled solution and the SIGINT handler restored, scs_solve_lin_sys returns
 * non-zero, and the library stays usable.  Returns the countdown that was armed before the call. */
long long scs_amd_test_fail_at(long long k);
/* ---- options (scs_amd/csrc/options.h holds the table; INTEGRATION.md section 5 prints it) ---------------------------------
 * The reference steers everything through ScsSettings (include/scs.h:61-101) and reads no environment variable.  This
 * library's own switches -- which implementation (host / device) of a step, which kernel schedule -- go through ONE entry:
 *   scs_amd_set_option("reorder", "0")   process-wide; takes effect for workspaces created AFTERWARDS (scs_init,
 *                                        scs_init_lin_sys_work, _scs_init_cone); value NULL = back to the default.
 *                                        Returns 0, or -1 for a key that is not in the table.
 *   scs_amd_get_option("reorder")        the value in force, NULL at the default (or for an unknown key)
 *   scs_amd_list_options(buf, cap)       the table as text, one row per line (key, class, numerics, values, meaning)
 * Environment fallback SCS_AMD_<KEY>: honoured for rows of class `supported` and `diag` only; rows of class `ab` (measurement
 * variants) and `test` (test hooks) are reachable from the environment only when SCS_AMD_ALLOW_ENV_HOOKS=1 is also set. */
scs_int scs_amd_set_option(const char *key, const char *value);
const char *scs_amd_get_option(const char *key);
scs_int scs_amd_list_options(char *buf, scs_int cap);
/* free device memory (bytes) on the selected device after a device-wide synchronise, < 0 on failure */
long long scs_amd_device_free_bytes(void);
/* number of visible HIP devices, or <0 with no usable runtime (never throws) */
scs_int scs_amd_device_count(void);
/* select the device used by subsequently created workspaces (default 0) */
scs_int scs_amd_set_device(scs_int dev);

#ifdef __cplusplus
}
#endif
#endif /* SCS_AMD_H */
