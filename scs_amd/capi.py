"""ctypes view of the C ABI declared in include/scs_amd.h.

The structs mirror reference include/scs.h:47-244 field for field, so the same
Python objects can be handed to libscsamd.so (this repo, HIP) and -- from tests
only -- to a build of the reference.  Nothing here computes anything: it is the
binding a scs-python maintainer would write.

The product library is loaded from scs_amd/lib/ (built in-tree by
``__graft_entry__.build()``); a missing library raises, there is no fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

scs_int = C.c_int


def make_types(ftype, scs_int=C.c_int):
    """Build the struct family for scs_float = ftype (c_double or c_float) and scs_int (c_int, or c_longlong
    for the -DDLONG library)."""
    fp = C.POINTER(ftype)
    ip = C.POINTER(scs_int)

    class ScsMatrix(C.Structure):
        _fields_ = [("x", fp), ("i", ip), ("p", ip), ("m", scs_int), ("n", scs_int)]

    class ScsSettings(C.Structure):
        _fields_ = [
            ("normalize", scs_int), ("scale", ftype), ("adaptive_scale", scs_int),
            ("rho_x", ftype), ("max_iters", scs_int), ("eps_abs", ftype),
            ("eps_rel", ftype), ("eps_infeas", ftype), ("alpha", ftype),
            ("time_limit_secs", ftype), ("verbose", scs_int), ("warm_start", scs_int),
            ("acceleration_lookback", scs_int), ("acceleration_interval", scs_int),
            ("acceleration_type_1", scs_int), ("acceleration_regularization", ftype),
            ("acceleration_relaxation", ftype),
            ("write_data_filename", C.c_char_p), ("log_csv_filename", C.c_char_p),
        ]

    class ScsData(C.Structure):
        _fields_ = [("m", scs_int), ("n", scs_int), ("A", C.POINTER(ScsMatrix)),
                    ("P", C.POINTER(ScsMatrix)), ("b", fp), ("c", fp)]

    class ScsCone(C.Structure):
        _fields_ = [
            ("z", scs_int), ("l", scs_int), ("bu", fp), ("bl", fp), ("bsize", scs_int),
            ("q", ip), ("qsize", scs_int), ("s", ip), ("ssize", scs_int),
            ("cs", ip), ("cssize", scs_int), ("ep", scs_int), ("ed", scs_int),
            ("p", fp), ("psize", scs_int),
        ]

    class ScsSolution(C.Structure):
        _fields_ = [("x", fp), ("y", fp), ("s", fp)]

    class AaStats(C.Structure):
        _fields_ = [
            ("iter", scs_int), ("n_accept", scs_int), ("n_reject_lapack", scs_int),
            ("n_reject_rank0", scs_int), ("n_reject_nonfinite", scs_int),
            ("n_reject_weight_cap", scs_int), ("n_safeguard_reject", scs_int),
            ("last_rank", scs_int), ("last_aa_norm", ftype), ("last_regularization", ftype),
        ]

    class ScsInfo(C.Structure):
        _fields_ = [
            ("iter", scs_int), ("status", C.c_char * 128), ("lin_sys_solver", C.c_char * 128),
            ("status_val", scs_int), ("scale_updates", scs_int), ("pobj", ftype),
            ("dobj", ftype), ("res_pri", ftype), ("res_dual", ftype), ("gap", ftype),
            ("res_infeas", ftype), ("res_unbdd_a", ftype), ("res_unbdd_p", ftype),
            ("setup_time", ftype), ("solve_time", ftype), ("scale", ftype),
            ("comp_slack", ftype), ("rejected_accel_steps", scs_int),
            ("accepted_accel_steps", scs_int), ("aa_stats", AaStats),
            ("lin_sys_time", ftype), ("cone_time", ftype), ("accel_time", ftype),
        ]

    class ScsAmdStats(C.Structure):
        _fields_ = [
            ("cg_iters", C.c_longlong), ("lin_sys_solves", C.c_longlong),
            ("mat_vecs", C.c_longlong), ("spmv_launches", C.c_longlong),
            ("spmv_ms", C.c_double), ("cg_ms", C.c_double), ("cone_ms", C.c_double),
            ("cone_projs", C.c_longlong), ("nnz", C.c_longlong), ("spmv_bytes", C.c_longlong),
            ("psd_unconverged", C.c_longlong),
        ]

    ns = type("ScsTypes", (), {})
    ns.ftype, ns.fp, ns.ip, ns.scs_int = ftype, fp, ip, scs_int
    ns.np_float = np.float64 if ftype is C.c_double else np.float32
    ns.np_int = np.int32 if scs_int is C.c_int else np.int64
    ns.ScsMatrix, ns.ScsSettings, ns.ScsData, ns.ScsCone = ScsMatrix, ScsSettings, ScsData, ScsCone
    ns.ScsSolution, ns.AaStats, ns.ScsInfo, ns.ScsAmdStats = ScsSolution, AaStats, ScsInfo, ScsAmdStats
    return ns


T64 = make_types(C.c_double)
T32 = make_types(C.c_float)
T64L = make_types(C.c_double, C.c_longlong)  # libscsamd_dlong.so


def bind_api(lib, T, full=True, linsys=True, cones=True, stats=True):
    """Attach argtypes/restypes for every entry point the library exports."""
    fp = T.fp
    scs_int = T.scs_int
    if full:
        lib.scs_init.restype = C.c_void_p
        lib.scs_init.argtypes = [C.POINTER(T.ScsData), C.POINTER(T.ScsCone), C.POINTER(T.ScsSettings)]
        lib.scs_update.restype = scs_int
        lib.scs_update.argtypes = [C.c_void_p, fp, fp]
        lib.scs_solve.restype = scs_int
        lib.scs_solve.argtypes = [C.c_void_p, C.POINTER(T.ScsSolution), C.POINTER(T.ScsInfo), scs_int]
        lib.scs_finish.restype = None
        lib.scs_finish.argtypes = [C.c_void_p]
        lib.scs.restype = scs_int
        lib.scs.argtypes = [C.POINTER(T.ScsData), C.POINTER(T.ScsCone), C.POINTER(T.ScsSettings),
                            C.POINTER(T.ScsSolution), C.POINTER(T.ScsInfo)]
        lib.scs_set_default_settings.restype = None
        lib.scs_set_default_settings.argtypes = [C.POINTER(T.ScsSettings)]
        lib.scs_version.restype = C.c_char_p
        lib.scs_version.argtypes = []
    if linsys:
        lib.scs_init_lin_sys_work.restype = C.c_void_p
        lib.scs_init_lin_sys_work.argtypes = [C.POINTER(T.ScsMatrix), C.POINTER(T.ScsMatrix), fp]
        lib.scs_solve_lin_sys.restype = scs_int
        lib.scs_solve_lin_sys.argtypes = [C.c_void_p, fp, fp, T.ftype]
        lib.scs_update_lin_sys_diag_r.restype = scs_int
        lib.scs_update_lin_sys_diag_r.argtypes = [C.c_void_p, fp]
        lib.scs_free_lin_sys_work.restype = None
        lib.scs_free_lin_sys_work.argtypes = [C.c_void_p]
        lib.scs_get_lin_sys_method.restype = C.c_char_p
        lib.scs_get_lin_sys_method.argtypes = []
        if stats:  # extension of the HIP libraries (the `linsys` branch alone also binds the reference backend)
            lib.scs_amd_linsys_update_values.restype = scs_int
            lib.scs_amd_linsys_update_values.argtypes = [C.c_void_p, fp, fp]
    if cones:
        lib.scs_amd_cone_init.restype = C.c_void_p
        lib.scs_amd_cone_init.argtypes = [C.POINTER(T.ScsCone), scs_int, fp]
        lib.scs_amd_cone_proj_dual.restype = scs_int
        lib.scs_amd_cone_proj_dual.argtypes = [C.c_void_p, fp, fp]
        lib.scs_amd_cone_finish.restype = None
        lib.scs_amd_cone_finish.argtypes = [C.c_void_p]
        # blocks of vectors (include/scs_amd.h, B1' section)
        lib.scs_amd_cone_multi_width.restype = scs_int
        lib.scs_amd_cone_multi_width.argtypes = [scs_int]
        lib.scs_amd_cone_proj_dual_multi.restype = scs_int
        lib.scs_amd_cone_proj_dual_multi.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp]
        lib.scs_amd_cone_proj_dual_dev.restype = scs_int
        lib.scs_amd_cone_proj_dual_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]  # device pointers
        lib.scs_amd_cone_proj_dual_multi_dev.restype = scs_int
        lib.scs_amd_cone_proj_dual_multi_dev.argtypes = [C.c_void_p, scs_int, C.c_void_p, C.c_void_p]
        lib.scs_amd_cone_sync.restype = scs_int
        lib.scs_amd_cone_sync.argtypes = [C.c_void_p]
    if stats:
        lib.scs_amd_linsys_get_stats.restype = None
        lib.scs_amd_linsys_get_stats.argtypes = [C.c_void_p, C.POINTER(T.ScsAmdStats)]
        lib.scs_amd_linsys_set_profiling.restype = None
        lib.scs_amd_linsys_set_profiling.argtypes = [C.c_void_p, scs_int]
        lib.scs_amd_linsys_get_cg_pacing.restype = None
        lib.scs_amd_linsys_get_cg_pacing.argtypes = [C.c_void_p, C.POINTER(C.c_longlong * 4)]
        for nm in ("scs_amd_linsys_mat_vec_dev", "scs_amd_linsys_mul_a_dev", "scs_amd_linsys_mul_at_dev"):
            fn = getattr(lib, nm)
            fn.restype = scs_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]  # device pointers
        # blocks of right-hand sides (include/scs_amd.h, B1 section); with the other scs_amd_linsys_* entries: the `linsys` branch also
        # binds the reference backend, which has the five plugin functions only
        lib.scs_amd_solve_lin_sys_multi.restype = scs_int
        lib.scs_amd_solve_lin_sys_multi.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, fp, T.ip]
        lib.scs_amd_linsys_multi_width.restype = scs_int
        lib.scs_amd_linsys_multi_width.argtypes = [scs_int]
        for nm in ("scs_amd_linsys_mat_vec_multi_dev", "scs_amd_linsys_mul_a_multi_dev", "scs_amd_linsys_mul_at_multi_dev"):
            fn = getattr(lib, nm)
            fn.restype = scs_int
            fn.argtypes = [C.c_void_p, scs_int, C.c_void_p, C.c_void_p]  # device pointers
        # every column of a block under its own diag_r
        lib.scs_amd_solve_lin_sys_multi_r.restype = scs_int
        lib.scs_amd_solve_lin_sys_multi_r.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, fp, scs_int, fp, T.ip]
        lib.scs_amd_linsys_mat_vec_multi_r_dev.restype = scs_int
        lib.scs_amd_linsys_mat_vec_multi_r_dev.argtypes = [C.c_void_p, scs_int, C.c_void_p, C.c_void_p, C.c_void_p]  # device pointers
        # every column of a block with its own values of A and P
        lib.scs_amd_linsys_set_values_multi.restype = scs_int
        lib.scs_amd_linsys_set_values_multi.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int]
        lib.scs_amd_solve_lin_sys_multi_v.restype = scs_int
        lib.scs_amd_solve_lin_sys_multi_v.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, fp, scs_int, fp, T.ip]
        lib.scs_amd_linsys_mat_vec_multi_v_dev.restype = scs_int
        lib.scs_amd_linsys_mat_vec_multi_v_dev.argtypes = [C.c_void_p, scs_int, C.c_void_p, C.c_void_p, C.c_void_p]  # device pointers
        lib.scs_amd_linsys_free_values_multi.restype = None
        lib.scs_amd_linsys_free_values_multi.argtypes = [C.c_void_p]
        lib.scs_amd_linsys_sync.restype = scs_int
        lib.scs_amd_linsys_sync.argtypes = [C.c_void_p]
        lib.scs_amd_linsys_spmv_kernel_name.restype = scs_int
        lib.scs_amd_linsys_spmv_kernel_name.argtypes = [C.c_void_p, scs_int, C.c_char_p, scs_int]
        lib.scs_amd_set_option.restype = scs_int
        lib.scs_amd_set_option.argtypes = [C.c_char_p, C.c_char_p]
        lib.scs_amd_get_option.restype = C.c_char_p
        lib.scs_amd_get_option.argtypes = [C.c_char_p]
        lib.scs_amd_list_options.restype = scs_int
        lib.scs_amd_list_options.argtypes = [C.c_char_p, scs_int]
        lib.scs_amd_device_free_bytes.restype = C.c_longlong
        lib.scs_amd_device_free_bytes.argtypes = []
        lib.scs_amd_test_fail_at.restype = C.c_longlong
        lib.scs_amd_test_fail_at.argtypes = [C.c_longlong]
        lib.scs_amd_device_count.restype = scs_int
        lib.scs_amd_device_count.argtypes = []
        lib.scs_amd_set_device.restype = scs_int
        lib.scs_amd_set_device.argtypes = [scs_int]
        if full:
            lib.scs_amd_get_stats.restype = None
            lib.scs_amd_get_stats.argtypes = [C.c_void_p, C.POINTER(T.ScsAmdStats)]
            lib.scs_amd_set_profiling.restype = None
            lib.scs_amd_set_profiling.argtypes = [C.c_void_p, scs_int]
            lib.scs_amd_get_cg_pacing.restype = None
            lib.scs_amd_get_cg_pacing.argtypes = [C.c_void_p, C.POINTER(C.c_longlong * 4)]
            lib.scs_amd_solve_begin.restype = scs_int
            lib.scs_amd_solve_begin.argtypes = [C.c_void_p, C.POINTER(T.ScsSolution), scs_int]
            lib.scs_amd_solve_steps.restype = scs_int
            lib.scs_amd_solve_steps.argtypes = [C.c_void_p, scs_int]
            lib.scs_amd_solve_converged.restype = scs_int
            lib.scs_amd_solve_converged.argtypes = [C.c_void_p]
            lib.scs_amd_solve_end.restype = scs_int
            lib.scs_amd_solve_end.argtypes = [C.c_void_p, C.POINTER(T.ScsSolution), C.POINTER(T.ScsInfo)]
            lib.scs_amd_set_cg_tol_override.restype = None
            lib.scs_amd_set_cg_tol_override.argtypes = [C.c_void_p, C.c_double]
            # a family of problems in one loop (include/scs_amd.h)
            lib.scs_amd_solve_family.restype = scs_int
            lib.scs_amd_solve_family.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, C.POINTER(T.ScsSolution),
                                                 C.POINTER(T.ScsInfo), scs_int]
            lib.scs_amd_solve_family_refusal.restype = C.c_char_p
            lib.scs_amd_solve_family_refusal.argtypes = [C.c_void_p]
            lib.scs_amd_solve_family_scaled.restype = scs_int
            lib.scs_amd_solve_family_scaled.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, fp, C.POINTER(T.ScsSolution),
                                                        C.POINTER(T.ScsInfo), scs_int]
            lib.scs_amd_solve_family_scaled_refusal.restype = C.c_char_p
            lib.scs_amd_solve_family_scaled_refusal.argtypes = [C.c_void_p]
            lib.scs_amd_solve_family_stream.restype = scs_int
            lib.scs_amd_solve_family_stream.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, scs_int, fp, scs_int,
                                                        C.POINTER(T.ScsSolution), C.POINTER(T.ScsInfo), scs_int]
            lib.scs_amd_solve_family_stream_refusal.restype = C.c_char_p
            lib.scs_amd_solve_family_stream_refusal.argtypes = [C.c_void_p, scs_int]
            lib.scs_amd_family_stream_get_counters.restype = None
            lib.scs_amd_family_stream_get_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong * 6)]
            # ... whose columns have their own values of A and P
            lib.scs_amd_family_set_values.restype = scs_int
            lib.scs_amd_family_set_values.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int]
            lib.scs_amd_solve_family_values.restype = scs_int
            lib.scs_amd_solve_family_values.argtypes = lib.scs_amd_solve_family_scaled.argtypes
            lib.scs_amd_family_free_values.restype = None
            lib.scs_amd_family_free_values.argtypes = [C.c_void_p]
            lib.scs_amd_solve_family_values_refusal.restype = C.c_char_p
            lib.scs_amd_solve_family_values_refusal.argtypes = [C.c_void_p]
            lib.scs_amd_box_bounds.restype = scs_int
            lib.scs_amd_box_bounds.argtypes = [C.POINTER(T.ScsCone), fp, fp, fp]
            # a block of Anderson accelerations at once (include/scs_amd.h; scs_amd/accel.py is the object form)
            lib.scs_amd_aa_multi_width.restype = scs_int
            lib.scs_amd_aa_multi_width.argtypes = [scs_int]
            lib.scs_amd_aa_multi_init.restype = C.c_void_p
            lib.scs_amd_aa_multi_init.argtypes = [scs_int] * 5 + [T.ftype] * 4 + [scs_int]
            lib.scs_amd_aa_multi_apply.restype = scs_int
            lib.scs_amd_aa_multi_apply.argtypes = [C.c_void_p, fp, scs_int, fp, scs_int, T.ip, fp]
            lib.scs_amd_aa_multi_safeguard.restype = scs_int
            lib.scs_amd_aa_multi_safeguard.argtypes = [C.c_void_p, fp, scs_int, fp, scs_int, T.ip, T.ip]
            lib.scs_amd_aa_multi_apply_dev.restype = scs_int
            lib.scs_amd_aa_multi_apply_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, T.ip, fp]  # device pointers
            lib.scs_amd_aa_multi_safeguard_dev.restype = scs_int
            lib.scs_amd_aa_multi_safeguard_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, T.ip, T.ip]
            lib.scs_amd_aa_multi_reset.restype = None
            lib.scs_amd_aa_multi_reset.argtypes = [C.c_void_p, scs_int]
            lib.scs_amd_aa_multi_get_stats.restype = None
            lib.scs_amd_aa_multi_get_stats.argtypes = [C.c_void_p, scs_int, C.POINTER(T.AaStats)]
            lib.scs_amd_aa_multi_get_counters.restype = None
            lib.scs_amd_aa_multi_get_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong * 4)]
            lib.scs_amd_aa_multi_finish.restype = None
            lib.scs_amd_aa_multi_finish.argtypes = [C.c_void_p]
            # one linear system split by rows across GPUs, native form (scs_amd/csrc/shard_native.cpp)
            lib.scs_amd_shard_unique_id.restype = scs_int
            lib.scs_amd_shard_unique_id.argtypes = [C.c_char_p]
            lib.scs_amd_shard_init_rccl.restype = C.c_void_p
            lib.scs_amd_shard_init_rccl.argtypes = [C.POINTER(T.ScsMatrix), fp, scs_int, scs_int, C.c_char_p]
            lib.scs_amd_shard_group_create.restype = C.c_void_p
            lib.scs_amd_shard_group_create.argtypes = [scs_int]
            lib.scs_amd_shard_group_free.restype = None
            lib.scs_amd_shard_group_free.argtypes = [C.c_void_p]
            lib.scs_amd_shard_init_threads.restype = C.c_void_p
            lib.scs_amd_shard_init_threads.argtypes = [C.POINTER(T.ScsMatrix), fp, C.c_void_p, scs_int]
            lib.scs_amd_shard_solve.restype = scs_int
            lib.scs_amd_shard_solve.argtypes = [C.c_void_p, fp, fp, T.ftype]
            lib.scs_amd_shard_update_diag_r.restype = scs_int
            lib.scs_amd_shard_update_diag_r.argtypes = [C.c_void_p, fp]
            lib.scs_amd_shard_get_stats.restype = None
            lib.scs_amd_shard_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
            lib.scs_amd_shard_set_profiling.restype = None
            lib.scs_amd_shard_set_profiling.argtypes = [C.c_void_p, scs_int]
            lib.scs_amd_shard_free.restype = None
            lib.scs_amd_shard_free.argtypes = [C.c_void_p]
            lib.scs_amd_update_matrix.restype = scs_int
            lib.scs_amd_update_matrix.argtypes = [C.c_void_p, fp, fp]
            lib.scs_amd_plan_reorder_entries.restype = scs_int
            lib.scs_amd_plan_reorder_entries.argtypes = [C.POINTER(T.ScsMatrix), C.POINTER(T.ScsCone), T.ip, T.ip, T.ip, C.POINTER(C.c_double)]
            lib.scs_amd_plan_reorder.restype = scs_int
            lib.scs_amd_plan_reorder.argtypes = [C.POINTER(T.ScsMatrix), C.POINTER(T.ScsCone), T.ip, T.ip, C.POINTER(C.c_double)]
            lib.scs_amd_get_reorder_info.restype = None
            lib.scs_amd_get_reorder_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
            lib.scs_amd_get_layout_info.restype = None
            lib.scs_amd_get_layout_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
            lib.scs_amd_get_spmv_kernel_name.restype = scs_int
            lib.scs_amd_get_spmv_kernel_name.argtypes = [C.c_void_p, scs_int, C.c_char_p, scs_int]
            lib.scs_amd_set_residuals_every_iter.restype = None
            lib.scs_amd_set_residuals_every_iter.argtypes = [C.c_void_p, scs_int]
            # a batch of small problems, one workgroup per problem (include/scs_amd.h; scs_amd/small.py is the object form)
            lib.scs_amd_small_init.restype = C.c_void_p
            lib.scs_amd_small_init.argtypes = [C.POINTER(T.ScsData), C.POINTER(T.ScsCone), C.POINTER(T.ScsSettings)]
            lib.scs_amd_small_refusal.restype = C.c_char_p
            lib.scs_amd_small_refusal.argtypes = []
            lib.scs_amd_small_limits.restype = None
            lib.scs_amd_small_limits.argtypes = [C.POINTER(scs_int * 2)]
            lib.scs_amd_small_solve.restype = scs_int
            lib.scs_amd_small_solve.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int, C.POINTER(T.ScsSolution),
                                                C.POINTER(T.ScsInfo), scs_int]
            lib.scs_amd_small_set_values.restype = scs_int
            lib.scs_amd_small_set_values.argtypes = [C.c_void_p, scs_int, fp, scs_int, fp, scs_int]
            lib.scs_amd_small_solve_values.restype = scs_int
            lib.scs_amd_small_solve_values.argtypes = lib.scs_amd_small_solve.argtypes
            lib.scs_amd_small_free_values.restype = None
            lib.scs_amd_small_free_values.argtypes = [C.c_void_p]
            lib.scs_amd_small_set_grid.restype = scs_int
            lib.scs_amd_small_set_grid.argtypes = [C.c_void_p, scs_int]
            lib.scs_amd_small_get_counters.restype = None
            lib.scs_amd_small_get_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong * 4)]
            lib.scs_amd_small_get_occupancy.restype = None
            lib.scs_amd_small_get_occupancy.argtypes = [C.c_void_p, C.POINTER(C.c_longlong * 5)]
            lib.scs_amd_small_finish.restype = None
            lib.scs_amd_small_finish.argtypes = [C.c_void_p]
    lib._scs_types = T
    return lib


_cache = {}


def lib_path(name):
    return os.path.join(LIB_DIR, name)


def load(name="libscsamd.so"):
    """Load a product library from scs_amd/lib/.  Raises if it was not built."""
    if name in _cache:
        return _cache[name]
    path = lib_path(name)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback in the product path.")
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    T = T32 if name.endswith("_f32.so") else (T64L if name.endswith("_dlong.so") else T64)
    only_linsys = "linsys" in name
    bind_api(lib, T, full=not only_linsys, linsys=True, cones=not only_linsys, stats=True)
    _cache[name] = lib
    return lib


def set_option(key, value, libs=None):
    """scs_amd_set_option on every product library loaded so far (each shared object keeps its own table): process-wide,
    in force for workspaces created afterwards.  value None = back to the default.  Raises on a key the table does not hold."""
    for name, lib in list(_cache.items()) if libs is None else [(None, l) for l in libs]:
        rc = lib.scs_amd_set_option(key.encode(), None if value is None else str(value).encode())
        if rc != 0:
            raise KeyError(f"scs_amd: unknown option {key!r}")


def list_options(lib=None):
    """The option table of scs_amd/csrc/options.h as a list of dicts (key, cls, numerics, values, doc)."""
    lib = lib or load("libscsamd.so")
    n = lib.scs_amd_list_options(None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.scs_amd_list_options(buf, n + 1)
    rows = []
    for line in buf.value.decode().splitlines():
        k, cls, num, vals, doc = line.split("\t")
        rows.append(dict(key=k, cls=cls, numerics=int(num), values=vals, doc=doc))
    return rows


# ---- numpy <-> struct helpers ---------------------------------------------------

class Problem:
    """Owns the numpy arrays behind one (ScsData, ScsCone) pair so ctypes
    pointers stay valid.  A: scipy.sparse CSC (m x n); P: upper-tri CSC or None."""

    def __init__(self, A, b, c, cone, P=None, T=T64):
        import scipy.sparse as sp
        self.T = T
        f = T.np_float
        A = sp.csc_matrix(A)
        A.sort_indices()
        self.m, self.n = A.shape
        self.Ax = np.ascontiguousarray(A.data, dtype=f)
        self.Ai = np.ascontiguousarray(A.indices, dtype=T.np_int)
        self.Ap = np.ascontiguousarray(A.indptr, dtype=T.np_int)
        self.b = np.ascontiguousarray(b, dtype=f)
        self.c = np.ascontiguousarray(c, dtype=f)
        self.cone = dict(cone)
        self.matA = T.ScsMatrix(self.Ax.ctypes.data_as(T.fp), self.Ai.ctypes.data_as(T.ip),
                                self.Ap.ctypes.data_as(T.ip), self.m, self.n)
        self.matP = None
        if P is not None:
            P = sp.csc_matrix(sp.triu(P))
            P.sort_indices()
            self.Px = np.ascontiguousarray(P.data, dtype=f)
            self.Pi = np.ascontiguousarray(P.indices, dtype=T.np_int)
            self.Pp = np.ascontiguousarray(P.indptr, dtype=T.np_int)
            self.matP = T.ScsMatrix(self.Px.ctypes.data_as(T.fp), self.Pi.ctypes.data_as(T.ip),
                                    self.Pp.ctypes.data_as(T.ip), self.n, self.n)
        self.data = T.ScsData(self.m, self.n, C.pointer(self.matA),
                              C.pointer(self.matP) if self.matP is not None else None,
                              self.b.ctypes.data_as(T.fp), self.c.ctypes.data_as(T.fp))
        self.k = make_cone(self.cone, T, keep=self)

    def sparse(self):
        import scipy.sparse as sp
        return sp.csc_matrix((self.Ax, self.Ai, self.Ap), shape=(self.m, self.n))

    def values_of(self, M, which="A"):
        """New values for A (or, which="P", for P) on the pattern this problem was built with, as the contiguous array the
        update entries take (scs_amd_update_matrix, scs_amd_linsys_update_values).  M: a scipy sparse matrix -- canonicalised as the
        constructor does (CSC, P's upper triangle, sorted indices) and required to have exactly the stored pattern -- or a 1-D array of
        values in that CSC order.  ValueError on any mismatch; the library is not called."""
        import scipy.sparse as sp
        if which == "P" and self.matP is None:
            raise ValueError("this problem has no P")
        ind, ptr = (self.Ai, self.Ap) if which == "A" else (self.Pi, self.Pp)
        shape = (self.m, self.n) if which == "A" else (self.n, self.n)
        if sp.issparse(M):
            if M.shape != shape:
                raise ValueError(f"{which} has shape {M.shape}, the workspace was built for {shape}")
            M = sp.csc_matrix(sp.triu(M)) if which == "P" else sp.csc_matrix(M)
            M.sort_indices()
            if len(M.indices) != len(ind) or not np.array_equal(M.indptr, ptr) or not np.array_equal(M.indices, ind):
                raise ValueError(f"the sparsity pattern of {which} differs from the one the workspace was built with "
                                 "(new values only; a new pattern needs a new workspace)")
            vals = M.data
        else:
            vals = np.asarray(M)
            if vals.ndim != 1 or vals.shape[0] != len(ind):
                raise ValueError(f"{which} values must be a 1-D array of the {len(ind)} stored entries in CSC order")
        return np.ascontiguousarray(vals, dtype=self.T.np_float)


def make_cone(cone, T=T64, keep=None):
    """dict(z=, l=, bu=, bl=, q=[...], s=[...]) -> ScsCone (arrays kept alive on `keep`)."""
    f = T.np_float
    k = T.ScsCone()
    holder = keep if keep is not None else k
    k.z = int(cone.get("z", 0))
    k.l = int(cone.get("l", 0))
    bu = np.ascontiguousarray(cone.get("bu", []), dtype=f)
    bl = np.ascontiguousarray(cone.get("bl", []), dtype=f)
    assert len(bu) == len(bl)
    k.bsize = int(cone.get("bsize", len(bu) + 1 if len(bu) else 0))
    q = np.ascontiguousarray(cone.get("q", []), dtype=T.np_int)
    s = np.ascontiguousarray(cone.get("s", []), dtype=T.np_int)
    pw = np.ascontiguousarray(cone.get("p", []), dtype=f)
    cs = np.ascontiguousarray(cone.get("cs", []), dtype=T.np_int)
    holder._cone_arrays = (bu, bl, q, s, pw, cs)
    k.bu = bu.ctypes.data_as(T.fp) if len(bu) else None
    k.bl = bl.ctypes.data_as(T.fp) if len(bl) else None
    k.q = q.ctypes.data_as(T.ip) if len(q) else None
    k.qsize = len(q)
    k.s = s.ctypes.data_as(T.ip) if len(s) else None
    k.ssize = len(s)
    k.cs = cs.ctypes.data_as(T.ip) if len(cs) else None
    k.cssize = len(cs)
    k.ep, k.ed = int(cone.get("ep", 0)), int(cone.get("ed", 0))
    k.p = pw.ctypes.data_as(T.fp) if len(pw) else None
    k.psize = len(pw)
    return k


def cone_rows(cone):
    """Total number of rows a cone dict covers."""
    q = list(cone.get("q", []))
    s = list(cone.get("s", []))
    bs = cone.get("bsize", len(cone.get("bu", [])) + 1 if len(cone.get("bu", [])) else 0)
    return int(cone.get("z", 0) + cone.get("l", 0) + bs + sum(q) + sum(v * (v + 1) // 2 for v in s) +
               sum(int(v) ** 2 for v in cone.get("cs", [])) +
               3 * (cone.get("ep", 0) + cone.get("ed", 0) + len(cone.get("p", []))))


def cone_and_settings(cone, settings, **defaults):
    """The cone dict and the settings keywords of scs-python as `Problem` and `default_settings` take them: the legacy 'f' joins 'z',
    a scalar for a single cone becomes a list, `use_indirect` / `gpu` / `mkl` / `linear_solver` are dropped (there is one backend),
    file names become bytes, verbose defaults to 0 and every key of `defaults` to its value."""
    cone = dict(cone)
    if "f" in cone:  # scs < 3 name of the zero cone
        cone["z"] = cone.pop("f") + cone.get("z", 0)
    for k in ("q", "s", "cs", "p", "bu", "bl"):  # scs-python accepts scalars for single cones
        if k in cone and np.isscalar(cone[k]):
            cone[k] = [cone[k]]
    kw = {k: v for k, v in settings.items() if k not in ("use_indirect", "gpu", "mkl", "linear_solver")}
    for k in ("write_data_filename", "log_csv_filename"):
        if isinstance(kw.get(k), str):
            kw[k] = kw[k].encode()
    for k, v in dict(verbose=0, **defaults).items():
        kw.setdefault(k, v)
    return cone, kw


def default_settings(lib, **over):
    T = lib._scs_types
    st = T.ScsSettings()
    lib.scs_set_default_settings(C.byref(st))
    for k, v in over.items():
        if not hasattr(st, k):
            raise AttributeError(k)
        setattr(st, k, v)
    return st


INFO_FIELDS = ["iter", "status_val", "scale_updates", "pobj", "dobj", "res_pri", "res_dual", "gap",
               "res_infeas", "res_unbdd_a", "res_unbdd_p", "setup_time", "solve_time", "scale",
               "comp_slack", "rejected_accel_steps", "accepted_accel_steps", "lin_sys_time",
               "cone_time", "accel_time"]


def info_dict(info):
    d = {k: getattr(info, k) for k in INFO_FIELDS}
    d["status"] = info.status.decode()
    d["lin_sys_solver"] = info.lin_sys_solver.decode()
    return d


class SolutionBlock:
    """What K problems of one call come back in: X (n x K), Y and S (m x K), column-major and zero or, with warm = (X, Y, S), filled
    from it; `sols`, an ScsSolution array over their columns, and `infos`, an ScsInfo array, to hand to the library."""

    def __init__(self, T, n, m, K, warm=None):
        self.K = K
        self.X, self.Y, self.S = (np.zeros((rows, K), dtype=T.np_float, order="F") for rows in (n, m, m))
        if warm is not None:
            self.X[:], self.Y[:], self.S[:] = warm
        self.sols, self.infos = (T.ScsSolution * max(K, 1))(), (T.ScsInfo * max(K, 1))()
        x0, y0, s0, sz = self.X.ctypes.data, self.Y.ctypes.data, self.S.ctypes.data, np.dtype(T.np_float).itemsize
        for k, sol in zip(range(K), self.sols):
            sol.x, sol.y, sol.s = C.cast(x0 + k * n * sz, T.fp), C.cast(y0 + k * m * sz, T.fp), C.cast(s0 + k * m * sz, T.fp)

    def results(self):
        """K dicts in the shape of `solve`"""
        return [dict(x=self.X[:, k].copy(), y=self.Y[:, k].copy(), s=self.S[:, k].copy(), info=info_dict(self.infos[k])) for k in range(self.K)]


def solve(lib, prob, settings=None, warm=None, want_stats=False, profiling=False, cg_tol_override=None, **over):
    """scs_init -> scs_solve -> scs_finish through the C ABI of `lib`.
    Returns dict(x, y, s, info[, stats])."""
    T = lib._scs_types
    st = settings if settings is not None else default_settings(lib, **over)
    f = T.np_float
    x = np.zeros(prob.n, dtype=f)
    y = np.zeros(prob.m, dtype=f)
    s = np.zeros(prob.m, dtype=f)
    if warm is not None:
        x[:], y[:], s[:] = warm
    sol = T.ScsSolution(x.ctypes.data_as(T.fp), y.ctypes.data_as(T.fp), s.ctypes.data_as(T.fp))
    info = T.ScsInfo()
    w = lib.scs_init(C.byref(prob.data), C.byref(prob.k), C.byref(st))
    if not w:
        raise RuntimeError("scs_init returned NULL")
    try:
        if profiling and hasattr(lib, "scs_amd_set_profiling"):
            lib.scs_amd_set_profiling(w, 1)
        if cg_tol_override is not None:
            lib.scs_amd_set_cg_tol_override(w, float(cg_tol_override))  # test hook (HIP library only)
        lib.scs_solve(w, C.byref(sol), C.byref(info), 1 if warm is not None else 0)
        out = dict(x=x, y=y, s=s, info=info_dict(info))
        if want_stats and hasattr(lib, "scs_amd_get_stats"):
            stt = T.ScsAmdStats()
            lib.scs_amd_get_stats(w, C.byref(stt))
            out["stats"] = {k: getattr(stt, k) for k, _ in T.ScsAmdStats._fields_}
    finally:
        lib.scs_finish(w)
    return out


def solve_family(lib, w, B, Cc, warm=None, warm_start=None):
    """scs_amd_solve_family on an initialised workspace `w`.  B (m x K), Cc (n x K): anything numpy turns into 2-D arrays;
    they are passed column-major.  warm: (X, Y, S) of shapes n x K, m x K, m x K, or None.  Returns (rc, list of K dicts
    in the shape of `solve`); the arrays of a refused call come back as they went in (zeros, or the warm start)."""
    return _solve_family(lib, w, B, Cc, warm, warm_start, False, None)


def solve_family_scaled(lib, w, B, Cc, scales=None, warm=None, warm_start=None):
    """scs_amd_solve_family_scaled: solve_family with column k under its own scale.  scales: K initial scales, or None for the
    workspace's scale in every column (passed as NULL).  A `scales` that is not K numbers raises ValueError before the library
    is called."""
    return _solve_family(lib, w, B, Cc, warm, warm_start, True, scales)


STREAM_WIDTHS = (0, 2, 4, 8, 16)


def solve_family_stream(lib, w, B, Cc, width=0, own_scale=False, scales=None, warm=None, warm_start=None):
    """scs_amd_solve_family_stream: any number K >= 1 of problems through one block of `width` columns (0: chosen from K), a
    finished column's slot going to the next problem of the queue.  own_scale: scs_amd_solve_family_scaled's form, `scales` as
    there; without it `scales` is passed on as given and the library refuses one.  A width outside STREAM_WIDTHS, a B / Cc that
    are not m x K and n x K, or a `scales` that is not K numbers raise ValueError before the library is called."""
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or int(width) not in STREAM_WIDTHS:
        raise ValueError("width must be 0, 2, 4, 8 or 16")
    return _solve_family(lib, w, B, Cc, warm, warm_start, bool(own_scale), scales, stream_width=int(width))


def family_stream_counters(lib, w):
    """scs_amd_family_stream_get_counters of the last stream call on `w`: a dict of block_iters, run_slot_iters, idle_slot_iters,
    refills, resid_evals, width"""
    out = (C.c_longlong * 6)()
    lib.scs_amd_family_stream_get_counters(w, C.byref(out))
    return dict(zip(("block_iters", "run_slot_iters", "idle_slot_iters", "refills", "resid_evals", "width"), (int(v) for v in out)))


def values_block(V, nnz, what, f):
    """V as the nnz x K column-major block of the family's value entries: a 2-D array of K columns of `nnz` (None: any number of) finite
    values, 1 <= K <= 16.
    ValueError otherwise; the library is not called."""
    V = np.asarray(V, dtype=f)
    if V.ndim != 2 or (nnz is not None and V.shape[0] != nnz):
        raise ValueError(f"{what} must be a 2-D array with one row per stored entry ({nnz}) and one column per problem")
    if not 1 <= V.shape[1] <= 16:
        raise ValueError(f"{what} must have 1 .. 16 columns (set and solve in groups)")
    if not np.all(np.isfinite(V)):
        raise ValueError(f"{what}: matrix values must be finite")
    return np.asfortranarray(V)


def family_set_values(lib, w, AX, PX=None):
    """scs_amd_family_set_values: AX (nnz(A) x K) and, for a workspace with P, PX (nnz(upper P) x K), the values of every column's
    matrices in the CSC order of the matrices given to scs_init.  Shapes and finiteness are checked here (ValueError); whether PX
    goes with the workspace is the library's check.  Returns rc."""
    T = lib._scs_types
    AX = values_block(AX, None, "AX", T.np_float)
    px, ldp = None, 0
    if PX is not None:
        PX = values_block(PX, None, "PX", T.np_float)
        if PX.shape[1] != AX.shape[1]:
            raise ValueError("AX and PX must have the same number of columns")
        px, ldp = PX.ctypes.data_as(T.fp), max(PX.shape[0], 1)
    return lib.scs_amd_family_set_values(w, AX.shape[1], AX.ctypes.data_as(T.fp), max(AX.shape[0], 1), px, ldp)


def family_free_values(lib, w):
    """scs_amd_family_free_values: releases what family_set_values allocated; a solve_family_values is refused until the next set"""
    lib.scs_amd_family_free_values(w)


def solve_family_values(lib, w, B, Cc, scales=None, warm=None, warm_start=None):
    """scs_amd_solve_family_values: solve_family_scaled with column k under the values of the last family_set_values; K must be that
    call's.  Arguments and return as solve_family_scaled."""
    return _solve_family(lib, w, B, Cc, warm, warm_start, True, scales, values=True)


def _solve_family(lib, w, B, Cc, warm, warm_start, scaled, scales, stream_width=None, values=False):
    T = lib._scs_types
    f = T.np_float
    B = np.asfortranarray(np.asarray(B, dtype=f))
    Cc = np.asfortranarray(np.asarray(Cc, dtype=f))
    if B.ndim != 2 or Cc.ndim != 2 or B.shape[1] != Cc.shape[1]:
        raise ValueError("B must be m x K and C n x K")
    m, K = B.shape
    n = Cc.shape[0]
    blk = SolutionBlock(T, n, m, K, warm)
    sols, infos = blk.sols, blk.infos
    ws =(1 if warm is not None else 0) if warm_start is None else int(warm_start)
    sp = None
    if (scaled or stream_width is not None) and scales is not None:
        scales = np.ascontiguousarray(scales, dtype=f)
        if scales.shape != (K,):
            raise ValueError("scales must hold one scale per column of B")
        sp = scales.ctypes.data_as(T.fp)
    if stream_width is not None:
        rc = lib.scs_amd_solve_family_stream(w, K, B.ctypes.data_as(T.fp), m, Cc.ctypes.data_as(T.fp), n, 1 if scaled else 0, sp,
                                             stream_width, sols, infos, ws)
    elif values:
        rc = lib.scs_amd_solve_family_values(w, K, B.ctypes.data_as(T.fp), m, Cc.ctypes.data_as(T.fp), n, sp, sols, infos, ws)
    elif scaled:
        rc = lib.scs_amd_solve_family_scaled(w, K, B.ctypes.data_as(T.fp), m, Cc.ctypes.data_as(T.fp), n, sp, sols, infos, ws)
    else:
        rc = lib.scs_amd_solve_family(w, K, B.ctypes.data_as(T.fp), m, Cc.ctypes.data_as(T.fp), n, sols, infos, ws)
    return rc, blk.results()
