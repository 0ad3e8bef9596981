"""ctypes binding of libplspm_hip.so (C-ABI: include/plspm_hip.h).  No torch, no fallback.

The library is built in-tree by ``make -C plspm-python_amd/csrc`` (or ``__graft_entry__.build()``) into
``plspm/_lib/libplspm_hip.so``.  If it is missing, or no HIP device is visible, the estimator raises
``NativeBackendError`` -- there is deliberately no NumPy path behind this module.
"""
import atexit
import ctypes
import os
import time
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLSPM_HIP_LIB", os.path.join(_HERE, "_lib", "libplspm_hip.so"))
ABI_VERSION = 4

STATUS_OK, STATUS_NOT_CONVERGED, STATUS_SINGULAR, STATUS_NONFINITE = 0, 1, 2, 3
STATUS_INADMISSIBLE = 4      # PLSc, model-fit and geodesic records only (plspm_plsc_*, plspm_modelfit_*, plspm_geodesic_*)
KERNELS = {"resample": 0, "gram": 1, "solver": 2, "scores": 3, "pack": 4, "reduce": 5, "assess": 6, "moderation_counts": 7, "moderation_prepare": 8, "moderation_rows": 9,
           "moderation_finish": 10}
EXPORTS = ["plspm_abi_version", "plspm_device_count", "plspm_last_error", "plspm_model_create", "plspm_model_destroy", "plspm_model_set_nonmetric", "plspm_model_set_categorical", "plspm_model_set_missing", "plspm_model_attach_second_stage", "plspm_model_set_incomplete_rows",
           "plspm_upload", "plspm_effect_pairs", "plspm_row_width", "plspm_row_stride", "plspm_fit", "plspm_bootstrap", "plspm_bootstrap_device", "plspm_bootstrap_summary",
           "plspm_sync", "plspm_stream", "plspm_bootstrap_indices", "plspm_profile_enable", "plspm_profile_read", "plspm_profile_reset",
           "plspm_model_set_option", "plspm_model_get_option", "plspm_bootstrap_moments", "plspm_nonmetric_criteria", "plspm_bootstrap_fetch", "plspm_bootstrap_store", "plspm_rccl_unique_id", "plspm_comm_create", "plspm_comm_destroy",
           "plspm_comm_size", "plspm_comm_uses_rccl", "plspm_group_create", "plspm_group_destroy", "plspm_group_last_error", "plspm_group_size",
           "plspm_group_shard", "plspm_group_bootstrap", "plspm_group_sync", "plspm_group_records", "plspm_group_summary", "plspm_group_rows", "plspm_group_adopt", "plspm_bootstrap_prepare",
           "plspm_group_barrier", "plspm_group_max", "plspm_group_enqueue_times", "plspm_release_cached_memory",
           "plspm_op_inner_weights", "plspm_op_outer_weights", "plspm_op_outer_weights_nonmetric", "plspm_gram_tile_plan",
           "plspm_comm_create_ex", "plspm_comm_split", "plspm_comm_transport", "plspm_comm_max_channels", "plspm_group_set_option", "plspm_group_plan", "plspm_chunk_plan",
           "plspm_permutation_device", "plspm_permutation_counts", "plspm_permutation_members",
           "plspm_stratified_bootstrap_device", "plspm_stratified_pair_counts", "plspm_stratified_draws",
           "plspm_cv_folds", "plspm_cv_device", "plspm_cv_fold_ids", "plspm_cv_moments", "plspm_cv_targets", "plspm_cv_predict",
           "plspm_jackknife_device", "plspm_jackknife_fetch", "plspm_jackknife_stats", "plspm_bootstrap_intervals",
           "plspm_fimix_device", "plspm_fimix_width", "plspm_fimix_fetch", "plspm_fimix_posteriors", "plspm_fimix_starts",
           "plspm_rebus_device", "plspm_rebus_fetch", "plspm_rebus_residuals",
           "plspm_assess_enable", "plspm_assess_width", "plspm_assess_fit", "plspm_assess_fetch", "plspm_assess_summary", "plspm_assess_intervals",
           "plspm_plsc_enable", "plspm_plsc_width", "plspm_plsc_fit", "plspm_plsc_fetch", "plspm_plsc_summary", "plspm_plsc_intervals",
           "plspm_modelfit_enable", "plspm_modelfit_width", "plspm_modelfit_fit", "plspm_modelfit_fetch", "plspm_modelfit_summary", "plspm_modelfit_intervals",
           "plspm_geodesic_enable", "plspm_geodesic_width", "plspm_geodesic_fit", "plspm_geodesic_fetch", "plspm_geodesic_summary", "plspm_geodesic_intervals",
           "plspm_structural_enable", "plspm_structural_width", "plspm_structural_paths", "plspm_structural_fit", "plspm_structural_fetch", "plspm_structural_summary",
           "plspm_structural_intervals",
           "plspm_moderation_enable", "plspm_moderation_width", "plspm_moderation_fit", "plspm_moderation_fetch", "plspm_moderation_summary", "plspm_moderation_intervals",
           "plspm_tetrad_enable", "plspm_tetrad_width", "plspm_tetrad_list", "plspm_tetrad_fit", "plspm_tetrad_fetch", "plspm_tetrad_summary", "plspm_tetrad_intervals",
           "plspm_ipma_enable", "plspm_ipma_width", "plspm_ipma_targets", "plspm_ipma_fit", "plspm_ipma_fetch", "plspm_ipma_summary", "plspm_ipma_intervals",
           "plspm_micom_enable", "plspm_micom_width", "plspm_micom_fetch", "plspm_micom_summary", "plspm_micom_intervals", "plspm_micom_counts"]
CI_METHODS = ("percentile", "basic", "bc", "bca")      # method ids of plspm_bootstrap_intervals
CI_LDS_VALUES = 16384                                  # values of a column its kernel keeps in LDS (csrc/kernels_intervals.h); longer columns take a global scratch slice
UNIQUE_ID_BYTES = 128


class NativeBackendError(RuntimeError):
    pass


class _FitResult(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("weights", "loadings", "crossloadings", "path_coef", "r2", "lv_cov", "total", "direct",
                                               "indirect", "scores", "cov", "mean", "sign", "iterations", "status")]


_lib = None
# live native objects, closed in dependency order (groups -> communicators -> handles) by an atexit hook: at interpreter shutdown
# __del__ runs in arbitrary order and possibly after the HIP / RCCL runtimes have torn themselves down
_live_models, _live_comms, _live_groups = weakref.WeakSet(), weakref.WeakSet(), weakref.WeakSet()


def _shutdown():
    for pool in (_live_groups, _live_comms, _live_models):
        for obj in list(pool):
            try:
                obj.close()
            except Exception:
                pass


atexit.register(_shutdown)


def load():
    """Load the shared library once and declare the signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeBackendError("libplspm_hip.so not found at %s: build it with `make -C plspm-python_amd/csrc` "
                                 "(there is no CPU fallback)" % LIB_PATH)
    # multi-process RCCL / device-memory sharing on this platform needs dmabuf IPC (the host driver has no legacy IPC: without it
    # hipIpcGetMemHandle fails with "invalid argument" inside ncclCommInitRank); the HSA runtime reads the variable when it starts, i.e.
    # at the first HIP call behind this load -- a launcher that scrubbed the environment must not cost the job its collective
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    lib.plspm_abi_version.restype = ctypes.c_int
    lib.plspm_device_count.restype = ctypes.c_int
    lib.plspm_last_error.restype = ctypes.c_char_p
    lib.plspm_last_error.argtypes = [vp]
    lib.plspm_model_create.restype = vp
    lib.plspm_model_create.argtypes = [i32, i32, vp, vp, vp, i32, i32, i32, dbl, i32]
    lib.plspm_model_destroy.restype = None
    lib.plspm_model_destroy.argtypes = [vp]
    lib.plspm_model_set_nonmetric.argtypes = [vp, i32]
    lib.plspm_model_set_categorical.argtypes = [vp, i32, vp, vp]
    lib.plspm_model_set_missing.argtypes = [vp, i32, vp]
    lib.plspm_model_attach_second_stage.argtypes = [vp, vp, vp]
    lib.plspm_model_set_incomplete_rows.argtypes = [vp, i32, vp, vp, i32]
    lib.plspm_upload.argtypes = [vp, vp, i64, i32, i32, vp]
    lib.plspm_effect_pairs.restype = i32
    lib.plspm_effect_pairs.argtypes = [vp, vp, vp]
    lib.plspm_row_width.restype = i32
    lib.plspm_row_width.argtypes = [vp]
    lib.plspm_row_stride.restype = i32
    lib.plspm_row_stride.argtypes = [vp]
    lib.plspm_fit.argtypes = [vp, ctypes.POINTER(_FitResult)]
    lib.plspm_bootstrap.argtypes = [vp, i64, u64, i64, vp, vp, vp, vp]
    lib.plspm_bootstrap_device.argtypes = [vp, i64, u64, i64, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_bootstrap_summary.argtypes = [vp, vp, i64, i32, vp, vp, ctypes.POINTER(i64)]
    lib.plspm_sync.argtypes = [vp]
    lib.plspm_stream.restype = vp
    lib.plspm_stream.argtypes = [vp]
    lib.plspm_bootstrap_indices.argtypes = [u64, i64, i64, vp]
    lib.plspm_permutation_members.argtypes = [u64, i64, i64, i64, vp]
    lib.plspm_permutation_device.argtypes = [vp, i64, u64, i64, i64, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_permutation_counts.argtypes = [vp, i64, vp, vp, ctypes.POINTER(i64)]
    lib.plspm_stratified_draws.argtypes = [u64, i64, i64, vp, vp]
    lib.plspm_stratified_bootstrap_device.argtypes = [vp, i64, u64, i64, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_stratified_pair_counts.argtypes = [vp, i64, vp, vp, vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.plspm_cv_folds.argtypes = [u64, i64, i64, i32, vp]
    lib.plspm_cv_device.argtypes = [vp, i64, i32, u64, i64, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_cv_fold_ids.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.plspm_cv_moments.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.plspm_cv_targets.restype = i32
    lib.plspm_cv_targets.argtypes = [vp, vp]
    lib.plspm_cv_predict.argtypes = [vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.plspm_jackknife_device.argtypes = [vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_jackknife_fetch.argtypes = [vp, i64, i64, vp, vp, vp]
    lib.plspm_jackknife_stats.argtypes = [vp, i64, vp, vp, vp, ctypes.POINTER(i64)]
    lib.plspm_bootstrap_intervals.argtypes = [vp, vp, i64, i32, vp, vp, i32, dbl, vp, ctypes.POINTER(i64)]
    lib.plspm_fimix_starts.argtypes = [u64, i64, i64, i32, vp]
    lib.plspm_fimix_device.argtypes = [vp, i64, vp, i32, u64, i64, vp, i32, dbl, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_fimix_width.restype = i32
    lib.plspm_fimix_width.argtypes = [vp, i32]
    lib.plspm_fimix_fetch.argtypes = [vp, i64, i64, vp, vp, vp]
    lib.plspm_fimix_posteriors.argtypes = [vp, i64, vp]
    lib.plspm_rebus_device.argtypes = [vp, i32, vp, i32, dbl, i64, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.plspm_rebus_fetch.argtypes = [vp] * 12
    lib.plspm_rebus_residuals.argtypes = [vp, vp]
    # the six families of side records (assessment, PLSc, model fit, geodesic discrepancy, structural assessment, MICOM): one set of signatures; only MICOM has no
    # full-sample record
    lib.plspm_structural_paths.argtypes = [vp, ctypes.POINTER(i32), vp, vp, ctypes.POINTER(i32), vp, vp]
    lib.plspm_tetrad_list.argtypes = [vp, ctypes.POINTER(i32), vp, vp, vp, vp, vp]
    lib.plspm_ipma_targets.argtypes = [vp, ctypes.POINTER(i32), vp]
    for family in ("assess", "plsc", "modelfit", "geodesic", "structural", "micom", "moderation", "tetrad", "ipma"):
        getattr(lib, "plspm_%s_enable" % family).argtypes = ([vp, i32, vp] if family in ("plsc", "modelfit", "geodesic") else [vp, i32, vp, vp, vp] if family in ("moderation", "ipma")
                                                             else [vp, i32, vp, i32, i32] if family == "tetrad" else [vp, i32])
        getattr(lib, "plspm_%s_width" % family).restype = i32
        getattr(lib, "plspm_%s_width" % family).argtypes = [vp]
        if family != "micom":
            getattr(lib, "plspm_%s_fit" % family).argtypes = [vp, vp, ctypes.POINTER(i32)]
        getattr(lib, "plspm_%s_fetch" % family).argtypes = [vp, i64, i64, vp, vp]
        getattr(lib, "plspm_%s_summary" % family).argtypes = [vp, i64, vp, vp, ctypes.POINTER(i64)]
        getattr(lib, "plspm_%s_intervals" % family).argtypes = [vp, i64, vp, i32, dbl, vp, ctypes.POINTER(i64)]
    lib.plspm_micom_counts.argtypes = [vp, i64, vp, vp, vp, ctypes.POINTER(i64)]
    lib.plspm_profile_enable.argtypes = [vp, i32]
    lib.plspm_profile_read.argtypes = [vp, i32, ctypes.POINTER(dbl), ctypes.POINTER(i64)]
    lib.plspm_profile_reset.argtypes = [vp]
    lib.plspm_model_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    lib.plspm_model_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32)]
    lib.plspm_model_get_option.restype = ctypes.c_int
    lib.plspm_bootstrap_fetch.argtypes = [vp, i64, i64, vp, vp, vp]
    lib.plspm_bootstrap_moments.argtypes = [vp, i64, u64, i64, vp, vp]
    lib.plspm_nonmetric_criteria.argtypes = [vp, i64, vp]
    lib.plspm_bootstrap_store.argtypes = [vp, vp, i64]
    lib.plspm_bootstrap_prepare.argtypes = [vp]
    lib.plspm_rccl_unique_id.argtypes = [vp]
    lib.plspm_comm_create.restype = vp
    lib.plspm_comm_create.argtypes = [vp, i32, i32, i32, vp]
    lib.plspm_comm_create_ex.restype = vp
    lib.plspm_comm_create_ex.argtypes = [vp, i32, i32, i32, vp, i32, i32]
    lib.plspm_comm_split.restype = vp
    lib.plspm_comm_split.argtypes = [vp, i32]
    lib.plspm_comm_transport.restype = i32
    lib.plspm_comm_transport.argtypes = [vp]
    lib.plspm_comm_max_channels.restype = i32
    lib.plspm_comm_max_channels.argtypes = [vp]
    lib.plspm_group_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    lib.plspm_group_plan.argtypes = [vp, i64, ctypes.POINTER(i32), vp, vp]
    lib.plspm_chunk_plan.argtypes = [i64, i64, i32, i32, i64, vp]
    lib.plspm_comm_destroy.restype = None
    lib.plspm_comm_destroy.argtypes = [vp]
    lib.plspm_comm_size.restype = i32
    lib.plspm_comm_size.argtypes = [vp]
    lib.plspm_comm_uses_rccl.restype = i32
    lib.plspm_comm_uses_rccl.argtypes = [vp]
    lib.plspm_group_create.restype = vp
    lib.plspm_group_create.argtypes = [vp, vp]
    lib.plspm_group_destroy.restype = None
    lib.plspm_group_destroy.argtypes = [vp]
    lib.plspm_group_last_error.restype = ctypes.c_char_p
    lib.plspm_group_last_error.argtypes = [vp]
    lib.plspm_group_size.restype = i32
    lib.plspm_group_size.argtypes = [vp]
    lib.plspm_group_shard.argtypes = [vp, i64, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.plspm_group_bootstrap.argtypes = [vp, i64, u64, i64]
    lib.plspm_group_sync.argtypes = [vp]
    lib.plspm_group_records.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.plspm_group_summary.argtypes = [vp, vp, vp, ctypes.POINTER(i64)]
    lib.plspm_group_rows.argtypes = [vp, vp, vp, vp]
    lib.plspm_group_adopt.argtypes = [vp]
    lib.plspm_group_barrier.argtypes = [vp]
    lib.plspm_group_max.argtypes = [vp, ctypes.POINTER(dbl)]
    lib.plspm_group_enqueue_times.argtypes = [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
    lib.plspm_op_inner_weights.argtypes = [i32, i32, i32, vp, vp, i64, vp]
    lib.plspm_op_outer_weights.argtypes = [i32, i32, vp, vp, i64, i32, vp]
    lib.plspm_op_outer_weights_nonmetric.argtypes = [i32, i32, vp, vp, vp, i64, i32, dbl, vp, vp]
    if lib.plspm_abi_version() != ABI_VERSION:
        raise NativeBackendError("libplspm_hip.so ABI %d != expected %d" % (lib.plspm_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def device_count():
    return load().plspm_device_count()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def bootstrap_indices(seed, rep, n):
    """Host mirror of the on-device resampling stream (Philox4x32-10 keyed by (seed, replicate))."""
    idx = np.empty(n, dtype=np.int32)
    rc = load().plspm_bootstrap_indices(seed, rep, n, _ptr(idx))
    if rc:
        raise NativeBackendError("plspm_bootstrap_indices failed (%d)" % rc)
    return idx


def permutation_members(seed, perm, n, n1):
    """Host mirror of the on-device splits of the two-group permutation test: [n] bools, True = group a of permutation ``perm``."""
    member = np.empty(n, dtype=np.uint8)
    rc = load().plspm_permutation_members(seed, perm, n, n1, _ptr(member))
    if rc:
        raise NativeBackendError("plspm_permutation_members failed (%d)" % rc)
    return member.astype(bool)


def stratified_draws(seed, rep, member):
    """Host mirror of the on-device draws of the two-group bootstrap for resample ``rep``: [n] int32, entries [0, n_a) the drawn rows of
    group a (``member`` True), [n_a, n) those of group b."""
    member = np.ascontiguousarray(member, dtype=np.uint8)
    rows = np.empty(member.shape[0], dtype=np.int32)
    rc = load().plspm_stratified_draws(seed, rep, member.shape[0], _ptr(member), _ptr(rows))
    if rc:
        raise NativeBackendError("plspm_stratified_draws failed (%d)" % rc)
    return rows


def cv_folds(seed, rep, n, k):
    """Host mirror of the on-device fold draw of the k-fold cross-validation: [n] uint8, the fold of every row in repetition ``rep``."""
    fold = np.empty(n, dtype=np.uint8)
    rc = load().plspm_cv_folds(seed, rep, n, k, _ptr(fold))
    if rc:
        raise NativeBackendError("plspm_cv_folds failed (%d)" % rc)
    return fold


def fimix_starts(seed, start, n, k):
    """Host mirror of the on-device initial assignment of FIMIX-PLS: [n] uint8, the segment (below ``k``) of every row in start ``start``."""
    segment = np.empty(n, dtype=np.uint8)
    rc = load().plspm_fimix_starts(seed, start, n, k, _ptr(segment))
    if rc:
        raise NativeBackendError("plspm_fimix_starts failed (%d)" % rc)
    return segment


def i8_tile_plan(count_tiles, pair_tiles, cus=256, mix=True):
    """Host mirror of the int8 Gram's tile-row cut (plspm_gram_tile_plan): (launch of the 320-replicate kernel taken?, tall rows, short rows)."""
    tall, shrt = ctypes.c_int32(0), ctypes.c_int32(0)
    lib = load()
    lib.plspm_gram_tile_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    rc = lib.plspm_gram_tile_plan(count_tiles, pair_tiles, cus, 1 if mix else 0, ctypes.byref(tall), ctypes.byref(shrt))
    if rc not in (0, 1):
        raise NativeBackendError("plspm_gram_tile_plan failed (%d)" % rc)
    return bool(rc), tall.value, shrt.value


def chunk_plan(B, bytes_per_unit, chunks=0, ratio_pct=60, align=0):
    """Host mirror of the sub-batch planner (plspm_chunk_plan): the sizes of the sub-batches ONE call of B units runs as."""
    lib = load()
    parts = np.zeros(8, dtype=np.int64)
    n = lib.plspm_chunk_plan(B, bytes_per_unit, chunks, ratio_pct, align, _ptr(parts))
    if n < 1:
        raise NativeBackendError("plspm_chunk_plan failed (%d)" % n)
    return [int(v) for v in parts[:n]]


class NativeModel:
    """One compiled model on one GPU (an opaque ``plspm_model_t*``)."""

    def __init__(self, block_offset, path, modes, scheme, scaled, max_iter, tol, device_id=0, nonmetric=False, categorical=None, missing=None):
        lib = load()
        if lib.plspm_device_count() <= 0:
            raise NativeBackendError("no HIP device visible: the MI355X backend has no CPU fallback")
        self._lib = lib
        self.block_offset = np.ascontiguousarray(block_offset, dtype=np.int32)
        self.L = len(self.block_offset) - 1
        self.P = int(self.block_offset[-1])
        path = np.ascontiguousarray(path, dtype=np.uint8)
        modes = np.ascontiguousarray(modes, dtype=np.int32)
        self.n_endo = int((path.reshape(self.L, self.L).sum(axis=1) > 0).sum())      # LVs that have a predecessor
        self._h = lib.plspm_model_create(self.P, self.L, _ptr(self.block_offset), _ptr(path), _ptr(modes), int(scheme), int(bool(scaled)),
                                         int(max_iter), float(tol), int(device_id))
        if not self._h:
            raise NativeBackendError("plspm_model_create: " + lib.plspm_last_error(None).decode())
        if nonmetric:
            self._check(lib.plspm_model_set_nonmetric(self._h, 1), "plspm_model_set_nonmetric")
        self.P_out = self.P             # per-MV outputs: logical MVs (== device columns unless categorical)
        self.n_upload_cols = self.P     # device columns of the resident matrix (+ missing indicators, set below)
        if categorical is not None:     # (mv_off, mv_kind): device columns are indicator-augmented, see plspm_model_set_categorical
            mv_off = np.ascontiguousarray(categorical[0], dtype=np.int32)
            mv_kind = np.ascontiguousarray(categorical[1], dtype=np.int32)
            self.P_out = len(mv_kind)
            self._check(lib.plspm_model_set_categorical(self._h, self.P_out, _ptr(mv_off), _ptr(mv_kind)), "plspm_model_set_categorical")
        if missing is not None:         # ind_of [P]: upload column of every incomplete data column's 0/1 missing indicator (else -1)
            ind_of = np.ascontiguousarray(missing, dtype=np.int32)
            self._check(lib.plspm_model_set_missing(self._h, int((ind_of >= 0).sum()), _ptr(ind_of)), "plspm_model_set_missing")
            self.n_upload_cols = self.P + int((ind_of >= 0).sum())
        self.n_eff = lib.plspm_effect_pairs(self._h, None, None)
        ef = np.zeros(max(self.n_eff, 1), dtype=np.int32)
        et = np.zeros(max(self.n_eff, 1), dtype=np.int32)
        lib.plspm_effect_pairs(self._h, _ptr(ef), _ptr(et))
        self.eff_from, self.eff_to = ef[:self.n_eff], et[:self.n_eff]
        self.row_width = lib.plspm_row_width(self._h)
        self.row_stride = lib.plspm_row_stride(self._h)     # device rows: [row | status | iterations]
        self.N = 0
        self.last_B = 0
        self.device_id = int(device_id)
        _live_models.add(self)

    def set_incomplete_rows(self, rows, present, raw_scale=False):
        """Non-metric data with missing values (plspm_model_set_incomplete_rows), after ``upload``: ``rows`` ascending row numbers,
        ``present`` [K, P] booleans in device column order."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        present = np.ascontiguousarray(present, dtype=np.uint8)
        if present.shape != (len(rows), self.P):
            raise ValueError("present must have shape (K, P)")
        self._check(self._lib.plspm_model_set_incomplete_rows(self._h, len(rows), _ptr(rows), _ptr(present), int(bool(raw_scale))),
                    "plspm_model_set_incomplete_rows")

    def attach_second_stage(self, second, lv_first):
        """Two-stage HOC bootstrap (plspm_model_attach_second_stage): ``second`` is the data-less stage-2 handle; afterwards
        this handle's bootstrap rows / effect pairs / row width are the second stage's."""
        lv_first = np.ascontiguousarray(lv_first, dtype=np.int32)
        self._check(self._lib.plspm_model_attach_second_stage(self._h, second._h, _ptr(lv_first)), "plspm_model_attach_second_stage")
        self._second = second                       # keeps the stage-2 handle alive as long as this one
        self.n_eff, self.eff_from, self.eff_to = second.n_eff, second.eff_from, second.eff_to
        self.row_width = self._lib.plspm_row_width(self._h)
        self.row_stride = self._lib.plspm_row_stride(self._h)

    def _check(self, rc, what):
        if rc:
            raise NativeBackendError("%s failed (%d): %s" % (what, rc, self._lib.plspm_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plspm_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, X, col_index=None):
        """X: 2-D float64 array (C- or F-contiguous, used in place); col_index[p] = source column of device column p."""
        X = np.asarray(X)
        if X.dtype != np.float64 or X.ndim != 2:
            X = np.ascontiguousarray(X, dtype=np.float64)
        if X.flags.c_contiguous:
            layout = 0
        elif X.flags.f_contiguous:
            layout = 1
        else:
            X, layout = np.ascontiguousarray(X), 0
        ci = None if col_index is None else np.ascontiguousarray(col_index, dtype=np.int32)
        self._check(self._lib.plspm_upload(self._h, _ptr(X), X.shape[0], X.shape[1], layout, _ptr(ci)), "plspm_upload")
        self.N = X.shape[0]

    def fit(self, want_scores=True, want_cov=False, scores_out=None):
        """``scores_out``: a caller-owned [N, L] float64 C-contiguous buffer for the scores (as ``bootstrap(out=...)``: nothing is allocated -- or first
        touched -- per call; a fresh 160 MB array costs more in page faults than its copy over the link)."""
        P, L, ne = self.P_out, self.L, self.n_eff
        if scores_out is not None and (scores_out.shape != (self.N, L) or scores_out.dtype != np.float64 or not scores_out.flags.c_contiguous):
            raise ValueError("scores_out = [N, L] float64, C-contiguous")
        out = dict(weights=np.empty(P), loadings=np.empty(P), crossloadings=np.empty((P, L)), path_coef=np.empty((L, L)), r2=np.empty(L),
                   lv_cov=np.empty((L, L)), total=np.empty(ne), direct=np.empty(ne), indirect=np.empty(ne),
                   scores=(scores_out if scores_out is not None else np.empty((self.N, L))) if want_scores else None, cov=np.empty((P, P)) if want_cov else None, mean=np.empty(P),
                   sign=np.empty(L, dtype=np.int8), iterations=np.zeros(1, dtype=np.int32), status=np.full(1, -1, dtype=np.int32))
        res = _FitResult(**{k: (v.ctypes.data if v is not None and v.size else None) for k, v in out.items()})
        self._check(self._lib.plspm_fit(self._h, ctypes.byref(res)), "plspm_fit")
        out["iterations"] = int(out["iterations"][0])
        out["status"] = int(out["status"][0])
        return out

    def bootstrap(self, B, seed=0, rep_offset=0, idx=None, out=None):
        """Returns (rows [B, R], status [B], iters [B]) on the host."""
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            if idx.shape != (B, self.N):
                raise ValueError("idx must have shape (B, N)")
        if out is None:
            rows, status, iters = np.empty((B, self.row_width)), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        else:                                      # caller-owned buffers (the C-ABI's contract): nothing is allocated -- or first touched -- per call
            rows, status, iters = out
            if rows.shape != (B, self.row_width) or rows.dtype != np.float64 or not rows.flags.c_contiguous or status.shape != (B,) or iters.shape != (B,) \
                    or status.dtype != np.int32 or iters.dtype != np.int32:
                raise ValueError("out = (rows [B, row_width] float64, status [B] int32, iters [B] int32), C-contiguous")
        self._check(self._lib.plspm_bootstrap(self._h, B, seed, rep_offset, _ptr(idx), _ptr(rows), _ptr(status), _ptr(iters)), "plspm_bootstrap")
        self.last_B = B
        return rows, status, iters

    def bootstrap_moments(self, B, seed=0, rep_offset=0, idx=None):
        """Test seam (plspm_bootstrap_moments): the replicates' moment matrices [B, C, C] of the uploaded columns + the ones column,
        from the Gram path the ``gram_path`` option selects; no solver."""
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            if idx.shape != (B, self.N):
                raise ValueError("idx must have shape (B, N)")
        C = self.n_upload_cols + 1
        out = np.empty((B, C, C))
        self._check(self._lib.plspm_bootstrap_moments(self._h, B, seed, rep_offset, _ptr(idx), _ptr(out)), "plspm_bootstrap_moments")
        return out

    def nonmetric_criteria(self, B):
        """Test seam (plspm_nonmetric_criteria): the stop-rule value each of the first B problems of the last non-metric run was decided on."""
        out = np.empty(B)
        self._check(self._lib.plspm_nonmetric_criteria(self._h, B, _ptr(out)), "plspm_nonmetric_criteria")
        return out

    def prepare_bootstrap(self):
        """Enqueue the per-data-set preparation of a later bootstrap (digit planes of the int8 Gram) beside whatever runs next."""
        self._check(self._lib.plspm_bootstrap_prepare(self._h), "plspm_bootstrap_prepare")

    def bootstrap_device(self, B, seed=0, rep_offset=0):
        """Enqueue B replicates; returns raw device pointers (rows, status, iters) owned by the handle."""
        d_out, d_st, d_it = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.plspm_bootstrap_device(self._h, B, seed, rep_offset, None, ctypes.byref(d_out), ctypes.byref(d_st), ctypes.byref(d_it)),
                    "plspm_bootstrap_device")
        self.last_B = B
        return d_out.value, d_st.value, d_it.value

    def permutation(self, B, n1, seed=0, rep_offset=0, member=None):
        """Enqueue B permutations of the two-group test (plspm_permutation_device): 2B records stay on the handle, record 2p = group a
        (n1 rows) of permutation rep_offset + p, 2p + 1 = its group b.  ``member`` [B, N] bools: explicit memberships instead of the
        on-device splits (tests)."""
        if member is not None:
            member = np.ascontiguousarray(member, dtype=np.uint8)
            if member.shape != (B, self.N):
                raise ValueError("member must have shape (B, N)")
        d_out, d_st, d_it = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.plspm_permutation_device(self._h, B, seed, rep_offset, n1, _ptr(member), ctypes.byref(d_out), ctypes.byref(d_st),
                                                       ctypes.byref(d_it)), "plspm_permutation_device")
        self.last_B = 2 * B
        return d_out.value, d_st.value, d_it.value

    def permutation_counts(self, B, observed_diff):
        """Exceedance counts of the last ``permutation`` call (plspm_permutation_counts): ([R] int64 #{valid p : |d_p| >= |observed_diff|},
        number of valid permutations)."""
        observed_diff = np.ascontiguousarray(observed_diff, dtype=np.float64)
        if observed_diff.shape != (self.row_width,):
            raise ValueError("observed_diff must have row_width entries")
        exceed = np.empty(self.row_width, dtype=np.int64)
        used = ctypes.c_int64(0)
        self._check(self._lib.plspm_permutation_counts(self._h, B, _ptr(observed_diff), _ptr(exceed), ctypes.byref(used)), "plspm_permutation_counts")
        return exceed, used.value

    def stratified_bootstrap(self, B, member, seed=0, rep_offset=0, draws=None):
        """Enqueue B resamples of the two-group bootstrap (plspm_stratified_bootstrap_device): ``member`` [N] bools (True = group a); 2B
        records stay on the handle, record 2p = group a of resample rep_offset + p, 2p + 1 = its group b.  ``draws`` [B, N] int32: explicit
        draws in the layout of ``stratified_draws`` instead of the on-device ones (tests)."""
        member = np.ascontiguousarray(member, dtype=np.uint8)
        if member.shape != (self.N,):
            raise ValueError("member must have N entries")
        if draws is not None:
            draws = np.ascontiguousarray(draws, dtype=np.int32)
            if draws.shape != (B, self.N):
                raise ValueError("draws must have shape (B, N)")
        d_out, d_st, d_it = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.plspm_stratified_bootstrap_device(self._h, B, seed, rep_offset, _ptr(member), _ptr(draws), ctypes.byref(d_out),
                                                                ctypes.byref(d_st), ctypes.byref(d_it)), "plspm_stratified_bootstrap_device")
        self.last_B = 2 * B
        return d_out.value, d_st.value, d_it.value

    def stratified_pair_counts(self, B, center_a, center_b):
        """Henseler's all-pairs counts on the last ``stratified_bootstrap`` call (plspm_stratified_pair_counts): ([R] int64 #{(i, k) :
        2 center_a - x_a,i > 2 center_b - x_b,k}, OK records of group a, OK records of group b)."""
        center_a = np.ascontiguousarray(center_a, dtype=np.float64)
        center_b = np.ascontiguousarray(center_b, dtype=np.float64)
        if center_a.shape != (self.row_width,) or center_b.shape != (self.row_width,):
            raise ValueError("center_a / center_b must have row_width entries")
        above = np.empty(self.row_width, dtype=np.int64)
        used_a, used_b = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.plspm_stratified_pair_counts(self._h, B, _ptr(center_a), _ptr(center_b), _ptr(above), ctypes.byref(used_a),
                                                           ctypes.byref(used_b)), "plspm_stratified_pair_counts")
        return above, used_a.value, used_b.value

    def cv(self, reps, k, seed=0, rep_offset=0, fold=None):
        """Enqueue ``reps`` repetitions of a k-fold cross-validation (plspm_cv_device): reps * k records stay on the handle, record r * k + f =
        the fit on the rows outside fold f of repetition rep_offset + r.  ``fold`` [reps, N] uint8: explicit fold ids instead of the on-device
        draw (tests)."""
        if fold is not None:
            fold = np.ascontiguousarray(fold, dtype=np.uint8)
            if fold.shape != (reps, self.N):
                raise ValueError("fold must have shape (reps, N)")
        d_out, d_st, d_it = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.plspm_cv_device(self._h, reps, k, seed, rep_offset, _ptr(fold), ctypes.byref(d_out), ctypes.byref(d_st), ctypes.byref(d_it)),
                    "plspm_cv_device")
        self.last_B = reps * k
        return d_out.value, d_st.value, d_it.value

    def cv_fold_ids(self, reps, k):
        """What the last ``cv`` call left on the handle (plspm_cv_fold_ids): (fold [reps, N] uint8, order [reps, N] int32, offsets [reps, k + 1] int32)."""
        fold = np.empty((reps, self.N), dtype=np.uint8)
        order = np.empty((reps, self.N), dtype=np.int32)
        offsets = np.empty((reps, k + 1), dtype=np.int32)
        self._check(self._lib.plspm_cv_fold_ids(self._h, reps, k, _ptr(fold), _ptr(order), _ptr(offsets)), "plspm_cv_fold_ids")
        return fold, order, offsets

    def cv_moments(self, reps, k, cross=True):
        """Training moments of the last ``cv`` call's problems (plspm_cv_moments): (n_train [reps * k], mean [reps * k, P] of the raw columns,
        cross [reps * k, P (P + 1) / 2] centred cross-products, upper triangle by rows -- or None)."""
        nprob, P = reps * k, self.P
        n_train, mean = np.empty(nprob), np.empty((nprob, P))
        packed = np.empty((nprob, P * (P + 1) // 2)) if cross else None
        self._check(self._lib.plspm_cv_moments(self._h, reps, k, _ptr(n_train), _ptr(mean), _ptr(packed)), "plspm_cv_moments")
        return n_train, mean, packed

    def cv_targets(self):
        """Device columns of the target indicators (plspm_cv_targets): the MVs of every LV that has a predecessor."""
        cols = np.empty(self.P, dtype=np.int32)
        return cols[:self._lib.plspm_cv_targets(self._h, _ptr(cols))].copy()

    def cv_predict(self, reps, k, technique=0, coef=None, predictions=False):
        """Out-of-sample errors of the last ``cv`` call's problems (plspm_cv_predict): (sse, sae, sst [reps * k, T], rows [reps * k], pred_sum [N, T]
        or None, pred_cnt [N] or None).  ``coef`` [reps * k, T, P + 1]: explicit affine maps of the raw row instead of the PLS prediction."""
        nprob, T = reps * k, len(self.cv_targets())
        if coef is not None:
            coef = np.ascontiguousarray(coef, dtype=np.float64)
            if coef.shape != (nprob, T, self.P + 1):
                raise ValueError("coef must have shape (reps * k, T, P + 1)")
        sse, sae, sst = np.empty((nprob, T)), np.empty((nprob, T)), np.empty((nprob, T))
        rows = np.empty(nprob, dtype=np.int64)
        pred_sum = np.empty((self.N, T)) if predictions else None
        pred_cnt = np.empty(self.N, dtype=np.int32) if predictions else None
        self._check(self._lib.plspm_cv_predict(self._h, reps, k, int(technique), _ptr(coef), _ptr(sse), _ptr(sae), _ptr(sst), _ptr(rows), _ptr(pred_sum),
                                               _ptr(pred_cnt)), "plspm_cv_predict")
        return sse, sae, sst, rows, pred_sum, pred_cnt

    def jackknife(self, groups=None):
        """Enqueue the jackknife (plspm_jackknife_device): problem g of ``groups`` (None: N, leave-one-out) is the fit on the rows i with
        i % groups != g.  Its records live beside the handle's bootstrap records, which survive the call.  Returns the device pointers
        (rows, status, iters)."""
        G = self.N if groups is None else int(groups)
        d_out, d_st, d_it = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.plspm_jackknife_device(self._h, G, ctypes.byref(d_out), ctypes.byref(d_st), ctypes.byref(d_it)), "plspm_jackknife_device")
        self.last_G = G
        return d_out.value, d_st.value, d_it.value

    def jackknife_fetch(self, first=0, count=None):
        """Host copy of problems [first, first + count) of the last ``jackknife`` call: (rows [count, R], status, iters)."""
        if count is None:
            count = getattr(self, "last_G", 0) - first
        rows = np.empty((max(count, 0), self.row_width))
        status = np.empty(max(count, 0), dtype=np.int32)
        iters = np.empty(max(count, 0), dtype=np.int32)
        self._check(self._lib.plspm_jackknife_fetch(self._h, first, count, _ptr(rows), _ptr(status), _ptr(iters)), "plspm_jackknife_fetch")
        return rows, status, iters

    def jackknife_stats(self, groups=None):
        """Device reduction of the last ``jackknife`` call (plspm_jackknife_stats): (mean [R], std_error [R], accel [R], number of OK problems)."""
        G = self.N if groups is None else int(groups)
        mean, se, accel = np.empty(self.row_width), np.empty(self.row_width), np.empty(self.row_width)
        used = ctypes.c_int64(0)
        self._check(self._lib.plspm_jackknife_stats(self._h, G, _ptr(mean), _ptr(se), _ptr(accel), ctypes.byref(used)), "plspm_jackknife_stats")
        return mean, se, accel, used.value

    def fimix(self, k_of, kmax=None, seed=0, start_offset=0, init=None, max_iter=5000, tol=1e-10):
        """Enqueue FIMIX-PLS problems on the scores the last ``fit`` left on the device (plspm_fimix_device): problem s has ``k_of[s]`` segments and starts
        from ``init[s]`` ([nprob, N] uint8 segments) or, with ``init`` None, from the Philox draw keyed by (seed, start_offset + s).  Returns the device
        pointers (records, status, iters)."""
        k_of = np.ascontiguousarray(k_of, dtype=np.int32).ravel()
        kmax = int(k_of.max()) if kmax is None else int(kmax)
        if init is not None:
            init = np.ascontiguousarray(init, dtype=np.uint8)
            if init.shape != (len(k_of), self.N):
                raise ValueError("init must have shape (nprob, N)")
        d_out, d_st, d_it = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.plspm_fimix_device(self._h, len(k_of), _ptr(k_of), kmax, seed, start_offset, _ptr(init), int(max_iter), float(tol), ctypes.byref(d_out),
                                                 ctypes.byref(d_st), ctypes.byref(d_it)), "plspm_fimix_device")
        self.last_fimix = (len(k_of), kmax, k_of.copy())
        return d_out.value, d_st.value, d_it.value

    def rebus(self, classes, start, max_iter=100, stop_crit=0.005, min_size=10):
        """REBUS-PLS on the uploaded rows (plspm_rebus_device): ``start`` [N] labels below ``classes``.  Returns ``rebus_fetch()``."""
        start = np.ascontiguousarray(start, dtype=np.int32)
        if start.shape != (self.N,):
            raise ValueError("start = [N] labels")
        self._check(self._lib.plspm_rebus_device(self._h, int(classes), _ptr(start), int(max_iter), float(stop_crit), int(min_size), None, None), "plspm_rebus_device")
        self.last_rebus = (int(classes), int(max_iter))
        return self.rebus_fetch()

    def rebus_fetch(self):
        """Host copy of the last ``rebus`` run (plspm_rebus_fetch): dict(status, iterations, labels [N], cm [N, K], records [K, R], rec_status, rec_iters [K],
        sizes [K], within_e [K, P] (device column order), within_f [K, n_endo], changed [h], hist_sizes [h, K])."""
        K, max_iter = getattr(self, "last_rebus", (0, 0))
        n_endo = self.n_endo
        out = dict(labels=np.empty(self.N, dtype=np.int32), cm=np.empty((self.N, max(K, 1))), records=np.empty((max(K, 1), self.row_width)), rec_status=np.empty(max(K, 1), dtype=np.int32),
                   rec_iters=np.empty(max(K, 1), dtype=np.int32), sizes=np.empty(max(K, 1), dtype=np.int64), within_e=np.empty((max(K, 1), self.P)), within_f=np.empty((max(K, 1), n_endo)))
        run = np.zeros(3, dtype=np.int32)
        changed, hist = np.zeros(max(max_iter, 1), dtype=np.int32), np.zeros((max(max_iter, 1), max(K, 1)), dtype=np.int32)
        self._check(self._lib.plspm_rebus_fetch(self._h, _ptr(out["labels"]), _ptr(out["cm"]), _ptr(out["records"]), _ptr(out["rec_status"]), _ptr(out["rec_iters"]), _ptr(out["sizes"]),
                                                _ptr(out["within_e"]), _ptr(out["within_f"]), _ptr(run), _ptr(changed), _ptr(hist)), "plspm_rebus_fetch")
        out.update(status=int(run[0]), iterations=int(run[1]), changed=changed[:run[2]].copy(), hist_sizes=hist[:run[2]].copy())
        return out

    def rebus_residuals(self):
        """e [N, P] (device column order) and f [N, n_endo] of every row under the one-class model (plspm_rebus_residuals)."""
        n_endo = self.n_endo
        out = np.empty((self.N, self.P + n_endo))
        self._check(self._lib.plspm_rebus_residuals(self._h, _ptr(out)), "plspm_rebus_residuals")
        return out[:, :self.P].copy(), out[:, self.P:].copy()

    def fimix_width(self, kmax):
        return int(self._lib.plspm_fimix_width(self._h, int(kmax)))

    def fimix_fetch(self, first=0, count=None):
        """Host copy of problems [first, first + count) of the last ``fimix`` call: (records [count, width], status, iters)."""
        nprob, kmax, _ = getattr(self, "last_fimix", (0, 1, None))
        if count is None:
            count = nprob - first if nprob else 1      # (no call yet: the library says so)
        rows = np.empty((max(count, 0), self.fimix_width(kmax)))
        status = np.empty(max(count, 0), dtype=np.int32)
        iters = np.empty(max(count, 0), dtype=np.int32)
        self._check(self._lib.plspm_fimix_fetch(self._h, first, count, _ptr(rows), _ptr(status), _ptr(iters)), "plspm_fimix_fetch")
        return rows, status, iters

    def fimix_posteriors(self, problem):
        """The posteriors [N, K] of the stored parameters of one problem of the last ``fimix`` call (plspm_fimix_posteriors)."""
        nprob, _, k_of = getattr(self, "last_fimix", (0, 1, None))
        K = int(k_of[problem]) if k_of is not None and 0 <= problem < nprob else 1
        out = np.empty((self.N, K))
        self._check(self._lib.plspm_fimix_posteriors(self._h, int(problem), _ptr(out)), "plspm_fimix_posteriors")
        return out

    # ---- side records: the assessment, PLSc and model-fit records of a plain bootstrap and the MICOM records of a permutation call.  One C signature per
    # operation (plspm_<family>_enable / _width / _fit / _fetch / _summary / _intervals), so one implementation each; the public methods below name the family.
    def _side_call(self, family, op, *args):
        name = "plspm_%s_%s" % (family, op)
        self._check(getattr(self._lib, name)(self._h, *args), name)

    def _side_width(self, family):
        return int(getattr(self._lib, "plspm_%s_width" % family)(self._h))

    def _side_fit(self, family):
        out = np.empty(self._side_width(family))
        status = ctypes.c_int32(-1)
        self._side_call(family, "fit", _ptr(out), ctypes.byref(status))
        return out, status.value

    def _side_fetch(self, family, first, count):
        out = np.empty((max(count, 0), self._side_width(family)))
        status = np.empty(max(count, 0), dtype=np.int32)
        self._side_call(family, "fetch", first, count, _ptr(out), _ptr(status))
        return out, status

    def _side_table(self, family, op, B, original, method=None, level=None):
        """``summary`` (no method) / ``intervals`` of a family: ([width, 6] table, records used)."""
        width = self._side_width(family)
        original = np.ascontiguousarray(original, dtype=np.float64)
        if original.shape != (width,):
            raise ValueError("original must have %s_width entries" % family)
        how = () if method is None else (CI_METHODS.index(method) if isinstance(method, str) else int(method), float(level))
        out = np.empty((width, 6))
        used = ctypes.c_int64(0)
        self._side_call(family, op, B, _ptr(original), *how, _ptr(out), ctypes.byref(used))
        return out, used.value

    def assess_enable(self, on=True):
        """Measurement-model assessment (plspm_assess_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the assessment record
        alpha | rho_a | rho_c | ave [L each] | htmt | htmt2 | lv_cor [L (L - 1) / 2 each] of every replicate; the bootstrap's own records do not change."""
        self._side_call("assess", "enable", int(bool(on)))

    @property
    def assess_width(self):
        return self._side_width("assess")

    def assess_fit(self):
        """The full-sample assessment record (plspm_assess_fit): ([A] values, status of the solver problem behind them)."""
        return self._side_fit("assess")

    def assess_fetch(self, first=0, count=None):
        """Host copy of the assessment records [first, first + count) of the last assessed bootstrap: (records [count, A], status [count])."""
        return self._side_fetch("assess", first, self.last_B - first if count is None else count)

    def assess_summary(self, B, original):
        """``summary`` on the assessment records (plspm_assess_summary): ([A, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("assess", "summary", B, original)

    def assess_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the assessment records (plspm_assess_intervals; no bca): ([A, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("assess", "intervals", B, original, method, level)

    def moderation_enable(self, terms):
        """Moderation analysis (plspm_moderation_enable): ``terms`` a list of (predictor, moderator, target) LV indices -- every later ``bootstrap`` /
        ``bootstrap_device`` call also writes the record direct2 [n_dir] | interaction | f2 | slope_low | slope_high [T each] | r2 [L] of every replicate; no other
        record changes.  An empty list (or None) switches it off."""
        terms = np.ascontiguousarray(np.asarray(terms if terms is not None else [], dtype=np.int32).reshape(-1, 3).T)
        self._side_call("moderation", "enable", terms.shape[1], _ptr(terms[0]) if terms.shape[1] else None, _ptr(terms[1]) if terms.shape[1] else None,
                        _ptr(terms[2]) if terms.shape[1] else None)

    @property
    def moderation_width(self):
        return self._side_width("moderation")

    def moderation_fit(self):
        """The full-sample moderation record (plspm_moderation_fit): ([W] values, the record's status)."""
        return self._side_fit("moderation")

    def moderation_fetch(self, first=0, count=None):
        """Host copy of the moderation records [first, first + count) of the last moderated bootstrap: (records [count, W], status [count])."""
        return self._side_fetch("moderation", first, self.last_B - first if count is None else count)

    def moderation_summary(self, B, original):
        """``summary`` on the moderation records (plspm_moderation_summary): ([W, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("moderation", "summary", B, original)

    def moderation_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the moderation records (plspm_moderation_intervals; no bca): ([W, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("moderation", "intervals", B, original, method, level)

    def tetrad_enable(self, on=True, mask=None, tetrads="basis", matrix="correlation"):
        """Confirmatory tetrad analysis (plspm_tetrad_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the tetrads of the tested blocks of
        every replicate; no other record changes.  mask: uint8 [L], the tested blocks (None: every block of at least four items); tetrads "basis" / "all" (or 0 / 1);
        matrix "correlation" / "covariance" (or 0 / 1)."""
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (self.L,):
                raise ValueError("mask must have one entry per latent variable")
        set_id = ("basis", "all").index(tetrads) if isinstance(tetrads, str) else int(tetrads)
        matrix_id = ("correlation", "covariance").index(matrix) if isinstance(matrix, str) else int(matrix)
        self._side_call("tetrad", "enable", int(bool(on)), _ptr(mask) if mask is not None else None, set_id, matrix_id)

    @property
    def tetrad_width(self):
        return self._side_width("tetrad")

    def tetrad_list(self):
        """The tetrads in record order (plspm_tetrad_list): (block [n_tet] LV indices, a, b, c, d [n_tet] device-order MV indices)."""
        n = ctypes.c_int32(0)
        self._side_call("tetrad", "list", ctypes.byref(n), None, None, None, None, None)
        out = [np.empty(n.value, dtype=np.int32) for _ in range(5)]
        self._side_call("tetrad", "list", None, *[_ptr(v) for v in out])
        return tuple(out)

    def tetrad_fit(self):
        """The full-sample tetrad record (plspm_tetrad_fit): ([n_tet] values, the record's status)."""
        return self._side_fit("tetrad")

    def tetrad_fetch(self, first=0, count=None):
        """Host copy of the tetrad records [first, first + count) of the last bootstrap with tetrads: (records [count, n_tet], status [count])."""
        return self._side_fetch("tetrad", first, self.last_B - first if count is None else count)

    def tetrad_summary(self, B, original):
        """``summary`` on the tetrad records (plspm_tetrad_summary): ([n_tet, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("tetrad", "summary", B, original)

    def tetrad_intervals(self, B, original, method="bc", level=0.95):
        """``intervals`` on the tetrad records (plspm_tetrad_intervals; no bca): ([n_tet, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("tetrad", "intervals", B, original, method, level)

    def ipma_enable(self, on=True, targets=None, lo=None, hi=None):
        """Importance-performance map analysis (plspm_ipma_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the record perf [L] | sd [L] |
        total_u [n_eff] | direct_u [n_eff] | weight_r [P] | mvperf [P] | mvimp [n_t x P] of every replicate; no other record changes.  targets: uint8 [L], the
        target LVs (None: every LV with a predecessor); lo / hi: float64 [P], the bounds of every MV in device order."""
        if not on:
            self._side_call("ipma", "enable", 0, None, None, None)
            return
        if targets is not None:
            targets = np.ascontiguousarray(targets, dtype=np.uint8)
            if targets.shape != (self.L,):
                raise ValueError("targets must have one entry per latent variable")
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        if lo.shape != (self.P,) or hi.shape != (self.P,):
            raise ValueError("lo and hi must have one entry per manifest variable")
        self._side_call("ipma", "enable", 1, _ptr(targets) if targets is not None else None, _ptr(lo), _ptr(hi))

    @property
    def ipma_width(self):
        return self._side_width("ipma")

    def ipma_targets(self):
        """The target LVs of the record's mvimp rows, ascending (plspm_ipma_targets)."""
        n = ctypes.c_int32(0)
        self._side_call("ipma", "targets", ctypes.byref(n), None)
        out = np.empty(n.value, dtype=np.int32)
        self._side_call("ipma", "targets", None, _ptr(out))
        return out

    def ipma_fit(self):
        """The full-sample IPMA record (plspm_ipma_fit): ([W] values, the record's status)."""
        return self._side_fit("ipma")

    def ipma_fetch(self, first=0, count=None):
        """Host copy of the IPMA records [first, first + count) of the last bootstrap with the map on: (records [count, W], status [count])."""
        return self._side_fetch("ipma", first, self.last_B - first if count is None else count)

    def ipma_summary(self, B, original):
        """``summary`` on the IPMA records (plspm_ipma_summary): ([W, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("ipma", "summary", B, original)

    def ipma_intervals(self, B, original, method="bc", level=0.95):
        """``intervals`` on the IPMA records (plspm_ipma_intervals; no bca): ([W, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("ipma", "intervals", B, original, method, level)

    def structural_enable(self, on=True):
        """Structural-model assessment (plspm_structural_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the record f2 [n_dir] |
        vif [n_dir] | specific [n_spec] of every replicate -- and the assessment records, which the kernel reads; no other record changes."""
        self._side_call("structural", "enable", int(bool(on)))

    @property
    def structural_width(self):
        return self._side_width("structural")

    def structural_paths(self):
        """The direct paths and the chains in record order (plspm_structural_paths): (dir_from [n_dir], dir_to [n_dir], chain_off [n_spec + 1], chain_nodes)."""
        n_dir, n_spec = ctypes.c_int32(0), ctypes.c_int32(0)
        self._side_call("structural", "paths", ctypes.byref(n_dir), None, None, ctypes.byref(n_spec), None, None)
        dir_from, dir_to = np.empty(n_dir.value, dtype=np.int32), np.empty(n_dir.value, dtype=np.int32)
        chain_off = np.empty(n_spec.value + 1, dtype=np.int32)
        self._side_call("structural", "paths", None, _ptr(dir_from), _ptr(dir_to), None, _ptr(chain_off), None)
        chain_nodes = np.empty(max(int(chain_off[-1]), 1), dtype=np.int32)
        self._side_call("structural", "paths", None, None, None, None, None, _ptr(chain_nodes))
        return dir_from, dir_to, chain_off, chain_nodes[:int(chain_off[-1])]

    def structural_fit(self):
        """The full-sample structural record (plspm_structural_fit): ([S] values, the record's status)."""
        return self._side_fit("structural")

    def structural_fetch(self, first=0, count=None):
        """Host copy of the structural records [first, first + count) of the last structural bootstrap: (records [count, S], status [count])."""
        return self._side_fetch("structural", first, self.last_B - first if count is None else count)

    def structural_summary(self, B, original):
        """``summary`` on the structural records (plspm_structural_summary): ([S, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("structural", "summary", B, original)

    def structural_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the structural records (plspm_structural_intervals; no bca): ([S, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("structural", "intervals", B, original, method, level)

    def plsc_enable(self, on=True, factor=None):
        """Consistent PLS (plspm_plsc_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the PLSc record weights | r2 | total | direct |
        loadings | lv_cor_c of every replicate -- and the assessment records, which the PLSc kernel reads; the bootstrap's own records do not change.
        ``factor``: 0 / 1 per LV (None: every Mode-A block of two items or more)."""
        mask = None
        if factor is not None:
            mask = np.ascontiguousarray(factor, dtype=np.uint8)
            if mask.shape != (self.L,):
                raise ValueError("factor must have one entry per latent variable")
        self._check(self._lib.plspm_plsc_enable(self._h, int(bool(on)), _ptr(mask) if mask is not None else None), "plspm_plsc_enable")

    @property
    def plsc_width(self):
        return self._side_width("plsc")

    def plsc_fit(self):
        """The full-sample PLSc record (plspm_plsc_fit): ([W] values, the record's status)."""
        return self._side_fit("plsc")

    def plsc_fetch(self, first=0, count=None):
        """Host copy of the PLSc records [first, first + count) of the last PLSc bootstrap: (records [count, W], status [count])."""
        return self._side_fetch("plsc", first, self.last_B - first if count is None else count)

    def plsc_summary(self, B, original):
        """``summary`` on the PLSc records (plspm_plsc_summary): ([W, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("plsc", "summary", B, original)

    def plsc_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the PLSc records (plspm_plsc_intervals; no bca): ([W, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("plsc", "intervals", B, original, method, level)

    def modelfit_enable(self, on=True, factor=None):
        """Model fit (plspm_modelfit_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the record srmr_sat | d_uls_sat | srmr_est |
        d_uls_est of every replicate -- and the assessment and PLSc records, which the model-fit kernel builds on; the bootstrap's own records do not change.
        ``factor``: 0 / 1 per LV, the handle's one factor mask (None: the mask the handle has, PLSc's default if none was ever set)."""
        mask = None
        if factor is not None:
            mask = np.ascontiguousarray(factor, dtype=np.uint8)
            if mask.shape != (self.L,):
                raise ValueError("factor must have one entry per latent variable")
        self._check(self._lib.plspm_modelfit_enable(self._h, int(bool(on)), _ptr(mask) if mask is not None else None), "plspm_modelfit_enable")

    @property
    def modelfit_width(self):
        return self._side_width("modelfit")

    def modelfit_fit(self):
        """The full-sample model-fit record (plspm_modelfit_fit): ([4] values, the record's status)."""
        return self._side_fit("modelfit")

    def modelfit_fetch(self, first=0, count=None):
        """Host copy of the model-fit records [first, first + count) of the last model-fit bootstrap: (records [count, 4], status [count])."""
        return self._side_fetch("modelfit", first, self.last_B - first if count is None else count)

    def modelfit_summary(self, B, original):
        """``summary`` on the model-fit records (plspm_modelfit_summary): ([4, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("modelfit", "summary", B, original)

    def modelfit_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the model-fit records (plspm_modelfit_intervals; no bca): ([4, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("modelfit", "intervals", B, original, method, level)

    def geodesic_enable(self, on=True, factor=None):
        """Geodesic discrepancy (plspm_geodesic_enable): every later ``bootstrap`` / ``bootstrap_device`` call also writes the record d_g_sat | d_g_est of every
        replicate -- and the assessment, PLSc and model-fit records, which the geodesic kernel builds on; the bootstrap's own records do not change.
        ``factor``: as in ``modelfit_enable`` (the handle has one factor mask)."""
        mask = None
        if factor is not None:
            mask = np.ascontiguousarray(factor, dtype=np.uint8)
            if mask.shape != (self.L,):
                raise ValueError("factor must have one entry per latent variable")
        self._check(self._lib.plspm_geodesic_enable(self._h, int(bool(on)), _ptr(mask) if mask is not None else None), "plspm_geodesic_enable")

    @property
    def geodesic_width(self):
        return self._side_width("geodesic")

    def geodesic_fit(self):
        """The full-sample geodesic record (plspm_geodesic_fit): ([2] values, the record's status)."""
        return self._side_fit("geodesic")

    def geodesic_fetch(self, first=0, count=None):
        """Host copy of the geodesic records [first, first + count) of the last geodesic bootstrap: (records [count, 2], status [count])."""
        return self._side_fetch("geodesic", first, self.last_B - first if count is None else count)

    def geodesic_summary(self, B, original):
        """``summary`` on the geodesic records (plspm_geodesic_summary): ([2, 6] original, mean, std.error, perc.025, perc.975, t stat.; OK replicates)."""
        return self._side_table("geodesic", "summary", B, original)

    def geodesic_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the geodesic records (plspm_geodesic_intervals; no bca): ([2, 6] lower, upper, z0, accel, level.lower, level.upper; OK replicates)."""
        return self._side_table("geodesic", "intervals", B, original, method, level)

    def micom_enable(self, on=True):
        """MICOM (plspm_micom_enable): every later ``permutation`` call also writes the record c | dmean | dlogvar [L each] of every permutation --
        compositional invariance and the differences of the pooled composite's means and log variances; the permutation's own records do not change."""
        self._side_call("micom", "enable", int(bool(on)))

    @property
    def micom_width(self):
        return self._side_width("micom")

    def micom_fetch(self, first=0, count=None):
        """Host copy of the MICOM records [first, first + count) of the last MICOM permutation call: (records [count, 3 L], status [count])."""
        return self._side_fetch("micom", first, self.last_B // 2 - first if count is None else count)

    def micom_summary(self, B, original):
        """``summary`` on the MICOM records (plspm_micom_summary): ([3 L, 6] original, mean, std.error, perc.025, perc.975, t stat.; valid permutations)."""
        return self._side_table("micom", "summary", B, original)

    def micom_intervals(self, B, original, method="percentile", level=0.95):
        """``intervals`` on the MICOM records (plspm_micom_intervals; no bca): ([3 L, 6] lower, upper, z0, accel, level.lower, level.upper; valid permutations)."""
        return self._side_table("micom", "intervals", B, original, method, level)

    def micom_counts(self, B, observed):
        """Counts on the MICOM records of the last MICOM permutation call (plspm_micom_counts): ([3 L] int64 #{valid r : x_r <= observed},
        [3 L] int64 #{valid r : |x_r| >= |observed|}, number of valid permutations)."""
        observed = np.ascontiguousarray(observed, dtype=np.float64)
        if observed.shape != (self.micom_width,):
            raise ValueError("observed must have micom_width entries")
        below = np.empty(self.micom_width, dtype=np.int64)
        exceed = np.empty(self.micom_width, dtype=np.int64)
        used = ctypes.c_int64(0)
        self._check(self._lib.plspm_micom_counts(self._h, B, _ptr(observed), _ptr(below), _ptr(exceed), ctypes.byref(used)), "plspm_micom_counts")
        return below, exceed, used.value

    def intervals(self, B, original, method="percentile", level=0.95, accel=None, d_rows=None, stride=0):
        """Device confidence intervals of the last bootstrap on this handle, or of the device records at ``d_rows`` (plspm_bootstrap_intervals).
        Returns ([R, 6] array: lower, upper, z0, accel, level.lower, level.upper; number of OK replicates)."""
        original = np.ascontiguousarray(original, dtype=np.float64)
        if original.shape != (self.row_width,):
            raise ValueError("original must have row_width entries")
        if accel is not None:
            accel = np.ascontiguousarray(accel, dtype=np.float64)
            if accel.shape != (self.row_width,):
                raise ValueError("accel must have row_width entries")
        mid = CI_METHODS.index(method) if isinstance(method, str) else int(method)
        out = np.empty((self.row_width, 6))
        used = ctypes.c_int64(0)
        self._check(self._lib.plspm_bootstrap_intervals(self._h, d_rows, B, stride, _ptr(original), _ptr(accel), mid, float(level), _ptr(out), ctypes.byref(used)),
                    "plspm_bootstrap_intervals")
        return out, used.value

    def summary(self, B, original, d_rows=None, stride=0):
        """Device-side _create_summary of the last bootstrap on this handle (or of the device records at ``d_rows``).
        Returns ([R, 6] array: original, mean, std.error, perc.025, perc.975, t stat.; number of OK replicates)."""
        original = np.ascontiguousarray(original, dtype=np.float64)
        if original.shape != (self.row_width,):
            raise ValueError("original must have row_width entries")
        out = np.empty((self.row_width, 6))
        used = ctypes.c_int64(0)
        self._check(self._lib.plspm_bootstrap_summary(self._h, d_rows, B, stride, _ptr(original), _ptr(out), ctypes.byref(used)), "plspm_bootstrap_summary")
        return out, used.value

    def fetch(self, first=0, count=None):
        """Host copy of replicates [first, first + count) of the LAST bootstrap / bootstrap_device / store on this handle (their
        records are still in HBM): (rows [count, R], status, iters)."""
        if count is None:
            count = self.last_B - first
        rows = np.empty((count, self.row_width))
        status = np.empty(count, dtype=np.int32)
        iters = np.empty(count, dtype=np.int32)
        self._check(self._lib.plspm_bootstrap_fetch(self._h, first, count, _ptr(rows), _ptr(status), _ptr(iters)), "plspm_bootstrap_fetch")
        return rows, status, iters

    def store(self, records):
        """Put merged host records [B, row_stride] (device layout: row | status | iterations) into the handle, e.g. shards that a
        host-side transport gathered; ``summary`` / ``fetch`` then work on them."""
        records = np.ascontiguousarray(records, dtype=np.float64)
        if records.ndim != 2 or records.shape[1] != self.row_stride:
            raise ValueError("records must have shape (B, row_stride)")
        self._check(self._lib.plspm_bootstrap_store(self._h, _ptr(records), records.shape[0]), "plspm_bootstrap_store")
        self.last_B = records.shape[0]

    def set_option(self, key, value):
        """Launch-geometry option of the handle (include/plspm_hip.h, plspm_model_set_option)."""
        self._check(self._lib.plspm_model_set_option(self._h, key.encode(), int(value)), "plspm_model_set_option")

    def get_option(self, key):
        """Current value of an option; ``"last_gram_path"``: 1 = fp64 MFMA Gram, 2 = int8 digit-plane Gram (last bootstrap call)."""
        v = ctypes.c_int32(0)
        self._check(self._lib.plspm_model_get_option(self._h, key.encode(), ctypes.byref(v)), "plspm_model_get_option")
        return v.value

    def stream_ptr(self):
        """The handle's hipStream_t as an integer."""
        return int(self._lib.plspm_stream(self._h) or 0)

    def sync(self):
        self._check(self._lib.plspm_sync(self._h), "plspm_sync")

    def profile(self, on=True, only=None):
        """HIP-event timing of the handle's kernels: every kernel, or (``only="gram"`` ...) just one of them."""
        self._lib.plspm_profile_enable(self._h, (2 + KERNELS[only]) if (on and only is not None) else int(bool(on)))

    def profile_reset(self):
        self._lib.plspm_profile_reset(self._h)

    def profile_read(self, kernel):
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        self._check(self._lib.plspm_profile_read(self._h, KERNELS[kernel], ctypes.byref(ms), ctypes.byref(n)), "plspm_profile_read")
        return ms.value, n.value


def op_inner_weights(scheme_code, path, y, device_id=0):
    """Scheme operator on the device (plspm_op_inner_weights): path [L, L] 0/1, y [N, L] scores -> E [L, L]."""
    lib = load()
    path = np.ascontiguousarray(path, dtype=np.uint8)
    y = np.ascontiguousarray(y, dtype=np.float64)
    L = path.shape[0]
    if path.shape != (L, L) or y.ndim != 2 or y.shape[1] != L:
        raise ValueError("path must be L x L and y N x L")
    E = np.empty((L, L))
    rc = lib.plspm_op_inner_weights(int(device_id), int(scheme_code), L, _ptr(path), _ptr(y), y.shape[0], _ptr(E))
    if rc:
        raise NativeBackendError("plspm_op_inner_weights failed (%d): %s" % (rc, lib.plspm_last_error(None).decode()))
    return E


def op_outer_weights(mode_code, Xk, z, device_id=0):
    """Mode operator on the device (plspm_op_outer_weights): Xk [N, k], z [N] -> w [k]."""
    lib = load()
    Xk = np.ascontiguousarray(Xk, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    if Xk.ndim != 2 or z.shape[0] != Xk.shape[0]:
        raise ValueError("Xk must be N x k and z of length N")
    w = np.empty(Xk.shape[1])
    rc = lib.plspm_op_outer_weights(int(device_id), int(mode_code), _ptr(Xk), _ptr(z), Xk.shape[0], Xk.shape[1], _ptr(w))
    if rc:
        raise NativeBackendError("plspm_op_outer_weights failed (%d): %s" % (rc, lib.plspm_last_error(None).decode()))
    return w


def op_outer_weights_nonmetric(mode_code, Xk, present, z, correction, device_id=0):
    """Non-metric Mode operator on the device (plspm_op_outer_weights_nonmetric): Xk [N, k] (NaN = missing), present [N, k] 0/1 or None,
    z [N] -> (w [k], Y [N])."""
    lib = load()
    Xk = np.ascontiguousarray(Xk, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    if Xk.ndim != 2 or z.shape != (Xk.shape[0],):
        raise ValueError("Xk must be [N, k] and z [N]")
    mask = None
    if present is not None:
        mask = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
        if mask.shape != Xk.shape:
            raise ValueError("present must have the shape of Xk")
    w, Y = np.empty(Xk.shape[1]), np.empty(Xk.shape[0])
    rc = lib.plspm_op_outer_weights_nonmetric(int(device_id), int(mode_code), _ptr(Xk), _ptr(mask), _ptr(z), Xk.shape[0], Xk.shape[1], float(correction), _ptr(w), _ptr(Y))
    if rc:
        raise NativeBackendError("plspm_op_outer_weights_nonmetric failed (%d): %s" % (rc, lib.plspm_last_error(None).decode()))
    return w, Y


def release_cached_memory():
    """Hand the library's cached device / pinned-host blocks back to the HIP runtime."""
    load().plspm_release_cached_memory()


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 of a one-process-per-GPU job hands them to every rank)."""
    lib = load()
    buf = (ctypes.c_uint8 * UNIQUE_ID_BYTES)()
    rc = lib.plspm_rccl_unique_id(buf)
    if rc:
        raise NativeBackendError("plspm_rccl_unique_id failed (%d): %s" % (rc, lib.plspm_group_last_error(None).decode()))
    return bytes(buf)


class NativeComm:
    """The RCCL communicators of this process's ranks (an opaque ``plspm_comm_t*``): every rank of a single-process multi-GPU job
    (``NativeComm(devices)``) or one rank of a one-process-per-GPU job (``NativeComm([device], nranks, rank, unique_id)``).
    Expensive to create (librccl load + ncclCommInit*); create once, bind to groups one after the other."""

    TRANSPORTS = {"auto": 0, "rccl": 1, "copy": 2}

    def __init__(self, devices, nranks=None, first_rank=0, unique_id=None, transport="auto", max_channels=0, _handle=None):
        """``transport``: "auto" (RCCL between distinct devices), "rccl", or "copy" (single-process jobs: device-to-device copies on
        peer-mapped buffers -- the SDMA engines move the records, no kernel of the exchange takes a CU).  ``max_channels`` > 0 caps the
        workgroups RCCL runs for this communicator's collectives (ncclConfig_t.maxCTAs)."""
        if _handle is None and transport not in self.TRANSPORTS:
            raise ValueError("transport must be one of %s (got %r; PLSPM_TRANSPORT sets the default)" % (", ".join(sorted(self.TRANSPORTS)), transport))
        lib = load()
        self._lib = lib
        self.devices = [int(d) for d in devices]
        self.nranks = len(self.devices) if nranks is None else int(nranks)
        self.first_rank = int(first_rank)
        if _handle is not None:
            self._h = _handle
        else:
            dev = np.ascontiguousarray(self.devices, dtype=np.int32)
            uid = None
            if unique_id is not None:
                if len(unique_id) != UNIQUE_ID_BYTES:
                    raise ValueError("unique_id must have %d bytes" % UNIQUE_ID_BYTES)
                uid = (ctypes.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
            t0 = time.perf_counter()
            self._h = lib.plspm_comm_create_ex(_ptr(dev), len(self.devices), self.nranks, self.first_rank, uid, self.TRANSPORTS[transport], int(max_channels))
            self.create_s = time.perf_counter() - t0
            if not self._h:
                raise NativeBackendError("plspm_comm_create: " + lib.plspm_group_last_error(None).decode())
        self.uses_rccl = bool(lib.plspm_comm_uses_rccl(self._h))
        self.transport = {1: "rccl", 2: "copy-engines", 3: "device-copies"}.get(lib.plspm_comm_transport(self._h), "?")
        self.max_channels = int(lib.plspm_comm_max_channels(self._h))
        self._bound = None              # weak reference to the group this communicator currently serves (one at a time)
        _live_comms.add(self)

    def split(self, max_channels):
        """A second communicator over the same ranks with its own channel cap (ncclCommSplit: collective over this one, every rank calls it)."""
        t0 = time.perf_counter()
        h = self._lib.plspm_comm_split(self._h, int(max_channels))
        if not h:
            raise NativeBackendError("plspm_comm_split: " + self._lib.plspm_group_last_error(None).decode())
        twin = NativeComm(self.devices, self.nranks, self.first_rank, _handle=h)
        twin.create_s = time.perf_counter() - t0
        return twin

    def busy(self):
        """True while a live group is bound to this communicator (plspm_group_create refuses a second one)."""
        g = self._bound() if self._bound is not None else None
        return g is not None and bool(getattr(g, "_h", None))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.plspm_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeGroup:
    """Replicate shards over the handles of a communicator + ONE all-gather (an opaque ``plspm_group_t*``).  ``models[i]`` lives on
    ``comm.devices[i]`` and holds the same model and data as every other handle of the job."""

    def __init__(self, comm, models):
        lib = load()
        self._lib = lib
        self.comm, self.models = comm, list(models)
        if len(self.models) != len(comm.devices):
            raise ValueError("one handle per local rank of the communicator")
        arr = (ctypes.c_void_p * len(self.models))(*[m._h for m in self.models])
        self._h = lib.plspm_group_create(comm._h, arr)
        if not self._h:
            raise NativeBackendError("plspm_group_create: " + lib.plspm_group_last_error(None).decode())
        self.nranks = lib.plspm_group_size(self._h)
        self.first_rank = int(comm.first_rank)        # rank of local handle 0 (0: this process holds the rank that summarises)
        self.row_width, self.row_stride = self.models[0].row_width, self.models[0].row_stride
        self.last_B = 0
        comm._bound = weakref.ref(self)
        _live_groups.add(self)

    def _check(self, rc, what):
        if rc:
            raise NativeBackendError("%s failed (%d): %s" % (what, rc, self._lib.plspm_group_last_error(self._h).decode()))

    def close(self):
        # (a communicator that was destroyed first only RELEASED this group -- streams, buffers, its hold on the handles --; the
        # struct is still ours to free, and calls on it in between report PLSPM_E_STATE)
        if getattr(self, "_h", None):
            self._lib.plspm_group_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, B, rank):
        first, count = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.plspm_group_shard(self._h, B, rank, ctypes.byref(first), ctypes.byref(count)), "plspm_group_shard")
        return first.value, count.value

    def set_option(self, key, value):
        """"chunks" 0 automatic | 1 .. 8 sub-batches per call; "chunk_ratio" percent (include/plspm_hip.h, plspm_group_bootstrap)."""
        self._check(self._lib.plspm_group_set_option(self._h, key.encode(), int(value)), "plspm_group_set_option")

    def plan(self, B):
        """The sub-batches a call of B replicates runs as: [(first, count), ...] in replicate-id order."""
        n = ctypes.c_int32(0)
        first, count = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        self._check(self._lib.plspm_group_plan(self._h, B, ctypes.byref(n), _ptr(first), _ptr(count)), "plspm_group_plan")
        return [(int(first[k]), int(count[k])) for k in range(n.value)]

    def bootstrap(self, B, seed=0, rep_offset=0):
        """Enqueue B replicates over the group + the all-gather (no host synchronisation for metric models)."""
        self._check(self._lib.plspm_group_bootstrap(self._h, B, seed, rep_offset), "plspm_group_bootstrap")
        self.last_B = B

    def sync(self):
        self._check(self._lib.plspm_group_sync(self._h), "plspm_group_sync")

    def barrier(self):
        self._check(self._lib.plspm_group_barrier(self._h), "plspm_group_barrier")

    def max(self, value):
        v = ctypes.c_double(float(value))
        self._check(self._lib.plspm_group_max(self._h, ctypes.byref(v)), "plspm_group_max")
        return v.value

    def enqueue_times(self):
        """(shards_ms, exchange_ms): host time of the last bootstrap call's two enqueue phases on this process."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self._lib.plspm_group_enqueue_times(self._h, ctypes.byref(a), ctypes.byref(b)), "plspm_group_enqueue_times")
        return a.value, b.value

    def records(self, local=0):
        """(device pointer, n_records, stride) of the gathered records of the last bootstrap on local handle ``local``."""
        ptr, n, stride = ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int32(0)
        self._check(self._lib.plspm_group_records(self._h, local, ctypes.byref(ptr), ctypes.byref(n), ctypes.byref(stride)), "plspm_group_records")
        return ptr.value, n.value, stride.value

    def summary(self, original):
        original = np.ascontiguousarray(original, dtype=np.float64)
        if original.shape != (self.row_width,):
            raise ValueError("original must have row_width entries")
        out = np.empty((self.row_width, 6))
        used = ctypes.c_int64(0)
        self._check(self._lib.plspm_group_summary(self._h, _ptr(original), _ptr(out), ctypes.byref(used)), "plspm_group_summary")
        return out, used.value

    def adopt(self):
        """Move the last bootstrap's records into ``models[0]`` (device-to-device); the group may be closed afterwards."""
        self._check(self._lib.plspm_group_adopt(self._h), "plspm_group_adopt")

    def rows(self):
        """(rows [B, R], status, iters) of the last bootstrap in replicate-id order, on the host."""
        B = self.last_B
        rows = np.empty((B, self.row_width))
        status = np.empty(B, dtype=np.int32)
        iters = np.empty(B, dtype=np.int32)
        self._check(self._lib.plspm_group_rows(self._h, _ptr(rows), _ptr(status), _ptr(iters)), "plspm_group_rows")
        return rows, status, iters
