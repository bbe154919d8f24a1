"""ctypes binding of libmvs_amd.so (include/mvs_amd.h).

The product path has no CPU fallback: if the HIP library is missing or fails
to load, every entry point raises RuntimeError (the one exception the
reference's main() catches, main.py:43-46).
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmvs_amd.so")

_dp = ctypes.POINTER(ctypes.c_double)
_fp = ctypes.POINTER(ctypes.c_float)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p

# (name, restype, argtypes) -- mirrors include/mvs_amd.h one to one
SIGNATURES = [
    ("mvs_version", ctypes.c_char_p, []),
    ("mvs_last_error", ctypes.c_char_p, [_vp]),
    ("mvs_ctx_create", ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _u8p,
                                      _dp, _dp, _dp, _dp, ctypes.POINTER(_vp)]),
    ("mvs_ctx_destroy", None, [_vp]),
    ("mvs_ctx_rproj", ctypes.c_int, [_vp, _dp]),
    ("mvs_ctx_rebuild", ctypes.c_int, [_vp, _vp]),
    ("mvs_ctx_set_images", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _u8p]),
    ("mvs_score", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _i32p, ctypes.c_int, ctypes.c_double,
                                 _dp, _u64p, _i32p, _dp]),
    ("mvs_score_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, ctypes.c_int,
                                        ctypes.c_double, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_score_device_rec", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, ctypes.c_int, ctypes.c_double,
                                            _vp, _vp, _vp]),
    ("mvs_score_warped", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _i32p, ctypes.c_int, ctypes.c_double,
                                        ctypes.c_double, _dp, _u64p, _i32p, _dp, _dp]),
    ("mvs_score_warped_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int,
                                               ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_refine_warped", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _i32p, _i32p, ctypes.c_int, _dp,
                                         ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_double, ctypes.c_double, _dp, _dp, _i32p, _dp, _dp]),
    ("mvs_refine_warped_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, ctypes.c_int, _vp,
                                                ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_refine_lists_device", ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp,
                                               ctypes.c_double, ctypes.c_int, ctypes.c_double, _vp, _vp, _vp]),
    ("mvs_refine_lists", ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _i64p, _dp, _dp, _i32p,
                                        ctypes.c_double, ctypes.c_int, ctypes.c_double, _i32p, _dp]),
    ("mvs_wexp_children_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, ctypes.c_int, _vp,
                                                ctypes.c_double, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_wexp_claim_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int,
                                             _vp, _vp]),
    ("mvs_wexp_claim", ctypes.c_int, [_vp, ctypes.c_int64, _i32p, _u8p, _dp, ctypes.c_int, ctypes.c_int, _u8p]),
    ("mvs_wexp_mark_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp,
                                            _vp]),
    ("mvs_wfilt_front_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp]),
    ("mvs_wfilt_test_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                             ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_wfilt_front", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _i32p, _u64p, ctypes.c_int, _i32p, _dp]),
    ("mvs_wfilt_test", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _i32p, _u64p, _dp, ctypes.c_int,
                                      ctypes.c_double, ctypes.c_int, _i32p, _u64p, _i64p, _u8p]),
    ("mvs_wfilt_support_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, ctypes.c_int,
                                                ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp, _vp, _vp, _vp,
                                                _vp]),
    ("mvs_wfilt_support", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _i32p, _u64p, ctypes.c_int, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_int, _i32p, _i32p, _i32p, _u8p]),
    ("mvs_wseed_match_device", ctypes.c_int, [_vp, _vp, _i64p, ctypes.c_int64, _i32p, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_wseed_match", ctypes.c_int, [_vp, _i32p, _i64p, ctypes.c_int64, _i32p, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_int64, _dp, _dp, _i32p, _i32p, _dp, _i64p]),
    ("mvs_wpatch_color_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_wpatch_color", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _i32p, _u64p, _dp, _i32p]),
    ("mvs_wdepth_splat_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_double,
                                               ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    ("mvs_wdepth_splat", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _i32p, _u64p, ctypes.c_int, ctypes.c_double,
                                        ctypes.c_int, ctypes.c_int, _dp, _i32p]),
    ("mvs_wdepth_consist_device", ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, _vp,
                                                 _vp]),
    ("mvs_wdepth_consist", ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _u8p, _u8p]),
    ("mvs_wdepth_points_device", ctypes.c_int, [_vp, ctypes.c_int64, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                                _vp]),
    ("mvs_wdepth_points", ctypes.c_int, [_vp, ctypes.c_int64, _i32p, _dp, ctypes.c_int, ctypes.c_int, _dp, _u8p]),
    ("mvs_wprop_sweep_device", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _i32p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_wprop_sweep", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp, _dp, _i32p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, _dp, _dp,
                                       _dp, _i32p, _dp]),
    ("mvs_wtsdf_integrate_device", ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                  _vp, _vp, _vp, _vp, _vp]),
    ("mvs_wtsdf_integrate", ctypes.c_int, [_vp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, _dp,
                                           _i32p, _u8p, _u8p]),
    ("mvs_wmesh_extract_device", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double,
                                                _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp,
                                                _vp]),
    ("mvs_wmesh_extract", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double, _dp,
                                         _u8p, _u8p, ctypes.c_int64, ctypes.c_int64, _dp, _u8p, _i32p, _i64p]),
    ("mvs_pack_accepted", ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int,
                                         ctypes.c_int64, _vp, _vp]),
    ("mvs_set_scorer_grid", ctypes.c_int, [_vp, ctypes.c_int]),
    ("mvs_proxy_copy", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp]),
    ("mvs_filter_outliers", ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p,
                                           _u64p, _i32p, _dp, _dp, _dp, _u8p, _i64p]),
    ("mvs_exact_hits", ctypes.c_int64, [_vp]),
    ("mvs_scorer_stats", ctypes.c_int, [_vp, _i64p]),
    ("mvs_bin_runs_batches", ctypes.c_int64, [_vp]),
    ("mvs_stream_retiring", ctypes.c_int, [_vp, _vp]),
    ("mvs_kernel_timing", ctypes.c_int, [_vp, ctypes.c_int]),
    ("mvs_kernel_time", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_int64)]),
    ("mvs_timed_kernel", ctypes.c_char_p, [_vp]),
    ("mvs_ncc_windows", ctypes.c_int, [ctypes.c_int64, ctypes.c_int, _vp, _vp, ctypes.c_double,
                                       ctypes.c_int, _vp, _vp, _vp]),
    ("mvs_stage_run", ctypes.c_int, [_vp, ctypes.c_int64, _i64p, _i32p, _fp, ctypes.c_int,
                                     ctypes.c_double, ctypes.c_int, ctypes.c_int64,
                                     ctypes.POINTER(_vp)]),
    ("mvs_stage_begin", ctypes.c_int, [_vp, ctypes.c_int64, _i64p, _i32p, _fp, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(_vp)]),
    ("mvs_stage_plan", ctypes.c_int64, [_vp]),
    ("mvs_stage_record_width", ctypes.c_int, [_vp]),
    ("mvs_stage_score_slice", ctypes.c_int, [_vp, _vp]),
    ("mvs_stage_ingest", ctypes.c_int, [_vp, _vp]),
    ("mvs_stage_finish", ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    ("mvs_stage_destroy", None, [_vp]),
    ("mvs_stage_count", ctypes.c_int64, [_vp, ctypes.c_int]),
    ("mvs_stage_rows", ctypes.c_int, [_vp, ctypes.c_int, _dp]),
    ("mvs_stage_rows_device", ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    ("mvs_stage_stats", ctypes.c_int, [_vp, _i64p]),
    ("mvs_stage_times", ctypes.c_int, [_vp, _dp]),
    ("mvs_stage_set_options", ctypes.c_int, [_vp, ctypes.c_int]),
    ("mvs_exact_avg", ctypes.c_int, [_vp, ctypes.c_int64, _i32p, _dp, _u64p, ctypes.c_int, _dp]),
    ("mvs_stage_filter_stats", ctypes.c_int, [_vp, _i64p]),
    ("mvs_stage_free", None, [_vp]),
    ("mvs_expand_candidates", ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, _dp, ctypes.c_int64,
                                             _i32p, _i32p, _i32p, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_int, ctypes.c_double, _dp, _dp, _u8p, _dp,
                                             _u64p, _i32p, _u8p]),
    ("mvs_rodrigues_roundtrip", ctypes.c_int, [_dp, _dp]),
    ("mvs_triangulate", ctypes.c_int, [_dp, _dp, _dp, _dp, _dp]),
    ("mvs_harris_points", ctypes.c_int, [_vp, ctypes.c_int, _i32p, ctypes.c_int64, _i64p]),
    ("mvs_match_two_sided", ctypes.c_int, [_vp, ctypes.c_int, _i32p, ctypes.c_int64, ctypes.c_int,
                                           _i32p, ctypes.c_int64, ctypes.c_int, ctypes.c_double,
                                           _i32p, _i32p, _i32p]),
    ("mvs_sfm_pair", ctypes.c_int, [_dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int64, _fp, _fp,
                                    ctypes.c_double, _fp, _u8p]),
]

_lib = None


def load(path=None):
    """Load libmvs_amd.so; raises RuntimeError if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("MVS_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise RuntimeError(
            f"libmvs_amd.so not found at {path}: build it with __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # torch first: its bundled HIP runtime (SONAME libamdhip64.so.7) is then
    # the one libmvs_amd.so's NEEDED entry binds to, so torch tensors, torch
    # streams and the library share one runtime.  Loaded the other way round
    # the process would hold two HIP runtimes and torch.cuda would not start.
    import torch  # noqa: F401
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError(f"cannot load {path}: {e}") from e
    for name, res, args in SIGNATURES:
        if path != LIB_PATH and not hasattr(lib, name):
            continue   # an older A/B build (MVS_LIB) without a newer entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def last_error(ctx=None):
    msg = load().mvs_last_error(ctx)
    return msg.decode() if msg else ""


MVS_E_DIVZERO = -5
MVS_STAGE_FILTER_OUTLIERS = 1


def check(rc, ctx=None, what="mvs"):
    if rc == MVS_E_DIVZERO:
        # where the reference itself raises (filter_out_outlier, MVS2.py:144)
        raise ZeroDivisionError(f"{what}: {last_error(ctx)}")
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error(ctx)}")
