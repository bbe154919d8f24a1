"""ctypes binding of libmvs_amd.so (include/mvs_amd.h).

The product path has no CPU fallback: if the HIP library is missing or fails
to load, every entry point raises RuntimeError (the one exception the
reference's main() catches, main.py:43-46).
"""
import atexit
import ctypes
import math
import os
import weakref

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


def rodrigues_roundtrip(R):
    """R' = Rodrigues(Rodrigues(R)) -- the rotation cv2.projectPoints applies (utils.py:242-243)."""
    R = _c(R, np.float64).reshape(9)
    out = np.empty(9)
    check(load().mvs_rodrigues_roundtrip(_p(R, _dp), _p(out, _dp)), what="rodrigues")
    return out.reshape(3, 3)


def sfm_pair(KA, RA, tA, KB, RB, tB, q, tr, max_err):
    """One pair of StructureFromMotion's loop (SFM.py:60-80), host C++:
    (float32 points (n, 3), keep (n,) bool)."""
    mats = [_c(m, np.float64).reshape(-1) for m in (KA, RA, tA, KB, RB, tB)]
    q = _c(q, np.float32).reshape(-1, 2)
    tr = _c(tr, np.float32).reshape(-1, 2)
    n = len(q)
    if len(tr) != n:
        raise RuntimeError("query and train correspondences differ in length")
    pt = np.empty((max(n, 1), 3), np.float32)
    keep = np.empty(max(n, 1), np.uint8)
    check(load().mvs_sfm_pair(*[_p(m, _dp) for m in mats], n, _p(q, _fp), _p(tr, _fp),
                              float(max_err), _p(pt, _fp), _p(keep, _u8p)), None, "mvs_sfm_pair")
    return pt[:n], keep[:n].astype(bool)


def filter_outliers(cell, mask, count, avg, c, nrm, nci, ncj):
    """CellTable.filter_out_outlier (MVS2.py:132-158) on the host over accepted
    patches in fill order (mvs_filter_outliers): -> (alive bool (n,), removed,
    "remove a outlier" lines).  Raises ZeroDivisionError where the reference does."""
    cell = _c(cell, np.int32).reshape(-1, 2)
    n = len(cell)
    mask = _c(mask, np.uint64).reshape(n, -1)
    count = _c(count, np.int32).reshape(n)
    avg = _c(avg, np.float64).reshape(n)
    c = _c(c, np.float64).reshape(n, 3)
    nrm = _c(nrm, np.float64).reshape(n, 3)
    alive = np.empty(max(n, 1), np.uint8)
    stats = np.zeros(2, np.int64)
    check(load().mvs_filter_outliers(n, mask.shape[1], int(nci), int(ncj), _p(cell, _i32p), _p(mask, _u64p),
                                     _p(count, _i32p), _p(avg, _dp), _p(c, _dp), _p(nrm, _dp),
                                     _p(alive, _u8p), _p(stats, _i64p)), None, "mvs_filter_outliers")
    return alive[:n].astype(bool), int(stats[0]), int(stats[1])


def triangulate(P1, P2, x1, x2):
    """cv2.triangulatePoints for one correspondence (utils.py:238-239), homogeneous 4-vector."""
    P1 = _c(P1, np.float64).reshape(12)
    P2 = _c(P2, np.float64).reshape(12)
    x1 = _c(x1, np.float64).reshape(2)
    x2 = _c(x2, np.float64).reshape(2)
    out = np.empty(4)
    check(load().mvs_triangulate(_p(P1, _dp), _p(P2, _dp), _p(x1, _dp), _p(x2, _dp), _p(out, _dp)),
          what="triangulate")
    return out


def seed_view_pairs(Rp, neighbours=4, min_axis_cos=0.5):
    """The ordered view pairs (r, v) the seed matcher is fed, from the
    rotations Rp (V,3,3) alone: per r the views v != r ranked by the descending
    dot product of the optical axes (the third rows of Rp; Python floats, left
    to right), ties to the lower v; those with a dot >= min_axis_cos; the first
    `neighbours` of them.  (np, 2) int32, r-major."""
    ax = [[float(x) for x in row] for row in np.asarray(Rp, np.float64).reshape(-1, 3, 3)[:, 2, :]]
    V = len(ax)
    out = []
    for r in range(V):
        dots = [(ax[r][0] * ax[v][0] + ax[r][1] * ax[v][1] + ax[r][2] * ax[v][2], v) for v in range(V) if v != r]
        keep = sorted((d, v) for d, v in dots if d >= float(min_axis_cos))
        keep.sort(key=lambda dv: (-dv[0], dv[1]))
        out += [(r, v) for _, v in keep[:max(int(neighbours), 0)]]
    return np.array(out, np.int32).reshape(-1, 2)


def wprop_view_lists(Rp, tv=4, min_axis_cos=0.5, v0=0, nv=None):
    """The view lists of the propagation sweep for the views v0 .. v0 + nv - 1
    -> (nv, tv) int32: the rows of seed_view_pairs(Rp, tv, min_axis_cos) grouped
    by their first view, in that order, padded with -1."""
    Rp = np.asarray(Rp, np.float64).reshape(-1, 3, 3)
    nv = len(Rp) - v0 if nv is None else int(nv)
    out = np.full((nv, int(tv)), -1, np.int32)
    fill = [0] * nv
    for r, v in seed_view_pairs(Rp, int(tv), min_axis_cos).tolist():
        if v0 <= r < v0 + nv:
            out[r - v0, fill[r - v0]] = v
            fill[r - v0] += 1
    return out


# live contexts: a retiring caller stream is announced to each of them
# (stream_retiring), and the ones still open at interpreter exit are closed by
# an atexit hook, before the HIP runtime's own teardown
_LIVE = weakref.WeakSet()


def stream_retiring(stream):
    """A caller stream (a hipStream_t handle) is about to be destroyed: every
    live context waits for its work there now (mvs_stream_retiring)."""
    for cx in list(_LIVE):
        h = getattr(cx, "_h", None)
        if h:
            check(load().mvs_stream_retiring(h, stream), h, "mvs_stream_retiring")


@atexit.register
def _close_live_contexts():
    for cx in list(_LIVE):
        try:
            cx.close()
        except Exception:
            pass


def mesh_grid(points, bounds, resolution, trunc_voxels):
    """The lattice of MvsContext.mesh_depth -> origin (3,) float64, voxel, dims
    (nx, ny, nz), trunc.  bounds = (lo, hi) is taken as given: voxel = its longest
    side / resolution.  bounds None: the per-axis 0.5 to 99.5 percentile box of
    `points` gives the voxel the same way and is then grown by 2 trunc on every
    side.  dims = ceil(side / voxel), at least 1, per axis."""
    if bounds is None:
        pts = np.zeros((0, 3)) if points is None else np.asarray(points, np.float64).reshape(-1, 3)
        if len(pts) == 0:
            raise RuntimeError("mesh_depth: no points to take the bounds from")
        lo, hi = np.percentile(pts, 0.5, axis=0), np.percentile(pts, 99.5, axis=0)
    else:
        lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
    if int(resolution) < 1:
        raise RuntimeError("mesh_depth: resolution must be >= 1")
    voxel = float((hi - lo).max()) / float(resolution)
    if not (voxel > 0 and math.isfinite(voxel) and float(trunc_voxels) > 0):
        raise RuntimeError("mesh_depth: the bounds must be finite with a positive longest side, trunc_voxels > 0")
    trunc = float(trunc_voxels) * voxel
    if bounds is None:
        lo, hi = lo - 2.0 * trunc, hi + 2.0 * trunc
    dims = tuple(max(1, int(math.ceil(float(s) / voxel))) for s in hi - lo)
    return np.ascontiguousarray(lo, np.float64), voxel, dims, trunc


class MvsContext:
    """One device-resident scene (images + cameras) on one GPU.

    imgs: (V,H,W,3) uint8 RGB (main.py:17-18 convention) or a list of such
    frames; K, R: (V,3,3); t: (V,3) or (V,3,1).
    """

    def __init__(self, imgs, K, R, t, device=0, Rp=None):
        lib = load()
        rgb = _c(np.stack(imgs) if isinstance(imgs, (list, tuple)) else imgs, np.uint8)
        if rgb.ndim != 4 or rgb.shape[-1] != 3:
            raise RuntimeError(f"images must be (V,H,W,3) uint8 RGB, got {rgb.shape}")
        self.V, self.H, self.W = (int(x) for x in rgb.shape[:3])
        self.words = (self.V + 63) // 64
        K = _c(K, np.float64).reshape(self.V, 9)
        R = _c(R, np.float64).reshape(self.V, 9)
        t = _c(t, np.float64).reshape(self.V, 3)
        rp = _c(Rp, np.float64).reshape(self.V, 9) if Rp is not None else None
        h = _vp()
        rc = lib.mvs_ctx_create(int(device), self.V, self.H, self.W, _p(rgb, _u8p), _p(K, _dp),
                                _p(R, _dp), _p(t, _dp), _p(rp, _dp) if rp is not None else None,
                                ctypes.byref(h))
        check(rc, None, "mvs_ctx_create")
        self._h = h
        self.device = device
        self._K = K.reshape(self.V, 3, 3).copy()   # refine_depth_steps
        self._t = t.copy()
        self._refine_stream = None   # refine_warped's torch side stream
        self._stages = weakref.WeakSet()
        _LIVE.add(self)

    def close(self):
        if getattr(self, "_h", None):
            # stepped stages hold the context: they go first
            for st in list(getattr(self, "_stages", ())):
                st.close()
            load().mvs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def rproj(self):
        out = np.empty((self.V, 9))
        check(load().mvs_ctx_rproj(self._h, _p(out, _dp)), self._h, "mvs_ctx_rproj")
        return out.reshape(self.V, 3, 3)

    def exact_hits(self):
        return int(load().mvs_exact_hits(self._h))

    def scorer_stats(self):
        """{'direct': candidates the direct path re-scored (guard band +
        bucket overflow), 'overflow': of them bucket overflow, 'batches':
        tiled batches} since the context was created (mvs_scorer_stats)."""
        out = np.zeros(3, np.int64)
        check(load().mvs_scorer_stats(self._h, _p(out, _i64p)), self._h, "mvs_scorer_stats")
        return {"direct": int(out[0]), "overflow": int(out[1]), "batches": int(out[2])}

    def bin_runs_batches(self):
        """Tiled batches since the context was created that were binned into
        workgroup-private sorted runs (mvs_bin_runs_batches); the others used
        the atomic tile buckets."""
        return int(load().mvs_bin_runs_batches(self._h))

    def rebuild(self, stream=None):
        """Rebuild the device gray stack / view-major copy from the resident
        RGB images (stream-ordered; for cold-sweep timing)."""
        check(load().mvs_ctx_rebuild(self._h, stream), self._h, "mvs_ctx_rebuild")

    def set_images(self, first_view, imgs):
        """Replace the resident RGB images of views first_view, first_view + 1,
        ... by imgs (k, H, W, 3) uint8 (mvs_ctx_set_images, synchronous).  The
        gray stack and the moment tables follow at the next rebuild()."""
        rgb = _c(imgs, np.uint8)
        if rgb.ndim != 4 or rgb.shape[1:] != (self.H, self.W, 3):
            raise RuntimeError(f"images must be (k,{self.H},{self.W},3) uint8 RGB, got {rgb.shape}")
        check(load().mvs_ctx_set_images(self._h, int(first_view), len(rgb), _p(rgb, _u8p)), self._h,
              "mvs_ctx_set_images")

    def kernel_timing(self, enable=True, every=1):
        """Start (reset) or stop HIP-event timing of the dominant scoring kernel;
        every = k times every k-th scoring call."""
        check(load().mvs_kernel_timing(self._h, int(every) if enable else 0), self._h, "mvs_kernel_timing")

    def kernel_time(self):
        """-> (total kernel milliseconds, timed launches) since kernel_timing(True)."""
        ms = ctypes.c_double(0.0)
        k = ctypes.c_int64(0)
        check(load().mvs_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(k)), self._h,
              "mvs_kernel_time")
        return ms.value, int(k.value)

    def timed_kernel(self):
        """Name of the kernel the last timed event pair bracketed."""
        name = load().mvs_timed_kernel(self._h)
        return name.decode() if name else ""

    def score(self, c, ref, min_ncc=0.7, wid=5):
        """Batched photo_consistenecy_test (MVS2.py:62-77) on host arrays.

        Returns xy (n,2), mask (n,words) uint64, count (n,), avg (n,)."""
        c = _c(c, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        if len(c) != n:
            raise RuntimeError("c and ref lengths differ")
        xy = np.empty((n, 2))
        mask = np.empty((n, self.words), np.uint64)
        count = np.empty(n, np.int32)
        avg = np.empty(n)
        rc = load().mvs_score(self._h, n, _p(c, _dp), _p(ref, _i32p), int(wid), float(min_ncc),
                              _p(xy, _dp), _p(mask, _u64p), _p(count, _i32p), _p(avg, _dp))
        check(rc, self._h, "mvs_score")
        return xy, mask, count, avg

    def exact_avg(self, ref, xy, mask, wid=5):
        """avg_ncc_score in the reference's arithmetic (numpy-order ctNcc, summed in
        view order) for candidates scored by `score`: bit-exact, where score's avg
        is within 1e-12."""
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        xy = _c(xy, np.float64).reshape(n, 2)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        out = np.empty(n)
        check(load().mvs_exact_avg(self._h, n, _p(ref, _i32p), _p(xy, _dp), _p(mask, _u64p), int(wid),
                                   _p(out, _dp)), self._h, "mvs_exact_avg")
        return out

    def score_device(self, c, ref, xy, mask, count, avg, min_ncc=0.7, wid=5, stream=None):
        """Same on device tensors (torch: pass .data_ptr() ints); stream-ordered."""
        n = int(ref.numel()) if hasattr(ref, "numel") else int(len(ref))
        ptr = (lambda x: x.data_ptr()) if hasattr(ref, "data_ptr") else (lambda x: int(x))
        rc = load().mvs_score_device(self._h, n, ptr(c), ptr(ref), int(wid), float(min_ncc),
                                     ptr(xy), ptr(mask), ptr(count),
                                     ptr(avg) if avg is not None else None,
                                     stream if stream is not None else None)
        check(rc, self._h, "mvs_score_device")

    def score_device_rec(self, c, ref, xy, rec, min_ncc=0.7, wid=5, stream=None):
        """The photo test into records (device int64 tensor (n, words + 1): mask
        words, avg bits; |V| = popcount), stream-ordered."""
        n = int(ref.numel())
        if rec.dtype.itemsize != 8 or tuple(rec.shape) != (n, self.words + 1) or not rec.is_contiguous():
            raise RuntimeError(f"score_device_rec: rec must be contiguous int64 ({n}, {self.words + 1})")
        rc = load().mvs_score_device_rec(self._h, n, c.data_ptr(), ref.data_ptr(), int(wid), float(min_ncc),
                                         xy.data_ptr(), rec.data_ptr(), stream if stream is not None else None)
        check(rc, self._h, "mvs_score_device_rec")

    def score_warped(self, c, nrm, ref, min_ncc=0.7, wid=5, min_cos=0.0, want_ncc=False):
        """Plane-warped, per-view reprojected photo test (mvs_score_warped) on
        host arrays: the reference window of patch (c, nrm) in view ref is
        carried through the patch plane into every other view whose camera the
        normal faces (cosine > min_cos), sampled bilinearly and compared with
        ctNcc's scaling.  nrm: unit normals pointing towards the cameras (not
        checked).  Call it where the patch normal is known and the views differ
        enough that windows at one pixel no longer show the same surface;
        `score` is the reference's test.

        Returns xy (n,2), mask (n,words) uint64, count (n,), avg (n,) and, with
        want_ncc, ncc (n,V) float64 (nan for ref, culled and failed views)."""
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        if len(c) != n or len(nrm) != n:
            raise RuntimeError("c, nrm and ref lengths differ")
        xy = np.empty((n, 2))
        mask = np.empty((n, self.words), np.uint64)
        count = np.empty(n, np.int32)
        avg = np.empty(n)
        ncc = np.empty((n, self.V)) if want_ncc else None
        rc = load().mvs_score_warped(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), int(wid),
                                     float(min_ncc), float(min_cos), _p(xy, _dp), _p(mask, _u64p),
                                     _p(count, _i32p), _p(avg, _dp), _p(ncc, _dp) if want_ncc else None)
        check(rc, self._h, "mvs_score_warped")
        return (xy, mask, count, avg, ncc) if want_ncc else (xy, mask, count, avg)

    def score_warped_device(self, c, nrm, ref, xy, mask, count, avg=None, ncc=None, min_ncc=0.7, wid=5,
                            min_cos=0.0, stream=None):
        """score_warped on torch device tensors (contiguous: c, nrm float64
        (n,3), ref int32 (n,), xy float64 (n,2), mask int64 (n,words), count
        int32 (n,), avg float64 (n,) or None, ncc float64 (n,V) or None);
        stream-ordered (stream = a hipStream_t handle, None = the context's)."""
        n = int(ref.numel())
        want = [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)), ("xy", xy, 8, (n, 2)),
                ("mask", mask, 8, (n, self.words)), ("count", count, 4, (n,))]
        if avg is not None:
            want.append(("avg", avg, 8, (n,)))
        if ncc is not None:
            want.append(("ncc", ncc, 8, (n, self.V)))
        for name, x, size, shape in want:
            # the kernel indexes rows at a fixed pitch
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"score_warped_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_score_warped_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), int(wid),
                                            float(min_ncc), float(min_cos), xy.data_ptr(), mask.data_ptr(),
                                            count.data_ptr(), avg.data_ptr() if avg is not None else None,
                                            ncc.data_ptr() if ncc is not None else None,
                                            stream if stream is not None else None)
        check(rc, self._h, "mvs_score_warped_device")

    @staticmethod
    def refine_hypotheses(kd, ka):
        """H = (2 kd + 1)(2 ka + 1)^2, the grid size of one refinement level."""
        return (2 * int(kd) + 1) * (2 * int(ka) + 1) ** 2

    def refine_warped_level(self, c, nrm, ref, views, dstep, wid=5, min_cos=0.0, kd=2, ka=1,
                            astep=math.radians(8), step_scale=1.0, want_scores=False):
        """One level of the fixed-grid depth and normal refinement
        (mvs_refine_warped) on host arrays: the H = (2 kd + 1)(2 ka + 1)^2
        plane hypotheses around patch (c, nrm) -- depths k dstep step_scale
        along the reference ray, normals tilted by tan(i astep step_scale) along
        two tangents -- are scored by the mean warped ncc over the patch's view
        list views[i] (int32 (n, tv), -1 padded at the end), and the best is
        chosen; the input patch is kept unless another scores strictly higher.

        Returns c_out (n,3), nrm_out (n,3), best (n,) int32 (-1: nothing valid),
        score_best (n,) and, with want_scores, scores (n, H)."""
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        views = _c(views, np.int32)
        if views.ndim != 2 or len(views) != n:
            raise RuntimeError("views must be (n, tv) int32")
        tv = views.shape[1]
        dstep = _c(dstep, np.float64).reshape(-1)
        if len(c) != n or len(nrm) != n or len(dstep) != n:
            raise RuntimeError("c, nrm, ref, views and dstep lengths differ")
        c_out = np.empty((n, 3))
        nrm_out = np.empty((n, 3))
        best = np.empty(n, np.int32)
        score_best = np.empty(n)
        scores = np.empty((n, self.refine_hypotheses(kd, ka))) if want_scores and 0 <= kd <= 3 and 0 <= ka <= 2 \
            else None
        rc = load().mvs_refine_warped(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(views, _i32p),
                                      int(tv), _p(dstep, _dp), int(wid), float(min_cos), int(kd), int(ka),
                                      float(astep), float(step_scale), _p(c_out, _dp), _p(nrm_out, _dp),
                                      _p(best, _i32p), _p(score_best, _dp),
                                      _p(scores, _dp) if scores is not None else None)
        check(rc, self._h, "mvs_refine_warped")
        return (c_out, nrm_out, best, score_best, scores) if want_scores else (c_out, nrm_out, best, score_best)

    def refine_warped_level_device(self, c, nrm, ref, views, dstep, c_out, nrm_out, best, score_best, scores=None,
                                   wid=5, min_cos=0.0, kd=2, ka=1, astep=math.radians(8), step_scale=1.0,
                                   stream=None):
        """refine_warped_level on torch device tensors (contiguous: c, nrm,
        c_out, nrm_out float64 (n,3), ref, best int32 (n,), views int32 (n,tv),
        dstep, score_best float64 (n,), scores float64 (n,H) or None);
        stream-ordered (stream = a hipStream_t handle, None = the context's).
        c_out / nrm_out must be other tensors than c / nrm."""
        n = int(ref.numel())
        tv = int(views.shape[1]) if views.dim() == 2 else 0
        want = [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)), ("views", views, 4, (n, tv)),
                ("dstep", dstep, 8, (n,)), ("c_out", c_out, 8, (n, 3)), ("nrm_out", nrm_out, 8, (n, 3)),
                ("best", best, 4, (n,)), ("score_best", score_best, 8, (n,))]
        if scores is not None:
            want.append(("scores", scores, 8, (n, self.refine_hypotheses(kd, ka))))
        for name, x, size, shape in want:
            # the kernel indexes rows at a fixed pitch
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(
                    f"refine_warped_level_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_refine_warped_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(),
                                             views.data_ptr(), tv, dstep.data_ptr(), int(wid), float(min_cos),
                                             int(kd), int(ka), float(astep), float(step_scale), c_out.data_ptr(),
                                             nrm_out.data_ptr(), best.data_ptr(), score_best.data_ptr(),
                                             scores.data_ptr() if scores is not None else None,
                                             stream if stream is not None else None)
        check(rc, self._h, "mvs_refine_warped_device")

    @staticmethod
    def refine_view_lists(ncc, min_ncc=0.7, max_views=8):
        """The view lists refine_warped builds from score_warped's ncc (n, V):
        per patch the max_views passing views (ncc > min_ncc) with the highest
        ncc, ties to the lower view index, in ascending view order, padded with
        -1 -> int32 (n, max_views)."""
        ncc = np.asarray(ncc, np.float64)
        n, V = ncc.shape
        with np.errstate(invalid="ignore"):
            key = np.where(ncc > min_ncc, ncc, -np.inf)      # nan and failing views last
        order = np.argsort(-key, axis=1, kind="stable")[:, :max_views]   # stable: ties keep the lower view first
        keep = np.take_along_axis(key, order, 1) > -np.inf
        lists = np.where(keep, order, V)                     # V sorts after every view
        lists.sort(axis=1)
        lists[lists == V] = -1
        out = np.full((n, max_views), -1, np.int32)
        out[:, :lists.shape[1]] = lists
        return out

    def refine_depth_steps(self, c, ref, depth_px=1.5):
        """dstep = depth_px * (depth of c in its reference view) / ((fx + fy) / 2):
        the world size of depth_px pixels at the patch."""
        c = _c(c, np.float64).reshape(-1, 3)
        ref = np.asarray(ref).reshape(-1)
        Rp, t, K = self.rproj(), self._t, self._K
        depth = Rp[ref, 2, 0] * c[:, 0] + Rp[ref, 2, 1] * c[:, 1] + Rp[ref, 2, 2] * c[:, 2] + t[ref, 2]
        return depth_px * depth / ((K[ref, 0, 0] + K[ref, 1, 1]) / 2)

    def refine_lists_device(self, ncc, c, ref, views, dstep, sel=None, min_ncc=0.7, max_views=8, depth_px=1.5,
                            stream=None):
        """refine_view_lists and refine_depth_steps on the device
        (mvs_refine_lists_device), bit for bit, on torch device tensors
        (contiguous): ncc float64 (rows,V) as score_warped_device writes it, c
        float64 (rows,3), ref int32 (rows,), views int32 (n,max_views) and dstep
        float64 (n,) the outputs, sel int64 (n,) or None -- output row k is made
        from source row sel[k] (None: row k, n <= rows).  dstep None: lists
        only, c and ref may then be None.  A sel entry outside 0..rows-1 gives
        an all -1 list and dstep nan; a ref outside 0..V-1 gives dstep nan.
        Stream-ordered (stream = a hipStream_t handle, None = the context's);
        the call keeps no state and may run on several streams at once."""
        rows = int(ncc.shape[0]) if ncc.dim() == 2 else 0
        n = int(views.shape[0]) if views.dim() == 2 else 0
        want = [("ncc", ncc, 8, (rows, self.V)), ("views", views, 4, (n, int(max_views)))]
        if dstep is not None:
            if c is None or ref is None:
                raise RuntimeError("refine_lists_device: dstep needs c and ref")
            want += [("c", c, 8, (rows, 3)), ("ref", ref, 4, (rows,)), ("dstep", dstep, 8, (n,))]
        if sel is not None:
            want.append(("sel", sel, 8, (n,)))
        for name, x, size, shape in want:
            # the kernel indexes rows at a fixed pitch
            if x.dtype.itemsize != size or x.dtype.is_floating_point != (name in ("ncc", "c", "dstep")) or \
                    tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"refine_lists_device: {name} must be contiguous, {size}-byte elements, {shape}")
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = load().mvs_refine_lists_device(self._h, n, rows, ptr(sel), ncc.data_ptr(),
                                            ptr(c) if dstep is not None else None,
                                            ptr(ref) if dstep is not None else None, float(min_ncc), int(max_views),
                                            float(depth_px), views.data_ptr(), ptr(dstep),
                                            stream if stream is not None else None)
        check(rc, self._h, "mvs_refine_lists_device")

    def refine_lists(self, ncc, c=None, ref=None, sel=None, min_ncc=0.7, max_views=8, depth_px=1.5):
        """refine_lists_device on host arrays (mvs_refine_lists, synchronous):
        ncc (rows,V), c (rows,3) and ref (rows,) or both None (lists only), sel
        (n,) int64 or None.  A sel entry outside 0..rows-1 or a ref outside
        0..V-1 raises.  Returns views (n,max_views) int32 and dstep (n,) float64
        (None without c and ref)."""
        ncc = _c(ncc, np.float64)
        if ncc.ndim != 2 or ncc.shape[1] != self.V:
            raise RuntimeError(f"refine_lists: ncc must be (rows, {self.V})")
        rows = len(ncc)
        if (c is None) != (ref is None):
            raise RuntimeError("refine_lists: c and ref go together")
        if c is not None:
            c = _c(c, np.float64).reshape(-1, 3)
            ref = _c(ref, np.int32).reshape(-1)
            if len(c) != rows or len(ref) != rows:
                raise RuntimeError("refine_lists: ncc, c and ref lengths differ")
        if sel is not None:
            sel = _c(sel, np.int64).reshape(-1)
        n = len(sel) if sel is not None else rows
        mv = int(max_views)
        views = np.empty((n, mv if 1 <= mv <= 32 else 1), np.int32)
        dstep = np.empty(n) if c is not None else None
        rc = load().mvs_refine_lists(self._h, n, rows, _p(sel, _i64p) if sel is not None else None, _p(ncc, _dp),
                                     _p(c, _dp) if c is not None else None,
                                     _p(ref, _i32p) if c is not None else None, float(min_ncc), mv, float(depth_px),
                                     _p(views, _i32p), _p(dstep, _dp) if dstep is not None else None)
        check(rc, self._h, "mvs_refine_lists")
        return views, dstep

    def refine_warped(self, c, nrm, ref, wid=5, min_ncc=0.7, min_cos=0.0, max_views=8, levels=4, kd=2, ka=1,
                      depth_px=1.5, astep=math.radians(8)):
        """Coarse-to-fine depth and normal refinement of patches against the
        plane-warped photo test, one upload, one chain on the context's side
        stream, one download:
          1. score_warped_device with per-view ncc;
          2. refine_lists_device: per patch the view list of refine_view_lists
             (the max_views best passing views) and
          3. dstep = the world size of depth_px pixels at the patch
             (refine_depth_steps);
          4. `levels` level calls (refine_warped_level_device) with step_scale
             = 2^-level, c / nrm ping-ponging between two device buffers, no
             host synchronisation in between;
          5. score_warped_device of the refined patches.
        A patch with no passing view, or invalid in its reference view, comes
        back unchanged (best -1 at every level).

        Returns c' (n,3), nrm' (n,3), (xy, mask, count, avg) of the final test
        and an info dict: views (n, max_views), best (levels, n), score_first
        (n,) the first level's centre score, score_last (n,) the last level's
        best score."""
        import torch
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        levels = int(levels)
        if levels < 1:
            raise RuntimeError("refine_warped: levels must be >= 1")
        if not 1 <= int(max_views) <= 32:
            raise RuntimeError("refine_warped: max_views must be in 1..32")
        if len(c) != n or len(nrm) != n:
            raise RuntimeError("c, nrm and ref lengths differ")
        if n and (ref.min() < 0 or ref.max() >= self.V):
            raise RuntimeError("refine_warped: ref view out of range")
        H = self.refine_hypotheses(kd, ka)
        dev = torch.device(f"cuda:{self.device}")
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        # the context's torch side stream carries the whole chain
        st = self._side_stream()
        with torch.cuda.stream(st):
            cur = [torch.from_numpy(c).to(dev), torch.from_numpy(nrm).to(dev)]
            nxt = [torch.empty((n, 3), **f64), torch.empty((n, 3), **f64)]
            t_ref = torch.from_numpy(ref).to(dev)
            xy = torch.empty((n, 2), **f64)
            mask = torch.empty((n, self.words), dtype=torch.int64, device=dev)
            count = torch.empty(n, **i32)
            avg = torch.empty(n, **f64)
            ncc = torch.empty((n, self.V), **f64)
            self.score_warped_device(cur[0], cur[1], t_ref, xy, mask, count, None, ncc, min_ncc, wid, min_cos,
                                     stream=st.cuda_stream)
            t_views = torch.empty((n, int(max_views)), **i32)
            t_dstep = torch.empty(n, **f64)
            self.refine_lists_device(ncc, cur[0], t_ref, t_views, t_dstep, None, min_ncc, int(max_views), depth_px,
                                     stream=st.cuda_stream)
            best = torch.empty((levels, n), **i32)
            sbest = torch.empty(n, **f64)
            first = torch.empty((n, H), **f64)
            for lev in range(levels):
                self.refine_warped_level_device(cur[0], cur[1], t_ref, t_views, t_dstep, nxt[0], nxt[1], best[lev],
                                                sbest, first if lev == 0 else None, wid, min_cos, kd, ka, astep,
                                                2.0 ** -lev, stream=st.cuda_stream)
                cur, nxt = nxt, cur
            self.score_warped_device(cur[0], cur[1], t_ref, xy, mask, count, avg, None, min_ncc, wid, min_cos,
                                     stream=st.cuda_stream)
            info = {"views": t_views.cpu().numpy(), "best": best.cpu().numpy(),
                    "score_first": first[:, (H - 1) // 2].cpu().numpy(), "score_last": sbest.cpu().numpy()}
            out = (cur[0].cpu().numpy(), cur[1].cpu().numpy(),
                   (xy.cpu().numpy(), mask.cpu().numpy().view(np.uint64), count.cpu().numpy(), avg.cpu().numpy()),
                   info)
        st.synchronize()
        return out

    # ---- level-synchronous expansion driven by the warped test ----

    def cell_grid(self, cell_size):
        """(nci, ncj) of the expansion's cell grid: whole cells only."""
        s = int(cell_size)
        if not 1 <= s <= 16:
            raise RuntimeError("cell_size must be in 1..16")
        return self.W // s, self.H // s

    def _dev_tensor(self, x, dtype, shape):
        """numpy array or torch tensor -> contiguous tensor of dtype on the context's device."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if not isinstance(x, torch.Tensor):
            a = np.ascontiguousarray(x)
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            x = torch.from_numpy(a)
        return x.to(device=dev, dtype=dtype).reshape(shape).contiguous()

    @staticmethod
    def _stream_handle(stream):
        return stream if stream is not None else None

    def wexp_children_device(self, c, nrm, ref, mask, cell_size, occ, max_dist, job, cc, cn, cref, total,
                             stream=None):
        """mvs_wexp_children_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), occ uint8
        (V,ncj,nci), job int32 (cap,4), cc, cn float64 (cap,3), cref int32
        (cap,), total int64 (1,)); stream-ordered."""
        n, cap = int(ref.numel()), int(cref.numel())
        nci, ncj = self.cell_grid(cell_size)
        want = [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)),
                ("mask", mask, 8, (n, self.words)), ("occ", occ, 1, (self.V, ncj, nci)), ("job", job, 4, (cap, 4)),
                ("cc", cc, 8, (cap, 3)), ("cn", cn, 8, (cap, 3)), ("cref", cref, 4, (cap,)), ("total", total, 8, (1,))]
        for name, x, size, shape in want:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wexp_children_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wexp_children_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(),
                                             mask.data_ptr(), int(cell_size), occ.data_ptr(), float(max_dist), cap,
                                             job.data_ptr(), cc.data_ptr(), cn.data_ptr(), cref.data_ptr(),
                                             total.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wexp_children_device")

    def wexp_claim_device(self, job, accept, score, nci, ncj, win, stream=None):
        """mvs_wexp_claim_device on torch device tensors (contiguous: job int32
        (m,4), accept, win uint8 (m,), score float64 (m,)); stream-ordered."""
        m = int(accept.numel())
        for name, x, size, shape in [("job", job, 4, (m, 4)), ("accept", accept, 1, (m,)), ("score", score, 8, (m,)),
                                     ("win", win, 1, (m,))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wexp_claim_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wexp_claim_device(self._h, m, job.data_ptr(), accept.data_ptr(), score.data_ptr(), int(nci),
                                          int(ncj), win.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wexp_claim_device")

    def wexp_mark_device(self, job, win, cc, cref, mask, cell_size, occ, stream=None):
        """mvs_wexp_mark_device on torch device tensors (contiguous: job int32
        (m,4), win uint8 (m,), cc float64 (m,3), cref int32 (m,), mask int64
        (m,words), occ uint8 (V,ncj,nci), updated in place); stream-ordered."""
        m = int(win.numel())
        nci, ncj = self.cell_grid(cell_size)
        for name, x, size, shape in [("job", job, 4, (m, 4)), ("win", win, 1, (m,)), ("cc", cc, 8, (m, 3)),
                                     ("cref", cref, 4, (m,)), ("mask", mask, 8, (m, self.words)),
                                     ("occ", occ, 1, (self.V, ncj, nci))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wexp_mark_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wexp_mark_device(self._h, m, job.data_ptr(), win.data_ptr(), cc.data_ptr(), cref.data_ptr(),
                                         mask.data_ptr(), int(cell_size), occ.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wexp_mark_device")

    def _side_stream(self):
        """The context's torch side stream (the handle of torch's default stream
        is 0, which the C-ABI reads as "the context's own stream")."""
        import torch
        if self._refine_stream is None:
            self._refine_stream = torch.cuda.Stream(torch.device(f"cuda:{self.device}"))
        return self._refine_stream

    def wexp_children(self, c, nrm, ref, mask, cell_size, occ, max_dist, cap=None):
        """Child jobs and geometry of frontier patches (mvs_wexp_children_device)
        from numpy arrays or torch tensors, through torch device tensors: per
        patch and per view of {ref} + mask, the up to four vacant neighbour cells
        of the patch's cell in that view whose centre ray meets the parent's
        tangent plane within max_dist of the parent.  cap None: room for every
        job.  Returns jobs (k,4) int32 [parent, view, cell i, cell j], cc (k,3),
        cn (k,3), cref (k,) and the total found (k = min(total, cap)), as numpy."""
        import torch
        n = int(np.asarray(ref.cpu() if isinstance(ref, torch.Tensor) else ref).size)
        nci, ncj = self.cell_grid(cell_size)
        dev = torch.device(f"cuda:{self.device}")
        t_c = self._dev_tensor(c, torch.float64, (n, 3))
        t_n = self._dev_tensor(nrm, torch.float64, (n, 3))
        t_r = self._dev_tensor(ref, torch.int32, (n,))
        t_m = self._dev_tensor(mask, torch.int64, (n, self.words))
        t_o = self._dev_tensor(occ, torch.uint8, (self.V, ncj, nci))
        cap = 4 * self.V * n if cap is None else int(cap)
        job = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        cc = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        cn = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        cref = torch.empty(cap, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        st = self._side_stream()
        torch.cuda.current_stream(dev).synchronize()   # the inputs' copies, before the side stream reads them
        self.wexp_children_device(t_c, t_n, t_r, t_m, cell_size, t_o, max_dist, job, cc, cn, cref, total,
                                  stream=st.cuda_stream)
        st.synchronize()
        tot = int(total.item())
        k = min(tot, cap)
        return job[:k].cpu().numpy(), cc[:k].cpu().numpy(), cn[:k].cpu().numpy(), cref[:k].cpu().numpy(), tot

    def wexp_claim(self, jobs, accept, score, nci, ncj):
        """One winner per (view, cell) (mvs_wexp_claim_device) from numpy arrays or
        torch tensors: among the jobs with accept != 0 and a finite score that
        name one cell, the highest score wins, ties to the lowest index.
        Returns win (m,) uint8 as numpy."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        t_a = self._dev_tensor(accept, torch.uint8, (-1,))
        m = int(t_a.numel())
        t_j = self._dev_tensor(jobs, torch.int32, (m, 4))
        t_s = self._dev_tensor(score, torch.float64, (m,))
        win = torch.zeros(m, dtype=torch.uint8, device=dev)
        st = self._side_stream()
        torch.cuda.current_stream(dev).synchronize()
        self.wexp_claim_device(t_j, t_a, t_s, nci, ncj, win, stream=st.cuda_stream)
        st.synchronize()
        return win.cpu().numpy()

    def wexp_claim_checked(self, jobs, accept, score, nci, ncj):
        """The host-pointer claim (mvs_wexp_claim): as wexp_claim on numpy
        arrays, but a job whose (view, cell) lies outside the grid raises."""
        jobs = _c(jobs, np.int32).reshape(-1, 4)
        m = len(jobs)
        accept = _c(accept, np.uint8).reshape(m)
        score = _c(score, np.float64).reshape(m)
        win = np.zeros(max(m, 1), np.uint8)
        rc = load().mvs_wexp_claim(self._h, m, _p(jobs, _i32p), _p(accept, _u8p), _p(score, _dp), int(nci), int(ncj),
                                   _p(win, _u8p))
        check(rc, self._h, "mvs_wexp_claim")
        return win[:m]

    def wexp_mark(self, jobs, win, cc, cref, mask, cell_size, occ):
        """Fill the cells of the winners (mvs_wexp_mark_device) from numpy arrays
        or torch tensors: the job's own cell in its reference view and the cell
        of the centre's projection in every view of its mask.  Returns the new
        occupancy (V, ncj, nci) uint8 as numpy; the input is not modified."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        nci, ncj = self.cell_grid(cell_size)
        t_w = self._dev_tensor(win, torch.uint8, (-1,))
        m = int(t_w.numel())
        t_j = self._dev_tensor(jobs, torch.int32, (m, 4))
        t_c = self._dev_tensor(cc, torch.float64, (m, 3))
        t_r = self._dev_tensor(cref, torch.int32, (m,))
        t_m = self._dev_tensor(mask, torch.int64, (m, self.words))
        t_o = self._dev_tensor(occ, torch.uint8, (self.V, ncj, nci)).clone()
        st = self._side_stream()
        torch.cuda.current_stream(dev).synchronize()
        self.wexp_mark_device(t_j, t_w, t_c, t_r, t_m, cell_size, t_o, stream=st.cuda_stream)
        st.synchronize()
        return t_o.cpu().numpy()

    def expand_warped(self, c, nrm, ref, rounds, cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2, max_dist=None,
                      refine_levels=0, max_views=8, depth_px=1.0, max_patches=None, trace=False, timer=None):
        """Grow a patch set from seed patches (c, nrm, ref) by `rounds` rounds of a
        level-synchronous expansion driven by the plane-warped photo test:

          round 0: the seeds are the candidates, job (-1, ref, cell of the
            seed's projection into ref); a seed outside the grid is not accepted;
          every round: score_warped_device of the candidates; accept = count >=
            vlb; one winner per (view, cell) by the highest avg (wexp_claim);
            with refine_levels > 0 the winners are refined (refine_lists_device:
            the rule of refine_view_lists and refine_depth_steps(depth_px) on the
            device; refine_levels level calls at step_scale
            2^-level, kd 2, ka 1) and re-scored, and the refined patch replaces
            the winner when its count >= vlb and its avg >= the winner's; the
            winners' cells are filled (wexp_mark) with their final masks; the
            winners join the patch set and are the next frontier;
          later rounds: the candidates are the frontier's children (wexp_children).

        It stops after `rounds` rounds, when a round has no winner, or at
        max_patches (the last round's winners truncated in job order).
        max_dist None: 2 cell_size pixels at the first seed's depth in its
        reference view.  Everything runs on one torch side stream; the host
        reads two counters once per round (the next round's job total and this
        round's winners) and, with refinement, the winners' number once more
        (it sizes their buffers); no array crosses to the host inside a round.

        Returns a dict of numpy arrays over the patch set: c, nrm (P,3), ref
        (P,), mask (P,words) uint64, count, avg, round, parent (index into the
        patch set, -1 for seeds), cell (P,2) and occ (V,ncj,nci), max_dist.  With
        trace=True also "trace": per round a dict of jobs, cc, cn, cref, xy,
        mask, count, avg, ncc (as scored), accept, win, lists (nw, max_views)
        and dstep (nw,) fed to the level calls, kept (winners whose refined
        patch replaced them), refined (c, nrm, count, avg of the
        winners' refined patches, in winner order) and occ after marking.
        timer: an optional callable timer(phase, round) called on the chain's
        stream before each phase and with phase "end" after the last."""
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n0 = len(ref)
        if len(c) != n0 or len(nrm) != n0:
            raise RuntimeError("c, nrm and ref lengths differ")
        if n0 and (ref.min() < 0 or ref.max() >= self.V):
            raise RuntimeError("expand_warped: ref view out of range")
        rounds, refine_levels, vlb = int(rounds), int(refine_levels), int(vlb)
        s = int(cell_size)
        nci, ncj = self.cell_grid(s)
        if refine_levels and not 1 <= int(max_views) <= 32:
            raise RuntimeError("expand_warped: max_views must be in 1..32")
        Rp, K, t = self.rproj(), self._K, self._t
        if max_dist is None and n0:
            max_dist = 2.0 * s * float(self.refine_depth_steps(c[:1], ref[:1], 1.0)[0])
        # round 0 on the host: the seeds' cells (the library's projection, in Python floats)
        jobs0 = np.full((n0, 4), -1, np.int32)
        inside0 = np.zeros(n0, np.uint8)
        for k in range(n0):
            r = int(ref[k])
            jobs0[k, 1] = r
            X, Y, Z = (float(x) for x in c[k])
            R9 = [float(x) for x in Rp[r].reshape(9)]
            x = R9[0] * X + R9[1] * Y + R9[2] * Z + float(t[r, 0])
            y = R9[3] * X + R9[4] * Y + R9[5] * Z + float(t[r, 1])
            z = R9[6] * X + R9[7] * Y + R9[8] * Z + float(t[r, 2])
            w = 1.0 / z if z != 0.0 else 1.0
            x = x * w * float(K[r, 0, 0]) + float(K[r, 0, 2])
            y = y * w * float(K[r, 1, 1]) + float(K[r, 1, 2])
            if z > 0 and 0 <= x < self.W and 0 <= y < self.H and int(x) // s < nci and int(y) // s < ncj:
                jobs0[k, 2:] = (int(x) // s, int(y) // s)
                inside0[k] = 1
        return self._wexp_chain(rounds, (c, nrm, ref, jobs0, inside0), None, s, wid, min_ncc, min_cos, vlb, max_dist,
                                refine_levels, max_views, depth_px, max_patches, trace, timer)

    def _wexp_chain(self, rounds, seeds, start, s, wid, min_ncc, min_cos, vlb, max_dist, refine_levels, max_views,
                    depth_px, max_patches, trace, timer):
        """The rounds of expand_warped (seeds = (c, nrm, ref, jobs, inside) of
        round 0, start None) and of resume_warped (seeds None, start = the host
        arrays of an existing set and its occ or None).  From a set, the
        frontier of every round is the whole current set in row order and the
        first round's children cost one more counter read."""
        import torch
        V, words = self.V, self.words
        nci, ncj = self.cell_grid(s)
        dev = torch.device(f"cuda:{self.device}")
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        st = self._side_stream()
        sh = st.cuda_stream
        tick = timer if timer is not None else (lambda phase, rnd: None)
        want_ncc = trace or refine_levels > 0
        keys = ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell")
        out = {k: [] for k in keys}
        traces = []
        total, base, r0 = 0, 0, 0
        S = None   # from a set: its c, nrm, ref and mask on the device, every round's winners appended
        with torch.cuda.stream(st):
            counters = torch.zeros(2, **i64)   # [the next round's job total, this round's winners]

            def children(F, cap):
                nb = [torch.empty((cap, 4), **i32), torch.empty((cap, 3), **f64), torch.empty((cap, 3), **f64),
                      torch.empty(cap, **i32)]
                self.wexp_children_device(F[0], F[1], F[2], F[3], s, occ, max_dist, nb[0], nb[1], nb[2], nb[3],
                                          counters[:1], stream=sh)
                return nb

            if start is None:
                c, nrm, ref, jobs0, inside0 = seeds
                occ = torch.zeros((V, ncj, nci), **u8)
                job = torch.from_numpy(jobs0).to(dev)
                cc, cn, cref = (torch.from_numpy(x).to(dev) for x in (c, nrm, ref))
                inside = torch.from_numpy(inside0).to(dev)
                m = len(ref)
            else:
                host, occ0 = start
                for k in keys:
                    x = host[k].view(np.int64) if k == "mask" else host[k]
                    out[k].append(torch.from_numpy(x).to(dev))
                S = [out[k][0] for k in ("c", "nrm", "ref", "mask")]
                total = len(host["ref"])
                r0 = int(host["round"].max()) + 1 if total else 0
                if occ0 is not None:
                    occ = torch.from_numpy(occ0).to(dev)
                else:   # the set's cells, as filter_warped marks them
                    occ = torch.zeros((V, ncj, nci), **u8)
                    job = torch.cat([torch.full((total, 1), -1, **i32), S[2].reshape(total, 1), out["cell"][0]],
                                    1).contiguous()
                    self.wexp_mark_device(job, torch.ones(total, **u8), S[0], S[2], S[3], s, occ, stream=sh)
                inside = None
                m = 0
                if rounds > 0 and total and (max_patches is None or total < int(max_patches)):
                    tick("children", r0 - 1)
                    cap = min(4 * V * total, max(1 << 20, 16 * total))
                    nb = children(S, cap)
                    tot = int(counters[0].item())   # the first round's job total
                    if tot > cap:
                        cap = tot
                        nb = children(S, cap)
                    m = min(tot, cap)
                    job, cc, cn, cref = (x[:m].contiguous() for x in nb)
            for rnd in range(r0, r0 + rounds):
                if m == 0:
                    break
                tick("score", rnd)
                xy = torch.empty((m, 2), **f64)
                mask = torch.empty((m, words), **i64)
                count = torch.empty(m, **i32)
                avg = torch.empty(m, **f64)
                ncc = torch.empty((m, V), **f64) if want_ncc else None
                self.score_warped_device(cc, cn, cref, xy, mask, count, avg, ncc, min_ncc, wid, min_cos, stream=sh)
                tick("claim", rnd)
                accept = (count >= vlb).to(torch.uint8)
                if inside is not None:
                    accept = accept * inside
                win = torch.empty(m, **u8)
                self.wexp_claim_device(job, accept, avg, nci, ncj, win, stream=sh)
                if max_patches is not None:
                    room = max(int(max_patches) - total, 0)
                    win = win * (torch.cumsum(win.to(torch.int64), 0) <= room).to(torch.uint8)
                tr = None
                if trace:
                    tr = {"jobs": job, "cc": cc.clone(), "cn": cn.clone(), "cref": cref, "xy": xy, "mask": mask.clone(),
                          "count": count.clone(), "avg": avg.clone(), "ncc": ncc, "accept": accept, "win": win}
                if refine_levels > 0:
                    tick("refine", rnd)
                    # the winners' view lists and depth steps, from the round's ncc on the device
                    idx = torch.nonzero(win).reshape(-1)   # sizes the winners' buffers: the phase's one read
                    nw = int(idx.numel())
                    if nw:
                        wc, wn, wr_ = cc[idx].contiguous(), cn[idx].contiguous(), cref[idx].contiguous()
                        t_lists, t_dstep = torch.empty((nw, int(max_views)), **i32), torch.empty(nw, **f64)
                        self.refine_lists_device(ncc, cc, cref, t_lists, t_dstep, idx, min_ncc, int(max_views),
                                                 depth_px, stream=sh)
                        cur, nxt = [wc, wn], [torch.empty((nw, 3), **f64), torch.empty((nw, 3), **f64)]
                        best, sbest = torch.empty(nw, **i32), torch.empty(nw, **f64)
                        for lev in range(refine_levels):
                            self.refine_warped_level_device(cur[0], cur[1], wr_, t_lists, t_dstep, nxt[0], nxt[1],
                                                            best, sbest, None, wid, min_cos, 2, 1, math.radians(8),
                                                            2.0 ** -lev, stream=sh)
                            cur, nxt = nxt, cur
                        xy2 = torch.empty((nw, 2), **f64)
                        mask2 = torch.empty((nw, words), **i64)
                        count2 = torch.empty(nw, **i32)
                        avg2 = torch.empty(nw, **f64)
                        self.score_warped_device(cur[0], cur[1], wr_, xy2, mask2, count2, avg2, None, min_ncc, wid,
                                                 min_cos, stream=sh)
                        kept = (count2 >= vlb) & (avg2 >= avg[idx])
                        ki = idx[kept]
                        cc[ki], cn[ki] = cur[0][kept], cur[1][kept]
                        mask[ki], count[ki], avg[ki] = mask2[kept], count2[kept], avg2[kept]
                        if trace:
                            tr["lists"], tr["dstep"] = t_lists, t_dstep
                            tr["kept"] = kept.to(torch.uint8)
                            tr["refined"] = {"c": cur[0], "nrm": cur[1], "count": count2, "avg": avg2}
                tick("mark", rnd)
                self.wexp_mark_device(job, win, cc, cref, mask, s, occ, stream=sh)
                if trace:
                    tr["occ"] = occ.clone()
                    traces.append(tr)
                # the next round's children from every job: a job that did not win gets
                # no view (ref -1, empty mask), so the order is the winners' order
                last = rnd + 1 >= r0 + rounds
                winb = win.bool()
                counters[1] = win.sum()
                if not last:
                    tick("children", rnd)
                    f_ref = torch.where(winb, cref, torch.full_like(cref, -1))
                    f_mask = mask * winb.to(torch.int64)[:, None]
                    F = [cc, cn, f_ref, f_mask]
                    if S is not None:   # the whole set first, then this round's jobs
                        F = [torch.cat([x, y]) for x, y in zip(S, F)]
                    nf = int(F[2].numel())
                    cap = min(4 * V * nf, max(1 << 20, 16 * nf))
                    nb = children(F, cap)
                tick("sync", rnd)
                tot, nw = (int(x) for x in counters.cpu())   # the round's one read
                if not last and tot > cap and nw and (max_patches is None or total + nw < max_patches):
                    # more jobs than the first guess holds: the same call again with room for all
                    cap = tot
                    nb = children(F, cap)
                tick("append", rnd)
                if nw == 0:
                    break
                rank = torch.cumsum(win.to(torch.int64), 0) - 1   # a job's index among the round's winners
                out["c"].append(cc[winb]); out["nrm"].append(cn[winb]); out["ref"].append(cref[winb])
                out["mask"].append(mask[winb]); out["count"].append(count[winb]); out["avg"].append(avg[winb])
                out["round"].append(torch.full((nw,), rnd, **i32))
                par = job[winb, 0].to(torch.int64)
                # from a set the parent already is a row of the set (the remapping below)
                out["parent"].append(torch.where(par >= 0, par + base, par) if S is None else par)
                out["cell"].append(job[winb, 2:])
                base, total = total, total + nw
                if last or (max_patches is not None and total >= int(max_patches)):
                    break
                m = min(tot, cap)
                job, cc, cn, cref = (x[:m].contiguous() for x in nb)
                j0 = job[:, 0].long()
                if S is None:
                    job[:, 0] = rank[j0].to(torch.int32)   # parent: job index -> index among the winners
                else:
                    # parent: a row of the set as it is, a job index -> the winner's row behind the set
                    job[:, 0] = torch.where(j0 < base, j0, base + rank[(j0 - base).clamp(min=0)]).to(torch.int32)
                    S = [torch.cat([x, out[k][-1]]) for x, k in zip(S, ("c", "nrm", "ref", "mask"))]
                inside = None
            tick("end", r0 + rounds)
            empty = {"c": torch.empty((0, 3), **f64), "nrm": torch.empty((0, 3), **f64), "ref": torch.empty(0, **i32),
                     "mask": torch.empty((0, words), **i64), "count": torch.empty(0, **i32),
                     "avg": torch.empty(0, **f64), "round": torch.empty(0, **i32), "parent": torch.empty(0, **i64),
                     "cell": torch.empty((0, 2), **i32)}
            res = {k: (torch.cat(v) if v else empty[k]).cpu().numpy() for k, v in out.items()}
            res["mask"] = res["mask"].view(np.uint64)
            res["occ"] = occ.cpu().numpy()
            res["max_dist"] = max_dist
            if trace:
                def host(x):
                    if isinstance(x, dict):
                        return {k: host(v) for k, v in x.items()}
                    x = x.cpu().numpy()
                    return x.view(np.uint64) if x.dtype == np.int64 and x.ndim == 2 and x.shape[1] == words else x
                res["trace"] = [host(tr) for tr in traces]
        st.synchronize()
        return res

    def resume_warped(self, patches, rounds, cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2, max_dist=None,
                      refine_levels=0, max_views=8, depth_px=1.0, max_patches=None, trace=False, timer=None):
        """Grow an existing patch set by `rounds` more rounds of expand_warped's
        expansion.  `patches` is a dict as expand_warped or filter_warped
        returns it; it needs c, nrm, ref, mask, count, avg, round, parent and
        cell.  Every row must be alive (ref in 0..V-1) and every cell inside the
        grid of cell_size.  occ is patches["occ"] when that has the shape
        (V,ncj,nci); otherwise it is rebuilt from the rows (wexp_mark_device
        with the jobs (-1, ref, cell), as filter_warped does).  max_dist: the
        argument, else patches["max_dist"], else expand_warped's rule on the
        first row.

        No row of the input is scored again.  The frontier of every round is
        the whole current set in row order, the input first; its children
        (wexp_children_device) are the round's candidates, and the round is an
        expand_warped round from there: score, accept, claim, optional
        refinement, mark.  An older patch's vacant neighbours are the candidates
        that failed before; they fail again and compete for nothing, so
        resuming k rounds from the set of R rounds gives the set of R + k
        rounds.  The host reads the same two counters once per round, and the
        first round's job total once more.  It stops after `rounds` rounds, at
        a round with no job or no winner, or at max_patches, which counts the
        input.

        Returns expand_warped's dict: the input rows unchanged, then the new
        rows (parent indexes the returned set, round continues from the
        input's highest + 1), occ and max_dist.  rounds = 0 returns the input
        with its occ."""
        keys = ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell")
        for k in keys:
            if k not in patches:
                raise RuntimeError(f"resume_warped: patches has no '{k}'")
        rounds, refine_levels, vlb = int(rounds), int(refine_levels), int(vlb)
        if rounds < 0:
            raise RuntimeError("resume_warped: rounds < 0")
        if refine_levels and not 1 <= int(max_views) <= 32:
            raise RuntimeError("resume_warped: max_views must be in 1..32")
        s = int(cell_size)
        nci, ncj = self.cell_grid(s)
        ref = _c(patches["ref"], np.int32).reshape(-1)
        n = len(ref)
        host = {"c": _c(patches["c"], np.float64).reshape(n, 3), "nrm": _c(patches["nrm"], np.float64).reshape(n, 3),
                "ref": ref, "mask": _c(patches["mask"], np.uint64).reshape(n, self.words),
                "count": _c(patches["count"], np.int32).reshape(n), "avg": _c(patches["avg"], np.float64).reshape(n),
                "round": _c(patches["round"], np.int32).reshape(n),
                "parent": _c(patches["parent"], np.int64).reshape(n),
                "cell": _c(patches["cell"], np.int32).reshape(n, 2)}
        if n and (ref.min() < 0 or ref.max() >= self.V):
            raise RuntimeError("resume_warped: a row is dead (ref outside 0..V-1)")
        cell = host["cell"]
        if n and (cell.min() < 0 or cell[:, 0].max() >= nci or cell[:, 1].max() >= ncj):
            raise RuntimeError("resume_warped: a cell lies outside the grid")
        occ = patches.get("occ")
        if occ is not None:
            occ = np.asarray(occ)
            occ = _c(occ, np.uint8) if occ.shape == (self.V, ncj, nci) else None
        if max_dist is None:
            max_dist = patches.get("max_dist")
        if max_dist is None and n:
            max_dist = 2.0 * s * float(self.refine_depth_steps(host["c"][:1], ref[:1], 1.0)[0])
        return self._wexp_chain(rounds, None, (host, occ), s, wid, min_ncc, min_cos, vlb, max_dist, refine_levels,
                                max_views, depth_px, max_patches, trace, timer)

    # ---- visibility-consistency filter of a warped patch set ----

    def wfilt_front_device(self, c, ref, mask, cell_size, front, zfront, stream=None):
        """mvs_wfilt_front_device on torch device tensors (contiguous: c float64
        (n,3), ref int32 (n,), mask int64 (n,words), front int32 and zfront
        float64 (V,ncj,nci), both written whole); stream-ordered."""
        n = int(ref.numel())
        nci, ncj = self.cell_grid(cell_size)
        for name, x, size, shape in [("c", c, 8, (n, 3)), ("ref", ref, 4, (n,)), ("mask", mask, 8, (n, self.words)),
                                     ("front", front, 4, (self.V, ncj, nci)),
                                     ("zfront", zfront, 8, (self.V, ncj, nci))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wfilt_front_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wfilt_front_device(self._h, n, c.data_ptr(), ref.data_ptr(), mask.data_ptr(), int(cell_size),
                                           front.data_ptr(), zfront.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wfilt_front_device")

    def wfilt_test_device(self, c, nrm, ref, mask, avg, cell_size, adj_px, min_views, front, vis, conf, keep,
                          stream=None):
        """mvs_wfilt_test_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), avg float64 (n,),
        front int32 (V,ncj,nci), vis int64 (n,words), conf int64 (n,), keep uint8
        (n,)); stream-ordered."""
        n = int(ref.numel())
        nci, ncj = self.cell_grid(cell_size)
        for name, x, size, shape in [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)),
                                     ("mask", mask, 8, (n, self.words)), ("avg", avg, 8, (n,)),
                                     ("front", front, 4, (self.V, ncj, nci)), ("vis", vis, 8, (n, self.words)),
                                     ("conf", conf, 8, (n,)), ("keep", keep, 1, (n,))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wfilt_test_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wfilt_test_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                          avg.data_ptr(), int(cell_size), float(adj_px), int(min_views),
                                          front.data_ptr(), vis.data_ptr(), conf.data_ptr(), keep.data_ptr(),
                                          self._stream_handle(stream))
        check(rc, self._h, "mvs_wfilt_test_device")

    def wfilt_front(self, c, ref, mask, cell_size):
        """The front grid of a patch set (mvs_wfilt_front, host pointers): per
        (view, cell) the placed patch of least depth, ties to the lowest index.
        Returns front (V,ncj,nci) int32 (-1 = empty) and zfront float64 (+inf)."""
        nci, ncj = self.cell_grid(cell_size)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        c = _c(c, np.float64).reshape(n, 3)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        front = np.empty((self.V, ncj, nci), np.int32)
        zfront = np.empty((self.V, ncj, nci), np.float64)
        rc = load().mvs_wfilt_front(self._h, n, _p(c, _dp), _p(ref, _i32p), _p(mask, _u64p), int(cell_size),
                                    _p(front, _i32p), _p(zfront, _dp))
        check(rc, self._h, "mvs_wfilt_front")
        return front, zfront

    def wfilt_test(self, c, nrm, ref, mask, avg, cell_size, adj_px, min_views, front):
        """The visibility and conflict test of a patch set against a front grid
        (mvs_wfilt_test, host pointers; a front entry outside -1..n-1 raises).
        Returns vis (n,words) uint64, conf (n,) int64 and keep (n,) uint8."""
        nci, ncj = self.cell_grid(cell_size)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        c = _c(c, np.float64).reshape(n, 3)
        nrm = _c(nrm, np.float64).reshape(n, 3)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        avg = _c(avg, np.float64).reshape(n)
        front = _c(front, np.int32).reshape(self.V, ncj, nci)
        vis = np.zeros((max(n, 1), self.words), np.uint64)
        conf = np.zeros(max(n, 1), np.int64)
        keep = np.zeros(max(n, 1), np.uint8)
        rc = load().mvs_wfilt_test(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(mask, _u64p),
                                   _p(avg, _dp), int(cell_size), float(adj_px), int(min_views), _p(front, _i32p),
                                   _p(vis, _u64p), _p(conf, _i64p), _p(keep, _u8p))
        check(rc, self._h, "mvs_wfilt_test")
        return vis[:n], conf[:n], keep[:n]

    def wfilt_support_device(self, c, nrm, ref, mask, cell_size, adj_px, min_support, min_neigh, front, nb, adj, keep,
                             stream=None):
        """mvs_wfilt_support_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), front int32
        (V,ncj,nci), nb and adj int32 (n,), keep uint8 (n,)); stream-ordered."""
        n = int(ref.numel())
        nci, ncj = self.cell_grid(cell_size)
        for name, x, size, shape in [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)),
                                     ("mask", mask, 8, (n, self.words)), ("front", front, 4, (self.V, ncj, nci)),
                                     ("nb", nb, 4, (n,)), ("adj", adj, 4, (n,)), ("keep", keep, 1, (n,))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wfilt_support_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wfilt_support_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                             int(cell_size), float(adj_px), float(min_support), int(min_neigh),
                                             front.data_ptr(), nb.data_ptr(), adj.data_ptr(), keep.data_ptr(),
                                             self._stream_handle(stream))
        check(rc, self._h, "mvs_wfilt_support_device")

    def wfilt_support(self, c, nrm, ref, mask, cell_size, adj_px, min_support, min_neigh, front):
        """The neighbour-support test of a patch set against a front grid
        (mvs_wfilt_support, host pointers; a front entry outside -1..n-1 raises).
        Returns nb (n,) int32, adj (n,) int32 and keep (n,) uint8."""
        nci, ncj = self.cell_grid(cell_size)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        c = _c(c, np.float64).reshape(n, 3)
        nrm = _c(nrm, np.float64).reshape(n, 3)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        front = _c(front, np.int32).reshape(self.V, ncj, nci)
        nb = np.zeros(max(n, 1), np.int32)
        adj = np.zeros(max(n, 1), np.int32)
        keep = np.zeros(max(n, 1), np.uint8)
        rc = load().mvs_wfilt_support(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(mask, _u64p),
                                      int(cell_size), float(adj_px), float(min_support), int(min_neigh),
                                      _p(front, _i32p), _p(nb, _i32p), _p(adj, _i32p), _p(keep, _u8p))
        check(rc, self._h, "mvs_wfilt_support")
        return nb[:n], adj[:n], keep[:n]

    def filter_warped(self, patches, cell_size=2, adj_px=2.0, min_views=3, passes=2, timer=None, min_support=None,
                      min_neigh=1, support_passes=1):
        """Remove the patches of a warped patch set that contradict the
        visibility of the rest (the definition is in include/mvs_amd.h).
        `patches` is the dict expand_warped returns; it needs c, nrm, ref, mask,
        avg and cell.  Each pass builds the front grid of the rows still alive
        (wfilt_front_device), runs the test (wfilt_test_device) and sets the
        removed rows' ref to -1 on the device; nothing is compacted between
        passes.  It stops after `passes` passes or when a pass removes nothing.
        Everything runs on the context's torch side stream; the host reads one
        counter per pass, the survivors.

        min_support not None: after the visibility passes, up to support_passes
        passes of the neighbour-support test (wfilt_support_device with adj_px,
        min_support and min_neigh) in the same way: the front grid of the rows
        still alive, the test, ref = -1 for the removed rows, one counter read;
        they stop when a pass removes nothing.  The dict then also holds nb and
        adj (int32, the last support pass over the input; zeros when none ran)
        and removed_support (per support pass).  The timer's phases of a
        support pass are "sfront", "support" and "ssync".

        Returns a dict of numpy arrays: the surviving rows of every per-patch
        array of the input (parent keeps the input's numbering), index (their
        rows in the input), keep (over the input), vis (words uint64) and conf
        (int64) of the last pass over the input, removed (per pass), front and
        zfront (V,ncj,nci) rebuilt from the survivors, and occ (V,ncj,nci): the
        survivors' cells through wexp_mark_device with the jobs (-1, ref, cell).
        timer: an optional callable timer(phase, pass) called on the chain's
        stream before each phase and with phase "end" after the last."""
        import torch
        for k in ("c", "nrm", "ref", "mask", "avg", "cell"):
            if k not in patches:
                raise RuntimeError(f"filter_warped: patches has no '{k}'")
        ref0 = _c(patches["ref"], np.int32).reshape(-1)
        n = len(ref0)
        V, words = self.V, self.words
        s = int(cell_size)
        nci, ncj = self.cell_grid(s)
        passes = int(passes)
        if passes < 0:
            raise RuntimeError("filter_warped: passes < 0")
        support_passes = int(support_passes) if min_support is not None else 0
        if support_passes < 0:
            raise RuntimeError("filter_warped: support_passes < 0")
        c0 = _c(patches["c"], np.float64).reshape(n, 3)
        n0 = _c(patches["nrm"], np.float64).reshape(n, 3)
        m0 = _c(patches["mask"], np.uint64).reshape(n, words)
        a0 = _c(patches["avg"], np.float64).reshape(n)
        cell0 = _c(patches["cell"], np.int32).reshape(n, 2)
        dev = torch.device(f"cuda:{self.device}")
        st = self._side_stream()
        sh = st.cuda_stream
        tick = timer if timer is not None else (lambda phase, k: None)
        removed = []
        alive = int(((ref0 >= 0) & (ref0 < V)).sum())
        with torch.cuda.stream(st):
            c, nrm, ref, avg = (torch.from_numpy(x).to(dev) for x in (c0, n0, ref0.copy(), a0))
            mask = torch.from_numpy(m0.view(np.int64)).to(dev)
            front = torch.empty((V, ncj, nci), dtype=torch.int32, device=dev)
            zfront = torch.empty((V, ncj, nci), dtype=torch.float64, device=dev)
            vis = torch.zeros((n, words), dtype=torch.int64, device=dev)
            conf = torch.zeros(n, dtype=torch.int64, device=dev)
            keep = torch.empty(n, dtype=torch.uint8, device=dev)
            for k in range(passes):
                tick("front", k)
                self.wfilt_front_device(c, ref, mask, s, front, zfront, stream=sh)
                tick("test", k)
                self.wfilt_test_device(c, nrm, ref, mask, avg, s, adj_px, min_views, front, vis, conf, keep, stream=sh)
                ref.masked_fill_(keep == 0, -1)
                tick("sync", k)
                left = int(keep.sum().item())   # the pass's one read
                removed.append(alive - left)
                alive = left
                if removed[-1] == 0:
                    break
            if min_support is not None:
                removed_support = []
                nb = torch.zeros(n, dtype=torch.int32, device=dev)
                adj = torch.zeros(n, dtype=torch.int32, device=dev)
                if support_passes == 0 or n == 0:   # no pass runs the call: its scalar checks all the same
                    self.wfilt_support_device(c[:0], nrm[:0], ref[:0], mask[:0], s, adj_px, min_support, min_neigh,
                                              front, nb[:0], adj[:0], keep[:0], stream=sh)
                for k in range(support_passes):
                    tick("sfront", k)
                    self.wfilt_front_device(c, ref, mask, s, front, zfront, stream=sh)
                    tick("support", k)
                    self.wfilt_support_device(c, nrm, ref, mask, s, adj_px, min_support, min_neigh, front, nb, adj,
                                              keep, stream=sh)
                    ref.masked_fill_(keep == 0, -1)
                    tick("ssync", k)
                    left = int(keep.sum().item())   # the pass's one read
                    removed_support.append(alive - left)
                    alive = left
                    if removed_support[-1] == 0:
                        break
            tick("rebuild", passes)
            self.wfilt_front_device(c, ref, mask, s, front, zfront, stream=sh)
            tick("occ", passes)
            live = ((ref >= 0) & (ref < V)).to(torch.uint8)
            job = torch.cat([torch.full((n, 1), -1, dtype=torch.int32, device=dev), ref.reshape(n, 1),
                             torch.from_numpy(cell0).to(dev)], 1).contiguous()
            occ = torch.zeros((V, ncj, nci), dtype=torch.uint8, device=dev)
            self.wexp_mark_device(job, live, c, ref, mask, s, occ, stream=sh)
            tick("end", passes)
            h_keep = live.cpu().numpy()
            res = {"keep": h_keep, "vis": vis.cpu().numpy().view(np.uint64), "conf": conf.cpu().numpy(),
                   "front": front.cpu().numpy(), "zfront": zfront.cpu().numpy(), "occ": occ.cpu().numpy()}
            if min_support is not None:
                res.update({"nb": nb.cpu().numpy(), "adj": adj.cpu().numpy(), "removed_support": removed_support})
        st.synchronize()
        index = np.flatnonzero(h_keep).astype(np.int64)
        out = {k: np.asarray(v)[index] for k, v in patches.items()
               if k not in ("occ", "trace") and isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n}
        out.update(res)
        out["index"] = index
        out["removed"] = removed
        return out

    @staticmethod
    def renumber_parents(parent, index, n):
        """The parents of the rows `index` (ascending) of an n-row set in the
        numbering of those rows alone: a removed parent becomes -2, a seed's -1
        and an earlier -2 stay."""
        parent = np.asarray(parent, np.int64)
        new = np.full(n + 1, -2, np.int64)        # the last element serves the negative parents
        new[np.asarray(index, np.int64)] = np.arange(len(index))
        return np.where(parent >= 0, new[np.where(parent >= 0, parent, n)], parent)

    def reconstruct_warped(self, c, nrm, ref, iterations=3, rounds=4, resume_rounds=2, expand=None, filter=None,
                           start=None, timer=None):
        """PMVS's expand -> filter loop on the warped pipeline: expand_warped of
        the seeds (c, nrm, ref) for `rounds` rounds, then `iterations` times
        filter_warped and, unless it was the last filter, resume_warped for
        resume_rounds rounds from the survivors and their occ.  `expand` holds
        the keywords of expand_warped and resume_warped, `filter` those of
        filter_warped; cell_size is shared (give it in `expand`).  After every
        filter the survivors' parent is renumbered through index
        (renumber_parents).  start: an existing set (a dict as resume_warped
        takes it, with max_dist) to loop on in place of the seeds' expansion;
        c, nrm, ref and rounds are then unused.  timer: an optional callable
        timer(stage, iteration, phase, k) that receives the phase marks of every
        stage ("expand", "filter", "resume") as that stage's own timer would.

        Returns the last filter_warped's dict with parent renumbered, max_dist,
        and history: per iteration a dict of patches (the set's size before the
        filter), removed, removed_support and resumed (the size after the
        resumption, None after the last filter)."""
        expand, filt = dict(expand or {}), dict(filter or {})
        for k in ("trace", "timer"):
            if k in expand or k in filt:
                raise RuntimeError(f"reconstruct_warped: '{k}' belongs to the single calls")

        def stage(name, it):   # the stages' phase marks, told apart
            return None if timer is None else (lambda phase, k: timer(name, it, phase, k))

        if filt.setdefault("cell_size", expand.get("cell_size", 2)) != expand.get("cell_size", 2):
            raise RuntimeError("reconstruct_warped: expand and filter disagree on cell_size")
        iterations = int(iterations)
        if iterations < 1:
            raise RuntimeError("reconstruct_warped: iterations < 1")
        ps = start if start is not None else self.expand_warped(c, nrm, ref, rounds, timer=stage("expand", 0),
                                                                **expand)
        grow = dict(expand, max_dist=ps["max_dist"])
        history = []
        for it in range(iterations):
            before = len(ps["ref"])
            ps = self.filter_warped(ps, timer=stage("filter", it), **filt)
            ps["parent"] = self.renumber_parents(ps["parent"], ps["index"], before)
            history.append({"patches": before, "removed": ps["removed"],
                            "removed_support": ps.get("removed_support", []), "resumed": None})
            if it + 1 < iterations:
                ps = self.resume_warped(ps, resume_rounds, timer=stage("resume", it), **grow)
                history[-1]["resumed"] = len(ps["ref"])
        ps["max_dist"] = grow["max_dist"]
        ps["history"] = history
        return ps

    # ---- seeds from image features, patch colours ----

    def wseed_pairs(self, neighbours=4, min_axis_cos=0.5):
        """The view pairs the seed matcher is fed (seed_view_pairs on the
        context's rotations): (np, 2) int32, r-major."""
        return seed_view_pairs(self.rproj(), neighbours, min_axis_cos)

    def _seed_tables(self, feat_off, pairs):
        feat_off = _c(feat_off, np.int64).reshape(-1)
        if len(feat_off) != self.V + 1:
            raise RuntimeError(f"wseed_match: feat_off must have V + 1 = {self.V + 1} entries")
        pairs = _c(pairs, np.int32).reshape(-1, 2)
        return feat_off, pairs

    def wseed_match_device(self, feat, feat_off, pairs, epi_px, min_sin2, c, nrm, ref, cand, err, total, stream=None):
        """mvs_wseed_match_device: feat a torch device tensor (contiguous int32
        (F,2) [col, row]), feat_off (V+1,) and pairs (np,2) host arrays, the
        outputs torch device tensors (contiguous: c, nrm float64 (cap,3), ref
        int32 (cap,), cand int32 (cap,4), err float64 (cap,), total int64 (1,))
        or, to count only, c = nrm = ref = cand = err = None; stream-ordered."""
        feat_off, pairs = self._seed_tables(feat_off, pairs)
        F = int(feat.shape[0])
        if feat.dtype.itemsize != 4 or tuple(feat.shape) != (F, 2) or not feat.is_contiguous():
            raise RuntimeError("wseed_match_device: feat must be contiguous int32 (F, 2)")
        if len(feat_off) and int(feat_off[-1]) > F:
            raise RuntimeError("wseed_match_device: feat_off names more features than feat holds")
        outs = [c, nrm, ref, cand, err]
        cap = 0
        if any(x is not None for x in outs):
            cap = int(ref.numel())
            for name, x, size, shape in [("c", c, 8, (cap, 3)), ("nrm", nrm, 8, (cap, 3)), ("ref", ref, 4, (cap,)),
                                         ("cand", cand, 4, (cap, 4)), ("err", err, 8, (cap,))]:
                if x is None or x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                    raise RuntimeError(f"wseed_match_device: {name} must be contiguous, {size}-byte elements, {shape}")
        if total.dtype.itemsize != 8 or tuple(total.shape) != (1,):
            raise RuntimeError("wseed_match_device: total must be int64 (1,)")
        ptr = (lambda x: x.data_ptr() if cap else None)
        rc = load().mvs_wseed_match_device(self._h, feat.data_ptr(), _p(feat_off, _i64p), len(pairs), _p(pairs, _i32p),
                                           float(epi_px), float(min_sin2), cap, ptr(c), ptr(nrm), ptr(ref), ptr(cand),
                                           ptr(err), total.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wseed_match_device")

    def wseed_match(self, feat, feat_off, pairs, epi_px=1.5, min_sin2=1e-4, cap=None):
        """Seed candidates from features (mvs_wseed_match, host pointers): every
        pair (feature a of view r, feature b of view v) of the ordered view
        pairs whose rays pass each other in front of both cameras, with the point
        on a's ray within epi_px pixels of b in v, triangulated into a patch
        (centre on a's ray, normal towards r's camera); the definition is in
        include/mvs_amd.h.  feat (F,2) int32 [col, row] of all views, feat_off
        (V+1,), pairs (np,2).  cap None: a counting call first, then room for
        every candidate.  Returns c (k,3), nrm (k,3), ref (k,) int32, cand (k,4)
        int32 [pair, a, b, v], err (k,) and the total found (k = min(total, cap))."""
        feat_off, pairs = self._seed_tables(feat_off, pairs)
        feat = _c(feat, np.int32).reshape(-1, 2)
        if len(feat_off) and int(feat_off[-1]) > len(feat):
            raise RuntimeError("wseed_match: feat_off names more features than feat holds")
        lib = load()
        total = np.zeros(1, np.int64)

        def call(cap, c, nrm, ref, cand, err):
            opt = (lambda x, t: _p(x, t) if cap else None)
            rc = lib.mvs_wseed_match(self._h, _p(feat, _i32p), _p(feat_off, _i64p), len(pairs), _p(pairs, _i32p),
                                     float(epi_px), float(min_sin2), int(cap), opt(c, _dp), opt(nrm, _dp),
                                     opt(ref, _i32p), opt(cand, _i32p), opt(err, _dp), _p(total, _i64p))
            check(rc, self._h, "mvs_wseed_match")

        if cap is None:
            call(0, None, None, None, None, None)
            cap = int(total[0])
        cap = int(cap)
        c, nrm = np.empty((max(cap, 1), 3)), np.empty((max(cap, 1), 3))
        ref, cand = np.empty(max(cap, 1), np.int32), np.empty((max(cap, 1), 4), np.int32)
        err = np.empty(max(cap, 1))
        total[0] = 0
        call(cap, c, nrm, ref, cand, err)
        k = min(int(total[0]), cap)
        return c[:k], nrm[:k], ref[:k], cand[:k], err[:k], int(total[0])

    def seed_features(self, border):
        """harris_points of every view without the points closer than `border`
        pixels to an image edge: a list of (n_v, 2) int32 [col, row]."""
        b = int(border)
        out = []
        for v in range(self.V):
            p = self.harris_points(v)
            out.append(p[(p[:, 0] >= b) & (p[:, 0] <= self.W - 1 - b) & (p[:, 1] >= b) & (p[:, 1] <= self.H - 1 - b)])
        return out

    def seed_warped(self, feats=None, pairs=None, epi_px=1.5, min_sin2=1e-4, border=None, wid=5):
        """Seed candidates of the warped pipeline from image features (PMVS's
        match step): feats None: harris_points per view; the features closer
        than border (None: wid + 1) to an image edge are dropped; pairs None:
        wseed_pairs(); then one counting and one emitting wseed_match_device
        call on the context's side stream.  feats: a list of V arrays (n_v, 2)
        [col, row].  Returns c (n,3), nrm (n,3), ref (n,) int32, cand (n,4) int32
        [pair, a, b, v] (a, b index the features kept) and err (n,) as numpy;
        the counts are left in self.last_seed (features, pairs, tests, candidates)."""
        import torch
        border = int(wid) + 1 if border is None else int(border)
        if feats is None:
            feats = self.seed_features(border)
        else:
            if len(feats) != self.V:
                raise RuntimeError("seed_warped: feats must hold one array per view")
            feats = [_c(f, np.int32).reshape(-1, 2) for f in feats]
            feats = [f[(f[:, 0] >= border) & (f[:, 0] <= self.W - 1 - border) & (f[:, 1] >= border)
                       & (f[:, 1] <= self.H - 1 - border)] for f in feats]
        pairs = self.wseed_pairs() if pairs is None else _c(pairs, np.int32).reshape(-1, 2)
        nv = np.array([len(f) for f in feats], np.int64)
        feat_off = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
        feat = np.concatenate(feats) if len(feats) else np.empty((0, 2), np.int32)
        tests = int(sum(int(nv[r]) * int(nv[v]) for r, v in pairs)) if len(pairs) and pairs.min() >= 0 \
            and pairs.max() < self.V else 0
        self.last_seed = {"features": int(nv.sum()), "pairs": len(pairs), "tests": tests, "candidates": 0,
                          "feats": feats}
        dev = torch.device(f"cuda:{self.device}")
        st = self._side_stream()
        with torch.cuda.stream(st):
            t_feat = torch.from_numpy(_c(feat, np.int32).reshape(-1, 2)).to(dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            self.wseed_match_device(t_feat, feat_off, pairs, epi_px, min_sin2, None, None, None, None, None, total,
                                    stream=st.cuda_stream)
            n = int(total.item())
            c = torch.empty((n, 3), dtype=torch.float64, device=dev)
            nrm = torch.empty((n, 3), dtype=torch.float64, device=dev)
            ref = torch.empty(n, dtype=torch.int32, device=dev)
            cand = torch.empty((n, 4), dtype=torch.int32, device=dev)
            err = torch.empty(n, dtype=torch.float64, device=dev)
            if n:
                self.wseed_match_device(t_feat, feat_off, pairs, epi_px, min_sin2, c, nrm, ref, cand, err, total,
                                        stream=st.cuda_stream)
            out = tuple(x.cpu().numpy() for x in (c, nrm, ref, cand, err))
        st.synchronize()
        self.last_seed["candidates"] = n
        return out

    def wpatch_color_device(self, c, ref, mask, color, nviews, stream=None):
        """mvs_wpatch_color_device on torch device tensors (contiguous: c float64
        (n,3), ref int32 (n,), mask int64 (n,words), color float64 (n,3), nviews
        int32 (n,)); stream-ordered."""
        n = int(ref.numel())
        for name, x, size, shape in [("c", c, 8, (n, 3)), ("ref", ref, 4, (n,)), ("mask", mask, 8, (n, self.words)),
                                     ("color", color, 8, (n, 3)), ("nviews", nviews, 4, (n,))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wpatch_color_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wpatch_color_device(self._h, n, c.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                            color.data_ptr(), nviews.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wpatch_color_device")

    def wpatch_color(self, c, ref, mask):
        """The colour of patches (mvs_wpatch_color, host pointers): per channel
        the mean over the views of {ref} + mask that see the centre of the
        bilinear sample of the resident RGB image there, in steps of 1/256.
        Returns color (n,3) float64 (0 where no view sees it) and nviews (n,) int32."""
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        c = _c(c, np.float64).reshape(n, 3)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        color = np.zeros((max(n, 1), 3))
        nviews = np.zeros(max(n, 1), np.int32)
        rc = load().mvs_wpatch_color(self._h, n, _p(c, _dp), _p(ref, _i32p), _p(mask, _u64p), _p(color, _dp),
                                     _p(nviews, _i32p))
        check(rc, self._h, "mvs_wpatch_color")
        return color[:n], nviews[:n]

    def _view_range(self, views):
        """(v0, nv) of a view range given as None (every view) or (v0, nv)."""
        v0, nv = (0, self.V) if views is None else (int(views[0]), int(views[1]))
        if v0 < 0 or nv < 1 or v0 + nv > self.V:
            raise RuntimeError("the view range (v0, nv) must lie inside 0..V-1, nv >= 1")
        return v0, nv

    def wdepth_splat_device(self, c, nrm, ref, mask, radius, slope, v0, nv, zmap, idmap, stream=None):
        """mvs_wdepth_splat_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), zmap float64 and
        idmap int32 (nv,H,W), both written whole); stream-ordered."""
        n = int(ref.numel())
        maps = (int(nv), self.H, self.W)
        for name, x, size, shape in [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)),
                                     ("mask", mask, 8, (n, self.words)), ("zmap", zmap, 8, maps),
                                     ("idmap", idmap, 4, maps)]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wdepth_splat_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wdepth_splat_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                            int(radius), float(slope), int(v0), int(nv), zmap.data_ptr(),
                                            idmap.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wdepth_splat_device")

    def wdepth_consist_device(self, zmap, v0, nv, rel_tol, cons, viol=None, stream=None):
        """mvs_wdepth_consist_device on torch device tensors (contiguous: zmap
        float64, cons and viol uint8 (nv,H,W); viol may be None); stream-ordered."""
        maps = (int(nv), self.H, self.W)
        for name, x, size in [("zmap", zmap, 8), ("cons", cons, 1), ("viol", viol, 1)]:
            if x is not None and (x.dtype.itemsize != size or tuple(x.shape) != maps or not x.is_contiguous()):
                raise RuntimeError(f"wdepth_consist_device: {name} must be contiguous, {size}-byte elements, {maps}")
        rc = load().mvs_wdepth_consist_device(self._h, zmap.data_ptr(), int(v0), int(nv), float(rel_tol),
                                              cons.data_ptr(), viol.data_ptr() if viol is not None else None,
                                              self._stream_handle(stream))
        check(rc, self._h, "mvs_wdepth_consist_device")

    def wdepth_points_device(self, pix, zmap, v0, nv, xyz, rgb, stream=None):
        """mvs_wdepth_points_device on torch device tensors (contiguous: pix int32
        (m,3) rows (view, x, y), zmap float64 (nv,H,W), xyz float64 (m,3), rgb
        uint8 (m,3)); stream-ordered."""
        m = int(pix.shape[0])
        for name, x, size, shape in [("pix", pix, 4, (m, 3)), ("zmap", zmap, 8, (int(nv), self.H, self.W)),
                                     ("xyz", xyz, 8, (m, 3)), ("rgb", rgb, 1, (m, 3))]:
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wdepth_points_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wdepth_points_device(self._h, m, pix.data_ptr(), zmap.data_ptr(), int(v0), int(nv),
                                             xyz.data_ptr(), rgb.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wdepth_points_device")

    def wdepth_splat(self, c, nrm, ref, mask, radius=1, slope=4.0, views=None):
        """Depth and patch-index maps of a patch set (mvs_wdepth_splat, host
        pointers): zmap (nv,H,W) float64 (+inf = empty) and idmap int32 (-1)."""
        v0, nv = self._view_range(views)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        c = _c(c, np.float64).reshape(n, 3)
        nrm = _c(nrm, np.float64).reshape(n, 3)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        zmap = np.empty((nv, self.H, self.W), np.float64)
        idmap = np.empty((nv, self.H, self.W), np.int32)
        rc = load().mvs_wdepth_splat(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(mask, _u64p),
                                     int(radius), float(slope), v0, nv, _p(zmap, _dp), _p(idmap, _i32p))
        check(rc, self._h, "mvs_wdepth_splat")
        return zmap, idmap

    def wdepth_consist(self, zmap, rel_tol=0.01, views=None):
        """The cross-view consistency count of depth maps (mvs_wdepth_consist,
        host pointers) -> cons, viol (nv,H,W) uint8."""
        v0, nv = self._view_range(views)
        zmap = _c(zmap, np.float64).reshape(nv, self.H, self.W)
        cons = np.empty((nv, self.H, self.W), np.uint8)
        viol = np.empty((nv, self.H, self.W), np.uint8)
        rc = load().mvs_wdepth_consist(self._h, _p(zmap, _dp), v0, nv, float(rel_tol), _p(cons, _u8p), _p(viol, _u8p))
        check(rc, self._h, "mvs_wdepth_consist")
        return cons, viol

    def wdepth_points(self, pix, zmap, views=None):
        """World points and colours of listed pixels (mvs_wdepth_points, host
        pointers; a pixel outside the range or the image raises) -> xyz (m,3)
        float64 and rgb (m,3) uint8."""
        v0, nv = self._view_range(views)
        pix = _c(pix, np.int32).reshape(-1, 3)
        m = len(pix)
        zmap = _c(zmap, np.float64).reshape(nv, self.H, self.W)
        xyz = np.zeros((max(m, 1), 3))
        rgb = np.zeros((max(m, 1), 3), np.uint8)
        rc = load().mvs_wdepth_points(self._h, m, _p(pix, _i32p), _p(zmap, _dp), v0, nv, _p(xyz, _dp), _p(rgb, _u8p))
        check(rc, self._h, "mvs_wdepth_points")
        return xyz[:m], rgb[:m]

    def depth_maps(self, patches, radius=1, slope=4.0, views=None, rel_tol=0.01, min_consistent=2, max_violations=0,
                   timer=None):
        """Per-view depth and normal maps of a warped patch set and the dense
        cloud fused from them (the definitions are in include/mvs_amd.h).
        `patches` is the dict expand_warped, filter_warped or reconstruct_warped
        returns; it needs c, nrm, ref and mask.  views: None (every view) or
        (v0, nv).  The maps are splatted (wdepth_splat_device), the other views
        that agree with or see through each pixel are counted
        (wdepth_consist_device), and a pixel (v, q) is fused when id >= 0,
        ref[id] = v, cons >= min_consistent and viol <= max_violations: the ref
        rule emits a surface point once, in its patch's reference view.  The
        fused points and colours come from wdepth_points_device; selection and
        gathers are torch indexing on the device.  Everything runs on the
        context's torch side stream.

        Returns a dict of numpy arrays: z (nv,H,W) float64 (+inf = empty), id
        int32 (-1), cons and viol uint8, normal (nv,H,W,3) float64 (nan where
        empty), and the fused cloud points (m,3), normals (m,3), colors (m,3)
        uint8 and pix (m,3) int32 rows (view, x, y) in the maps' order.
        timer: an optional callable timer(phase, 0) called on the chain's stream
        before each phase ("splat", "consist", "select", "points") and with
        phase "end" after the last."""
        import torch
        for k in ("c", "nrm", "ref", "mask"):
            if k not in patches:
                raise RuntimeError(f"depth_maps: patches has no '{k}'")
        v0, nv = self._view_range(views)
        ref0 = _c(patches["ref"], np.int32).reshape(-1)
        n = len(ref0)
        c0 = _c(patches["c"], np.float64).reshape(n, 3)
        n0 = _c(patches["nrm"], np.float64).reshape(n, 3)
        m0 = _c(patches["mask"], np.uint64).reshape(n, self.words)
        dev = torch.device(f"cuda:{self.device}")
        st = self._side_stream()
        sh = st.cuda_stream
        tick = timer if timer is not None else (lambda phase, k: None)
        H, W = self.H, self.W
        with torch.cuda.stream(st):
            c, nrm, ref = (torch.from_numpy(x).to(dev) for x in (c0, n0, ref0))
            mask = torch.from_numpy(m0.view(np.int64)).to(dev)
            z = torch.empty((nv, H, W), dtype=torch.float64, device=dev)
            idm = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
            cons = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            tick("splat", 0)
            self.wdepth_splat_device(c, nrm, ref, mask, radius, slope, v0, nv, z, idm, stream=sh)
            tick("consist", 0)
            self.wdepth_consist_device(z, v0, nv, rel_tol, cons, viol, stream=sh)
            tick("select", 0)
            drawn = idm >= 0
            row = idm.clamp(min=0).long()
            if n:
                owner = ref[row.reshape(-1)].reshape(nv, H, W)
                normal = torch.where(drawn.unsqueeze(-1), nrm[row.reshape(-1)].reshape(nv, H, W, 3),
                                     torch.full((), float("nan"), dtype=torch.float64, device=dev))
            else:
                owner = torch.full((nv, H, W), -1, dtype=torch.int32, device=dev)
                normal = torch.full((nv, H, W, 3), float("nan"), dtype=torch.float64, device=dev)
            here = torch.arange(v0, v0 + nv, dtype=torch.int32, device=dev).reshape(nv, 1, 1)
            sel = drawn & (owner == here) & (cons >= int(min_consistent)) & (viol <= int(max_violations))
            at = sel.nonzero()                                   # (view of the range, row, column), in the maps' order
            pix = torch.stack([at[:, 0] + v0, at[:, 2], at[:, 1]], 1).to(torch.int32).contiguous()
            m = int(pix.shape[0])
            xyz = torch.empty((m, 3), dtype=torch.float64, device=dev)
            rgb = torch.empty((m, 3), dtype=torch.uint8, device=dev)
            tick("points", 0)
            self.wdepth_points_device(pix, z, v0, nv, xyz, rgb, stream=sh)
            normals = normal[at[:, 0], at[:, 1], at[:, 2]]
            tick("end", 0)
            out = {"z": z.cpu().numpy(), "id": idm.cpu().numpy(), "cons": cons.cpu().numpy(),
                   "viol": viol.cpu().numpy(), "normal": normal.cpu().numpy(), "points": xyz.cpu().numpy(),
                   "normals": normals.cpu().numpy().reshape(m, 3), "colors": rgb.cpu().numpy(),
                   "pix": pix.cpu().numpy()}
        st.synchronize()
        return out

    # the default schedule of densify_depth: (step, kd, ka, step_scale) per sweep
    DENSIFY_SCHEDULE = tuple((st, 1, 1, 1.0 if k < 4 else 0.5)
                             for k, st in enumerate((1, 3, 1, 5, 1, 3, 1, 1, 1, 1, 1, 1)))
    DENSIFY_ASTEP = math.radians(8)
    DENSIFY_DEPTH_PX = 1.0

    @staticmethod
    def wprop_hypotheses(kd, ka):
        """HY = 5 + (2 kd + 1)(2 ka + 1)^2: the hypotheses of a pixel in one sweep."""
        return 5 + (2 * int(kd) + 1) * (2 * int(ka) + 1) ** 2

    def wprop_view_lists(self, tv=4, min_axis_cos=0.5, views=None):
        """The view lists a sweep is fed -> (nv, tv) int32: the rows of
        seed_view_pairs(rproj(), tv, min_axis_cos) grouped by their first view
        (in that order) and padded with -1: one rule for neighbour views in the
        whole warped family.  views: None (every view) or (v0, nv)."""
        v0, nv = self._view_range(views)
        return wprop_view_lists(self.rproj(), tv, min_axis_cos, v0, nv)

    def _wprop_lists(self, lists, nv):
        lists = _c(lists, np.int32)
        if lists.ndim != 2 or lists.shape[0] != nv or not 1 <= lists.shape[1] <= 32:
            raise RuntimeError(f"wprop_sweep: lists must be ({nv}, tv) with tv in 1..32")
        return lists

    def wprop_sweep_device(self, zmap, nmap, lists, v0, nv, z_out, n_out, score, best, scores=None, wid=5,
                           min_cos=0.3, min_ncc=0.7, top_k=2, step=1, kd=1, ka=1, astep=math.radians(8),
                           depth_px=1.0, step_scale=1.0, stream=None):
        """mvs_wprop_sweep_device on torch device tensors (contiguous: zmap,
        z_out, score float64 (nv,H,W), nmap, n_out float64 (nv,H,W,3), best int32
        (nv,H,W), scores float64 (nv,H,W,HY) or None; every output written whole);
        lists is a host int32 array (nv, tv).  Stream-ordered."""
        nv = int(nv)
        lists = self._wprop_lists(lists, nv)
        maps = (nv, self.H, self.W)
        hy = self.wprop_hypotheses(kd, ka)
        for name, x, size, shape in [("zmap", zmap, 8, maps), ("nmap", nmap, 8, maps + (3,)), ("z_out", z_out, 8, maps),
                                     ("n_out", n_out, 8, maps + (3,)), ("score", score, 8, maps),
                                     ("best", best, 4, maps), ("scores", scores, 8, maps + (hy,))]:
            if x is None and name == "scores":
                continue
            if x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous():
                raise RuntimeError(f"wprop_sweep_device: {name} must be contiguous, {size}-byte elements, {shape}")
        rc = load().mvs_wprop_sweep_device(self._h, int(v0), nv, zmap.data_ptr(), nmap.data_ptr(), _p(lists, _i32p),
                                           lists.shape[1], int(wid), float(min_cos), float(min_ncc), int(top_k),
                                           int(step), int(kd), int(ka), float(astep), float(depth_px),
                                           float(step_scale), z_out.data_ptr(), n_out.data_ptr(), score.data_ptr(),
                                           best.data_ptr(), scores.data_ptr() if scores is not None else None,
                                           self._stream_handle(stream))
        check(rc, self._h, "mvs_wprop_sweep_device")

    def wprop_sweep(self, zmap, nmap, lists, views=None, wid=5, min_cos=0.3, min_ncc=0.7, top_k=2, step=1, kd=1, ka=1,
                    astep=math.radians(8), depth_px=1.0, step_scale=1.0, want_scores=False):
        """One propagation sweep on numpy maps (mvs_wprop_sweep, host pointers)
        -> dict z (nv,H,W), normal (nv,H,W,3), score, best int32 and, with
        want_scores, scores (nv,H,W,HY)."""
        v0, nv = self._view_range(views)
        lists = self._wprop_lists(lists, nv)
        maps = (nv, self.H, self.W)
        zmap = _c(zmap, np.float64).reshape(maps)
        nmap = _c(nmap, np.float64).reshape(maps + (3,))
        z = np.empty(maps)
        n = np.empty(maps + (3,))
        score = np.empty(maps)
        best = np.empty(maps, np.int32)
        scores = np.empty(maps + (self.wprop_hypotheses(kd, ka),)) if want_scores else None
        rc = load().mvs_wprop_sweep(self._h, v0, nv, _p(zmap, _dp), _p(nmap, _dp), _p(lists, _i32p), lists.shape[1],
                                    int(wid), float(min_cos), float(min_ncc), int(top_k), int(step), int(kd), int(ka),
                                    float(astep), float(depth_px), float(step_scale), _p(z, _dp), _p(n, _dp),
                                    _p(score, _dp), _p(best, _i32p), _p(scores, _dp) if want_scores else None)
        check(rc, self._h, "mvs_wprop_sweep")
        out = {"z": z, "normal": n, "score": score, "best": best}
        if want_scores:
            out["scores"] = scores
        return out

    def densify_depth(self, maps, views=None, lists=None, tv=4, wid=5, min_ncc=0.7, min_cos=0.3, top_k=2,
                      schedule=None, rel_tol=0.01, min_consistent=2, max_violations=0, timer=None):
        """Densify the maps depth_maps returns (`maps` needs z and normal) by
        per-pixel plane propagation (mvs_wprop_sweep, include/mvs_amd.h) and fuse
        them.  Two sets of device maps are ping-ponged through the sweeps of
        `schedule`, a list of (step, kd, ka, step_scale) (default
        DENSIFY_SCHEDULE: 12 sweeps, steps 1,3,1,5,1,3,1,1,1,1,1,1, a 3 x 3 x 3
        grid of 1 px in depth and 8 degrees, halved after the fourth sweep);
        lists: the (nv, tv) view lists (default wprop_view_lists(tv)).  Then
        wdepth_consist_device counts the agreeing views and a pixel is fused
        when it holds a depth, cons >= min_consistent and viol <=
        max_violations.  There is no ref rule here -- a densified pixel has no
        owner patch -- so a surface point is emitted in every view that holds
        it; the cloud is not de-duplicated across views.  Everything runs on
        the context's torch side stream.

        Returns a dict of numpy arrays: z (nv,H,W) float64 (+inf = empty),
        normal (nv,H,W,3) (nan where empty), score float64, best int32 (of the
        last sweep), cons and viol uint8, the fused cloud points (m,3), normals
        (m,3), colors (m,3) uint8, pix (m,3) int32 rows (view, x, y) in the
        maps' order, and history (sweeps, 2) int64: per sweep the pixels that
        hold a depth after it and the pixels whose best > 0 (gathered on the
        device, copied once at the end).  timer: an optional callable
        timer(phase, k) called on the chain's stream before sweep k ("sweep"),
        before "consist", "select" and "points", and with "end" after the last."""
        import torch
        v0, nv = self._view_range(views)
        H, W = self.H, self.W
        if lists is None:
            lists = self.wprop_view_lists(tv, views=(v0, nv))
        lists = self._wprop_lists(lists, nv)
        schedule = list(self.DENSIFY_SCHEDULE if schedule is None else schedule)
        z0 = _c(maps["z"], np.float64).reshape(nv, H, W)
        n0 = _c(maps["normal"], np.float64).reshape(nv, H, W, 3)
        dev = torch.device(f"cuda:{self.device}")
        st = self._side_stream()
        sh = st.cuda_stream
        tick = timer if timer is not None else (lambda phase, k: None)
        with torch.cuda.stream(st):
            z = [torch.from_numpy(z0).to(dev), torch.empty((nv, H, W), dtype=torch.float64, device=dev)]
            nm = [torch.from_numpy(n0).to(dev), torch.empty((nv, H, W, 3), dtype=torch.float64, device=dev)]
            score = torch.full((nv, H, W), float("nan"), dtype=torch.float64, device=dev)
            best = torch.full((nv, H, W), -1, dtype=torch.int32, device=dev)
            hist = torch.zeros((max(len(schedule), 1), 2), dtype=torch.int64, device=dev)
            cur = 0
            for k, (step, kd, ka, scale) in enumerate(schedule):
                tick("sweep", k)
                self.wprop_sweep_device(z[cur], nm[cur], lists, v0, nv, z[1 - cur], nm[1 - cur], score, best, None,
                                        wid, min_cos, min_ncc, top_k, step, kd, ka, self.DENSIFY_ASTEP,
                                        self.DENSIFY_DEPTH_PX, scale, stream=sh)
                cur = 1 - cur
                hist[k, 0] = (best >= 0).sum()
                hist[k, 1] = (best > 0).sum()
            zf, nf = z[cur], nm[cur]
            if not schedule:   # no sweep: the maps as given
                zf = torch.where(torch.isfinite(zf) & (zf > 0), zf, torch.full((), float("inf"), dtype=torch.float64,
                                                                               device=dev))
            cons = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            tick("consist", 0)
            self.wdepth_consist_device(zf, v0, nv, rel_tol, cons, viol, stream=sh)
            tick("select", 0)
            sel = torch.isfinite(zf) & (zf > 0) & (cons >= int(min_consistent)) & (viol <= int(max_violations))
            at = sel.nonzero()                                   # (view of the range, row, column), in the maps' order
            pix = torch.stack([at[:, 0] + v0, at[:, 2], at[:, 1]], 1).to(torch.int32).contiguous()
            m = int(pix.shape[0])
            xyz = torch.empty((m, 3), dtype=torch.float64, device=dev)
            rgb = torch.empty((m, 3), dtype=torch.uint8, device=dev)
            tick("points", 0)
            self.wdepth_points_device(pix, zf, v0, nv, xyz, rgb, stream=sh)
            normals = nf[at[:, 0], at[:, 1], at[:, 2]]
            tick("end", 0)
            out = {"z": zf.cpu().numpy(), "normal": nf.cpu().numpy(), "score": score.cpu().numpy(),
                   "best": best.cpu().numpy(), "cons": cons.cpu().numpy(), "viol": viol.cpu().numpy(),
                   "points": xyz.cpu().numpy(), "normals": normals.cpu().numpy().reshape(m, 3),
                   "colors": rgb.cpu().numpy(), "pix": pix.cpu().numpy(),
                   "history": hist.cpu().numpy()[:len(schedule)]}
        st.synchronize()
        return out

    @staticmethod
    def _lattice(dims, origin):
        """(nx, ny, nz) as ints, the lattice's shape (nz+1, ny+1, nx+1) and origin as 3 contiguous doubles."""
        nx, ny, nz = (int(d) for d in dims)
        origin = _c(origin, np.float64).reshape(-1)
        if len(origin) != 3:
            raise RuntimeError("origin must hold 3 values")
        return (nx, ny, nz), (nz + 1, ny + 1, nx + 1), origin

    def wtsdf_integrate_device(self, zmap, v0, nv, dims, origin, voxel, trunc, min_weight, tsdf, weight, rgb, cnt,
                               stream=None):
        """mvs_wtsdf_integrate_device on torch device tensors (contiguous: zmap
        float64 (nv,H,W); over the lattice (nz+1,ny+1,nx+1) of dims = (nx, ny,
        nz): tsdf float64, weight int32, rgb uint8 (..,3), cnt uint8, all written
        whole); origin: 3 host doubles; stream-ordered."""
        (nx, ny, nz), shape, origin = self._lattice(dims, origin)
        for name, x, size, shp in [("zmap", zmap, 8, (int(nv), self.H, self.W)), ("tsdf", tsdf, 8, shape),
                                   ("weight", weight, 4, shape), ("rgb", rgb, 1, shape + (3,)),
                                   ("cnt", cnt, 1, shape)]:
            if x.dtype.itemsize != size or tuple(x.shape) != shp or not x.is_contiguous():
                raise RuntimeError(f"wtsdf_integrate_device: {name} must be contiguous, {size}-byte elements, {shp}")
        rc = load().mvs_wtsdf_integrate_device(self._h, zmap.data_ptr(), int(v0), int(nv), nx, ny, nz, _p(origin, _dp),
                                               float(voxel), float(trunc), int(min_weight), tsdf.data_ptr(),
                                               weight.data_ptr(), rgb.data_ptr(), cnt.data_ptr(),
                                               self._stream_handle(stream))
        check(rc, self._h, "mvs_wtsdf_integrate_device")

    def wtsdf_integrate(self, zmap, dims, origin, voxel, trunc, min_weight=1, views=None):
        """The signed-distance lattice of depth maps (mvs_wtsdf_integrate, host
        pointers) -> tsdf (nz+1,ny+1,nx+1) float64 (nan below min_weight), weight
        int32, rgb (..,3) uint8, cnt uint8."""
        v0, nv = self._view_range(views)
        (nx, ny, nz), shape, origin = self._lattice(dims, origin)
        if min(nx, ny, nz) < 0 or (nx + 1) * (ny + 1) * (nz + 1) > 1 << 27:
            raise RuntimeError("wtsdf_integrate: more than 2^27 lattice points")
        zmap = _c(zmap, np.float64).reshape(nv, self.H, self.W)
        tsdf = np.empty(shape, np.float64)
        weight = np.empty(shape, np.int32)
        rgb = np.empty(shape + (3,), np.uint8)
        cnt = np.empty(shape, np.uint8)
        rc = load().mvs_wtsdf_integrate(self._h, _p(zmap, _dp), v0, nv, nx, ny, nz, _p(origin, _dp), float(voxel),
                                        float(trunc), int(min_weight), _p(tsdf, _dp), _p(weight, _i32p),
                                        _p(rgb, _u8p), _p(cnt, _u8p))
        check(rc, self._h, "mvs_wtsdf_integrate")
        return tsdf, weight, rgb, cnt

    def wmesh_extract_device(self, dims, origin, voxel, tsdf, rgb, cnt, vert, vcol, tri, total, stream=None):
        """mvs_wmesh_extract_device on torch device tensors (contiguous: over the
        lattice (nz+1,ny+1,nx+1) of dims: tsdf float64, rgb uint8 (..,3), cnt
        uint8; vert float64 (cap_v,3), vcol uint8 (cap_v,3), tri int32 (cap_t,3),
        each may be None for a cap of 0 (vert and vcol together); total int64
        (2,): vertices, triangles); stream-ordered."""
        (nx, ny, nz), shape, origin = self._lattice(dims, origin)
        if (vert is None) != (vcol is None):
            raise RuntimeError("wmesh_extract_device: vert and vcol come together")
        cap_v = 0 if vert is None else int(vert.shape[0])
        cap_t = 0 if tri is None else int(tri.shape[0])
        for name, x, size, shp in [("tsdf", tsdf, 8, shape), ("rgb", rgb, 1, shape + (3,)), ("cnt", cnt, 1, shape),
                                   ("vert", vert, 8, (cap_v, 3)), ("vcol", vcol, 1, (cap_v, 3)),
                                   ("tri", tri, 4, (cap_t, 3)), ("total", total, 8, (2,))]:
            if x is not None and (x.dtype.itemsize != size or tuple(x.shape) != shp or not x.is_contiguous()):
                raise RuntimeError(f"wmesh_extract_device: {name} must be contiguous, {size}-byte elements, {shp}")
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        rc = load().mvs_wmesh_extract_device(self._h, nx, ny, nz, _p(origin, _dp), float(voxel), tsdf.data_ptr(),
                                             rgb.data_ptr(), cnt.data_ptr(), cap_v, cap_t, ptr(vert), ptr(vcol),
                                             ptr(tri), total.data_ptr(), self._stream_handle(stream))
        check(rc, self._h, "mvs_wmesh_extract_device")

    def wmesh_extract(self, tsdf, rgb, cnt, origin, voxel, cap_v=None, cap_t=None):
        """Marching tetrahedra over a lattice (mvs_wmesh_extract, host pointers):
        tsdf (nz+1,ny+1,nx+1) float64, rgb (..,3) uint8, cnt uint8 -> vertices
        (n,3) float64, colors (n,3) uint8, faces (m,3) int32 and total (2,) int64,
        the full counts.  cap_v, cap_t None: a counting call first, then the exact
        sizes; given: the first min(cap, total) entries."""
        tsdf = _c(tsdf, np.float64)
        if tsdf.ndim != 3 or min(tsdf.shape) < 2:
            raise RuntimeError("wmesh_extract: tsdf must be (nz+1, ny+1, nx+1) with at least 2 points per axis")
        nz, ny, nx = (n - 1 for n in tsdf.shape)
        _, shape, origin = self._lattice((nx, ny, nz), origin)
        rgb = _c(rgb, np.uint8).reshape(shape + (3,))
        cnt = _c(cnt, np.uint8).reshape(shape)
        total = np.zeros(2, np.int64)

        def call(cv, ct):
            vert = np.zeros((max(cv, 1), 3))
            vcol = np.zeros((max(cv, 1), 3), np.uint8)
            tri = np.zeros((max(ct, 1), 3), np.int32)
            rc = load().mvs_wmesh_extract(self._h, nx, ny, nz, _p(origin, _dp), float(voxel), _p(tsdf, _dp),
                                          _p(rgb, _u8p), _p(cnt, _u8p), cv, ct, _p(vert, _dp), _p(vcol, _u8p),
                                          _p(tri, _i32p), _p(total, _i64p))
            check(rc, self._h, "mvs_wmesh_extract")
            nv_, nt_ = min(cv, int(total[0])), min(ct, int(total[1]))
            return vert[:nv_], vcol[:nv_], tri[:nt_]

        if cap_v is None or cap_t is None:
            call(0, 0)
            cap_v = int(total[0]) if cap_v is None else cap_v
            cap_t = int(total[1]) if cap_t is None else cap_t
        vert, vcol, tri = call(int(cap_v), int(cap_t))
        return vert, vcol, tri, total

    def mesh_depth(self, maps, views=None, bounds=None, resolution=256, trunc_voxels=3.0, min_weight=1, rel_tol=0.01,
                   min_consistent=2, max_violations=0, timer=None):
        """A triangle mesh from the depth maps that depth_maps or densify_depth
        returns (`maps` needs z; the definitions are in include/mvs_amd.h).
        wdepth_consist_device counts the agreeing views of the maps as given;
        a pixel that fails the fusion rule of those calls (a finite depth, cons
        >= min_consistent, viol <= max_violations) is set to +inf, so an
        unconfirmed depth neither votes nor carves.  The lattice (mesh_grid):
        bounds = (lo, hi) as given with voxel = its longest side / resolution;
        by default the per-axis 0.5 to 99.5 percentile box of maps["points"],
        which gives the voxel the same way and is then grown by 2 trunc; trunc =
        trunc_voxels voxel.  wtsdf_integrate_device fuses the maps and
        wmesh_extract_device meshes the lattice, once to count and once to
        write.  Everything runs on the context's torch side stream.

        Returns a dict of numpy arrays: vertices (n,3) float64, colors (n,3)
        uint8, faces (m,3) int32, tsdf (nz+1,ny+1,nx+1) float64 (nan = unseen),
        weight int32, origin (3,) float64, voxel (a float) and dims (3,) int32
        (nx, ny, nz).  timer: an optional callable timer(phase, 0) called on the
        chain's stream before each phase ("consist", "mask", "integrate",
        "count", "extract") and with "end" after the last."""
        import torch
        if "z" not in maps:
            raise RuntimeError("mesh_depth: maps has no 'z'")
        v0, nv = self._view_range(views)
        H, W = self.H, self.W
        z0 = _c(maps["z"], np.float64).reshape(nv, H, W)
        origin, voxel, dims, trunc = mesh_grid(maps.get("points"), bounds, resolution, trunc_voxels)
        nx, ny, nz = dims
        shape = (nz + 1, ny + 1, nx + 1)
        if shape[0] * shape[1] * shape[2] > 1 << 27:
            raise RuntimeError("mesh_depth: more than 2^27 lattice points; lower the resolution")
        dev = torch.device(f"cuda:{self.device}")
        st = self._side_stream()
        sh = st.cuda_stream
        tick = timer if timer is not None else (lambda phase, k: None)
        with torch.cuda.stream(st):
            z = torch.from_numpy(z0).to(dev)
            cons = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            tick("consist", 0)
            self.wdepth_consist_device(z, v0, nv, rel_tol, cons, viol, stream=sh)
            tick("mask", 0)
            keep = torch.isfinite(z) & (cons >= int(min_consistent)) & (viol <= int(max_violations))
            z = torch.where(keep, z, torch.full((), float("inf"), dtype=torch.float64, device=dev)).contiguous()
            tsdf = torch.empty(shape, dtype=torch.float64, device=dev)
            weight = torch.empty(shape, dtype=torch.int32, device=dev)
            rgb = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
            cnt = torch.empty(shape, dtype=torch.uint8, device=dev)
            total = torch.zeros(2, dtype=torch.int64, device=dev)
            tick("integrate", 0)
            self.wtsdf_integrate_device(z, v0, nv, dims, origin, voxel, trunc, min_weight, tsdf, weight, rgb, cnt,
                                        stream=sh)
            tick("count", 0)
            self.wmesh_extract_device(dims, origin, voxel, tsdf, rgb, cnt, None, None, None, total, stream=sh)
            n, m = (int(x) for x in total.cpu().numpy())
            if n >= 1 << 31 or m >= 1 << 31:
                raise RuntimeError("mesh_depth: 2^31 or more vertices or triangles; lower the resolution")
            vert = torch.empty((n, 3), dtype=torch.float64, device=dev)
            vcol = torch.empty((n, 3), dtype=torch.uint8, device=dev)
            tri = torch.empty((m, 3), dtype=torch.int32, device=dev)
            tick("extract", 0)
            if n or m:
                self.wmesh_extract_device(dims, origin, voxel, tsdf, rgb, cnt, vert, vcol, tri, total, stream=sh)
            tick("end", 0)
            out = {"vertices": vert.cpu().numpy(), "colors": vcol.cpu().numpy(), "faces": tri.cpu().numpy(),
                   "tsdf": tsdf.cpu().numpy(), "weight": weight.cpu().numpy(), "origin": origin, "voxel": voxel,
                   "dims": np.array(dims, np.int32)}
        st.synchronize()
        return out

    def pack_accepted(self, offset, count, mask, vlb, out, stream=None, c=None):
        """mvs_pack_accepted: the accepted candidates (count >= vlb) of a scored
        slice as exchange rows of out (device int64 tensor (cap + 1, width):
        row 0 = [accepted, n, 0...], then rows
        [offset + i, mask words(, x y z bits with c)]: each 8,192-candidate
        chunk in index order, the chunks in any order -- sort_rows() orders
        them); c = the
        slice's (n, 3) float64 centres or None (width 1 + words [+ 3]);
        stream-ordered, no host sync.  count None: mask is score_device_rec's
        records and |V| their popcount."""
        n = int(count.numel()) if count is not None else int(mask.shape[0])
        # the kernel indexes rows at a fixed pitch: strided views would give wrong rows
        if count is None and (mask.dtype.itemsize != 8 or mask.dim() != 2 or mask.shape[1] != self.words + 1
                              or not mask.is_contiguous()):
            raise RuntimeError("pack_accepted: records must be contiguous int64 (n, words + 1)")
        if count is not None and (count.dtype.itemsize != 4 or not count.is_contiguous()
                                  or mask.dtype.itemsize != 8 or tuple(mask.shape) != (n, self.words)
                                  or not mask.is_contiguous()):
            raise RuntimeError(f"pack_accepted: count must be contiguous int32 (n,) and mask contiguous "
                               f"int64 (n, {self.words})")
        cap = int(out.shape[0]) - 1
        width = 1 + self.words + (3 if c is not None else 0)
        if out.dtype.itemsize != 8 or out.shape[1] != width or not out.is_contiguous():
            raise RuntimeError(f"pack_accepted: out must be contiguous int64 (cap + 1, {width})")
        if c is not None and (c.dtype.itemsize != 8 or tuple(c.shape) != (n, 3) or not c.is_contiguous()):
            raise RuntimeError("pack_accepted: c must be contiguous float64 (n, 3)")
        rc = load().mvs_pack_accepted(self._h, n, int(offset), count.data_ptr() if count is not None else None,
                                      mask.data_ptr(),
                                      c.data_ptr() if c is not None else None,
                                      int(vlb), cap, out.data_ptr(),
                                      stream if stream is not None else None)
        check(rc, self._h, "mvs_pack_accepted")

    def set_scorer_grid(self, workgroups=0):
        """Hold the persistent scorers to `workgroups` workgroups (0: default,
        two per CU): the grid for a CU-masked scoring stream."""
        check(load().mvs_set_scorer_grid(self._h, int(workgroups)), self._h, "mvs_set_scorer_grid")

    def harris_points(self, view):
        """getHarrisPoints(imgs[view]) (HarrisFeatures.py:135-161) on the GPU:
        int32 (n, 2) [col, row] in np.where's row-major order."""
        lib = load()
        n = ctypes.c_int64(0)
        check(lib.mvs_harris_points(self._h, int(view), None, 0, ctypes.byref(n)), self._h,
              "mvs_harris_points")
        out = np.empty((max(n.value, 1), 2), np.int32)
        check(lib.mvs_harris_points(self._h, int(view), _p(out, _i32p), n.value, ctypes.byref(n)),
              self._h, "mvs_harris_points")
        return out[:n.value]

    def match_two_sided(self, view_a, pts_a, view_b, pts_b, thr=0.5, wid=5):
        """MatchTwoSided over getDescFeatures windows (HarrisFeatures.py:15-67) on the
        GPU; pts_* [row, col] inside getDescFeatures' bounds.
        Returns (m12, best12, best21) int32 (-1 = none)."""
        a = _c(pts_a, np.int32).reshape(-1, 2)
        b = _c(pts_b, np.int32).reshape(-1, 2)
        m12 = np.empty(max(len(a), 1), np.int32)
        b12 = np.empty(max(len(a), 1), np.int32)
        b21 = np.empty(max(len(b), 1), np.int32)
        check(load().mvs_match_two_sided(self._h, int(view_a), _p(a, _i32p), len(a), int(view_b),
                                         _p(b, _i32p), len(b), int(wid), float(thr), _p(m12, _i32p),
                                         _p(b12, _i32p), _p(b21, _i32p)),
              self._h, "mvs_match_two_sided")
        return m12[:len(a)], b12[:len(a)], b21[:len(b)]

    def expand_candidates(self, pc, pn, pxy, job_parent, job_view, job_di, cell_size=2,
                          scale=10.0, wid=5, min_ncc=0.7):
        """patch_expansion candidates (MVS2.py:329-369) for explicit jobs (see mvs_amd.h)."""
        pc = _c(pc, np.float64).reshape(-1, 3)
        pn = _c(pn, np.float64).reshape(-1, 3)
        pxy = _c(pxy, np.float64).reshape(-1, 2)
        jp = _c(job_parent, np.int32)
        jv = _c(job_view, np.int32)
        jd = _c(job_di, np.int32)
        n = len(jp)
        X, nX, xy = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 2))
        color = np.empty((n, 3), np.uint8)
        mask = np.empty((n, self.words), np.uint64)
        count = np.empty(n, np.int32)
        acc = np.empty(n, np.uint8)
        rc = load().mvs_expand_candidates(self._h, len(pc), _p(pc, _dp), _p(pn, _dp), _p(pxy, _dp),
                                          n, _p(jp, _i32p), _p(jv, _i32p), _p(jd, _i32p),
                                          int(cell_size), float(scale), int(wid), float(min_ncc),
                                          _p(X, _dp), _p(nX, _dp), _p(color, _u8p), _p(xy, _dp),
                                          _p(mask, _u64p), _p(count, _i32p), _p(acc, _u8p))
        check(rc, self._h, "mvs_expand_candidates")
        return X, nX, color, xy, mask, count, acc

    def stage(self, track_off, obs_view, obs_xy, cell_size=2, scale=1.0, wid=5, max_pops=100000,
              filter_outliers=False):
        """DensePointsWithMVS2 minus IO; returns (initial N0x6, all Nx6, stats dict).
        filter_outliers: run CellTable.filter_out_outlier (MVS2.py:132-158) before
        the reconstruction, as if MVS2.py:281 were enabled."""
        lib = load()
        track_off, obs_view, obs_xy = _tracks(track_off, obs_view, obs_xy)
        self.set_stage_options(filter_outliers)
        res = _vp()
        rc = lib.mvs_stage_run(self._h, len(track_off) - 1, _p(track_off, _i64p),
                               _p(obs_view, _i32p), _p(obs_xy, _fp), int(cell_size), float(scale),
                               int(wid), int(max_pops), ctypes.byref(res))
        check(rc, self._h, "mvs_stage_run")
        return _take_result(res, self._h)

    def set_stage_options(self, filter_outliers=False):
        """Options of the stage runs that follow (mvs_stage_set_options)."""
        flags = MVS_STAGE_FILTER_OUTLIERS if filter_outliers else 0
        check(load().mvs_stage_set_options(self._h, flags), self._h, "mvs_stage_set_options")

    def stage_begin(self, track_off, obs_view, obs_xy, cell_size=2, scale=1.0, wid=5,
                    max_pops=100000, rank=0, world=1):
        """The stage in steps (mvs_stage_begin ...); see parallel.stage_sharded."""
        return Stage(self, track_off, obs_view, obs_xy, cell_size, scale, wid, max_pops, rank, world)


STAGE_STATS = ["pops", "tests", "accepts", "queue_left", "scored", "sweeps", "seed_candidates",
               "exact_hits"]
STAGE_TIMES = ["seed_s", "commit_s", "gpu_sweeps_s", "copy_back_s", "output_s", "total_s"]
# + "rows_to_host_s": the copy of the PLY rows from HBM into the numpy arrays


def _tracks(track_off, obs_view, obs_xy):
    return (_c(track_off, np.int64), _c(obs_view, np.int32),
            _c(obs_xy, np.float32).reshape(-1, 2))


def _take_result(res, h):
    """Copy an mvs_stage_result out and free it -> (initial, all, stats)."""
    import time
    lib = load()
    try:
        t0 = time.perf_counter()
        out = []
        for which in (0, 1):
            n = lib.mvs_stage_count(res, which)
            rows = np.empty((n, 6))
            if n:
                check(lib.mvs_stage_rows(res, which, _p(rows, _dp)), h, "mvs_stage_rows")
            out.append(rows)
        t_rows = time.perf_counter() - t0
        st = np.empty(8, np.int64)
        check(lib.mvs_stage_stats(res, _p(st, _i64p)), h, "mvs_stage_stats")
        tm = np.empty(6)
        check(lib.mvs_stage_times(res, _p(tm, _dp)), h, "mvs_stage_times")
        fl = np.empty(2, np.int64)
        check(lib.mvs_stage_filter_stats(res, _p(fl, _i64p)), h, "mvs_stage_filter_stats")
    finally:
        lib.mvs_stage_free(res)
    stats = dict(zip(STAGE_STATS, (int(x) for x in st)))
    stats["times"] = dict(zip(STAGE_TIMES, (float(x) for x in tm)))
    stats["times"]["rows_to_host_s"] = t_rows
    stats["outliers_removed"], stats["outlier_lines"] = int(fl[0]), int(fl[1])
    return out[0], out[1], stats


class Stage:
    """One rank's view of a stepped stage run (include/mvs_amd.h, mvs_stage_*)."""

    def __init__(self, ctx, track_off, obs_view, obs_xy, cell_size, scale, wid, max_pops, rank,
                 world):
        lib = load()
        self.ctx = ctx
        self.rank, self.world = int(rank), int(world)
        self._tr = _tracks(track_off, obs_view, obs_xy)
        h = _vp()
        rc = lib.mvs_stage_begin(ctx.handle, len(self._tr[0]) - 1, _p(self._tr[0], _i64p),
                                 _p(self._tr[1], _i32p), _p(self._tr[2], _fp), int(cell_size),
                                 float(scale), int(wid), int(max_pops), self.rank, self.world,
                                 ctypes.byref(h))
        check(rc, ctx.handle, "mvs_stage_begin")
        self._st = h
        self.width = lib.mvs_stage_record_width(h)
        ctx._stages.add(self)   # closed before their context (MvsContext.close)

    def plan(self):
        """Commit and plan the next sweep -> its job count (0: finished)."""
        n = load().mvs_stage_plan(self._st)
        if n < 0:
            check(int(n), self.ctx.handle, "mvs_stage_plan")
        return int(n)

    def slice_max(self, nj):
        return -(-nj // self.world)

    def score_slice(self, out=None):
        """Score this rank's slice; out = device int64 tensor (slice_max, width) when world > 1."""
        ptr = out.data_ptr() if out is not None else None
        check(load().mvs_stage_score_slice(self._st, ptr), self.ctx.handle, "mvs_stage_score_slice")

    def ingest(self, gathered=None):
        """gathered = device int64 tensor (world, slice_max, width) when world > 1.

        The library reads it on its own stream, which does not wait for torch's:
        the producer (all-gather, torch.stack) is synchronised here first."""
        if gathered is not None and getattr(gathered, "is_cuda", False):
            import torch
            torch.cuda.current_stream(gathered.device).synchronize()
        ptr = gathered.data_ptr() if gathered is not None else None
        check(load().mvs_stage_ingest(self._st, ptr), self.ctx.handle, "mvs_stage_ingest")

    def finish(self):
        res = _vp()
        check(load().mvs_stage_finish(self._st, ctypes.byref(res)), self.ctx.handle, "mvs_stage_finish")
        return _take_result(res, self.ctx.handle)

    def close(self):
        if self._st:
            load().mvs_stage_destroy(self._st)
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def proxy_copy(dst, src, nbytes, workgroups, stream=None):
    """Measurement only: copy nbytes between device tensors with a kernel of
    `workgroups` workgroups on `stream` (a collective's CU footprint)."""
    check(load().mvs_proxy_copy(dst.data_ptr(), src.data_ptr(), int(nbytes), int(workgroups), stream),
          None, "mvs_proxy_copy")


def ncc_windows(a, b, thr, force_exact=False, stream=None):
    """ctNcc on device window pairs (torch uint8 tensors (n, npx)); returns (ncc, pass) tensors."""
    import torch
    n, npx = a.shape
    ncc = torch.empty(n, dtype=torch.float64, device=a.device)
    ok = torch.empty(n, dtype=torch.uint8, device=a.device)
    rc = load().mvs_ncc_windows(n, npx, a.data_ptr(), b.data_ptr(), float(thr), int(force_exact),
                                ncc.data_ptr(), ok.data_ptr(), stream)
    check(rc, None, "mvs_ncc_windows")
    return ncc, ok
