"""The one import point of the ctypes binding of libmvs_amd.so (_abi has the no-fallback rule): MvsContext is
assembled here from its core (_context) and one class per kernel family, and every name is re-exported.  The
family modules import from _abi and _context only."""
from ._abi import (HERE, LIB_PATH, MVS_E_DIVZERO, MVS_STAGE_FILTER_OUTLIERS, SIGNATURES, _c, _dp, _fp,  # noqa: F401
                   _i32p, _i64p, _p, _u8p, _u64p, _vp, check, last_error, load)
# importing _context registers the atexit hook that closes the live contexts
from ._context import (_LIVE, _Core, _close_live_contexts, filter_outliers, ncc_windows, proxy_copy,  # noqa: F401
                       rodrigues_roundtrip, seed_view_pairs, sfm_pair, stream_retiring, triangulate)
from ._stage import STAGE_STATS, STAGE_TIMES, Stage, _StageCalls, _take_result, _tracks  # noqa: F401
from ._warp import _Warp
from ._wdepth import _Wdepth, wprop_view_lists  # noqa: F401
from ._wexp import _Wexp
from ._wfilt import _Wfilt
from ._wmesh import _Wmesh, mesh_grid  # noqa: F401
from ._wseed import _Wseed


class MvsContext(_Core, _StageCalls, _Warp, _Wexp, _Wfilt, _Wseed, _Wdepth, _Wmesh):
    """One device-resident scene (images + cameras) on one GPU.

    imgs: (V,H,W,3) uint8 RGB (main.py:17-18 convention) or a list of such
    frames; K, R: (V,3,3); t: (V,3) or (V,3,1).
    """
