"""The stage API (the stage half of csrc/mvs_engine.cpp): whole and stepped runs of the reference's dense stage."""
import ctypes

import numpy as np

from ._abi import MVS_STAGE_FILTER_OUTLIERS, _c, _dp, _fp, _i32p, _i64p, _p, _vp, check, load

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


class _StageCalls:
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
