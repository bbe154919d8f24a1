"""Timing of the visibility-consistency filter (mvs_wfilt_front_device,
mvs_wfilt_test_device, MvsContext.filter_warped) on dinoRing.  The patch set is
the refined chain of tools/expand_time.py: 2^12 synthetic.candidates as seeds,
normal = unit vector from the centre to the reference camera, 4 rounds, wid 5,
cell 2, min_ncc 0.7, min_cos 0.3, vlb 2, two refinement levels.  Prints one
JSON line:

  front_call, test_call: device-event time of one call (median of `windows`
    windows of `reps` back-to-back calls on one stream, after a warm-up), the
    bytes the call cannot avoid (byte floor: every input row read once, every
    output written once, one 12-byte or 4-byte grid access per placement) and
    that floor over the time as a rate;
  chain: the two-pass MvsContext.filter_warped (adj_px 2, min_views 3), the
    median run of `windows` by device time from the first phase mark to the
    last: device milliseconds between the chain's phase marks (front, test,
    sync = the pass's one read, rebuild, occ), the wall time of the call, and
    the counts (patches, placements, removed per pass).

Nothing earlier exists to compare against: the figures say what is measured
and where the time goes; they set no target.

usage: python tools/filter_time.py [--n 4096] [--rounds 4] [--windows 5] [--reps 50]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
DATA = os.path.join(REPO, "data", "dinoRing")
PHASES = ("front", "test", "sync", "rebuild", "occ")


class Timer:
    """timer(phase, pass) of filter_warped: an event on the chain's stream at every mark."""

    def __init__(self, torch):
        self.torch = torch
        self.marks = []

    def __call__(self, phase, k):
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record()                       # the current stream is the chain's
        self.marks.append((phase, ev))

    def phases(self):
        self.marks[-1][1].synchronize()
        out = {k: 0.0 for k in PHASES}
        for (ph, ev), (_, ev1) in zip(self.marks[:-1], self.marks[1:]):
            out[ph] += ev.elapsed_time(ev1)
        return out, self.marks[0][1].elapsed_time(self.marks[-1][1])


def windows_of(torch, stream, call, windows, reps):
    """Median over the windows of the device time of one call, in milliseconds."""
    with torch.cuda.stream(stream):
        for _ in range(3):
            call()
        per = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / reps)
    return float(np.median(per)), float(min(per)), float(max(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import torch
    assert torch.cuda.is_available(), "filter_time needs the GPU"
    from make_seeds import load_dino
    mvs = importlib.import_module(PKG)
    imgs, K, R, t = load_dino(DATA)
    rgb = np.stack(imgs)
    c, ref = mvs.synthetic.candidates(a.n, K, R, t, seed=0)
    cell, adj_px, min_views = 2, 2.0, 3
    with mvs.MvsContext(rgb, K, R, t, device=0) as ctx:
        O = -np.einsum("vji,vj->vi", ctx.rproj(), t.reshape(-1, 3))
        nrm = O[ref] - c
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        ps = ctx.expand_warped(c, nrm, ref, a.rounds, cell_size=cell, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2,
                               refine_levels=2)
        n, V, words = len(ps["ref"]), ctx.V, ctx.words
        nci, ncj = ctx.cell_grid(cell)
        cells = V * ncj * nci
        dev = torch.device("cuda:0")
        st = torch.cuda.Stream(dev)
        with torch.cuda.stream(st):
            tc, tn, tr, ta = (torch.from_numpy(np.ascontiguousarray(ps[k])).to(dev) for k in ("c", "nrm", "ref", "avg"))
            tm = torch.from_numpy(ps["mask"].view(np.int64)).to(dev)
            front = torch.empty((V, ncj, nci), dtype=torch.int32, device=dev)
            zfront = torch.empty((V, ncj, nci), dtype=torch.float64, device=dev)
            vis = torch.empty((n, words), dtype=torch.int64, device=dev)
            conf = torch.empty(n, dtype=torch.int64, device=dev)
            keep = torch.empty(n, dtype=torch.uint8, device=dev)
        st.synchronize()
        sh = st.cuda_stream
        t_front = windows_of(torch, st, lambda: ctx.wfilt_front_device(tc, tr, tm, cell, front, zfront, stream=sh),
                             a.windows, a.reps)
        t_test = windows_of(torch, st, lambda: ctx.wfilt_test_device(tc, tn, tr, tm, ta, cell, adj_px, min_views, front,
                                                                     vis, conf, keep, stream=sh), a.windows, a.reps)
        with torch.cuda.stream(st):
            h_vis = vis.cpu().numpy().view(np.uint64)
            kept1 = int(keep.sum().item())
            taken = int((front >= 0).sum().item())
        runs = []
        for _ in range(a.windows + 1):
            tm_ = Timer(torch)
            t0 = time.perf_counter()
            out = ctx.filter_warped(ps, cell_size=cell, adj_px=adj_px, min_views=min_views, passes=2, timer=tm_)
            wall = (time.perf_counter() - t0) * 1e3
            per, total = tm_.phases()
            runs.append((total, wall, per, out["removed"], int(out["keep"].sum())))
        runs = sorted(runs[1:], key=lambda x: x[0])     # the first run warms up
        total, wall, per, removed, survivors = runs[len(runs) // 2]
    views = int(sum(bin(int(x)).count("1") for x in ps["mask"].reshape(-1))) + n    # an upper bound of the placements
    seen = int(sum(bin(int(x)).count("1") for x in h_vis.reshape(-1)))
    row_in = 24 + 4 + 8 * words
    floor_front = n * row_in + cells * 12 + views * 12
    floor_test = n * (row_in + 24 + 8) + views * 4 + n * (8 * words + 8 + 8 + 1)

    def call(t3, floor):
        return {"device_ms": round(t3[0], 5), "device_ms_min": round(t3[1], 5), "device_ms_max": round(t3[2], 5),
                "byte_floor": int(floor), "floor_gb_per_s": round(floor / (t3[0] * 1e-3) / 1e9, 2)}

    print(json.dumps({"tool": "filter_time", "scene": "dinoRing 48 x 640 x 480", "seeds": a.n, "rounds": a.rounds,
                      "patches": n, "cell_size": cell, "adj_px": adj_px, "min_views": min_views, "cells": cells,
                      "cells_taken": taken, "views_upper_bound": views, "views_seen_first_pass": seen,
                      "kept_first_pass": kept1, "windows": a.windows, "reps": a.reps,
                      "front_call": call(t_front, floor_front), "test_call": call(t_test, floor_test),
                      "chain": {"passes": 2, "removed": removed, "survivors": survivors, "device_ms": round(total, 4),
                                "device_ms_min": round(runs[0][0], 4), "device_ms_max": round(runs[-1][0], 4),
                                "wall_ms": round(wall, 3), "phase_device_ms": {k: round(v, 4) for k, v in per.items()}}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
