"""Timing of the warped pipeline's seeding (mvs_wseed_match_device,
mvs_wpatch_color_device, MVS2.DensePointsWarped) on dinoRing: Harris features
of every view (border wid + 1 = 6), wseed_pairs(4, 0.5), epi_px 1.5, min_sin2
1e-4.  Prints one JSON line:

  features, pairs, pair_tests: the matcher's input and the (a, b) tests it runs;
  match_count_call, match_call: device-event time of a counting call (cap 0:
    count pass and scan) and of a full call (count, scan, emit), the median of
    `windows` windows of `reps` back-to-back calls on one stream after a
    warm-up, and the pair tests per second of the full call (which runs every
    test twice: 2 pair_tests over the time is the kernels' own rate);
  candidates and score_warped_ms: their number and the device time of one
    score_warped_device call over all of them (wid 5, min_ncc 0.7, min_cos 0.3);
  winners0: the candidates round 0 of expand_warped keeps;
  color_call: the colour call's device time on the final patch set;
  dense: DensePointsWarped's wall time (rounds, iterations as given) and its
    patches per iteration.

Nothing earlier exists to compare against: the figures say what is measured;
they set no target.

usage: python tools/seed_time.py [--rounds 4] [--iterations 3] [--windows 5] [--reps 5]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
DATA = os.path.join(REPO, "data", "dinoRing")


def windows_of(torch, stream, call, windows, reps):
    """Median over the windows of the device time of one call, in milliseconds."""
    with torch.cuda.stream(stream):
        for _ in range(2):
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
    return {"device_ms": round(float(np.median(per)), 4), "device_ms_min": round(float(min(per)), 4),
            "device_ms_max": round(float(max(per)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import torch
    assert torch.cuda.is_available(), "seed_time needs the GPU"
    from make_seeds import load_dino
    mvs = importlib.import_module(PKG)
    imgs, K, R, t = load_dino(DATA)
    args = types.SimpleNamespace(par_path=os.path.join(DATA, "dinoR_par.txt"))
    epi_px, min_sin2 = 1.5, 1e-4
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        out = mvs.DensePointsWarped(imgs, args, rounds=a.rounds, iterations=a.iterations, epi_px=epi_px,
                                    min_sin2=min_sin2, path=os.path.join(tmp, "warped_patches"))
        wall = time.perf_counter() - t0
    counts, ps = out["counts"], out["patches"]
    par_K, par_r, par_t = mvs.read_pars(args)
    ctx = mvs.MVS2.scene_context(imgs, par_K, par_r, par_t)
    feats = ctx.last_seed["feats"]
    pairs = ctx.wseed_pairs(4, 0.5)
    feat_off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    st = torch.cuda.Stream(dev)
    sh = st.cuda_stream
    n = counts["candidates"]
    with torch.cuda.stream(st):
        tf = torch.from_numpy(np.concatenate(feats)).to(dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        c = torch.empty((n, 3), dtype=torch.float64, device=dev)
        nrm = torch.empty((n, 3), dtype=torch.float64, device=dev)
        ref = torch.empty(n, dtype=torch.int32, device=dev)
        cand = torch.empty((n, 4), dtype=torch.int32, device=dev)
        err = torch.empty(n, dtype=torch.float64, device=dev)
        xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
        mask = torch.empty((n, ctx.words), dtype=torch.int64, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        avg = torch.empty(n, dtype=torch.float64, device=dev)
    st.synchronize()
    t_count = windows_of(torch, st, lambda: ctx.wseed_match_device(tf, feat_off, pairs, epi_px, min_sin2, None, None,
                                                                   None, None, None, total, stream=sh),
                         a.windows, a.reps)
    t_match = windows_of(torch, st, lambda: ctx.wseed_match_device(tf, feat_off, pairs, epi_px, min_sin2, c, nrm, ref,
                                                                   cand, err, total, stream=sh), a.windows, a.reps)
    assert int(total.item()) == n
    t_score = windows_of(torch, st, lambda: ctx.score_warped_device(c, nrm, ref, xy, mask, count, avg, min_ncc=0.7,
                                                                    wid=5, min_cos=0.3, stream=sh), a.windows, 1)
    m = len(ps["ref"])
    with torch.cuda.stream(st):
        pc = torch.from_numpy(np.ascontiguousarray(ps["c"])).to(dev)
        pr = torch.from_numpy(np.ascontiguousarray(ps["ref"])).to(dev)
        pm = torch.from_numpy(ps["mask"].view(np.int64)).to(dev)
        col = torch.empty((m, 3), dtype=torch.float64, device=dev)
        nv = torch.empty(m, dtype=torch.int32, device=dev)
    st.synchronize()
    t_color = windows_of(torch, st, lambda: ctx.wpatch_color_device(pc, pr, pm, col, nv, stream=sh), a.windows, 20)
    tests = counts["tests"]
    t_match["pair_tests_per_s"] = round(tests / (t_match["device_ms"] * 1e-3), 1)
    t_match["kernel_tests_per_s"] = round(2 * tests / (t_match["device_ms"] * 1e-3), 1)
    t_count["pair_tests_per_s"] = round(tests / (t_count["device_ms"] * 1e-3), 1)
    print(json.dumps({"tool": "seed_time", "scene": "dinoRing 48 x 640 x 480", "epi_px": epi_px, "min_sin2": min_sin2,
                      "features": counts["features"], "pairs": counts["pairs"], "pair_tests": tests,
                      "windows": a.windows, "reps": a.reps, "match_count_call": t_count, "match_call": t_match,
                      "candidates": n, "score_warped_ms": t_score, "winners0": counts["winners0"],
                      "color_call": dict(t_color, patches=m),
                      "dense": {"rounds": a.rounds, "iterations": a.iterations, "wall_s": round(wall, 3),
                                "patches": counts["patches"]}}))
    mvs.MVS2.clear_context_cache()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
