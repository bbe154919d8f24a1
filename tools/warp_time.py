"""Timing of the plane-warped photo test (mvs_score_warped_device, kernel
k_score_warp) on dinoRing: 2^16 synthetic.candidates, normal = unit vector from
the centre to the reference camera, min_ncc 0.7, min_cos 0.3, at wid 5 and
wid 3.  Each wid runs in a child process of its own under a time limit; the
calls are timed with device events on one stream after warm-up, over several
windows (the median window is reported, with the fastest and slowest).
Prints one JSON line:

  us_per_call, candidates_per_s, tested_pairs_per_s, samples_per_s per wid,
  plus the counts they are made of and binary64 FLOP/s at FLOP_PER_SAMPLE.

A tested pair is (valid candidate, view the kernel walks); a sample is one
window pixel of a tested pair (the kernel walks every sample of a tested pair,
border failures included).  The counts come from a numpy restatement of the
candidate and view tests, not from the kernel.

usage: python tools/warp_time.py [--n 65536] [--calls 50] [--windows 5] [--limit 240]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
DATA = os.path.join(REPO, "data", "dinoRing")
# binary64 operations per sample in k_score_warp's loop, an fma counted as 2:
# projection 9 fma, reciprocal 1 + 4 fma, 2 mul + 2 fma to pixels, 4 clamps,
# 2 fractions, bilinear 3 sub + 3 fma, sums 1 add + 2 fma
FLOP_PER_SAMPLE = 18 + 9 + 6 + 4 + 2 + 9 + 5


def workload(mvs, n, wid, min_cos):
    """Inputs and the work they stand for: (c, nrm, ref, valid candidates, tested pairs)."""
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    from make_seeds import load_dino
    imgs, K, R, t = load_dino(DATA)
    rgb = np.stack(imgs)
    V, H, W = rgb.shape[:3]
    c, ref = mvs.synthetic.candidates(n, K, R, t, seed=0)
    Rp = np.stack([mvs.rodrigues_roundtrip(r) for r in R])
    O = -np.einsum("vji,vj->vi", Rp, t.reshape(V, 3))
    nrm = O[ref] - c
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    # the candidate test: window inside the image and not constant
    p = np.einsum("nij,nj->ni", Rp[ref], c) + t.reshape(V, 3)[ref]
    x = p[:, 0] / p[:, 2] * K[ref, 0, 0] + K[ref, 0, 2]
    y = p[:, 1] / p[:, 2] * K[ref, 1, 1] + K[ref, 1, 2]
    ok = (p[:, 2] > 0) & (x >= 0) & (y >= 0)
    x0, y0 = np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64)
    ok &= (x0 - wid >= 0) & (x0 + wid <= W - 1) & (y0 - wid >= 0) & (y0 + wid <= H - 1)
    g = ((rgb[..., 0].astype(np.uint32) * 1868 + rgb[..., 1].astype(np.uint32) * 9617 +
          rgb[..., 2].astype(np.uint32) * 4899 + 8192) >> 14).astype(np.uint8)
    dy, dx = np.mgrid[-wid:wid + 1, -wid:wid + 1]
    yy = np.clip(y0[:, None] + dy.ravel()[None], 0, H - 1)
    xx = np.clip(x0[:, None] + dx.ravel()[None], 0, W - 1)
    win = g[ref[:, None], yy, xx]
    ok &= win.max(1) > win.min(1)
    # the view test
    e = O[None, :, :] - c[:, None, :]
    faces = np.einsum("nvk,nk->nv", e, nrm) > min_cos * np.linalg.norm(e, axis=2)
    faces[np.arange(n), ref] = False
    pairs = int(faces[ok].sum())
    return rgb, K, R, t, c, nrm, ref, int(ok.sum()), pairs


def child(a):
    import torch
    assert torch.cuda.is_available(), "warp_time needs the GPU"
    mvs = importlib.import_module(PKG)
    rgb, K, R, t, c, nrm, ref, valid, pairs = workload(mvs, a.n, a.wid, a.min_cos)
    dev = torch.device("cuda:0")
    with mvs.MvsContext(rgb, K, R, t, device=0) as ctx:
        st = torch.cuda.Stream(dev)
        with torch.cuda.stream(st):
            tc, tn, tr = (torch.from_numpy(v).to(dev) for v in (c, nrm, ref))
            xy = torch.empty((a.n, 2), dtype=torch.float64, device=dev)
            mask = torch.empty((a.n, ctx.words), dtype=torch.int64, device=dev)
            count = torch.empty(a.n, dtype=torch.int32, device=dev)
            avg = torch.empty(a.n, dtype=torch.float64, device=dev)

            def call():
                ctx.score_warped_device(tc, tn, tr, xy, mask, count, avg, None, 0.7, a.wid, a.min_cos,
                                        stream=st.cuda_stream)
            for _ in range(5):
                call()
            st.synchronize()
            us = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.calls):
                    call()
                e1.record(st)
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        passing = int(count.sum().item())
        accepted = int((count >= 3).sum().item())
    us.sort()
    med = us[len(us) // 2]
    N = (2 * a.wid + 1) ** 2
    samples = pairs * N
    print(json.dumps({"wid": a.wid, "n": a.n, "calls_per_window": a.calls, "windows": a.windows,
                      "us_per_call": round(med, 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2),
                      "valid_candidates": valid, "tested_pairs": pairs, "samples": samples,
                      "passing_views": passing, "candidates_with_3_views": accepted,
                      "candidates_per_s": a.n / med * 1e6, "tested_pairs_per_s": pairs / med * 1e6,
                      "samples_per_s": samples / med * 1e6,
                      "fp64_flop_per_s": samples * FLOP_PER_SAMPLE / med * 1e6}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-cos", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to each wid's process")
    ap.add_argument("--wid", type=int, default=0, help="(child) the one wid to time")
    a = ap.parse_args()
    if a.wid:
        sys.path.insert(0, REPO)
        child(a)
        return 0
    out = {"kernel": "k_score_warp", "scene": "dinoRing 48 x 640 x 480", "min_ncc": 0.7, "min_cos": a.min_cos,
           "flop_per_sample": FLOP_PER_SAMPLE}
    for wid in (5, 3):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--wid", str(wid),
               "--n", str(a.n), "--calls", str(a.calls), "--windows", str(a.windows), "--min-cos", str(a.min_cos)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            # nothing more is started on the GPU after a step that failed
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(json.dumps({"error": f"wid {wid} exited with {p.returncode}", **out}))
            return 1
        out[f"wid{wid}"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
