"""Timing of the warped expansion chain (MvsContext.expand_warped) on dinoRing:
2^12 synthetic.candidates as seeds, normal = unit vector from the centre to the
reference camera, 4 rounds, wid 5, cell 2, min_ncc 0.7, min_cos 0.3, vlb 2,
without and with two refinement levels.  Each configuration runs in a child
process of its own under a time limit: one traced run for the counts, then
timed runs (the median run is reported).  Prints one JSON line; per round:

  frontier, jobs, shared (the share of jobs whose (view, cell) another job names
  too), accepted, winners, kept (refined patches that replaced their winner);
  device milliseconds between the chain's phase marks (events on its stream):
    score     mvs_score_warped_device of the round's jobs
    claim     accept flags (a torch op) + k_wexp_claim_max / _min / _win / _reset
    refine    the winners' refinement: k_refine_lists, level calls, re-score
    mark      k_wexp_mark
    children  the frontier's masking (torch ops) + k_wexp_children count pass,
              k_wexp_scan, emit pass
    sync      the round's one read of [job total, winners]
    append    the winners' gather into the patch set
  and host_ms: the wall time the host spent in each phase (for sync: the wait
  for the device to drain plus the 16-byte copy).

usage: python tools/expand_time.py [--n 4096] [--rounds 4] [--runs 5] [--limit 300] [--ply FILE]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
DATA = os.path.join(REPO, "data", "dinoRing")
PHASES = ("score", "claim", "refine", "mark", "children", "sync", "append")


class Timer:
    """timer(phase, round) of expand_warped: an event on the chain's stream and the host clock at every mark."""

    def __init__(self, torch):
        self.torch = torch
        self.marks = []

    def __call__(self, phase, rnd):
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record()                       # the current stream is the chain's
        self.marks.append((phase, rnd, ev, time.perf_counter()))

    def rounds(self):
        self.marks[-1][2].synchronize()
        out = {}
        for (ph, rnd, ev, tm), (_, _, ev1, tm1) in zip(self.marks[:-1], self.marks[1:]):
            r = out.setdefault(rnd, {"device_ms": {}, "host_ms": {}})
            r["device_ms"][ph] = r["device_ms"].get(ph, 0.0) + ev.elapsed_time(ev1)
            r["host_ms"][ph] = r["host_ms"].get(ph, 0.0) + (tm1 - tm) * 1e3
        return out


def child(a):
    import torch
    assert torch.cuda.is_available(), "expand_time needs the GPU"
    mvs = importlib.import_module(PKG)
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    from make_seeds import load_dino
    imgs, K, R, t = load_dino(DATA)
    rgb = np.stack(imgs)
    c, ref = mvs.synthetic.candidates(a.n, K, R, t, seed=0)
    kw = dict(cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2, refine_levels=a.levels)
    with mvs.MvsContext(rgb, K, R, t, device=0) as ctx:
        O = -np.einsum("vji,vj->vi", ctx.rproj(), t.reshape(-1, 3))
        nrm = O[ref] - c
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        res = ctx.expand_warped(c, nrm, ref, a.rounds, trace=True, **kw)
        rounds = []
        for rnd, tr in enumerate(res["trace"]):
            key = tr["jobs"][:, 1:].astype(np.int64)
            _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
            rounds.append({"round": rnd, "frontier": int((res["round"] == rnd - 1).sum()) if rnd else 0,
                           "jobs": len(key), "shared": float((cnt[inv.reshape(-1)] > 1).mean()) if len(key) else 0.0,
                           "accepted": int((tr["accept"] != 0).sum()), "winners": int((tr["win"] != 0).sum()),
                           "kept": int(tr["kept"].sum()) if "kept" in tr else 0})
        patches = len(res["ref"])
        if a.ply:
            r, xy = res["ref"], ctx.score(res["c"], res["ref"], 0.7, 5)[0]
            px = np.clip(xy.astype(np.int64), 0, [ctx.W - 1, ctx.H - 1])
            mvs.export2ply(res["c"], rgb[r, px[:, 1], px[:, 0]], path=os.path.splitext(a.ply)[0])
        del res
        runs = []
        for _ in range(a.runs):
            tm = Timer(torch)
            t0 = time.perf_counter()
            out = ctx.expand_warped(c, nrm, ref, a.rounds, timer=tm, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            assert len(out["ref"]) == patches, "the chain is not deterministic"
            runs.append((wall, tm.rounds()))
    runs.sort(key=lambda x: x[0])
    wall, per = runs[len(runs) // 2]
    for r in rounds:
        p = per.get(r["round"], {"device_ms": {}, "host_ms": {}})
        r["device_ms"] = {k: round(p["device_ms"].get(k, 0.0), 4) for k in PHASES}
        r["host_ms"] = {k: round(p["host_ms"].get(k, 0.0), 4) for k in PHASES}
        dev = r["device_ms"]
        r["new_kernels_share"] = round((dev["claim"] + dev["mark"] + dev["children"]) / max(sum(dev.values()), 1e-9), 4)
    print(json.dumps({"refine_levels": a.levels, "seeds": a.n, "patches": patches, "wall_ms": round(wall, 2),
                      "wall_ms_min": round(runs[0][0], 2), "wall_ms_max": round(runs[-1][0], 2), "runs": a.runs,
                      "rounds": rounds}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds allowed to each configuration's process")
    ap.add_argument("--ply", default="", help="write the refined chain's cloud to FILE")
    ap.add_argument("--levels", type=int, default=-1, help="(child) the one refine_levels to time")
    a = ap.parse_args()
    if a.levels >= 0:
        sys.path.insert(0, REPO)
        child(a)
        return 0
    out = {"chain": "expand_warped", "scene": "dinoRing 48 x 640 x 480", "wid": 5, "cell_size": 2, "min_ncc": 0.7,
           "min_cos": 0.3, "vlb": 2, "rounds": a.rounds}
    for levels in (0, 2):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--levels", str(levels),
               "--n", str(a.n), "--rounds", str(a.rounds), "--runs", str(a.runs)]
        if a.ply and levels:
            cmd += ["--ply", a.ply]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            # nothing more is started on the GPU after a step that failed
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(json.dumps({"error": f"refine_levels {levels} exited with {p.returncode}", **out}))
            return 1
        out[f"refine_levels_{levels}"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
