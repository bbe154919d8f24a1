"""Timing of the per-pixel plane propagation (mvs_wprop_sweep_device,
MvsContext.densify_depth) on dinoRing.  The input maps are depth_maps (radius 1)
of the refined chain of tools/depth_time.py, over the full view range; the lists
are wprop_view_lists(4).  Prints one JSON line, per window half-width (5 and 3):

  sweeps: for each distinct (step, kd, ka) of the default schedule, at its
    first and its last place in the schedule, on the maps the chain holds there:
    device-event time of one sweep (median of `windows` windows of `reps`
    calls), and counted from those maps with torch --
      active_pixels   pixels inside the wid ring with a non-constant window
                      that hold a plane or have a neighbour `step` away that does
                      (the pixels phase B of the kernel walks);
      hypotheses      the hypotheses that exist on them: the own plane and its
                      grid (HY - 5 - 1 entries), and each neighbour that holds a
                      plane (the rare zero denominator is not subtracted);
      pairs_per_s     (hypothesis, list view) pairs over the sweep time;
      samples_per_s   pairs x (2 wid + 1)^2 over the sweep time (an upper bound:
                      a pair that fails a facing test samples nothing);
      lane_use        pairs over 64 lanes x passes x active pixels, the passes of
                      each view from its list (segments of the next power of
                      two >= |T| lanes, 64 / S hypotheses per pass);
      idle_share      the time of a sweep over empty maps (every pixel idle),
                      scaled by the share of idle pixels, over the sweep time;
  chain: densify_depth at the defaults -- device ms from the first mark to the
    last (median run of `windows`), wall ms, pixels holding a depth before and
    after, fused points, device ms per phase;
  baseline: the parent's only way to score the same hypotheses: 2^14 sampled
    active pixels of the last sweep's input, 31 candidates each for
    score_warped_device with ncc out (every view is tested there, not a
    list): the 27 planes of the grid around the own plane (its centre is the
    own plane) and, standing in for the four neighbour planes, four more
    copies of the own plane -- the same count and the same kind of plane per
    pixel, not the neighbours' planes themselves; time per candidate there
    over the sweep's time per hypothesis.

usage: python tools/densify_time.py [--n 4096] [--rounds 4] [--windows 5] [--reps 1] [--wids 5 3]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
DATA = os.path.join(REPO, "data", "dinoRing")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_time import Timer, windows_of  # noqa: E402

OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def holds(torch, z, n):
    return torch.isfinite(z) & (z > 0) & ~torch.isnan(n).any(-1)


def shifted(torch, m, dx, dy):
    """m at (x + dx, y + dy), False outside the image; m is (V,H,W) bool."""
    out = torch.zeros_like(m)
    H, W = m.shape[1:]
    ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
    xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
    if dy < H and -dy < H and dx < W and -dx < W:
        out[:, yd, xd] = m[:, ys, xs]
    return out


def textured(torch, rgb, wid, dev):
    """(V,H,W) bool: the window lies inside the image and is not constant (exact integer sums)."""
    p = torch.from_numpy(rgb.astype(np.int64)).to(dev)
    g = ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).to(torch.float64) - 128.0
    k = 2 * wid + 1
    w = torch.ones((1, 1, k, k), dtype=torch.float64, device=dev)
    x = g.unsqueeze(1)
    s1 = torch.nn.functional.conv2d(x, w)[:, 0]
    s2 = torch.nn.functional.conv2d(x * x, w)[:, 0]
    out = torch.zeros(g.shape, dtype=torch.bool, device=dev)
    out[:, wid:g.shape[1] - wid, wid:g.shape[2] - wid] = (k * k * s2 - s1 * s1) > 0.5
    return out


def active_per_view(torch, z, n, tex, step):
    """(V,) float64: the active pixels of each view."""
    own = holds(torch, z, n)
    nb = [shifted(torch, own, ox * step, oy * step) for ox, oy in OFFSETS]
    return (tex & (own | nb[0] | nb[1] | nb[2] | nb[3])).sum((1, 2)).to(torch.float64)


def sweep_counts(torch, z, n, tex, step, kd, ka, T):
    own = holds(torch, z, n)
    nb = [shifted(torch, own, ox * step, oy * step) for ox, oy in OFFSETS]
    any_nb = nb[0] | nb[1] | nb[2] | nb[3]
    active = tex & (own | any_nb)
    grid = (2 * kd + 1) * (2 * ka + 1) ** 2 - 1
    hyp = (own & active).sum() * (1 + grid) + sum((m & active).sum() for m in nb)
    pairs = ((own & active).sum((1, 2)) * (1 + grid) + sum((m & active).sum((1, 2)) for m in nb)) * T
    return int(active.sum().item()), int(hyp.item()), int(pairs.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--wids", type=int, nargs="+", default=[5, 3])
    ap.add_argument("--sample", type=int, default=1 << 14)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import torch
    assert torch.cuda.is_available(), "densify_time needs the GPU"
    from make_seeds import load_dino
    mvs = importlib.import_module(PKG)
    imgs, K, R, t = load_dino(DATA)
    rgb = np.stack(imgs)
    c, ref = mvs.synthetic.candidates(a.n, K, R, t, seed=0)
    res = {"tool": "densify_time", "scene": "dinoRing 48 x 640 x 480", "seeds": a.n, "rounds": a.rounds,
           "windows": a.windows, "reps": a.reps}
    with mvs.MvsContext(rgb, K, R, t, device=0) as ctx:
        Rp = ctx.rproj()
        O = -np.einsum("vji,vj->vi", Rp, t.reshape(-1, 3))
        nrm = O[ref] - c
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        ps = ctx.expand_warped(c, nrm, ref, a.rounds, cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2,
                               refine_levels=2)
        maps = ctx.depth_maps(ps, radius=1)
        V, H, W = ctx.V, ctx.H, ctx.W
        lists = ctx.wprop_view_lists(4)
        T = torch.from_numpy((lists >= 0).sum(1)).to("cuda:0")
        sched = list(ctx.DENSIFY_SCHEDULE)
        kinds = sorted({s[:3] for s in sched})
        places = sorted({p for k in kinds for p in (min(i for i, s in enumerate(sched) if s[:3] == k),
                                                    max(i for i, s in enumerate(sched) if s[:3] == k))})
        res.update(patches=len(ps["ref"]), pixels=V * H * W, lists_tv=4, list_views_mean=round(float((lists >= 0).sum(1).mean()), 2),
                   schedule=[list(s) for s in sched])
        dev = torch.device("cuda:0")
        st = torch.cuda.Stream(dev)
        sh = st.cuda_stream
        for wid in a.wids:
            N = (2 * wid + 1) ** 2
            with torch.cuda.stream(st):
                tex = textured(torch, rgb, wid, dev)
                z = [torch.from_numpy(maps["z"]).to(dev), torch.empty((V, H, W), dtype=torch.float64, device=dev)]
                n = [torch.from_numpy(maps["normal"]).to(dev), torch.empty((V, H, W, 3), dtype=torch.float64, device=dev)]
                score = torch.empty((V, H, W), dtype=torch.float64, device=dev)
                best = torch.empty((V, H, W), dtype=torch.int32, device=dev)
                zo, no = torch.empty_like(z[0]), torch.empty_like(n[0])
                ze = torch.full((V, H, W), float("inf"), dtype=torch.float64, device=dev)
                ne = torch.full((V, H, W, 3), float("nan"), dtype=torch.float64, device=dev)
            st.synchronize()

            def sweep(zi, ni, zz, nn, k):
                step, kd, ka, scale = sched[k]
                ctx.wprop_sweep_device(zi, ni, lists, 0, V, zz, nn, score, best, None, wid, 0.3, 0.7, 2, step, kd, ka,
                                       ctx.DENSIFY_ASTEP, ctx.DENSIFY_DEPTH_PX, scale, stream=sh)
            rows = []
            cur = 0
            last_in = None
            for k in range(len(sched)):
                if k in places:
                    step, kd, ka, scale = sched[k]
                    tm = windows_of(torch, st, lambda: sweep(z[cur], n[cur], zo, no, k), a.windows, a.reps)
                    idle = windows_of(torch, st, lambda: sweep(ze, ne, zo, no, k), a.windows, a.reps)
                    with torch.cuda.stream(st):
                        act, hyp, pairs = sweep_counts(torch, z[cur], n[cur], tex, step, kd, ka, T)
                        held = int(holds(torch, z[cur], n[cur]).sum().item())
                    hy = ctx.wprop_hypotheses(kd, ka)
                    # per view: segments of S = the next power of two >= |T| lanes, 64 / S hypotheses per pass
                    seg = [1 << max(int(x) - 1, 0).bit_length() for x in (lists >= 0).sum(1)]
                    passes_v = torch.tensor([math.ceil(hy / (64 // s_)) for s_ in seg], dtype=torch.float64, device=dev)
                    with torch.cuda.stream(st):
                        lanes = float((active_per_view(torch, z[cur], n[cur], tex, step) * passes_v).sum().item()) * 64.0
                    sec = tm[0] * 1e-3
                    rows.append({"sweep": k, "step": step, "kd": kd, "ka": ka, "step_scale": scale,
                                 "device_ms": round(tm[0], 3), "device_ms_min": round(tm[1], 3),
                                 "device_ms_max": round(tm[2], 3), "pixels_holding_a_depth": held, "active_pixels": act,
                                 "hypotheses": hyp, "pairs": pairs, "pairs_per_s": round(pairs / sec, 1),
                                 "samples_per_s": round(pairs * N / sec, 1),
                                 "lane_use": round(pairs / max(lanes, 1.0), 3),
                                 "all_idle_ms": round(idle[0], 3),
                                 "idle_share": round(idle[0] * (1 - act / (V * H * W)) / tm[0], 4)})
                    if k == len(sched) - 1:
                        with torch.cuda.stream(st):
                            last_in = (z[cur].clone(), n[cur].clone(), act, hyp, tm[0])
                with torch.cuda.stream(st):
                    sweep(z[cur], n[cur], z[1 - cur], n[1 - cur], k)
                cur = 1 - cur
            st.synchronize()
            # the whole chain
            runs = []
            for _ in range(a.windows + 1):
                tk = Timer(torch)
                t0 = time.perf_counter()
                out = ctx.densify_depth(maps, lists=lists, wid=wid, timer=tk)
                wall = (time.perf_counter() - t0) * 1e3
                tk.marks[-1][1].synchronize()
                per = {}
                for (ph, ev), (_, ev1) in zip(tk.marks[:-1], tk.marks[1:]):
                    per[ph] = per.get(ph, 0.0) + ev.elapsed_time(ev1)
                runs.append((tk.marks[0][1].elapsed_time(tk.marks[-1][1]), wall, per))
            runs = sorted(runs[1:], key=lambda x: x[0])
            total, wall, per = runs[len(runs) // 2]
            chain = {"device_ms": round(total, 2), "device_ms_min": round(runs[0][0], 2),
                     "device_ms_max": round(runs[-1][0], 2), "wall_ms": round(wall, 1),
                     "pixels_before": int(np.isfinite(maps["z"]).sum()), "pixels_after": int(np.isfinite(out["z"]).sum()),
                     "fused_before": len(maps["pix"]), "fused": len(out["pix"]), "history": out["history"].tolist(),
                     "phase_device_ms": {k: round(v, 2) for k, v in per.items()}}
            # the baseline: the hypotheses of sampled active pixels of the last sweep as score_warped candidates
            zi, ni, act, hyp, sweep_ms = last_in
            step, kd, ka, scale = sched[-1]
            with torch.cuda.stream(st):
                own = holds(torch, zi, ni) & tex
                at = own.nonzero()
                pick = at[torch.randperm(len(at), device=dev, generator=torch.Generator(dev).manual_seed(0))[:a.sample]]
                pv, py, px = (pick[:, 0].cpu().numpy(), pick[:, 1].cpu().numpy(), pick[:, 2].cpu().numpy())
                zs = zi[pick[:, 0], pick[:, 1], pick[:, 2]].cpu().numpy()
                ns = ni[pick[:, 0], pick[:, 1], pick[:, 2]].cpu().numpy()
            st.synchronize()
            fx, fy, cx, cy = K[pv, 0, 0], K[pv, 1, 1], K[pv, 0, 2], K[pv, 1, 2]
            ray = np.einsum("nji,nj->ni", Rp[pv], np.stack([(px - cx) / fx, (py - cy) / fy, np.ones(len(pv))], 1))
            dz = zs / ((fx + fy) / 2)
            cc, cn = [], []
            tans = [math.tan(i * ctx.DENSIFY_ASTEP * scale) for i in range(-ka, ka + 1)]
            ax = np.eye(3)[np.argmin(np.abs(ns), 1)]
            e1 = np.cross(ns, ax)
            e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
            e2 = np.cross(ns, e1)
            for kk in range(-kd, kd + 1):
                for tj in tans:
                    for ti in tans:
                        w = ns + ti * e1 + tj * e2
                        cc.append(O[pv] + ray * (zs + kk * dz * scale)[:, None])
                        cn.append(w / np.linalg.norm(w, axis=1, keepdims=True))
            for _ in range(4):                                       # stand-ins for the four neighbour planes: the own plane again
                cc.append(cc[len(cc) // 2])
                cn.append(cn[len(cn) // 2])
            bc, bn = np.ascontiguousarray(np.concatenate(cc)), np.ascontiguousarray(np.concatenate(cn))
            br = np.ascontiguousarray(np.tile(pv.astype(np.int32), len(cc)))
            nb = len(br)
            with torch.cuda.stream(st):
                tc, tn, tr = torch.from_numpy(bc).to(dev), torch.from_numpy(bn).to(dev), torch.from_numpy(br).to(dev)
                xy = torch.empty((nb, 2), dtype=torch.float64, device=dev)
                mask = torch.empty((nb, ctx.words), dtype=torch.int64, device=dev)
                count = torch.empty(nb, dtype=torch.int32, device=dev)
                ncc = torch.empty((nb, V), dtype=torch.float64, device=dev)
            st.synchronize()
            base = windows_of(torch, st, lambda: ctx.score_warped_device(tc, tn, tr, xy, mask, count, None, ncc, 0.7, wid,
                                                                         0.3, stream=sh), a.windows, a.reps)
            us_base = base[0] * 1e3 / nb
            us_sweep = sweep_ms * 1e3 / max(hyp, 1)
            res[f"wid{wid}"] = {"sweeps": rows, "chain": chain,
                                "baseline": {"pixels": len(pv), "candidates": nb, "device_ms": round(base[0], 3),
                                             "us_per_hypothesis": round(us_base, 4),
                                             "sweep_us_per_hypothesis": round(us_sweep, 4),
                                             "ratio": round(us_base / us_sweep, 2)}}
            del z, n, zo, no, ze, ne, tex, score, best, last_in
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
