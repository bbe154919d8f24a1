"""Timing of the signed-distance fusion and marching tetrahedra
(mvs_wtsdf_integrate_device, mvs_wmesh_extract_device, MvsContext.mesh_depth) on
dinoRing.  The input maps are the densified maps of tools/densify_time.py's
chain (depth_maps at radius 1 of the refined expansion, then densify_depth at
the defaults), masked by mesh_depth's fusion rule; the lattice is mesh_depth's
default one at --resolution.  Prints one JSON line:

  integrate: device-event time of k_wtsdf_integrate (median of `windows` windows
    of `reps` calls); projections = lattice points x views; landed = those that
    pass step 1 (in front of the camera, nearest pixel inside the image),
    counted with torch in the kernel's operation order; floor_bytes = the four
    outputs once (16 B per lattice point) + one 8-B depth per landed projection,
    floor_ms at --peak_gbs (default 8000, the MI355X's HBM), and the achieved
    rates;
  extract: the counting call (a memset, k_wmesh_mark, k_wmesh_vcount,
    k_wmesh_scan) and the writing call (those four, then k_wmesh_vertex and
    k_wmesh_tri); emit_ms is their difference.  The passes run inside one
    library call each, so the five kernels are not timed one by one;
  chain: mesh_depth -- device ms from the first mark to the last (median run of
    `windows`), wall ms, device ms per phase, vertices and faces, beside the
    points of the fused cloud the mesh replaces.

usage: python tools/mesh_time.py [--n 4096] [--rounds 4] [--resolution 256] [--windows 5] [--reps 1]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from filter_time import Timer, windows_of  # noqa: E402


def landed_projections(torch, ctx, K, t, dims, origin, voxel, dev):
    """The (lattice point, view) pairs that pass step 1 of the integration."""
    nx, ny, nz = dims
    Rp = ctx.rproj()
    i = torch.arange(nx + 1, dtype=torch.float64, device=dev)
    j = torch.arange(ny + 1, dtype=torch.float64, device=dev)
    k = torch.arange(nz + 1, dtype=torch.float64, device=dev)
    X = (origin[0] + i * voxel).reshape(1, 1, -1)
    Y = (origin[1] + j * voxel).reshape(1, -1, 1)
    Z = (origin[2] + k * voxel).reshape(-1, 1, 1)
    landed = 0
    for v in range(ctx.V):
        r, tv = [float(x) for x in Rp[v].reshape(9)], [float(x) for x in t[v].reshape(3)]
        x = r[0] * X + r[1] * Y + r[2] * Z + tv[0]
        y = r[3] * X + r[4] * Y + r[5] * Z + tv[1]
        z = r[6] * X + r[7] * Y + r[8] * Z + tv[2]
        r1 = torch.where(z != 0.0, 1.0 / z, torch.ones_like(z))      # project(): the reciprocal, then two products
        x = x * r1 * float(K[v][0, 0]) + float(K[v][0, 2])
        y = y * r1 * float(K[v][1, 1]) + float(K[v][1, 2])
        landed += int(((z > 0) & (x >= 0) & (y >= 0) & (x + 0.5 < ctx.W) & (y + 0.5 < ctx.H)).sum().item())
    return landed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--peak_gbs", type=float, default=8000.0)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import torch
    assert torch.cuda.is_available(), "mesh_time needs the GPU"
    from make_seeds import load_dino
    mvs = importlib.import_module(PKG)
    imgs, K, R, t = load_dino(DATA)
    rgb = np.stack(imgs)
    c, ref = mvs.synthetic.candidates(a.n, K, R, t, seed=0)
    res = {"tool": "mesh_time", "scene": "dinoRing 48 x 640 x 480", "seeds": a.n, "rounds": a.rounds,
           "resolution": a.resolution, "windows": a.windows, "reps": a.reps}
    with mvs.MvsContext(rgb, K, R, t, device=0) as ctx:
        Rp = ctx.rproj()
        O = -np.einsum("vji,vj->vi", Rp, t.reshape(-1, 3))
        nrm = O[ref] - c
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        ps = ctx.expand_warped(c, nrm, ref, a.rounds, cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2,
                               refine_levels=2)
        maps = ctx.densify_depth(ctx.depth_maps(ps, radius=1))
        V, H, W = ctx.V, ctx.H, ctx.W
        origin, voxel, dims, trunc = mvs._lib.mesh_grid(maps["points"], None, a.resolution, 3.0)
        nx, ny, nz = dims
        shape = (nz + 1, ny + 1, nx + 1)
        points = shape[0] * shape[1] * shape[2]
        res.update(patches=len(ps["ref"]), cloud_points=len(maps["points"]), dims=list(dims), voxel=voxel,
                   lattice_points=points, origin=[float(x) for x in origin])
        dev = torch.device("cuda:0")
        st = torch.cuda.Stream(dev)
        sh = st.cuda_stream
        with torch.cuda.stream(st):
            z = torch.from_numpy(maps["z"]).to(dev)
            cons = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
            ctx.wdepth_consist_device(z, 0, V, 0.01, cons, viol, stream=sh)
            z = torch.where(torch.isfinite(z) & (cons >= 2) & (viol <= 0), z,
                            torch.full((), float("inf"), dtype=torch.float64, device=dev)).contiguous()
            tsdf = torch.empty(shape, dtype=torch.float64, device=dev)
            weight = torch.empty(shape, dtype=torch.int32, device=dev)
            col = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
            cnt = torch.empty(shape, dtype=torch.uint8, device=dev)
            total = torch.zeros(2, dtype=torch.int64, device=dev)
            landed = landed_projections(torch, ctx, K, t, dims, origin, voxel, dev)
        st.synchronize()
        tm = windows_of(torch, st, lambda: ctx.wtsdf_integrate_device(z, 0, V, dims, origin, voxel, trunc, 1, tsdf, weight,
                                                                      col, cnt, stream=sh), a.windows, a.reps)
        floor_bytes = points * 16 + landed * 8
        sec = tm[0] * 1e-3
        res["integrate"] = {"device_ms": round(tm[0], 3), "device_ms_min": round(tm[1], 3), "device_ms_max": round(tm[2], 3),
                            "projections": points * V, "landed": landed, "floor_bytes": floor_bytes,
                            "floor_ms": round(floor_bytes / (a.peak_gbs * 1e9) * 1e3, 4),
                            "projections_per_s": round(points * V / sec, 1),
                            "floor_gbs": round(floor_bytes / sec / 1e9, 2)}
        count = windows_of(torch, st, lambda: ctx.wmesh_extract_device(dims, origin, voxel, tsdf, col, cnt, None, None,
                                                                       None, total, stream=sh), a.windows, a.reps)
        n, m = (int(x) for x in total.cpu().numpy())
        with torch.cuda.stream(st):
            vert = torch.empty((n, 3), dtype=torch.float64, device=dev)
            vcol = torch.empty((n, 3), dtype=torch.uint8, device=dev)
            tri = torch.empty((m, 3), dtype=torch.int32, device=dev)
        st.synchronize()
        full = windows_of(torch, st, lambda: ctx.wmesh_extract_device(dims, origin, voxel, tsdf, col, cnt, vert, vcol, tri,
                                                                      total, stream=sh), a.windows, a.reps)
        res["extract"] = {"count_ms": round(count[0], 3), "count_ms_min": round(count[1], 3),
                          "count_ms_max": round(count[2], 3), "write_ms": round(full[0], 3),
                          "write_ms_min": round(full[1], 3), "write_ms_max": round(full[2], 3),
                          "emit_ms": round(full[0] - count[0], 3), "vertices": n, "faces": m,
                          "seen_points": int(torch.isfinite(tsdf).sum().item())}
        del vert, vcol, tri, tsdf, weight, col, cnt
        runs = []
        for _ in range(a.windows + 1):
            tk = Timer(torch)
            t0 = time.perf_counter()
            out = ctx.mesh_depth(maps, resolution=a.resolution, timer=tk)
            wall = (time.perf_counter() - t0) * 1e3
            tk.marks[-1][1].synchronize()
            per = {}
            for (ph, ev), (_, ev1) in zip(tk.marks[:-1], tk.marks[1:]):
                per[ph] = per.get(ph, 0.0) + ev.elapsed_time(ev1)
            runs.append((tk.marks[0][1].elapsed_time(tk.marks[-1][1]), wall, per))
        runs = sorted(runs[1:], key=lambda x: x[0])
        dev_ms, wall, per = runs[len(runs) // 2]
        res["chain"] = {"device_ms": round(dev_ms, 2), "device_ms_min": round(runs[0][0], 2),
                        "device_ms_max": round(runs[-1][0], 2), "wall_ms": round(wall, 1),
                        "phase_device_ms": {k: round(v, 2) for k, v in per.items()},
                        "vertices": len(out["vertices"]), "faces": len(out["faces"]),
                        "cloud_points": len(maps["points"])}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
