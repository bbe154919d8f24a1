"""K-steps of k_score_tab over a sweep, recounted on the CPU (numpy; no GPU).

From a sweep's candidates: the candidates the scorer sees (a valid window whose
reference window is not constant, as bench.floor_bytes decides it), its work
items (the tiles in index order, chunks of 1024, candidates in index order),
the M-blocks of 16, each wave's block range (wave w takes blocks
[w nblk / 8, (w + 1) nblk / 8)), the stable sort by row pair inside
the wave and the units of two blocks -- then per unit the span in K-steps
(WID + 1 + the distance in row pairs between its first and last candidate) and
the K-steps the kernel issues for it under a pass rule:

  parent  exact passes for span WID + 1 and WID + 2, two passes of WID + 1 beyond
  exact   one pass of the span's length                       (the shipped rule)
  one     exact for WID + 1 and WID + 2, the whole region (WID + 4) beyond

MFMA = sum over units of (blocks x K-steps) x view blocks: the counter
SQ_INSTS_VALU_MFMA_I8 of one launch.  Tiles above the bucket cap are not
modelled (their tail goes to the direct path).

usage: python tools/kstep_count.py [--wid 5 3] [--n 1048576]
  the bench's sweep (synthetic.candidates, seed 0) on dinoRing: one JSON line
  per window size.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
TILE_W, TILE_H, WAVES, CHUNK = 16, 8, 8, 1024
RULES = ("parent", "exact", "one")


def wave_bounds(nblk):
    """The first block of each wave and the end: 9 numbers."""
    return [nblk * w // WAVES for w in range(WAVES + 1)]


def steps_of(span, wid, rule):
    """K-steps issued for units of the given spans (array)."""
    ksk, ks = wid + 1, wid + 4
    span = np.asarray(span)
    assert ((span >= ksk) & (span <= ks)).all()
    if rule == "exact":
        return span.copy()
    return np.where(span <= ksk + 1, span, 2 * ksk if rule == "parent" else ks)


def gray_of(rgb):
    """OpenCV's BGR2GRAY weights on RGB data (HarrisFeatures.py:125), as bench.floor_bytes."""
    c = rgb.astype(np.int64)
    return (c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14


def project(c, ref, K, R, t):
    """Pixel coordinates of the candidates in their reference views."""
    V = len(K)
    K, R, t = (np.asarray(a, np.float64).reshape(V, *s) for a, s in ((K, (3, 3)), (R, (3, 3)), (t, (3,))))
    p = np.einsum("nij,nj->ni", K[ref], np.einsum("nij,nj->ni", R[ref], c) + t[ref])
    return p[:, :2] / p[:, 2:3]


def scored(gray, xy, ref, wid):
    """(q, r) of the candidates the scorer sees, in index order: a valid
    window, not constant in the reference view (integral images)."""
    V, H, W = gray.shape
    npx = (2 * wid + 1) ** 2
    with np.errstate(invalid="ignore"):
        q, r = np.trunc(xy[:, 0]).astype(np.int64), np.trunc(xy[:, 1]).astype(np.int64)
    ok = np.isfinite(xy).all(1) & (xy[:, 0] >= 0) & (xy[:, 1] >= 0)
    ok &= (r - wid >= 0) & (r + wid + 1 < H) & (q - wid > 0) & (q + wid + 1 < W)
    q, r, rv = q[ok], r[ok], np.asarray(ref)[ok].astype(np.int64)
    S, Q = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    for v in range(V):
        sel = rv == v
        if not sel.any():
            continue
        g = gray[v].astype(np.int64)
        for src, dst in ((g, S), (g * g, Q)):
            ii = np.zeros((H + 1, W + 1), np.int64)
            ii[1:, 1:] = src.cumsum(0).cumsum(1)
            rr, qq = r[sel], q[sel]
            dst[sel] = (ii[rr + wid + 1, qq + wid + 1] - ii[rr - wid, qq + wid + 1]
                        - ii[rr + wid + 1, qq - wid] + ii[rr - wid, qq - wid])
    seen = npx * Q != S * S
    return q[seen], r[seen]


def units_of(q, r, W, wid):
    """The sweep's units: (blocks, span) per unit, and the per-tile counts."""
    ntx = (W + TILE_W - 1) // TILE_W
    tile = (r // TILE_H) * ntx + q // TILE_W
    pair = (r % TILE_H) >> 1
    order = np.argsort(tile, kind="stable")
    tile, pair = tile[order], pair[order]
    tiles, first, per_tile = np.unique(tile, return_index=True, return_counts=True)
    pos = np.arange(len(tile)) - np.repeat(first, per_tile)
    item = np.repeat(np.arange(len(tiles)), per_tile) * (1 << 20) + pos // CHUNK   # (tile, chunk)
    pos %= CHUNK
    _, nc = np.unique(item, return_counts=True)
    nblk = (nc + 15) // 16
    # the wave of every block, per block count
    wave_of = np.zeros((CHUNK // 16 + 1, CHUNK // 16), np.int64)
    for nb in range(CHUNK // 16 + 1):
        b = wave_bounds(nb)
        assert b[0] == 0 and b[-1] == nb and all(0 <= b[w + 1] - b[w] <= 8 for w in range(WAVES))
        for w in range(WAVES):
            wave_of[nb, b[w]:b[w + 1]] = w
    wave = wave_of[np.repeat(nblk, nc), pos // 16]
    # the stable sort by row pair inside (item, wave), then units of 32
    o2 = np.lexsort((np.arange(len(tile)), pair, wave, item))
    item, wave, pair = item[o2], wave[o2], pair[o2]
    key = item * WAVES + wave
    _, kfirst, kcnt = np.unique(key, return_index=True, return_counts=True)
    wpos = np.arange(len(key)) - np.repeat(kfirst, kcnt)
    ukey = key * (CHUNK // 32) + wpos // 32
    _, ufirst, ucnt = np.unique(ukey, return_index=True, return_counts=True)
    p_lo, p_hi = pair[ufirst], pair[ufirst + ucnt - 1]
    return (ucnt + 15) // 16, p_hi - p_lo + wid + 1, per_tile


def count(q, r, W, V, wid):
    """Units, span histogram and block K-steps / MFMA under every rule."""
    blocks, span, per_tile = units_of(q, r, W, wid)
    out = {"scored_candidates": int(len(q)), "tiles": int(len(per_tile)), "max_per_tile": int(per_tile.max(initial=0)),
           "blocks": int(blocks.sum()), "units": int(len(blocks)), "double_units": int((blocks == 2).sum()),
           "single_units": int((blocks == 1).sum()),
           "span_units": {int(s): int((span == s).sum()) for s in range(wid + 1, wid + 5)}}
    nvb = (V + 15) // 16
    for rule in RULES:
        bk = int((blocks * steps_of(span, wid, rule)).sum())
        out[rule] = {"block_ksteps": bk, "mfma": bk * nvb}
    return out


def span_histogram(xy, ref, gray, wid):
    """{span: units} of a batch on a scene's gray stack (V, H, W)."""
    q, r = scored(gray, xy, ref, wid)
    return count(q, r, gray.shape[2], gray.shape[0], wid)["span_units"]


def dino_sweep(n):
    import glob
    from PIL import Image
    sys.path.insert(0, REPO)
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    files = sorted(glob.glob(os.path.join(REPO, "data", "dinoRing", "*.png")))
    rgb = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    K, R, t = [], [], []
    for line in open(os.path.join(REPO, "data", "dinoRing", "dinoR_par.txt")).readlines()[1:]:
        v = [float(x) for x in line.split()[1:]]
        K.append(np.array(v[0:9]).reshape(3, 3))
        R.append(np.array(v[9:18]).reshape(3, 3))
        t.append(np.array(v[18:21]))
    K, R, t = np.array(K), np.array(R), np.array(t)
    c, ref = syn.candidates(n, K, R, t, W=rgb.shape[2], H=rgb.shape[1], seed=0)
    return gray_of(rgb), project(c, ref, K, R, t), ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wid", type=int, nargs="+", default=[5, 3])
    ap.add_argument("--n", type=int, default=1 << 20)
    a = ap.parse_args()
    gray, xy, ref = dino_sweep(a.n)
    V, H, W = gray.shape
    for wid in a.wid:
        q, r = scored(gray, xy, ref, wid)
        print(json.dumps({"scene": "dinoRing", "V": V, "wid": wid, "n": a.n, **count(q, r, W, V, wid)}))


if __name__ == "__main__":
    main()
