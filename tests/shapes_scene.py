"""Scenes and candidates for the odd-image-size tests of the MVS kernels
(test_mvs_shapes_host.py, test_mvs_shapes_gpu.py).  No GPU.

The sphere scene of synthetic.py only passes the photo test in the image
centre and synthetic.candidates keeps away from the border, so neither puts a
passing candidate into a partial tile.  Here every view is a noisy copy of one
random image: the same-pixel photo test passes anywhere, with counts from 0 to
nearly V, and the candidates cover the whole image and a margin around it."""
import importlib

import numpy as np

from conftest import PKG_NAME
from oracle import oracle as orc

TILE_W, TILE_H = 16, 8          # the tiled scorers' pixel tile
N_UNIFORM, N_AIMED = 6000, 256  # candidates: uniform part, and per aimed box
THR = (0.7, 0.4, 0.0)
WIDS = (1, 2, 3, 4, 5)
# (H, W, V) of the scoring tests
SCENES = [(16, 16, 5), (16, 16, 64), (23, 29, 16), (39, 45, 17), (67, 81, 48), (57, 93, 64),
          (41, 2061, 6), (47, 61, 65), (55, 77, 130),
          # W mod 4 = 3: the last, partial quad of a row holds column W-2, the
          # last one a window reaches (at W mod 4 = 1 it holds column W-1 alone)
          (26, 31, 20)]
# Inputs changed where the defaults leave an edge tile short of passing
# candidates (test_mvs_shapes_host.py asserts the floors):
#   amp_shift 5 at V = 5 and 6: views 0 and 3 are constant in the corner and
#     view 1 everywhere, so the noise cycle starts where views 2 and 4, the
#     textured ones, get the low amplitudes 8 and 58 and pass at 0.7;
#   n_aimed 1024: at 16 x 16 only 1 pixel in 16 of the last tile row is a valid
#     centre at wid 5, and at W = 2061 the uniform part puts 35 candidates into
#     the last tile column.
SCENE_INPUTS = {(16, 16, 5): dict(amp_shift=5, n_aimed=1024), (16, 16, 64): dict(n_aimed=1024),
                (41, 2061, 6): dict(amp_shift=5, n_aimed=1024)}


def copies_scene(V, H, W, seed, amp_shift=0):
    """V noisy gray copies of one uniform-random image, as RGB with R = G = B
    (the gray conversion keeps such a pixel's value), seen by ring cameras:
    view v adds N(0, amp_v), amp_v = 8 + 150 ((v + amp_shift) mod 7) / 6, so
    that view pairs correlate from nearly 1 down to about 0.2.  Every third view is constant
    (37 + v mod 5) over the bottom-right 14 x 16 pixels -- constant windows in
    the corner tiles -- and view 1 is constant 200 everywhere.
    -> (rgb (V, H, W, 3) uint8, K, R, t)."""
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    rng = np.random.default_rng([seed, V, H, W])
    base = rng.integers(0, 256, (H, W)).astype(np.float64)
    gray = np.empty((V, H, W), np.uint8)
    for v in range(V):
        amp = 8.0 + 150.0 * ((v + amp_shift) % 7) / 6.0
        gray[v] = np.clip(base + rng.normal(0.0, amp, (H, W)), 0, 255).astype(np.uint8)
        if v % 3 == 0:
            gray[v, H - 14:, W - 16:] = 37 + v % 5
    if V > 1:
        gray[1] = 200
    rgb = np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=-1))
    assert np.array_equal(orc.gray_from_rgb(rgb), gray)
    K, R, t = syn.ring_cameras(V, H, W, 0.33)
    return rgb, K, R, t


def at_pixels(x, y, ref, K, R, t, depth=0.33):
    """Candidates that project to pixel (x, y) of their reference view."""
    n = len(ref)
    ray = np.einsum("nij,nj->ni", np.linalg.inv(K)[ref], np.stack([x, y, np.ones(n)], 1))
    c = np.einsum("nji,nj->ni", R[ref], depth * ray - t[ref].reshape(n, 3))
    return np.ascontiguousarray(c), ref


def last_tile_origin(W, H):
    """(x, y) of the first pixel of the tile column / row holding pixel W-1 / H-1."""
    return (W - 1) // TILE_W * TILE_W, (H - 1) // TILE_H * TILE_H


def full_candidates(n, K, R, t, W, H, seed, n_aimed=N_AIMED):
    """n candidates whose pixel is uniform over the image and a 2-pixel margin
    around it, then n_aimed in each of the last tile column, the last tile row
    and the tile both share; reference views uniform.  -> (c (m, 3), ref (m,))."""
    V = len(K)
    K = np.asarray(K, np.float64).reshape(V, 3, 3)
    R = np.asarray(R, np.float64).reshape(V, 3, 3)
    t = np.asarray(t, np.float64).reshape(V, 3)
    rng = np.random.default_rng([seed, n, W, H])
    xl, yl = last_tile_origin(W, H)
    xs, ys = [rng.uniform(-2, W + 2, n)], [rng.uniform(-2, H + 2, n)]
    for x0, y0 in ((xl, 0), (0, yl), (xl, yl)):
        xs.append(rng.uniform(x0, W, n_aimed))
        ys.append(rng.uniform(y0, H, n_aimed))
    x, y = np.concatenate(xs), np.concatenate(ys)
    ref = rng.integers(0, V, len(x)).astype(np.int32)
    return at_pixels(x, y, ref, K, R, t)


def scene_and_candidates(H, W, V, seed=1):
    """The scoring tests' inputs of one of SCENES: (rgb, K, R, t), (c, ref)."""
    inp = SCENE_INPUTS.get((H, W, V), {})
    scene = copies_scene(V, H, W, seed, amp_shift=inp.get("amp_shift", 0))
    return scene, full_candidates(N_UNIFORM, *scene[1:], W, H, seed, n_aimed=inp.get("n_aimed", N_AIMED))


def coverage(xy, count, H, W, wid):
    """What a scored batch (oracle xy and count) reaches: candidates with a
    passing view in the last tile column, the last tile row and the corner
    tile, whether those hold a valid window centre at all, distinct counts,
    non-passing candidates inside the image and invalid windows."""
    q, r = np.floor(xy[:, 0]), np.floor(xy[:, 1])
    valid = (q >= wid + 1) & (q <= W - wid - 2) & (r >= wid) & (r <= H - wid - 2)
    inside = (xy[:, 0] >= 0) & (xy[:, 0] < W) & (xy[:, 1] >= 0) & (xy[:, 1] < H)
    xl, yl = last_tile_origin(W, H)
    col, row, hit = q >= xl, r >= yl, valid & (count > 0)
    return {
        "col_has_centre": bool(xl <= W - wid - 2), "row_has_centre": bool(yl <= H - wid - 2),
        "col": int((hit & col).sum()), "row": int((hit & row).sum()), "corner": int((hit & col & row).sum()),
        "counts": int(len(np.unique(count))), "zero_inside": int((inside & (count == 0)).sum()),
        "invalid": int((~valid).sum()), "passing": int(hit.sum()),
    }
