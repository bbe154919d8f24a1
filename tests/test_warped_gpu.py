"""mvs_score_warped (k_score_warp) against the float64 restatement of its
definition (tests/warped_reference.py).

Comparison rule, for every tested pair (valid candidate, view v != ref whose
camera the normal faces):
  |ncc_gpu - ncc_ref| <= 1e-8 / min(1, sigma_b)
(1.5e-12 px between two binary64 formulations of the sample position, x 255
gray per px, x 2 axes, x 2 for the sigma term, / sigma_b ~ 1.5e-9 / sigma_b,
with a margin of about 7).  The nan pattern and the mask bits are equal except
in three bands: the reference's |ncc - min_ncc| within that tolerance (mask
bit only), a border margin below 1e-9 px, a min_cos margin below 1e-12.  The
pairs the bands leave out may be at most 0.5 % of the tested pairs.  count and
avg are recomputed from the GPU's own mask and ncc; xy is bit-equal to
ctx.score's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import warped_reference as wr
from conftest import PKG_NAME, REPO, bench_candidates

pytestmark = pytest.mark.gpu

BORDER_BAND = 1e-9
COS_BAND = 1e-12
MAX_LEFT_OUT = 0.005


def _context(pkg, rgb, K, R, t):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return pkg.MvsContext(rgb, K, R, t, device=0)


def _bits(mask, V):
    """(n, words) uint64 -> (n, 64 * words) bool, and the pad bits' union."""
    n, words = mask.shape
    b = (mask[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    b = b.reshape(n, 64 * words).astype(bool)
    return b[:, :V], b[:, V:].any()


def check_against_reference(out, o, ref, min_ncc, V, label="", budget=True):
    """out = ctx.score_warped(..., want_ncc=True); o = wr.warped_batch(...).
    budget=False (cases placed on a band on purpose) drops the 0.5 % limit."""
    xy, mask, count, avg, ncc = out
    n = len(ref)
    bits, pad_set = _bits(mask, V)
    assert not pad_set, "a pad view's bit is set"
    is_ref = np.arange(V)[None, :] == np.asarray(ref)[:, None]
    cos_band = np.abs(o["cosm"]) < COS_BAND
    cand_band = cos_band[np.arange(n), ref]                     # the reference view's own min_cos test
    tested = o["valid"][:, None] & ~is_ref & (o["cosm"] > 0)
    near = tested | cos_band | cand_band[:, None]
    # pairs no band touches and the reference does not test: nan, bit clear
    off = ~near
    assert np.all(np.isnan(ncc[off])) and not bits[off].any()
    left_out = tested & (cos_band | cand_band[:, None] | (np.abs(o["border"]) < BORDER_BAND))
    cmp_ = tested & ~left_out
    tol = 1e-8 / np.minimum(1.0, np.where(o["sigma_b"] > 0, o["sigma_b"], 1.0))
    gnan, rnan = np.isnan(ncc), np.isnan(o["ncc"])
    assert np.array_equal(gnan[cmp_], rnan[cmp_]), f"nan pattern differs on {(gnan != rnan)[cmp_].sum()} pairs"
    both = cmp_ & ~rnan
    err = np.abs(ncc - o["ncc"])
    worst = float(np.max((err / tol)[both])) if both.any() else 0.0
    print(f"{label}: {int(o['valid'].sum())} valid candidates, {int(tested.sum())} tested pairs, "
          f"{int(both.sum())} scored, {int((tested & (o['border'] < 0)).sum())} border failures, "
          f"{int((both & (o['sigma_b'] < 0.5)).sum())} with sigma_b < 0.5, {int(left_out.sum())} left out, "
          f"worst error {float(np.max(err[both])) if both.any() else 0.0:.3e} ({worst:.3f} of the tolerance)")
    assert np.all(err[both] <= tol[both])
    want = o["ncc"] > min_ncc                                   # False for nan
    thr_band = both & (np.abs(o["ncc"] - min_ncc) <= tol)
    sure = cmp_ & ~thr_band
    assert np.array_equal(bits[sure], want[sure])
    if budget:
        assert int(left_out.sum()) + int(thr_band.sum()) <= MAX_LEFT_OUT * max(int(tested.sum()), 1)
    # the outputs agree with each other everywhere
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits, ncc > min_ncc)
    assert np.array_equal(count, bits.sum(1))
    mean = np.array([ncc[i, bits[i]].mean() if bits[i].any() else 0.0 for i in range(n)])
    np.testing.assert_allclose(avg, mean, rtol=0, atol=1e-12)
    return bits


def toward_camera(Rp, t, c, ref):
    O = wr.centres(Rp, t)
    n = O[ref] - c
    return n / np.linalg.norm(n, axis=1, keepdims=True)


# ---------------------------------------------------------------------------
# 1. sphere scene
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere(pkg):
    rgb, K, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=0.02)[:4]
    ctx = _context(pkg, rgb, K, R, t)
    c, nrm, ref, shift = wr.sphere_patches(K, R, t, 256, 0.02, np.random.default_rng(1), (0.0, 0.002, -0.002))
    yield ctx, wr.gray_stack(rgb), K, t, ctx.rproj(), c, nrm, ref, shift
    ctx.close()


@pytest.mark.parametrize("wid,min_cos", [(5, 0.3), (3, 0.0)])
def test_sphere_scene(sphere, wid, min_cos):
    ctx, gray, K, t, Rp, c, nrm, ref, shift = sphere
    o = wr.warped_batch(gray, K, Rp, t, c, nrm, ref, wid, min_cos)
    out = ctx.score_warped(c, nrm, ref, 0.7, wid, min_cos, want_ncc=True)
    assert np.array_equal(out[0], ctx.score(c, ref, 0.7, wid)[0])
    check_against_reference(out, o, ref, 0.7, ctx.V, f"sphere wid {wid}")
    count = out[2]
    on, outw, inw = (float((count[shift == s] >= 3).mean()) for s in (0.0, 0.002, -0.002))
    print(f"share with >= 3 views: on the surface {on:.3f}, +2 mm {outw:.3f}, -2 mm {inw:.3f}")
    assert on >= 0.85 and outw <= 0.40 and inw <= 0.40


def test_device_call_on_a_torch_stream(sphere):
    """score_warped_device on a non-default torch stream: the host call's results, bit for bit."""
    import torch
    ctx, gray, K, t, Rp, c, nrm, ref, shift = sphere
    host = ctx.score_warped(c, nrm, ref, 0.7, 5, 0.3, want_ncc=True)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    n = len(ref)
    with torch.cuda.stream(st):
        tc, tn, tr = (torch.from_numpy(x).to(dev) for x in (c, nrm, ref))
        xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
        mask = torch.empty((n, ctx.words), dtype=torch.int64, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        avg = torch.empty(n, dtype=torch.float64, device=dev)
        ncc = torch.empty((n, ctx.V), dtype=torch.float64, device=dev)
        ctx.score_warped_device(tc, tn, tr, xy, mask, count, avg, ncc, 0.7, 5, 0.3, stream=st.cuda_stream)
        # without avg and ncc
        mask2 = torch.empty_like(mask)
        count2 = torch.empty_like(count)
        ctx.score_warped_device(tc, tn, tr, xy, mask2, count2, None, None, 0.7, 5, 0.3, stream=st.cuda_stream)
    st.synchronize()
    got = (xy.cpu().numpy(), mask.cpu().numpy().view(np.uint64), count.cpu().numpy(), avg.cpu().numpy(),
           ncc.cpu().numpy())
    for g, h in zip(got, host):
        assert np.array_equal(g, h, equal_nan=True)
    assert torch.equal(mask, mask2) and torch.equal(count, count2)
    with pytest.raises(RuntimeError, match="contiguous"):
        ctx.score_warped_device(tc, tn, tr, xy, mask[:, :0], count, stream=st.cuda_stream)


# ---------------------------------------------------------------------------
# 2. dinoRing
# ---------------------------------------------------------------------------
def test_dino_ring(pkg, dino):
    """512 synthetic.candidates (seed 3; conftest.bench_candidates is that
    generator) of dinoRing, normal towards the reference camera, wid 5, min_cos
    0.3.  On the context's gray stack -- the reference's cvtColor(BGR2GRAY) on
    RGB bytes, i.e. 0.114 R + 0.587 G + 0.299 B -- the restatement finds 378
    valid candidates, 5,276 scored pairs, 1,146 border failures and 633 pairs
    with 0 < sigma_b < 0.5.  The figures 381 / 5,375 / 1,159 / 663 quoted when
    the test was specified come from the same candidates on a gray image with
    the weights in RGB order (0.299 R + 0.587 G + 0.114 B: 381 / 5,374 / 1,159 /
    662 with this module's restatement); the definition names the context's
    gray stack, so that is what both sides use here."""
    rgb, K, R, t = dino
    ctx = _context(pkg, rgb, K, R, t)
    try:
        Rp = ctx.rproj()
        c, ref = bench_candidates(512, K, R, t, seed=3)
        nrm = toward_camera(Rp, t, c, ref)
        o = wr.warped_batch(wr.gray_stack(rgb), K, Rp, t, c, nrm, ref, 5, 0.3)
        out = ctx.score_warped(c, nrm, ref, 0.7, 5, 0.3, want_ncc=True)
        assert np.array_equal(out[0], ctx.score(c, ref, 0.7, 5)[0])
        check_against_reference(out, o, ref, 0.7, ctx.V, "dinoRing wid 5")
        scored = ~np.isnan(o["ncc"])
        assert scored.sum() > 1000 and ((o["sigma_b"] < 0.5) & scored).sum() > 100   # small-sigma pairs are covered
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 3. V > 64
# ---------------------------------------------------------------------------
def test_more_than_64_views(pkg):
    rgb, K, R, t = pkg.synthetic.ring_scene(V=80, H=48, W=64)
    ctx = _context(pkg, rgb, K, R, t)
    try:
        assert ctx.words == 2
        Rp = ctx.rproj()
        rng = np.random.default_rng(4)
        c = rng.uniform(-0.005, 0.005, (128, 3)) / np.sqrt(3)
        ref = rng.integers(0, 80, 128).astype(np.int32)
        nrm = toward_camera(Rp, t, c, ref)
        # random textures: the scores scatter around 0, so a threshold of -0.05 sets bits in both words
        o = wr.warped_batch(wr.gray_stack(rgb), K, Rp, t, c, nrm, ref, 5, 0.3)
        out = ctx.score_warped(c, nrm, ref, -0.05, 5, 0.3, want_ncc=True)
        assert np.array_equal(out[0], ctx.score(c, ref, 0.7, 5)[0])
        check_against_reference(out, o, ref, -0.05, 80, "ring V=80")
        mask = out[1]
        assert mask[:, 0].any() and mask[:, 1].any()
        assert not (mask[:, 1] >> np.uint64(16)).any()          # pad views 80..127
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(pkg):
    """Four cameras over one random texture: 0 and 1 identical, 2 and 3 moved so
    that their samples land 3.3 px down-right / up-left of the reference window."""
    H, W = 40, 48
    rng = np.random.default_rng(7)
    g = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
    rgb = np.tile(np.repeat(g, 3, axis=2)[None], (4, 1, 1, 1))
    K = np.tile(np.array([[300.0, 0, 24.0], [0, 310.0, 20.0], [0, 0, 1.0]]), (4, 1, 1))
    R = np.tile(np.eye(3), (4, 1, 1))
    t = np.tile(np.array([0.01, -0.02, 0.0]), (4, 1))
    t[2] += [0.011, 0.011, 0.0]
    t[3] -= [0.011, 0.011, 0.0]
    ctx = _context(pkg, rgb, K, R, t)
    yield ctx, wr.gray_stack(rgb), K, t, ctx.rproj(), H, W
    ctx.close()


def _at_pixel(K, t, x, y, z=1.0):
    return np.array([(x - K[0, 0, 2]) / K[0, 0, 0] * z, (y - K[0, 1, 2]) / K[0, 1, 1] * z, z]) - t[0]


@pytest.mark.parametrize("wid", [5, 2])
def test_window_edges_and_identity(twin, wid):
    ctx, gray, K, t, Rp, H, W = twin
    N = (2 * wid + 1) ** 2
    front = np.array([0.0, 0.0, -1.0])
    # (x0, y0, valid): the window touching each border, then one pixel further out
    cases = [(wid, 20, True), (W - 1 - wid, 20, True), (24, wid, True), (24, H - 1 - wid, True),
             (wid - 1, 20, False), (W - wid, 20, False), (24, wid - 1, False), (24, H - wid, False),
             (W - 2 - wid, 20, True)]
    c = np.array([_at_pixel(K, t, x0 + 0.5, y0 + 0.5) for x0, y0, _ in cases])
    nrm = np.tile(front, (len(cases), 1))
    ref = np.zeros(len(cases), np.int32)
    xy, mask, count, avg, ncc = ctx.score_warped(c, nrm, ref, 0.7, wid, 0.0, want_ncc=True)
    assert np.array_equal(xy, ctx.score(c, ref, 0.7, wid)[0])
    o = wr.warped_batch(gray, K, Rp, t, c, nrm, ref, wid, 0.0)
    # the identical camera's samples sit on the border itself: inside the border band
    check_against_reference((xy, mask, count, avg, ncc), o, ref, 0.7, ctx.V, f"edges wid {wid}", budget=False)
    for k, (x0, y0, valid) in enumerate(cases):
        assert (int(xy[k, 0]), int(xy[k, 1])) == (x0, y0)
        assert bool(o["valid"][k]) == valid, k
        if valid:
            assert np.isfinite(ncc[k]).any(), k       # view 2 or 3 keeps the window inside
        else:
            assert count[k] == 0 and mask[k, 0] == 0 and avg[k] == 0 and np.all(np.isnan(ncc[k])), k
    # identity warp, the window's last column at W - 2: every sample inside, ncc = N / (N - 1)
    k = len(cases) - 1
    assert count[k] == 1 and mask[k, 0] == 2 and np.isnan(ncc[k, 0])
    assert abs(ncc[k, 1] - N / (N - 1)) <= 1e-9 and abs(avg[k] - N / (N - 1)) <= 1e-9
    assert abs(o["ncc"][k, 1] - N / (N - 1)) <= 1e-9


def test_behind_camera_and_back_facing(twin):
    ctx, gray, K, t, Rp, H, W = twin
    c = np.array([_at_pixel(K, t, 24.5, 20.5, 1.0), _at_pixel(K, t, 24.5, 20.5, -1.0),
                  _at_pixel(K, t, 24.5, 20.5, 1.0)])
    nrm = np.array([[0, 0, -1.0], [0, 0, -1.0], [0, 0, 1.0]])    # facing, behind the camera, back-facing
    ref = np.zeros(3, np.int32)
    xy, mask, count, avg, ncc = ctx.score_warped(c, nrm, ref, 0.7, 5, 0.0, want_ncc=True)
    assert np.array_equal(xy, ctx.score(c, ref, 0.7, 5)[0])
    o = wr.warped_batch(gray, K, Rp, t, c, nrm, ref, 5, 0.0)
    assert list(o["valid"]) == [True, False, False]
    assert count[0] == 1 and mask[0, 0] == 2
    for k in (1, 2):
        assert count[k] == 0 and mask[k, 0] == 0 and avg[k] == 0 and np.all(np.isnan(ncc[k]))


# ---------------------------------------------------------------------------
# 5. interleaving with the tiled scorer
# ---------------------------------------------------------------------------
INTERLEAVE = r"""
import sys, numpy as np, importlib
sys.path.insert(0, {repo!r}); sys.path.insert(0, {golden!r})
from make_seeds import load_dino
from oracle import oracle as orc
pkg = importlib.import_module({pkg!r})
imgs, K, R, t = load_dino({data!r})
rgb = np.stack(imgs)
ctx = pkg.MvsContext(rgb, K, R, t, device=0)
c, ref = pkg.synthetic.candidates(4096, K, R, t, seed=11)
O = -np.einsum("vji,vj->vi", ctx.rproj(), t.reshape(-1, 3))
nrm = O[ref] - c
nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
first = ctx.score(c, ref, 0.7, 5)
warped = ctx.score_warped(c[:1024], nrm[:1024], ref[:1024], 0.7, 5, 0.3)
again = ctx.score(c, ref, 0.7, 5)
assert ctx.scorer_stats()["batches"] == 2, ctx.scorer_stats()
want = orc.Scene(rgb, K, R, t).score_batch(c, ref, 0.7, 5)
for a, b in zip(first, again):
    assert np.array_equal(a, b)
for a, w in zip(first[:3], want[:3]):
    assert np.array_equal(a, w)
assert np.allclose(first[3], want[3], rtol=0, atol=1e-12)
assert warped[2].sum() > 0
ctx.close()
print("interleaved ok", flush=True)
"""


def test_interleaved_with_tiled_scorer():
    """score, score_warped, score under MVS_SCORE_KERNEL=tiled in a fresh
    process: the warped call leaves the tiled scorer's scratch and counter
    sets alone, so both score results are equal and are the oracle's."""
    code = INTERLEAVE.format(repo=REPO, golden=os.path.join(REPO, "tests", "golden"), pkg=PKG_NAME,
                             data=os.path.join(REPO, "data", "dinoRing"))
    env = dict(os.environ, MVS_SCORE_KERNEL="tiled")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode == 0 and "interleaved ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


# ---------------------------------------------------------------------------
# 6. arguments
# ---------------------------------------------------------------------------
def test_arguments(twin):
    ctx, gray, K, t, Rp, H, W = twin
    e3, e1 = np.empty((0, 3)), np.empty(0, np.int32)
    xy, mask, count, avg, ncc = ctx.score_warped(e3, e3, e1, want_ncc=True)
    assert xy.shape == (0, 2) and mask.shape == (0, 1) and count.shape == (0,) and ncc.shape == (0, 4)
    c = np.array([_at_pixel(K, t, 24.5, 20.5)])
    nrm = np.array([[0, 0, -1.0]])
    ref = np.zeros(1, np.int32)
    for kw, msg in (({"wid": 0}, "wid must be in 1..5"), ({"wid": 6}, "wid must be in 1..5"),
                    ({"min_cos": 1.0}, r"min_cos must be in \[0, 1\)"), ({"min_cos": -0.1}, "min_cos")):
        with pytest.raises(RuntimeError, match=msg):
            ctx.score_warped(c, nrm, ref, **kw)
    with pytest.raises(RuntimeError, match="ref view out of range"):
        ctx.score_warped(c, nrm, np.array([4], np.int32))
    full = ctx.score_warped(c, nrm, ref, 0.7, 3, 0.0, want_ncc=True)
    lean = ctx.score_warped(c, nrm, ref, 0.7, 3, 0.0)
    assert len(lean) == 4 and full[2][0] == 1
    for a, b in zip(lean, full):
        assert np.array_equal(a, b)
