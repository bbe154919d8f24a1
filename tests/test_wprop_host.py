"""The float64 restatement of the per-pixel plane propagation
(tests/prop_reference.py) on its own, without a GPU: the rules the GPU tests
rely on when they compare mvs_wprop_sweep_device against it, the view-list rule,
and the quality experiment on the sphere scene whose figures stand in DESIGN 4.12."""
import functools
import math

import numpy as np
import pytest

import depth_reference as dr
import filter_reference as fr
import prop_reference as pr
import warped_reference as wr
from test_wdepth_host import depth_quality

RAD = 0.02
W, H = 64, 48
FRONT = np.array([0.0, 0.0, -1.0])


@functools.lru_cache(maxsize=None)
def plane_scene():
    """A textured plane Z = 1 seen by three cameras with identity rotation, 6 mm
    apart: gray (3,H,W) uint8, K, Rp, t.  Every camera sees the plane at depth 1."""
    rng = np.random.default_rng(5)
    K = np.array([[[300.0, 0, 32.0], [0, 310.0, 24.0], [0, 0, 1.0]]] * 3)
    Rp = np.array([np.eye(3)] * 3)
    t = np.array([[0.0, 0.0, 0.0], [0.006, 0.002, 0.0], [-0.004, 0.005, 0.0]])
    f, p = rng.normal(0, 1, (8, 2)) * 60.0, rng.uniform(0, 2 * np.pi, 8)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    gray = np.empty((3, H, W), np.uint8)
    for v in range(3):
        X = (xs - K[v, 0, 2]) / K[v, 0, 0] - t[v, 0]
        Y = (ys - K[v, 1, 2]) / K[v, 1, 1] - t[v, 1]
        gray[v] = np.clip(128 + 25 * sum(np.sin(X * a + Y * b + c) for (a, b), c in zip(f, p)), 0, 255).astype(np.uint8)
    return gray, K, Rp, t


KW = dict(wid=2, min_cos=0.3, min_ncc=0.7, top_k=2)


def seeded(q=(24, 32)):
    z = np.full((H, W), np.inf)
    n = np.full((H, W, 3), np.nan)
    z[q], n[q] = 1.0, FRONT
    return z, n


def test_propagation_fills_a_diamond():
    """From one seeded pixel, k sweeps at step 1 and kd = ka = 0 fill exactly the
    valid pixels with |dx| + |dy| <= k, every depth on the plane; step 3 reaches
    (+-3, 0) and (0, +-3) in one sweep."""
    gray, K, Rp, t = plane_scene()
    full = pr.sweep_view(gray, K, Rp, t, np.ones((H, W)), np.broadcast_to(FRONT, (H, W, 3)), 0, [1, 2], kd=0, ka=0,
                         details=False, **KW)
    valid = full["best"] >= 0
    ys, xs = np.mgrid[0:H, 0:W]
    dist = np.abs(ys - 24) + np.abs(xs - 32)
    assert valid[dist <= 4].all() and not valid[:2].any() and not valid[:, :2].any()
    z, n = seeded()
    for k in range(1, 4):
        o = pr.sweep_view(gray, K, Rp, t, z, n, 0, [1, 2], step=1, kd=0, ka=0, details=False, **KW)
        z, n = o["z_out"], o["n_out"]
        held = np.isfinite(z)
        assert np.array_equal(held, valid & (dist <= k)), k
        assert np.array_equal(held, o["best"] >= 0) and (np.abs(z[held] - 1.0) <= 1e-9).all()
        assert (n[held] == FRONT).all() and np.isnan(n[~held]).all() and np.isinf(z[~held]).all()
    z, n = seeded()
    o = pr.sweep_view(gray, K, Rp, t, z, n, 0, [1, 2], step=3, kd=0, ka=0, details=False, **KW)
    assert {tuple(q) for q in np.argwhere(o["best"] >= 0)} == {(24, 32), (24, 29), (24, 35), (21, 32), (27, 32)}
    assert o["best"][24, 35] == 1 and o["best"][24, 29] == 2 and o["best"][27, 32] == 3 and o["best"][21, 32] == 4


def test_the_choice_rule():
    nan = np.nan
    assert pr.choose(np.array([0.9, 0.9, 0.8])) == 0                # own kept on a tie
    assert pr.choose(np.array([0.9, 0.95, 0.95, 0.8])) == 1          # lowest h among the others
    assert pr.choose(np.array([0.9, 0.8, 0.7])) == 0
    assert pr.choose(np.array([nan, 0.8, nan, 0.8])) == 1
    assert pr.choose(np.array([nan, nan, nan, 0.1])) == 3
    assert pr.choose(np.array([0.5, nan, nan])) == 0
    assert pr.choose(np.array([nan, nan, nan])) == -1
    # the vectorised choice is this rule on every pixel
    gray, K, Rp, t = plane_scene()
    z, n = noisy_plane_maps()
    o = pr.sweep_view(gray, K, Rp, t, z, n, 0, [1, 2], details=False, **KW)
    want = np.array([[pr.choose(o["scores"][y, x]) for x in range(W)] for y in range(H)])
    assert np.array_equal(o["best"], want) and (want > 4).any() and ((want > 0) & (want < 5)).any() and (want < 0).any()


def test_the_top_k_rule_by_hand():
    nan = np.nan
    s, order = pr.topk_score(np.array([0.9, nan, 0.8, 0.95]), 0.7, 2)
    assert order == [3, 0] and s == (0.95 + 0.9) / 2               # an occluded view does not lower the score
    assert pr.topk_score(np.array([0.9, 0.8, 0.95, 0.6]), 0.7, 2)[0] == s
    s, order = pr.topk_score(np.array([0.9, 0.6, 0.5]), 0.7, 2)     # fewer than top_k passing views
    assert np.isnan(s) and order == []
    assert pr.topk_score(np.array([0.7, 0.9]), 0.7, 2)[1] == []     # ncc = min_ncc does not pass
    s, order = pr.topk_score(np.array([0.8, 0.9, 0.8, 0.8]), 0.7, 3)
    assert order == [1, 0, 2] and s == (0.9 + 0.8 + 0.8) / 3        # equal values in list order
    s, order = pr.topk_score(np.array([0.75, 0.9, 0.8]), 0.7, 3)
    assert order == [1, 2, 0] and s == ((0.9 + 0.8) + 0.75) / 3     # added in descending order
    assert pr.topk_score(np.array([-0.2]), -1.0, 1) == (-0.2, [0])


def test_what_yields_empty():
    gray, K, Rp, t = plane_scene()
    gray = gray.copy()
    gray[:, 36:, 50:] = 77                                           # a constant corner
    z, n = seeded()
    ref = lambda zz, nn, qx, qy, **kw: pr.pixel_reference(gray, K, Rp, t, zz, nn, 0, qx, qy, [1, 2], **dict(KW, kd=0, ka=0, **kw))
    good = ref(z, n, 32, 24)
    assert good["ok"] and good["best"] == 0 and good["score"] > 0.9 and good["z_out"] == 1.0
    # the border ring: the pixel holds a plane and still comes out empty
    for q in ((24, 1), (1, 32), (H - 2, 32), (24, W - 2)):
        z, n = seeded(q)
        o = ref(z, n, q[1], q[0])
        assert not o["ok"] and o["best"] == -1 and np.isinf(o["z_out"]) and np.isnan(o["scores"]).all(), q
    # ... but it is a valid source for its neighbour inside the ring
    z, n = seeded((1, 32))
    assert ref(z, n, 32, 2)["best"] == 3
    # a constant window
    z, n = seeded((40, 56))
    assert not ref(z, n, 56, 40)["ok"] and ref(z, n, 56, 40)["best"] == -1
    # a back-facing plane exists and is never valid
    z, n = seeded()
    n[24, 32] = [0.0, 0.0, 1.0]
    o = pr.pixel_reference(gray, K, Rp, t, z, n, 0, 32, 24, [1, 2], **KW)            # with the 3 x 3 x 3 grid
    assert o["ok"] and o["exists"][0] and o["exists"][5:].sum() == 26 and o["best"] == -1 and np.isnan(o["scores"]).all()
    # a neighbour whose normal is perpendicular to this pixel's ray: denominator 0
    z, n = seeded((24, 31))
    n[24, 31] = [1.0, 0.0, 0.0]
    o = ref(z, n, 32, 24)                                            # the ray of (32, 24) is (0, 0, 1)
    assert o["ok"] and not o["exists"].any() and o["best"] == -1
    # empty inputs: z <= 0, nan, inf, a nan normal component
    for bad in (-1.0, 0.0, np.nan, np.inf, -np.inf):
        z, n = seeded()
        z[24, 32] = bad
        assert not pr.holds(z, n).any() and ref(z, n, 32, 24)["best"] == -1 and ref(z, n, 33, 24)["best"] == -1
    z, n = seeded()
    n[24, 32, 1] = np.nan
    assert not pr.holds(z, n).any() and ref(z, n, 33, 24)["best"] == -1


@functools.lru_cache(maxsize=None)
def _noisy():
    rng = np.random.default_rng(11)
    z = np.where(rng.random((H, W)) < 0.4, 1.0 + rng.uniform(-0.004, 0.004, (H, W)), np.inf)
    n = np.full((H, W, 3), np.nan)
    m = np.isfinite(z)
    w = FRONT + rng.uniform(-0.15, 0.15, (int(m.sum()), 3)) * [1, 1, 0]
    n[m] = w / np.linalg.norm(w, axis=1, keepdims=True)
    true = m & (rng.random((H, W)) < 0.3)                            # some pixels hold the plane itself
    z[true], n[true] = 1.0, FRONT
    z[5, 5], z[6, 9], z[9, 6] = -1.0, 0.0, np.nan
    n[7, 7, 2] = np.nan
    return z, n


def noisy_plane_maps():
    z, n = _noisy()
    return z.copy(), n.copy()


@pytest.mark.parametrize("kw", [dict(step=1, kd=1, ka=1), dict(step=3, kd=0, ka=0, top_k=1),
                                dict(step=2, kd=2, ka=1, step_scale=0.5, depth_px=1.5, wid=1)])
def test_the_vectorised_restatement_is_the_per_pixel_one(kw):
    """sweep_view against pixel_reference on every pixel of a 20 x 24 block that
    reaches the border ring (and on the whole image's choice)."""
    gray, K, Rp, t = plane_scene()
    z, n = noisy_plane_maps()
    k = dict(KW, **kw)
    o = pr.sweep_view(gray, K, Rp, t, z, n, 0, [1, 2], **k)
    scored = 0
    for qy in range(0, 20):
        for qx in range(0, 24):
            p = pr.pixel_reference(gray, K, Rp, t, z, n, 0, qx, qy, [1, 2], **k)
            assert p["ok"] == o["ok"][qy, qx] and np.array_equal(p["exists"], o["exists"][qy, qx]), (qx, qy)
            e = p["exists"]
            assert np.allclose(p["zh"][e], o["zh"][qy, qx][e], rtol=1e-15, atol=0)
            assert np.allclose(p["nh"][e], o["nh"][qy, qx][e], rtol=0, atol=1e-15)
            for key, tol in (("scores", 1e-12), ("ncc", 1e-12), ("sigma_b", 1e-9), ("border", 1e-9), ("cosm", 1e-14)):
                a, b = p[key], o[key][qy, qx]
                assert np.array_equal(np.isnan(a), np.isnan(b)), (key, qx, qy)
                both = ~np.isnan(a) & np.isfinite(a)
                assert np.allclose(a[both], b[both], rtol=0, atol=tol), (key, qx, qy)
            for h in range(len(e)):
                assert sorted(p["chosen"][h]) == list(np.nonzero(o["chosen"][qy, qx, h])[0]), (qx, qy, h)
            scored += int((~np.isnan(p["scores"])).sum())
            # equal scores are common (the grid's k = 0 normals see the same window): the choices agree in score
            if p["best"] != o["best"][qy, qx]:
                assert abs(o["scores"][qy, qx][p["best"]] - o["score"][qy, qx]) <= 1e-12, (qx, qy)
            else:
                assert p["best"] < 0 or (p["z_out"] == o["z_out"][qy, qx] or
                                         abs(p["z_out"] - o["z_out"][qy, qx]) <= 1e-15), (qx, qy)
    assert scored > 500


def test_view_lists_are_the_seed_pairs_rows(pkg):
    lib = pkg._lib
    _, _, R, _ = pkg.synthetic.sphere_scene(V=24, H=24, W=32, rad=RAD, n_seeds=0)[:4]
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    for tv, cosv in ((4, 0.5), (6, 0.9), (2, 0.5), (32, 0.0)):
        pairs = lib.seed_view_pairs(Rp, tv, cosv)
        lists = lib.wprop_view_lists(Rp, tv, cosv)
        assert lists.shape == (24, tv) and lists.dtype == np.int32
        for r in range(24):
            want = [int(v) for a, v in pairs if a == r]
            assert list(lists[r, :len(want)]) == want and (lists[r, len(want):] == -1).all(), (tv, r)
            assert r not in want and len(set(want)) == len(want)
        sub = lib.wprop_view_lists(Rp, tv, cosv, 5, 3)
        assert np.array_equal(sub, lists[5:8])
    assert (lib.wprop_view_lists(Rp, 6, 0.9)[:, -1] == -1).all()     # 15 degrees apart: four views within cos 0.9
    assert (lib.wprop_view_lists(Rp, 4, 0.5) >= 0).all()


# ---------------------------------------------------------------------------
# quality on the sphere scene
# ---------------------------------------------------------------------------
QV = 6      # the view range 0..5 with lists inside it: the full 24-view run takes minutes on the CPU
QWID = 3    # the window of the issue's prototype (wid 5 costs 2.5 times as much here)


@functools.lru_cache(maxsize=None)
def quality_inputs(pkg):
    """The 24-view 96 x 128 sphere, the restatement's radius-1 splat of the
    unrefined 442-patch chain over the views 0..QV-1, and the lists of the
    pair rule applied to those views alone."""
    rgb, Ks, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    t = np.asarray(t, np.float64).reshape(-1, 3)
    gray = wr.gray_stack(rgb)
    s = fr.mixed_set(gray, Ks, R, t, Rp, RAD)
    chain = {k: s[k][s["kind"] == 0] for k in ("c", "nrm", "ref", "mask")}
    res = dr.depth_chain(Ks, Rp, t, 128, 96, rgb, chain, radius=1, views=(0, QV))
    lists = pkg._lib.wprop_view_lists(Rp[:QV], 4, 0.5)
    return {"gray": gray, "cam": (Ks, Rp, t), "z": res["z"], "normal": res["normal"], "lists": lists,
            "fused_before": len(res["pix"])}


# measured by test_quality_on_the_sphere_chain (its printed lines): (coverage, median, p95)
RECORDED = {"splat": (0.0610, 0.3891, 1.1437), "after": (0.3635, 0.2431, 2.9520), "fused": (0.3494, 0.2323, 2.2565)}


def assert_quality(before, after, fused):
    """The recorded figures with the factor 2 of DESIGN 4.7 / 4.11 (the margin
    guards the restatement against later edits), and the two statements that make
    the feature worth having: at least 3 times the splat's coverage at no more
    than the splat's median error."""
    for got, key in ((before, "splat"), (after, "after"), (fused, "fused")):
        cov, med, p95 = RECORDED[key]
        assert got[0] >= cov / 2 and got[1] <= med * 2 and got[2] <= p95 * 2, (key, got)
    assert after[0] >= 3 * before[0] and after[1] <= before[1]
    assert fused[0] >= 3 * before[0] and fused[1] <= before[1]


def test_quality_on_the_sphere_chain(pkg):
    """The default schedule (12 sweeps) on the views 0..5 of the quality test's
    sphere at wid 3, lists of the 4 nearest views inside the range, best 2 views
    above 0.7, min_cos 0.3, against the analytic depth; then the consistency count
    at the defaults.  Measured here (the bounds are these with a factor of 2):
      splat:  6.10 % of the hit pixels hold a depth, median 0.389 and 95th percentile 1.144 footprints;
      after:  36.35 %, 0.243, 2.952 (6.0 times the coverage at 0.62 times the median error);
      fused:  34.94 %, 0.232, 2.257.
    The tail grows (the 95th percentile doubles): planes carried across the
    silhouette and a few low-texture pixels; the consistency count trims some of it."""
    q = quality_inputs(pkg)
    Ks, Rp, t = q["cam"]
    before = depth_quality(Ks[:QV], Rp[:QV], t[:QV], q["z"], RAD)
    out = pr.chain(q["gray"], Ks, Rp, t, q["z"], q["normal"], 0, q["lists"], wid=QWID)
    after = depth_quality(Ks[:QV], Rp[:QV], t[:QV], out["z"], RAD)
    cons, viol = dr.consist_fast(Ks, Rp, t, 128, 96, out["z"], 0, QV, 0.01)
    sel = np.isfinite(out["z"]) & (cons >= 2) & (viol <= 0)
    fused = depth_quality(Ks[:QV], Rp[:QV], t[:QV], out["z"], RAD, sel)
    print(f"splat {before}\nafter {after}\nfused {int(sel.sum())} px {fused}\nhistory {out['history'].tolist()}")
    assert_quality(before, after, fused)
    hist = out["history"]
    assert hist[-1, 0] == int(np.isfinite(out["z"]).sum()) and (np.diff(hist[:, 0]) > 0).all()
