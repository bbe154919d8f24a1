"""The float64 restatement of the plane-warped photo test
(tests/warped_reference.py) on its own, without a GPU: the properties the GPU
tests rely on when they compare mvs_score_warped against it."""
import numpy as np
import pytest

import warped_reference as wr


@pytest.fixture(scope="module")
def sphere(pkg):
    rgb, K, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=0.02)[:4]
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    return wr.gray_stack(rgb), K, R, t, Rp


def _two_camera_scene(rng, H=40, W=48):
    K = np.tile(np.array([[300.0, 0, 24.0], [0, 310.0, 20.0], [0, 0, 1.0]]), (2, 1, 1))
    Rp = np.tile(np.eye(3), (2, 1, 1))
    t = np.tile(np.array([0.01, -0.02, 0.0]), (2, 1))
    gray = np.tile(rng.integers(0, 256, (1, H, W), dtype=np.uint8), (2, 1, 1))
    return gray, K, Rp, t


@pytest.mark.parametrize("wid", [1, 3, 5])
def test_identity_warp(wid):
    """Two identical cameras and a fronto-parallel patch: the warp is the
    identity, the windows are equal and ncc is ctNcc's N / (N - 1)."""
    rng = np.random.default_rng(0)
    gray, K, Rp, t = _two_camera_scene(rng)
    N = (2 * wid + 1) ** 2
    for _ in range(20):
        x, y = rng.uniform(wid + 1, 48 - wid - 2), rng.uniform(wid + 1, 40 - wid - 2)
        z = rng.uniform(0.5, 2.0)
        c = np.array([(x - 24.0) / 300.0 * z, (y - 20.0) / 310.0 * z, z]) - t[0]
        o = wr.warped_reference(gray, K, Rp, t, c, [0, 0, -1.0], 0, wid, 0.0)
        assert o["valid"] and o["border"][1] >= 0
        assert abs(o["ncc"][1] - N / (N - 1)) <= 1e-9
        assert np.isnan(o["ncc"][0])


def test_two_forms_agree(pkg):
    """The homography of the patch plane and the ray-plane construction give
    the same sample positions within 1e-11 px at dinoRing-sized ring cameras
    (2,000 random patches, every view that keeps the warped window inside the
    image)."""
    V, H, W = 48, 480, 640
    K, R, t = pkg.synthetic.ring_cameras(V, H, W)
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    O = wr.centres(Rp, t)
    c, ref = pkg.synthetic.candidates(2000, K, R, t, W=W, H=H, seed=1)
    rng = np.random.default_rng(1)
    worst, pairs = 0.0, 0
    for i in range(len(ref)):
        r = int(ref[i])
        n = O[r] - c[i]
        n = n / np.linalg.norm(n) + rng.normal(0, 0.2, 3)
        n /= np.linalg.norm(n)
        x, y, _ = wr.project_ref(K[r], Rp[r], t[r], c[i])
        q = wr.window_pixels(int(x), int(y), 5)
        for v in rng.choice(V, 6, replace=False):
            if v == r or n @ (O[v] - c[i]) <= 0.3 * np.linalg.norm(O[v] - c[i]):
                continue
            p1, z = wr.positions_rayplane(K, Rp, t, c[i], n, r, v, q)
            if not (np.all(z > 0) and p1.min() >= 0 and p1[:, 0].max() <= W - 1 and p1[:, 1].max() <= H - 1):
                continue
            p2 = wr.positions_homography(K, Rp, t, c[i], n, r, v, q)
            worst = max(worst, float(np.abs(p1 - p2).max()))
            pairs += 1
    print(f"two forms: {pairs} pairs, worst difference {worst:.3e} px")
    assert pairs > 1000
    assert worst <= 1e-11


def _shares(gray, K, R, t, Rp, shift, wid=5, min_ncc=0.7, min_cos=0.3, n=300):
    c, nrm, ref, _ = wr.sphere_patches(K, R, t, n, 0.02, np.random.default_rng(1), (shift,))
    o = wr.warped_batch(gray, K, Rp, t, c, nrm, ref, wid, min_cos)
    passing = (o["ncc"] > min_ncc).sum(1)
    return float((passing >= 3).mean()), float(passing.mean())


def test_sphere_discrimination(sphere):
    """The test separates surface from non-surface on the textured sphere
    (V=24, 96x128, radius 20 mm; 300 patches facing their reference camera,
    true normals, wid 5, min_ncc 0.7, min_cos 0.3, rng seed 1): on the surface
    at least 85 % of the patches keep 3 or more views, 2 mm off it at most 40 %."""
    gray, K, R, t, Rp = sphere
    on = _shares(gray, K, R, t, Rp, 0.0)
    out = _shares(gray, K, R, t, Rp, 0.002)
    inn = _shares(gray, K, R, t, Rp, -0.002)
    print(f"share with >= 3 views / mean views: on {on}, +2 mm {out}, -2 mm {inn}")
    assert on[0] >= 0.85
    assert out[0] <= 0.40
    assert inn[0] <= 0.40


def test_flat_warped_window_fails():
    """A warped window that falls on a constant region has D_b = 0 exactly (the
    difference-form interpolation returns a constant neighbourhood exactly)
    and fails, at sub-pixel sample positions too."""
    rng = np.random.default_rng(2)
    H, W = 40, 48
    K = np.tile(np.array([[300.0, 0, 24.0], [0, 300.0, 20.0], [0, 0, 1.0]]), (2, 1, 1))
    Rp = np.tile(np.eye(3), (2, 1, 1))
    t = np.array([[0.0, 0, 0], [0.0123, 0.0071, 0]])   # view 1 shifted: sub-pixel sample positions
    gray = np.stack([rng.integers(0, 256, (H, W), dtype=np.uint8), np.full((H, W), 37, np.uint8)])
    c = np.array([0.0, 0.0, 1.0])
    o = wr.warped_reference(gray, K, Rp, t, c, [0, 0, -1.0], 0, 5, 0.0)
    assert o["valid"] and o["border"][1] >= 0
    assert o["sigma_b"][1] == 0.0 and np.isnan(o["ncc"][1])
    # and the bilinear form itself, on a constant image at random positions
    b = wr.bilinear(np.full((H, W), 201.0), rng.uniform(0, W - 1, 1000), rng.uniform(0, H - 1, 1000))
    assert np.all(b == 201.0)
