"""The float64 restatement of the depth and normal refinement
(tests/refine_reference.py) on its own, without a GPU: the properties the GPU
tests rely on when they compare mvs_refine_warped against it."""
import math

import numpy as np
import pytest

import refine_reference as rr
import warped_reference as wr


@pytest.fixture(scope="module")
def sphere(pkg):
    rgb, K, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=0.02)[:4]
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    return wr.gray_stack(rgb), K, R, t, Rp


def test_single_hypothesis_is_the_warped_test(sphere):
    """kd = ka = 0: the one hypothesis is the input patch, and its score is the
    mean over the list, in list order, of warped_reference's ncc -- exactly."""
    gray, K, R, t, Rp = sphere
    c, nrm, ref, _ = wr.sphere_patches(K, R, t, 12, 0.02, np.random.default_rng(1), (0.0, 0.0005))
    o = wr.warped_batch(gray, K, Rp, t, c, nrm, ref, 3, 0.0)
    views = rr.view_lists(o["ncc"], 0.7, 8)
    scored = 0
    for i in range(len(ref)):
        lst = [int(v) for v in views[i] if v >= 0]
        out = rr.refine_level_reference(gray, K, Rp, t, c[i], nrm[i], ref[i], views[i], 0.0008, 3, 0.0, 0, 0)
        assert out["H"] == 1 and out["scores"].shape == (1,)
        if not lst:
            assert not out["valid"] and out["best"] == -1 and np.isnan(out["scores"][0])
            continue
        total = 0.0
        for v in lst:
            total = total + o["ncc"][i, v]
        assert out["scores"][0] == total / len(lst)
        assert out["best"] == 0 and out["score_best"] == out["scores"][0]
        assert np.array_equal(out["c_out"], c[i]) and np.array_equal(out["nrm_out"], nrm[i])
        scored += 1
    assert scored >= 8


def test_view_list_rule():
    ncc = np.array([[0.9, np.nan, 0.8, 0.8, 0.95, 0.5, 0.8],
                    [np.nan, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    got = rr.view_lists(ncc, 0.7, 3)
    assert got.dtype == np.int32
    assert got.tolist() == [[0, 2, 4], [-1, -1, -1]]          # the tie 0.8/0.8/0.8 goes to view 2
    assert rr.view_lists(ncc, 0.7, 8)[0].tolist() == [0, 2, 3, 4, 6, -1, -1, -1]
    assert rr.list_ok([3, 5, -1], 8, 0) and not rr.list_ok([3, -1, 5], 8, 0)
    assert not rr.list_ok([3, 3, -1], 8, 0) and not rr.list_ok([3, 0, -1], 8, 0) and not rr.list_ok([8], 8, 0)


@pytest.mark.parametrize("nrm", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (1, -1, 0), (0.3, -0.5, 0.81)])
def test_grid_geometry(nrm):
    """e1, e2 and nrm are orthonormal (axis normals and equal-component ties
    included); the angle between n_i0 and nrm is |i| alpha; every c_k projects
    into the reference view within 1e-9 px of c."""
    nrm = np.array(nrm, np.float64)
    nrm /= np.linalg.norm(nrm)
    e1, e2 = rr.tangent_basis(nrm)
    G = np.array([nrm, e1, e2])
    assert np.abs(G @ G.T - np.eye(3)).max() <= 1e-15
    assert abs(np.linalg.det(G) - 1.0) <= 1e-15               # right-handed: e2 = nrm x e1
    Kr = np.array([[660.0, 0, 64.0], [0, 650.0, 48.0], [0, 0, 1.0]])
    Rpr, tr = np.eye(3), np.array([0.01, -0.02, 0.33])
    O = -Rpr.T @ tr
    c = np.array([0.004, -0.003, 0.01])
    kd, ka, astep, scale = 3, 2, math.radians(8), 0.5
    ck, nij = rr.grid(c, nrm, O, 0.0008, kd, ka, astep, scale)
    A = 2 * ka + 1
    assert len(ck) == (2 * kd + 1) * A * A
    hc = (len(ck) - 1) // 2
    assert np.array_equal(ck[hc], c) and np.array_equal(nij[hc], nrm)
    x, y, _ = wr.project_ref(Kr, Rpr, tr, c)
    for k in range(-kd, kd + 1):
        for j in range(-ka, ka + 1):
            for i in range(-ka, ka + 1):
                h = ((k + kd) * A + (j + ka)) * A + (i + ka)
                assert abs(np.linalg.norm(nij[h]) - 1.0) <= 1e-15
                if j == 0:
                    ang = math.atan2(np.linalg.norm(np.cross(nij[h], nrm)), nij[h] @ nrm)
                    assert abs(ang - abs(i) * astep * scale) <= 1e-14
                xk, yk, _ = wr.project_ref(Kr, Rpr, tr, ck[h])
                assert abs(xk - x) <= 1e-9 and abs(yk - y) <= 1e-9
                assert abs(np.linalg.norm(ck[h] - c) - abs(k) * 0.0008 * scale) <= 1e-15


def test_choice_rule():
    ck = np.arange(15.0).reshape(5, 3)
    nij = -ck
    c, nrm = ck[2], nij[2]
    nan = np.nan
    assert rr.choose(np.array([0.5, 0.7, 0.7, 0.7, 0.1]), ck, nij, c, nrm)["best"] == 2     # ties keep the centre
    assert rr.choose(np.array([0.5, 0.8, 0.7, 0.8, 0.1]), ck, nij, c, nrm)["best"] == 1     # lowest index of a tie
    assert rr.choose(np.array([nan, nan, nan, 0.2, 0.1]), ck, nij, c, nrm)["best"] == 3     # centre invalid
    o = rr.choose(np.full(5, nan), ck, nij, c, nrm)
    assert o["best"] == -1 and np.isnan(o["score_best"]) and np.array_equal(o["c_out"], c)
    o = rr.choose(np.array([0.5, 0.8, 0.7, 0.9, 0.1]), ck, nij, c, nrm)
    assert o["best"] == 3 and o["score_best"] == 0.9 and np.array_equal(o["c_out"], ck[3])


def test_sphere_recovery(sphere):
    """Sphere scene (V 24, 96x128), seed 1, 48 patches moved by U(-1.5, 1.5) mm
    along their reference ray and tilted by U(5, 15) degrees; lists from the
    wrapper's rule (min_ncc 0.7, 8 views) on the perturbed patches; wid 3, the
    45-hypothesis grid (kd 2, ka 1), 4 levels from 0.8 mm and 8 degrees.  The
    median depth error and the median angle error must at least halve."""
    gray, K, R, t, Rp = sphere
    c0, n0, ref, c, nrm = rr.perturbed_sphere_patches(K, R, t, Rp, 48, np.random.default_rng(1))
    o = wr.warped_batch(gray, K, Rp, t, c, nrm, ref, 3, 0.0)
    views = rr.view_lists(o["ncc"], 0.7, 8)
    d0, a0 = rr.patch_errors(c, nrm, c0, n0)
    c1, n1, best = rr.refine_reference(gray, K, Rp, t, c, nrm, ref, views, np.full(48, 0.0008), 3, 0.0, 4, 2, 1,
                                       math.radians(8))
    d1, a1 = rr.patch_errors(c1, n1, c0, n0)
    T = (views >= 0).sum(1)
    print(f"median depth error {np.median(d0) * 1e3:.3f} -> {np.median(d1) * 1e3:.3f} mm, "
          f"median angle error {np.median(a0):.2f} -> {np.median(a1):.2f} deg; |T| {T.min()}..{T.max()}, "
          f"{int((T == 0).sum())} empty lists, {int((best < 0).sum())} (patch, level) without a valid hypothesis")
    assert np.median(d1) <= 0.5 * np.median(d0)
    assert np.median(a1) <= 0.5 * np.median(a0)
