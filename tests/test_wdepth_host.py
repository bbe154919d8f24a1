"""The float64 restatement of the depth maps (tests/depth_reference.py) on its
own, without a GPU: the rules the GPU tests rely on when they compare
mvs_wdepth_splat_device, mvs_wdepth_consist_device, mvs_wdepth_points_device and
MvsContext.depth_maps against it, and the quality experiment on the sphere scene
whose figures stand in DESIGN 4.11."""
import numpy as np
import pytest

import depth_reference as dr
import filter_reference as fr
import warped_reference as wr

RAD = 0.02
W, H = 64, 48
# test_wfilt_host's two cameras facing each other along z: camera 0 at the origin
# looking down +z, camera 1 at (0, 0, 1) looking down -z (a half turn about x)
K = np.array([[[300.0, 0, 31.3], [0, 310.0, 23.9], [0, 0, 1.0]]] * 2)
RP = np.array([np.eye(3), np.diag([1.0, -1.0, -1.0])])
T = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
TOWARDS0 = [0.0, 0.0, -1.0]
FBAR = 305.0


def at_pixel(qx, qy, z):
    """The point of depth z on the ray of pixel (qx, qy) of camera 0."""
    return [(qx - 31.3) / 300.0 * z, (qy - 23.9) / 310.0 * z, z]


def run(c, nrm, ref, mask, radius=1, slope=4.0, v0=0, nv=2):
    c = np.asarray(c, np.float64).reshape(-1, 3)
    return dr.splat(K, RP, T, W, H, c, np.asarray(nrm, np.float64).reshape(-1, 3), np.asarray(ref, np.int32),
                    np.asarray(mask, np.uint64).reshape(len(c), 1), radius, slope, v0, nv)


def test_a_fronto_parallel_patch_is_flat():
    for radius in (0, 1, 2, 3):
        z, idm = run([at_pixel(20, 30, 0.5)], [TOWARDS0], [0], [0], radius)
        got = np.argwhere(idm[0] == 0)
        side = 2 * radius + 1
        assert len(got) == side * side and (idm[1] == -1).all() and np.isinf(z[1]).all()
        assert got.min(0).tolist() == [30 - radius, 20 - radius] and got.max(0).tolist() == [30 + radius, 20 + radius]
        assert (z[0][idm[0] == 0] == 0.5).all()                 # s = z to the bit over the whole footprint
        assert np.isinf(z[0][idm[0] < 0]).all()
    # the footprint is clipped at the image corner, and a view outside the range draws nothing
    z, idm = run([at_pixel(0.2, 47.3, 0.5)], [TOWARDS0], [0], [0], 2)
    assert np.argwhere(idm[0] == 0).tolist() == [[y, x] for y in (45, 46, 47) for x in (0, 1, 2)]
    z, idm = run([at_pixel(20, 30, 0.5)], [TOWARDS0], [0], [0], 1, v0=1, nv=1)
    assert z.shape == (1, H, W) and (idm == -1).all()


def test_a_tilted_patch_follows_its_plane_and_the_slope_guard_cuts_by_hand():
    """n = (0.96, 0, -0.28) at depth 0.5 through pixel (31, 24): along the row the
    plane's depth is s(dx) = 0.5 den(0) / den(dx) with den(dx) = den(0) + 0.96 dx / 300
    and den(0) = 0.96 (31 - 31.3) / 300 - 0.28 = -0.28096: s changes by +0.5 (0.0032 dx) /
    (0.28096 - 0.0032 dx), in footprints of 0.5 / 305: 3.51 and 7.11 and 10.78 at dx = 1, 2, 3, and
    -3.43, -6.79, -10.07 at dx = -1, -2, -3 (the normal has no y component: the same in every row).
    slope 3 allows 3 (m + 1) = 6, 9, 12 at m = max(|dx|, |dy|) = 1, 2, 3: everything passes.
    slope 1.7 allows 3.4, 5.1, 6.8: dx = 0 always passes; dx = +-1 (3.51, 3.43) needs m >= 2, the
    rows |dy| >= 2; dx = -2 (6.79) needs m = 3, the rows |dy| = 3; dx = +2 (7.11) and +-3 never."""
    n = [0.96, 0.0, -0.28]
    c = at_pixel(31, 24, 0.5)
    z, idm = run([c], [n], [0], [0], 3, slope=3.0)
    assert (idm[0, 21:28, 28:35] == 0).all() and (idm[0] == 0).sum() == 49
    for qy in range(21, 28):
        for qx in range(28, 35):
            d = np.array([(qx - 31.3) / 300.0, (qy - 23.9) / 310.0, 1.0])
            want = (np.array(n) @ np.array(c)) / (np.array(n) @ d)
            assert abs(z[0, qy, qx] - want) <= 1e-13 * want
    steps = (z[0, 24, 28:35] - 0.5) / (0.5 / FBAR)
    assert np.allclose(steps, [-10.07, -6.79, -3.43, 0.0, 3.51, 7.11, 10.78], atol=0.01)
    z, idm = run([c], [n], [0], [0], 3, slope=1.7)
    want = [[24 + dy, 31 + dx] for dy in range(-3, 4) for dx in range(-3, 4)
            if dx == 0 or (abs(dx) == 1 and abs(dy) >= 2) or (dx == -2 and abs(dy) == 3)]
    assert len(want) == 17 and np.argwhere(idm[0] == 0).tolist() == want
    # a slope so small that only the column without a depth change is left; with a tilt in y as well (0.6 / 300
    # against 0.6 / 310 per pixel: no two pixels of the footprint share a depth) only the centre pixel
    z, idm = run([c], [n], [0], [0], 3, slope=1e-3)
    assert np.argwhere(idm[0] == 0).tolist() == [[y, 31] for y in range(21, 28)]
    z, idm = run([c], [[0.6, 0.6, -0.53]], [0], [0], 3, slope=1e-3)
    assert np.argwhere(idm[0] == 0).tolist() == [[24, 31]] and abs(z[0, 24, 31] - 0.5) < 1e-15


def test_the_nearer_patch_wins_and_ties_go_to_the_lowest_index():
    c = [at_pixel(20, 30, 0.6), at_pixel(20, 30, 0.4), at_pixel(20, 30, 0.5)]
    z, idm = run(c, [TOWARDS0] * 3, [0, 0, 0], [0, 0, 0])
    assert (idm[0, 29:32, 19:22] == 1).all() and (z[0, 29:32, 19:22] == 0.4).all()
    same = [at_pixel(20, 30, 0.6)] + [at_pixel(20, 30, 0.5)] * 3
    z, idm = run(same, [TOWARDS0] * 4, [0] * 4, [0] * 4)
    assert (idm[0, 29:32, 19:22] == 1).all()
    z, idm = run(same[::-1], [TOWARDS0] * 4, [0] * 4, [0] * 4)
    assert (idm[0, 29:32, 19:22] == 0).all()


def test_what_draws_nothing():
    c = at_pixel(20, 30, 0.5)
    for nrm, ref, mask, why in (([0.0, 0.0, 1.0], 0, 0, "back-facing"),
                                (TOWARDS0, -1, 1, "dead row"), (TOWARDS0, 2, 1, "dead row, ref = V"),
                                ([np.nan, 0.0, -1.0], 0, 0, "nan normal")):
        z, idm = run([c], [nrm], [ref], [mask])
        assert (idm == -1).all() and np.isinf(z).all(), why
    # behind the camera, and mask bits >= V name no view
    z, idm = run([[0, 0, -0.5]], [TOWARDS0], [0], [0xFFFC])
    assert (idm == -1).all()
    # a normal perpendicular to the centre pixel's ray: den = 0 there and h = 0, so nothing is drawn
    d = np.array([(20 - 31.3) / 300.0, (30 - 23.9) / 310.0, 1.0])
    n = np.array([1.0, 0.0, -d[0]])
    assert n @ d == 0.0
    z, idm = run([(d * 0.5).tolist()], [n.tolist()], [0], [0], 0)
    assert (idm == -1).all()
    # it faces camera 1 only: view 0 stays empty though the mask names it
    z, idm = run([c], [[0.0, 0.0, 1.0]], [0], [2])
    assert (idm[0] == -1).all() and (idm[1] == 0).sum() == 9


def test_consistency_rules():
    """Both cameras look at the plane z = 0.5 from opposite sides, so camera 1's
    depth of a point at z is 1 - z."""
    both = np.full((2, H, W), 0.5)
    for fn in (dr.consist, dr.consist_fast):
        # two views of one plane agree (inside the part of it both images hold)
        cons, viol = fn(K, RP, T, W, H, both, 0, 2, 0.01)
        assert (cons[:, 8:40, 8:56] == 1).all() and not viol.any()
        # a plane behind another: camera 0's points at z = 0.5 lie at depth 0.5 in camera 1, whose map
        # holds 0.3 there: occluded, no violation; camera 1's points at z = 0.7 are hidden from camera 0
        z = both.copy()
        z[1] = 0.3
        cons, viol = fn(K, RP, T, W, H, z, 0, 2, 0.01)
        assert not cons.any() and not viol.any()
        # a point floating in front of a surface: camera 0 claims z = 0.5, camera 1 claims to see past it
        # to depth 0.9 (z = 0.1): a violation of camera 0's pixels in camera 1, and of camera 1's in camera
        # 0, which claims to see past z = 0.1 to its 0.5
        z = both.copy()
        z[1] = 0.9
        cons, viol = fn(K, RP, T, W, H, z, 0, 2, 0.01)
        assert (viol[0, 8:40, 8:56] == 1).all() and not cons.any()
        assert viol[1, 24, 31] == 1                                  # (most of camera 1's points leave camera 0's image)
        # one pixel of camera 0 at z = 0.8 floats 0.2 in front of camera 1, whose surface lies at 0.5: camera 1
        # sees through it, and camera 0 claims to see through the one point of camera 1's plane on that ray
        z = both.copy()
        z[0, 24, 31] = 0.8
        cons, viol = fn(K, RP, T, W, H, z, 0, 2, 0.01)
        assert viol[0, 24, 31] == 1 and cons[0, 24, 31] == 0 and viol[0].sum() == 1 and viol[1].sum() == 1
        # the same pixel at z = 0.3 lies behind camera 1's surface: occluded, and it hides one point from camera 0
        z[0, 24, 31] = 0.3
        cons, viol = fn(K, RP, T, W, H, z, 0, 2, 0.01)
        assert not viol.any() and cons[0, 24, 31] == 0 and (cons[1, 8:40, 8:56] == 0).sum() == 1
        # within rel_tol it agrees, just outside it does not: depth 0.5, tolerance 0.005
        z = both.copy()
        z[1] = 0.5049
        assert (fn(K, RP, T, W, H, z, 0, 2, 0.01)[0][0, 8:40, 8:56] == 1).all()
        z[1] = 0.5051
        cons, viol = fn(K, RP, T, W, H, z, 0, 2, 0.01)
        assert not cons[0].any() and (viol[0, 8:40, 8:56] == 1).all()
        # a hole in u is unknown
        z = both.copy()
        z[1] = np.inf
        z[1, 0, 0] = np.nan
        cons, viol = fn(K, RP, T, W, H, z, 0, 2, 0.01)
        assert not cons.any() and not viol.any()
        # a range of one view: the self view is skipped
        cons, viol = fn(K, RP, T, W, H, both[:1], 0, 1, 0.01)
        assert not cons.any() and not viol.any()


def test_consist_fast_is_consist_to_the_byte():
    rng = np.random.default_rng(3)
    z = np.full((2, H, W), 0.5) + rng.choice([0.0, 0.004, -0.004, 0.2], (2, H, W), p=[0.7, 0.1, 0.1, 0.1])
    z[rng.random((2, H, W)) < 0.1] = np.inf
    z[0, 3, 3], z[0, 4, 4], z[1, 5, 5], z[1, 6, 6] = np.nan, -1.0, 0.0, -np.inf
    for tol in (0.0, 0.01):
        a, b = dr.consist(K, RP, T, W, H, z, 0, 2, tol), dr.consist_fast(K, RP, T, W, H, z, 0, 2, tol)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[0].any() and a[1].any()
    assert a[0][0, 4, 4] == 0 and a[0][1, 5, 5] == 0 and a[1][0, 4, 4] == 0


def test_points_and_the_fusion_rule():
    rgb = np.random.default_rng(0).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    c = [at_pixel(20, 30, 0.5), at_pixel(40, 10, 0.5)]
    patches = {"c": np.array(c), "nrm": np.array([TOWARDS0, [0.0, 0.0, 1.0]]), "ref": np.array([0, 1], np.int32),
               "mask": np.array([[0], [0]], np.uint64)}
    z, idm = dr.splat(K, RP, T, W, H, patches["c"], patches["nrm"], patches["ref"], patches["mask"], 1, 4.0)
    pix = np.array([[0, 20, 30], [0, 0, 0], [1, 40, 37]], np.int32)      # camera 1 flips y: 47.8 - 10 = 37.8
    assert idm[0, 30, 20] == 0 and idm[1, 38, 40] == 1
    xyz, col = dr.points(K, RP, T, W, H, rgb, z, 0, 2, pix)
    assert np.allclose(xyz[0], c[0], rtol=0, atol=1e-15) and np.isnan(xyz[1]).all() and not col[1].any()
    assert np.array_equal(col[0], rgb[0, 30, 20]) and np.array_equal(col[2], rgb[1, 37, 40])
    # the fusion rule: only the reference view of the drawing patch emits the pixel
    cons = np.full(idm.shape, 2, np.uint8)
    viol = np.zeros(idm.shape, np.uint8)
    got = dr.fuse(idm, cons, viol, patches["ref"], 0)
    assert len(got) == 18 and set(got[:, 0].tolist()) == {0, 1}
    assert len(dr.fuse(idm, cons, viol, np.array([1, 0], np.int32), 0)) == 0
    assert len(dr.fuse(idm, cons - 1, viol, patches["ref"], 0)) == 0
    viol[0, 30, 20] = 1
    assert len(dr.fuse(idm, cons, viol, patches["ref"], 0)) == 17
    assert len(dr.fuse(idm, cons, viol, patches["ref"], 0, max_violations=1)) == 18
    # a range that starts at view 1
    got1 = dr.fuse(idm[1:], cons[1:], viol[1:], patches["ref"], 1)
    assert np.array_equal(got1, got[got[:, 0] == 1])


def test_the_files_of_a_result(pkg, tmp_path):
    """MVS2.write_depth_maps: depth_%04d.npy (float32, nan = empty), normal_%04d.npy and the fused cloud."""
    rgb = np.zeros((2, H, W, 3), np.uint8)
    patches = {"c": np.array([at_pixel(20, 30, 0.5)]), "nrm": np.array([TOWARDS0]), "ref": np.array([0], np.int32),
               "mask": np.array([[0]], np.uint64)}
    res = dr.depth_chain(K, RP, T, W, H, rgb, patches, views=(0, 2), min_consistent=0)
    assert len(res["pix"]) == 9
    pkg.MVS2.write_depth_maps(res, str(tmp_path / "maps"), dense_path=str(tmp_path / "dense"))
    for v in (0, 1):
        z = np.load(tmp_path / "maps" / ("depth_%04d.npy" % v))
        n = np.load(tmp_path / "maps" / ("normal_%04d.npy" % v))
        assert z.dtype == np.float32 and z.shape == (H, W) and n.dtype == np.float32 and n.shape == (H, W, 3)
        assert np.array_equal(np.isnan(z), res["id"][v] < 0) and np.array_equal(np.isnan(n[..., 0]), res["id"][v] < 0)
    assert (np.load(tmp_path / "maps" / "depth_0000.npy")[29:32, 19:22] == np.float32(0.5)).all()
    pts, nrm, col = pkg.read_ply_oriented(str(tmp_path / "dense.ply"))
    assert np.array_equal(pts, res["points"]) and np.array_equal(nrm, res["normals"]) and len(col) == 9


# ---------------------------------------------------------------------------
# quality on the sphere scene
# ---------------------------------------------------------------------------
def depth_quality(K_, Rp, t, z, rad, select=None):
    """(coverage, median, 95th percentile) of a stack of depth maps over every
    view's analytically hit pixels: the share of them that hold a depth (and are
    selected), and |z - analytic depth| over those in pixel footprints
    (analytic depth / ((fx + fy) / 2))."""
    hit = covered = 0
    err = []
    for v in range(len(z)):
        za = dr.sphere_depth(K_, Rp, t, z.shape[2], z.shape[1], v, rad)
        on = np.isfinite(za)
        got = on & np.isfinite(z[v]) & (True if select is None else select[v])
        hit += int(on.sum())
        covered += int(got.sum())
        fbar = (float(K_[v][0, 0]) + float(K_[v][1, 1])) / 2
        err.append(np.abs(z[v][got] - za[got]) / (za[got] / fbar))
    err = np.concatenate(err)
    return covered / hit, float(np.median(err)), float(np.percentile(err, 95))


@pytest.fixture(scope="module")
def quality(pkg):
    rgb, Ks, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    t = np.asarray(t, np.float64).reshape(-1, 3)
    s = fr.mixed_set(wr.gray_stack(rgb), Ks, R, t, Rp, RAD)
    chain = {k: s[k][s["kind"] == 0] for k in ("c", "nrm", "ref", "mask")}
    out = {"set": s, "cam": (Ks, Rp, t)}
    for radius in (1, 2):
        out[radius] = dr.depth_chain(Ks, Rp, t, 128, 96, rgb, chain, radius=radius)
    out["mixed"] = dr.depth_chain(Ks, Rp, t, 128, 96, rgb, s, radius=1)
    return out


def fused_mask(res):
    m = np.zeros(res["id"].shape, bool)
    m[res["pix"][:, 0], res["pix"][:, 2], res["pix"][:, 1]] = True
    return m


def test_quality_on_the_sphere_chain(quality):
    """The depth maps of the restatement's unrefined 442-patch chain on the
    24-view 96 x 128 sphere, against the analytic depth, at slope 4 and the
    fusion defaults (rel_tol 0.01, two consistent views, no violation).
    Measured here (the bounds are these with a factor of 2):
      radius 1: 3.86 % of the hit pixels hold a depth, median 0.432 and 95th percentile 1.402 footprints;
      radius 2: 5.51 %, 0.613, 2.144;
      fused, radius 1: 511 pixels, 0.42 %, 0.425, 1.091; radius 2: 735 pixels, 0.61 %, 0.580, 1.565;
      mixed set (442 chain patches + 114 outliers, radius 1): 538 fused pixels; 38 of the 114 outliers and
      127 of the 442 chain patches own one.  The chain is sparse (one patch per 2 x 2 cell of a few views),
      so most hit pixels stay empty, and the fusion defaults do not tell the 2 mm outliers from the chain:
      they are there for the maps of a filtered set."""
    Ks, Rp, t = quality["cam"]
    got = {}
    for radius in (1, 2):
        res = quality[radius]
        got[radius] = depth_quality(Ks, Rp, t, res["z"], RAD)
        got[radius, "fused"] = depth_quality(Ks, Rp, t, res["z"], RAD, fused_mask(res))
        print(f"radius {radius}: coverage {got[radius][0]:.4f} median {got[radius][1]:.4f} p95 {got[radius][2]:.4f}; "
              f"fused {len(res['pix'])} px: coverage {got[radius, 'fused'][0]:.4f} median "
              f"{got[radius, 'fused'][1]:.4f} p95 {got[radius, 'fused'][2]:.4f}")
    s, mixed = quality["set"], quality["mixed"]
    owners = np.unique(mixed["id"][fused_mask(mixed)])
    n_out, n_chain = int((s["kind"][owners] != 0).sum()), int((s["kind"][owners] == 0).sum())
    print(f"mixed set: {len(mixed['pix'])} fused px, owners: {n_out} of {int((s['kind'] != 0).sum())} outliers, "
          f"{n_chain} of {int((s['kind'] == 0).sum())} chain patches")
    assert int((s["kind"] == 0).sum()) == 442 and int((s["kind"] != 0).sum()) == 114
    bounds = BOUNDS
    for key, (cov, med, p95) in bounds.items():
        assert got[key][0] >= cov / 2, key
        assert got[key][1] <= med * 2 and got[key][2] <= p95 * 2, key
    assert n_out <= 2 * OWNERS[0] and n_chain >= OWNERS[1] / 2
    # the fused points are the points call's, on the sphere within the same error
    r = np.linalg.norm(quality[1]["points"], axis=1)
    assert len(r) == len(quality[1]["pix"]) > 0 and np.isfinite(r).all()


def test_fast_count_is_the_python_count_on_the_quality_maps(quality):
    """The numpy count that the quality test and the GPU tests use, against the
    Python-float one on the first three views of the radius-1 maps."""
    Ks, Rp, t = quality["cam"]
    z = quality[1]["z"][:3]
    pairs = int(np.isfinite(z).sum()) * 2
    assert 0 < pairs <= 200000
    a, b = dr.consist(Ks, Rp, t, 128, 96, z, 0, 3, 0.01), dr.consist_fast(Ks, Rp, t, 128, 96, z, 0, 3, 0.01)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()


# measured by test_quality_on_the_sphere_chain (its printed line): (coverage, median, p95)
BOUNDS = {1: (0.0386, 0.4321, 1.4023), 2: (0.0551, 0.6128, 2.1441),
          (1, "fused"): (0.0042, 0.4247, 1.0914), (2, "fused"): (0.0061, 0.5801, 1.5650)}
OWNERS = (38, 127)     # outliers, chain patches that own a fused pixel of the mixed set
