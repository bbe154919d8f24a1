"""The depth maps of a warped patch set on the GPU (k_wdepth_fill,
k_wdepth_splat, k_wdepth_consist, k_wdepth_points and MvsContext.depth_maps)
against the float64 restatement (tests/depth_reference.py).

Every comparison is exact, with no element left out and no tolerance: the bits
of zmap, idmap, cons, viol, the bits of xyz, and rgb; the maps are filled with
a canary pattern before each call.  The arithmetic is the projection and the
ray-plane intersection that tests/test_expand_gpu.py already finds bit-equal.

Sizes: the splat puts 4 patches in a workgroup (n = 1, 3, 4, 5 and 257: a
partial last workgroup) and flattens (view, footprint pixel) pairs over 64
lanes (radius 0..3: 1, 9, 25 and 49 pixels per view, so the pair count is no
multiple of 64); the 80- and 130-view rings take its second and third group of
64 views; 23 x 29, 26 x 31 and 41 x 2061 images are no multiple of the
consistency kernel's 256-pixel workgroup.
"""
import ctypes

import numpy as np
import pytest

import depth_reference as dr
import filter_reference as fr
import warped_reference as wr
import warped_shapes as ws
from test_expand_gpu import random_masks

pytestmark = pytest.mark.gpu

RAD = 0.02


class G:
    """A warped_shapes.Scene with its context."""

    def __init__(self, pkg, sc):
        import torch
        assert torch.cuda.is_available(), "GPU test without a GPU"
        self.sc = sc
        self.ctx = pkg.MvsContext(sc.rgb, sc.K, sc.R, sc.t_raw, device=0)
        assert np.array_equal(self.ctx.rproj(), sc.Rp)
        self.V, self.H, self.W = sc.V, sc.H, sc.W

    def cam(self):
        return self.sc.cam()


def _scene(pkg, sc):
    g = G(pkg, sc)
    yield g
    g.ctx.close()


@pytest.fixture(scope="module")
def sphere(pkg):
    yield from _scene(pkg, ws.Scene(*pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]))


@pytest.fixture(scope="module")
def small(pkg):
    yield from _scene(pkg, ws.sphere(26, 31))


@pytest.fixture(scope="module")
def ring80(pkg):
    yield from _scene(pkg, ws.Scene(*pkg.synthetic.ring_scene(V=80, H=48, W=64)))


@pytest.fixture(scope="module")
def ring130(pkg):
    yield from _scene(pkg, ws.ring(130))                       # 23 x 29


@pytest.fixture(scope="module")
def wide(pkg):
    yield from _scene(pkg, ws.Scene(*pkg.synthetic.ring_scene(V=3, H=41, W=2061)))


def _dev(x):
    import torch
    a = np.ascontiguousarray(x)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to("cuda:0")


def gpu_splat(g, c, nrm, ref, mask, radius, slope, v0, nv):
    """mvs_wdepth_splat_device on maps pre-filled with a canary pattern -> zmap, idmap."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tc = _dev(np.asarray(c, np.float64).reshape(n, 3))
        tn = _dev(np.asarray(nrm, np.float64).reshape(n, 3))
        tr = _dev(np.asarray(ref, np.int32))
        tm = _dev(np.asarray(mask, np.uint64).reshape(n, g.ctx.words))
        z = torch.full((nv, g.H, g.W), -77.0, dtype=torch.float64, device=dev)
        idm = torch.full((nv, g.H, g.W), -77, dtype=torch.int32, device=dev)
        g.ctx.wdepth_splat_device(tc, tn, tr, tm, radius, slope, v0, nv, z, idm, stream=st.cuda_stream)
        out = z.cpu().numpy(), idm.cpu().numpy()
    st.synchronize()
    return out


def gpu_consist(g, zmap, v0, nv, rel_tol, with_viol=True):
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        z = _dev(np.asarray(zmap, np.float64).reshape(nv, g.H, g.W))
        cons = torch.full((nv, g.H, g.W), 77, dtype=torch.uint8, device=dev)
        viol = torch.full((nv, g.H, g.W), 77, dtype=torch.uint8, device=dev)
        g.ctx.wdepth_consist_device(z, v0, nv, rel_tol, cons, viol if with_viol else None, stream=st.cuda_stream)
        out = cons.cpu().numpy(), viol.cpu().numpy()
    st.synchronize()
    return out


def gpu_points(g, pix, zmap, v0, nv):
    import torch
    dev = torch.device("cuda:0")
    m = len(pix)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        z = _dev(np.asarray(zmap, np.float64).reshape(nv, g.H, g.W))
        tp = _dev(np.asarray(pix, np.int32).reshape(m, 3))
        xyz = torch.full((m, 3), -77.0, dtype=torch.float64, device=dev)
        rgb = torch.full((m, 3), 77, dtype=torch.uint8, device=dev)
        g.ctx.wdepth_points_device(tp, z, v0, nv, xyz, rgb, stream=st.cuda_stream)
        out = xyz.cpu().numpy(), rgb.cpu().numpy()
    st.synchronize()
    return out


def compare_splat(g, c, nrm, ref, mask, radius=1, slope=4.0, v0=0, nv=None, label=""):
    nv = g.V - v0 if nv is None else nv
    want = dr.splat(*g.cam(), c, nrm, ref, mask, radius, slope, v0, nv)
    z, idm = gpu_splat(g, c, nrm, ref, mask, radius, slope, v0, nv)
    assert idm.dtype == np.int32 and np.array_equal(idm, want[1]), label
    assert z.tobytes() == want[0].tobytes(), label
    drawn = want[1] >= 0
    print(f"{label}: n {len(ref)}, radius {radius}, views {v0}..{v0 + nv - 1}: {int(drawn.sum())} of {drawn.size} pixels "
          f"drawn by {len(np.unique(want[1][drawn]))} patches")
    return want


def compare_consist(g, zmap, v0, nv, rel_tol, label=""):
    want = dr.consist_fast(*g.cam(), zmap, v0, nv, rel_tol)
    cons, viol = gpu_consist(g, zmap, v0, nv, rel_tol)
    assert cons.dtype == np.uint8 and np.array_equal(cons, want[0]), label
    assert np.array_equal(viol, want[1]), label
    only, canary = gpu_consist(g, zmap, v0, nv, rel_tol, with_viol=False)
    assert np.array_equal(only, want[0]) and (canary == 77).all(), label
    print(f"{label}: {int((want[0] > 0).sum())} pixels with a consistent view (max {int(want[0].max())}), "
          f"{int((want[1] > 0).sum())} with a violation")
    return want


def sphere_set(g, n, seed, p=0.4):
    rng = np.random.default_rng(seed)
    c, nrm, ref, _ = wr.sphere_patches(g.sc.K, g.sc.R, g.sc.t, n, RAD, rng, (0.0, 0.002, -0.002))
    return rng, c, nrm, ref, random_masks(rng, n, g.V, p)


def origin_set(g, n, seed, spread=0.005, p=0.3):
    """Patches near the origin of a ring scene facing their reference camera, pad bits planted."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, g.V, n).astype(np.int32)
    return rng, c, ws.toward_camera(g.sc, c, ref), ref, ws.plant_pad_bits(random_masks(rng, n, g.V, p), g.V)


# ---------------------------------------------------------------------------
# 1. the splat
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_splat_sizes(sphere, n, radius):
    g = sphere
    _, c, nrm, ref, mask = sphere_set(g, n, 100 + n)
    want = compare_splat(g, c, nrm, ref, mask, radius, label=f"sizes n {n}")
    if n == 0:
        assert np.all(want[1] == -1) and np.all(np.isposinf(want[0]))
    else:
        assert (want[1] >= 0).any()


@pytest.mark.parametrize("v0,nv", [(0, 24), (5, 1), (7, 11), (23, 1)])
def test_splat_view_ranges(sphere, v0, nv):
    g = sphere
    _, c, nrm, ref, mask = sphere_set(g, 120, 7)
    full = dr.splat(*g.cam(), c, nrm, ref, mask, 2, 4.0)
    want = compare_splat(g, c, nrm, ref, mask, 2, v0=v0, nv=nv, label="range")
    assert np.array_equal(want[1], full[1][v0:v0 + nv]) and (want[1] >= 0).any()


@pytest.mark.parametrize("radius", [1, 3])
def test_splat_small_image(small, radius):
    """26 x 31, a sphere that fills the image: footprints are clipped on every border."""
    g = small
    c, nrm, ref = ws.border_patches(g.sc, 150, 3)
    mask = random_masks(np.random.default_rng(3), len(ref), g.V, 0.4)
    want = compare_splat(g, c, nrm, ref, mask, radius, label="26 x 31")
    for edge in (want[1][:, 0], want[1][:, -1], want[1][:, :, 0], want[1][:, :, -1]):
        assert (edge >= 0).any()


@pytest.mark.parametrize("radius", [0, 2])
def test_splat_more_than_64_views(ring80, radius):
    g = ring80
    _, c, nrm, ref, mask = origin_set(g, 61, 4)
    assert mask.shape[1] == 2 and (mask[::3, 1] >> np.uint64(16)).all()          # bits 80..127 name no view
    want = compare_splat(g, c, nrm, ref, mask, radius, label="ring V=80")
    assert (want[1][64:] >= 0).any() and (want[1][:64] >= 0).any()
    compare_splat(g, c, nrm, ref, mask, radius, v0=60, nv=9, label="ring V=80, a range across the words")


def test_splat_130_views_23_x_29(ring130):
    g = ring130
    _, c, nrm, ref, mask = origin_set(g, 40, 9, p=0.5)
    assert mask.shape[1] == 3
    want = compare_splat(g, c, nrm, ref, mask, 3, label="ring V=130, 23 x 29")
    assert (want[1][128:] >= 0).any() and (want[1][64:128] >= 0).any()
    compare_splat(g, c, nrm, ref, mask, 1, v0=127, nv=3, label="ring V=130, views 127..129")


def wide_set(g, n=60, seed=2):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, g.V, n).astype(np.int32)
    x, y = rng.uniform(0, g.W - 0.01, n), rng.uniform(0, g.H - 0.01, n)
    x[:4] = [0.2, g.W - 0.7, g.W - 0.3, 1024.5]
    c = np.array([g.sc.at_pixel(int(v), a, b, s) for v, a, b, s in zip(ref, x, y, rng.uniform(0.9, 1.1, n))])
    return c, ws.toward_camera(g.sc, c, ref), ref, random_masks(rng, n, g.V, 0.5)


def test_splat_wide_image(wide):
    """41 x 2061: row pitch and column range far past the other scenes'."""
    g = wide
    c, nrm, ref, mask = wide_set(g)
    want = compare_splat(g, c, nrm, ref, mask, 3, label="41 x 2061")
    assert (want[1][:, :, 2060] >= 0).any() and (want[1][:, :, 0] >= 0).any()


def special_rows(g):
    """Rows the splat must leave out or clip, among ordinary ones (view 7 is their reference view)."""
    sc = g.sc
    rng, c, nrm, ref, mask = sphere_set(g, 40, 5)
    v = 7
    ref[0], ref[1] = -1, g.V
    c[2, 1] = np.nan
    c[3, 0] = np.inf
    nrm[4, 2] = np.nan
    nrm[5] = [np.inf, 0.0, 0.0]
    c[6] = sc.O[3] * 1.2                                         # behind camera 3
    ref[6], mask[6] = 3, 0
    spots = {7: (g.W - 0.7, 40.2), 8: (g.W - 0.3, 70.6), 9: (0.2, 30.4), 10: (60.3, g.H - 0.2),   # x in [W-1, W), [0, 0.5)
             11: (0.3, 0.4), 12: (g.W - 0.6, 0.3), 13: (0.4, g.H - 0.6), 14: (g.W - 0.7, g.H - 0.8)}   # the corners
    for k, (x, y) in spots.items():
        c[k] = sc.at_pixel(v, x, y, 0.5)
        ref[k], mask[k] = v, 0
    nrm[7:15] = ws.toward_camera(sc, c[7:15], ref[7:15])
    # 15: its normal is perpendicular to the ray of the pixel right of its centre pixel, to the bit
    c[15] = sc.at_pixel(v, 70.0, 50.0, 0.5)
    ref[15], mask[15] = v, 0
    cam = dr.er._cam(sc.K, sc.Rp, sc.t, v)
    d = dr.pixel_ray(cam[0], *cam[2:], 71, 50)
    n15 = np.array([d[1], -d[0], 0.0])
    nrm[15] = n15 if n15 @ (sc.O[v] - c[15]) > 0 else -n15
    assert nrm[15][0] * d[0] + nrm[15][1] * d[1] + nrm[15][2] * d[2] == 0.0
    # 16: back-facing in its only view
    c[16] = sc.at_pixel(v, 90.0, 20.0, 0.5)
    ref[16], mask[16] = v, 0
    nrm[16] = -ws.toward_camera(sc, c[16:17], ref[16:17])[0]
    return c, nrm, ref, mask


@pytest.mark.parametrize("radius", [0, 2, 3])
def test_splat_special_rows(sphere, radius):
    g = sphere
    c, nrm, ref, mask = special_rows(g)
    want = compare_splat(g, c, nrm, ref, mask, radius, label="special rows")
    idm = want[1]
    for k in (0, 1, 2, 3, 4, 5, 6, 16):
        assert not (idm == k).any(), k
    r, W, H = radius, g.W, g.H
    side = 2 * r + 1
    # the aimed patches lie nearer than the sphere: their whole clipped footprint is theirs
    assert (idm[7, 40 - r:41 + r, W - 1 - r:] == 7).all() and (idm == 7).sum() == side * (r + 1)     # x0 = W - 1
    assert (idm[7, 71 - r:72 + r, W - r:] == 8).all() and (idm == 8).sum() == side * r               # x0 = W
    assert (idm[7, 30 - r:31 + r, :r + 1] == 9).all() and (idm == 9).sum() == side * (r + 1)         # x0 = 0
    assert (idm[7, H - r:, 60 - r:61 + r] == 10).all() and (idm == 10).sum() == side * r             # y0 = H
    for k, ys, xs in ((11, slice(0, r + 1), slice(0, r + 1)), (12, slice(0, r + 1), slice(W - 1 - r, W)),
                      (13, slice(H - 1 - r, H), slice(0, r + 1)), (14, slice(H - 1 - r, H), slice(W - 1 - r, W))):
        assert (idm[7, ys, xs] == k).all() and (idm == k).sum() == (r + 1) ** 2, k
    # den = 0 at the pixel right of 15's centre; the plane grazes the rays around it
    assert idm[7, 50, 70] == 15 and idm[7, 50, 71] != 15


def test_splat_tiny_slope_leaves_the_centre_pixels(sphere):
    """Sphere patches through integer pixels of their reference view, their only
    view: at the centre pixel s = z up to rounding, and the sphere's tilt changes
    the depth by far more than 0.001 footprints per pixel, except along a
    patch's line of equal depth where that passes through a neighbour pixel."""
    g = sphere
    rng = np.random.default_rng(8)
    n = 60
    ref = rng.integers(0, g.V, n).astype(np.int32)
    x, y = rng.integers(40, 89, n), rng.integers(24, 73, n)
    hits = [g.sc.on_sphere(int(v), float(a), float(b), RAD) for v, a, b in zip(ref, x, y)]
    c, nrm = np.array([h[0] for h in hits]), np.array([h[1] for h in hits])
    mask = np.zeros((n, 1), np.uint64)
    want = compare_splat(g, c, nrm, ref, mask, 3, slope=1e-3, label="slope 1e-3")
    centre = compare_splat(g, c, nrm, ref, mask, 0, slope=1e-3, label="slope 1e-3, radius 0")
    for got in (want, centre):
        assert (got[1][ref, y, x] == np.arange(n)).all()
    assert (centre[1] >= 0).sum() == n <= (want[1] >= 0).sum() < 2 * n
    assert (dr.splat(*g.cam(), c, nrm, ref, mask, 3, 4.0)[1] >= 0).sum() > 40 * n


@pytest.mark.parametrize("reverse", [False, True])
def test_splat_contention_and_ties(sphere, reverse):
    """3,000 fronto-parallel patches on one pixel ray of view 5: every atomic of both
    passes lands on the same nine addresses.  100 rows are bit-identical copies
    of the nearest: the lowest index wins."""
    g = sphere
    rng = np.random.default_rng(12)
    n, v = 3000, 5
    scale = rng.uniform(0.9, 1.1, n)
    c = np.array([g.sc.at_pixel(v, 60.9, 40.9, k) for k in scale])
    near = int(np.argmin(scale))
    copies = rng.choice(np.setdiff1d(np.arange(n), [near]), 100, replace=False)
    c[copies] = c[near]
    if reverse:
        c = c[::-1].copy()
    ref = np.full(n, v, np.int32)
    nrm = np.tile(g.sc.Rp[v].T @ np.array([0.0, 0.0, -1.0]), (n, 1))        # along the optical axis: s varies little
    want = compare_splat(g, c, nrm, ref, np.zeros((n, 1), np.uint64), 1, label=f"one pixel, reversed {reverse}")
    assert (want[1] >= 0).sum() == 9
    winner = int(want[1][v, 41, 61])
    same = np.flatnonzero((c == c[winner]).all(1))
    assert len(same) == 101 and winner == same.min()


# ---------------------------------------------------------------------------
# 2. the consistency count
# ---------------------------------------------------------------------------
def test_consist_on_crafted_maps(small):
    g = small
    rng = np.random.default_rng(31)
    shape = (g.V, g.H, g.W)
    empty = np.full(shape, np.inf)
    want = compare_consist(g, empty, 0, g.V, 0.01, "all empty")
    assert not want[0].any() and not want[1].any()
    # the depth of the sphere's centre in every view, with noise, holes and entries that are no depth
    z0 = np.array([float(g.sc.t[v][2]) for v in range(g.V)])[:, None, None]
    z = z0 * rng.choice([1.0, 1.0, 0.995, 1.004, 0.9, 1.1], shape)
    z[rng.random(shape) < 0.15] = np.inf
    odd = rng.random(shape)
    z[odd < 0.02], z[(odd >= 0.02) & (odd < 0.04)], z[(odd >= 0.04) & (odd < 0.06)] = np.nan, -1.0, 0.0
    z[(odd >= 0.06) & (odd < 0.07)] = -np.inf
    for tol in (0.0, 0.01, 0.2):
        want = compare_consist(g, z, 0, g.V, tol, f"crafted, rel_tol {tol}")
    assert want[0].any() and want[1].any()
    # an entry that is no depth is no pixel of its own view (and, when finite, still an entry of the others' lookups)
    bad = ~(np.isfinite(z) & (z > 0))
    assert not want[0][bad].any() and not want[1][bad].any()
    compare_consist(g, z[3:12], 3, 9, 0.01, "crafted, views 3..11")
    one = compare_consist(g, z[5:6], 5, 1, 0.01, "one view against itself")
    assert not one[0].any() and not one[1].any()


def test_consist_rounding_to_column_w_and_row_h(small):
    """Points whose projection into the next view has int(x + 0.5) = W or int(y +
    0.5) = H: seen by nothing, though x < W and y < H."""
    g = small
    sc = g.sc
    z = np.full((2, g.H, g.W), np.inf)
    hits = []
    for qy in range(g.H):
        for qx in range(g.W):
            for s in (0.8, 1.0, 1.2):
                zz = float(sc.t[0][2]) * s
                X = dr.world_point(dr.er._cam(sc.K, sc.Rp, sc.t, 0), qx, qy, zz)
                x, y, depth = wr.project_ref(sc.K[1], sc.Rp[1], sc.t[1], X)
                if depth > 0 and ((g.W - 0.5 <= x < g.W and 0 <= y < g.H - 0.5) or (g.H - 0.5 <= y < g.H and 0 <= x < g.W - 0.5)):
                    z[0, qy, qx] = zz
                    hits.append((qy, qx))
    assert hits, "no point rounds out of the next view"
    z[1] = float(sc.t[1][2])
    want = compare_consist(g, z, 0, 2, 0.5, "rounding out")
    assert not want[0][0].any() and not want[1][0].any()


def test_consist_bit_equal_depths_at_rel_tol_0(small):
    """A map rendered from a patch set, then view 1's entries replaced by the
    exact depths of view 0's points there: consistent at rel_tol 0."""
    g = small
    sc = g.sc
    z = np.full((2, g.H, g.W), np.inf)
    n_set = 0
    for qy in range(2, g.H - 2):
        for qx in range(2, g.W - 2):
            zz = float(sc.t[0][2]) * (1.0 + 0.001 * ((qx * 7 + qy * 3) % 11))
            X = dr.world_point(dr.er._cam(sc.K, sc.Rp, sc.t, 0), qx, qy, zz)
            x, y, depth = wr.project_ref(sc.K[1], sc.Rp[1], sc.t[1], X)
            xi, yi = dr.nearest(x), dr.nearest(y)
            if depth > 0 and x >= 0 and y >= 0 and xi < g.W and yi < g.H and np.isinf(z[1, yi, xi]):
                z[0, qy, qx], z[1, yi, xi] = zz, depth
                n_set += 1
    want = compare_consist(g, z, 0, 2, 0.0, "bit-equal depths")
    assert n_set > 50 and int((want[0][0] == 1).sum()) == n_set


def test_consist_on_the_splats_own_maps(sphere):
    g = sphere
    _, c, nrm, ref, mask = sphere_set(g, 257, 357, p=0.6)
    for radius in (1, 3):
        z, _ = dr.splat(*g.cam(), c, nrm, ref, mask, radius, 4.0)
        want = compare_consist(g, z, 0, g.V, 0.01, f"sphere maps, radius {radius}")
        assert want[0].max() >= 2 and want[1].any()
    compare_consist(g, z[10:], 10, 14, 0.002, "sphere maps, views 10..23")


def test_consist_rings_and_wide(ring80, ring130, wide):
    for g, n, spread in ((ring80, 80, 0.02), (ring130, 60, 0.01)):
        _, c, nrm, ref, mask = origin_set(g, n, 5, spread=spread, p=0.5)
        z, _ = dr.splat(*g.cam(), c, nrm, ref, mask, 2, 4.0)
        want = compare_consist(g, z, 0, g.V, 0.05, f"ring V={g.V}")
        assert want[0].any()
    c, nrm, ref, mask = wide_set(wide, 200, 4)
    z, _ = dr.splat(*wide.cam(), c, nrm, ref, mask, 3, 4.0)
    compare_consist(wide, z, 0, 3, 0.05, "41 x 2061")


# ---------------------------------------------------------------------------
# 3. the points call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "wide", "ring130"])
def test_points(request, which):
    g = request.getfixturevalue(which)
    if which == "sphere":
        _, c, nrm, ref, mask = sphere_set(g, 100, 11)
    elif which == "wide":
        c, nrm, ref, mask = wide_set(g)
    else:
        _, c, nrm, ref, mask = origin_set(g, 40, 9, p=0.5)
    v0, nv = (0, g.V) if which != "ring130" else (120, 10)
    z, idm = dr.splat(*g.cam(), c, nrm, ref, mask, 2, 4.0, v0, nv)
    z[0, 0, 0], z[0, 0, 1], z[0, 1, 0] = np.nan, -1.0, 0.0
    rng = np.random.default_rng(1)
    drawn = np.argwhere(idm >= 0)
    drawn = drawn[rng.permutation(len(drawn))[:300]]
    empty = np.argwhere(idm < 0)[:: max(1, int((idm < 0).sum()) // 50)]
    at = np.concatenate([drawn, empty, [[0, 0, 0], [0, 0, 1], [0, 1, 0], [nv - 1, g.H - 1, g.W - 1]]])
    pix = np.stack([at[:, 0] + v0, at[:, 2], at[:, 1]], 1).astype(np.int32)
    want = dr.points(*g.cam(), g.sc.rgb, z, v0, nv, pix)
    xyz, rgb = gpu_points(g, pix, z, v0, nv)
    assert xyz.tobytes() == want[0].tobytes() and rgb.dtype == np.uint8 and np.array_equal(rgb, want[1])
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and want[1].any()
    # the host-pointer call agrees; the device call reads nothing for a pixel outside and writes nan and 0
    hx, hr = g.ctx.wdepth_points(pix, z, (v0, nv))
    assert hx.tobytes() == want[0].tobytes() and np.array_equal(hr, want[1])
    out = np.array([[v0 - 1, 0, 0], [v0 + nv, 0, 0], [v0, g.W, 0], [v0, 0, g.H], [v0, -1, 0], [v0, 0, -1]], np.int32)
    xyz, rgb = gpu_points(g, out, z, v0, nv)
    assert np.isnan(xyz).all() and not rgb.any()
    for k in range(len(out)):
        with pytest.raises(RuntimeError, match="listed pixel outside"):
            g.ctx.wdepth_points(out[k:k + 1], z, (v0, nv))
    xyz, rgb = g.ctx.wdepth_points(np.empty((0, 3), np.int32), z, (v0, nv))
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3)


# ---------------------------------------------------------------------------
# 4. the chain
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(sphere):
    s = sphere.sc
    return fr.mixed_set(s.gray, s.K, s.R, s.t, s.Rp, RAD)


CHAIN_KEYS = ("z", "id", "cons", "viol", "normal", "points", "normals", "colors", "pix")


@pytest.mark.parametrize("kw", [{}, {"radius": 2, "views": (3, 17), "rel_tol": 0.02, "min_consistent": 1,
                                     "max_violations": 1}])
def test_chain_is_the_restatement(sphere, mixed, orc, pkg, kw):
    """score, the chain twice on the side stream, score on one context: the
    chain is the restatement's, bit-identical both times, and both score results
    are the oracle's."""
    g, m = sphere, mixed
    patches = {k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell")}
    first = g.ctx.score(m["c"], m["ref"], 0.7, 5)
    a = pkg.depth_maps_warped(g.ctx, patches, **kw)
    b = g.ctx.depth_maps(patches, **kw)
    again = g.ctx.score(m["c"], m["ref"], 0.7, 5)
    want = dr.depth_chain(*g.cam(), g.sc.rgb, patches, **kw)
    assert len(want["pix"]) > 100 and want["pix"].dtype == np.int32
    for k in CHAIN_KEYS:
        assert a[k].dtype == want[k].dtype and a[k].shape == want[k].shape, k
        assert a[k].tobytes() == want[k].tobytes(), k
        assert a[k].tobytes() == b[k].tobytes(), k
    sc = orc.Scene(g.sc.rgb, g.sc.K, g.sc.R, g.sc.t_raw).score_batch(m["c"], m["ref"], 0.7, 5)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    for x, w in zip(first[:3], sc[:3]):
        assert np.array_equal(x, w)
    assert np.allclose(first[3], sc[3], rtol=0, atol=1e-12)
    print(f"chain {kw}: {len(want['pix'])} fused pixels of {int((want['id'] >= 0).sum())} drawn")


def test_chain_on_an_empty_set(sphere):
    g = sphere
    none = g.ctx.depth_maps({"c": np.empty((0, 3)), "nrm": np.empty((0, 3)), "ref": np.empty(0, np.int32),
                             "mask": np.empty((0, 1), np.uint64)}, views=(2, 3))
    assert none["z"].shape == (3, g.H, g.W) and np.isposinf(none["z"]).all() and (none["id"] == -1).all()
    assert not none["cons"].any() and np.isnan(none["normal"]).all() and none["pix"].shape == (0, 3)
    assert none["points"].shape == (0, 3) and none["colors"].shape == (0, 3)
    with pytest.raises(RuntimeError, match="no 'nrm'"):
        g.ctx.depth_maps({"c": np.empty((0, 3)), "ref": np.empty(0, np.int32), "mask": np.empty((0, 1), np.uint64)})
    with pytest.raises(RuntimeError, match="view range"):
        g.ctx.depth_maps({"c": np.empty((0, 3)), "nrm": np.empty((0, 3)), "ref": np.empty(0, np.int32),
                          "mask": np.empty((0, 1), np.uint64)}, views=(20, 5))


def test_dense_points_warped_writes_the_maps(pkg, sphere, tmp_path, capsys):
    """MVS2.DensePointsWarped(depth_maps=DIR) on test_seed_gpu's planted sphere:
    the maps are MvsContext.depth_maps of the final set (held against the
    restatement above), the files hold them, and the count line and last_stats
    gain the dense count."""
    import types

    import seed_reference as sd
    from test_seed_gpu import write_pars
    p = sd.planted(pkg)
    par = str(tmp_path / "par.txt")
    write_pars(par, p["K"], p["R"], p["t_raw"])
    imgs = [p["rgb"][v] for v in range(sphere.V)]
    out = pkg.DensePointsWarped(imgs, types.SimpleNamespace(par_path=par), rounds=2, iterations=1, epi_px=1.5,
                                feats=p["feats"], pairs=p["pairs"], path=str(tmp_path / "cloud"),
                                depth_maps=str(tmp_path / "maps"), depth_radius=2, dense_path=str(tmp_path / "dense"))
    maps = out["maps"]
    want = sphere.ctx.depth_maps(out["patches"], radius=2)
    for k in CHAIN_KEYS:
        assert maps[k].tobytes() == want[k].tobytes(), k
    m = len(maps["pix"])
    assert m > 1000 and out["counts"]["dense"] == m == pkg.MVS2.last_stats["dense"]
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("warped:")]
    assert len(line) == 1 and line[0].endswith(f" dense {m}")
    for v in (0, 11, sphere.V - 1):
        z = np.load(tmp_path / "maps" / ("depth_%04d.npy" % v))
        n = np.load(tmp_path / "maps" / ("normal_%04d.npy" % v))
        drawn = maps["id"][v] >= 0
        assert z.dtype == np.float32 and np.array_equal(np.isnan(z), ~drawn) and drawn.any()
        assert np.array_equal(z[drawn], maps["z"][v][drawn].astype(np.float32))
        assert np.array_equal(n[drawn], maps["normal"][v][drawn].astype(np.float32)) and np.isnan(n[~drawn]).all()
    assert len(list((tmp_path / "maps").iterdir())) == 2 * sphere.V
    pts, nrm, col = pkg.read_ply_oriented(str(tmp_path / "dense.ply"))
    assert pts.tobytes() == maps["points"].tobytes() and nrm.tobytes() == maps["normals"].tobytes()
    assert np.array_equal(col, maps["colors"].astype(np.float64))
    # the fused points lie on the sphere as the patches do
    r = np.linalg.norm(maps["points"], axis=1)
    print(f"{len(out['patches']['ref'])} patches, {int((maps['id'] >= 0).sum())} pixels drawn, {m} fused; "
          f"within 5 % of the radius {float((np.abs(r - p['rad']) <= 0.05 * p['rad']).mean()):.4f}")


# ---------------------------------------------------------------------------
# 5. host-pointer variants and arguments
# ---------------------------------------------------------------------------
def test_host_pointer_variants(sphere, ring80):
    for g, (c, nrm, ref, mask), views in ((sphere, sphere_set(sphere, 90, 21)[1:], (4, 9)),
                                          (ring80, origin_set(ring80, 50, 22)[1:], None)):
        v0, nv = (0, g.V) if views is None else views
        dz, di = gpu_splat(g, c, nrm, ref, mask, 2, 4.0, v0, nv)
        hz, hi = g.ctx.wdepth_splat(c, nrm, ref, mask, 2, 4.0, views)
        assert hz.tobytes() == dz.tobytes() and np.array_equal(hi, di) and (hi >= 0).any()
        dc, dv = gpu_consist(g, dz, v0, nv, 0.01)
        hc, hv = g.ctx.wdepth_consist(hz, 0.01, views)
        assert np.array_equal(hc, dc) and np.array_equal(hv, dv) and hc.any()
    e3, e1 = np.empty((0, 3)), np.empty(0, np.int32)
    z, idm = sphere.ctx.wdepth_splat(e3, e3, e1, np.empty((0, 1), np.uint64), 1, 4.0, (1, 2))
    assert z.shape == (2, sphere.H, sphere.W) and np.isposinf(z).all() and (idm == -1).all()


def test_arguments(pkg, sphere):
    g = sphere
    lib = pkg._lib.load()
    h = g.ctx.handle
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails its checks
    V = g.V

    def splat(n=1, radius=1, slope=4.0, v0=0, nv=V, ptr=one, zmap=one, idmap=one):
        return lib.mvs_wdepth_splat_device(h, n, ptr, one, one, one, radius, slope, v0, nv, zmap, idmap, None)

    def consist(v0=0, nv=V, rel_tol=0.01, zmap=one, cons=one):
        return lib.mvs_wdepth_consist_device(h, zmap, v0, nv, rel_tol, cons, None, None)

    def points(m=1, v0=0, nv=V, pix=one, zmap=one):
        return lib.mvs_wdepth_points_device(h, m, pix, zmap, v0, nv, one, one, None)

    nan, inf = float("nan"), float("inf")
    for call, msg in ((lambda: splat(n=-1), "n < 0"), (lambda: splat(n=1 << 31), "below 2^31"),
                      (lambda: splat(radius=-1), "radius must be in 0..3"),
                      (lambda: splat(radius=4), "radius must be in 0..3"),
                      (lambda: splat(slope=0.0), "slope must be finite and > 0"),
                      (lambda: splat(slope=-1.0), "slope must be finite and > 0"),
                      (lambda: splat(slope=nan), "slope must be finite and > 0"),
                      (lambda: splat(slope=inf), "slope must be finite and > 0"),
                      (lambda: splat(v0=-1), "view range"), (lambda: splat(v0=1), "view range"),
                      (lambda: splat(nv=0), "view range"), (lambda: splat(v0=V, nv=1), "view range"),
                      (lambda: splat(v0=2 ** 31 - 1, nv=2 ** 31 - 1), "view range"),
                      (lambda: splat(ptr=None), "null pointer"), (lambda: splat(n=0, zmap=None), "null pointer"),
                      (lambda: splat(n=0, idmap=None), "null pointer"),
                      (lambda: consist(rel_tol=-0.1), "rel_tol must be finite and >= 0"),
                      (lambda: consist(rel_tol=nan), "rel_tol must be finite and >= 0"),
                      (lambda: consist(rel_tol=inf), "rel_tol must be finite and >= 0"),
                      (lambda: consist(v0=3, nv=V - 2), "view range"), (lambda: consist(nv=0), "view range"),
                      (lambda: consist(zmap=None), "null pointer"), (lambda: consist(cons=None), "null pointer"),
                      (lambda: points(m=-1), "m < 0"), (lambda: points(m=1 << 31), "below 2^31"),
                      (lambda: points(v0=V), "view range"), (lambda: points(pix=None), "null pointer"),
                      (lambda: points(m=0, zmap=None), "null pointer")):
        assert call() == -1                      # MVS_E_ARG
        assert msg in pkg._lib.last_error(h), (msg, pkg._lib.last_error(h))
    assert points(m=0, pix=None) == 0
    # the host-pointer variants run the same checks
    e3, e1, em = np.empty((0, 3)), np.empty(0, np.int32), np.empty((0, 1), np.uint64)
    with pytest.raises(RuntimeError, match="radius"):
        g.ctx.wdepth_splat(e3, e3, e1, em, 4)
    with pytest.raises(RuntimeError, match="slope"):
        g.ctx.wdepth_splat(e3, e3, e1, em, 1, 0.0)
    with pytest.raises(RuntimeError, match="rel_tol"):
        g.ctx.wdepth_consist(np.zeros((V, g.H, g.W)), -1.0)
    with pytest.raises(RuntimeError, match="view range"):
        g.ctx.wdepth_splat(e3, e3, e1, em, 1, 4.0, (V - 1, 2))
