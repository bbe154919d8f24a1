"""The restatement of the signed-distance fusion and of marching tetrahedra
(tests/mesh_reference.py) alone, on the CPU: the rules of include/mvs_amd.h
worked out by hand or held against their geometric meaning, the topology of
every sign pattern of a cube, and the quality on a closed sphere scene.

The sphere scene: 14 views of 48 x 64 (6 cameras on the axes, 8 on the cube
diagonals, 0.33 from the origin, focal length 3310.4 W / 640), analytic depth
maps of the sphere of radius 0.02 through every integer pixel, a lattice of 40^3
cubes over +-0.026, trunc 3 voxels, min_weight 1.  Measured with this
restatement: 13,562 vertices and 27,120 faces, closed (every edge in two
triangles, once each way), Euler characteristic 2, no zero-area triangle; the
vertices' radial error has median 0.0833, 95th percentile 0.2608 and maximum
0.7095 voxels, and the enclosed volume is 1.00286 of 4 pi r^3 / 3.  The bounds
below are twice the measured errors and twice the volume's deviation: the GPU
returns the same arrays bit for bit (test_wmesh_gpu.py), so the margin only
guards the restatement against later edits.
"""
import importlib
import itertools
import math

import numpy as np
import pytest

import depth_reference as dr
import mesh_reference as mr
from conftest import PKG_NAME

RAD = 0.02
NAN = float("nan")


def extract(vol, origin=(0.0, 0.0, 0.0), voxel=1.0, rgb=None, cnt=None):
    vol = np.asarray(vol, np.float64)
    rgb = np.zeros(vol.shape + (3,), np.uint8) if rgb is None else rgb
    cnt = np.zeros(vol.shape, np.uint8) if cnt is None else cnt
    return mr.extract(vol, rgb, cnt, origin, voxel)


def cube(values):
    """A one-cube volume from the 8 corner values, corner = x + 2 y + 4 z."""
    return np.array(values, np.float64).reshape(2, 2, 2)


def check_no_unreferenced(vert, faces):
    assert len(vert) == 0 and len(faces) == 0 or sorted(set(faces.reshape(-1).tolist())) == list(range(len(vert)))


# ---------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------
def test_one_tetrahedron_by_hand():
    """Only corner (1,0,0) is inside: it lies in the tetrahedra of the
    permutations 012 and 021 alone (as c1).  Its value is -1 against +3 at the
    origin, +1 elsewhere."""
    v = [3.0, -1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    rgb = np.zeros((2, 2, 2, 3), np.uint8)
    cnt = np.zeros((2, 2, 2), np.uint8)
    rgb[0, 0, 0], cnt[0, 0, 0] = (10, 20, 30), 1       # the origin
    rgb[0, 0, 1], cnt[0, 0, 1] = (200, 100, 50), 1     # corner (1,0,0)
    rgb[1, 1, 1], cnt[1, 1, 1] = (7, 8, 9), 1          # corner (1,1,1)
    vert, col, faces = extract(cube(v), origin=(10.0, 20.0, 30.0), voxel=2.0, rgb=rgb, cnt=cnt)
    # the edges at corner 1: from the origin (owner 0, type x = 0), and from corner 1 to 3 (type y), 5 (z), 7 (yz)
    want = np.array([[10.0 + 0.75 * 2.0, 20.0, 30.0],           # t = 3 / (3 + 1) on the owner's side
                     [12.0, 20.0 + 0.5 * 2.0, 30.0],            # owner corner 1, type 1 (y): t = -1 / -2
                     [12.0, 20.0, 31.0],                        # type 3 (z)
                     [12.0, 21.0, 31.0]])                       # type 5 (y + z)
    assert np.array_equal(vert, want)
    # t = 0.75: the far endpoint's colour; t = 0.5 takes b, which has none except (1,1,1): falls back to a
    assert col.tolist() == [[200, 100, 50], [200, 100, 50], [200, 100, 50], [7, 8, 9]]
    assert faces.dtype == np.int32 and len(faces) == 2
    # tetrahedron 012 = corners 0, 1, 3, 7 uses the edges to 0, 3, 7; 021 = 0, 1, 5, 7 the edges to 0, 5, 7
    assert sorted(faces[0].tolist()) == [0, 1, 3] and sorted(faces[1].tolist()) == [0, 2, 3]
    inside = np.array([12.0, 20.0, 30.0])
    for tri in faces:
        p = vert[tri]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert n @ (p.mean(0) - inside) > 0      # away from the inside corner


def test_winding_of_every_permutation_and_case():
    """Every (tetrahedron, inside mask) of one cube with values -1 and +1: the
    normal (p1 - p0) x (p2 - p0) of every triangle points from the mean of the
    inside corners to the mean of the outside ones."""
    seen = 0
    for tp, perm in enumerate(mr.PERMS):
        cc = mr.tet_corners(perm)
        for case in range(1, 15):
            v = [NAN] * 8
            for m in range(4):
                v[cc[m]] = -1.0 if case >> m & 1 else 1.0
            vert, _, faces = extract(cube(v))
            assert len(faces) == (2 if bin(case).count("1") == 2 else 1)
            xyz = np.array([[c & 1, c >> 1 & 1, c >> 2 & 1] for c in cc], np.float64)
            ins = np.array([bool(case >> m & 1) for m in range(4)])
            direction = xyz[~ins].mean(0) - xyz[ins].mean(0)
            for tri in faces:
                p = vert[tri]
                assert np.cross(p[1] - p[0], p[2] - p[0]) @ direction > 0, (perm, case)
                seen += 1
            check_no_unreferenced(vert, faces)
    assert seen == 6 * (8 + 6 * 2)


def test_all_256_sign_patterns_are_consistently_oriented():
    for pattern in range(256):
        v = [-1.0 if pattern >> c & 1 else 1.0 for c in range(8)]
        vert, _, faces = extract(cube(v))
        und, directed, _, _ = mr.manifold_report(faces)
        assert und <= 2 and directed <= 1, pattern
        assert (len(faces) == 0) == (pattern in (0, 255))
        check_no_unreferenced(vert, faces)
        assert (mr.areas2(vert, faces) > 0).all()


@pytest.mark.parametrize("corner", range(8))
def test_nan_in_one_corner_leaves_no_unreferenced_vertex(corner):
    rng = np.random.default_rng(corner)
    for _ in range(20):
        vol = rng.normal(0, 1, (3, 3, 3))
        vol[corner >> 2 & 1, corner >> 1 & 1, corner & 1] = NAN
        vert, _, faces = extract(vol)
        check_no_unreferenced(vert, faces)
        assert np.isfinite(vert).all()
        und, directed, _, _ = mr.manifold_report(faces)
        assert und <= 2 and directed <= 1
    # the corners 0 and 7 lie in all six tetrahedra of their cube
    only = np.ones((2, 2, 2))
    only[0, 0, 1] = -1.0
    only[corner >> 2 & 1, corner >> 1 & 1, corner & 1] = NAN
    vert, _, faces = extract(only)
    assert (len(faces) == 0) == (corner in (0, 1, 7))


def test_exact_zeros_are_outside():
    for zero in (0.0, -0.0):
        v = [zero] * 8
        assert len(extract(cube(v))[2]) == 0          # nothing is inside
        v[0] = -1.0
        vert, _, faces = extract(cube(v))
        # t = -1 / (-1 - 0) = 1: all seven vertices sit on the far endpoints
        assert len(vert) == 7 and len(faces) == 6
        assert sorted(map(tuple, vert.tolist())) == sorted(
            (float(c & 1), float(c >> 1 & 1), float(c >> 2 & 1)) for c in range(1, 8))
        v = [1.0] * 8
        v[0], v[7] = -1.0, zero
        vert, _, faces = extract(cube(v))
        assert len(faces) == 6 and (mr.areas2(vert, faces) > 0).all()
    # a lone outside corner of value 0: t = 0 on its three edges of a tetrahedron, the triangle
    # collapses into the corner -- zero area, kept, on seven different vertices
    v = [0.0] + [-1.0] * 7
    vert, _, faces = extract(cube(v))
    assert len(faces) == 6 and len(vert) == 7 and (vert == 0.0).all() and (mr.areas2(vert, faces) == 0).all()
    check_no_unreferenced(vert, faces)
    v = [0.0] * 8
    v[7] = -1.0
    vert, _, faces = extract(cube(v))
    assert len(faces) == 6 and (mr.areas2(vert, faces) > 0).all()     # t = 0 of seven different owners
    v = [-1.0] + [0.0] * 7
    vert, _, faces = extract(np.pad(cube(v), ((0, 1), (0, 1), (0, 1)), constant_values=0.0))
    assert len(faces) == 6


def test_uniform_volumes_give_nothing():
    for value in (1.0, -1.0, NAN):
        vert, col, faces = extract(np.full((4, 3, 5), value))
        assert vert.shape == (0, 3) and col.shape == (0, 3) and faces.shape == (0, 3) and faces.dtype == np.int32


def test_vertex_and_triangle_order():
    rng = np.random.default_rng(3)
    vol = rng.normal(0, 1, (4, 5, 3))
    vol[rng.random(vol.shape) < 0.2] = NAN
    vert, _, faces = extract(vol)
    assert len(faces) > 20
    # vertices ascend in (owner's linear index, edge type): the owner is the lattice point below the vertex
    own = np.floor(vert + 1e-12).astype(int)
    lin = (own[:, 2] * 5 + own[:, 1]) * 3 + own[:, 0]
    assert (np.diff(lin) >= 0).all()
    frac = vert - own
    etype = (frac[:, 0] > 1e-12) * 1 + (frac[:, 1] > 1e-12) * 2 + (frac[:, 2] > 1e-12) * 4 - 1
    same = np.diff(lin) == 0
    assert (np.diff(etype)[same] > 0).all()
    # triangles ascend in the cube's linear index: the cube holds the triangle's centroid
    cen = np.floor(vert[faces].mean(1)).astype(int)
    cl = (cen[:, 2] * 4 + cen[:, 1]) * 2 + cen[:, 0]
    assert (np.diff(cl) >= 0).all()


def test_ply_mesh_round_trip(tmp_path):
    pkg = importlib.import_module(PKG_NAME)
    rng = np.random.default_rng(0)
    vert = rng.normal(0, 1, (11, 3))
    col = rng.integers(0, 256, (11, 3)).astype(np.uint8)
    faces = rng.integers(0, 11, (17, 3)).astype(np.int32)
    pkg.export2ply_mesh(vert, col, faces, path=str(tmp_path / "m"))
    v, c, f = pkg.read_ply_mesh(str(tmp_path / "m.ply"))
    assert v.dtype == np.float64 and c.dtype == np.uint8 and f.dtype == np.int32
    assert np.array_equal(v, vert) and np.array_equal(c, col) and np.array_equal(f, faces)
    pkg.export2ply_mesh(np.empty((0, 3)), np.empty((0, 3), np.uint8), np.empty((0, 3), np.int32),
                        path=str(tmp_path / "e"))
    v, c, f = pkg.read_ply_mesh(str(tmp_path / "e.ply"))
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(RuntimeError, match="does not exist"):
        pkg.export2ply_mesh(vert, col, np.array([[0, 1, 11]]), path=str(tmp_path / "bad"))
    pkg.export2ply(vert, col, path=str(tmp_path / "cloud"))
    with pytest.raises(RuntimeError, match="not a mesh"):
        pkg.read_ply_mesh(str(tmp_path / "cloud.ply"))


# ---------------------------------------------------------------------------
# the integration
# ---------------------------------------------------------------------------
class Sphere14:
    """The closed sphere scene with a grey-ramp texture (colour = the view's number and the pixel)."""

    def __init__(self):
        pkg = importlib.import_module(PKG_NAME)
        self.H, self.W = 48, 64
        self.K, self.R, self.t_raw = mr.sphere14(self.H, self.W)
        self.t = self.t_raw
        self.V = len(self.K)
        self.Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in self.R])
        self.z = np.stack([dr.sphere_depth(self.K, self.Rp, self.t, self.W, self.H, v, RAD) for v in range(self.V)])
        ys, xs = np.mgrid[0:self.H, 0:self.W]
        self.rgb = np.stack([np.stack([(xs * 3 + v) % 256, (ys * 5 + 2 * v) % 256, (xs + ys + 7 * v) % 256], -1)
                             for v in range(self.V)]).astype(np.uint8)

    def cam(self):
        return self.K, self.Rp, self.t, self.W, self.H


@pytest.fixture(scope="module")
def scene():
    return Sphere14()


@pytest.fixture(scope="module")
def sphere_mesh(scene):
    n = 40
    voxel = 0.052 / n
    origin = [-0.026] * 3
    tsdf, weight, col, cnt = mr.integrate_fast(*scene.cam(), scene.rgb, scene.z, 0, scene.V, (n, n, n), origin, voxel,
                                               3 * voxel, 1)
    return mr.extract(tsdf, col, cnt, origin, voxel) + (voxel, tsdf, weight, cnt)


def test_integrate_fast_is_integrate(scene):
    """The numpy form against the Python floats on a small lattice that cuts the
    surface, with an origin that is no multiple of the voxel, over a view
    sub-range, with holes of every kind in the maps."""
    z = scene.z.copy()
    z[3, 20:24, 30:34] = np.inf
    z[4, 20:24, 30:34] = -1.0
    z[5, 20:24, 30:34] = 0.0
    z[6, 22, 30:34] = -np.inf
    args = (*scene.cam(), scene.rgb, z[2:13], 2, 11, (7, 5, 6), [-0.0211, -0.0093, 0.0102], 0.0021, 0.0047, 3)
    slow, fast = mr.integrate(*args), mr.integrate_fast(*args)
    for a, b in zip(slow, fast):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    tsdf, weight, col, cnt = slow
    assert np.isnan(tsdf).any() and (tsdf < 0).any() and (tsdf > 0).any() and cnt.any() and col.any()
    assert np.array_equal(np.isnan(tsdf), weight < 3)


def test_integration_rules_by_hand(scene):
    """One lattice line along the optical axis of view 0 (the camera on +x looks
    down -x at the sphere's near pole, 0.31 away)."""
    g = scene
    voxel, trunc = 0.001, 0.0025
    # points at x = 0.016 .. 0.024 on the axis: the pole is at 0.02
    tsdf, weight, col, cnt = mr.integrate(*g.cam(), g.rgb, g.z[:1], 0, 1, (8, 1, 1), [0.016, 0.0, 0.0], voxel, trunc, 1)
    line = tsdf[0, 0]
    depth = float(g.z[0, g.H // 2, g.W // 2])
    assert abs(depth - 0.31) < 1e-6
    # sdf = surface depth - point depth = x - 0.02 (to rounding); beyond -trunc hidden, clamped at +1
    want = np.array([NAN, NAN, -0.002, -0.001, 0.0, 0.001, 0.002, 0.003, 0.004]) / trunc
    assert np.array_equal(np.isnan(line), np.isnan(want))
    assert np.allclose(np.minimum(want[2:], 1.0), line[2:], rtol=0, atol=1e-6)
    assert line[-1] == 1.0 and line[-2] == 1.0
    assert weight[0, 0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert cnt[0, 0].tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0]          # |sdf| <= trunc
    assert col[0, 0, 4].tolist() == g.rgb[0, g.H // 2, g.W // 2].tolist() and col[0, 0, 8].tolist() == [0, 0, 0]
    # min_weight above every weight: all nan, the weights unchanged
    t2, w2, _, _ = mr.integrate(*g.cam(), g.rgb, g.z[:1], 0, 1, (8, 1, 1), [0.016, 0.0, 0.0], voxel, trunc, 2)
    assert np.isnan(t2).all() and np.array_equal(w2, weight)


def test_colour_is_the_rounded_mean(scene):
    g = scene
    voxel = 0.001
    tsdf, weight, col, cnt = mr.integrate(*g.cam(), g.rgb, g.z, 0, g.V, (2, 2, 2), [0.0105, 0.0105, 0.0105], voxel,
                                          0.004, 1)
    assert cnt.max() >= 3
    k, j, i = np.unravel_index(np.argmax(cnt), cnt.shape)
    P = mr.lattice_point([0.0105] * 3, voxel, i, j, k)
    px = []
    for v in range(g.V):
        x, y, z = dr.wr.project_ref(g.K[v], g.Rp[v], g.t[v], P)
        xi, yi = int(x + 0.5), int(y + 0.5)
        zu = g.z[v, yi, xi]
        if np.isfinite(zu) and abs(zu - z) <= 0.004:
            px.append(g.rgb[v, yi, xi].astype(int))
    assert len(px) == cnt[k, j, i]
    assert col[k, j, i].tolist() == [int(math.floor(sum(p[m] for p in px) / len(px) + 0.5)) for m in range(3)]


# ---------------------------------------------------------------------------
# the sphere
# ---------------------------------------------------------------------------
def test_sphere_is_closed_and_of_genus_zero(sphere_mesh):
    vert, col, faces = sphere_mesh[:3]
    print(f"sphere14: {len(vert)} vertices, {len(faces)} faces")
    uses = mr.edge_uses(faces)
    assert all(n == 1 for n in uses.values())                          # no directed edge twice
    assert all((b, a) in uses for a, b in uses)                        # every edge once each way: two triangles
    edges = len(uses) // 2
    assert len(vert) - edges + len(faces) == 2
    assert (mr.areas2(vert, faces) > 0).all()
    check_no_unreferenced(vert, faces)


def test_sphere_quality(sphere_mesh):
    vert, col, faces, voxel = sphere_mesh[:4]
    r = np.abs(np.linalg.norm(vert, axis=1) - RAD) / voxel
    ratio = mr.enclosed_volume(vert, faces) / (4 * math.pi * RAD ** 3 / 3)
    print(f"sphere14: radial error median {np.median(r):.4f} p95 {np.percentile(r, 95):.4f} max {r.max():.4f} voxels, "
          f"volume ratio {ratio:.5f}")
    # measured 0.0833, 0.2608, 0.7095 and 1.00286 (the module's docstring): a factor 2, twice the deviation
    assert np.median(r) <= 2 * 0.0833 and np.percentile(r, 95) <= 2 * 0.2608 and r.max() <= 2 * 0.7095
    assert abs(ratio - 1.0) <= 2 * 0.00286
    # a positive volume of a consistently oriented closed surface: the triangles face outward
    assert col.any()


def test_ring_cameras_leave_an_open_but_oriented_surface():
    """synthetic.sphere_scene's ring cameras do not see the poles: the surface
    has a boundary there, and is consistently oriented everywhere."""
    pkg = importlib.import_module(PKG_NAME)
    K, R, t = pkg.synthetic.ring_cameras(12, 48, 64, 0.33)
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    z = np.stack([dr.sphere_depth(K, Rp, t, 64, 48, v, RAD) for v in range(12)])
    n = 24
    voxel = 0.052 / n
    rgb = np.zeros((12, 48, 64, 3), np.uint8)
    tsdf, _, col, cnt = mr.integrate_fast(K, Rp, t, 64, 48, rgb, z, 0, 12, (n, n, n), [-0.026] * 3, voxel, 3 * voxel, 1)
    vert, _, faces = mr.extract(tsdf, col, cnt, [-0.026] * 3, voxel)
    und, directed, boundary, _ = mr.manifold_report(faces)
    print(f"ring: {len(vert)} vertices, {len(faces)} faces, {boundary} boundary edges")
    assert len(faces) > 1000 and und <= 2 and directed <= 1


def test_mesh_grid():
    lo, voxel, dims, trunc = mr.mesh_grid(None, ([0.0, 0.0, 0.0], [1.0, 0.5, 0.26]), 10, 3.0)
    assert lo.tolist() == [0, 0, 0] and voxel == 0.1 and dims == (10, 5, 3) and trunc == 3.0 * 0.1
    # by hand: 201 equidistant points per axis put the 0.5 and 99.5 percentiles on the second and the last but one
    assert mr.percentile([0.0, 10.0], 25) == 2.5 and mr.percentile([10.0, 0.0], 75) == 7.5 and mr.percentile([3.0], 99.5) == 3.0
    line = np.arange(201.0)[:, None] * [1.0, 2.0, 0.5]
    pkg = importlib.import_module(PKG_NAME)
    for fn in (mr.mesh_grid, pkg._lib.mesh_grid):
        lo, voxel, dims, trunc = fn(line[::-1], None, 99, 1.0)          # box (1, 2, 0.5) .. (199, 398, 99.5), then 8 more
        assert voxel == 4.0 and trunc == 4.0 and lo.tolist() == [-7.0, -6.0, -7.5] and dims == (54, 103, 29)
    pts = np.random.default_rng(0).uniform(-1, 1, (1000, 3)) * [1.0, 0.5, 0.1]
    lo, voxel, dims, trunc = mr.mesh_grid(pts, None, 20, 2.0)
    p0, p1 = np.percentile(pts, 0.5, axis=0), np.percentile(pts, 99.5, axis=0)
    assert voxel == (p1 - p0).max() / 20 and np.array_equal(lo, p0 - 2.0 * (2.0 * voxel))
    assert dims[0] == 20 + 8 and dims[2] >= 1
    pkg = importlib.import_module(PKG_NAME)
    for a, b in zip(pkg._lib.mesh_grid(pts, None, 20, 2.0), (lo, voxel, dims, trunc)):
        assert np.array_equal(a, b)
    with pytest.raises(RuntimeError):
        mr.mesh_grid(np.empty((0, 3)), None, 20, 2.0)


def test_mesh_needs_depth_maps():
    """DensePointsWarped(mesh=N) without depth_maps is refused before anything is read, and main.py
    -mesh without -depth_maps is an argument error."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    pkg = importlib.import_module(PKG_NAME)
    with pytest.raises(RuntimeError, match="mesh needs depth_maps"):
        pkg.DensePointsWarped([], None, mesh=64)
    with pytest.raises(RuntimeError, match="mesh must be >= 0"):
        pkg.DensePointsWarped([], None, mesh=-1, depth_maps="maps")
    for extra in (["--warped", "-mesh", "64"], ["-depth_maps", "maps", "-mesh", "64"],
                  ["--warped", "-depth_maps", "maps", "-mesh", "-3"]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "-img_p", "nowhere", *extra],
                           capture_output=True, text=True)
        assert r.returncode == 2 and "-mesh" in r.stderr, (extra, r.returncode, r.stderr)
