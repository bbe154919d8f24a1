"""The signed-distance fusion and marching tetrahedra on the GPU
(k_wtsdf_integrate, k_wmesh_mark / _vcount / _scan / _vertex / _tri and
MvsContext.mesh_depth) against the float64 restatement (tests/mesh_reference.py).

Every comparison is exact, with no element left out and no tolerance: the bits
of tsdf, weight, rgb, cnt, of the vertices, their colours, the faces and the
totals; every output is filled with a canary pattern before each call.

Sizes: the integration's workgroup is a brick of 16 x 4 x 4 lattice points
(lattices of 2 x 2 x 2, 6 x 8 x 4, 66 x 3 x 3 and 41^3 points: none a multiple,
one brick and many); the extraction's workgroups hold 256 cubes or points (767
and 64,000 cubes; 240 cubes in one partial workgroup).
"""
import ctypes

import numpy as np
import pytest

import mesh_reference as mr
import warped_reference as wr
import warped_shapes as ws
from test_wmesh_host import RAD, Sphere14

pytestmark = pytest.mark.gpu


class G:
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
def s14(pkg):
    yield from _scene(pkg, Sphere14())


@pytest.fixture(scope="module")
def ring80(pkg):
    yield from _scene(pkg, ws.Scene(*pkg.synthetic.ring_scene(V=80, H=48, W=64)))


@pytest.fixture(scope="module")
def ring_small(pkg):
    yield from _scene(pkg, ws.ring(63))                        # 23 x 29


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def gpu_integrate(g, z, v0, nv, dims, origin, voxel, trunc, min_weight):
    import torch
    dev = torch.device("cuda:0")
    shape = (dims[2] + 1, dims[1] + 1, dims[0] + 1)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tz = _dev(np.asarray(z, np.float64).reshape(nv, g.H, g.W))
        tsdf = torch.full(shape, -77.0, dtype=torch.float64, device=dev)
        weight = torch.full(shape, -77, dtype=torch.int32, device=dev)
        rgb = torch.full(shape + (3,), 77, dtype=torch.uint8, device=dev)
        cnt = torch.full(shape, 77, dtype=torch.uint8, device=dev)
        g.ctx.wtsdf_integrate_device(tz, v0, nv, dims, origin, voxel, trunc, min_weight, tsdf, weight, rgb, cnt,
                                     stream=st.cuda_stream)
        out = tsdf.cpu().numpy(), weight.cpu().numpy(), rgb.cpu().numpy(), cnt.cpu().numpy()
    st.synchronize()
    return out


def compare_integrate(g, z, v0, nv, dims, origin, voxel, trunc, min_weight=1, label=""):
    points = (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    fn = mr.integrate if points * nv <= 20000 else mr.integrate_fast
    want = fn(*g.cam(), g.sc.rgb, z, v0, nv, dims, origin, voxel, trunc, min_weight)
    got = gpu_integrate(g, z, v0, nv, dims, origin, voxel, trunc, min_weight)
    for name, a, b in zip(("tsdf", "weight", "rgb", "cnt"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (label, name)
        assert a.tobytes() == b.tobytes(), (label, name, int((a != b).sum()))
    return want


def ring_depths(g, seed, holes=False):
    """Depth maps around the rings' distance from the origin (0.66), varying by +-2 cm per pixel."""
    rng = np.random.default_rng([seed, g.V, g.H, g.W])
    z = 0.66 + rng.uniform(-0.02, 0.02, (g.V, g.H, g.W))
    if holes:
        kind = rng.integers(0, 12, z.shape)
        for k, value in enumerate((np.nan, -1.0, 0.0, np.inf, -np.inf, -0.0)):
            z[kind == k] = value
    return z


# ---------------------------------------------------------------------------
# 1. the integration
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_volume(s14):
    """41^3 lattice points over the sphere, the origin no multiple of the voxel -> (want, origin, voxel)."""
    n, voxel = 40, 0.0013
    origin = [-0.02613, -0.02587, -0.02601]
    want = compare_integrate(s14, s14.sc.z, 0, s14.V, (n, n, n), origin, voxel, 3 * voxel, 1, "sphere 41^3")
    return want, origin, voxel


def test_integrate_sphere(sphere_volume):
    tsdf, weight, rgb, cnt = sphere_volume[0]
    assert (tsdf < 0).sum() > 1000 and (tsdf > 0).sum() > 1000 and np.isnan(tsdf).any()
    assert weight.max() >= 7 and cnt.max() >= 3 and rgb.any()


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 7, 3), (65, 2, 2)])
def test_integrate_small_lattices(ring80, dims):
    g = ring80
    z = ring_depths(g, 1)
    span = 0.16                                               # +-0.08 m: past the image's 0.064 m half-width
    voxel = span / max(dims)
    want = compare_integrate(g, z, 0, g.V, dims, [-0.08, -0.05, -0.03], voxel, 0.015, 2, f"dims {dims}")
    assert want[1].max() > 0


@pytest.mark.parametrize("views", [(3, 1), (5, 20), (60, 10), (0, 80), (79, 1)])
def test_integrate_view_ranges(ring80, views):
    g = ring80
    v0, nv = views
    z = ring_depths(g, 2, holes=True)[v0:v0 + nv]
    want = compare_integrate(g, z, v0, nv, (5, 7, 3), [-0.05, -0.06, -0.03], 0.019, 0.012, 1, f"views {views}")
    assert want[1].max() > 0 and want[3].max() > 0


def test_integrate_behind_the_cameras(ring80):
    """A 2 m lattice around the ring of radius 0.66: most points lie behind some cameras."""
    g = ring80
    z = 0.3 + np.random.default_rng(5).uniform(0, 1.2, (g.V, g.H, g.W))
    origin, voxel, dims = [-1.0, -1.4, -0.6], 0.4, (5, 7, 3)
    behind = 0
    for k in range(dims[0] + 1):
        P = mr.lattice_point(origin, voxel, k, 3, 1)
        behind += sum(wr.project_ref(g.sc.K[v], g.sc.Rp[v], g.sc.t[v], P)[2] <= 0 for v in range(g.V))
    assert behind > 10
    compare_integrate(g, z, 0, g.V, dims, origin, voxel, 0.5, 1, "behind")


@pytest.mark.parametrize("side", ["right", "left"])
def test_integrate_at_the_image_border(ring80, side):
    """A line of 66 lattice points whose projections into view 20 (the camera on
    +y, image x along world x) cross the border in steps of 0.023 px: nearest
    pixel W - 1 on [W - 1, W - 0.5), nothing on [W - 0.5, W) and beyond; pixel 0
    on [0, 0.5), nothing below 0."""
    g = ring80
    v = 20
    f, depth = float(g.sc.K[v][0, 0]), 0.6619
    x_from = g.W - 1.2 if side == "right" else -0.8
    voxel = 1.5 / 65 * depth / f
    origin = [(x_from - g.W / 2) * depth / f, 0.0, 0.0]
    dims = (65, 2, 2)
    xs = [wr.project_ref(g.sc.K[v], g.sc.Rp[v], g.sc.t[v], mr.lattice_point(origin, voxel, i, 0, 0))[0]
          for i in range(66)]
    if side == "right":
        assert any(g.W - 1 <= x < g.W - 0.5 for x in xs) and any(g.W - 0.5 <= x < g.W for x in xs)
        assert any(x >= g.W for x in xs) and any(x < g.W - 1 for x in xs)
    else:
        assert any(0 <= x < 0.5 for x in xs) and any(-0.5 < x < 0 for x in xs) and any(x >= 0.5 for x in xs)
    z = ring_depths(g, 3)[v:v + 1]
    want = compare_integrate(g, z, v, 1, dims, origin, voxel, 0.05, 1, f"border {side}")
    assert set(np.unique(want[1]).tolist()) == {0, 1}


def test_integrate_crafted_holes_tiny_trunc_and_high_min_weight(ring80):
    g = ring80
    z = ring_depths(g, 4, holes=True)[10:30]
    args = (g, z, 10, 20, (5, 7, 3), [-0.05, -0.06, -0.03], 0.019)
    want = compare_integrate(*args, 0.012, 1, "holes")
    assert 0 < want[1].max() < 20
    tiny = compare_integrate(*args, 1e-9, 1, "trunc 1e-9")
    seen = tiny[0][~np.isnan(tiny[0])]
    assert len(seen) and (seen == 1.0).all() and not tiny[3].any()
    none = compare_integrate(*args, 0.012, 21, "min_weight 21")
    assert np.isnan(none[0]).all() and np.array_equal(none[1], want[1])


def test_integrate_odd_image(ring_small):
    g = ring_small
    z = ring_depths(g, 6, holes=True)
    want = compare_integrate(g, z, 0, g.V, (6, 4, 5), [-0.07, -0.04, -0.05], 0.021, 0.015, 1, "23 x 29")
    assert want[1].max() > 3


def test_integrate_host_pointers(ring80):
    g = ring80
    z = ring_depths(g, 7, holes=True)[4:9]
    want = mr.integrate(*g.cam(), g.sc.rgb, z, 4, 5, (5, 7, 3), [-0.05, -0.06, -0.03], 0.019, 0.012, 2)
    got = g.ctx.wtsdf_integrate(z, (5, 7, 3), [-0.05, -0.06, -0.03], 0.019, 0.012, 2, views=(4, 5))
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 2. the extraction
# ---------------------------------------------------------------------------
def gpu_extract(g, vol, rgb, cnt, origin, voxel, cap_v, cap_t):
    """mvs_wmesh_extract_device into canary-filled outputs of cap_v and cap_t rows -> vert, vcol, tri, total."""
    import torch
    dev = torch.device("cuda:0")
    nz, ny, nx = (n - 1 for n in vol.shape)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tv, tr, tc = _dev(np.asarray(vol, np.float64)), _dev(rgb), _dev(cnt)
        vert = torch.full((cap_v, 3), -77.0, dtype=torch.float64, device=dev) if cap_v else None
        vcol = torch.full((cap_v, 3), 77, dtype=torch.uint8, device=dev) if cap_v else None
        tri = torch.full((cap_t, 3), -77, dtype=torch.int32, device=dev) if cap_t else None
        total = torch.full((2,), -77, dtype=torch.int64, device=dev)
        g.ctx.wmesh_extract_device((nx, ny, nz), origin, voxel, tv, tr, tc, vert, vcol, tri, total,
                                   stream=st.cuda_stream)
        out = tuple(None if x is None else x.cpu().numpy() for x in (vert, vcol, tri, total))
    st.synchronize()
    return out


def compare_extract(g, vol, rgb, cnt, origin, voxel, want=None, caps=None, label=""):
    want = mr.extract(vol, rgb, cnt, origin, voxel) if want is None else want
    n, m = len(want[0]), len(want[2])
    cap_v, cap_t = (n + 5, m + 5) if caps is None else caps
    vert, vcol, tri, total = gpu_extract(g, vol, rgb, cnt, origin, voxel, cap_v, cap_t)
    assert total.tolist() == [n, m], (label, total)
    kv, kt = min(n, cap_v), min(m, cap_t)
    if cap_v:
        assert vert[:kv].tobytes() == want[0][:kv].tobytes(), label
        assert vcol[:kv].tobytes() == want[1][:kv].tobytes(), label
        assert (vert[kv:] == -77.0).all() and (vcol[kv:] == 77).all(), label        # nothing past the total or the cap
    if cap_t:
        assert tri.dtype == np.int32 and tri[:kt].tobytes() == want[2][:kt].tobytes(), label
        assert (tri[kt:] == -77).all(), label
    return want


def random_colours(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape + (3,)).astype(np.uint8), (rng.integers(0, 3, shape) * 100).astype(np.uint8)


def test_extract_all_256_sign_patterns(s14):
    """Cube p of a 2 x 2 x 768 lattice holds pattern p; a nan column after each
    kills the two cubes between neighbours (their corners 7 and 0)."""
    vol = np.full((2, 2, 768), np.nan)
    for p in range(256):
        for c in range(8):
            vol[c >> 2 & 1, c >> 1 & 1, 3 * p + (c & 1)] = -1.0 - 0.01 * c if p >> c & 1 else 1.0 + 0.03 * c
    rgb, cnt = random_colours(vol.shape, 1)
    want = compare_extract(s14, vol, rgb, cnt, [0.5, -1.0, 2.0], 0.25, label="256 patterns")
    # the cubes do not touch: the whole is the sum of the 256 single cubes
    assert len(want[2]) == sum(len(mr.extract(vol[:, :, 3 * p:3 * p + 2], rgb[:, :, 3 * p:3 * p + 2],
                                              cnt[:, :, 3 * p:3 * p + 2], [0, 0, 0], 1.0)[2]) for p in range(256))


def test_extract_random_volume_with_nan_and_zeros(s14):
    rng = np.random.default_rng(9)
    vol = rng.normal(0, 1, (5, 6, 9))
    kind = rng.random(vol.shape)
    vol[kind < 0.3] = np.nan
    vol[(kind >= 0.3) & (kind < 0.36)] = 0.0
    vol[(kind >= 0.36) & (kind < 0.4)] = -0.0
    rgb, cnt = random_colours(vol.shape, 2)
    want = compare_extract(s14, vol, rgb, cnt, [0.1, 0.2, 0.3], 0.7, label="random 9 x 6 x 5")
    assert len(want[2]) > 30
    vert, vcol, tri, total = s14.ctx.wmesh_extract(vol, rgb, cnt, [0.1, 0.2, 0.3], 0.7)          # host pointers
    assert total.tolist() == [len(want[0]), len(want[2])]
    for a, b in zip((vert, vcol, tri), want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    vert, vcol, tri, total = s14.ctx.wmesh_extract(vol, rgb, cnt, [0.1, 0.2, 0.3], 0.7, cap_v=3, cap_t=2)
    assert total.tolist() == [len(want[0]), len(want[2])]
    assert vert.tobytes() == want[0][:3].tobytes() and tri.tobytes() == want[2][:2].tobytes()


@pytest.fixture(scope="module")
def sphere_surface(s14, sphere_volume):
    (tsdf, _, rgb, cnt), origin, voxel = sphere_volume
    return mr.extract(tsdf, rgb, cnt, origin, voxel)


def test_extract_sphere_twice(s14, sphere_volume, sphere_surface):
    (tsdf, _, rgb, cnt), origin, voxel = sphere_volume
    want = sphere_surface
    n, m = len(want[0]), len(want[2])
    assert n > 10000 and m > 20000
    _, _, boundary, _ = mr.manifold_report(want[2])
    assert boundary == 0
    compare_extract(s14, tsdf, rgb, cnt, origin, voxel, want=want, label="sphere")
    a = gpu_extract(s14, tsdf, rgb, cnt, origin, voxel, n, m)
    b = gpu_extract(s14, tsdf, rgb, cnt, origin, voxel, n, m)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("caps", [(0, 0), (1, 1), (5000, 9999), (0, 300), (300, 0), (10 ** 5, 7)])
def test_extract_caps(s14, sphere_volume, sphere_surface, caps):
    (tsdf, _, rgb, cnt), origin, voxel = sphere_volume
    compare_extract(s14, tsdf, rgb, cnt, origin, voxel, want=sphere_surface, caps=caps, label=f"caps {caps}")


@pytest.mark.parametrize("value", [1.0, -1.0, float("nan")])
def test_extract_empty(s14, value):
    vol = np.full((4, 7, 11), value)                          # 240 cubes: one partial workgroup
    rgb, cnt = random_colours(vol.shape, 3)
    want = compare_extract(s14, vol, rgb, cnt, [0, 0, 0], 1.0, label=f"all {value}")
    assert len(want[0]) == 0 and len(want[2]) == 0
    compare_extract(s14, vol, rgb, cnt, [0, 0, 0], 1.0, want=want, caps=(0, 0))


# ---------------------------------------------------------------------------
# 3. the chain
# ---------------------------------------------------------------------------
CHAIN_KEYS = ("vertices", "colors", "faces", "tsdf", "weight", "origin", "dims")


@pytest.mark.parametrize("kw", [{"bounds": ([-0.026, -0.026, -0.026], [0.026, 0.024, 0.02]), "resolution": 24},
                                {"resolution": 20, "trunc_voxels": 2.0, "min_weight": 2, "rel_tol": 0.02,
                                 "min_consistent": 1, "max_violations": 1, "views": (1, 12)}])
def test_chain_is_the_restatement(s14, orc, pkg, kw):
    """score, the chain twice on the side stream, score on one context: the
    chain is the restatement's, bit-identical both times, and both score results
    are the oracle's."""
    g = s14
    v0, nv = kw.get("views", (0, g.V))
    rng = np.random.default_rng(8)
    d = rng.normal(0, 1, (500, 3))
    maps = {"z": g.sc.z[v0:v0 + nv], "points": RAD * d / np.linalg.norm(d, axis=1, keepdims=True)}
    c, ref = pkg.synthetic.candidates(512, g.sc.K, g.sc.R, g.sc.t_raw, W=g.W, H=g.H, seed=3)
    first = g.ctx.score(c, ref, 0.7, 5)
    a = pkg.mesh_depth_warped(g.ctx, maps, **kw)
    b = g.ctx.mesh_depth(maps, **kw)
    again = g.ctx.score(c, ref, 0.7, 5)
    want = mr.mesh_chain(*g.cam(), g.sc.rgb, maps, **kw)
    assert len(want["faces"]) > 1000 and want["faces"].dtype == np.int32
    assert a["voxel"] == want["voxel"] == b["voxel"]
    for k in CHAIN_KEYS:
        assert a[k].dtype == want[k].dtype and a[k].shape == want[k].shape, k
        assert a[k].tobytes() == want[k].tobytes(), k
        assert a[k].tobytes() == b[k].tobytes(), k
    sc = orc.Scene(g.sc.rgb, g.sc.K, g.sc.R, g.sc.t_raw).score_batch(c, ref, 0.7, 5)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    for x, w in zip(first[:3], sc[:3]):
        assert np.array_equal(x, w)
    assert np.allclose(first[3], sc[3], rtol=0, atol=1e-12)
    und, directed, boundary, _ = mr.manifold_report(a["faces"])
    assert und <= 2 and directed <= 1
    print(f"chain {kw}: {len(a['vertices'])} vertices, {len(a['faces'])} faces, {boundary} boundary edges")


def test_chain_refuses(s14):
    g = s14
    with pytest.raises(RuntimeError, match="no 'z'"):
        g.ctx.mesh_depth({"points": np.zeros((3, 3))})
    with pytest.raises(RuntimeError, match="no points"):
        g.ctx.mesh_depth({"z": g.sc.z})
    with pytest.raises(RuntimeError, match="view range"):
        g.ctx.mesh_depth({"z": g.sc.z}, views=(10, 9), bounds=([0, 0, 0], [1, 1, 1]))
    with pytest.raises(RuntimeError, match="2\\^27"):
        g.ctx.mesh_depth({"z": g.sc.z}, bounds=([0, 0, 0], [1, 1, 1]), resolution=600)
    empty = g.ctx.mesh_depth({"z": np.full_like(g.sc.z, np.inf)}, bounds=([0, 0, 0], [1, 1, 1]), resolution=4)
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and np.isnan(empty["tsdf"]).all()


def test_dense_points_warped_writes_the_mesh(pkg, tmp_path, capsys):
    """MVS2.DensePointsWarped(depth_maps=DIR, mesh=N) on test_seed_gpu's planted
    sphere: the mesh is MvsContext.mesh_depth of the maps at resolution N, the
    file holds it, and the count line and last_stats gain the counts."""
    import types

    import seed_reference as sd
    from test_seed_gpu import write_pars
    p = sd.planted(pkg)
    par = str(tmp_path / "par.txt")
    write_pars(par, p["K"], p["R"], p["t_raw"])
    imgs = [p["rgb"][v] for v in range(len(p["rgb"]))]
    out = pkg.DensePointsWarped(imgs, types.SimpleNamespace(par_path=par), rounds=2, iterations=1, epi_px=1.5,
                                feats=p["feats"], pairs=p["pairs"], path=str(tmp_path / "cloud"),
                                depth_maps=str(tmp_path / "maps"), depth_radius=2, dense_path=str(tmp_path / "dense"),
                                mesh=40, mesh_path=str(tmp_path / "mesh"))
    mesh = out["mesh"]
    with pkg.MvsContext(p["rgb"], p["K"], p["R"], p["t_raw"], device=0) as ctx:
        want = ctx.mesh_depth(out["maps"], resolution=40)
    for k in CHAIN_KEYS:
        assert mesh[k].tobytes() == want[k].tobytes(), k
    n, m = len(mesh["vertices"]), len(mesh["faces"])
    assert n > 500 and m > 500 and max(mesh["dims"]) >= 40
    assert out["counts"]["mesh_vertices"] == n == pkg.MVS2.last_stats["mesh_vertices"]
    assert out["counts"]["mesh_faces"] == m == pkg.MVS2.last_stats["mesh_faces"]
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("warped:")]
    assert len(line) == 1 and line[0].endswith(f" mesh vertices {n} faces {m}")
    v, c, f = pkg.read_ply_mesh(str(tmp_path / "mesh.ply"))
    assert v.tobytes() == mesh["vertices"].tobytes() and c.tobytes() == mesh["colors"].tobytes()
    assert f.tobytes() == mesh["faces"].tobytes()
    und, directed, boundary, _ = mr.manifold_report(mesh["faces"])
    assert und <= 2 and directed <= 1
    r = np.linalg.norm(mesh["vertices"], axis=1)
    print(f"{n} vertices, {m} faces, {boundary} boundary edges; within 5 % of the radius "
          f"{float((np.abs(r - p['rad']) <= 0.05 * p['rad']).mean()):.4f}")


# ---------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------
def test_arguments(pkg, s14):
    g = s14
    lib = pkg._lib.load()
    h = g.ctx.handle
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails its checks
    V = g.V
    good = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def org(*v):
        return (ctypes.c_double * 3)(*v)

    def integ(zmap=one, v0=0, nv=V, nx=2, ny=2, nz=2, origin=good, voxel=1.0, trunc=1.0, min_weight=1, tsdf=one,
              weight=one, rgb=one, cnt=one):
        return lib.mvs_wtsdf_integrate_device(h, zmap, v0, nv, nx, ny, nz, origin, voxel, trunc, min_weight, tsdf,
                                              weight, rgb, cnt, None)

    def ext(nx=2, ny=2, nz=2, origin=good, voxel=1.0, tsdf=one, rgb=one, cnt=one, cap_v=1, cap_t=1, vert=one,
            vcol=one, tri=one, total=one):
        return lib.mvs_wmesh_extract_device(h, nx, ny, nz, origin, voxel, tsdf, rgb, cnt, cap_v, cap_t, vert, vcol,
                                            tri, total, None)

    cases = [(lambda: integ(nx=0), "must be >= 1"), (lambda: integ(ny=-1), "must be >= 1"),
             (lambda: integ(nz=0), "must be >= 1"),
             (lambda: integ(nx=511, ny=511, nz=512), "2^27"), (lambda: integ(nx=2 ** 31 - 1), "2^27"),
             (lambda: integ(nx=2 ** 27 - 1, ny=1, nz=1), "2^27"),
             (lambda: integ(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), "2^27"),
             (lambda: integ(origin=None), "origin"), (lambda: integ(origin=org(0.0, nan, 0.0)), "origin must be finite"),
             (lambda: integ(origin=org(inf, 0.0, 0.0)), "origin must be finite"),
             (lambda: integ(voxel=0.0), "voxel"), (lambda: integ(voxel=-1.0), "voxel"), (lambda: integ(voxel=nan), "voxel"),
             (lambda: integ(voxel=inf), "voxel"),
             (lambda: integ(trunc=0.0), "trunc"), (lambda: integ(trunc=nan), "trunc"), (lambda: integ(trunc=inf), "trunc"),
             (lambda: integ(trunc=-1.0), "trunc"),
             (lambda: integ(min_weight=0), "min_weight"), (lambda: integ(min_weight=-3), "min_weight"),
             (lambda: integ(v0=-1), "view range"), (lambda: integ(v0=1), "view range"), (lambda: integ(nv=0), "view range"),
             (lambda: integ(v0=V, nv=1), "view range"), (lambda: integ(v0=2 ** 31 - 1, nv=2 ** 31 - 1), "view range"),
             (lambda: integ(zmap=None), "null pointer"), (lambda: integ(tsdf=None), "null pointer"),
             (lambda: integ(weight=None), "null pointer"), (lambda: integ(rgb=None), "null pointer"),
             (lambda: integ(cnt=None), "null pointer"),
             (lambda: ext(nx=0), "must be >= 1"), (lambda: ext(nx=511, ny=511, nz=512), "2^27"),
             (lambda: ext(origin=None), "origin"), (lambda: ext(origin=org(0.0, 0.0, nan)), "origin must be finite"),
             (lambda: ext(voxel=0.0), "voxel"), (lambda: ext(voxel=nan), "voxel"), (lambda: ext(voxel=inf), "voxel"),
             (lambda: ext(cap_v=-1), "cap_v < 0"), (lambda: ext(cap_t=-1), "cap_t < 0"),
             (lambda: ext(cap_v=1 << 31), "below 2^31"), (lambda: ext(cap_t=1 << 31), "below 2^31"),
             (lambda: ext(tsdf=None), "null pointer"), (lambda: ext(rgb=None), "null pointer"),
             (lambda: ext(cnt=None), "null pointer"), (lambda: ext(total=None), "null pointer"),
             (lambda: ext(vert=None), "null pointer"), (lambda: ext(vcol=None), "null pointer"),
             (lambda: ext(tri=None), "null pointer")]
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k                   # MVS_E_ARG
        assert msg in pkg._lib.last_error(h), (k, msg, pkg._lib.last_error(h))
    # the largest lattice passes the size check (and then fails on its NULL map)
    assert integ(nx=511, ny=511, nz=511, zmap=None) == -1 and "null pointer" in pkg._lib.last_error(h)
    # the host-pointer variants run the same checks
    z = np.zeros((V, g.H, g.W))
    with pytest.raises(RuntimeError, match="trunc"):
        g.ctx.wtsdf_integrate(z, (2, 2, 2), [0, 0, 0], 1.0, 0.0)
    with pytest.raises(RuntimeError, match="min_weight"):
        g.ctx.wtsdf_integrate(z, (2, 2, 2), [0, 0, 0], 1.0, 1.0, 0)
    with pytest.raises(RuntimeError, match="view range"):
        g.ctx.wtsdf_integrate(z[:2], (2, 2, 2), [0, 0, 0], 1.0, 1.0, 1, views=(V - 1, 2))
    with pytest.raises(RuntimeError, match="origin must be finite"):
        g.ctx.wtsdf_integrate(z, (2, 2, 2), [0, np.nan, 0], 1.0, 1.0)
    vol = np.ones((2, 2, 2))
    with pytest.raises(RuntimeError, match="voxel"):
        g.ctx.wmesh_extract(vol, np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 2, 2), np.uint8), [0, 0, 0], -1.0)
    with pytest.raises(RuntimeError, match="cap_v < 0"):
        g.ctx.wmesh_extract(vol, np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 2, 2), np.uint8), [0, 0, 0], 1.0,
                            cap_v=-1, cap_t=0)
