"""One sweep of the per-pixel plane propagation on the GPU (k_wprop_sweep,
mvs_wprop_sweep_device / mvs_wprop_sweep, MvsContext.densify_depth) against the
float64 restatement (tests/prop_reference.py) on the same input maps.

The comparison rule (test_refine_gpu.py's, adapted), per view of a case:
  scores   |gpu - ref| <= the mean over the hypothesis's top_k chosen views of
           1e-8 / min(1, sigma_b);
  nan      the pattern is equal, except for hypotheses on a band -- a border
           margin below 1e-9 px, a facing margin below 1e-12, or a list view
           whose reference ncc lies within its tolerance of min_ncc -- which are
           left out, at most 0.5 % of a case's hypotheses (the seeded inputs
           below hit none: the count is asserted to be 0);
  choice   the restatement's score of the GPU's best is within twice the
           tolerance of the restatement's best score; best is 0 whenever the
           restatement's own-plane score exceeds every other by more than that;
           score equals scores[best] bitwise.  Index equality is not demanded:
           the pixels of one splat footprint hold the same plane, so
           equal-score hypotheses are the normal case;
  geometry z_out, n_out of the GPU's best match the restatement's geometry of
           that index within 1e-13 relative; for best = 0 they are the inputs
           bit for bit, for best in 1..4 n_out is the neighbour's normal bit
           for bit.
Every output is filled with a canary before the call and must be written whole.

Shapes: a wave owns 16 consecutive pixels and a workgroup 64, so 26 x 31 = 806,
39 x 45, 45 x 61 and 23 x 29 end in a partial wave and a partial workgroup;
lanes are (hypothesis, list view) in segments of the next power of two >= |T|,
so |T| = 1, 3, 4, 5 and 23 take segments of 1, 4, 4, 8 and 32 lanes, and HY = 5,
32, 50 and 180 hypotheses take one to many passes.
"""
import ctypes
import math

import numpy as np
import pytest

import depth_reference as dr
import prop_reference as pr
import warped_reference as wr
import warped_shapes as ws
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

A8 = math.radians(8)
CANARY = -77.0


class G:
    """A warped_shapes.Scene with its context."""

    def __init__(self, pkg, sc):
        import torch
        assert torch.cuda.is_available(), "GPU test without a GPU"
        self.sc = sc
        self.ctx = pkg.MvsContext(sc.rgb, sc.K, sc.R, sc.t_raw, device=0)
        assert np.array_equal(self.ctx.rproj(), sc.Rp)
        self.V, self.H, self.W = sc.V, sc.H, sc.W


def _scene(pkg, sc):
    g = G(pkg, sc)
    yield g
    g.ctx.close()


@pytest.fixture(scope="module")
def s26(pkg):
    yield from _scene(pkg, ws.sphere(26, 31))


@pytest.fixture(scope="module")
def s39(pkg):
    yield from _scene(pkg, ws.sphere(39, 45))


@pytest.fixture(scope="module")
def s45(pkg):
    yield from _scene(pkg, ws.sphere(45, 61))


@pytest.fixture(scope="module")
def ring130(pkg):
    yield from _scene(pkg, ws.ring(130))                       # 23 x 29


@pytest.fixture(scope="module")
def wide(pkg):
    yield from _scene(pkg, ws.Scene(*pkg.synthetic.ring_scene(V=3, H=41, W=2061)))


@pytest.fixture(scope="module")
def big(pkg):
    yield from _scene(pkg, ws.Scene(*pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=0.02)[:4]))


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


KW = dict(wid=5, min_cos=0.3, min_ncc=0.7, top_k=2, step=1, kd=1, ka=1, astep=A8, depth_px=1.0, step_scale=1.0)


def gpu_sweep(g, zmap, nmap, lists, v0, want_scores=True, stream=None, **kw):
    """mvs_wprop_sweep_device on outputs pre-filled with a canary -> dict."""
    import torch
    k = dict(KW, **kw)
    dev = torch.device("cuda:0")
    nv = len(lists)
    hy = pr.n_hyp(k["kd"], k["ka"])
    st = torch.cuda.Stream(dev) if stream is None else stream
    with torch.cuda.stream(st):
        z = _dev(np.asarray(zmap, np.float64).reshape(nv, g.H, g.W))
        n = _dev(np.asarray(nmap, np.float64).reshape(nv, g.H, g.W, 3))
        zo = torch.full((nv, g.H, g.W), CANARY, dtype=torch.float64, device=dev)
        no = torch.full((nv, g.H, g.W, 3), CANARY, dtype=torch.float64, device=dev)
        sc = torch.full((nv, g.H, g.W), CANARY, dtype=torch.float64, device=dev)
        be = torch.full((nv, g.H, g.W), -77, dtype=torch.int32, device=dev)
        ss = torch.full((nv, g.H, g.W, hy), CANARY, dtype=torch.float64, device=dev) if want_scores else None
        g.ctx.wprop_sweep_device(z, n, lists, v0, nv, zo, no, sc, be, ss, stream=st.cuda_stream, **k)
        out = {"z": zo.cpu().numpy(), "normal": no.cpu().numpy(), "score": sc.cpu().numpy(), "best": be.cpu().numpy()}
        if want_scores:
            out["scores"] = ss.cpu().numpy()
    st.synchronize()
    return out


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_view(got, o, zmap_v, nmap_v, min_ncc, top_k, step, label):
    """The comparison rule for one view: got = the GPU's arrays of the view, o =
    pr.sweep_view(..., details=True).  -> (hypotheses that exist on tested pixels, left out)."""
    Hh, W, HY = o["scores"].shape
    gs, rs = got["scores"], o["scores"]
    best, score = got["best"], got["score"]
    assert not (gs == CANARY).any() and not (got["z"] == CANARY).any() and not (got["normal"] == CANARY).any(), label
    assert not (score == CANARY).any() and not (best == -77).any(), label
    tested = o["exists"] & o["ok"][..., None]
    # every hypothesis that does not exist, and every pixel that fails its test, is nan
    assert np.isnan(gs[~tested]).all(), label
    with np.errstate(invalid="ignore", divide="ignore"):
        vt = 1e-8 / np.minimum(1.0, o["sigma_b"])                        # per (hypothesis, view)
        tol = np.where(o["chosen"], vt, 0.0).sum(-1) / top_k
        band = tested & ((np.abs(o["border"]) < 1e-9).any(-1) | (np.abs(o["cosm"]) < 1e-12).any(-1)
                         | (np.abs(o["ncc"] - min_ncc) <= vt).any(-1))
    left = int(band.sum())
    cmp = tested & ~band
    assert np.array_equal(np.isnan(gs[cmp]), np.isnan(rs[cmp])), label
    both = cmp & ~np.isnan(rs)
    assert (np.abs(gs[both] - rs[both]) <= tol[both]).all(), (label, float(np.abs(gs[both] - rs[both]).max()))
    # the choice
    clean = ~band.any(-1)
    assert np.array_equal(best[clean] >= 0, o["best"][clean] >= 0), label
    assert ((best >= -1) & (best < HY)).all(), label
    has = best >= 0
    bi = np.maximum(best, 0)[..., None]
    pick = lambda a: np.take_along_axis(a, bi, -1)[..., 0]
    assert same_bits(score[has], pick(gs)[has]) and np.isnan(score[~has]).all(), label
    assert np.isnan(gs[~has]).all() and np.isinf(got["z"][~has]).all() and (got["z"][~has] > 0).all(), label
    assert np.isnan(got["normal"][~has]).all(), label
    rb = np.take_along_axis(rs, np.maximum(o["best"], 0)[..., None], -1)[..., 0]
    ok = has & clean
    tb = np.maximum(pick(tol), np.take_along_axis(tol, np.maximum(o["best"], 0)[..., None], -1)[..., 0])
    assert (np.abs(pick(rs)[ok] - rb[ok]) <= 2 * tb[ok]).all(), label
    others = np.where(np.isnan(rs), -np.inf, rs)
    others[..., 0] = -np.inf
    with np.errstate(invalid="ignore"):
        own_wins = ok & (rs[..., 0] - others.max(-1) > 2 * tol.max(-1))
    assert (best[own_wins] == 0).all(), label
    # the geometry
    zr, nr = pick(o["zh"]), np.take_along_axis(o["nh"], bi[..., None], 2)[..., 0, :]
    assert (np.abs(got["z"][has] - zr[has]) <= 1e-13 * np.abs(zr[has])).all(), label
    assert (np.abs(got["normal"][has] - nr[has]).max(-1) <= 1e-13 * np.sqrt((nr[has] ** 2).sum(-1))).all(), label
    own = best == 0
    assert same_bits(got["z"][own], zmap_v[own]) and same_bits(got["normal"][own], nmap_v[own]), label
    ys, xs = np.mgrid[0:Hh, 0:W]
    for h, (ox, oy) in enumerate(pr.OFFSETS, 1):
        m = best == h
        assert same_bits(got["normal"][m], nmap_v[ys[m] + oy * step, xs[m] + ox * step]), (label, h)
    return int(tested.sum()), left


def compare(g, zmap, nmap, lists, v0, label="", **kw):
    """One sweep on the GPU against the restatement -> (hypotheses, pixels with a best >= 0, best > 0)."""
    k = dict(KW, **kw)
    got = gpu_sweep(g, zmap, nmap, lists, v0, **kw)
    hyp = left = 0
    for i in range(len(lists)):
        o = pr.sweep_view(g.sc.gray, g.sc.K, g.sc.Rp, g.sc.t, zmap[i], nmap[i], v0 + i, pr.list_of(lists[i]), **k)
        a, b = check_view({x: got[x][i] for x in got}, o, zmap[i], nmap[i], k["min_ncc"], k["top_k"], k["step"],
                          f"{label} view {v0 + i}")
        hyp += a
        left += b
    print(f"{label}: {hyp} hypotheses, {left} left out, {int((got['best'] >= 0).sum())} pixels hold a plane, "
          f"{int((got['best'] > 0).sum())} changed")
    assert left == 0 and left <= 0.005 * max(hyp, 1), label
    return hyp, int((got["best"] >= 0).sum()), int((got["best"] > 0).sum())


def noisy_maps(sc, v0, nv, n=90, seed=1, radius=2):
    """The restatement's radius-2 splat of n sphere patches whose depth is off by
    U(-1.5, 1.5) pixel footprints along the reference ray and whose normal is
    tilted by 5..15 degrees -> zmap (nv,H,W), nmap (nv,H,W,3) (nan where empty)."""
    import refine_reference as rr
    rng = np.random.default_rng([seed, sc.H, sc.W])
    c, nrm, ref = ws.border_patches(sc, n, seed)
    c, nrm = c.copy(), nrm.copy()
    for i in range(n):
        r = int(ref[i])
        u = c[i] - sc.O[r]
        depth = float(sc.Rp[r][2] @ c[i] + sc.t[r][2])
        u /= np.linalg.norm(u)
        c[i] += rng.uniform(-1.5, 1.5) * depth / ((sc.K[r][0, 0] + sc.K[r][1, 1]) / 2) * u
        e1, e2 = rr.tangent_basis(nrm[i])
        th, ph = math.radians(rng.uniform(5, 15)), rng.uniform(0, 2 * math.pi)
        w = math.cos(th) * nrm[i] + math.sin(th) * (math.cos(ph) * e1 + math.sin(ph) * e2)
        nrm[i] = w / np.linalg.norm(w)
    mask = np.full((n, sc.words), (1 << sc.V) - 1, np.uint64)
    z, idm = dr.splat(sc.K, sc.Rp, sc.t, sc.W, sc.H, c, nrm, ref, mask, radius, 4.0, v0, nv)
    nmap = np.full((nv, sc.H, sc.W, 3), np.nan)
    nmap[idm >= 0] = nrm[idm[idm >= 0]]
    return z, nmap


def ring_lists(V, v0, nv, tv, T=None):
    """Row k: the tv views after v0 + k round the ring, alternating sides; entries past T are -1."""
    out = np.full((nv, tv), -1, np.int32)
    for k in range(nv):
        v = v0 + k
        row = []
        for d in range(1, V):
            row += [(v + d) % V, (v - d) % V]
        row = list(dict.fromkeys(row))[:tv if T is None else T]
        out[k, :len(row)] = row
    return out


# ---------------------------------------------------------------------------
# 1. sphere scenes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("wid", [1, 2, 3, 4, 5])
def test_every_window_size(s26, wid):
    """26 x 31, a view range with v0 > 0 whose lists leave the range."""
    z, n = noisy_maps(s26.sc, 3, 2)
    hyp, held, moved = compare(s26, z, n, ring_lists(24, 3, 2, 4), 3, f"26x31 wid {wid}", wid=wid)
    assert hyp > 300 and held > 10 and moved > 0


@pytest.mark.parametrize("step,kd,ka,top_k,tv,T,min_ncc", [(1, 0, 0, 1, 1, 1, 0.5), (3, 1, 1, 2, 4, 4, 0.5),
                                                            (64, 2, 1, 3, 3, 3, 0.5), (3, 0, 0, 2, 5, 3, 0.5),
                                                            (1, 1, 1, 5, 5, 5, 0.5)])
def test_steps_grids_and_lists(s39, step, kd, ka, top_k, tv, T, min_ncc):
    """39 x 45 at wid 3: step 1, 3 and 64 (every neighbour outside the image), HY = 5,
    32 and 50, top_k = 1, 2 and |T|, tv 1, 3, 4, 5 and a list with a -1 tail."""
    z, n = noisy_maps(s39.sc, 0, 2, seed=2)
    hyp, held, _ = compare(s39, z, n, ring_lists(24, 0, 2, tv, T), 0, f"39x45 step {step} grid {kd},{ka} top {top_k}/{T}",
                           wid=3, step=step, kd=kd, ka=ka, top_k=top_k, min_ncc=min_ncc)
    assert hyp > 300 and (held > 0 or top_k == 5)      # five views 15 to 45 degrees away never see one window together


def test_the_largest_grid_and_the_longest_list(s45, s26):
    """45 x 61, nv = 1: HY = 180 at |T| = 3; 26 x 31: tv = 32 with |T| = 23 (segments of 32 lanes)."""
    z, n = noisy_maps(s45.sc, 7, 1, n=60, seed=3)
    hyp, held, _ = compare(s45, z, n, ring_lists(24, 7, 1, 3), 7, "45x61 grid 3,2", wid=2, kd=3, ka=2, astep=0.1,
                           step_scale=0.5)
    assert hyp > 5000 and held > 10
    z, n = noisy_maps(s26.sc, 0, 1, seed=4)
    hyp, held, _ = compare(s26, z, n, ring_lists(24, 0, 1, 32, 23), 0, "26x31 tv 32", wid=2, kd=0, ka=0, top_k=2,
                           min_cos=0.0)
    assert hyp > 100 and held > 0


def test_a_list_shorter_than_top_k_empties_its_view(s26):
    z, n = noisy_maps(s26.sc, 0, 2, seed=5)
    lists = ring_lists(24, 0, 2, 4)
    lists[1, 1:] = -1
    got = gpu_sweep(s26, z, n, lists, 0, wid=2)
    assert (got["best"][0] >= 0).any()
    assert (got["best"][1] == -1).all() and np.isnan(got["scores"][1]).all() and np.isinf(got["z"][1]).all()
    compare(s26, z, n, lists, 0, "26x31 |T| < top_k", wid=2)


def test_views_past_64_and_128(ring130):
    """23 x 29, 130 views of random texture: lists naming views >= 64 and >= 128.
    Every pixel holds a fronto-parallel plane near the origin's depth; the random
    textures correlate around 0, so min_ncc is -0.05."""
    g = ring130
    rng = np.random.default_rng(130)
    v0, nv = 126, 2
    z = np.stack([float(g.sc.t[v][2]) * rng.uniform(0.98, 1.02, (g.H, g.W)) for v in range(v0, v0 + nv)])
    n = np.stack([np.broadcast_to(-g.sc.Rp[v][2], (g.H, g.W, 3)) for v in range(v0, v0 + nv)]).copy()
    lists = np.array([[127, 128, 129, 64], [129, 5, 128, 126]], np.int32)
    hyp, held, _ = compare(g, z, n, lists, v0, "130 views", wid=2, min_cos=0.0, min_ncc=-0.05, top_k=1, kd=0, ka=0)
    assert hyp > 1000 and held > 0


def test_rows_wider_than_2048(wide):
    """41 x 2061, 3 views 120 degrees apart: every 5th pixel holds a plane whose
    normal lies between the directions to the view and to its first list view."""
    g = wide
    rng = np.random.default_rng(2061)
    z = np.full((3, g.H, g.W), np.inf)
    n = np.full((3, g.H, g.W, 3), np.nan)
    for v in range(3):
        m = rng.random((g.H, g.W)) < 0.2
        z[v][m] = float(g.sc.t[v][2]) * rng.uniform(0.99, 1.01, int(m.sum()))
        w = -g.sc.Rp[v][2] - 0.9 * g.sc.Rp[(v + 1) % 3][2]      # between the view's direction and its first list view's
        n[v][m] = w / np.linalg.norm(w)
    lists = np.array([[1, 2], [2, 0], [0, 1]], np.int32)
    kw = dict(wid=1, min_cos=0.0, min_ncc=-2.0, top_k=1, kd=0, ka=0)
    hyp, held, _ = compare(g, z, n, lists, 0, "41x2061", **kw)
    assert hyp > 50000 and held > 100
    assert (gpu_sweep(g, z, n, lists, 0, **kw)["best"][:, :, 2049:] >= 0).any()


# ---------------------------------------------------------------------------
# 2. crafted maps on the two-camera scene of test_refine_gpu.py
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(pkg):
    """test_refine_gpu.py's four cameras over one random texture: 0 and 1
    identical, 2 and 3 moved so that their samples land 3.3 px off (at depth 1)."""
    H, W = 40, 48
    rng = np.random.default_rng(7)
    gr = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
    rgb = np.tile(np.repeat(gr, 3, axis=2)[None], (4, 1, 1, 1))
    rgb[:, 30:, 36:] = 90                                        # a constant corner
    K = np.tile(np.array([[300.0, 0, 24.0], [0, 310.0, 20.0], [0, 0, 1.0]]), (4, 1, 1))
    R = np.tile(np.eye(3), (4, 1, 1))
    t = np.tile(np.array([0.01, -0.02, 0.0]), (4, 1))
    t[2] += [0.011, 0.011, 0.0]
    t[3] -= [0.011, 0.011, 0.0]
    yield from _scene(pkg, ws.Scene(rgb, K, R, t))


FRONT = np.array([0.0, 0.0, -1.0])
# the moved views 2 and 3 (the twin view 1 would put every sample on an integer position and the windows of the
# ring's pixels exactly on the border: the band); they see other texture, so every ncc passes at min_ncc -2
TW = dict(wid=2, min_cos=0.0, min_ncc=-2.0, top_k=1, kd=0, ka=0)
TWL = np.array([[2, 3]], np.int32)


def empty_maps(g, nv=1):
    return np.full((nv, g.H, g.W), np.inf), np.full((nv, g.H, g.W, 3), np.nan)


def test_own_plane_and_single_neighbours(twin):
    g = twin
    z, n = empty_maps(g)
    z[0, 20, 24], n[0, 20, 24] = 1.0, FRONT
    got = gpu_sweep(g, z, n, TWL, 0, **TW)
    compare(g, z, n, TWL, 0, "one seeded pixel", **TW)
    held = np.argwhere(got["best"][0] >= 0)
    assert {tuple(x) for x in held} == {(20, 24), (20, 23), (20, 25), (19, 24), (21, 24)}
    assert got["best"][0, 20, 24] == 0 and got["z"][0, 20, 24] == 1.0
    # each neighbour is the only source of its hypothesis: left h = 1, right 2, up 3, down 4
    assert got["best"][0, 20, 25] == 1 and got["best"][0, 20, 23] == 2
    assert got["best"][0, 21, 24] == 3 and got["best"][0, 19, 24] == 4
    for q in ((20, 25), (20, 23), (21, 24), (19, 24)):
        assert same_bits(got["normal"][0][q], FRONT) and abs(got["z"][0][q] - 1.0) < 1e-15
    # step 3 reaches (+-3, 0), (0, +-3)
    got3 = gpu_sweep(g, z, n, TWL, 0, step=3, **TW)
    assert {tuple(x) for x in np.argwhere(got3["best"][0] >= 0)} == {(20, 24), (20, 21), (20, 27), (17, 24), (23, 24)}


def test_borders_corners_and_the_ring(twin):
    """Sources on every border and corner (their neighbours outside the image do
    not exist), and pixels on the wid ring, which come out empty though they hold
    a plane."""
    g = twin
    z, n = empty_maps(g)
    for q in ((0, 0), (0, 47), (39, 0), (39, 47), (0, 20), (39, 20), (15, 0), (15, 47), (1, 10), (2, 10), (2, 2),
              (37, 20), (38, 20)):
        z[0][q], n[0][q] = 1.0, FRONT
    for step in (1, 2, 64):
        compare(g, z, n, TWL, 0, f"borders step {step}", step=step, **TW)
    got = gpu_sweep(g, z, n, TWL, 0, **TW)
    assert got["best"][0, 1, 10] == -1 and got["best"][0, 2, 10] == 0 and got["best"][0, 2, 2] == 0
    assert got["best"][0, 37, 20] == 0 and got["best"][0, 38, 20] == -1
    ring = np.ones((g.H, g.W), bool)
    ring[2:-2, 2:-2] = False
    assert (got["best"][0][ring] == -1).all()


def test_what_is_empty(twin):
    g = twin
    z, n = empty_maps(g)
    cases = {(10, 10): -1.0, (10, 14): 0.0, (10, 18): np.nan, (10, 22): np.inf, (10, 26): -np.inf}
    for q, v in cases.items():
        z[0][q], n[0][q] = v, FRONT
    z[0, 14, 10], n[0, 14, 10] = 1.0, [0.0, np.nan, -1.0]        # a nan normal component
    z[0, 14, 16], n[0, 14, 16] = 1.0, [0.0, 0.0, 1.0]            # back-facing: exists, never valid
    z[0, 33, 40], n[0, 33, 40] = 1.0, FRONT                      # inside the constant corner
    # n'.d_q = 0 exactly: the ray of (24, 20) is (0, 0, 1), the neighbour (23, 20) holds a normal along x
    z[0, 20, 23], n[0, 20, 23] = 1.0, [-1.0, 0.0, 0.0]
    assert not pr.pixel_planes(g.sc.K, g.sc.Rp, g.sc.t, z[0], n[0], 0, 24, 20, 1, 0, 0, A8, 1.0, 1.0)[2].any()
    got = gpu_sweep(g, z, n, TWL, 0, **TW)
    compare(g, z, n, TWL, 0, "empties", **TW)
    assert (got["best"][0, 8:17, 8:30] == -1).all()
    assert (got["best"][0, 31:36, 38:43] == -1).all()
    assert np.isnan(got["scores"][0, 20, 24, 1]) and got["best"][0, 20, 24] == -1


# ---------------------------------------------------------------------------
# 3. determinism, streams, the host call, interleaving, arguments
# ---------------------------------------------------------------------------
def test_determinism_torch_stream_and_host_call(s26):
    import torch
    z, n = noisy_maps(s26.sc, 2, 3, seed=6)
    lists = ring_lists(24, 2, 3, 4)
    a = gpu_sweep(s26, z, n, lists, 2, wid=3)
    b = gpu_sweep(s26, z, n, lists, 2, wid=3, stream=torch.cuda.Stream(torch.device("cuda:0")))
    c = gpu_sweep(s26, z, n, lists, 2, wid=3, want_scores=False)
    h = s26.ctx.wprop_sweep(z, n, lists, (2, 3), want_scores=True, **dict(KW, wid=3))
    for k in a:
        assert same_bits(a[k], b[k]) and same_bits(a[k], h[k]), k
        assert k == "scores" or same_bits(a[k], c[k]), k
    assert (a["best"] > 0).any()


def test_a_sweep_between_two_score_calls(s26, orc):
    g = s26
    c, _, ref = ws.border_patches(g.sc, 64, 9)
    z, n = noisy_maps(g.sc, 0, 2, seed=7)
    lists = ring_lists(24, 0, 2, 4)
    alone = gpu_sweep(g, z, n, lists, 0, wid=3)
    first = g.ctx.score(c, ref, 0.7, 3)
    mid = g.ctx.wprop_sweep(z, n, lists, (0, 2), want_scores=True, **dict(KW, wid=3))
    again = g.ctx.score(c, ref, 0.7, 3)
    want = orc.Scene(g.sc.rgb, g.sc.K, g.sc.R, g.sc.t_raw).score_batch(c, ref, 0.7, 3)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    for x, w in zip(first[:3], want[:3]):
        assert np.array_equal(x, w)
    for k in alone:
        assert same_bits(alone[k], mid[k]), k


def test_arguments(s26):
    import importlib
    g = s26
    ctx = g.ctx
    z, n = noisy_maps(g.sc, 0, 1, seed=8)
    lists = ring_lists(24, 0, 1, 4)
    ok = ctx.wprop_sweep(z, n, lists, (0, 1))
    assert (ok["best"] >= 0).any()
    for kw, msg in (({"wid": 0}, "wid must be in 1..5"), ({"wid": 6}, "wid must be in 1..5"),
                    ({"min_cos": 1.0}, r"min_cos must be in \[0, 1\)"), ({"min_cos": -0.1}, "min_cos"),
                    ({"min_ncc": float("nan")}, "min_ncc is nan"), ({"top_k": 0}, "top_k must be in 1..tv"),
                    ({"top_k": 5}, "top_k must be in 1..tv"), ({"step": 0}, "step must be in 1..64"),
                    ({"step": 65}, "step must be in 1..64"), ({"kd": 4}, "kd must be in 0..3"),
                    ({"kd": -1}, "kd must be in 0..3"), ({"ka": 3}, "ka must be in 0..2"),
                    ({"ka": -1}, "ka must be in 0..2"), ({"astep": -0.1}, "astep"),
                    ({"depth_px": 0.0}, "depth_px must be finite and > 0"),
                    ({"depth_px": float("inf")}, "depth_px must be finite and > 0"),
                    ({"step_scale": 0.0}, "step_scale must be > 0"),
                    ({"ka": 2, "astep": 0.7, "step_scale": 1.0}, r"ka \* astep \* step_scale")):
        with pytest.raises(RuntimeError, match=msg):
            ctx.wprop_sweep(z, n, lists, (0, 1), **kw)
    ctx.wprop_sweep(z, n, lists, (0, 1), ka=2, astep=0.6, step_scale=1.0, wid=1)     # 1.2: allowed
    for bad, msg in (([1, 24, -1, -1], "list view out of range"), ([-2, -1, -1, -1], "list view out of range"),
                     ([1, 0, -1, -1], "equal to the row's own view"), ([3, 3, -1, -1], "list view repeated"),
                     ([-1, 3, -1, -1], "list view after a -1")):
        with pytest.raises(RuntimeError, match=msg):
            ctx.wprop_sweep(z, n, np.array([bad], np.int32), (0, 1))
    with pytest.raises(RuntimeError, match="tv in 1..32"):
        ctx.wprop_sweep(z, n, np.full((1, 33), -1, np.int32), (0, 1))
    # the C entry points themselves: the view range, NULL pointers, aliased arrays, nothing to do
    lib = importlib.import_module(PKG_NAME + "._lib").load()
    ip = ctypes.POINTER(ctypes.c_int32)
    L = np.ascontiguousarray(lists).ctypes.data_as(ip)
    px = g.H * g.W
    buf = [np.zeros(px * 3) for _ in range(5)]
    ib = np.zeros(px, np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    P = [b.ctypes.data_as(dp) for b in buf]
    I = ib.ctypes.data_as(ip)
    err = lambda: lib.mvs_last_error(ctx._h).decode()

    def host(v0=0, nv=1, zi=P[0], ni=P[1], li=L, zo=P[2], no=P[3], sc=P[4], be=I, tv=4):
        return lib.mvs_wprop_sweep(ctx._h, v0, nv, zi, ni, li, tv, 2, 0.3, 0.7, 2, 1, 1, 1, 0.1, 1.0, 1.0, zo, no, sc, be,
                                   None)
    assert host() == 0
    assert host(v0=24) == -1 and "view range" in err()
    assert host(v0=-1) == -1 and "view range" in err()
    assert host(nv=25) == -1 and "view range" in err()
    assert host(v0=24, nv=0) == 0 and host(nv=0, li=None) == 0            # nv H W = 0: nothing to do
    assert host(tv=0) == -1 and "tv must be in 1..32" in err()
    assert host(li=None) == -1 and "null pointer" in err()
    for name in ("zi", "ni", "zo", "no", "sc", "be"):
        assert host(**{name: None}) == -1 and "null pointer" in err(), name
    assert host(zo=P[0]) == -1 and "overlaps an input" in err()
    assert host(no=P[1]) == -1 and "overlaps an input" in err()
    assert host(sc=P[0]) == -1 and "overlaps an input" in err()
    assert host(sc=P[2]) == -1 and "outputs overlap" in err()
    inside = ctypes.cast(ctypes.c_void_p(ctypes.addressof(P[2].contents) + 8), dp)
    assert host(sc=inside) == -1 and "outputs overlap" in err()
    dev = lambda **k: lib.mvs_wprop_sweep_device(ctx._h, k.get("v0", 0), k.get("nv", 1), k.get("zi", 256), 512, L, 4, 2,
                                                 0.3, 0.7, 2, 1, 1, 1, 0.1, 1.0, 1.0, k.get("zo", 1 << 20), 2 << 20,
                                                 3 << 20, 4 << 20, None, None)
    assert dev(zi=None) == -1 and "null pointer" in err()
    assert dev(zo=256) == -1 and "overlaps an input" in err()
    assert dev(v0=30) == -1 and "view range" in err()
    assert dev(nv=0) == 0


# ---------------------------------------------------------------------------
# 4. chains
# ---------------------------------------------------------------------------
def test_three_sweeps_each_against_the_restatement_of_the_one_before(s45):
    """45 x 61, 6 views, steps 1, 3, 1: GPU sweep k is checked against the
    restatement applied to the GPU's own sweep k - 1 maps (the chains are not
    bit-equal once an equal-score choice differs)."""
    g = s45
    z, n = noisy_maps(g.sc, 4, 6, n=120, seed=10)
    lists = ring_lists(24, 4, 6, 4)
    held = [int(pr.holds(z, n).sum())]
    for k, step in enumerate((1, 3, 1)):
        kw = dict(wid=3, step=step, step_scale=1.0 if k < 2 else 0.5)
        got = gpu_sweep(g, z, n, lists, 4, **kw)
        compare(g, z, n, lists, 4, f"chain sweep {k}", **kw)
        z, n = got["z"], got["normal"]
        held.append(int((got["best"] >= 0).sum()))
    print("pixels holding a plane:", held)
    assert held[3] > held[1]


def test_densify_depth_on_the_sphere(big, pkg):
    """MvsContext.densify_depth on the 96 x 128 sphere: the restatement's radius-1
    splat of the 442-patch chain, the six views 0..5 with lists inside the range,
    wid 3, the default schedule -- test_wprop_host.py's configuration and its
    recorded bounds (factor 2)."""
    import test_wprop_host as th
    g = big
    q = th.quality_inputs(pkg)
    res = g.ctx.densify_depth({"z": q["z"], "normal": q["normal"]}, views=(0, th.QV), lists=q["lists"], wid=3)
    Ks, Rp, t = q["cam"]
    before = th.depth_quality(Ks, Rp, t, q["z"], th.RAD)
    after = th.depth_quality(Ks, Rp, t, res["z"], th.RAD)
    fused = np.zeros(res["z"].shape, bool)
    fused[res["pix"][:, 0], res["pix"][:, 2], res["pix"][:, 1]] = True
    fz = th.depth_quality(Ks, Rp, t, res["z"], th.RAD, fused)
    print(f"before {before}, after {after}, fused {len(res['pix'])} px {fz}, history {res['history'].tolist()}")
    th.assert_quality(before, after, fz)
    # history and the maps agree
    assert res["history"].shape == (12, 2)
    assert res["history"][-1, 0] == int((res["best"] >= 0).sum()) == int(np.isfinite(res["z"]).sum())
    assert res["history"][-1, 1] == int((res["best"] > 0).sum())
    assert np.array_equal(np.isfinite(res["z"]), ~np.isnan(res["normal"]).any(-1))
    sel = np.isfinite(res["z"]) & (res["cons"] >= 2) & (res["viol"] <= 0)
    assert np.array_equal(sel, fused) and len(res["points"]) == len(res["pix"]) == len(res["normals"])
    cons, viol = dr.consist_fast(Ks, Rp, t, 128, 96, res["z"], 0, th.QV, 0.01)
    assert np.array_equal(cons, res["cons"]) and np.array_equal(viol, res["viol"])
    r = np.linalg.norm(res["points"], axis=1)
    assert np.isfinite(r).all() and abs(float(np.median(r)) - th.RAD) < 1e-3
