"""The visibility-consistency filter on the GPU (k_wfilt_fill, k_wfilt_front,
k_wfilt_conflict, k_wfilt_decide and MvsContext.filter_warped) against the
float64 restatement (tests/filter_reference.py).

Every comparison is exact, with no row left out and no tolerance: front, the
bits of zfront, vis, conf and keep.  The arithmetic is the projection that
tests/test_expand_gpu.py already finds bit-equal, unfused dot products and
integer sums.

Sizes: the front and conflict kernels put 4 patches in a workgroup (n = 1, 3,
4, 5 and 257: a partial last workgroup); the 80-view ring takes the two-word
path of both (lane = view in groups of 64).
"""
import ctypes

import numpy as np
import pytest

import expand_reference as er
import filter_reference as fr
import warped_reference as wr
from test_expand_gpu import random_masks
from test_warped_gpu import toward_camera

pytestmark = pytest.mark.gpu

RAD = 0.02


class Scene:
    def __init__(self, pkg, rgb, K, R, t):
        import torch
        assert torch.cuda.is_available(), "GPU test without a GPU"
        self.rgb, self.t_raw = rgb, t
        self.ctx = pkg.MvsContext(rgb, K, R, t, device=0)
        self.K, self.R, self.t = K, R, np.asarray(t, np.float64).reshape(-1, 3)
        self.Rp = self.ctx.rproj()
        self.V, self.H, self.W = self.ctx.V, self.ctx.H, self.ctx.W
        self.O = np.array([er.centre_of([float(x) for x in self.Rp[v].reshape(9)], [float(x) for x in self.t[v]])
                           for v in range(self.V)])

    def cam(self):
        return self.K, self.Rp, self.t, self.W, self.H

    def at_pixel(self, v, x, y, depth_scale=1.0):
        """A point on the ray of pixel (x, y) of view v, at depth_scale times the depth of the origin."""
        d = self.Rp[v].T @ np.array([(x - self.K[v][0, 2]) / self.K[v][0, 0], (y - self.K[v][1, 2]) / self.K[v][1, 1], 1.0])
        z0 = float(self.t[v][2])        # the depth of the world origin in view v
        return self.O[v] + d * (z0 * depth_scale)


@pytest.fixture(scope="module")
def sphere(pkg):
    rgb, K, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]
    s = Scene(pkg, rgb, K, R, t)
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def ring(pkg):
    rgb, K, R, t = pkg.synthetic.ring_scene(V=80, H=48, W=64)
    s = Scene(pkg, rgb, K, R, t)
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def mixed(sphere):
    """The host quality test's mixed set (chain + outliers), generated on the
    CPU once, and the restatement's two-pass chain on it."""
    s = sphere
    m = fr.mixed_set(wr.gray_stack(s.rgb), s.K, s.R, s.t, s.Rp, RAD)
    m["chain"] = fr.filter_chain(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], m["avg"], 2, 2.0, 3, passes=2)
    m["front"] = fr.front_grid(*s.cam(), m["c"], m["ref"], m["mask"], 2)
    return m


def _dev(x, dtype=None):
    import torch
    a = np.ascontiguousarray(x)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a).to("cuda:0")
    return t if dtype is None else t.to(dtype)


def gpu_front(s, c, ref, mask, cell):
    """mvs_wfilt_front_device on grids pre-filled with a canary pattern -> front, zfront."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tc = _dev(np.asarray(c, np.float64).reshape(n, 3))
        tr = _dev(np.asarray(ref, np.int32))
        tm = _dev(np.asarray(mask, np.uint64).reshape(n, s.ctx.words))
        front = torch.full((s.V, ncj, nci), -77, dtype=torch.int32, device=dev)
        zfront = torch.full((s.V, ncj, nci), -77.0, dtype=torch.float64, device=dev)
        s.ctx.wfilt_front_device(tc, tr, tm, cell, front, zfront, stream=st.cuda_stream)
        out = front.cpu().numpy(), zfront.cpu().numpy()
    st.synchronize()
    return out


def gpu_test(s, c, nrm, ref, mask, avg, cell, adj_px, min_views, front):
    """mvs_wfilt_test_device on outputs pre-filled with a canary pattern -> vis, conf, keep."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tc = _dev(np.asarray(c, np.float64).reshape(n, 3))
        tn = _dev(np.asarray(nrm, np.float64).reshape(n, 3))
        tr = _dev(np.asarray(ref, np.int32))
        tm = _dev(np.asarray(mask, np.uint64).reshape(n, s.ctx.words))
        ta = _dev(np.asarray(avg, np.float64))
        tf = _dev(np.asarray(front, np.int32))
        vis = torch.full((n, s.ctx.words), -77, dtype=torch.int64, device=dev)
        conf = torch.full((n,), -77, dtype=torch.int64, device=dev)
        keep = torch.full((n,), 77, dtype=torch.uint8, device=dev)
        s.ctx.wfilt_test_device(tc, tn, tr, tm, ta, cell, adj_px, min_views, tf, vis, conf, keep, stream=st.cuda_stream)
        out = vis.cpu().numpy().view(np.uint64), conf.cpu().numpy(), keep.cpu().numpy()
    st.synchronize()
    return out


def compare_front(s, c, ref, mask, cell, label=""):
    want = fr.front_grid(*s.cam(), c, ref, mask, cell)
    front, zfront = gpu_front(s, c, ref, mask, cell)
    assert front.dtype == np.int32 and np.array_equal(front, want[0])
    assert zfront.tobytes() == want[1].tobytes()
    print(f"{label}: n {len(ref)}, {int((want[0] >= 0).sum())} of {want[0].size} cells taken, "
          f"{len(np.unique(want[0][want[0] >= 0]))} patches in front somewhere")
    return want


def compare_test(s, c, nrm, ref, mask, avg, cell, adj_px, min_views, front, label=""):
    want = fr.vistest(*s.cam(), c, nrm, ref, mask, avg, cell, adj_px, min_views, front)
    vis, conf, keep = gpu_test(s, c, nrm, ref, mask, avg, cell, adj_px, min_views, front)
    assert np.array_equal(vis, want[0]), label
    assert conf.dtype == np.int64 and np.array_equal(conf, want[1]), label
    assert keep.dtype == np.uint8 and np.array_equal(keep, want[2]), label
    return want


def sphere_set(s, n, seed):
    rng = np.random.default_rng(seed)
    c, nrm, ref, _ = wr.sphere_patches(s.K, s.R, s.t, n, RAD, rng, (0.0, 0.002, -0.002))
    return rng, c, nrm, ref, random_masks(rng, n, s.V)


# ---------------------------------------------------------------------------
# 1. the front grid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 2, 3, 4])
def test_front_sphere(sphere, cell):
    s = sphere
    _, c, _, ref, mask = sphere_set(s, 200, 10 + cell)
    want = compare_front(s, c, ref, mask, cell, f"sphere cell {cell}")
    assert (want[0] >= 0).sum() > 200


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_front_sizes(sphere, n):
    s = sphere
    _, c, _, ref, mask = sphere_set(s, n, 100 + n)
    want = compare_front(s, c, ref, mask, 2, f"sizes n {n}")
    if n == 0:
        assert np.all(want[0] == -1) and np.all(np.isinf(want[1]))
    else:
        assert (want[0] >= 0).any()


@pytest.mark.parametrize("cell", [1, 2, 3])
def test_front_more_than_64_views(ring, cell):
    s = ring
    rng = np.random.default_rng(4)
    n = 61
    c = rng.uniform(-0.005, 0.005, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, 80, n).astype(np.int32)
    mask = random_masks(rng, n, 80, 0.3)
    assert mask.shape[1] == 2
    mask[::3, 1] |= np.uint64(0xFFFF) << np.uint64(16)               # bits 80..95 name no view
    want = compare_front(s, c, ref, mask, cell, f"ring V=80 cell {cell}")
    assert (want[0][64:] >= 0).any() and (want[0][:64] >= 0).any()


def special_rows(s, cell=3):
    """Rows that the placement must leave out, among ordinary ones."""
    rng, c, nrm, ref, mask = sphere_set(s, 24, 5)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    ref[0] = -1
    ref[1] = s.V
    c[2, 1] = np.nan
    c[3, 0] = np.inf
    c[4] = s.O[3] * 1.2                                  # behind camera 3 (the cameras look at the origin)
    ref[4] = 3
    c[5] = np.array([0.4, 0.3, 0.2])                     # outside every image
    c[6] = s.at_pixel(7, nci * cell + 0.5, 40.2, 0.5)    # in the pixel strip past the last whole cell
    ref[6], mask[6] = 7, 0
    c[7] = s.at_pixel(7, nci * cell - 0.5, 40.2, 0.5)    # its neighbour in the last whole cell, nearer than the sphere
    ref[7], mask[7] = 7, 0
    return rng, c, nrm, ref, mask


def test_special_rows(sphere):
    s = sphere
    cell = 3
    rng, c, nrm, ref, mask = special_rows(s, cell)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    assert nci * cell < s.W
    x6 = wr.project_ref(s.K[7], s.Rp[7], s.t[7], c[6])
    assert nci * cell <= x6[0] < s.W and x6[2] > 0 and er.cell_of(*s.cam()[:3], 7, c[6], s.W, s.H, cell) is None
    assert er.cell_of(*s.cam()[:3], 7, c[7], s.W, s.H, cell) == (nci - 1, 13)
    want = compare_front(s, c, ref, mask, cell, "special rows")
    for k in (0, 1, 2, 3, 5, 6):
        assert not (want[0] == k).any(), k
    assert not (want[0][3] == 4).any() and (want[0] == 7).any()
    avg = rng.uniform(0.7, 1.0, len(ref))
    got = compare_test(s, c, nrm, ref, mask, avg, cell, 2.0, 1, want[0], "special rows")
    for k in (0, 1, 2, 3, 5, 6):
        assert not got[0][k].any() and got[2][k] == 0, k
    assert got[0][7, 0] == np.uint64(1 << 7) and got[2].sum() > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_front_contention_and_ties(sphere, reverse):
    """3,000 patches on one pixel ray of view 5: every atomic of both passes
    lands on one cell.  100 rows are bit-identical copies of the nearest
    centre: the lowest index wins."""
    s = sphere
    rng = np.random.default_rng(12)
    n, v = 3000, 5
    scale = rng.uniform(0.9, 1.1, n)
    c = np.array([s.at_pixel(v, 60.9, 40.9, k) for k in scale])
    near = int(np.argmin(scale))
    copies = rng.choice(np.setdiff1d(np.arange(n), [near]), 100, replace=False)
    c[copies] = c[near]
    if reverse:
        c = c[::-1].copy()
    ref = np.full(n, v, np.int32)
    mask = np.zeros((n, 1), np.uint64)
    want = compare_front(s, c, ref, mask, 2, f"one cell, reversed {reverse}")
    assert (want[0] >= 0).sum() == 1
    winner = int(want[0].max())
    same = np.flatnonzero((c == c[winner]).all(1))
    assert len(same) == 101 and winner == same.min()


# ---------------------------------------------------------------------------
# 2. the test call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("adj_px", [0.0, 1.0, 2.0, 4.0])
def test_test_call_on_the_mixed_set(sphere, mixed, adj_px):
    s, m = sphere, mixed
    front, zfront = gpu_front(s, m["c"], m["ref"], m["mask"], 2)
    assert np.array_equal(front, m["front"][0]) and zfront.tobytes() == m["front"][1].tobytes()
    avg = m["avg"].copy()
    avg[3], avg[40], avg[77], avg[200] = np.nan, np.inf, -0.3, 3.0
    kept = []
    for min_views in (0, 1, 3, s.V + 1):
        want = compare_test(s, m["c"], m["nrm"], m["ref"], m["mask"], avg, 2, adj_px, min_views, front,
                            f"adj_px {adj_px} min_views {min_views}")
        kept.append(int(want[2].sum()))
    conflicts = sum(len(f) for f in want[3])
    print(f"adj_px {adj_px}: {len(avg)} patches, {conflicts} conflicts, kept at min_views 0, 1, 3, V + 1: {kept}")
    assert kept[3] == 0 and kept[0] >= kept[1] >= kept[2] > 0
    assert conflicts > 0


def test_test_call_on_a_crafted_front_grid(sphere, mixed):
    """A front grid that was not built from the set: -1 and valid indices at
    random, so that patches meet fronts far from them, behind them and dead."""
    s, m = sphere, mixed
    n = len(m["ref"])
    rng = np.random.default_rng(21)
    front = np.where(rng.random(m["front"][0].shape) < 0.3, -1, rng.integers(0, n, m["front"][0].shape)).astype(np.int32)
    ref = m["ref"].copy()
    ref[::7] = -1                                         # dead rows, named by the grid all the same
    want = compare_test(s, m["c"], m["nrm"], ref, m["mask"], m["avg"], 2, 2.0, 1, front, "crafted grid")
    assert sum(len(f) for f in want[3]) > n and want[2].sum() > 0
    assert not want[1][::7].any() and not want[2][::7].any()
    # the host-pointer call agrees on a valid grid
    vis, conf, keep = s.ctx.wfilt_test(m["c"], m["nrm"], ref, m["mask"], m["avg"], 2, 2.0, 1, front)
    assert np.array_equal(vis, want[0]) and np.array_equal(conf, want[1]) and np.array_equal(keep, want[2])
    hf, hz = s.ctx.wfilt_front(m["c"], m["ref"], m["mask"], 2)
    assert np.array_equal(hf, m["front"][0]) and hz.tobytes() == m["front"][1].tobytes()
    # entries outside -1..n-1 read as -1 on the device and are refused by the host-pointer call
    bad = front.copy()
    taken = np.argwhere(m["front"][0] >= 0)
    for k, value in enumerate((n, n + 5, -2, np.iinfo(np.int32).min, np.iinfo(np.int32).max)):
        v, j, i = taken[k * 50]
        bad[v, j, i] = value
    as_empty = np.where((bad < 0) | (bad >= n), -1, bad).astype(np.int32)
    vis, conf, keep = gpu_test(s, m["c"], m["nrm"], ref, m["mask"], m["avg"], 2, 2.0, 1, bad)
    want = fr.vistest(*s.cam(), m["c"], m["nrm"], ref, m["mask"], m["avg"], 2, 2.0, 1, as_empty)
    assert np.array_equal(vis, want[0]) and np.array_equal(conf, want[1]) and np.array_equal(keep, want[2])
    with pytest.raises(RuntimeError, match="front entry outside"):
        s.ctx.wfilt_test(m["c"], m["nrm"], ref, m["mask"], m["avg"], 2, 2.0, 1, bad)


def test_one_patch_hides_two_thousand(sphere):
    """One near patch and 2,000 patches behind it on the same pixel ray, none
    adjacent: every atomic add of the conflict kernel lands on conf[0]."""
    s = sphere
    rng = np.random.default_rng(13)
    n, v = 2001, 5
    scale = np.concatenate([[0.8], rng.uniform(1.0, 1.2, n - 1)])
    c = np.array([s.at_pixel(v, 60.9, 40.9, k) for k in scale])
    nrm = toward_camera(s.Rp, s.t, c, np.full(n, v))
    ref = np.full(n, v, np.int32)
    mask = np.zeros((n, 1), np.uint64)
    avg = rng.uniform(0.7, 1.0, n)
    front = compare_front(s, c, ref, mask, 2, "one near patch")[0]
    assert (front >= 0).sum() == 1 and front.max() == 0
    want = compare_test(s, c, nrm, ref, mask, avg, 2, 2.0, 1, front, "one near patch")
    assert all(f == {0} for f in want[3][1:]) and want[3][0] == set()
    assert int(want[1][0]) == sum(fr.weight(a) for a in avg[1:])
    assert not want[2].any()       # the near patch's own support is far below the sum; the rest see nothing


def test_test_call_more_than_64_views(ring):
    """The two-word path: placements, ballots and the distinct front patches
    across the groups of 64 lanes; several patches share a front patch in views
    of both words."""
    s = ring
    rng = np.random.default_rng(6)
    n = 120
    c = rng.uniform(-0.02, 0.02, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, 80, n).astype(np.int32)
    nrm = toward_camera(s.Rp, s.t, c, ref)
    mask = random_masks(rng, n, 80, 0.5)
    mask[::3, 1] |= np.uint64(0xFFFF) << np.uint64(16)
    avg = rng.uniform(0.5, 1.0, n)
    for cell in (2, 4):
        front = compare_front(s, c, ref, mask, cell, f"ring test cell {cell}")[0]
        want = compare_test(s, c, nrm, ref, mask, avg, cell, 1.0, 3, front, f"ring cell {cell}")
        per_patch = [len(f) for f in want[3]]
        # the placed views of a patch whose front patch is in its conflict set: more of them
        # than the set has members means that a front patch was named in several views
        views = [sum(1 for v, (i, j), _ in row if int(front[v, j, i]) in want[3][p])
                 for p, row in enumerate(fr.placements(*s.cam(), c, ref, mask, cell))]
        repeats = sum(v - k for v, k in zip(views, per_patch))
        print(f"ring cell {cell}: conflicts per patch max {max(per_patch)}, total {sum(per_patch)}, "
              f"{repeats} repeated namings, {int(want[2].sum())} kept")
        assert sum(per_patch) > 0 and repeats > 0
        assert any(v >= 64 and int(front[v, j, i]) in want[3][p] for p, row in
                   enumerate(fr.placements(*s.cam(), c, ref, mask, cell)) for v, (i, j), _ in row)


# ---------------------------------------------------------------------------
# 3. the chain
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_chain(sphere, mixed):
    s, m = sphere, mixed
    patches = {k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")}
    return (s.ctx.filter_warped(patches, cell_size=2, adj_px=2.0, min_views=3, passes=2),
            s.ctx.filter_warped(patches, cell_size=2, adj_px=2.0, min_views=3, passes=2))


def test_chain_is_the_restatement(sphere, mixed, gpu_chain, pkg):
    s, m = sphere, mixed
    a, b = gpu_chain
    want = m["chain"]
    assert a["removed"] == want["removed"] and len(a["removed"]) == 2
    for k in ("keep", "vis", "conf", "front"):
        assert np.array_equal(a[k], want[k]), k
    assert a["zfront"].tobytes() == want["zfront"].tobytes()
    idx = np.flatnonzero(want["keep"])
    assert np.array_equal(a["index"], idx)
    for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind"):
        assert np.array_equal(a[k], m[k][idx]), k
    # two runs are bit-identical
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k
    # the occupancy of the survivors
    jobs = np.column_stack([np.full(len(idx), -1), m["ref"][idx], m["cell"][idx]]).astype(np.int32)
    nci, ncj = er.grid_shape(s.W, s.H, 2)
    occ = er.mark(*s.cam(), jobs, np.ones(len(idx), np.uint8), m["c"][idx], m["ref"][idx], m["mask"][idx], 2,
                  np.zeros((s.V, ncj, nci), np.uint8))
    assert np.array_equal(a["occ"], occ) and occ.sum() > len(idx)
    # the thin wrapper, and early exit: a third pass removes nothing and is the last one run
    more = pkg.filter_patches_warped(s.ctx, {k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell")}, passes=5)
    ref5 = fr.filter_chain(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], m["avg"], 2, 2.0, 3, passes=5)
    assert more["removed"] == ref5["removed"] and more["removed"][-1] == 0 and len(more["removed"]) < 5
    assert np.array_equal(more["keep"], ref5["keep"])
    none = s.ctx.filter_warped({"c": np.empty((0, 3)), "nrm": np.empty((0, 3)), "ref": np.empty(0, np.int32),
                                "mask": np.empty((0, 1), np.uint64), "avg": np.empty(0), "cell": np.empty((0, 2), np.int32)})
    assert none["c"].shape == (0, 3) and none["removed"] == [0] and np.all(none["front"] == -1) and not none["occ"].any()


def test_chain_quality(mixed, gpu_chain):
    """The bounds of tests/test_wfilt_host.py on the GPU chain's own keep vector."""
    m = mixed
    keep, kind = gpu_chain[0]["keep"], m["kind"]
    counts = [(int(keep[kind == k].sum()), int((kind == k).sum())) for k in (0, 1, 2)]
    print(f"GPU chain: chain patches {counts[0][0]}/{counts[0][1]} kept, outliers outside {counts[1][0]}/{counts[1][1]}, "
          f"inside {counts[2][0]}/{counts[2][1]}, removed per pass {gpu_chain[0]['removed']}")
    assert counts[0][0] >= 0.98 * counts[0][1]
    assert counts[1][0] + counts[2][0] <= 0.25 * (counts[1][1] + counts[2][1])


def test_no_shared_state(sphere, mixed, gpu_chain, orc):
    """score, a filter chain on the side stream, score on one context: both
    score results are the oracle's, and the chain gives the same bytes as the
    chains before them."""
    s, m = sphere, mixed
    c, ref = m["c"], m["ref"]
    first = s.ctx.score(c, ref, 0.7, 5)
    again_chain = s.ctx.filter_warped({k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")})
    again = s.ctx.score(c, ref, 0.7, 5)
    want = orc.Scene(s.rgb, s.K, s.R, s.t_raw).score_batch(c, ref, 0.7, 5)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    for x, w in zip(first[:3], want[:3]):
        assert np.array_equal(x, w)
    assert np.allclose(first[3], want[3], rtol=0, atol=1e-12)
    for k, v in gpu_chain[0].items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == again_chain[k].tobytes(), k
    assert again_chain["removed"] == gpu_chain[0]["removed"]


# ---------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------
def test_arguments(pkg, sphere):
    s = sphere
    lib = pkg._lib.load()
    h = s.ctx.handle
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails its checks

    def front(n=1, cell=2, ptr=one, grid=one):
        return lib.mvs_wfilt_front_device(h, n, ptr, one, one, cell, grid, one, None)

    def test(n=1, cell=2, adj_px=2.0, min_views=3, ptr=one):
        return lib.mvs_wfilt_test_device(h, n, ptr, one, one, one, one, cell, adj_px, min_views, one, one, one, one, None)

    for call, msg in ((lambda: front(cell=0), "cell_size must be in 1..16"),
                      (lambda: front(cell=17), "cell_size must be in 1..16"),
                      (lambda: front(n=-1), "n < 0"),
                      (lambda: front(n=1 << 31), "below 2^31"),
                      (lambda: front(ptr=None), "null pointer"),
                      (lambda: front(n=0, grid=None), "null pointer"),
                      (lambda: test(cell=0), "cell_size must be in 1..16"),
                      (lambda: test(cell=17), "cell_size must be in 1..16"),
                      (lambda: test(n=-1), "n < 0"),
                      (lambda: test(adj_px=-1.0), "adj_px must be finite and >= 0"),
                      (lambda: test(adj_px=float("nan")), "adj_px must be finite and >= 0"),
                      (lambda: test(adj_px=float("inf")), "adj_px must be finite and >= 0"),
                      (lambda: test(min_views=-1), "min_views < 0"),
                      (lambda: test(ptr=None), "null pointer")):
        assert call() == -1                      # MVS_E_ARG
        assert msg in pkg._lib.last_error(h), (msg, pkg._lib.last_error(h))
    assert test(n=0, ptr=None) == 0
    # n = 0 returns OK with both grids empty (test_front_sizes[0] holds them against the restatement)
    e3, e1 = np.empty((0, 3)), np.empty(0, np.int32)
    f, z = s.ctx.wfilt_front(e3, e1, np.empty((0, 1), np.uint64), 4)
    assert f.shape == (s.V, s.H // 4, s.W // 4) and np.all(f == -1) and np.all(np.isposinf(z))
    with pytest.raises(RuntimeError, match="cell_size"):
        s.ctx.wfilt_front(e3, e1, np.empty((0, 1), np.uint64), 0)
    with pytest.raises(RuntimeError, match="adj_px"):
        s.ctx.filter_warped({"c": e3, "nrm": e3, "ref": e1, "mask": np.empty((0, 1), np.uint64), "avg": np.empty(0),
                             "cell": np.empty((0, 2), np.int32)}, adj_px=-1.0)
    with pytest.raises(RuntimeError, match="no 'avg'"):
        s.ctx.filter_warped({"c": e3, "nrm": e3, "ref": e1, "mask": np.empty((0, 1), np.uint64),
                             "cell": np.empty((0, 2), np.int32)})
