"""The neighbour-support test on the GPU (k_wfilt_support through
mvs_wfilt_support_device and mvs_wfilt_support) against the float64 restatement
(tests/support_reference.py).

Every comparison is exact, with no row left out and no tolerance: nb, adj and
keep.  The arithmetic is the placement and the adjacency test that
tests/test_wfilt_gpu.py already finds bit-equal, two integer sums and one
binary64 product.

Sizes: four patches in a workgroup (n = 1, 3, 4, 5 and 257: a partial last
workgroup); the 80-view ring takes the runtime loop over the groups of 64 views
twice; cell sizes 1-4 (at 3 the image has a pixel strip past the last whole
cell).
"""
import ctypes

import numpy as np
import pytest

import expand_reference as er
import filter_reference as fr
import support_reference as sr
from test_expand_gpu import random_masks
from test_warped_gpu import toward_camera
from test_wfilt_gpu import RAD, Scene, _dev, special_rows, sphere_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sphere(pkg):
    m = sr.sphere_mixed(pkg, RAD)
    s = Scene(pkg, m["rgb"], m["K"], m["R"], m["t_raw"])
    assert np.array_equal(s.Rp, m["Rp"])
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def ring(pkg):
    rgb, K, R, t = pkg.synthetic.ring_scene(V=80, H=48, W=64)
    s = Scene(pkg, rgb, K, R, t)
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def mixed(pkg, sphere):
    """The quality experiment's mixed set and its front grid (restatement)."""
    m = dict(sr.sphere_mixed(pkg, RAD)["set"])
    m["front"] = fr.front_grid(*sphere.cam(), m["c"], m["ref"], m["mask"], 2)[0]
    return m


def gpu_support(s, c, nrm, ref, mask, cell, adj_px, min_support, min_neigh, front, stream=None):
    """mvs_wfilt_support_device on outputs pre-filled with a canary pattern -> nb, adj, keep."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    st = stream if stream is not None else torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tc = _dev(np.asarray(c, np.float64).reshape(n, 3))
        tn = _dev(np.asarray(nrm, np.float64).reshape(n, 3))
        tr = _dev(np.asarray(ref, np.int32))
        tm = _dev(np.asarray(mask, np.uint64).reshape(n, s.ctx.words))
        tf = _dev(np.asarray(front, np.int32))
        nb = torch.full((n,), -77, dtype=torch.int32, device=dev)
        adj = torch.full((n,), -77, dtype=torch.int32, device=dev)
        keep = torch.full((n,), 77, dtype=torch.uint8, device=dev)
        s.ctx.wfilt_support_device(tc, tn, tr, tm, cell, adj_px, min_support, min_neigh, tf, nb, adj, keep,
                                   stream=st.cuda_stream)
        out = nb.cpu().numpy(), adj.cpu().numpy(), keep.cpu().numpy()
    st.synchronize()
    return out


def compare(s, c, nrm, ref, mask, cell, adj_px, min_support, min_neigh, front, label=""):
    want = sr.support(*s.cam(), c, nrm, ref, mask, cell, adj_px, min_support, min_neigh, front)
    got = gpu_support(s, c, nrm, ref, mask, cell, adj_px, min_support, min_neigh, front)
    for g, w, name in zip(got, want, ("nb", "adj", "keep")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (label, name)
    return want


# ---------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("adj_px", [0.0, 1.0, 2.0, 4.0])
def test_mixed_set(sphere, mixed, adj_px):
    """nb and adj do not depend on the decision's scalars: the restatement runs
    once per adj_px and its rule (support_reference.decide) gives keep for the
    other settings."""
    s, m = sphere, mixed
    nb, adj, _ = compare(s, m["c"], m["nrm"], m["ref"], m["mask"], 2, adj_px, 0.25, 1, m["front"], f"adj_px {adj_px}")
    kept = {}
    for ms in (0.0, 0.25, 0.5, 1.0):
        for mn in (0, 1, 4):
            g = gpu_support(s, m["c"], m["nrm"], m["ref"], m["mask"], 2, adj_px, ms, mn, m["front"])
            keep = np.array([sr.decide(N, A, ms, mn) for N, A in zip(nb, adj)], np.uint8)
            assert np.array_equal(g[0], nb) and np.array_equal(g[1], adj) and np.array_equal(g[2], keep), (ms, mn)
            kept[(ms, mn)] = int(keep.sum())
    print(f"adj_px {adj_px}: {len(nb)} patches, N sum {int(nb.sum())} max {int(nb.max())}, A sum {int(adj.sum())}, "
          f"kept {kept}")
    assert nb.sum() > 8 * len(nb) and nb.max() > 8          # several views per patch
    assert kept[(0.0, 0)] == len(nb) and kept[(1.0, 4)] <= kept[(0.25, 1)] <= kept[(0.0, 1)]
    assert (adj.sum() == 0) == (adj_px == 0.0)


@pytest.mark.parametrize("cell", [1, 2, 3, 4])
def test_cell_sizes(sphere, cell):
    s = sphere
    _, c, nrm, ref, mask = sphere_set(s, 200, 30 + cell)
    front = fr.front_grid(*s.cam(), c, ref, mask, cell)[0]
    nb, adj, keep = compare(s, c, nrm, ref, mask, cell, 2.0, 0.25, 1, front, f"cell {cell}")
    print(f"cell {cell}: N sum {int(nb.sum())}, A sum {int(adj.sum())}, kept {int(keep.sum())}/200")
    if cell > 1:
        assert nb.sum() > 0
    if cell > 2:
        assert 0 < adj.sum() < nb.sum() and 0 < keep.sum() < 200


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_sizes(sphere, n):
    s = sphere
    _, c, nrm, ref, mask = sphere_set(s, n, 100 + n)
    front = fr.front_grid(*s.cam(), c, ref, mask, 4)[0]
    nb, adj, keep = compare(s, c, nrm, ref, mask, 4, 2.0, 0.25, 0, front, f"n {n}")
    assert len(nb) == n
    if n == 257:
        assert nb.sum() > 0 and nb[256] == sr.support(*s.cam(), c, nrm, ref, mask, 4, 2.0, 0.25, 0, front)[0][256]


def test_special_rows(sphere):
    """Dead rows, nan and inf centres, a patch behind its camera, one outside
    every image, one in the pixel strip past the last whole cell and a nan
    normal, among ordinary rows, at cell size 3."""
    s = sphere
    cell = 3
    rng, c, nrm, ref, mask = special_rows(s, cell)
    nrm[9] = np.nan
    front = fr.front_grid(*s.cam(), c, ref, mask, cell)[0]
    nb, adj, keep = compare(s, c, nrm, ref, mask, cell, 4.0, 0.0, 0, front, "special rows")
    for k in (0, 1):
        assert nb[k] == 0 and adj[k] == 0 and keep[k] == 0, k       # dead
    for k in (2, 3, 5, 6):
        assert nb[k] == 0 and keep[k] == 1, k                       # alive, placed nowhere: kept only at min_neigh 0
    assert adj[9] == 0                                              # its own normal is nan
    assert nb.sum() > 0
    compare(s, c, nrm, ref, mask, cell, 4.0, 0.5, 1, front, "special rows, min_neigh 1")
    # every neighbour cell names the nan-normal row: adjacent to nobody
    everywhere = np.full_like(front, 9)
    nb, adj, _ = compare(s, c, nrm, ref, mask, cell, 4.0, 0.5, 1, everywhere, "nan normal everywhere")
    assert nb.sum() > 0 and adj.sum() == 0


def test_more_than_64_views(ring):
    """The runtime loop over the groups of 64 views; mask bits >= V name no view."""
    s = ring
    rng = np.random.default_rng(6)
    n = 120
    c = rng.uniform(-0.02, 0.02, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, 80, n).astype(np.int32)
    nrm = toward_camera(s.Rp, s.t, c, ref)
    mask = random_masks(rng, n, 80, 0.5)
    assert mask.shape[1] == 2
    mask[::3, 1] |= np.uint64(0xFFFF) << np.uint64(16)
    for cell in (2, 4):
        front = fr.front_grid(*s.cam(), c, ref, mask, cell)[0]
        nb, adj, keep = compare(s, c, nrm, ref, mask, cell, 4.0, 0.75, 1, front, f"ring cell {cell}")
        print(f"ring cell {cell}: N sum {int(nb.sum())}, A sum {int(adj.sum())}, kept {int(keep.sum())}/{n}")
        assert nb.sum() > 0 and 0 < adj.sum() <= nb.sum() and 0 < keep.sum() < n
        # views of the second group have neighbours too
        assert any(v >= 64 and (front[v, max(j - 1, 0):j + 2, max(i - 1, 0):i + 2] >= 0).sum() > 1
                   for row in fr.placements(*s.cam(), c, ref, mask, cell) for v, (i, j), _ in row)


# ---------------------------------------------------------------------------
# 2. crafted grids
# ---------------------------------------------------------------------------
def test_crafted_front_grid(sphere, mixed):
    """A grid that was not built from the set: -1 and valid indices at random
    (dead rows among them), then entries outside -1..n-1, then p in its own
    neighbour cells."""
    s, m = sphere, mixed
    n = len(m["ref"])
    rng = np.random.default_rng(22)
    front = np.where(rng.random(m["front"].shape) < 0.3, -1, rng.integers(0, n, m["front"].shape)).astype(np.int32)
    ref = m["ref"].copy()
    ref[::7] = -1                                           # dead rows, named by the grid all the same
    want = compare(s, m["c"], m["nrm"], ref, m["mask"], 2, 2.0, 0.25, 1, front, "crafted grid")
    assert want[0].sum() > n and not want[0][::7].any() and not want[2][::7].any()
    host = s.ctx.wfilt_support(m["c"], m["nrm"], ref, m["mask"], 2, 2.0, 0.25, 1, front)
    for g, w in zip(host, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # entries outside -1..n-1 read as -1 on the device and are refused by the host-pointer call
    bad = front.copy()
    places = [(v, j, i) for p, row in enumerate(fr.placements(*s.cam(), m["c"], ref, m["mask"], 2)) if row
              for v, (i, j), _ in row[:1]]
    for k, value in enumerate((n, n + 5, -2, np.iinfo(np.int32).min, np.iinfo(np.int32).max)):
        v, j, i = places[k * 40]
        bad[v, j, i + 1] = value                            # a neighbour cell of a placed patch
    as_empty = np.where((bad < 0) | (bad >= n), -1, bad).astype(np.int32)
    got = gpu_support(s, m["c"], m["nrm"], ref, m["mask"], 2, 2.0, 0.25, 1, bad)
    want = sr.support(*s.cam(), m["c"], m["nrm"], ref, m["mask"], 2, 2.0, 0.25, 1, as_empty)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    with pytest.raises(RuntimeError, match="front entry outside"):
        s.ctx.wfilt_support(m["c"], m["nrm"], ref, m["mask"], 2, 2.0, 0.25, 1, bad)
    # every patch named in the cells around its own in every view it is placed in
    own = np.full_like(front, -1)
    count = np.zeros(n, np.int64)
    for p, row in enumerate(fr.placements(*s.cam(), m["c"], m["ref"], m["mask"], 2)):
        for v, (i, j), _ in row:
            if i + 1 < own.shape[2] and own[v, j, i + 1] < 0:
                own[v, j, i + 1] = p
                count[p] += 1
    assert count.sum() > n
    nb, _, _ = compare(s, m["c"], m["nrm"], m["ref"], m["mask"], 2, 2.0, 0.25, 1, own, "p beside itself")
    merged = np.where(own >= 0, own, m["front"])
    nb_m = compare(s, m["c"], m["nrm"], m["ref"], m["mask"], 2, 2.0, 0.25, 1, merged, "p beside itself, merged")[0]
    plain = sr.support(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], 2, 2.0, 0.25, 1, m["front"])[0]
    assert (nb_m < plain).any()                             # a neighbour replaced by p itself is one incidence less


def test_three_thousand_patches_around_one_neighbour(sphere):
    """3,000 patches on one pixel ray of view 5 and one common patch named in
    all eight cells around theirs: every wave gathers the same row."""
    s = sphere
    rng = np.random.default_rng(14)
    n, v = 3001, 5
    scale = np.concatenate([[1.0], rng.uniform(0.98, 1.02, n - 1)])
    c = np.array([s.at_pixel(v, 60.9, 40.9, k) for k in scale])
    nrm = toward_camera(s.Rp, s.t, c, np.full(n, v))
    ref = np.full(n, v, np.int32)
    mask = np.zeros((n, 1), np.uint64)
    i, j = er.cell_of(*s.cam()[:3], v, c[1], s.W, s.H, 2)
    front = np.full((s.V, s.H // 2, s.W // 2), -1, np.int32)
    front[v, j - 1:j + 2, i - 1:i + 2] = 0
    front[v, j, i] = 1
    nb, adj, keep = compare(s, c, nrm, ref, mask, 2, 2.0, 0.5, 8, front, "one neighbour")
    assert nb[0] == 0 and np.all(nb[1:] == 8) and set(adj[1:].tolist()) == {0, 8}
    assert 0 < keep.sum() < n - 1 and np.array_equal(keep[1:], (adj[1:] == 8).astype(np.uint8))


# ---------------------------------------------------------------------------
# 3. no shared state, arguments
# ---------------------------------------------------------------------------
def test_no_shared_state(sphere, mixed, orc):
    """score on the main stream, the support test on a side stream, score
    again: both scores are the oracle's and the support results the restatement's."""
    import torch
    s, m = sphere, mixed
    c, ref = m["c"], m["ref"]
    want_s = sr.support(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], 2, 2.0, 0.25, 1, m["front"])
    side = torch.cuda.Stream(torch.device("cuda:0"))
    first = s.ctx.score(c, ref, 0.7, 5)
    got = gpu_support(s, m["c"], m["nrm"], m["ref"], m["mask"], 2, 2.0, 0.25, 1, m["front"], stream=side)
    again = s.ctx.score(c, ref, 0.7, 5)
    got2 = gpu_support(s, m["c"], m["nrm"], m["ref"], m["mask"], 2, 2.0, 0.25, 1, m["front"], stream=side)
    want = orc.Scene(s.rgb, s.K, s.R, s.t_raw).score_batch(c, ref, 0.7, 5)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    for x, w in zip(first[:3], want[:3]):
        assert np.array_equal(x, w)
    assert np.allclose(first[3], want[3], rtol=0, atol=1e-12)
    for g, g2, w in zip(got, got2, want_s):
        assert np.array_equal(g, w) and np.array_equal(g2, w)


def test_arguments(pkg, sphere):
    s = sphere
    lib = pkg._lib.load()
    h = s.ctx.handle
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails its checks

    def call(n=1, cell=2, adj_px=2.0, ms=0.25, mn=1, ptr=one):
        return lib.mvs_wfilt_support_device(h, n, ptr, one, one, one, cell, adj_px, ms, mn, one, one, one, one, None)

    for bad, msg in ((dict(ms=float("nan")), "min_support must be in 0..1"),
                     (dict(ms=-0.1), "min_support must be in 0..1"),
                     (dict(ms=1.5), "min_support must be in 0..1"),
                     (dict(ms=float("inf")), "min_support must be in 0..1"),
                     (dict(mn=-1), "min_neigh < 0"),
                     (dict(cell=0), "cell_size must be in 1..16"),
                     (dict(cell=17), "cell_size must be in 1..16"),
                     (dict(adj_px=-1.0), "adj_px must be finite and >= 0"),
                     (dict(adj_px=float("nan")), "adj_px must be finite and >= 0"),
                     (dict(n=-1), "n < 0"),
                     (dict(n=1 << 31), "below 2^31"),
                     (dict(ptr=None), "null pointer")):
        assert call(**bad) == -1, bad                # MVS_E_ARG
        assert msg in pkg._lib.last_error(h), (msg, pkg._lib.last_error(h))
    assert call(n=0, ptr=None) == 0
    e3, e1, em = np.empty((0, 3)), np.empty(0, np.int32), np.empty((0, 1), np.uint64)
    front = np.full((s.V, s.H // 2, s.W // 2), -1, np.int32)
    nb, adj, keep = s.ctx.wfilt_support(e3, e3, e1, em, 2, 2.0, 0.25, 1, front)
    assert len(nb) == len(adj) == len(keep) == 0
    for kw, msg in ((dict(min_support=float("nan")), "min_support"), (dict(min_support=-0.1), "min_support"),
                    (dict(min_support=1.5), "min_support"), (dict(min_support=0.25, min_neigh=-1), "min_neigh")):
        with pytest.raises(RuntimeError, match=msg):
            s.ctx.wfilt_support(e3, e3, e1, em, 2, 2.0, kw.get("min_support"), kw.get("min_neigh", 1), front)
        with pytest.raises(RuntimeError, match=msg):
            s.ctx.filter_warped({"c": e3, "nrm": e3, "ref": e1, "mask": em, "avg": np.empty(0),
                                 "cell": np.empty((0, 2), np.int32)}, **kw)
