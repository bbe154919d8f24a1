"""The runs path of the tiled scorer: k_bin sorts each workgroup's candidates
by tile into a private run (no global atomics) and k_score_tab gathers a tile's
list from the runs.  Every case is checked against the oracle: projections,
masks and counts bit-exact, avg within AVG_TOL, the record buffer pre-filled
with -1 so that an unwritten record shows."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AVG_TOL = 1e-12
N1 = 2 * 4096 + 17   # three binning workgroups, the last one partial


def _context(pkg, scene, **env):
    """A fresh context created under the given environment overrides."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.MvsContext(*scene, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _at_pixels(x, y, ref, K, R, t):
    """Candidates that project to pixel (x, y) of their reference view."""
    n = len(ref)
    z = np.full(n, 0.33)
    ray = np.einsum("nij,nj->ni", np.linalg.inv(K)[ref], np.stack([x, y, np.ones(n)], 1))
    c = np.einsum("nji,nj->ni", R[ref], z[:, None] * ray - t[ref].reshape(n, 3))
    return np.ascontiguousarray(c), ref


def _uniform(n, V, K, R, t, seed, W=128, H=96):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, V, n).astype(np.int32)
    return _at_pixels(rng.uniform(0, W, n), rng.uniform(0, H, n), ref, K, R, t)


def _score_rec(cx, c, ref, wid, stream=None):
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    tc, tr = torch.from_numpy(c).to(dev), torch.from_numpy(ref).to(dev)
    xy = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
    rec = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    if stream is None:
        cx.score_device_rec(tc, tr, xy, rec, 0.7, wid)
        torch.cuda.synchronize()
    else:
        cx.score_device_rec(tc, tr, xy, rec, 0.7, wid, stream=stream.cuda_stream)
        stream.synchronize()
    return xy.cpu().numpy(), rec.cpu().numpy()


def _check(got, want, tag=""):
    xy, rec = got
    oxy, omask, ocount, oavg = want
    mask = rec[:, 0].view(np.uint64)
    assert np.array_equal(xy, oxy), tag
    assert np.array_equal(mask, omask[:, 0]), tag
    assert np.array_equal(np.bitwise_count(mask).astype(np.int32), ocount), tag
    assert np.allclose(rec[:, 1].view(np.float64), oavg, rtol=0, atol=AVG_TOL), tag


class Small:
    """synthetic.sphere_scene(V, 96, 128): 96 tiles, dense from 6144 candidates."""

    def __init__(self, pkg, orc, V):
        rgb, K, R, t = pkg.synthetic.sphere_scene(V=V, H=96, W=128)[:4]
        self.V, self.scene, self.K, self.R, self.t = V, (rgb, K, R, t), K, R, t
        self.oracle = orc.Scene(rgb, K, R, t)
        self._want = {}

    def want(self, name, c, ref, wid):
        if (name, wid) not in self._want:
            self._want[name, wid] = self.oracle.score_batch(c, ref, 0.7, wid, nthreads=16)
        return self._want[name, wid]

    def uniform(self):
        return _uniform(N1, self.V, self.K, self.R, self.t, seed=71)

    def tiles(self, n, boxes, seed):
        """n candidates spread evenly over pixel boxes (x0, y0, w, h)."""
        rng = np.random.default_rng(seed)
        ref = rng.integers(0, self.V, n).astype(np.int32)
        b = np.asarray(boxes, np.float64)[rng.integers(0, len(boxes), n)]
        x = b[:, 0] + rng.random(n) * b[:, 2]
        y = b[:, 1] + rng.random(n) * b[:, 3]
        return _at_pixels(x, y, ref, self.K, self.R, self.t)


@pytest.fixture(scope="module")
def small(pkg, orc):
    return Small(pkg, orc, 24)


@pytest.fixture(scope="module")
def small_ctx(pkg, small):
    cx = pkg.MvsContext(*small.scene, device=0)
    yield cx
    cx.close()


def test_uniform_three_runs(small, small_ctx):
    """Case 1: three runs, the last from a partial workgroup."""
    c, ref = small.uniform()
    before = small_ctx.bin_runs_batches()
    _check(_score_rec(small_ctx, c, ref, 5), small.want("uniform", c, ref, 5))
    assert small_ctx.bin_runs_batches() == before + 1


def test_empty_run_between_full_ones(small, small_ctx):
    """Case 2: the second workgroup's 4096 candidates all project outside the
    image, so its run is empty."""
    c, ref = small.uniform()
    x = np.full(4096, -50.0)
    c = c.copy()
    c[4096:8192] = _at_pixels(x, x, ref[4096:8192], small.K, small.R, small.t)[0]
    before = small_ctx.bin_runs_batches()
    _check(_score_rec(small_ctx, c, ref, 5), small.want("hole", c, ref, 5))
    assert small_ctx.bin_runs_batches() == before + 1


def test_one_tile_chunks_and_overflow(pkg, small, small_ctx):
    """Case 3: 8192 candidates in one textured tile: more than one chunk of
    them below the bucket capacity (further rounds of the gathering
    workgroup), the rest past it (the direct path's list): exact outputs, and
    the same overflow count as the atomic path's."""
    c, ref = small.tiles(8192, [(64.01, 48.01, 15.98, 7.98)], seed=72)
    want = small.want("one_tile", c, ref, 5)
    before, runs_before = small_ctx.scorer_stats(), small_ctx.bin_runs_batches()
    _check(_score_rec(small_ctx, c, ref, 5), want)
    over = small_ctx.scorer_stats()["overflow"] - before["overflow"]
    assert small_ctx.bin_runs_batches() == runs_before + 1
    ca = _context(pkg, small.scene, MVS_BIN="atomic")
    try:
        before = ca.scorer_stats()
        _check(_score_rec(ca, c, ref, 5), want, "atomic")
        assert ca.bin_runs_batches() == 0
        # cap = 16 x the mean load (1408 here): two chunks below it, the rest over
        assert over == ca.scorer_stats()["overflow"] - before["overflow"] == 8192 - 1408
    finally:
        ca.close()


def test_two_diagonal_tiles_and_a_few_elsewhere(small, small_ctx):
    """Case 4: most tiles have no entry in most runs."""
    c, ref = small.tiles(8192, [(48.01, 40.01, 15.98, 7.98), (64.01, 48.01, 15.98, 7.98)], seed=73)
    c2, ref2 = _uniform(300, small.V, small.K, small.R, small.t, seed=74)
    c, ref = np.concatenate([c, c2]), np.concatenate([ref, ref2])
    before = small_ctx.bin_runs_batches()
    _check(_score_rec(small_ctx, c, ref, 5), small.want("two_tiles", c, ref, 5))
    assert small_ctx.bin_runs_batches() == before + 1


def test_wid3_and_20_views(pkg, orc, small, small_ctx):
    """Case 5: window half-width 3, and a scene of 20 views (not a multiple
    of 16), at case 1's shape."""
    c, ref = small.uniform()
    _check(_score_rec(small_ctx, c, ref, 3), small.want("uniform", c, ref, 3), "wid 3")
    s20 = Small(pkg, orc, 20)
    c, ref = s20.uniform()
    with pkg.MvsContext(*s20.scene, device=0) as cx:
        for wid in (5, 3):
            _check(_score_rec(cx, c, ref, wid), s20.want("uniform", c, ref, wid), f"V 20 wid {wid}")
        assert cx.bin_runs_batches() == 2


def test_run_limit_falls_back_to_atomic(pkg, small, small_ctx):
    """Case 6: with MVS_BIN_RUNS_MAX=2 case 1's three workgroups keep the
    atomic buckets; same outputs as the runs path."""
    c, ref = small.uniform()
    runs = _score_rec(small_ctx, c, ref, 5)
    cx = _context(pkg, small.scene, MVS_BIN_RUNS_MAX="2")
    try:
        got = _score_rec(cx, c, ref, 5)
        assert cx.bin_runs_batches() == 0
        _check(got, small.want("uniform", c, ref, 5))
        assert np.array_equal(got[0], runs[0]) and np.array_equal(got[1][:, 0], runs[1][:, 0])
        assert np.allclose(got[1][:, 1].view(np.float64), runs[1][:, 1].view(np.float64), rtol=0, atol=AVG_TOL)
        # two workgroups are within the limit
        c2, ref2 = c[:8192], ref[:8192]
        _check(_score_rec(cx, c2, ref2, 5), small.oracle.score_batch(c2, ref2, 0.7, 5, nthreads=16))
        assert cx.bin_runs_batches() == 1
    finally:
        cx.close()


def test_paths_alternate_on_two_streams(pkg, dino, oracle_scene):
    """Case 7: one dinoRing context, two streams in turn: dense (runs), sparse
    (atomic buckets, k_item_scan), dense, small (direct kernel), dense -- the
    counter sets' zero-on-next-batch logic across the two binning paths."""
    import torch
    from conftest import bench_candidates
    rgb, K, R, t = dino
    dev = torch.device("cuda:0")
    batches = {
        "dense": bench_candidates(1 << 18, K, R, t, seed=61),
        "sparse": bench_candidates(50000, K, R, t, seed=62),
        "small": bench_candidates(1500, K, R, t, seed=63),
    }
    want = {k: oracle_scene.score_batch(c, ref, 0.7, 5, nthreads=16) for k, (c, ref) in batches.items()}
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    with pkg.MvsContext(rgb, K, R, t, device=0) as cx:
        runs = []
        for j, kind in enumerate(["dense", "sparse", "dense", "small", "dense"]):
            c, ref = batches[kind]
            _check(_score_rec(cx, c, ref, 5, stream=streams[j % 2]), want[kind], (j, kind))
            runs.append(cx.bin_runs_batches())
        assert runs == [1, 1, 2, 2, 3]


@pytest.mark.parametrize("fresh", [False, True])
def test_empty_batch_keeps_counter_sets(pkg, small, fresh):
    """Case 8: under MVS_SCORE_KERNEL=tiled an empty batch launches nothing,
    so it must leave the counter sets' parity and clean state alone: the next
    real batch is exact, with the empty batch after a real one and as the
    context's first."""
    c, ref = small.uniform()
    want = small.want("uniform", c, ref, 5)
    cx = _context(pkg, small.scene, MVS_SCORE_KERNEL="tiled")
    try:
        if not fresh:
            _check(_score_rec(cx, c, ref, 5), want, "before")
        xy, rec = _score_rec(cx, c[:0], ref[:0], 5)
        assert xy.shape == (0, 2) and rec.shape == (0, 2)
        _check(_score_rec(cx, c, ref, 5), want, "after")
        _check(_score_rec(cx, c, ref, 5), want, "again")
    finally:
        cx.close()
