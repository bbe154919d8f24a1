"""The MVS scene build, moment tables, binning and scorers at image sizes that
are no multiple of their blocks (k_build_scene: 64-pixel strips, 16-byte
pieces, quads; k_moments: 32 x 16 pixels x 16 views; k_bin and the scorers:
16 x 8 tiles), at the minimum size and past 2048 columns, with passing
candidates in the partial edge tiles (shapes_scene.py; what the batches reach
is asserted by test_mvs_shapes_host.py).  Every case against the oracle: xy,
masks and counts bit-exact, avg within AVG_TOL."""
import os

import numpy as np
import pytest

import shapes_scene as ss

pytestmark = pytest.mark.gpu

AVG_TOL = 1e-12
DENSE_MEAN = 64   # candidates per tile, on average, from which a batch is binned into runs (mvs_bin.hip)
# MVS_SCORE_KERNEL (None: unset) and MVS_BIN of a fresh context
MODES = {"auto": (None, None), "direct": ("direct", None), "tiled": ("tiled", None), "mma": ("mma", None),
         "tab": ("tab", None), "atomic": (None, "atomic")}


def _context(pkg, scene, kernel=None, binning=None):
    """A fresh context created under MVS_SCORE_KERNEL = kernel and MVS_BIN =
    binning (None: unset), the environment as it was afterwards."""
    env = {"MVS_SCORE_KERNEL": kernel, "MVS_BIN": binning}
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return pkg.MvsContext(*scene, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Case:
    """One of shapes_scene.SCENES: scene, candidates, and the oracle's answers,
    computed once per (wid, thr) and shared by every context."""

    def __init__(self, orc, H, W, V):
        self.H, self.W, self.V = H, W, V
        self.scene, (self.c, self.ref) = ss.scene_and_candidates(H, W, V)
        self.oracle = orc.Scene(*self.scene)
        self._want = {}

    def want(self, wid, thr):
        if (wid, thr) not in self._want:
            self._want[wid, thr] = self.oracle.score_batch(self.c, self.ref, thr, wid, nthreads=16)
        return self._want[wid, thr]


_cases = {}


def _case(orc, H, W, V):
    if (H, W, V) not in _cases:
        _cases[H, W, V] = Case(orc, H, W, V)
    return _cases[H, W, V]


def _check_arrays(got, want, tag):
    for name, g, e in zip(("xy", "mask", "count"), got[:3], want[:3]):
        assert np.array_equal(g, e), (tag, name, np.nonzero(np.asarray(g != e).reshape(len(e), -1).any(1))[0][:8])
    assert np.allclose(got[3], want[3], rtol=0, atol=AVG_TOL), tag


def _score_rec(cx, c, ref, thr, wid):
    """score_device_rec into xy and records pre-filled with -1: a record or a
    projection left unwritten shows."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    tc, tr = torch.from_numpy(c).to(dev), torch.from_numpy(ref).to(dev)
    xy = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
    rec = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cx.score_device_rec(tc, tr, xy, rec, thr, wid)
    torch.cuda.synchronize()
    return xy.cpu().numpy(), rec.cpu().numpy()


def _check_rec(got, want, tag):
    xy, rec = got
    mask = rec[:, 0].view(np.uint64)
    got4 = (xy, mask.reshape(-1, 1), np.bitwise_count(mask).astype(np.int32), rec[:, 1].view(np.float64))
    _check_arrays(got4, want, tag)


def _expected_path(case, mode, n):
    """(timed kernel, whether the batch is binned into runs) of a batch of n
    >= 2048 candidates: the direct kernel only where it is forced; the
    view-group scorer at V > 64; the table scorer at V <= 64 unless the
    in-kernel moments are forced; runs only ahead of the table scorer, on a
    dense batch, and not under MVS_BIN=atomic."""
    ntiles = -(-case.W // ss.TILE_W) * -(-case.H // ss.TILE_H)
    if mode == "direct":
        return "k_score", False
    if case.V > 64:
        return "k_score_mma_v", False
    if mode == "mma":
        return "k_score_mma", False
    return "k_score_tab", mode != "atomic" and n >= DENSE_MEAN * ntiles


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H,W,V", ss.SCENES)
def test_scores_at_odd_sizes(pkg, orc, H, W, V, mode):
    """Every window size and three thresholds through a fresh context of each
    scoring path, host arrays and (V <= 64) records; the context took the
    path the mode names."""
    case = _case(orc, H, W, V)
    n = len(case.ref)
    assert n >= 2048   # the auto mode tiles
    kernel, runs = _expected_path(case, mode, n)
    cx = _context(pkg, case.scene, *MODES[mode])
    try:
        cx.kernel_timing(True)
        for wid in ss.WIDS:
            for thr in ss.THR:
                want = case.want(wid, thr)
                before = cx.bin_runs_batches()
                _check_arrays(cx.score(case.c, case.ref, thr, wid), want, (wid, thr))
                assert cx.timed_kernel() == kernel, (wid, thr)
                assert cx.bin_runs_batches() - before == int(runs), (wid, thr)
                if V <= 64:
                    _check_rec(_score_rec(cx, case.c, case.ref, thr, wid), want, (wid, thr, "rec"))
                    assert cx.timed_kernel() == kernel and cx.bin_runs_batches() - before == 2 * int(runs)
    finally:
        cx.close()


def test_both_binning_paths_are_reached(orc):
    """The scenes put the table scorer behind the runs and behind the atomic
    tile buckets (the wide image: too few candidates per tile)."""
    runs = {s: _expected_path(_case(orc, *s), "auto", len(_case(orc, *s).ref)) for s in ss.SCENES}
    assert ("k_score_tab", True) in runs.values() and ("k_score_tab", False) in runs.values()
    assert "k_score_mma_v" in [k for k, _ in runs.values()]


def test_rebuild_follows_image_edits(pkg, orc):
    """Images edited across the last tile column of 39 x 45 x 17 -- a textured
    block made constant in one view, new colours in another, the constant
    corner of a third textured -- then rebuild(): the gray copies, the moment
    tables built before the edit (wid 5, 2) and the constant-window bits
    follow it; a table built afterwards (wid 3) too."""
    case = _case(orc, 39, 45, 17)
    rgb, K, R, t = case.scene
    rng = np.random.default_rng(13)
    new = rgb.copy()
    new[2, 8:30, 26:41] = 90
    new[4, 8:30, 26:41] = rng.integers(0, 256, (22, 15, 3), dtype=np.uint8)
    new[0, 25:, 29:] = rng.integers(0, 256, (14, 16, 3), dtype=np.uint8)
    fresh = orc.Scene(new, K, R, t)
    with pkg.MvsContext(rgb, K, R, t, device=0) as cx:
        for wid in (5, 2):
            _check_arrays(cx.score(case.c, case.ref, 0.7, wid), case.want(wid, 0.7), ("before", wid))
        cx.set_images(2, new[2:5])
        cx.set_images(0, new[:1])
        cx.rebuild()
        for wid in (5, 2, 3):
            want = fresh.score_batch(case.c, case.ref, 0.7, wid, nthreads=16)
            old = case.want(wid, 0.7)
            assert (want[1] != old[1]).any(1).sum() > 200   # the edit changes many masks
            _check_arrays(cx.score(case.c, case.ref, 0.7, wid), want, ("after", wid))
            _check_rec(_score_rec(cx, case.c, case.ref, 0.7, wid), want, ("after", wid, "rec"))


def _border_parents(orc, K, R, t, W, H, n, seed):
    """Parent patches whose projections cover the image up to its border:
    centre, normal toward the reference camera, projection into the reference
    view (MVS2.py:238-247)."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, len(K), n).astype(np.int32)
    x = np.where(rng.random(n) < 0.5, rng.uniform(0, W, n), rng.uniform(W - 14, W, n))
    y = np.where(rng.random(n) < 0.5, rng.uniform(0, H, n), rng.uniform(H - 12, H, n))
    c, _ = ss.at_pixels(x, y, ref, K, R, t)
    pn, pxy = np.empty_like(c), np.empty((n, 2))
    for k in range(n):
        O = -(R[ref[k]].T @ t[ref[k]].ravel())
        pn[k] = (O - c[k]) / np.linalg.norm(O - c[k])
        pxy[k] = orc.project(K[ref[k]], orc.rodrigues_roundtrip(R[ref[k]]), t[ref[k]].ravel(), c[k])
    return c, pn, pxy


@pytest.mark.parametrize("n_jobs", [700, 4096])
def test_expand_candidates_near_the_border(pkg, orc, n_jobs):
    """mvs_expand_candidates on 39 x 45 x 17 with parents up to the image
    border (children in the partial tiles and outside the image): every
    output of every job bit-exact against the oracle, on the direct path
    (below 2,048 jobs) and the tiled one."""
    case = _case(orc, 39, 45, 17)
    rgb, K, R, t = case.scene
    rng = np.random.default_rng(n_jobs)
    pc, pn, pxy = _border_parents(orc, K, R, t, case.W, case.H, 400, seed=n_jobs)
    jp = rng.integers(0, len(pc), n_jobs).astype(np.int32)
    jv = rng.integers(0, case.V, n_jobs).astype(np.int32)
    jd = rng.choice(np.array([-1, 1], np.int32), n_jobs)
    exp = case.oracle.expand_candidates(pc, pn, pxy, jp, jv, jd, cell_size=2, scale=10.0, wid=5, thr=0.7)
    with pkg.MvsContext(rgb, K, R, t, device=0) as cx:
        got = cx.expand_candidates(pc, pn, pxy, jp, jv, jd, cell_size=2, scale=10.0, wid=5, min_ncc=0.7)
    for name, g, e in zip(("X", "nX", "color", "xy", "mask", "count", "accept"), got, exp):
        assert np.array_equal(g, e), name
    xl, yl = ss.last_tile_origin(case.W, case.H)
    edge = (exp[3][:, 0] >= xl) | (exp[3][:, 1] >= yl)
    assert (exp[5][edge] > 0).sum() >= 20 and exp[6].sum() > 0
    # children whose cell centre lies past the last column or row (colour 0 0 0)
    cc = 2.0 * (np.floor(pxy[jp] / 2.0) + jd[:, None] + 0.5)
    past = (cc[:, 0] >= case.W) | (cc[:, 1] >= case.H)
    assert past.sum() >= 10 and not exp[2][past].any()


def _emulated_ranks(pkg, scene, tracks, pops, world):
    """The multi-rank protocol on one device, as test_stage_sphere_scene runs
    it: one context and stepped stage per rank, the slices exchanged by hand."""
    import torch
    ctxs = [pkg.MvsContext(*scene, device=0) for _ in range(world)]
    try:
        sts = [c.stage_begin(*tracks, cell_size=2, scale=10.0, wid=5, max_pops=pops, rank=r, world=world)
               for r, c in enumerate(ctxs)]
        dev = torch.device("cuda", 0)
        while True:
            njs = [s.plan() for s in sts]
            assert len(set(njs)) == 1
            if njs[0] == 0:
                break
            smax = sts[0].slice_max(njs[0])
            outs = [torch.full((smax, sts[0].width), -7, dtype=torch.int64, device=dev) for _ in range(world)]
            for s, o in zip(sts, outs):
                s.score_slice(o)
            allbuf = torch.stack(outs)
            for s in sts:
                s.ingest(allbuf)
        res = [s.finish() for s in sts]
        for s in sts:
            s.close()
    finally:
        for c in ctxs:
            c.close()
    return res


@pytest.mark.parametrize("V,H,W,pops,world", [(24, 89, 125, 2000, 1), (70, 71, 109, 800, 2)])
def test_stage_at_odd_sizes(pkg, orc, V, H, W, pops, world):
    """The whole stage on sphere scenes of odd sizes (the cell grid at odd
    H / 2 and W / 2, partial tiles in every sweep): rows, tests and queue_left
    equal to the oracle's, single rank and the emulated 2-rank protocol."""
    rgb, K, R, t, off, ov, oxy = pkg.synthetic.sphere_scene(V=V, H=H, W=W, seed=V)
    oini, oall, ost = orc.Scene(rgb, K, R, t).mvs_stage(off, ov, oxy, scale=10.0, max_pops=pops)
    assert len(oini) > 100 and len(oall) > 5000
    with pkg.MvsContext(rgb, K, R, t, device=0) as cx:
        res = [cx.stage(off, ov, oxy, cell_size=2, scale=10.0, wid=5, max_pops=pops)]
    if world > 1:
        res += _emulated_ranks(pkg, (rgb, K, R, t), (off, ov, oxy), pops, world)
    for ini, allp, st in res:
        assert np.array_equal(ini, oini) and np.array_equal(allp, oall)
        assert st["tests"] == ost["tests"] and st["queue_left"] == ost["queue_left"]
