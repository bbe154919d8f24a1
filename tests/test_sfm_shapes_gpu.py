"""SfM front-end kernels (csrc/sfm_kernels.hip) against the oracle at the
shapes, window sizes and inputs the dinoRing tests of test_sfm.py never
reach: odd widths and heights, W < 64 and W, H > 1024, more than 2^20 pixels,
saturated gradients, maxima on the image border, every wid in 1..5, row counts
that do not fill a workgroup, more than 32,768 points, thresholds placed on a
reference value, and near ties that only the numpy-order ctNcc separates.

Reference: the oracle (harris_points, descriptors, match_best) on
gray_from_rgb of the same images.  Every comparison is exact (np.array_equal,
order included).  Every input is generated here from a fixed seed; the unmarked
tests check on the oracle alone that the constructed inputs are what the GPU
tests take them for."""
import ctypes
import functools

import numpy as np
import pytest

HARRIS_SHAPES = [(16, 16), (17, 19), (35, 67), (33, 257), (16, 1030), (1030, 17), (1030, 1030)]
HARRIS_KINDS = ["random", "binary", "border"]
FLAT_SHAPES = [(16, 16), (35, 67)]
FLAT_KINDS = ["constant", "ramp"]
ALL_KINDS = HARRIS_KINDS + FLAT_KINDS


def cameras(V):
    K = np.tile(np.array([[50., 0, 32], [0, 50., 24], [0, 0, 1]]), (V, 1, 1))
    return K, np.tile(np.eye(3), (V, 1, 1)), np.tile(np.array([0., 0, 1]), (V, 1))


def rgb_of(grays):
    return np.stack([np.repeat(g[:, :, None], 3, axis=2) for g in grays]).astype(np.uint8)


def context(pkg, grays):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return pkg.MvsContext(rgb_of(grays), *cameras(len(grays)))


def oracle_two_sided(orc, da, db, thr):
    b12, n12, f12 = orc.match_best(da, db, thr)
    b21, _, f21 = orc.match_best(db, da, thr)
    m12 = np.array([j if j >= 0 and b21[j] == i else -1 for i, j in enumerate(b12)], np.int32)
    return m12, b12, b21, f12, f21, n12


def assert_match_equal(cx, orc, grays, pa, pb, thr, wid):
    """match_two_sided(view 0 -> view 1) equals the oracle; returns the oracle's answer."""
    m12, b12, b21 = cx.match_two_sided(0, pa, 1, pb, thr, wid)
    ref = oracle_two_sided(orc, orc.descriptors(grays[0], pa, wid), orc.descriptors(grays[1], pb, wid), thr)
    assert b12.shape == ref[1].shape and b21.shape == ref[2].shape
    assert np.array_equal(b12, ref[1]), (wid, thr, np.flatnonzero(b12 != ref[1])[:8])
    assert np.array_equal(b21, ref[2]), (wid, thr, np.flatnonzero(b21 != ref[2])[:8])
    assert np.array_equal(m12, ref[0])
    return ref


# ---------------------------------------------------------------- 1. Harris shapes

def harris_image(kind, H, W, view):
    rng = np.random.default_rng([H, W, view, ALL_KINDS.index(kind)])
    if kind == "random":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)
    if kind == "border":
        # single bright pixels at the four corners and on each border: the
        # maxima sit where BORDER_REFLECT_101 and the border-ignoring dilation act
        g = np.full((H, W), 10 * view, np.uint8)
        hi = 255 - 55 * view
        for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2 + view),
                     (H - 1, W // 3 + view), (H // 2 + view, 0), (H // 3 + view, W - 1)]:
            g[y, x] = hi
        return g
    if kind == "constant":
        return np.full((H, W), 77 + 100 * view, np.uint8)
    ramp = (np.arange(W) * 255 // (W - 1)).astype(np.uint8)      # horizontal ramp, 0..255
    return np.ascontiguousarray(np.broadcast_to(ramp[::-1] if view else ramp, (H, W)))


@functools.lru_cache(maxsize=None)
def harris_case(orc, H, W, kind):
    """(gray views, oracle points per view) of one two-view case; computed once."""
    grays = [orc.gray_from_rgb(rgb_of([harris_image(kind, H, W, v)])[0]) for v in range(2)]
    for v in range(2):
        assert np.array_equal(grays[v], harris_image(kind, H, W, v))    # R = G = B keeps the value
    return grays, [orc.harris_points(g) for g in grays]


def test_harris_case_inputs(orc):
    """The constant and ramp images have no Harris point, every other case has
    some, and the two views of a case differ."""
    for H, W in FLAT_SHAPES:
        for kind in FLAT_KINDS:
            assert [len(p) for p in harris_case(orc, H, W, kind)[1]] == [0, 0], (H, W, kind)
    for H, W in HARRIS_SHAPES:
        for kind in HARRIS_KINDS:
            grays, pts = harris_case(orc, H, W, kind)
            assert len(pts[0]) > 0 and len(pts[1]) > 0, (H, W, kind)
            assert not np.array_equal(grays[0], grays[1])
    assert 1030 * 1030 > 4096 * 256            # k_harris / k_dilate_max grid stride entered


@pytest.mark.gpu
@pytest.mark.parametrize("kind", HARRIS_KINDS)
@pytest.mark.parametrize("shape", HARRIS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_harris_points_shapes(pkg, orc, shape, kind):
    grays, ref = harris_case(orc, *shape, kind)
    with context(pkg, grays) as cx:
        for v in (1, 0):
            got = cx.harris_points(v)
            assert got.shape == ref[v].shape, (v, got.shape, ref[v].shape)
            assert np.array_equal(got, ref[v]), v


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FLAT_KINDS)
@pytest.mark.parametrize("shape", FLAT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_harris_points_none(pkg, orc, shape, kind):
    grays, ref = harris_case(orc, *shape, kind)
    assert len(ref[0]) == 0 and len(ref[1]) == 0
    with context(pkg, grays) as cx:
        for v in range(2):
            got = cx.harris_points(v)
            assert got.shape == (0, 2)


# ---------------------------------------------------------------- 2. mvs_harris_points' cap

@pytest.mark.gpu
def test_harris_points_cap(pkg, orc):
    grays, ref = harris_case(orc, 35, 67, "random")
    lib = pkg._lib.load()
    i32p = ctypes.POINTER(ctypes.c_int32)
    total = len(ref[1])
    assert total > 20
    CANARY = -7777

    def call(cx, cap, null_out=False):
        buf = np.full((cap + 16, 2), CANARY, np.int32)
        n = ctypes.c_int64(-1)
        rc = lib.mvs_harris_points(cx._h, 1, None if null_out else buf.ctypes.data_as(i32p), cap,
                                   ctypes.byref(n))
        assert rc == 0, pkg._lib.last_error(cx._h)
        return n.value, buf

    with context(pkg, grays) as cx:
        n, _ = call(cx, 0, null_out=True)
        assert n == total
        n, buf = call(cx, 0)                                   # cap 0 with a buffer: nothing written
        assert n == total and (buf == CANARY).all()
        cap = total // 2
        n, buf = call(cx, cap)
        assert n == total
        assert np.array_equal(buf[:cap], ref[1][:cap]) and (buf[cap:] == CANARY).all()
        n, buf = call(cx, total + 5)
        assert n == total
        assert np.array_equal(buf[:total], ref[1]) and (buf[total:] == CANARY).all()
        # cap > 0 with a null buffer is an argument error, not a write
        n = ctypes.c_int64(-1)
        assert lib.mvs_harris_points(cx._h, 1, None, 4, ctypes.byref(n)) != 0


# ---------------------------------------------------------------- 3. matching, wid 1..5

MH, MW = 96, 128


@functools.lru_cache(maxsize=None)
def match_grays(orc):
    """Two 96x128 views: random bytes and a noisy copy (matching windows pass 0.5)."""
    rng = np.random.default_rng(11)
    g0 = rng.integers(0, 256, (MH, MW), dtype=np.uint8)
    g1 = np.clip(g0.astype(np.int32) + rng.integers(-12, 13, (MH, MW)), 0, 255).astype(np.uint8)
    grays = [orc.gray_from_rgb(rgb_of([g])[0]) for g in (g0, g1)]
    assert np.array_equal(grays[0], g0) and np.array_equal(grays[1], g1)
    return grays


def rand_points(rng, n, wid):
    """[row, col] inside getDescFeatures' bounds (HarrisFeatures.py:128)."""
    r = rng.integers(wid, MH - wid - 1, n)
    c = rng.integers(wid + 1, MW - wid - 1, n)
    return np.stack([r, c], 1).astype(np.int32)


def match_points(wid, n_a, n_b, shared=None):
    """n_a points of view 0 and n_b of view 1; the first `shared` of A also
    appear in B, at permuted indices."""
    rng = np.random.default_rng([17, wid, n_a, n_b])
    pa = rand_points(rng, n_a, wid)
    ns = min(n_a, n_b) if shared is None else shared
    pb = np.concatenate([pa[:ns], rand_points(rng, n_b - ns, wid)])
    return pa, pb[rng.permutation(n_b)]


MATCH_SIZES = [(1, 1, 1), (1, 130, 200), (2, 3, 63), (3, 4, 64), (3, 130, 200), (4, 5, 65),
               (5, 7, 129), (5, 130, 200)]


@pytest.fixture(scope="module")
def mctx(pkg, orc):
    with context(pkg, match_grays(orc)) as cx:
        yield cx


@pytest.mark.gpu
@pytest.mark.parametrize("wid,n_a,n_b", MATCH_SIZES)
def test_match_sizes(mctx, orc, wid, n_a, n_b):
    pa, pb = match_points(wid, n_a, n_b)
    ref = assert_match_equal(mctx, orc, match_grays(orc), pa, pb, 0.5, wid)
    assert (ref[0] >= 0).any()                  # mutual matches exist at every size


@pytest.mark.gpu
@pytest.mark.parametrize("wid", [1, 2, 3, 4, 5])
def test_match_empty_sides(mctx, orc, wid):
    grays = match_grays(orc)
    pa, pb = match_points(wid, 5, 9)
    none = np.zeros((0, 2), np.int32)
    m12, b12, b21 = mctx.match_two_sided(0, pa, 1, none, 0.5, wid)       # n_b = 0
    assert np.array_equal(m12, np.full(5, -1)) and np.array_equal(b12, np.full(5, -1))
    assert b21.shape == (0,)
    ref = assert_match_equal(mctx, orc, grays, pa, none, 0.5, wid)
    assert (ref[3] == 2).all()
    m12, b12, b21 = mctx.match_two_sided(0, none, 1, pb, 0.5, wid)       # n_a = 0
    assert m12.shape == (0,) and b12.shape == (0,)
    assert np.array_equal(b21, np.full(9, -1))
    assert_match_equal(mctx, orc, grays, none, pb, 0.5, wid)


@pytest.mark.gpu
def test_match_many_points_with_duplicates(mctx, orc):
    """33,000 A points drawn with repetition (more than 32,768: k_gather_desc's
    grid stride) against 40 B points: every B row sees exact duplicates of its
    best, several per lane."""
    wid = 2
    rng = np.random.default_rng(23)
    pa = rand_points(rng, 33000, wid)
    pb = pa[rng.choice(33000, 40, replace=False)]
    assert len(np.unique(pa, axis=0)) < 16500             # every point about three times
    ref = assert_match_equal(mctx, orc, match_grays(orc), pa, pb, 0.5, wid)
    assert (ref[4] == 1).sum() >= 20                      # tie rows in the reverse direction
    assert (ref[1] >= 0).sum() > 100


# ---------------------------------------------------------------- 4. thresholds on reference values

THR_ROWS = (0, 50, 95)


@functools.lru_cache(maxsize=None)
def threshold_case(orc, wid):
    """100 x 100 points (80 shared) and, for three rows, thr = the oracle's
    best ncc of that row, the double below it and the double above it."""
    grays = match_grays(orc)
    pa, pb = match_points(wid, 100, 100, shared=80)
    da, db = orc.descriptors(grays[0], pa, wid), orc.descriptors(grays[1], pb, wid)
    best, ncc, flags = orc.match_best(da, db, -2.0)
    thrs = []
    for i in THR_ROWS:
        v = float(ncc[i])
        thrs += [v, float(np.nextafter(v, -np.inf)), float(np.nextafter(v, np.inf))]
    return pa, pb, da, db, best, thrs


@pytest.mark.parametrize("wid", [1, 2, 3, 4, 5])
def test_threshold_case_inputs(orc, wid):
    """Each threshold is an oracle ncc bit for bit (or its neighbour), so the
    decision `ncc > thr` of that pair rests on the last bit."""
    pa, pb, da, db, best, thrs = threshold_case(orc, wid)
    for k, i in enumerate(THR_ROWS):
        assert best[i] >= 0
        v = orc.ctncc(da[i], db[best[i]])
        assert thrs[3 * k] == v and thrs[3 * k + 1] < v < thrs[3 * k + 2]
        assert np.float64(thrs[3 * k]).tobytes() == np.float64(v).tobytes()
        at, below, above = (orc.match_best(da[i:i + 1], db, t)[0][0] for t in thrs[3 * k:3 * k + 3])
        assert below == best[i] and at != best[i] and above != best[i]
    # a shared row's best is far above an unshared row's
    assert thrs[0] > 0.9 and thrs[3] > 0.9 and thrs[6] < 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("wid", [1, 2, 3, 4, 5])
def test_match_threshold_on_reference_value(mctx, orc, wid):
    pa, pb, _, _, _, thrs = threshold_case(orc, wid)
    for thr in thrs:
        assert_match_equal(mctx, orc, match_grays(orc), pa, pb, thr, wid)


# ---------------------------------------------------------------- 5. near ties

TIE_I, TIE_J, TIE_NA, TIE_NB = 2, 3, 6, 200
TIE_GRID = (10, 20)                                   # tiles per column, per row
# B index of each variant: "b", "b1" (first pair swapped), "b2" (second pair
# swapped; strictly the largest numpy-order ncc); (layout, expected best, oracle flag)
TIE_CASES = {
    "same_lane": ({TIE_J: "b", TIE_J + 64: "b1", TIE_J + 128: "b2"}, TIE_J + 128, 0),
    "other_lanes": ({TIE_J: "b", TIE_J + 1: "b1", TIE_J + 67: "b2"}, TIE_J + 67, 0),
    "best_first": ({TIE_J: "b2", TIE_J + 64: "b", TIE_J + 128: "b1"}, TIE_J, 0),
    "duplicate_best": ({TIE_J: "b", TIE_J + 1: "b1", TIE_J + 64: "b2", TIE_J + 128: "b2"}, TIE_J + 64, 1),
}


@functools.lru_cache(maxsize=None)
def tie_triple(orc, wid):
    """a, b, b1, b2 with equal integer moments against a (so equal closed-form
    ncc) and ctncc(a, b2) strictly above ctncc(a, b) and ctncc(a, b1)."""
    n = (2 * wid + 1) ** 2
    for seed in range(4000):
        rng = np.random.default_rng([5, wid, seed])
        a = rng.integers(0, 256, n, dtype=np.uint8)
        p = rng.permutation(n)[:4]
        a[p[1]] = a[p[0]]
        a[p[3]] = a[p[2]]
        b = np.clip(a.astype(np.int32) + rng.integers(-20, 21, n), 0, 255).astype(np.uint8)
        if b[p[0]] == b[p[1]] or b[p[2]] == b[p[3]]:
            continue
        b1, b2 = b.copy(), b.copy()
        b1[[p[0], p[1]]] = b[[p[1], p[0]]]
        b2[[p[2], p[3]]] = b[[p[3], p[2]]]
        v, v1, v2 = orc.ctncc(a, b), orc.ctncc(a, b1), orc.ctncc(a, b2)
        if v2 > v and v2 > v1:
            return a, {"b": b, "b1": b1, "b2": b2}
    raise AssertionError("no near-tie triple found")


@functools.lru_cache(maxsize=None)
def tie_scene(orc, wid, case):
    """Two mosaics of non-overlapping (2 wid + 1)^2 tiles, one descriptor per
    tile: view 0 holds the A windows (row TIE_I is `a`), view 1 the B windows
    (the variants of b at the case's indices, unrelated noise elsewhere)."""
    nb = 2 * wid + 1
    ty, tx = TIE_GRID
    H, W = ty * nb + 2, tx * nb + 3
    rng = np.random.default_rng([7, wid])
    g = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2)]
    a, var = tie_triple(orc, wid)
    pts = np.array([[(k // tx) * nb + wid, 1 + (k % tx) * nb + wid] for k in range(TIE_NB)], np.int32)

    def put(img, k, d):
        r, c = pts[k]
        img[r - wid:r + wid + 1, c - wid:c + wid + 1] = d.reshape(nb, nb)

    put(g[0], TIE_I, a)
    layout, expect, flag = TIE_CASES[case]
    for k, name in layout.items():
        put(g[1], k, var[name])
    grays = [orc.gray_from_rgb(rgb_of([x])[0]) for x in g]
    assert np.array_equal(grays[0], g[0]) and np.array_equal(grays[1], g[1])
    return grays, pts[:TIE_NA].copy(), pts, expect, flag


@pytest.mark.parametrize("wid", [5, 1])
def test_tie_construction(orc, wid):
    """The near-tie inputs are what test_match_near_ties takes them for: equal
    integer moments, the claimed order of the numpy-order values, and a row
    whose three variants beat every other entry."""
    a, var = tie_triple(orc, wid)
    ai = a.astype(np.int64)
    mom = [(int((ai * d.astype(np.int64)).sum()), int(d.astype(np.int64).sum()),
            int((d.astype(np.int64) ** 2).sum())) for d in var.values()]
    assert mom[0] == mom[1] == mom[2]
    assert len({d.tobytes() for d in var.values()}) == 3
    v = {k: orc.ctncc(a, d) for k, d in var.items()}
    assert v["b2"] > v["b"] and v["b2"] > v["b1"]
    assert v["b2"] - min(v.values()) < 1e-12                # inside the re-rank band
    for case, (layout, expect, flag) in TIE_CASES.items():
        grays, pa, pb, _, _ = tie_scene(orc, wid, case)
        da, db = orc.descriptors(grays[0], pa, wid), orc.descriptors(grays[1], pb, wid)
        assert np.array_equal(da[TIE_I], a)
        for k, name in layout.items():
            assert np.array_equal(db[k], var[name])
        best, ncc, flags = orc.match_best(da, db, 0.5)
        assert best[TIE_I] == expect and flags[TIE_I] == flag, case
        row = np.array([orc.ctncc(a, d) for d in db])
        others = np.delete(row, list(layout))
        assert not (others > min(v.values()) - 0.1).any()   # the variants are far above the rest
        assert ncc[TIE_I] == v["b2"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TIE_CASES))
@pytest.mark.parametrize("wid", [5, 1])
def test_match_near_ties(pkg, orc, wid, case):
    """Candidates whose closed-form ncc is bit-identical are ranked by their
    numpy-order ctNcc, however many of them one lane of k_match_rows meets
    (same_lane: j, j + 64, j + 128); exact duplicates go to the smallest j."""
    grays, pa, pb, expect, _ = tie_scene(orc, wid, case)
    with context(pkg, grays) as cx:
        m12, b12, b21 = cx.match_two_sided(0, pa, 1, pb, 0.5, wid)
        print(f"near tie wid {wid} {case}: oracle {expect}, GPU {b12[TIE_I]}")
        assert b12[TIE_I] == expect
        assert_match_equal(cx, orc, grays, pa, pb, 0.5, wid)
