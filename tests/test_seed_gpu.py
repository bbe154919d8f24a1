"""The seed matcher and the patch colours on the GPU (k_wseed_pairs,
k_wseed_scan, k_wpatch_color through mvs_wseed_match[_device],
mvs_wpatch_color[_device], MvsContext.seed_warped and MVS2.DensePointsWarped)
against the float64 restatement (tests/seed_reference.py).

Every comparison with the restatement is exact, with no row left out and no
tolerance: the bits of c, nrm and err, the rows of cand and ref, the total; the
bits of color and nviews.

Sizes: a workgroup of k_wseed_pairs takes 256 features a (first blocks of 0, 1,
63, 64, 65 and 257), a tile of LDS 256 features b (255, 256, 257), k_wseed_scan
1,024 rows at a time (1,023, 1,024, 1,025 rows); k_wpatch_color puts four
patches in a workgroup (n = 1, 3, 4, 5, 257) and loops over groups of 64 views
(the 80-view ring).
"""
import ctypes
import types

import numpy as np
import pytest

import seed_reference as sd
from test_expand_gpu import random_masks
from test_wfilt_gpu import Scene, _dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sphere(pkg):
    p = sd.planted(pkg)
    s = Scene(pkg, p["rgb"], p["K"], p["R"], p["t_raw"])
    assert np.array_equal(s.Rp, p["Rp"])
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def ring(pkg):
    rgb, K, R, t = pkg.synthetic.ring_scene(V=80, H=48, W=64)
    s = Scene(pkg, rgb, K, R, t)
    yield s
    s.ctx.close()


def gpu_match(s, feat, feat_off, pairs, epi_px, min_sin2, cap=None, stream=None):
    """mvs_wseed_match_device on outputs of cap + 3 rows pre-filled with a
    canary pattern (cap None: a counting call gives it) -> the restatement's
    dict of the first min(total, cap) rows, and the total; the rows past them
    must hold the canary."""
    import torch
    dev = torch.device("cuda:0")
    st = stream if stream is not None else torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tf = _dev(np.asarray(feat, np.int32).reshape(-1, 2))
        total = torch.full((1,), -77, dtype=torch.int64, device=dev)
        if cap is None:
            s.ctx.wseed_match_device(tf, feat_off, pairs, epi_px, min_sin2, None, None, None, None, None, total,
                                     stream=st.cuda_stream)
            cap = int(total.item())
            total.fill_(-77)
        room = cap + 3
        c = torch.full((room, 3), -77.0, dtype=torch.float64, device=dev)
        nrm = torch.full((room, 3), -77.0, dtype=torch.float64, device=dev)
        ref = torch.full((room,), -77, dtype=torch.int32, device=dev)
        cand = torch.full((room, 4), -77, dtype=torch.int32, device=dev)
        err = torch.full((room,), -77.0, dtype=torch.float64, device=dev)
        if cap:
            s.ctx.wseed_match_device(tf, feat_off, pairs, epi_px, min_sin2, c[:cap], nrm[:cap], ref[:cap], cand[:cap],
                                     err[:cap], total, stream=st.cuda_stream)
        else:
            s.ctx.wseed_match_device(tf, feat_off, pairs, epi_px, min_sin2, None, None, None, None, None, total,
                                     stream=st.cuda_stream)
        out = {k: x.cpu().numpy() for k, x in (("c", c), ("nrm", nrm), ("ref", ref), ("cand", cand), ("err", err))}
        tot = int(total.item())
    st.synchronize()
    k = min(tot, cap) if tot >= 0 else 0
    for name, x in out.items():
        assert np.all(x[k:] == -77), (name, "written past min(total, cap)")
    return {name: x[:k] for name, x in out.items()}, tot


def same(got, want, label=""):
    for k in ("c", "nrm", "err"):
        assert got[k].tobytes() == want[k].tobytes(), (label, k)
    for k in ("ref", "cand"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (label, k)


def compare(s, feat, feat_off, pairs, epi_px=1.5, min_sin2=1e-4, label=""):
    want = sd.match(s.K, s.Rp, s.t, feat, feat_off, pairs, epi_px, min_sin2)
    got, tot = gpu_match(s, feat, feat_off, pairs, epi_px, min_sin2)
    assert tot == len(want["err"]), (label, tot, len(want["err"]))
    same(got, want, label)
    return want


def random_feats(s, rng, counts, margin=0):
    """counts[v] distinct random integer pixels per view -> feat, feat_off."""
    feats = []
    for n in counts:
        flat = rng.choice((s.W - 2 * margin) * (s.H - 2 * margin), size=int(n), replace=False)
        w = s.W - 2 * margin
        feats.append(np.stack([flat % w + margin, flat // w + margin], 1).astype(np.int32).reshape(-1, 2))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return np.concatenate(feats).reshape(-1, 2), off


# ---------------------------------------------------------------------------
# 1. against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("epi_px", [0.75, 1.5, 2.0])
def test_planted_set(pkg, sphere, epi_px):
    s, p = sphere, sd.planted(pkg)
    want = sd.planted_match(pkg, epi_px)
    got, tot = gpu_match(s, p["feat"], p["feat_off"], p["pairs"], epi_px, 1e-4)
    assert tot == len(want["err"])
    same(got, want, f"epi_px {epi_px}")
    true = sd.true_rows(p, want)
    print(f"epi_px {epi_px}: {tot} candidates, {int(true.sum())} of one planted point")
    if epi_px == 1.5:
        assert tot == 52822 and true.sum() == 7481


@pytest.mark.parametrize("na", [0, 1, 63, 64, 65, 257])
def test_first_block(sphere, na):
    """View 0 holds na features: 0, 1 or 2 workgroups per pair, a partial last
    wave; view 2 in the middle of the pair list has none."""
    s = sphere
    counts = np.full(s.V, 40)
    counts[0], counts[2] = na, 0
    feat, off = random_feats(s, np.random.default_rng(na), counts)
    pairs = [(0, 1), (1, 2), (2, 1), (1, 0), (0, 23), (3, 4), (0, 2), (23, 0)]
    want = compare(s, feat, off, pairs, 2.0, 1e-4, f"na {na}")
    if na >= 63:
        assert len(want["err"]) > 0 and (want["cand"][:, 0] == 0).any() and (want["cand"][:, 0] == 5).any()


@pytest.mark.parametrize("nb", [255, 256, 257])
def test_lds_tile(sphere, nb):
    s = sphere
    counts = np.full(s.V, 0)
    counts[4], counts[5], counts[6] = 70, nb, 513
    feat, off = random_feats(s, np.random.default_rng(nb), counts)
    want = compare(s, feat, off, [(4, 5), (5, 4), (4, 6)], 2.0, 1e-4, f"nb {nb}")
    b45 = want["cand"][want["cand"][:, 0] == 0][:, 2]
    assert b45.max() >= nb - 6 and want["cand"][want["cand"][:, 0] == 2][:, 2].max() >= 512 - 30


@pytest.mark.parametrize("rows", [1023, 1024, 1025])
def test_scan_block(sphere, rows):
    s = sphere
    counts = np.full(s.V, 0)
    counts[0], counts[1], counts[2], counts[3] = 341, 341, rows - 682, 12
    feat, off = random_feats(s, np.random.default_rng(rows), counts)
    want = compare(s, feat, off, [(0, 3), (1, 3), (2, 3)], 2.0, 1e-4, f"rows {rows}")
    assert (want["cand"][:, 0] == 2).any()


def test_cap(pkg, sphere):
    s, p = sphere, sd.planted(pkg)
    pairs = p["pairs"][:6]
    want = sd.match(s.K, s.Rp, s.t, p["feat"], p["feat_off"], pairs, 1.5, 1e-4)
    n = len(want["err"])
    assert n > 1000
    for cap in (0, n - 1, n, n + 5):
        got, tot = gpu_match(s, p["feat"], p["feat_off"], pairs, 1.5, 1e-4, cap=cap)
        assert tot == n
        same(got, {k: v[:cap] for k, v in want.items()}, f"cap {cap}")
    # the host-pointer call: the same rows through the staging arena
    c, nrm, ref, cand, err, tot = s.ctx.wseed_match(p["feat"], p["feat_off"], pairs, 1.5, 1e-4)
    assert tot == n
    same({"c": c, "nrm": nrm, "ref": ref, "cand": cand, "err": err}, want, "host pointers")
    c, nrm, ref, cand, err, tot = s.ctx.wseed_match(p["feat"], p["feat_off"], pairs, 1.5, 1e-4, cap=7)
    assert tot == n and len(ref) == 7 and np.array_equal(cand, want["cand"][:7])


def test_repeated_pair_duplicate_feature_and_border(sphere):
    s = sphere
    rng = np.random.default_rng(3)
    counts = np.full(s.V, 30)
    feat, off = random_feats(s, rng, counts)
    feat[off[7] + 3] = feat[off[7] + 2]                                  # a duplicated feature
    corners = [(0, 0), (s.W - 1, 0), (0, s.H - 1), (s.W - 1, s.H - 1), (0, 40), (s.W - 1, 41), (60, 0), (61, s.H - 1)]
    feat[off[8]:off[8] + 8] = corners                                    # features on the image border
    feat[off[7] + 10:off[7] + 18] = corners
    pairs = [(7, 8), (8, 7), (7, 8), (7, 6), (8, 9)]
    want = compare(s, feat, off, pairs, 3.0, 1e-4, "repeat")
    k0, k2 = want["cand"][:, 0] == 0, want["cand"][:, 0] == 2
    assert k0.sum() > 0 and np.array_equal(want["cand"][k0][:, 1:], want["cand"][k2][:, 1:])
    assert want["c"][k0].tobytes() == want["c"][k2].tobytes()
    a = want["cand"][k0]
    assert (a[:, 1] == 2).sum() == (a[:, 1] == 3).sum()


def test_parallel_rays_and_min_sin2(pkg, sphere):
    """A second context in which views 0 and 1 share a rotation, with one
    feature pixel in common: d_a and d_b are the same bits and den is exactly 0.
    min_sin2 = 0 must skip that pair; a min_sin2 near 1 removes every pair."""
    p = sd.planted(pkg)
    R = p["R"].copy()
    R[1] = R[0]
    s = Scene(pkg, p["rgb"], p["K"], R, p["t_raw"])
    try:
        assert np.array_equal(s.Rp[0], s.Rp[1])
        counts = np.full(s.V, 25)
        feat, off = random_feats(s, np.random.default_rng(8), counts)
        feat[off[1] + 5] = feat[off[0] + 9]
        da = sd.pixel_ray([float(x) for x in s.Rp[0].reshape(9)], float(s.K[0][0, 0]), float(s.K[0][1, 1]),
                          float(s.K[0][0, 2]), float(s.K[0][1, 2]), *feat[off[0] + 9])
        A = sd.dot3(da, da)
        assert A * A - A * A == 0.0
        for ms in (0.0, 1e-4):
            want = compare(s, feat, off, [(0, 1), (1, 0), (0, 2), (2, 0)], 2.0, ms, f"min_sin2 {ms}")
            assert len(want["err"]) > 0
            assert not ((want["cand"][:, 0] == 0) & (want["cand"][:, 1] == 9) & (want["cand"][:, 2] == 5)).any()
        want = compare(s, feat, off, [(0, 1), (1, 0), (0, 2), (2, 0)], 2.0, 0.999999, "min_sin2 near 1")
        assert len(want["err"]) == 0
    finally:
        s.ctx.close()


def test_crossing_behind_a_camera(sphere):
    """Views 0 and 6 look at the scene at a right angle.  A point behind camera
    0 on the ray of a feature of view 0 has a positive depth in view 6; its
    rounded projection there (a pixel far outside the image: a feature is any
    integer pixel) is a feature b whose ray meets a's ray behind camera 0: s < 0
    in the pair (0, 6), u < 0 in (6, 0), no candidate.  The same construction
    in front of camera 0 gives one candidate per pair."""
    s = sphere
    a = (s.W // 2 + 3, s.H // 2 - 2)
    found = {}
    for name, scale in (("behind", -0.5), ("front", 1.0)):
        Y = s.at_pixel(0, a[0], a[1], scale)
        x, y, depth = sd.wr.project_ref(s.K[6], s.Rp[6], s.t[6], Y)
        assert depth > 0
        feat = np.array([a, (int(round(x)), int(round(y)))], np.int32)
        off = np.zeros(s.V + 1, np.int64)
        off[1:7] = 1
        off[7:] = 2
        want = compare(s, feat, off, [(0, 6), (6, 0)], 3.0, 0.0, name)
        found[name] = len(want["err"])
    assert found == {"behind": 0, "front": 2}


def test_more_than_64_views(ring):
    s = ring
    counts = np.zeros(s.V, np.int64)
    counts[[0, 1, 62, 63, 64, 65, 70, 71, 78, 79]] = 45
    feat, off = random_feats(s, np.random.default_rng(12), counts)
    pairs = [(64, 65), (65, 64), (63, 64), (79, 0), (0, 79), (70, 71), (78, 79), (1, 62)]
    want = compare(s, feat, off, pairs, 2.0, 1e-4, "ring")
    assert len(want["err"]) > 50 and (want["ref"] >= 64).sum() > 20 and (want["cand"][:, 3] >= 64).sum() > 20


def test_two_runs_and_no_shared_state(pkg, sphere, orc):
    """score on the main stream, the match on a side stream, score again: both
    scores are the oracle's, both matches the restatement's, bit for bit."""
    import torch
    s, p = sphere, sd.planted(pkg)
    want = sd.planted_match(pkg, 1.5)
    c, ref = want["c"][:3000], want["ref"][:3000]
    side = torch.cuda.Stream(torch.device("cuda:0"))
    first = s.ctx.score(c, ref, 0.7, 5)
    got, tot = gpu_match(s, p["feat"], p["feat_off"], p["pairs"], 1.5, 1e-4, stream=side)
    again = s.ctx.score(c, ref, 0.7, 5)
    got2, tot2 = gpu_match(s, p["feat"], p["feat_off"], p["pairs"], 1.5, 1e-4, stream=side)
    ws = orc.Scene(s.rgb, s.K, s.R, s.t_raw).score_batch(c, ref, 0.7, 5)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    for x, w in zip(first[:3], ws[:3]):
        assert np.array_equal(x, w)
    assert np.allclose(first[3], ws[3], rtol=0, atol=1e-12)
    assert tot == tot2 == len(want["err"])
    same(got, want, "first")
    same(got2, want, "second")


def test_arguments(pkg, sphere):
    s = sphere
    lib = pkg._lib.load()
    h = s.ctx.handle
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails its checks
    V = s.V
    off_ok = np.arange(V + 1, dtype=np.int64)
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)

    def call(dev=True, off=off_ok, pairs=((0, 1),), np_=None, epi=1.5, ms=1e-4, cap=4, feat=one, out=one, total=one):
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pr) if np_ is None else np_
        o = off.ctypes.data_as(i64p) if off is not None else None
        q = pr.ctypes.data_as(i32p) if pairs is not None else None
        if dev:
            return lib.mvs_wseed_match_device(h, feat, o, n, q, epi, ms, cap, out, out, out, out, out, total, None)
        cast = (lambda t: ctypes.cast(out, t) if out is not None else None)
        return lib.mvs_wseed_match(h, ctypes.cast(feat, i32p) if feat is not None else None, o, n, q, epi, ms, cap,
                                   cast(ctypes.POINTER(ctypes.c_double)), cast(ctypes.POINTER(ctypes.c_double)),
                                   cast(i32p), cast(i32p), cast(ctypes.POINTER(ctypes.c_double)),
                                   ctypes.cast(total, i64p) if total is not None else None)

    dec = off_ok.copy()
    dec[5] = 2
    for dev in (True, False):
        for bad, msg in ((dict(pairs=((3, 3),)), "with itself"), (dict(pairs=((0, V),)), "out of range"),
                         (dict(pairs=((-1, 2),)), "out of range"), (dict(off=dec), "decreases"),
                         (dict(off=off_ok + 1), "feat_off[0]"), (dict(epi=0.0), "epi_px"),
                         (dict(epi=float("inf")), "epi_px"), (dict(epi=float("nan")), "epi_px"),
                         (dict(ms=-0.1), "min_sin2"), (dict(ms=1.0), "min_sin2"), (dict(ms=float("nan")), "min_sin2"),
                         (dict(cap=-1), "cap < 0"), (dict(np_=-1), "np < 0"), (dict(off=None), "null pointer"),
                         (dict(feat=None), "null pointer"), (dict(total=None), "null pointer"),
                         (dict(out=None), "null pointer")):
            assert call(dev=dev, **bad) == -1, (dev, bad)            # MVS_E_ARG
            assert msg in pkg._lib.last_error(h), (msg, pkg._lib.last_error(h))
        # nothing to do: MVS_OK before any pointer is looked at
        assert call(dev=dev, np_=0, off=None, feat=None, out=None, total=None) == 0
        assert call(dev=dev, off=np.zeros(V + 1, np.int64), feat=None, out=None, total=None) == 0
    with pytest.raises(RuntimeError, match="V \\+ 1"):
        s.ctx.wseed_match(np.zeros((4, 2), np.int32), np.arange(V, dtype=np.int64), [(0, 1)])
    c, nrm, ref, cand, err, tot = s.ctx.wseed_match(np.zeros((0, 2), np.int32), np.zeros(V + 1, np.int64), [(0, 1)])
    assert tot == 0 and len(ref) == 0
    assert lib.mvs_wpatch_color_device(h, -1, one, one, one, one, one, None) == -1
    assert "n < 0" in pkg._lib.last_error(h)
    assert lib.mvs_wpatch_color_device(h, 1, one, None, one, one, one, None) == -1
    assert "null pointer" in pkg._lib.last_error(h)
    assert lib.mvs_wpatch_color_device(h, 0, None, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------
# 2. the colour call
# ---------------------------------------------------------------------------
def gpu_color(s, c, ref, mask):
    """mvs_wpatch_color_device on outputs pre-filled with a canary pattern."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tc = _dev(np.asarray(c, np.float64).reshape(n, 3))
        tr = _dev(np.asarray(ref, np.int32))
        tm = _dev(np.asarray(mask, np.uint64).reshape(n, s.ctx.words))
        color = torch.full((n + 2, 3), -77.0, dtype=torch.float64, device=dev)
        nv = torch.full((n + 2,), -77, dtype=torch.int32, device=dev)
        s.ctx.wpatch_color_device(tc, tr, tm, color[:n], nv[:n], stream=st.cuda_stream)
        color, nv = color.cpu().numpy(), nv.cpu().numpy()
    st.synchronize()
    assert np.all(color[n:] == -77) and np.all(nv[n:] == -77)
    return color[:n], nv[:n]


def compare_color(s, c, ref, mask, label=""):
    want = sd.color(s.rgb, s.K, s.Rp, s.t, c, ref, mask)
    got = gpu_color(s, c, ref, mask)
    assert got[0].tobytes() == want[0].tobytes(), (label, "color")
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), (label, "nviews")
    return want


def test_color_of_true_candidates(pkg, sphere):
    s, p = sphere, sd.planted(pkg)
    m = sd.planted_match(pkg, 1.5)
    rows = np.flatnonzero(sd.true_rows(p, m))[::5]
    c, nrm, ref = m["c"][rows], m["nrm"][rows], m["ref"][rows]
    _, mask, count, _ = s.ctx.score_warped(c, nrm, ref, 0.7, 5, 0.3)
    assert (count >= 2).mean() > 0.5
    color, nv = compare_color(s, c, ref, mask, "true candidates")
    assert np.array_equal(nv, count + 1)                  # every passing view sees the centre, and so does ref
    host = s.ctx.wpatch_color(c, ref, mask)
    assert host[0].tobytes() == color.tobytes() and np.array_equal(host[1], nv)
    # the sphere's texture: green = 0.9 red, blue = 0.8 red, up to the bytes' truncation
    lit = color[:, 0] > 40
    assert lit.mean() > 0.9 and np.all(np.abs(color[lit, 1] - 0.9 * color[lit, 0]) < 1.5)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_color_sizes(pkg, sphere, n):
    s = sphere
    m = sd.planted_match(pkg, 1.5)
    rng = np.random.default_rng(50 + n)
    rows = rng.choice(len(m["ref"]), n, replace=False)
    mask = random_masks(rng, n, s.V, 0.3)
    _, nv = compare_color(s, m["c"][rows], m["ref"][rows], mask, f"n {n}")
    assert len(nv) == n and (n < 5 or nv.max() > 2)


def test_color_special_rows(sphere, ring):
    """A mask bit >= V, a ref outside 0..V-1, a patch outside every view (m = 0),
    a nan centre; the 80-view ring takes the loop over the groups twice."""
    s = sphere
    rng = np.random.default_rng(5)
    n = 12
    c = rng.uniform(-0.015, 0.015, (n, 3))
    ref = rng.integers(0, s.V, n).astype(np.int32)
    mask = random_masks(rng, n, s.V, 0.4)
    mask[::2, 0] |= np.uint64(0xFF) << np.uint64(40)          # bits >= V name no view
    ref[3], ref[4] = -1, s.V
    c[5] = (5.0, 5.0, 5.0)
    c[6] = np.nan
    mask[7] = 0
    color, nv = compare_color(s, c, ref, mask, "special rows")
    assert nv[5] == 0 and nv[6] == 0 and not color[5].any() and not color[6].any() and nv[7] == 1 and nv.max() > 3
    r = ring
    n = 40
    c = rng.uniform(-0.01, 0.01, (n, 3))
    ref = rng.integers(0, 80, n).astype(np.int32)
    mask = random_masks(rng, n, 80, 0.5)
    mask[::3, 1] |= np.uint64(0xFFFF) << np.uint64(16)
    _, nv = compare_color(r, c, ref, mask, "ring")
    assert nv.max() > 20


# ---------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------
def write_pars(path, K, R, t):
    with open(path, "w") as f:
        f.write(f"{len(K)}\n")
        for v in range(len(K)):
            vals = list(np.asarray(K[v]).reshape(9)) + list(np.asarray(R[v]).reshape(9)) + list(np.asarray(t[v]).reshape(3))
            f.write(f"v{v:04d}.png " + " ".join(repr(float(x)) for x in vals) + "\n")


def test_dense_points_warped(pkg, sphere, tmp_path, capsys):
    """MVS2.DensePointsWarped on the sphere with the planted features and ring
    pairs, two rounds and one iteration, twice.

    The restatements' own chain on the same inputs (seed_reference.match ->
    loop_reference.reconstruct with expand_reference.score_batch_fast, one
    iteration, two rounds; run on the CPU, 16 s) gives 8,374 patches from 11,550
    before the filter, 1,730 of them from round 0: 94.24 % of them within 5 % of
    the radius of the surface, mean dot of the normals with the sphere's 0.7602
    (the seeds' normals point at their reference cameras and nothing refines
    them here).  The GPU chain agrees with the restatement's on at least 98 % of
    its patches; if the other 2 % were all as bad as can be, the
    share would fall by 0.02 and the mean dot by 0.02 (1 + 0.7602): the bounds
    below."""
    s, p = sphere, sd.planted(pkg)
    par = str(tmp_path / "par.txt")
    write_pars(par, p["K"], p["R"], p["t_raw"])
    args = types.SimpleNamespace(par_path=par)
    imgs = [p["rgb"][v] for v in range(s.V)]
    runs = []
    for k in range(2):
        out = pkg.DensePointsWarped(imgs, args, rounds=2, iterations=1, epi_px=1.5, feats=p["feats"],
                                    pairs=p["pairs"], path=str(tmp_path / f"cloud{k}"))
        runs.append(out)
    a, b = runs
    for k in ("points", "normals", "colors"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counts"]["candidates"] == 52822 and a["counts"]["features"] == len(p["feat"])
    assert a["counts"]["tests"] == sum(len(p["feats"][r]) * len(p["feats"][v]) for r, v in p["pairs"])
    ps = a["patches"]
    n = len(ps["ref"])
    assert n == a["counts"]["patches"][-1] and len(a["counts"]["patches"]) == 2
    keys = set(zip(ps["ref"].tolist(), map(tuple, ps["cell"].tolist())))
    assert len(keys) == n                                               # one patch per (ref, cell)
    pts, nrm, col = pkg.read_ply_oriented(str(tmp_path / "cloud0.ply"))
    assert pts.tobytes() == a["points"].tobytes() and nrm.tobytes() == a["normals"].tobytes()
    assert col.tobytes() == a["colors"].tobytes()
    want_col, want_nv = sd.color(s.rgb, s.K, s.Rp, s.t, ps["c"][::20], ps["ref"][::20], ps["mask"][::20])
    assert a["colors"][::20].tobytes() == want_col.tobytes() and np.array_equal(a["nviews"][::20], want_nv)
    r = np.linalg.norm(a["points"], axis=1)
    within = float((np.abs(r - p["rad"]) <= 0.05 * p["rad"]).mean())
    dot = float(((a["points"] / r[:, None]) * a["normals"]).sum(1).mean())
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("warped:")]
    print(f"{n} patches (restatement 8,374), round-0 winners {a['counts']['winners0']}, {int((ps['round'] == 0).sum())} of them kept (1,730), within 5 % {within:.4f} "
          f"(0.9424), mean normal dot {dot:.4f} (0.7602)")
    assert len(line) == 2 and "round-0 winners" in line[0]
    assert within >= 0.9424 - 0.02
    assert dot >= 0.7602 - 0.02 * 1.7602
