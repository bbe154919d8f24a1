"""mvs_refine_lists (k_refine_lists): the refinement's view lists and depth
steps built on the device, against the numpy restatements that stay in the
wrapper -- MvsContext.refine_view_lists and MvsContext.refine_depth_steps.

Comparison rule: there is no tolerance.  Every list row equals the numpy
rule's row, and every depth step has the numpy step's bits (view(uint64))
unless both are nan.  No row is left out.

Sizes: one wave per row, four rows per workgroup (n around 4 and 256 * 4 + 1);
lane = view, one key per lane and group of 64 views (V = 64, 65, 80 and 256: a
full group, one view past it, a partial second group, four groups; V = 129,
192 and 193: the three-group instantiation, partial and full, and one view into
the fourth group; V = 1 and 2 lie below every max_views).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import warped_reference as wr
from conftest import PKG_NAME, REPO

pytestmark = pytest.mark.gpu

RAD = 0.02
I_CANARY = -77
D_CANARY = 7.25


def _context(pkg, rgb, K, R, t):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return pkg.MvsContext(rgb, K, R, t, device=0)


class Scene:
    def __init__(self, pkg, rgb, K, R, t):
        self.ctx = _context(pkg, rgb, K, R, t)
        self.K, self.R, self.t = K, R, np.asarray(t, np.float64).reshape(-1, 3)
        self.Rp = self.ctx.rproj()
        self.V = self.ctx.V
        self.O = -np.einsum("vji,vj->vi", self.Rp, self.t)


@pytest.fixture(scope="module")
def sphere(pkg):
    rgb, K, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]
    s = Scene(pkg, rgb, K, R, t)
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def ring80(pkg):
    rgb, K, R, t = pkg.synthetic.ring_scene(V=80, H=16, W=16)
    s = Scene(pkg, rgb, K, R, t)
    yield s
    s.ctx.close()


# ---------------------------------------------------------------------------
# the yardstick and the two ways to call the library
# ---------------------------------------------------------------------------
def expected(ctx, ncc, c, ref, sel, min_ncc, mv, depth_px):
    """The numpy rule on the source rows; an entry of sel outside 0..rows-1 gives
    an all -1 list and nan, a ref outside 0..V-1 gives nan (the device call)."""
    rows = len(ncc)
    src = np.arange(rows) if sel is None else np.asarray(sel, np.int64)
    ok = (src >= 0) & (src < rows)
    views = np.full((len(src), mv), -1, np.int32)
    views[ok] = ctx.refine_view_lists(ncc[src[ok]], min_ncc, mv)
    if c is None:
        return views, None
    dstep = np.full(len(src), np.nan)
    okr = ok.copy()
    okr[ok] = (ref[src[ok]] >= 0) & (ref[src[ok]] < ctx.V)
    with np.errstate(invalid="ignore", over="ignore"):
        dstep[okr] = ctx.refine_depth_steps(c[src[okr]], ref[src[okr]], depth_px)
    return views, dstep


def same_steps(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return got.shape == want.shape and bool(np.all(both_nan | (got.view(np.uint64) == want.view(np.uint64))))


def run_device(ctx, ncc, c, ref, sel, min_ncc, mv, depth_px, stream=None):
    """refine_lists_device on fresh tensors, outputs with one canary row past n."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ncc) if sel is None else len(sel)
    t_ncc = torch.from_numpy(np.ascontiguousarray(ncc)).to(dev)
    t_c = torch.from_numpy(np.ascontiguousarray(c)).to(dev) if c is not None else None
    t_ref = torch.from_numpy(np.ascontiguousarray(ref, np.int32)).to(dev) if c is not None else None
    t_sel = torch.from_numpy(np.ascontiguousarray(sel, np.int64)).to(dev) if sel is not None else None
    views = torch.full((n + 1, mv), I_CANARY, dtype=torch.int32, device=dev)
    dstep = torch.full((n + 1,), D_CANARY, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.refine_lists_device(t_ncc, t_c, t_ref, views[:n], dstep[:n] if c is not None else None, t_sel, min_ncc, mv,
                            depth_px, stream=stream)
    torch.cuda.synchronize()
    views, dstep = views.cpu().numpy(), dstep.cpu().numpy()
    assert np.all(views[n] == I_CANARY) and dstep[n] == D_CANARY, "the row past n was written"
    if c is None:
        assert np.all(dstep == D_CANARY)
        return views[:n], None
    return views[:n], dstep[:n]


def check_device(ctx, ncc, c, ref, sel, min_ncc, mv, depth_px, label):
    views, dstep = run_device(ctx, ncc, c, ref, sel, min_ncc, mv, depth_px)
    wv, wd = expected(ctx, ncc, c, ref, sel, min_ncc, mv, depth_px)
    assert views.dtype == np.int32 and views.shape == wv.shape, label
    bad = np.flatnonzero((views != wv).any(1))
    assert len(bad) == 0, (label, bad[:5], views[bad[:1]], wv[bad[:1]])
    if c is not None:
        assert same_steps(dstep, wd), (label, dstep[:4], wd[:4])
    return views, dstep


# ---------------------------------------------------------------------------
# 1. the rule on crafted ncc
# ---------------------------------------------------------------------------
def crafted_ncc(V, n=40, seed=0):
    """Multiples of 1/8 in [-1, 1] (ties across the max_views cut, across the
    groups of 64 and on the thresholds 0.5 and -0.5), 20 % nan, -0.0 for about
    half of the zeros and more, some +inf, an all-nan row, a row of all 1.0."""
    rng = np.random.default_rng(100 + V + seed)
    ncc = rng.integers(-8, 9, (n, V)) / 8.0
    ncc[(ncc == 0) & (rng.random((n, V)) < 0.5)] = -0.0
    ncc[rng.random((n, V)) < 0.04] = -0.0
    ncc[rng.random((n, V)) < 0.04] = 0.0
    ncc[rng.random((n, V)) < 0.03] = np.inf
    ncc[rng.random((n, V)) < 0.20] = np.nan
    ncc[n - 2] = np.nan
    ncc[n - 1] = 1.0
    return ncc


@pytest.mark.parametrize("V", [1, 2, 24, 64, 65, 80, 129, 192, 193, 256])
def test_rule_on_crafted_ncc(pkg, sphere, V):
    if V == 24:
        s, own = sphere, False
    else:
        s, own = Scene(pkg, *pkg.synthetic.ring_scene(V=V, H=16, W=16)), True
    try:
        ncc = crafted_ncc(V)
        if V >= 24:
            assert np.signbit(ncc[ncc == 0]).any() and (~np.signbit(ncc[ncc == 0])).any() and np.isinf(ncc).any()
            assert 0.1 < np.isnan(ncc[:-2]).mean() < 0.3
        rng = np.random.default_rng(V)
        ref = rng.integers(0, V, len(ncc)).astype(np.int32)
        c = rng.uniform(-0.01, 0.01, (len(ncc), 3))
        full = cut = 0
        for mv in (1, 3, 8, 32):
            for min_ncc in (0.7, 0.5, -0.5):
                views, _ = check_device(s.ctx, ncc, c, ref, None, min_ncc, mv, 1.5, f"V {V} mv {mv} thr {min_ncc}")
                assert np.all(views[-2] == -1)                                  # the all-nan row
                assert np.array_equal(views[-1][:min(mv, V)], np.arange(min(mv, V)))   # all 1.0: the lowest views
                full += int((views >= 0).all(1).sum())
                with np.errstate(invalid="ignore"):
                    cut += int(((ncc > min_ncc).sum(1) > mv).sum())
        print(f"V {V}: {full} full lists, {cut} rows with more passing views than max_views")
        if V >= 24:
            assert full > 100 and cut > 100
    finally:
        if own:
            s.ctx.close()


# ---------------------------------------------------------------------------
# 2. sizes and selection
# ---------------------------------------------------------------------------
def sphere_rows(s, rows, seed):
    rng = np.random.default_rng(seed)
    ncc = crafted_ncc(s.V, rows, seed)
    ref = rng.integers(0, s.V, rows).astype(np.int32)
    c = rng.uniform(-RAD, RAD, (rows, 3))
    return rng, ncc, c, ref


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257, 1025])
def test_sizes_and_selection(sphere, n):
    s = sphere
    rows = max(n, 2)
    rng, ncc, c, ref = sphere_rows(s, rows, n)
    # sel None: the first n rows of n
    check_device(s.ctx, ncc[:n], c[:n], ref[:n], None, 0.5, 8, 1.5, f"n {n} plain")
    # lists only
    check_device(s.ctx, ncc[:n], None, None, None, 0.5, 8, 1.5, f"n {n} lists only")
    if n == 0:
        check_device(s.ctx, ncc, c, ref, np.empty(0, np.int64), 0.5, 8, 1.5, "n 0 of 2 rows")
        return
    # a permutation, a strict subset with repeats, entries outside 0..rows-1
    check_device(s.ctx, ncc, c, ref, rng.permutation(rows)[:n], 0.5, 8, 1.5, f"n {n} permutation")
    sub = rng.integers(0, max(rows // 2, 1), n)
    sub[-1] = sub[0]
    check_device(s.ctx, ncc, c, ref, sub, 0.7, 3, 1.0, f"n {n} subset with repeats")
    out = rng.integers(0, rows, n)
    out[0] = -1
    out[-1] = rows
    out[n // 2] = rows if n > 2 else out[n // 2]
    views, dstep = check_device(s.ctx, ncc, c, ref, out, 0.5, 8, 1.5, f"n {n} sel outside")
    assert np.all(views[0] == -1) and np.isnan(dstep[0]) and np.all(views[-1] == -1) and np.isnan(dstep[-1])
    # a ref of -1 and V: nan, and the list still per the rule
    bad = ref.copy()
    bad[0], bad[-1] = -1, s.V
    views, dstep = check_device(s.ctx, ncc, c, bad, None, 0.5, 8, 1.5, f"n {n} bad ref")
    assert np.isnan(dstep[0]) and np.isnan(dstep[-1])
    assert np.array_equal(views, s.ctx.refine_view_lists(ncc, 0.5, 8))


# ---------------------------------------------------------------------------
# 3. depth steps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "ring80"])
def test_depth_steps(sphere, ring80, which):
    s = sphere if which == "sphere" else ring80
    rng = np.random.default_rng(5)
    n = 4 * s.V
    ref = (np.arange(n) % s.V).astype(np.int32)
    axis = s.Rp[ref, 2, :]                                  # the viewing direction of the reference camera
    z = np.repeat([0.33, 0.0, -0.2, 0.5], s.V)[:n]          # in front, on the camera plane, behind, (nan below)
    c = s.O[ref] + z[:, None] * axis + rng.uniform(-0.01, 0.01, (n, 3)) * (z != 0)[:, None]
    c[3 * s.V:, rng.integers(0, 3)] = np.nan
    ncc = crafted_ncc(s.V, n, 1)
    for depth_px in (1.0, 1.5):
        _, dstep = check_device(s.ctx, ncc, c, ref, None, 0.7, 8, depth_px, f"{which} depth_px {depth_px}")
        assert np.all(dstep[:s.V] > 0) and np.all(np.abs(dstep[s.V:2 * s.V]) < 1e-15)
        assert np.all(dstep[2 * s.V:3 * s.V] < 0) and np.all(np.isnan(dstep[3 * s.V:]))


# ---------------------------------------------------------------------------
# 4. the host pair, arguments
# ---------------------------------------------------------------------------
def test_host_pair_equals_device_pair(sphere, ring80):
    for s in (sphere, ring80):
        rng, ncc, c, ref = sphere_rows(s, 133, 9)
        for sel in (None, rng.integers(0, 133, 57)):
            for mv, thr, px in ((8, 0.7, 1.5), (32, -0.5, 1.0), (1, 0.5, 1.5)):
                dv, dd = run_device(s.ctx, ncc, c, ref, sel, thr, mv, px)
                hv, hd = s.ctx.refine_lists(ncc, c, ref, sel, thr, mv, px)
                assert hv.dtype == np.int32 and np.array_equal(hv, dv)
                assert hd.tobytes() == dd.tobytes()
                wv, wd = expected(s.ctx, ncc, c, ref, sel, thr, mv, px)
                assert np.array_equal(hv, wv) and same_steps(hd, wd)
        hv, hd = s.ctx.refine_lists(ncc)
        assert hd is None and np.array_equal(hv, s.ctx.refine_view_lists(ncc, 0.7, 8))
    e = sphere.ctx.refine_lists(np.empty((0, 24)), np.empty((0, 3)), np.empty(0, np.int32))
    assert e[0].shape == (0, 8) and e[1].shape == (0,)


def test_arguments(pkg, sphere):
    import torch
    s = sphere
    ctx = s.ctx
    _, ncc, c, ref = sphere_rows(s, 6, 2)
    ok = ctx.refine_lists(ncc, c, ref)
    assert ok[0].shape == (6, 8) and ok[1].shape == (6,)
    for kw, msg in (({"max_views": 0}, "max_views must be in 1..32"), ({"max_views": 33}, "max_views must be in 1..32"),
                    ({"min_ncc": np.nan}, "min_ncc is nan"), ({"depth_px": 0.0}, "depth_px must be finite and > 0"),
                    ({"depth_px": -1.0}, "depth_px must be finite and > 0"),
                    ({"depth_px": np.inf}, "depth_px must be finite and > 0"),
                    ({"depth_px": np.nan}, "depth_px must be finite and > 0")):
        with pytest.raises(RuntimeError, match=msg):
            ctx.refine_lists(ncc, c, ref, **kw)
        with pytest.raises(RuntimeError, match=msg):
            run_device(ctx, ncc, c, ref, None, kw.get("min_ncc", 0.7), kw.get("max_views", 8), kw.get("depth_px", 1.5))
    ctx.refine_lists(ncc, c, ref, min_ncc=-np.inf)      # allowed: every view that is not nan or -inf passes
    # host call: a sel entry outside 0..rows-1, a ref outside 0..V-1
    for bad in ([0, 6], [-1, 0]):
        with pytest.raises(RuntimeError, match="sel row out of range"):
            ctx.refine_lists(ncc, c, ref, np.array(bad))
    for bad in (-1, s.V):
        r2 = ref.copy()
        r2[3] = bad
        with pytest.raises(RuntimeError, match="ref view out of range"):
            ctx.refine_lists(ncc, c, r2)
        ctx.refine_lists(ncc, c, r2, np.array([0, 1, 2, 4, 5]))      # the bad row is not selected
        assert ctx.refine_lists(ncc)[1] is None                       # lists only: ref is not read
    # n > rows without sel
    dev = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="n > rows without sel"):
        ctx.refine_lists_device(torch.from_numpy(ncc).to(dev), None, None,
                                torch.empty((7, 8), dtype=torch.int32, device=dev), None)
    with pytest.raises(RuntimeError, match="contiguous"):
        ctx.refine_lists_device(torch.from_numpy(ncc).to(dev)[:, :8], None, None,
                                torch.empty((6, 8), dtype=torch.int32, device=dev), None)
    # the C entry points themselves: n < 0, rows < 0, NULL required pointers, n = 0
    lib = pkg._lib.load()
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    buf, ib, lb = np.zeros(6 * 24 + 64), np.zeros(64, np.int32), np.zeros(8, np.int64)
    ov, od = np.zeros(64, np.int32), np.zeros(8)                           # the host call's outputs
    P, I, L = buf.ctypes.data_as(dp), ib.ctypes.data_as(ip), lb.ctypes.data_as(lp)
    OV, OD = ov.ctypes.data_as(ip), od.ctypes.data_as(dp)

    def err():
        return lib.mvs_last_error(ctx._h).decode()

    def host(n=1, rows=1, sel=None, ncc_=P, c_=P, ref_=I, views=OV, dstep=OD):
        return lib.mvs_refine_lists(ctx._h, n, rows, sel, ncc_, c_, ref_, 0.7, 8, 1.5, views, dstep)

    def device(n=1, rows=1, sel=None, ncc_=1, c_=1, ref_=1, views=1, dstep=1):
        return lib.mvs_refine_lists_device(ctx._h, n, rows, sel, ncc_, c_, ref_, 0.7, 8, 1.5, views, dstep, None)

    for call in (host, device):
        assert call(n=-1) == -1 and "n < 0" in err()
        assert call(rows=-1) == -1 and "rows < 0" in err()
        assert call(n=2, rows=1) == -1 and "n > rows without sel" in err()
        for kw, msg in (({"n": -1}, "n < 0"), ({"rows": -1}, "rows < 0"), ({"n": 2, "rows": 1}, "n > rows without sel")):
            with pytest.raises(RuntimeError, match=msg):      # what the wrapper makes of the status
                pkg._lib.check(call(**kw), ctx._h, "mvs_refine_lists")
        for kw in ({"ncc_": None}, {"views": None}, {"c_": None}, {"ref_": None}):
            assert call(**kw) == -1 and "null pointer" in err(), kw
            with pytest.raises(RuntimeError, match="null pointer"):
                pkg._lib.check(call(**kw), ctx._h, "mvs_refine_lists")
        assert call(n=0, rows=0, ncc_=None, c_=None, ref_=None, views=None, dstep=None) == 0
    assert host(c_=None, ref_=None, dstep=None) == 0                      # lists only
    assert host(n=2, rows=1, sel=L) == 0                                   # with sel n may exceed rows
    assert np.all(ov[:16] == -1) and np.all(ov[16:] == 0) and od[0] == od[1] and np.all(od[2:] == 0)
    assert lib.mvs_refine_lists_device(None, 1, 1, None, 1, 1, 1, 0.7, 8, 1.5, 1, 1, None) == -1


# ---------------------------------------------------------------------------
# 5. on the scorer's own ncc
# ---------------------------------------------------------------------------
def test_on_the_scorers_ncc(pkg, dino):
    import torch
    rgb, K, R, t = dino
    ctx = _context(pkg, rgb, K, R, t)
    try:
        n, wid = 2048, 3
        c, ref = pkg.synthetic.candidates(n, K, R, t, seed=21)
        O = -np.einsum("vji,vj->vi", ctx.rproj(), np.asarray(t, np.float64).reshape(-1, 3))
        nrm = O[ref] - c
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        dev = torch.device("cuda:0")
        st = torch.cuda.Stream(dev)
        with torch.cuda.stream(st):
            tc, tn, tr = (torch.from_numpy(x).to(dev) for x in (c, nrm, ref))
            xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
            mask = torch.empty((n, ctx.words), dtype=torch.int64, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            ncc = torch.empty((n, ctx.V), dtype=torch.float64, device=dev)
            views = torch.empty((n, 8), dtype=torch.int32, device=dev)
            dstep = torch.empty(n, dtype=torch.float64, device=dev)
            ctx.score_warped_device(tc, tn, tr, xy, mask, count, None, ncc, 0.7, wid, 0.0, stream=st.cuda_stream)
            ctx.refine_lists_device(ncc, tc, tr, views, dstep, None, 0.7, 8, 1.5, stream=st.cuda_stream)
        st.synchronize()
        h_ncc = ncc.cpu().numpy()
        want = ctx.refine_view_lists(h_ncc, 0.7, 8)
        T = (want >= 0).sum(1)
        print(f"{int((T > 0).sum())} of {n} rows keep a list, {int((T == 8).sum())} full, mean |T| {T[T > 0].mean():.2f}")
        assert (T > 0).sum() > 200 and (T == 8).any()
        assert np.array_equal(views.cpu().numpy(), want)
        assert same_steps(dstep.cpu().numpy(), ctx.refine_depth_steps(c, ref, 1.5))
        # the wrapper's chain reports the device's lists: the rule on the host-pointer scorer's ncc
        host_ncc = ctx.score_warped(c, nrm, ref, 0.7, wid, 0.0, want_ncc=True)[4]
        assert host_ncc.tobytes() == h_ncc.tobytes()
        info = ctx.refine_warped(c, nrm, ref, wid=wid, levels=1)[3]
        assert info["views"].dtype == np.int32 and np.array_equal(info["views"], want)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 6. the chain
# ---------------------------------------------------------------------------
def test_chain_lists_and_steps(sphere):
    """expand_warped with the seeds and parameters of test_expand_gpu.py's
    gpu_chains fixture and two refinement levels, traced: what every round fed
    its level calls is the numpy rule on that round's own ncc, cc and cref at
    the winners; two runs are identical in every output array."""
    s = sphere
    c, nrm, ref, _ = wr.sphere_patches(s.K, s.R, s.t, 8, RAD, np.random.default_rng(1))
    kw = dict(cell_size=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2, refine_levels=2, trace=True)
    a = s.ctx.expand_warped(c, nrm, ref, 5, **kw)
    b = s.ctx.expand_warped(c, nrm, ref, 5, **kw)
    assert len(a["trace"]) == 5 and len(a["ref"]) > 1000
    for rnd, tr in enumerate(a["trace"]):
        wk = np.flatnonzero(tr["win"])
        assert len(wk) > 0
        assert tr["lists"].dtype == np.int32 and tr["lists"].shape == (len(wk), 8) and tr["dstep"].shape == (len(wk),)
        assert np.array_equal(tr["lists"], s.ctx.refine_view_lists(tr["ncc"][wk], 0.7, 8)), rnd
        assert same_steps(tr["dstep"], s.ctx.refine_depth_steps(tr["cc"][wk], tr["cref"][wk], 1.0)), rnd
        assert np.all(tr["dstep"] > 0)
        print(f"round {rnd}: {len(tr['win'])} jobs, {len(wk)} winners, mean |T| {(tr['lists'] >= 0).sum(1).mean():.2f}")

    def same(x, y, path):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), path
            for k in x:
                same(x[k], y[k], path + (k,))
        elif isinstance(x, list):
            assert len(x) == len(y), path
            for i, (p, q) in enumerate(zip(x, y)):
                same(p, q, path + (i,))
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), path
        else:
            assert x == y, path
    same(a, b, ())


# ---------------------------------------------------------------------------
# 7. interleaving with the tiled scorer
# ---------------------------------------------------------------------------
INTERLEAVE = r"""
import sys, numpy as np, importlib, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {golden!r})
from make_seeds import load_dino
pkg = importlib.import_module({pkg!r})
imgs, K, R, t = load_dino({data!r})
rgb = np.stack(imgs)
ctx = pkg.MvsContext(rgb, K, R, t, device=0)
c, ref = pkg.synthetic.candidates(4096, K, R, t, seed=11)
O = -np.einsum("vji,vj->vi", ctx.rproj(), t.reshape(-1, 3))
nrm = O[ref] - c
nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
m = 2048
ncc = ctx.score_warped(c[:m], nrm[:m], ref[:m], 0.7, 3, 0.3, want_ncc=True)[4]
sel = np.random.default_rng(0).integers(0, m, 1500)
want_v = ctx.refine_view_lists(ncc[sel], 0.7, 8)
want_d = ctx.refine_depth_steps(c[:m][sel], ref[:m][sel], 1.5)
assert int((want_v >= 0).any(1).sum()) > 100
dev = torch.device("cuda:0")
tc, tr = torch.from_numpy(c).to(dev), torch.from_numpy(ref).to(dev)
lc, lr, ln, ls = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (c[:m], ref[:m], ncc, sel))
side = torch.cuda.Stream(dev)
torch.cuda.synchronize()
n = len(ref)
def rec_batch():
    xy = torch.empty((n, 2), dtype=torch.float64, device=dev)
    rec = torch.empty((n, ctx.words + 1), dtype=torch.int64, device=dev)
    ctx.score_device_rec(tc, tr, xy, rec, 0.7, 5)
    return xy, rec
def lists():
    with torch.cuda.stream(side):
        v = torch.empty((len(sel), 8), dtype=torch.int32, device=dev)
        d = torch.empty(len(sel), dtype=torch.float64, device=dev)
        ctx.refine_lists_device(ln, lc, lr, v, d, ls, 0.7, 8, 1.5, stream=side.cuda_stream)
    return v, d
first = rec_batch()
alone = lists()
torch.cuda.synchronize()
a = rec_batch(); la = lists(); b = rec_batch(); lb = lists(); cc = rec_batch(); lc_ = lists()
torch.cuda.synchronize()
assert ctx.scorer_stats()["batches"] == 4, ctx.scorer_stats()
for got in (a, b, cc):
    assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
for v, d in (alone, la, lb, lc_):
    assert np.array_equal(v.cpu().numpy(), want_v)
    assert d.cpu().numpy().tobytes() == want_d.tobytes()
ctx.close()
print("interleaved ok", flush=True)
"""


def test_interleaved_with_tiled_scorer():
    """refine_lists_device on a side stream between score_device_rec batches of
    the tiled scorer (MVS_SCORE_KERNEL=tiled) on the context's stream, in a
    fresh process: the call keeps no state and uses none of the scorer's
    scratch or counter sets, so both results stay what they are alone."""
    code = INTERLEAVE.format(repo=REPO, golden=os.path.join(REPO, "tests", "golden"), pkg=PKG_NAME,
                             data=os.path.join(REPO, "data", "dinoRing"))
    env = dict(os.environ, MVS_SCORE_KERNEL="tiled")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode == 0 and "interleaved ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
