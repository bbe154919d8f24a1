"""The warped expansion on the GPU (k_wexp_children, k_wexp_scan, k_wexp_claim_*,
k_wexp_mark and MvsContext.expand_warped) against the float64 restatement
(tests/expand_reference.py).

Every decision of the three primitives is discrete and is compared exactly with
the restatement fed the same inputs.  A child's centre X = O_v + s d is compared
within 1e-13 |c_p - O_v| (1 + 1 / |cos|), cos the cosine between the parent's
normal and the cell centre's ray: a dozen binary64 operations, scaled by the
ray-plane conditioning (both sides take the products and sums in the same
order, so the difference is 0 as a rule).  The photo scores of the composition
tests follow tests/test_warped_gpu.py's rule.

Sizes: k_wexp_children puts 4 patches in a workgroup and k_wexp_scan is one
workgroup of 1024 threads (n = 1025: two counts per thread); the claim's
kernels run 256 jobs per workgroup.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import expand_reference as er
import warped_reference as wr
from conftest import PKG_NAME, REPO
from test_warped_gpu import check_against_reference, toward_camera

pytestmark = pytest.mark.gpu

RAD = 0.02
CANARY = 8            # rows kept past cap, which the call must leave alone


def _context(pkg, rgb, K, R, t):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return pkg.MvsContext(rgb, K, R, t, device=0)


class Scene:
    def __init__(self, pkg, rgb, K, R, t):
        self.ctx = _context(pkg, rgb, K, R, t)
        self.gray = wr.gray_stack(rgb)
        self.K, self.R, self.t = K, R, np.asarray(t, np.float64).reshape(-1, 3)
        self.Rp = self.ctx.rproj()
        self.V, self.H, self.W = self.ctx.V, self.ctx.H, self.ctx.W
        self.O = np.array([er.centre_of([float(x) for x in self.Rp[v].reshape(9)], [float(x) for x in self.t[v]])
                           for v in range(self.V)])


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


def random_masks(rng, n, V, p=0.4):
    words = (V + 63) // 64
    mask = np.zeros((n, words), np.uint64)
    bits = rng.random((n, V)) < p
    for v in range(V):
        mask[:, v >> 6] |= bits[:, v].astype(np.uint64) << np.uint64(v & 63)
    return mask


def occupancy(kind, rng, V, ncj, nci):
    if kind == "vacant":
        return np.zeros((V, ncj, nci), np.uint8)
    if kind == "taken":
        return np.full((V, ncj, nci), 3, np.uint8)
    return (rng.random((V, ncj, nci)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (V, ncj, nci)).astype(np.uint8)


def gpu_children(s, c, nrm, ref, mask, cell, occ, max_dist, cap):
    """mvs_wexp_children_device with CANARY rows past cap -> jobs, cc, cn, cref (first min(total, cap)), total."""
    import torch
    dev = torch.device("cuda:0")
    ctx = s.ctx
    n = len(ref)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        tc = torch.from_numpy(np.ascontiguousarray(c, np.float64).reshape(n, 3)).to(dev)
        tn = torch.from_numpy(np.ascontiguousarray(nrm, np.float64).reshape(n, 3)).to(dev)
        tr = torch.from_numpy(np.ascontiguousarray(ref, np.int32)).to(dev)
        tm = torch.from_numpy(np.ascontiguousarray(mask, np.uint64).view(np.int64).reshape(n, ctx.words)).to(dev)
        to = torch.from_numpy(np.ascontiguousarray(occ)).to(dev)
        job = torch.full((cap + CANARY, 4), -77, dtype=torch.int32, device=dev)
        cc = torch.full((cap + CANARY, 3), -77.0, dtype=torch.float64, device=dev)
        cn = torch.full((cap + CANARY, 3), -77.0, dtype=torch.float64, device=dev)
        cref = torch.full((cap + CANARY,), -77, dtype=torch.int32, device=dev)
        total = torch.full((1,), -77, dtype=torch.int64, device=dev)
        ctx.wexp_children_device(tc, tn, tr, tm, cell, to, max_dist, job[:cap], cc[:cap], cn[:cap], cref[:cap], total,
                                 stream=st.cuda_stream)
        out = [x.cpu().numpy() for x in (job, cc, cn, cref, total)]
    st.synchronize()
    job, cc, cn, cref, total = out
    tot = int(total[0])
    k = min(tot, cap)
    assert np.all(job[cap:] == -77) and np.all(cc[cap:] == -77.0) and np.all(cn[cap:] == -77.0) \
        and np.all(cref[cap:] == -77), "written past cap"
    assert np.all(job[k:] == -77) and np.all(cref[k:] == -77), "written past the total"
    return job[:k], cc[:k], cn[:k], cref[:k], tot


def compare_children(s, c, nrm, ref, mask, cell, occ, max_dist, cap=None, label=""):
    want = er.children(s.K, s.Rp, s.t, s.W, s.H, c, nrm, ref, mask, cell, occ, max_dist)
    m = len(want[0])
    cap = m + 5 if cap is None else cap
    jobs, cc, cn, cref, tot = gpu_children(s, c, nrm, ref, mask, cell, occ, max_dist, cap)
    assert tot == m, (tot, m)
    k = min(m, cap)
    assert np.array_equal(jobs, want[0][:k])
    assert np.array_equal(cref, want[3][:k])
    assert cn.tobytes() == want[2][:k].tobytes()
    worst = 0.0
    if k:
        p, v = jobs[:, 0], jobs[:, 1]
        cp, n = np.asarray(c, np.float64).reshape(-1, 3)[p], np.asarray(nrm, np.float64).reshape(-1, 3)[p]
        d = cc - s.O[v]
        cos = np.abs((d * n).sum(1)) / np.sqrt((d * d).sum(1)) / np.sqrt((n * n).sum(1))
        tol = 1e-13 * np.sqrt(((cp - s.O[v]) ** 2).sum(1)) * (1 + 1 / cos)
        err = np.sqrt(((cc - want[1][:k]) ** 2).sum(1))
        worst = float((err / tol).max())
        assert np.all(err <= tol)
    print(f"{label}: n {len(ref)}, {m} jobs, cap {cap}, {int((cc != want[1][:k]).any(1).sum()) if k else 0} centres "
          f"differ in a bit, worst {worst:.3f} of the tolerance")
    return want


def sphere_frontier(s, n, seed):
    rng = np.random.default_rng(seed)
    c, nrm, ref, _ = wr.sphere_patches(s.K, s.R, s.t, n, RAD, rng)
    return rng, c, nrm, ref, random_masks(rng, n, s.V)


# ---------------------------------------------------------------------------
# 1. children
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["vacant", "random", "taken"])
def test_children_sphere(sphere, cell, kind):
    s = sphere
    rng, c, nrm, ref, mask = sphere_frontier(s, 37, 10 + cell)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    occ = occupancy(kind, rng, s.V, ncj, nci)
    want = compare_children(s, c, nrm, ref, mask, cell, occ, 1.0, label=f"sphere cell {cell} {kind}")
    if kind == "taken":
        assert len(want[0]) == 0
    else:
        assert len(want[0]) > 37
    if cell == 3:
        assert nci * 3 < s.W and (len(want[0]) == 0 or want[0][:, 2].max() < nci)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])
def test_children_sizes(sphere, n):
    s = sphere
    rng, c, nrm, ref, mask = sphere_frontier(s, n, 100 + n)
    nci, ncj = er.grid_shape(s.W, s.H, 2)
    occ = occupancy("random", rng, s.V, ncj, nci)
    compare_children(s, c, nrm, ref, mask, 2, occ, 1.0, label=f"sizes n {n}")


def test_children_special_patches_and_max_dist(sphere):
    s = sphere
    rng, c, nrm, ref, mask = sphere_frontier(s, 24, 5)
    O = s.O
    # 0: behind the camera of mask view 3 (the cameras look at the origin)
    c[0] = O[3] * 1.2
    mask[0, 0] |= np.uint64(1 << 3)
    # 1: projects outside every image
    c[1] = np.array([0.4, 0.3, 0.2])
    # 2: grazing -- the normal is perpendicular to the reference ray: s is 0/0, huge or negative
    ray = c[2] - O[ref[2]]
    g = np.cross(ray, [0.0, 0.0, 1.0])
    nrm[2] = g / np.linalg.norm(g)
    # 3: the normal points away from the cameras (s keeps its sign: the plane is the same)
    nrm[3] = -nrm[3]
    # 4: nearly grazing, tilted so that some neighbours' rays meet the plane behind the camera
    ray = (c[4] - O[ref[4]]) / np.linalg.norm(c[4] - O[ref[4]])
    g = np.cross(ray, [0.0, 0.0, 1.0])
    nrm[4] = g / np.linalg.norm(g) + 1e-3 * ray
    nrm[4] /= np.linalg.norm(nrm[4])
    # 5: a reference view outside 0..V-1 and 6: no mask at all
    ref[5] = 99
    mask[6] = 0
    nci, ncj = er.grid_shape(s.W, s.H, 2)
    occ = np.zeros((s.V, ncj, nci), np.uint8)
    wide = compare_children(s, c, nrm, ref, mask, 2, occ, 1e9, label="special, no cut")
    per = np.bincount(wide[0][:, 0], minlength=24)
    assert per[1] == 0 and per[6] <= 4 and per[3] > 0
    # max_dist between two children's distances: about half of them are cut
    dist = np.sort(np.sqrt(((wide[1] - c[wide[0][:, 0]]) ** 2).sum(1)))
    k = len(dist) // 2
    while dist[k + 1] - dist[k] <= 1e-9 * dist[k]:
        k += 1
    cut = compare_children(s, c, nrm, ref, mask, 2, occ, 0.5 * (dist[k] + dist[k + 1]), label="special, cut")
    assert len(cut[0]) == k + 1 < len(wide[0])


@pytest.mark.parametrize("cap", [0, 1, 100])
def test_children_cap_below_the_total(sphere, cap):
    s = sphere
    rng, c, nrm, ref, mask = sphere_frontier(s, 9, 21)
    nci, ncj = er.grid_shape(s.W, s.H, 2)
    want = compare_children(s, c, nrm, ref, mask, 2, np.zeros((s.V, ncj, nci), np.uint8), 1.0, cap=cap,
                            label=f"cap {cap}")
    assert len(want[0]) > 100


@pytest.mark.parametrize("cell", [1, 2, 3])
def test_children_more_than_64_views(ring, cell):
    s = ring
    rng = np.random.default_rng(4)
    n = 41
    c = rng.uniform(-0.005, 0.005, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, 80, n).astype(np.int32)
    nrm = toward_camera(s.Rp, s.t, c, ref)
    mask = random_masks(rng, n, 80, 0.3)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    occ = occupancy("random", rng, s.V, ncj, nci)
    want = compare_children(s, c, nrm, ref, mask, cell, occ, 1.0, label=f"ring V=80 cell {cell}")
    assert (want[0][:, 1] >= 64).any() and (want[0][:, 1] < 64).any()


# ---------------------------------------------------------------------------
# 2. claim
# ---------------------------------------------------------------------------
def crafted_jobs(rng, m, V, nci, ncj, cells=40):
    """m jobs on a few cells (the grid's corners among them) with many exact
    ties, both zeros, nan, inf and refused jobs."""
    pool = np.column_stack([rng.integers(0, V, cells), rng.integers(0, nci, cells), rng.integers(0, ncj, cells)])
    pool[:4] = [[0, 0, 0], [V - 1, nci - 1, ncj - 1], [0, nci - 1, 0], [V - 1, 0, ncj - 1]]
    pick = rng.integers(0, cells, m)
    jobs = np.column_stack([rng.integers(-1, 50, m), pool[pick]]).astype(np.int32)
    values = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 0.75, -0.25, np.nan, np.inf, -np.inf, 0.9, 0.9, 1.0 - 2.0 ** -53])
    score = values[rng.integers(0, len(values), m)]
    accept = (rng.random(m) < 0.8).astype(np.uint8) * rng.integers(1, 256, m).astype(np.uint8)
    return jobs, accept, score


@pytest.mark.parametrize("m", [0, 1, 2, 255, 256, 257, 4097])
def test_claim_sizes(sphere, m):
    s = sphere
    nci, ncj = s.ctx.cell_grid(2)
    jobs, accept, score = crafted_jobs(np.random.default_rng(m), m, s.V, nci, ncj)
    win = s.ctx.wexp_claim(jobs, accept, score, nci, ncj)
    want = er.claim(jobs, accept, score, s.V, nci, ncj)
    assert win.dtype == np.uint8 and np.array_equal(win, want)
    if m >= 255:
        assert 4 <= want.sum() <= 40


def test_claim_one_cell_and_clean_scratch(sphere):
    """All 4097 jobs on one cell; then two unrelated job sets in a row on the
    same context, nothing marked in between: the second result is the
    restatement's, so the first call left its cells clean."""
    s = sphere
    nci, ncj = s.ctx.cell_grid(2)
    rng = np.random.default_rng(9)
    m = 4097
    jobs = np.tile(np.array([[0, 5, nci - 1, ncj - 1]], np.int32), (m, 1))
    score = rng.integers(0, 64, m) / 64.0                 # many exact ties at the maximum
    accept = np.ones(m, np.uint8)
    accept[int(np.argmax(score))] = 0                     # the first maximum is refused
    win = s.ctx.wexp_claim(jobs, accept, score, nci, ncj)
    want = er.claim(jobs, accept, score, s.V, nci, ncj)
    assert want.sum() == 1 and np.array_equal(win, want)
    # the same cells again with lower scores: a stale key or ticket would refuse every job
    low = s.ctx.wexp_claim(jobs, accept, score - 2.0, nci, ncj)
    assert np.array_equal(low, er.claim(jobs, accept, score - 2.0, s.V, nci, ncj)) and low.sum() == 1
    a = crafted_jobs(np.random.default_rng(31), 3000, s.V, nci, ncj)
    b = crafted_jobs(np.random.default_rng(32), 3000, s.V, nci, ncj)
    b[2][:] = np.where(np.isfinite(b[2]), b[2] - 3.0, b[2])       # below every key the first call wrote
    assert np.array_equal(s.ctx.wexp_claim(*a, nci, ncj), er.claim(*a, s.V, nci, ncj))
    assert np.array_equal(s.ctx.wexp_claim(*b, nci, ncj), er.claim(*b, s.V, nci, ncj))
    # another grid shape on the same context
    nci4, ncj4 = s.ctx.cell_grid(1)
    d = crafted_jobs(np.random.default_rng(33), 2000, s.V, nci4, ncj4)
    assert np.array_equal(s.ctx.wexp_claim(*d, nci4, ncj4), er.claim(*d, s.V, nci4, ncj4))


def test_claim_outside_the_grid(sphere):
    s = sphere
    nci, ncj = s.ctx.cell_grid(2)
    jobs = np.array([[0, 1, 2, 3], [1, s.V, 2, 3], [2, 1, nci, 3], [3, 1, 2, -1], [4, -1, 0, 0], [5, 1, 2, 3]], np.int32)
    accept = np.ones(6, np.uint8)
    score = np.array([0.1, 0.9, 0.9, 0.9, 0.9, 0.1])
    win = s.ctx.wexp_claim(jobs, accept, score, nci, ncj)
    assert win.tolist() == [1, 0, 0, 0, 0, 0] == er.claim(jobs, accept, score, s.V, nci, ncj).tolist()
    with pytest.raises(RuntimeError, match="outside the grid"):
        s.ctx.wexp_claim_checked(jobs, accept, score, nci, ncj)
    assert s.ctx.wexp_claim_checked(jobs[[0, 5]], accept[[0, 5]], score[[0, 5]], nci, ncj).tolist() == [1, 0]


# ---------------------------------------------------------------------------
# 3. mark
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [2, 3])
def test_mark(sphere, cell):
    s = sphere
    rng, c, nrm, ref, mask = sphere_frontier(s, 30, 40 + cell)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    jobs, cc, cn, cref, tot = gpu_children(s, c, nrm, ref, mask, cell, np.zeros((s.V, ncj, nci), np.uint8), 1.0, 4000)
    m = len(jobs)
    assert m == tot > 100
    win = (rng.random(m) < 0.5).astype(np.uint8) * rng.integers(1, 256, m).astype(np.uint8)
    cmask = random_masks(rng, m, s.V, 0.3)
    cc[0] = s.O[3] * 1.2                      # a winner behind a mask view's camera: only its own cell
    win[0] = 1
    cmask[0, 0] |= np.uint64(1 << 3)
    occ =((rng.random((s.V, ncj, nci)) < 0.2) * 5).astype(np.uint8)
    got = s.ctx.wexp_mark(jobs, win, cc, cref, cmask, cell, occ)
    want = er.mark(s.K, s.Rp, s.t, s.W, s.H, jobs, win, cc, cref, cmask, cell, occ.copy())
    assert np.array_equal(got, want)
    assert np.all(got[occ == 5] == 5) and (got == 1).sum() > win.astype(bool).sum()


# ---------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------
def test_arguments(pkg, sphere):
    s = sphere
    lib = pkg._lib.load()
    h = s.ctx.handle
    one = ctypes.c_void_p(16)                # never dereferenced: every call below fails its checks or has n = 0

    def children(n=1, cell=2, max_dist=1.0, cap=4, ptr=one):
        return lib.mvs_wexp_children_device(h, n, ptr, one, one, one, cell, one, max_dist, cap, one, one, one, one, one,
                                            None)

    def claim(m=1, nci=4, ncj=4, ptr=one):
        return lib.mvs_wexp_claim_device(h, m, ptr, one, one, nci, ncj, one, None)

    def mark(m=1, cell=2, ptr=one):
        return lib.mvs_wexp_mark_device(h, m, ptr, one, one, one, one, cell, one, None)

    for call, msg in ((lambda: children(cell=0), "cell_size must be in 1..16"),
                      (lambda: children(cell=17), "cell_size must be in 1..16"),
                      (lambda: children(max_dist=0.0), "max_dist must be > 0"),
                      (lambda: children(max_dist=float("nan")), "max_dist must be > 0"),
                      (lambda: children(cap=-1), "cap < 0"),
                      (lambda: children(n=-1), "n < 0"),
                      (lambda: children(ptr=None), "null pointer"),
                      (lambda: claim(m=-1), "m < 0"),
                      (lambda: claim(nci=0), "nci and ncj"),
                      (lambda: claim(ptr=None), "null pointer"),
                      (lambda: mark(m=-1), "m < 0"),
                      (lambda: mark(cell=0), "cell_size must be in 1..16"),
                      (lambda: mark(ptr=None), "null pointer")):
        assert call() == -1                      # MVS_E_ARG
        assert msg in pkg._lib.last_error(h), (msg, pkg._lib.last_error(h))
    # n = 0: MVS_OK whatever the pointers
    assert children(n=0, ptr=None) == 0 and claim(m=0, ptr=None) == 0 and mark(m=0, ptr=None) == 0
    with pytest.raises(RuntimeError, match="cell_size"):
        s.ctx.cell_grid(0)


# ---------------------------------------------------------------------------
# 5. composition
# ---------------------------------------------------------------------------
def seeds_of(s, n=8, seed=1):
    c, nrm, ref, _ = wr.sphere_patches(s.K, s.R, s.t, n, RAD, np.random.default_rng(seed))
    return c, nrm, ref


@pytest.mark.parametrize("cell", [2, 4])
def test_one_round_replay(sphere, cell):
    """Rounds 0 and 1 of a chain with two refinement levels, traced: the
    children's geometry and photo scores against the restatements, and every
    decision replayed by the restatement from the GPU's own count and avg."""
    s = sphere
    c, nrm, ref = seeds_of(s)
    vlb, wid, min_ncc, min_cos = 2, 3, 0.7, 0.3
    res = s.ctx.expand_warped(c, nrm, ref, 2, cell_size=cell, wid=wid, min_ncc=min_ncc, min_cos=min_cos, vlb=vlb,
                              refine_levels=2, trace=True)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    assert res["max_dist"] == er.default_max_dist(s.K, s.Rp, s.t, c[0], ref[0], cell)
    assert len(res["trace"]) == 2
    occ = np.zeros((s.V, ncj, nci), np.uint8)
    first = 0
    for rnd, tr in enumerate(res["trace"]):
        m = len(tr["jobs"])
        if rnd == 0:
            jobs, inside = er.seed_jobs(s.K, s.Rp, s.t, s.W, s.H, c, ref, cell)
            assert np.array_equal(tr["jobs"], jobs) and inside.all()
            assert np.array_equal(tr["cc"], c) and np.array_equal(tr["cn"], nrm) and np.array_equal(tr["cref"], ref)
        else:
            f = res["round"] == rnd - 1
            want = er.children(s.K, s.Rp, s.t, s.W, s.H, res["c"][f], res["nrm"][f], res["ref"][f], res["mask"][f],
                               cell, occ, res["max_dist"])
            assert np.array_equal(tr["jobs"], want[0]) and np.array_equal(tr["cref"], want[3])
            assert tr["cn"].tobytes() == want[2].tobytes()
            assert np.abs(tr["cc"] - want[1]).max() <= 1e-13 * 0.4 * 10      # |c - O| < 0.4, cos > 0.1 here
            inside = np.ones(m, bool)
        # photo scores: test_warped_gpu's rule
        o = wr.warped_batch(s.gray, s.K, s.Rp, s.t, tr["cc"], tr["cn"], tr["cref"], wid, min_cos)
        check_against_reference((tr["xy"], tr["mask"], tr["count"], tr["avg"], tr["ncc"]), o, tr["cref"], min_ncc,
                                s.V, f"cell {cell} round {rnd} ({m} jobs)")
        # decisions, from the GPU's own numbers
        accept = ((tr["count"] >= vlb) & inside).astype(np.uint8)
        assert np.array_equal(tr["accept"], accept)
        win = er.claim(tr["jobs"], accept, tr["avg"], s.V, nci, ncj)
        assert np.array_equal(tr["win"], win)
        wk = np.flatnonzero(win)
        assert len(wk) > 0
        kept = (tr["refined"]["count"] >= vlb) & (tr["refined"]["avg"] >= tr["avg"][wk])
        assert np.array_equal(tr["kept"].astype(bool), kept)
        # the patch set holds the final patches of the round, in job order
        f = np.flatnonzero(res["round"] == rnd)
        assert len(f) == len(wk) and f[0] == first
        cc, cn, mask, count, avg = (tr[k].copy() for k in ("cc", "cn", "mask", "count", "avg"))
        cc[wk[kept]], cn[wk[kept]] = tr["refined"]["c"][kept], tr["refined"]["nrm"][kept]
        count[wk[kept]], avg[wk[kept]] = tr["refined"]["count"][kept], tr["refined"]["avg"][kept]
        assert np.array_equal(res["c"][f], cc[wk]) and np.array_equal(res["nrm"][f], cn[wk])
        assert np.array_equal(res["count"][f], count[wk]) and np.array_equal(res["avg"][f], avg[wk])
        assert np.array_equal(res["cell"][f], tr["jobs"][wk, 2:]) and np.array_equal(res["ref"][f], tr["cref"][wk])
        assert np.array_equal(res["mask"][f][~kept], mask[wk][~kept])
        parent = tr["jobs"][wk, 0].astype(np.int64)
        assert np.array_equal(res["parent"][f], np.where(parent >= 0, parent + (first - prev_n if rnd else 0), -1))
        mask[wk] = res["mask"][f]
        er.mark(s.K, s.Rp, s.t, s.W, s.H, tr["jobs"], win, cc, tr["cref"], mask, cell, occ)
        assert np.array_equal(tr["occ"], occ)
        print(f"cell {cell} round {rnd}: {m} jobs, {int(accept.sum())} accepted, {len(wk)} winners, "
              f"{int(kept.sum())} refined patches kept")
        prev_n = len(wk)
        first += len(wk)
    assert np.array_equal(res["occ"], occ)


def owners(ch):
    return {(int(r), int(i), int(j)) for r, (i, j) in zip(ch["ref"], ch["cell"])}


def surface_error(c):
    return np.abs(np.sqrt((np.asarray(c) ** 2).sum(1)) - RAD)


@pytest.fixture(scope="module")
def gpu_chains(sphere):
    """8 seeds, 5 rounds, wid 3, cell 2 on the GPU: twice without refinement, once with two levels."""
    s = sphere
    c, nrm, ref = seeds_of(s)
    kw = dict(cell_size=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2)
    return (s.ctx.expand_warped(c, nrm, ref, 5, **kw), s.ctx.expand_warped(c, nrm, ref, 5, **kw),
            s.ctx.expand_warped(c, nrm, ref, 5, refine_levels=2, **kw))


def test_chain_is_deterministic_and_keeps_its_invariants(gpu_chains):
    a, b, refined = gpu_chains
    for k in ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell", "occ"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for ch in (a, refined):
        per_round = np.bincount(ch["round"], minlength=5)
        print("patches per round", per_round.tolist())
        assert len(owners(ch)) == len(ch["ref"]) > 1000
        assert np.all(ch["count"] >= 2)
        assert np.all(per_round > 0)
        kids = ch["parent"] >= 0
        assert np.array_equal(kids, ch["round"] > 0)
        assert np.array_equal(ch["round"][ch["parent"][kids]], ch["round"][kids] - 1)
        assert np.all(ch["occ"][ch["ref"], ch["cell"][:, 1], ch["cell"][:, 0]] == 1)


def test_chain_against_the_restatement(sphere, gpu_chains):
    """The (ref, cell) sets of the GPU chain and of the restatement's chain (CPU,
    no refinement) share at least 98 % of the larger set: a differing decision
    needs a pair of scores inside the 1e-8 band of the photo test's tolerance
    and then cascades."""
    s = sphere
    c, nrm, ref = seeds_of(s)
    cpu = er.expand_chain(s.gray, s.K, s.Rp, s.t, c, nrm, ref, 5, cell=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2,
                          scorer=er.score_batch_fast)
    g, r = owners(gpu_chains[0]), owners(cpu)
    share = len(g & r) / max(len(g), len(r))
    same_order = len(g) == len(r) and np.array_equal(gpu_chains[0]["cell"], cpu["cell"]) \
        and np.array_equal(gpu_chains[0]["ref"], cpu["ref"])
    print(f"GPU chain {len(g)} patches, restatement chain {len(r)}, shared {len(g & r)} = {share:.4f} of the larger "
          f"set; identical sets in identical order: {same_order}")
    assert share >= 0.98


def test_chain_refinement_keeps_the_surface(gpu_chains):
    """Median distance to the sphere of the last round's patches: with two
    refinement levels at most half of the unrefined chain's."""
    plain, _, refined = gpu_chains
    for name, ch in (("plain", plain), ("refine_levels=2", refined)):
        med = [float(np.median(surface_error(ch["c"][ch["round"] == r]))) * 1e3 for r in range(5)]
        print(f"{name}: {len(ch['ref'])} patches, median surface error per round (mm)",
              " ".join(f"{m:.4f}" for m in med))
    last_p = np.median(surface_error(plain["c"][plain["round"] == 4]))
    last_r = np.median(surface_error(refined["c"][refined["round"] == 4]))
    assert last_r <= 0.5 * last_p


def test_max_patches_and_empty_input(pkg, sphere):
    s = sphere
    c, nrm, ref = seeds_of(s)
    kw = dict(cell_size=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2)
    full = s.ctx.expand_warped(c, nrm, ref, 3, **kw)
    part = s.ctx.expand_warped(c, nrm, ref, 3, max_patches=100, **kw)
    assert len(part["ref"]) == 100 < len(full["ref"])
    for k in ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell"):
        assert np.array_equal(part[k], full[k][:100]), k
    none = s.ctx.expand_warped(np.empty((0, 3)), np.empty((0, 3)), np.empty(0, np.int32), 3, **kw)
    assert none["c"].shape == (0, 3) and none["mask"].shape == (0, 1) and not none["occ"].any()
    # seeds facing away from every camera are invalid: no winner, the chain stops
    away = s.ctx.expand_warped(c, -nrm, ref, 3, **kw)
    assert len(away["ref"]) == 0 and not away["occ"].any()
    helper = pkg.expand_patches_warped(s.ctx, c, nrm, ref, rounds=3, cell_size=2, wid=3)
    assert np.array_equal(helper["c"], full["c"])


# ---------------------------------------------------------------------------
# 6. interleaving with the tiled scorer
# ---------------------------------------------------------------------------
INTERLEAVE = r"""
import sys, numpy as np, importlib, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {golden!r})
from make_seeds import load_dino
from oracle import oracle as orc
pkg = importlib.import_module({pkg!r})
imgs, K, R, t = load_dino({data!r})
rgb = np.stack(imgs)
ctx = pkg.MvsContext(rgb, K, R, t, device=0)
c, ref = pkg.synthetic.candidates(4096, K, R, t, seed=11)
O = -np.einsum("vji,vj->vi", ctx.rproj(), t.reshape(-1, 3))
nrm = O[ref] - c
nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
dev = torch.device("cuda:0")
st = torch.cuda.Stream(dev)
def tiled():
    with torch.cuda.stream(st):
        tc, tr = torch.from_numpy(c).to(dev), torch.from_numpy(ref).to(dev)
        xy = torch.empty((len(ref), 2), dtype=torch.float64, device=dev)
        rec = torch.empty((len(ref), ctx.words + 1), dtype=torch.int64, device=dev)
        ctx.score_device_rec(tc, tr, xy, rec, 0.7, 5, stream=st.cuda_stream)
        out = xy.cpu().numpy(), rec.cpu().numpy()
    st.synchronize()
    return out
first = tiled()
grown = ctx.expand_warped(c[:1024], nrm[:1024], ref[:1024], 2, cell_size=2, wid=5, trace=True)
again = tiled()
assert ctx.scorer_stats()["batches"] == 2, ctx.scorer_stats()
want = orc.Scene(rgb, K, R, t).score_batch(c, ref, 0.7, 5)
for a, b in zip(first, again):
    assert np.array_equal(a, b)
assert np.array_equal(first[0], want[0])
assert np.array_equal(first[1][:, :ctx.words].view(np.uint64), want[1])
assert np.allclose(first[1][:, ctx.words].copy().view(np.float64), want[3], rtol=0, atol=1e-12)
assert len(grown["trace"]) == 2 and len(grown["trace"][1]["jobs"]) > 0 and grown["occ"].any()
ctx.close()
print("interleaved ok", len(grown["ref"]), "patches", len(grown["trace"][1]["jobs"]), "jobs", flush=True)
"""


def test_interleaved_with_tiled_scorer():
    """score_device_rec, a two-round expansion (children, claim and mark between
    the warped scorer's calls), score_device_rec under MVS_SCORE_KERNEL=tiled in
    a fresh process: the expansion leaves the tiled scorer's scratch and counter
    sets alone, so both tiled results are equal and are the oracle's."""
    code = INTERLEAVE.format(repo=REPO, golden=os.path.join(REPO, "tests", "golden"), pkg=PKG_NAME,
                             data=os.path.join(REPO, "data", "dinoRing"))
    env = dict(os.environ, MVS_SCORE_KERNEL="tiled")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=env)
    print(p.stdout[-300:])
    assert p.returncode == 0 and "interleaved ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
