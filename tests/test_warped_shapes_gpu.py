"""The warped family's kernels at odd image sizes, on the borders and at view
counts up to 256 (k_score_warp, k_refine_warp, k_wexp_children / _claim_* /
_mark, k_wfilt_front / _conflict / _decide / _support, k_wpatch_color and the
expand_warped / filter_warped / resume_warped / reconstruct_warped chains)
against the restatements under tests/, on the scenes and patch sets of
warped_shapes.py.  test_warped_shapes_host.py proves from the restatements
alone that those inputs reach the borders, the border cells, the strips and
every mask word.

Rules, unchanged from the family's other tests: score_warped by
test_warped_gpu.check_against_reference, refine_warped_level by
test_refine_gpu.check_level (their tolerances, bands and caps); everything
else bit-equal with no row left out, on outputs pre-filled with canaries (the
helpers of test_expand_gpu, test_wfilt_gpu, test_support_gpu and
test_seed_gpu).  The chains are held to what test_expand_gpu, test_wfilt_gpu
and test_loop_gpu demand at 96 x 128: the filter chain, the resumed expansion
and a loop whose filter removes nothing byte for byte; an expansion or a loop
with a real filter against the restatement's shares at least 98 % of the
(ref, cell) set (the scorers differ in the last bits of an ncc).
"""
import numpy as np
import pytest

import expand_reference as er
import filter_reference as fr
import loop_reference as lr
import refine_reference as rr
import support_reference as sr
import warped_shapes as ws
from test_expand_gpu import compare_children, crafted_jobs, occupancy
from test_loop_gpu import NOTHING, REAL, same_set
from test_refine_gpu import A8, _lists, check_level, reference_level
from test_seed_gpu import compare_color
from test_support_gpu import compare as compare_support, gpu_support
from test_warped_gpu import check_against_reference
from test_wfilt_gpu import compare_front, compare_test, gpu_test

pytestmark = pytest.mark.gpu


class Gpu(ws.Scene):
    """A warped_shapes scene with a context on it."""

    def __init__(self, pkg, host):
        import torch
        assert torch.cuda.is_available(), "GPU test without a GPU"
        self.__dict__.update(host.__dict__)
        self.ctx = pkg.MvsContext(host.rgb, host.K, host.R, host.t_raw, device=0)
        assert (self.ctx.V, self.ctx.H, self.ctx.W, self.ctx.words) == (host.V, host.H, host.W, host.words)
        assert np.array_equal(self.ctx.rproj(), host.Rp)


@pytest.fixture(scope="module", params=ws.SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def odd(request, pkg):
    s = Gpu(pkg, ws.sphere(*request.param))
    yield s
    s.ctx.close()


@pytest.fixture(scope="module", params=ws.VIEW_COUNTS, ids=lambda v: f"V{v}")
def ringv(request, pkg):
    s = Gpu(pkg, ws.ring(request.param))
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def chain_scene(pkg):
    s = Gpu(pkg, ws.sphere(*ws.CHAIN_SIZE))
    yield s
    s.ctx.close()


# ---------------------------------------------------------------------------
# 1. score_warped
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("min_cos", [0.0, 0.3])
@pytest.mark.parametrize("wid", ws.WIDS)
def test_score_odd_sizes(odd, wid, min_cos):
    s = odd
    case = ws.score_case(s.H, s.W, wid, min_cos)
    c, nrm, ref = case["c"], case["nrm"], case["ref"]
    out = s.ctx.score_warped(c, nrm, ref, ws.MIN_NCC, wid, min_cos, want_ncc=True)
    assert np.array_equal(out[0], s.ctx.score(c, ref, ws.MIN_NCC, wid)[0])
    assert out[0].tobytes() == np.asarray(case["o"]["xy"], np.float64).tobytes()
    check_against_reference(out, case["o"], ref, ws.MIN_NCC, s.V, f"k_score_warp {s.H}x{s.W} wid {wid} min_cos {min_cos}")
    lean = s.ctx.score_warped(c, nrm, ref, ws.MIN_NCC, wid, min_cos)
    for a, b in zip(lean, out):
        assert np.array_equal(a, b)


def test_score_view_counts(ringv):
    s = ringv
    case = ws.ring_score_case(s.V)
    c, nrm, ref, wid, min_cos = (case[k] for k in ("c", "nrm", "ref", "wid", "min_cos"))
    out = s.ctx.score_warped(c, nrm, ref, ws.RING_MIN_NCC, wid, min_cos, want_ncc=True)
    assert np.array_equal(out[0], s.ctx.score(c, ref, 0.7, wid)[0])
    check_against_reference(out, case["o"], ref, ws.RING_MIN_NCC, s.V, f"k_score_warp ring V {s.V} wid {wid}")
    xy, mask, count, avg, ncc = out
    assert mask.shape == (len(ref), s.words)
    if s.V & 63:
        assert not (mask[:, -1] >> np.uint64(s.V & 63)).any()            # pad views
    if s.V == 1:
        assert np.all(np.isnan(ncc)) and not count.any() and not mask.any() and not avg.any()
    if s.V >= 63:
        assert all(mask[:, g].any() for g in range(s.words))


# ---------------------------------------------------------------------------
# 2. refine_warped_level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("wid", [4, 5])
def test_refine_odd_sizes(odd, wid):
    s = odd
    r = ws.refine_set(s.H, s.W, wid)
    c, nrm, ref = r["c"], r["nrm"], r["ref"]
    views = _lists(s.ctx, c, nrm, ref, wid, 0.3)          # the library's own lists, checked against rr.view_lists
    dstep = s.ctx.refine_depth_steps(c, ref, 1.5)
    assert np.array_equal(dstep, rr.depth_steps(s.K, s.Rp, s.t, c, ref, 1.5))
    got = s.ctx.refine_warped_level(c, nrm, ref, views, dstep, wid, 0.3, 2, 1, A8, 1.0, want_scores=True)
    refs = reference_level(s.gray, s.K, s.Rp, s.t, c, nrm, ref, views, dstep, wid, 0.3, 2, 1)
    scored = check_level(got, refs, c, nrm, ref, s.Rp, s.t, f"k_refine_warp {s.H}x{s.W} wid {wid}")
    leaving = sum(int((o["border"] < 0).sum()) for o in refs if o["valid"])
    print(f"  {leaving} hypotheses leave the image")
    assert scored > 300 and leaving > 0


def test_refine_list_lengths_6_7_9_31(pkg):
    """Hand-built lists of 6, 7, 9 and 31 views (segment widths 8, 8, 16, 32) at wid 4 on the 65-view ring."""
    s = Gpu(pkg, ws.ring(65))
    try:
        rng = np.random.default_rng(8)
        lens = [6, 7, 9, 31, 31, 9, 7, 6]
        n = len(lens)
        c = rng.uniform(-0.004, 0.004, (n, 3)) / np.sqrt(3)
        ref = np.arange(55, 55 + n).astype(np.int32)            # the longer lists cross view 64 and wrap to 0
        nrm = ws.toward_camera(s, c, ref)
        views = np.full((n, 32), -1, np.int32)
        for i, L in enumerate(lens):
            near = sorted(range(65), key=lambda v: (min((v - ref[i]) % 65, (ref[i] - v) % 65), v))[1:L + 1]
            views[i, :L] = sorted(near)
        assert sorted((views >= 0).sum(1)) == sorted(lens) and (views == 64).any()
        dstep = np.full(n, 0.004)
        got = s.ctx.refine_warped_level(c, nrm, ref, views, dstep, 4, 0.0, 2, 1, A8, 1.0, want_scores=True)
        refs = reference_level(s.gray, s.K, s.Rp, s.t, c, nrm, ref, views, dstep, 4, 0.0, 2, 1)
        assert check_level(got, refs, c, nrm, ref, s.Rp, s.t, "k_refine_warp ring V 65 lists 6/7/9/31 wid 4",
                           budget=False) > 100
    finally:
        s.ctx.close()


# ---------------------------------------------------------------------------
# 3. children, claim, mark
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vacant", "random", "taken"])
@pytest.mark.parametrize("cell", ws.CELLS)
def test_children_odd_sizes(odd, cell, kind):
    s = odd
    p = ws.cell_set(s.H, s.W, cell)
    nci, ncj = er.grid_shape(s.W, s.H, cell)
    assert s.ctx.cell_grid(cell) == (nci, ncj)
    occ = occupancy(kind, np.random.default_rng([3, cell, s.H]), s.V, ncj, nci)
    want = compare_children(s, p["c"], p["nrm"], p["ref"], p["mask"], cell, occ, 1.0,
                            label=f"k_wexp_children {s.H}x{s.W} cell {cell} {kind}")
    jobs = want[0]
    if kind == "taken":
        assert len(jobs) == 0
        return
    border = (jobs[:, 2] == 0) | (jobs[:, 2] == nci - 1) | (jobs[:, 3] == 0) | (jobs[:, 3] == ncj - 1)
    assert border.sum() > 20 and jobs[:, 2].max() == nci - 1 and jobs[:, 3].max() == ncj - 1
    assert not np.isin(jobs[:, 0], np.flatnonzero(p["strip"])).any()
    print(f"  {int(border.sum())} children in border cells, {int(p['strip'].sum())} strip patches without a job: bit-equal")


@pytest.mark.parametrize("cell", ws.CELLS)
def test_claim_and_mark_odd_sizes(odd, cell):
    s = odd
    p = ws.cell_set(s.H, s.W, cell)
    nci, ncj = s.ctx.cell_grid(cell)
    assert (nci, ncj) == er.grid_shape(s.W, s.H, cell)
    # claim: crafted jobs on a few cells of this grid, its four corners among them
    jobs, accept, score = crafted_jobs(np.random.default_rng([5, cell, s.W]), 700, s.V, nci, ncj)
    win = s.ctx.wexp_claim(jobs, accept, score, nci, ncj)
    want = er.claim(jobs, accept, score, s.V, nci, ncj)
    assert win.dtype == np.uint8 and np.array_equal(win, want) and want.sum() >= 4
    # one past the grid each way: no contender
    out = jobs.copy()
    out[::2, 2], out[1::2, 3] = nci, ncj
    assert not s.ctx.wexp_claim(out, accept, score, nci, ncj).any() and not er.claim(out, accept, score, s.V, nci, ncj).any()
    # mark: every patch the winner of its own cell ((-1, -1) in a strip), its mask's views placed anywhere
    rng = np.random.default_rng([6, cell, s.W])
    sj = ws.seed_style_jobs(s, p, cell)
    m = len(sj)
    winm = np.ones(m, np.uint8)
    winm[::7] = 0
    occ = ((rng.random((s.V, ncj, nci)) < 0.2) * 5).astype(np.uint8)
    got = s.ctx.wexp_mark(sj, winm, p["c"], p["ref"], p["mask"], cell, occ)
    wantm = er.mark(*s.cam(), sj, winm, p["c"], p["ref"], p["mask"], cell, occ.copy())
    assert np.array_equal(got, wantm) and np.all(got[occ == 5] == 5)
    new = (got == 1)
    assert new[:, 0, :].any() and new[:, -1, :].any() and new[:, :, 0].any() and new[:, :, -1].any()
    strip = np.flatnonzero(p["strip"])
    if len(strip):
        only = s.ctx.wexp_mark(sj[strip], np.ones(len(strip), np.uint8), p["c"][strip], p["ref"][strip],
                               p["mask"][strip], cell, np.zeros_like(occ))
        assert not only.any()
    print(f"k_wexp_claim / k_wexp_mark {s.H}x{s.W} cell {cell}: grid {ncj}x{nci}, {int(want.sum())} winners, "
          f"{int(new.sum())} cells marked, {len(strip)} strip patches mark nothing: bit-equal")


def test_children_claim_mark_view_counts(ringv):
    s = ringv
    V = s.V
    rng = np.random.default_rng([4, V])
    n = 41
    c = rng.uniform(-0.005, 0.005, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, V, n).astype(np.int32)
    nrm = ws.toward_camera(s, c, ref)
    mask = ws.plant_pad_bits(ws.random_masks(rng, n, V, 0.3), V)
    for cell in (1, 3):
        nci, ncj = er.grid_shape(s.W, s.H, cell)
        occ = occupancy("random", rng, V, ncj, nci)
        want = compare_children(s, c, nrm, ref, mask, cell, occ, 1.0, label=f"k_wexp_children ring V {V} cell {cell}")
        jobs, cc, cn, cref = want
        if V > 64:
            assert all(((jobs[:, 1] >> 6) == g).any() for g in range(s.words))       # every group emits jobs
            groups = [len(set((jobs[jobs[:, 0] == k, 1] >> 6).tolist())) for k in range(n)]
            assert max(groups) == s.words                                            # one patch's run crosses every group
        m = len(jobs)
        win = (rng.random(m) < 0.5).astype(np.uint8)
        cmask = ws.plant_pad_bits(ws.random_masks(rng, m, V, 0.3), V)
        got = s.ctx.wexp_mark(jobs, win, cc, cref, cmask, cell, occ)
        assert np.array_equal(got, er.mark(*s.cam(), jobs, win, cc, cref, cmask, cell, occ.copy()))
        if V > 64:
            assert all((got[64 * g:64 * g + 64] == 1).any() for g in range(s.words))
    nci, ncj = s.ctx.cell_grid(2)
    cj = crafted_jobs(rng, 900, V, nci, ncj)
    assert np.array_equal(s.ctx.wexp_claim(*cj, nci, ncj), er.claim(*cj, V, nci, ncj))
    print(f"k_wexp_children / claim / mark ring V {V}: {s.words} group(s): bit-equal")


# ---------------------------------------------------------------------------
# 4. front, test, support
# ---------------------------------------------------------------------------
def decide_keep(s, p, vis, conf, min_views):
    """k_wfilt_decide's rule on the restatement's vis and conf (filter_reference.vistest's last loop)."""
    keep = np.zeros(len(p["ref"]), np.uint8)
    for k in range(len(keep)):
        views = fr.views_of(p["ref"][k], p["mask"][k], s.V)
        if views is None:
            continue
        seen = sum(bin(int(x)).count("1") for x in vis[k])
        keep[k] = seen >= min_views and len(views) * fr.weight(p["avg"][k]) >= int(conf[k])
    return keep


def sweep_test(s, p, cell, front, label):
    """mvs_wfilt_test_device at adj_px 0 and 2: vis, conf and keep at min_views
    3 against the restatement, keep at min_views 0, 1 and V + 1 by its rule."""
    conflicts = 0
    for adj_px in (0.0, 2.0):
        vis, conf, keep, F = compare_test(s, p["c"], p["nrm"], p["ref"], p["mask"], p["avg"], cell, adj_px, 3, front,
                                          f"{label} adj_px {adj_px}")
        conflicts += sum(len(f) for f in F)
        for min_views in (0, 1, s.V + 1):
            g = gpu_test(s, p["c"], p["nrm"], p["ref"], p["mask"], p["avg"], cell, adj_px, min_views, front)
            assert np.array_equal(g[0], vis) and np.array_equal(g[1], conf), (label, adj_px, min_views)
            assert np.array_equal(g[2], decide_keep(s, p, vis, conf, min_views)), (label, adj_px, min_views)
    return conflicts


def sweep_support(s, p, cell, front, label):
    """mvs_wfilt_support_device at adj_px 0 and 2 against the restatement, the decision's scalars swept by its rule."""
    total = 0
    for adj_px in (0.0, 2.0):
        nb, adj, _ = compare_support(s, p["c"], p["nrm"], p["ref"], p["mask"], cell, adj_px, 0.25, 1, front,
                                     f"{label} adj_px {adj_px}")
        total += int(nb.sum())
        for ms in (0.0, 0.5, 1.0):
            for mn in (0, 4):
                g = gpu_support(s, p["c"], p["nrm"], p["ref"], p["mask"], cell, adj_px, ms, mn, front)
                keep = np.array([sr.decide(N, A, ms, mn) for N, A in zip(nb, adj)], np.uint8)
                assert np.array_equal(g[0], nb) and np.array_equal(g[1], adj) and np.array_equal(g[2], keep), (label, ms, mn)
    return total


@pytest.mark.parametrize("cell", ws.CELLS)
def test_filter_kernels_odd_sizes(odd, cell):
    s = odd
    p = ws.cell_set(s.H, s.W, cell)
    n = len(p["ref"])
    label = f"{s.H}x{s.W} cell {cell}"
    front, _ = compare_front(s, p["c"], p["ref"], p["mask"], cell, f"k_wfilt_front {label}")
    assert (front[:, 0, :] >= 0).any() and (front[:, -1, :] >= 0).any() and (front[:, :, 0] >= 0).any() \
        and (front[:, :, -1] >= 0).any()
    assert not np.isin(front, np.flatnonzero(p["strip"])).any()
    dense = ws.cell_dense_front(s, p, cell)
    conflicts = sweep_test(s, p, cell, front, f"k_wfilt_conflict {label}")
    conflicts += sweep_test(s, p, cell, dense, f"k_wfilt_conflict {label} dense grid")
    N = sweep_support(s, p, cell, front, f"k_wfilt_support {label}")
    Nd = sweep_support(s, p, cell, dense, f"k_wfilt_support {label} dense grid")
    assert conflicts > 0 and Nd > 4 * n
    print(f"k_wfilt_front / conflict / decide / support {label}: {conflicts} conflicts, N {N} own grid / {Nd} dense grid: "
          f"bit-equal")


def test_filter_kernels_view_counts(ringv):
    s = ringv
    V = s.V
    p = ws.ring_set(V)
    n = len(p["ref"])
    conflicts = 0
    for cell in (2, 3):
        label = f"ring V {V} cell {cell}"
        front, _ = compare_front(s, p["c"], p["ref"], p["mask"], cell, f"k_wfilt_front {label}")
        if V > 64:
            assert all((front[64 * g:64 * g + 64] >= 0).any() for g in range(s.words))
        planted = ws.planted_front(s, p, cell)
        conflicts += sweep_test(s, p, cell, front, f"k_wfilt_conflict<{s.words}> {label}")
        conflicts += sweep_test(s, p, cell, planted, f"k_wfilt_conflict<{s.words}> {label} planted grid")
        sweep_support(s, p, cell, front, f"k_wfilt_support {label}")
        sweep_support(s, p, cell, ws.dense_front(np.random.default_rng([9, V, cell]), front.shape, n),
                      f"k_wfilt_support {label} dense")
    assert conflicts > 0
    print(f"k_wfilt_conflict<{s.words}> ran at V {V} ({s.words} group(s)), with k_wfilt_front / decide / support: "
          f"{conflicts} conflicts: bit-equal")


# ---------------------------------------------------------------------------
# 5. patch colours
# ---------------------------------------------------------------------------
def test_color_odd_sizes(odd):
    s = odd
    p = ws.cell_set(s.H, s.W, 2)
    e = ws.color_edge_rows("sphere", (s.H, s.W))
    c, ref, mask = (np.concatenate([p[k], e[k]]) for k in ("c", "ref", "mask"))
    color, nv = compare_color(s, c, ref, mask, f"k_wpatch_color {s.H}x{s.W}")
    edge = nv[len(p["ref"]):]
    assert np.array_equal(edge > 0, e["kind"] <= 2) and nv.max() > 3
    print(f"k_wpatch_color {s.H}x{s.W}: {len(ref)} rows, nviews up to {int(nv.max())}, edge rows counted "
          f"{int((edge > 0).sum())} / not counted {int((edge == 0).sum())}: bit-equal")


def test_color_view_counts(ringv):
    s = ringv
    p = ws.ring_set(s.V)
    e = ws.color_edge_rows("ring", s.V)
    c, ref, mask = (np.concatenate([p[k], e[k]]) for k in ("c", "ref", "mask"))
    color, nv = compare_color(s, c, ref, mask, f"k_wpatch_color ring V {s.V}")
    assert np.array_equal(nv[len(p["ref"]):] > 0, e["kind"] <= 2)
    if s.V >= 63:
        assert nv.max() > 0.3 * s.V
    print(f"k_wpatch_color ring V {s.V}: nviews up to {int(nv.max())}: bit-equal")


# ---------------------------------------------------------------------------
# 6. the chains
# ---------------------------------------------------------------------------
def owners(ch):
    return {(int(r), int(i), int(j)) for r, (i, j) in zip(ch["ref"], ch["cell"])}


def chain_kw(cell, wid, **more):
    return dict(cell_size=cell, wid=wid, **ws.CHAIN_KW, **more)


@pytest.fixture(scope="module")
def gpu_chains(chain_scene):
    """expand_warped from warped_shapes.chain_seeds, computed once per (cell, wid, rounds, refine_levels)."""
    cache = {}

    def get(cell, wid, rounds=3, refine_levels=0):
        key = (cell, wid, rounds, refine_levels)
        if key not in cache:
            cache[key] = chain_scene.ctx.expand_warped(*ws.chain_seeds(), rounds,
                                                       **chain_kw(cell, wid, refine_levels=refine_levels))
        return cache[key]
    return get


def check_invariants(s, ch, cell, rounds):
    assert len(owners(ch)) == len(ch["ref"]) and np.all(ch["count"] >= 2)
    assert np.all(np.bincount(ch["round"], minlength=rounds) > 0)
    kids = ch["parent"] >= 0
    assert np.array_equal(kids, ch["round"] > 0)
    assert np.array_equal(ch["round"][ch["parent"][kids]], ch["round"][kids] - 1)
    assert np.array_equal(ch["occ"], lr.occ_of(*s.cam(), ch["ref"], ch["cell"], ch["c"], ch["mask"], cell))


@pytest.mark.parametrize("cell,wid", ws.CHAINS)
def test_expand_chain(chain_scene, gpu_chains, cell, wid):
    """expand_warped without refinement: deterministic, its invariants, the
    occupancy of its own rows, and the restatement's chain."""
    s = chain_scene
    g = gpu_chains(cell, wid)
    again = s.ctx.expand_warped(*ws.chain_seeds(), 3, **chain_kw(cell, wid))
    same_set(g, again)
    check_invariants(s, g, cell, 3)
    cpu = ws.cpu_chain(cell, wid)
    a, b = owners(g), owners(cpu)
    share = len(a & b) / max(len(a), len(b))
    identical = len(a) == len(b) and np.array_equal(g["cell"], cpu["cell"]) and np.array_equal(g["ref"], cpu["ref"]) \
        and g["c"].tobytes() == cpu["c"].tobytes() and np.array_equal(g["mask"], cpu["mask"])
    own = int(ws.in_border_cells(s, g["ref"], g["cell"], cell).sum())
    bc = ws.border_cell_counts(s, g, cell)
    placed = bc["col0"] + bc["colN"] + bc["row0"] + bc["rowN"]
    print(f"expand_warped cell {cell} wid {wid}: GPU {len(a)} patches, restatement {len(b)}, shared {share:.4f}; "
          f"identical rows in identical order (c, ref, cell, mask bit-equal): {identical}; {own} patches own a border "
          f"cell, {placed} placements in border cells")
    assert share >= 0.98
    if (cell, wid) != (2, 3):          # at cell 2 and wid 3 no border cell can be reached (warped_shapes.CHAINS)
        assert own >= 20 and placed >= 100


@pytest.mark.parametrize("cell,wid", ws.CHAINS[:2])
def test_expand_chain_with_refinement(chain_scene, gpu_chains, cell, wid):
    """Two refinement levels: deterministic, the invariants, and every row's
    mask, count and avg are score_warped's on the row's final centre and normal."""
    s = chain_scene
    g = gpu_chains(cell, wid, 3, 2)
    same_set(g, s.ctx.expand_warped(*ws.chain_seeds(), 3, **chain_kw(cell, wid, refine_levels=2)))
    check_invariants(s, g, cell, 3)
    _, mask, count, avg = s.ctx.score_warped(g["c"], g["nrm"], g["ref"], 0.7, wid, 0.3)
    assert np.array_equal(mask, g["mask"]) and np.array_equal(count, g["count"]) and avg.tobytes() == g["avg"].tobytes()
    plain = gpu_chains(cell, wid)
    known = {row.tobytes() for row in plain["c"]}
    moved = sum(row.tobytes() not in known for row in g["c"])
    bc = ws.border_cell_counts(s, g, cell)
    print(f"expand_warped cell {cell} wid {wid} refine_levels 2: {len(g['ref'])} patches, {moved} centres not in the "
          f"unrefined chain, {bc['col0'] + bc['colN'] + bc['row0'] + bc['rowN']} placements in border cells: "
          f"deterministic, rows bit-equal to score_warped")
    assert moved > 0.2 * len(g["ref"])


@pytest.mark.parametrize("cell,wid", ws.CHAINS)
def test_filter_chain(pkg, chain_scene, cell, wid):
    """filter_warped, two visibility passes and support passes, on the
    restatement's chain with planted outliers: the restatement's chain, bit for bit."""
    s = chain_scene
    m = ws.chain_mixed_set(cell, wid)
    patches = {k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")}
    for kw in (dict(min_support=0.25), dict(min_support=0.5, min_neigh=4, support_passes=3)):
        a = s.ctx.filter_warped(patches, cell_size=cell, adj_px=2.0, min_views=3, passes=2, **kw)
        want = sr.filter_chain(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], m["avg"], cell, 2.0, 3, 2, **kw)
        assert a["removed"] == want["removed"] and a["removed_support"] == want["removed_support"], kw
        for k in ("keep", "vis", "conf", "front", "nb", "adj"):
            assert a[k].dtype == want[k].dtype and np.array_equal(a[k], want[k]), (kw, k)
        assert a["zfront"].tobytes() == want["zfront"].tobytes()
        idx = np.flatnonzero(want["keep"])
        assert np.array_equal(a["index"], idx)
        for k in patches:
            assert np.array_equal(a[k], m[k][idx]), k
        assert np.array_equal(a["occ"], lr.occ_of(*s.cam(), m["ref"][idx], m["cell"][idx], m["c"][idx], m["mask"][idx],
                                                  cell))
        print(f"filter_warped cell {cell} wid {wid} {kw}: {len(m['ref'])} patches, removed {a['removed']}, by support "
              f"{a['removed_support']}: bit-equal")
        assert sum(a["removed"]) > 0 and sum(a["removed_support"]) > 0


@pytest.mark.parametrize("refine_levels", [0, 2])
@pytest.mark.parametrize("cell,wid", ws.CHAINS[1:])
def test_resume_and_loop_without_removal(pkg, chain_scene, gpu_chains, cell, wid, refine_levels):
    """resume_warped(expand_warped(2), 1) and a loop whose filter removes nothing are expand_warped(3), byte for byte."""
    s = chain_scene
    kw = chain_kw(cell, wid, refine_levels=refine_levels)
    two, three = gpu_chains(cell, wid, 2, refine_levels), gpu_chains(cell, wid, 3, refine_levels)
    assert len(three["ref"]) > len(two["ref"]) > 0
    got = s.ctx.resume_warped(two, 1, **kw)
    same_set(three, got)
    bare = {k: v for k, v in two.items() if k not in ("occ", "max_dist")}
    same_set(three, s.ctx.resume_warped(bare, 1, max_dist=two["max_dist"], **kw))       # occ rebuilt from the rows
    loop = s.ctx.reconstruct_warped(*ws.chain_seeds(), iterations=2, rounds=2, resume_rounds=1, expand=kw, filter=NOTHING)
    same_set(three, loop)
    assert loop["keep"].all() and [h["removed"] for h in loop["history"]] == [[0], [0]]
    print(f"resume_warped / reconstruct_warped cell {cell} wid {wid} refine_levels {refine_levels}: "
          f"{len(two['ref'])} -> {len(three['ref'])} patches: bit-equal to expand_warped(3)")


def test_loop_with_planted_outliers(chain_scene):
    """reconstruct_warped with the real filter from a set with planted outliers
    (cell 3, wid 3): deterministic, one patch per (ref, cell), the occupancy of
    its rows, border cells held, and the restatement's loop."""
    s = chain_scene
    cell, wid = 3, 3
    start, src = ws.planted_chain_set(cell, wid)
    kw = chain_kw(cell, wid)
    runs = [s.ctx.reconstruct_warped(None, None, None, iterations=2, resume_rounds=1, expand=kw, filter=REAL, start=start)
            for _ in range(2)]
    a, b = runs
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k
    own = owners(a)
    assert len(own) == len(a["ref"])
    assert np.array_equal(a["occ"], lr.occ_of(*s.cam(), a["ref"], a["cell"], a["c"], a["mask"], cell))
    h = a["history"]
    assert h[0]["patches"] == len(start["ref"]) and sum(h[0]["removed"]) + sum(h[0]["removed_support"]) > 0
    assert h[0]["resumed"] > h[0]["patches"]
    cpu = lr.reconstruct(s.gray, s.K, s.Rp, s.t, None, None, None, iterations=2, resume_rounds=1,
                         expand=dict(cell=cell, wid=wid, **ws.CHAIN_KW), filter=REAL, scorer=er.score_batch_fast,
                         start=start)
    r = owners(cpu)
    share = len(own & r) / max(len(own), len(r))
    border = int(ws.in_border_cells(s, a["ref"], a["cell"], cell).sum())
    print(f"reconstruct_warped cell {cell} wid {wid}: GPU {len(own)} patches, restatement {len(r)}, shared {share:.4f}; "
          f"history GPU {h}, restatement {cpu['history']}; {len(src)} planted; {border} patches own a border cell")
    assert share >= 0.98
    assert border >= 20
