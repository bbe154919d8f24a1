"""Coverage of the warped family's odd-size, border and view-count cases
(warped_shapes.py), from the restatements alone: the GPU tests of
test_warped_shapes_gpu.py only mean something if windows really touch every
border, centres really lie in the border cells, the corner cells and the
strips, every mask word carries a bit and front patches really repeat across
view groups.  The floors below are conditions on the inputs: where a case
misses one, the inputs change, never the floor, the bands or the cap.  Run
with -s for the table (profiles/r18/host_coverage.txt)."""
import numpy as np
import pytest

import expand_reference as er
import filter_reference as fr
import refine_reference as rr
import seed_reference as sd
import support_reference as sr
import warped_reference as wr
import warped_shapes as ws
from test_warped_gpu import BORDER_BAND, COS_BAND, MAX_LEFT_OUT

# scoring sets, per scene, window size and min_cos
FLOOR_TOUCH = 4            # valid windows on each of the four borders, and with the last column at W - 2
FLOOR_CLAMP = 10           # tested pairs whose nearest sample lies within (1e-9, 1] px of a border
FLOOR_BORDER_FAIL = 100    # tested pairs with a sample outside the image
FLOOR_PASSING = 100        # tested pairs that pass min_ncc
FLOOR_SCORED_NON_PASSING = 5
FLOOR_INVALID = 16         # candidates whose window leaves the image (the aimed ones, one pixel out)
# cell sets, per scene and cell size
FLOOR_BORDER_LINE = 8      # placements in each border cell column and row
FLOOR_CORNER = 3           # placements in each corner cell
FLOOR_BORDER_CHILDREN = 50     # children emitted into border cells
FLOOR_SKIPPED = 40         # neighbours (4-walk) skipped for lying outside the grid
FLOOR_SHORT_SUPPORT = 30   # placements whose 8-walk has fewer than eight cells
FLOOR_BORDER_INCIDENCES = 500  # neighbour incidences (dense grid) of patches with a placement in a border cell
FLOOR_STRIP = 3            # patches per strip
# refinement sets, per scene and window size
FLOOR_REFINE_SCORED = 1000     # scored hypotheses
FLOOR_REFINE_LEAVING = 20      # hypotheses with a sample outside the image
# view counts
FLOOR_RING_PAIRS = 1000    # tested pairs, V >= 63
FLOOR_DUPLICATES = 10      # rows whose conflict set names a front patch in two different groups, V >= 129


@pytest.mark.parametrize("H,W", ws.SIZES)
def test_sizes_and_frames(H, W):
    """The sizes are what the issue asks for, and the sphere fills every view."""
    sc = ws.sphere(H, W)
    assert (sc.V, sc.H, sc.W) == (ws.V_SPHERE, H, W)
    assert not (sc.rgb.max(-1) == 0).any(), "a black pixel"
    widths = [w for _, w in ws.SIZES]
    heights = [h for h, _ in ws.SIZES]
    assert all(w % 16 for w in widths) and {1, 3} <= {w % 4 for w in widths} and any(h % 2 for h in heights)
    for cell in (2, 3):
        assert any(w % cell and h % cell for h, w in ws.SIZES), cell
    assert any(h > 64 and w > 64 for h, w in ws.SIZES)


def test_interior_patches_of_the_issue():
    """400 interior patches of 45 x 61 (wr.sphere_patches, true normals): the figures the sizes were chosen by."""
    sc = ws.sphere(45, 61)
    c, nrm, ref, _ = wr.sphere_patches(sc.K, sc.R, sc.t, 400, ws.RAD, np.random.default_rng(1), H=45, W=61)
    for wid, want in ((2, 365), (5, 251)):
        o = wr.warped_batch(sc.gray, sc.K, sc.Rp, sc.t, c, nrm, ref, wid, 0.3)
        with np.errstate(invalid="ignore"):
            count = (o["ncc"] > 0.7).sum(1)
        cv = ws.score_coverage(sc, o, ref, wid, 0.7, BORDER_BAND, COS_BAND)
        print(f"45x61 interior wid {wid}: {int((count >= 3).sum())} with >= 3 views, {cv['tested']} tested pairs, "
              f"{cv['left_out']} in a band")
        assert int((count >= 3).sum()) == want and cv["tested"] == 2942 and cv["left_out"] == 0
        assert cv["left"] == cv["right"] == cv["top"] == cv["bottom"] == 0      # what the new sets are for


@pytest.mark.parametrize("H,W", ws.SIZES)
def test_windows_reach_every_border(H, W):
    sc = ws.sphere(H, W)
    for wid in ws.WIDS:
        for min_cos in (0.0, 0.3):
            s = ws.score_case(H, W, wid, min_cos)
            cv = ws.score_coverage(sc, s["o"], s["ref"], wid, ws.MIN_NCC, BORDER_BAND, COS_BAND)
            share = cv["left_out"] / max(cv["tested"], 1)
            print(f"{H}x{W} wid {wid} min_cos {min_cos}: " + " ".join(f"{k}={v}" for k, v in cv.items()) +
                  f" left_out_share={share:.5f}")
            for k in ("left", "right", "right2", "top", "bottom"):
                assert cv[k] >= FLOOR_TOUCH, (wid, k, cv)
            assert cv["clamp"] >= FLOOR_CLAMP and cv["border_fail"] >= FLOOR_BORDER_FAIL, (wid, cv)
            assert cv["passing"] >= FLOOR_PASSING and cv["scored_non_passing"] >= FLOOR_SCORED_NON_PASSING, (wid, cv)
            assert len(s["ref"]) - cv["valid"] >= FLOOR_INVALID, (wid, cv)
            assert share <= MAX_LEFT_OUT, (wid, cv)
            # the aimed windows are where they were aimed
            x0, y0 = np.floor(s["o"]["xy"][:, 0]), np.floor(s["o"]["xy"][:, 1])
            spot = s["spot"]
            assert np.all(x0[spot == 0] + wid == W - 1) and np.all(x0[spot == 1] + wid == W - 2)
            assert np.all(y0[spot == 2] + wid == H - 1) and np.all(x0[spot == 3] == wid) and np.all(y0[spot == 4] == wid)
            assert not s["o"]["valid"][spot >= 9].any()


@pytest.mark.parametrize("V", ws.VIEW_COUNTS)
def test_view_counts_use_every_word(V):
    sc = ws.ring(V)
    assert (sc.V, sc.H, sc.W, sc.words) == (V, ws.RING_H, ws.RING_W, (V + 63) // 64)
    s = ws.ring_score_case(V)
    cv = ws.score_coverage(sc, s["o"], s["ref"], s["wid"], ws.RING_MIN_NCC, BORDER_BAND, COS_BAND)
    share = cv["left_out"] / max(cv["tested"], 1)
    print(f"ring V {V} scoring: " + " ".join(f"{k}={v}" for k, v in cv.items()) + f" left_out_share={share:.5f}")
    assert share <= MAX_LEFT_OUT
    if V >= 63:
        assert cv["tested"] >= FLOOR_RING_PAIRS and all(cv["words_set"]), cv
        assert cv["passing"] > 0 and cv["scored_non_passing"] > 0
    if V == 1:
        assert cv["tested"] == 0 and np.all(np.isnan(s["o"]["ncc"]))
    # the cell kernels' set: every word of mask, vis and the front grid is used
    r = ws.ring_set(V)
    bits = np.array([[bool(int(row[v >> 6]) >> (v & 63) & 1) for v in range(V)] for row in r["mask"]])
    front = fr.front_grid(*sc.cam(), r["c"], r["ref"], r["mask"], 2)[0]
    planted = ws.planted_front(sc, r, 2)
    vis, conf, keep, F = fr.vistest(*sc.cam(), r["c"], r["nrm"], r["ref"], r["mask"], r["avg"], 2, 2.0, 3, planted)
    groups = ws.conflict_groups(sc, r, 2, 2.0, planted)
    dup = sum(1 for d in groups if any(len(g) > 1 for g in d.values()))
    natural = sum(1 for d in ws.conflict_groups(sc, r, 2, 2.0, front) if any(len(g) > 1 for g in d.values()))
    pad = int((r["mask"][:, -1] >> np.uint64(V & 63)).astype(bool).sum()) if V & 63 else 0
    print(f"ring V {V} cells: mask bits per word {[int(bits[:, 64 * g:64 * g + 64].sum()) for g in range(sc.words)]}, "
          f"front cells per group {[int((front[64 * g:64 * g + 64] >= 0).sum()) for g in range(sc.words)]}, "
          f"vis bits per word {[int(sum(bin(int(x)).count('1') for x in vis[:, g])) for g in range(sc.words)]}, "
          f"{sum(len(f) for f in F)} conflicts, {int(keep.sum())} kept, rows with a front patch repeated across groups: "
          f"{dup} planted grid / {natural} own grid, {pad} rows with pad bits")
    if V > 64:
        for g in range(sc.words):
            assert bits[:, 64 * g:64 * g + 64].any() and (front[64 * g:64 * g + 64] >= 0).any() and vis[:, g].any(), g
    if V >= 129:
        assert dup >= FLOOR_DUPLICATES and natural >= 1
    if V & 63:
        assert pad >= len(r["ref"]) // 3
    if V >= 63:
        assert sum(len(f) for f in F) > 0 and 0 < keep.sum() < len(keep)


@pytest.mark.parametrize("H,W", ws.SIZES)
def test_cells_reach_the_border_and_the_strips(H, W):
    sc = ws.sphere(H, W)
    for cell in ws.CELLS:
        s = ws.cell_set(H, W, cell)
        n = len(s["ref"])
        nci, ncj = er.grid_shape(W, H, cell)
        boxes = ws.cell_boxes(H, W, cell)
        assert ("strip_x" in boxes) == (nci * cell < W) and ("strip_y" in boxes) == (ncj * cell < H)
        bc = ws.border_cell_counts(sc, s, cell)
        occ = np.zeros((sc.V, ncj, nci), np.uint8)
        jobs = er.children(*sc.cam()[:3], W, H, s["c"], s["nrm"], s["ref"], s["mask"], cell, occ, 1.0)[0]
        into_border = int(((jobs[:, 2] == 0) | (jobs[:, 2] == nci - 1) | (jobs[:, 3] == 0) | (jobs[:, 3] == ncj - 1)).sum())
        front = fr.front_grid(*sc.cam(), s["c"], s["ref"], s["mask"], cell)[0]
        nb = sr.support(*sc.cam(), s["c"], s["nrm"], s["ref"], s["mask"], cell, 2.0, 0.25, 1, front)[0]
        # the neighbour incidences of the patches with a placement in a border cell, on the dense grid
        nbd = sr.support(*sc.cam(), s["c"], s["nrm"], s["ref"], s["mask"], cell, 2.0, 0.25, 1,
                         ws.cell_dense_front(sc, s, cell))[0]
        at_border = np.array([any(i in (0, nci - 1) or j in (0, ncj - 1) for _, (i, j), _ in row or ())
                              for row in fr.placements(*sc.cam(), s["c"], s["ref"], s["mask"], cell)])
        strip = np.flatnonzero(s["strip"])
        print(f"{H}x{W} cell {cell}: grid {ncj}x{nci}, {n} patches, {len(strip)} in a strip, " +
              " ".join(f"{k}={v}" for k, v in bc.items()) + f" children={len(jobs)} into_border_cells={into_border} "
              f"front_cells={int((front >= 0).sum())} support_N={int(nb.sum())} "
              f"support_N_dense_grid={int(nbd.sum())} of_patches_in_border_cells={int(nbd[at_border].sum())}")
        for k in ("col0", "colN", "row0", "rowN"):
            assert bc[k] >= FLOOR_BORDER_LINE, (cell, k, bc)
        for k in ("corner00", "cornerN0", "corner0N", "cornerNN"):
            assert bc[k] >= FLOOR_CORNER, (cell, k, bc)
        assert into_border >= FLOOR_BORDER_CHILDREN and bc["skipped_neighbours"] >= FLOOR_SKIPPED, (cell, bc)
        assert bc["short_neighbourhoods"] >= FLOOR_SHORT_SUPPORT, (cell, bc)
        assert nbd[at_border].sum() >= FLOOR_BORDER_INCIDENCES and not nbd[s["strip"]].any(), cell
        # the aimed patches are where they were aimed
        own = ws.own_cells(sc, s, cell)
        for k in range(n):
            want = {"col0": (0, None), "colN": (nci - 1, None), "row0": (None, 0), "rowN": (None, ncj - 1),
                    "corner00": (0, 0), "cornerN0": (nci - 1, 0), "corner0N": (0, ncj - 1),
                    "cornerNN": (nci - 1, ncj - 1)}.get(str(s["box"][k]))
            if want:
                assert own[k] is not None and all(w is None or w == g for w, g in zip(want, own[k])), (k, own[k], want)
        # the strip: no job, no mark, no front cell, no neighbour
        for name in ("strip_x", "strip_y", "strip_xy"):
            assert (name in boxes) == bool((s["box"] == name).any())
            if name in boxes:
                assert (s["box"] == name).sum() >= FLOOR_STRIP
        if len(strip):
            assert all(own[k] is None for k in strip) and not np.isin(jobs[:, 0], strip).any()
            assert not np.isin(front, strip).any() and not nb[strip].any()
            sj = ws.seed_style_jobs(sc, s, cell)
            assert np.all(sj[strip, 2:] == -1)
            marked = er.mark(*sc.cam(), sj[strip], np.ones(len(strip), np.uint8), s["c"][strip], s["ref"][strip],
                             s["mask"][strip], cell, occ.copy())
            assert not marked.any()
            for k in strip:           # the projection is inside the image all the same
                x, y, depth = wr.project_ref(sc.K[s["ref"][k]], sc.Rp[s["ref"][k]], sc.t[s["ref"][k]], s["c"][k])
                assert depth > 0 and 0 <= x < W and 0 <= y < H and (x >= nci * cell or y >= ncj * cell)


@pytest.mark.parametrize("kind,key", [("sphere", (45, 61)), ("sphere", (26, 31)), ("ring", 129), ("ring", 256)])
def test_colour_rows_sit_on_the_edge(kind, key):
    sc = ws.sphere(*key) if kind == "sphere" else ws.ring(key)
    e = ws.color_edge_rows(kind, key)
    col, nv = sd.color(sc.rgb, sc.K, sc.Rp, sc.t, e["c"], e["ref"], e["mask"])
    xy = np.array([wr.project_ref(sc.K[v], sc.Rp[v], sc.t[v], c)[:2] for c, v in zip(e["c"], e["ref"])])
    k = e["kind"]
    print(f"{kind} {key}: colour edge rows, nviews {nv.tolist()}")
    assert np.all(xy[k == 0, 0] == sc.W - 1) and np.all(nv[k == 0] == 1)
    assert np.all(xy[k == 1, 1] == sc.H - 1) and np.all(nv[k == 1] == 1)
    assert np.all((xy[k == 2, 0] > sc.W - 2) & (xy[k == 2, 0] < sc.W - 1)) and np.all(nv[k == 2] == 1)
    assert np.all((xy[k == 3, 0] > sc.W - 1) & (xy[k == 3, 0] < sc.W)) and np.all(nv[k == 3] == 0)
    assert np.all((xy[k == 4, 1] > sc.H - 1) & (xy[k == 4, 1] < sc.H)) and np.all(nv[k == 4] == 0)
    assert (k == 0).sum() >= 2 and (k == 1).sum() >= 2
    # on the edge the colour is the edge pixel's own (x == W - 1: the clamped column has weight 0)
    for row in np.flatnonzero(k == 0):
        v, y = int(e["ref"][row]), xy[row, 1]
        iy = int(y)
        want = sc.rgb[v, iy, sc.W - 1].astype(float) + (y - iy) * (sc.rgb[v, min(iy + 1, sc.H - 1), sc.W - 1].astype(float)
                                                                 - sc.rgb[v, iy, sc.W - 1].astype(float))
        assert np.abs(col[row] - want).max() <= 1 / 256


@pytest.mark.parametrize("wid", [4, 5])
@pytest.mark.parametrize("H,W", ws.SIZES)
def test_refinement_hypotheses_leave_through_the_near_border(H, W, wid):
    """The refinement sets (lists from the restatement's own ncc): scored
    hypotheses, hypotheses that leave the image, patches with both; and the
    conditions test_refine_gpu.check_level puts on its inputs: at most 0.5 % of
    the hypotheses in a band, at most 2 % of the patches with a near tie."""
    sc = ws.sphere(H, W)
    s = ws.refine_set(H, W, wid)
    n = len(s["ref"])
    o = wr.warped_batch(sc.gray, sc.K, sc.Rp, sc.t, s["c"], s["nrm"], s["ref"], wid, 0.3)
    views = rr.view_lists(o["ncc"], 0.7, 8)
    dstep = rr.depth_steps(sc.K, sc.Rp, sc.t, s["c"], s["ref"], 1.5)
    mixed = scored = left = hyps = band = near = 0
    for i in range(n):
        r = rr.refine_level_reference(sc.gray, sc.K, sc.Rp, sc.t, s["c"][i], s["nrm"][i], s["ref"][i], views[i],
                                      dstep[i], wid, 0.3, 2, 1)
        hyps += r["H"]
        if not r["valid"]:
            continue
        ok, out = ~np.isnan(r["scores"]), r["border"] < 0
        scored += int(ok.sum())
        left += int(out.sum())
        mixed += bool(ok.any() and out.any())
        inband = (np.abs(r["border"]) < BORDER_BAND) | (r["cosm"] < COS_BAND)
        band += int(inband.sum())
        second = rr.second_best(r["scores"], r["best"])
        if r["best"] >= 0 and not inband.any() and not np.isnan(second):
            tol = (1e-8 / np.minimum(1.0, np.where(r["sigma_b"] > 0, r["sigma_b"], 1.0))).mean(1)
            sb = int(np.flatnonzero(r["scores"] == second)[0])
            near += bool(r["scores"][r["best"]] - second < 2 * max(tol[r["best"]], tol[sb]))
    print(f"{H}x{W} refinement wid {wid}: {n} patches, list lengths up to {int((views >= 0).sum(1).max())}, {hyps} "
          f"hypotheses, {scored} scored, {left} leave the image, {mixed} patches with both, {band} in a band, "
          f"{near} near ties")
    assert scored >= FLOOR_REFINE_SCORED and left >= FLOOR_REFINE_LEAVING and mixed >= 1
    assert band <= 0.005 * hyps and near <= 0.02 * n


@pytest.mark.parametrize("cell,wid", ws.CHAINS)
def test_chains_reach_border_cells(cell, wid):
    sc = ws.sphere(*ws.CHAIN_SIZE)
    ch = ws.cpu_chain(cell, wid)
    own = int(ws.in_border_cells(sc, ch["ref"], ch["cell"], cell).sum())
    bc = ws.border_cell_counts(sc, ch, cell)
    placed = bc["col0"] + bc["colN"] + bc["row0"] + bc["rowN"]
    print(f"chain cell {cell} wid {wid}: {len(ch['ref'])} patches, per round {np.bincount(ch['round']).tolist()}, "
          f"{own} own a border cell, {placed} placements in border cells")
    assert len(ch["ref"]) >= 500
    if (cell, wid) == (2, 3):
        assert own == 0 and placed == 0        # out of reach (warped_shapes.CHAINS)
    else:
        assert own >= 20 and placed >= 100
    m = ws.chain_mixed_set(cell, wid)
    f = sr.filter_chain(*sc.cam(), m["c"], m["nrm"], m["ref"], m["mask"], m["avg"], cell, 2.0, 3, 2, min_support=0.25)
    print(f"  mixed set {np.bincount(m['kind']).tolist()}, removed {f['removed']}, by support {f['removed_support']}")
    assert sum(f["removed"]) > 0 and sum(f["removed_support"]) > 0
