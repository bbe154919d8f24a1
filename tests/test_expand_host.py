"""The float64 restatement of the warped expansion (tests/expand_reference.py)
on its own, without a GPU: the properties the GPU tests rely on when they
compare mvs_wexp_children_device, mvs_wexp_claim_device, mvs_wexp_mark_device
and MvsContext.expand_warped against it."""
import numpy as np
import pytest

import expand_reference as er
import warped_reference as wr

RAD = 0.02


@pytest.fixture(scope="module")
def sphere(pkg):
    rgb, K, R, t = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]
    Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
    return wr.gray_stack(rgb), K, R, t, Rp


def surface_error(c):
    return np.abs(np.sqrt((np.asarray(c) ** 2).sum(1)) - RAD)


def test_claim_rule():
    nan, inf = np.nan, np.inf
    #        job  (p, v, i, j)   accept score
    rows = [((0, 1, 2, 3), 1, 0.5),      # 0  loses to 2
            ((1, 1, 2, 3), 1, 0.9),      # 1  ties with 2: the lower index wins
            ((2, 1, 2, 3), 1, 0.9),      # 2
            ((3, 1, 2, 3), 0, 0.99),     # 3  not accepted
            ((4, 1, 2, 3), 1, nan),      # 4  nan never contends
            ((5, 1, 2, 3), 1, inf),      # 5  nor does inf
            ((6, 0, 0, 0), 1, -0.0),     # 6  -0.0 = +0.0: the lower index wins
            ((7, 0, 0, 0), 1, 0.0),      # 7
            ((8, 2, 5, 5), 1, 0.0),      # 8  +0.0 first: still the lower index
            ((9, 2, 5, 5), 1, -0.0),     # 9
            ((10, 3, 7, 5), 1, -0.3),    # 10 alone, negative
            ((11, 3, 8, 5), 1, 0.4),     # 11 i outside nci = 8
            ((12, 4, 0, 0), 1, 0.4),     # 12 view outside V = 4
            ((13, 3, 7, -1), 1, 0.4),    # 13 j negative
            ((14, 3, 3, 3), 1, nan),     # 14 a cell with no contender at all
            ((15, 3, 3, 3), 0, 0.4)]     # 15
    jobs = np.array([r[0] for r in rows], np.int32)
    accept = np.array([r[1] for r in rows], np.uint8)
    score = np.array([r[2] for r in rows])
    win = er.claim(jobs, accept, score, 4, 8, 6)
    assert win.dtype == np.uint8
    assert np.flatnonzero(win).tolist() == [1, 6, 8, 10]
    # one cell, many contenders: the first of the maxima
    rng = np.random.default_rng(0)
    score = rng.integers(0, 50, 1000) / 50.0
    jobs = np.tile(np.array([[0, 2, 3, 4]], np.int32), (1000, 1))
    win = er.claim(jobs, np.ones(1000, np.uint8), score, 4, 8, 6)
    assert np.flatnonzero(win).tolist() == [int(np.argmax(score))]
    assert er.claim(np.zeros((0, 4), np.int32), np.zeros(0, np.uint8), np.zeros(0), 4, 8, 6).shape == (0,)


def _fronto():
    """One camera looking down +z at the plane z = 0.5, normal towards it."""
    W, H = 64, 48
    K = np.array([[[300.0, 0, 31.3], [0, 310.0, 23.9], [0, 0, 1.0]]])
    Rp = np.eye(3)[None]
    t = np.array([[0.01, -0.02, 0.0]])
    return W, H, K, Rp, t


@pytest.mark.parametrize("cell", [1, 2, 3, 4])
def test_children_on_a_fronto_parallel_plane(cell):
    W, H, K, Rp, t = _fronto()
    nci, ncj = er.grid_shape(W, H, cell)
    z = 0.5
    c = np.array([[(30.4 - K[0, 0, 2]) / K[0, 0, 0] * z, (20.7 - K[0, 1, 2]) / K[0, 1, 1] * z, z]]) - t[0]
    nrm = np.array([[1e-17, -0.0, -1.0]])          # bits that only a copy preserves
    occ = np.zeros((1, ncj, nci), np.uint8)
    jobs, cc, cn, cref = er.children(K, Rp, t, W, H, c, nrm, [0], np.zeros((1, 1), np.uint64), cell, occ, 1.0)
    i, j = 30 // cell, 20 // cell
    assert jobs.tolist() == [[0, 0, i + 1, j], [0, 0, i - 1, j], [0, 0, i, j + 1], [0, 0, i, j - 1]]
    assert cref.tolist() == [0, 0, 0, 0]
    for k in range(4):
        assert cn[k].tobytes() == nrm[0].tobytes()
        x, y, depth = wr.project_ref(K[0], Rp[0], t[0], cc[k])
        assert abs(x - (jobs[k, 2] * cell + (cell - 1) / 2)) <= 1e-9
        assert abs(y - (jobs[k, 3] * cell + (cell - 1) / 2)) <= 1e-9
        assert abs(depth - z) <= 1e-12             # the child stays on the plane
    # occupancy, max_dist and a backward normal each remove children
    occ[0, j, i + 1] = 1
    assert er.children(K, Rp, t, W, H, c, nrm, [0], np.zeros((1, 1), np.uint64), cell, occ, 1.0)[0][:, 2:].tolist() \
        == [[i - 1, j], [i, j + 1], [i, j - 1]]
    assert len(er.children(K, Rp, t, W, H, c, nrm, [0], np.zeros((1, 1), np.uint64), cell, occ, 1e-6)[0]) == 0
    # a grazing plane that contains the ray of a pixel between the patch and cell i + 1:
    # the ray of that cell's centre meets it behind the camera (s < 0)
    xm = (max(30.4, i * cell + (cell - 1) / 2) + (i + 1) * cell + (cell - 1) / 2) / 2
    grazing = np.array([[1.0, 0.0, -(xm - K[0, 0, 2]) / K[0, 0, 0]]])
    grazing /= np.linalg.norm(grazing)
    got = er.children(K, Rp, t, W, H, c, grazing, [0], np.zeros((1, 1), np.uint64), cell, np.zeros_like(occ), 1e3)[0]
    assert got[:, 2:].tolist() == [[i - 1, j], [i, j + 1], [i, j - 1]]


def test_children_at_the_grid_border_and_past_the_last_cell():
    """128 % 3 != 0: columns 126, 127 belong to no cell; a patch there has no children."""
    W, H, K, Rp, t = _fronto()
    cell = 3
    nci, ncj = er.grid_shape(W, H, cell)
    assert (nci, ncj) == (21, 16) and nci * cell < W
    z = 0.5
    def at(x, y):
        return np.array([(x - K[0, 0, 2]) / K[0, 0, 0] * z, (y - K[0, 1, 2]) / K[0, 1, 1] * z, z]) - t[0]
    c = np.array([at(63.5, 20.5), at(0.5, 0.5), at(62.5, 47.5), at(-0.5, 3.0)])
    nrm = np.tile([0, 0, -1.0], (4, 1))
    occ = np.zeros((1, ncj, nci), np.uint8)
    jobs = er.children(K, Rp, t, W, H, c, nrm, [0, 0, 0, 0], np.zeros((4, 1), np.uint64), cell, occ, 1.0)[0]
    assert jobs.tolist() == [[1, 0, 1, 0], [1, 0, 0, 1], [2, 0, 19, 15], [2, 0, 20, 14]]


@pytest.mark.parametrize("cell", [1, 3])
def test_mark_uses_the_job_cell_for_the_reference_view(cell):
    """At odd cell sizes a child's centre projects onto an integer pixel, and
    int() of the reprojection may fall one pixel short: the job's own cell is
    filled as the job names it."""
    W, H, K, Rp, t = _fronto()
    nci, ncj = er.grid_shape(W, H, cell)
    z = 0.5
    i, j = 7, 5
    qx, qy = i * cell + (cell - 1) / 2, j * cell + (cell - 1) / 2
    assert qx == int(qx)
    short = np.array([[(qx - 1e-9 - K[0, 0, 2]) / K[0, 0, 0] * z, (qy - K[0, 1, 2]) / K[0, 1, 1] * z, z]]) - t[0]
    assert int(wr.project_ref(K[0], Rp[0], t[0], short[0])[0]) == int(qx) - 1
    jobs = np.array([[0, 0, i, j], [0, 0, i + 2, j]], np.int32)
    cc = np.vstack([short, short])
    occ = np.zeros((1, ncj, nci), np.uint8)
    occ[0, 0, 0] = 7                                   # a pre-set byte stays as it is
    er.mark(K, Rp, t, W, H, jobs, [1, 0], cc, [0, 0], np.zeros((2, 1), np.uint64), cell, occ)
    want = np.zeros_like(occ)
    want[0, 0, 0] = 7
    want[0, j, i] = 1
    assert np.array_equal(occ, want)
    # with the view in the mask as well, the reprojection's cell is filled too
    er.mark(K, Rp, t, W, H, jobs, [1, 0], cc, [0, 0], np.ones((2, 1), np.uint64), cell, occ)
    want[0, j, (int(qx) - 1) // cell] = 1
    assert np.array_equal(occ, want)


def test_fast_scorer_is_the_restatement(sphere):
    """score_batch_fast against score_batch (warped_reference itself) on sphere
    patches on and off the surface: the same nan pattern, ncc within 1e-12,
    masks equal away from a 1e-12 band around min_ncc."""
    gray, K, R, t, Rp = sphere
    c, nrm, ref, _ = wr.sphere_patches(K, R, t, 64, RAD, np.random.default_rng(3), (0.0, 0.001, -0.001))
    c[5] = 10.0                                   # outside every image
    slow = er.score_batch(gray, K, Rp, t, c, nrm, ref, 3, 0.7, 0.3)
    fast = er.score_batch_fast(gray, K, Rp, t, c, nrm, ref, 3, 0.7, 0.3)
    assert np.array_equal(np.isnan(slow[3]), np.isnan(fast[3]))
    both = ~np.isnan(slow[3])
    assert both.sum() > 400 and np.abs(slow[3][both] - fast[3][both]).max() <= 1e-12
    sure = np.all(~both | (np.abs(np.where(both, slow[3], 0.0) - 0.7) > 1e-12), 1)
    assert sure.sum() >= 60
    assert np.array_equal(slow[0][sure], fast[0][sure]) and np.array_equal(slow[1][sure], fast[1][sure])
    assert np.abs(slow[2][sure] - fast[2][sure]).max() <= 1e-12


@pytest.fixture(scope="module")
def chains(sphere):
    """4 exact on-surface seeds (seed 1), 3 rounds, wid 3, cell 2: without and
    with two refinement levels (lists of 4 views, which halves the restatement's
    time: about 20 s for both chains).  Measured: 442 patches, median surface
    error per round 0.000, 0.029, 0.130 mm, against 474 patches, 0.000, 0.039,
    0.088 mm (lists of 8 views: 480 patches, 0.000, 0.065, 0.076 mm)."""
    gray, K, R, t, Rp = sphere
    c, nrm, ref, _ = wr.sphere_patches(K, R, t, 4, RAD, np.random.default_rng(1))
    kw = dict(cell=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2, scorer=er.score_batch_fast)
    plain = er.expand_chain(gray, K, Rp, t, c, nrm, ref, 3, **kw)
    refined = er.expand_chain(gray, K, Rp, t, c, nrm, ref, 3, refine_levels=2, max_views=4, **kw)
    return plain, refined


def test_sphere_chain_without_refinement(chains):
    plain, _ = chains
    per_round = np.bincount(plain["round"], minlength=3)
    print("patches per round", per_round.tolist())
    assert np.all(np.diff(np.cumsum(per_round)) > 0) and per_round[0] > 0
    owner = np.column_stack([plain["ref"], plain["cell"]])
    assert len(np.unique(owner, axis=0)) == len(owner)
    assert np.all(plain["count"] >= 2)
    # a child's parent is a patch of the round before
    kids = plain["parent"] >= 0
    assert np.array_equal(kids, plain["round"] > 0)
    assert np.array_equal(plain["round"][plain["parent"][kids]], plain["round"][kids] - 1)
    # every owned cell is taken
    assert np.all(plain["occ"][plain["ref"], plain["cell"][:, 1], plain["cell"][:, 0]] == 1)


def test_sphere_chain_refinement_stays_on_the_surface(chains):
    """Median distance to the sphere of the last round's patches, true
    rodrigues_roundtrip rotations: 4 seeds, 3 rounds, wid 3, cell 2."""
    plain, refined = chains
    last_p = surface_error(plain["c"][plain["round"] == 2])
    last_r = surface_error(refined["c"][refined["round"] == 2])
    for name, ch in (("plain", plain), ("refine_levels=2", refined)):
        med = [float(np.median(surface_error(ch["c"][ch["round"] == r]))) * 1e3 for r in range(3)]
        print(f"{name}: {len(ch['ref'])} patches, median surface error per round (mm)",
              " ".join(f"{m:.4f}" for m in med))
    assert len(last_p) and len(last_r)
    assert np.median(last_r) < np.median(last_p)
    owner = np.column_stack([refined["ref"], refined["cell"]])
    assert len(np.unique(owner, axis=0)) == len(owner) and np.all(refined["count"] >= 2)
