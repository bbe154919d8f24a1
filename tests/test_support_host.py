"""The float64 restatement of the neighbour-support test
(tests/support_reference.py) on its own, without a GPU: the rules the GPU tests
rely on when they compare mvs_wfilt_support_device and
MvsContext.filter_warped(min_support=...) against it, and the quality
experiment that the support filter's parameters come from."""
import numpy as np
import pytest

import filter_reference as fr
import support_reference as sr
from test_wfilt_host import K, RP, T, TOWARDS0, W, H, quality_counts

NCI, NCJ = W // 2, H // 2
MIN_SUPPORT, MIN_NEIGH = 0.25, 1          # the chain's settings in the quality experiment (PMVS's ratio)


def at(px, py, z=0.5):
    """The point of view 0's pixel (px, py) at depth z; (31.3, 23.9) is cell (15, 11) at cell size 2."""
    return [(px - 31.3) / 300.0 * z, (py - 23.9) / 310.0 * z, z]


CENTRE, RIGHT, LEFT, UP, DOWN = (31.3, 23.9), (33.0, 23.9), (29.0, 23.9), (31.3, 21.0), (31.3, 25.0)


def run(c, mask=None, nrm=None, adj_px=1.0, min_support=0.25, min_neigh=1, front=None, ref=None):
    c = np.asarray(c, np.float64).reshape(-1, 3)
    n = len(c)
    nrm = np.tile(TOWARDS0, (n, 1)) if nrm is None else np.asarray(nrm, np.float64)
    ref = np.zeros(n, np.int32) if ref is None else np.asarray(ref, np.int32)
    mask = np.zeros((n, 1), np.uint64) if mask is None else np.asarray(mask, np.uint64).reshape(n, 1)
    if front is None:
        front = fr.front_grid(K, RP, T, W, H, c, ref, mask, 2)[0]
    nb, adj, keep = sr.support(K, RP, T, W, H, c, nrm, ref, mask, 2, adj_px, min_support, min_neigh, front)
    return nb.tolist(), adj.tolist(), keep.tolist()


def test_a_lone_patch_has_no_neighbour():
    assert run([at(*CENTRE)]) == ([0], [0], [0])
    assert run([at(*CENTRE)], min_neigh=0) == ([0], [0], [1])
    assert run([at(*CENTRE)], min_neigh=0, min_support=1.0) == ([0], [0], [1])     # 0 >= 1.0 * 0
    # a dead row: N = A = 0 and never kept
    assert run([at(*CENTRE), at(*RIGHT)], ref=[-1, 0], min_neigh=0) == ([0, 0], [0, 0], [0, 1])
    assert run([at(*CENTRE), at(*RIGHT)], ref=[2, 0], min_neigh=0) == ([0, 0], [0, 0], [0, 1])


def test_corner_and_edge_cells_see_three_and_five_cells():
    """A grid that names patch 1 everywhere: N is the number of neighbour cells inside the grid."""
    front = np.ones((2, NCJ, NCI), np.int32)
    for pixel, cells in (((0.5, 0.5), 3), ((33.0, 0.5), 5), ((0.5, 25.0), 5), (CENTRE, 8),
                         ((W - 0.5, H - 0.5), 3), ((W - 0.5, 25.0), 5)):
        nb, adj, keep = run([at(*pixel), at(*CENTRE)], front=front)
        assert nb[0] == cells and adj[0] == cells and keep[0] == 1, pixel     # coplanar: d.n = 0
    # seen in both views: once per view
    nb, adj, _ = run([at(0.5, 0.5), at(*CENTRE)], mask=[3, 0], front=front)
    assert nb[0] == 3 + 3 and adj[0] == 6


def test_coplanar_neighbours_support_each_other():
    nb, adj, keep = run([at(*CENTRE), at(*RIGHT)], mask=[3, 3], min_support=1.0)
    assert nb == [2, 2] and adj == [2, 2] and keep == [1, 1]                     # one incidence per view
    nb, adj, keep = run([at(*CENTRE), at(*RIGHT)], min_support=1.0)
    assert nb == [1, 1] and adj == [1, 1] and keep == [1, 1]


def test_a_neighbour_behind_counts_in_n_only():
    """2 mm behind at adj_px 1: |d.n| + |d.n| = 4 mm against 2 rho = 2 * 0.5 / 305 = 3.3 mm."""
    assert 0.004 > 2 * (1.0 * 0.502) / 305.0
    nb, adj, keep = run([at(*CENTRE), at(*RIGHT, z=0.502)], mask=[3, 3])
    assert nb == [2, 2] and adj == [0, 0] and keep == [0, 0]
    # a wider footprint makes them adjacent again
    assert run([at(*CENTRE), at(*RIGHT, z=0.502)], mask=[3, 3], adj_px=2.0)[1] == [2, 2]
    # adj_px 0: nothing is adjacent, not even a coplanar neighbour
    assert run([at(*CENTRE), at(*RIGHT)], adj_px=0.0)[1] == [0, 0]


def test_a_nan_normal_is_never_adjacent():
    nan = [np.nan, 0.0, -1.0]
    nb, adj, keep = run([at(*CENTRE), at(*RIGHT)], nrm=[TOWARDS0, nan], min_support=0.25)
    assert nb == [1, 1] and adj == [0, 0] and keep == [0, 0]
    assert run([at(*CENTRE), at(*RIGHT)], nrm=[TOWARDS0, nan], min_support=0.0)[2] == [1, 1]


def test_min_support_zero_and_one():
    both = [at(*CENTRE), at(*RIGHT), at(*LEFT)]
    one_behind = [at(*CENTRE), at(*RIGHT), at(*LEFT, z=0.502)]
    assert run(both, min_support=1.0) == ([2, 1, 1], [2, 1, 1], [1, 1, 1])           # A = N
    nb, adj, keep = run(one_behind, min_support=1.0)
    assert (nb[0], adj[0], keep[0]) == (2, 1, 0)                                      # A = N - 1
    assert run(one_behind, min_support=0.0)[2] == [1, 1, 1]
    assert run(one_behind, min_support=0.5)[2][0] == 1                                # 1 >= 0.5 * 2


def test_the_ratio_boundary():
    four = [at(*CENTRE), at(*RIGHT), at(*LEFT, z=0.502), at(*UP, z=0.502), at(*DOWN, z=0.502)]
    nb, adj, keep = run(four, min_support=0.25)
    assert (nb[0], adj[0], keep[0]) == (4, 1, 1)                                      # 1 >= 0.25 * 4
    three = [at(*CENTRE), at(*LEFT, z=0.502), at(*UP, z=0.502), at(*DOWN, z=0.502)]
    nb, adj, keep = run(three, min_support=0.25)
    assert (nb[0], adj[0], keep[0]) == (3, 0, 0)                                      # 0 < 0.75
    # min_neigh counts incidences
    assert run(four, min_support=0.25, min_neigh=4)[2][0] == 1
    assert run(four, min_support=0.25, min_neigh=5)[2][0] == 0


def test_incidences_are_counted_not_patches():
    """One patch in front in all eight cells around p, in both views: 16 incidences."""
    front = np.full((2, NCJ, NCI), -1, np.int32)
    front[:, 10:13, 14:17] = 1
    front[:, 11, 15] = 0
    nb, adj, keep = run([at(*CENTRE), at(*RIGHT)], mask=[3, 0], front=front, min_neigh=16, min_support=1.0)
    assert (nb[0], adj[0], keep[0]) == (16, 16, 1)
    assert nb[1] == 1             # around cell (16, 11) of view 0 the grid names 1 itself (skipped), 0 once and -1


def test_a_grid_that_names_p_beside_itself_is_skipped():
    front = np.full((2, NCJ, NCI), -1, np.int32)
    front[0, 11, 16] = 0          # p = 0 itself in its right neighbour cell
    front[0, 11, 14] = 1
    front[0, 10, 15] = 7          # outside -1..n-1: reads as -1
    front[0, 12, 15] = -5
    nb, adj, keep = run([at(*CENTRE), at(*LEFT)], front=front)
    assert (nb[0], adj[0], keep[0]) == (1, 1, 1)


def test_refused_scalars():
    for bad in (dict(min_support=np.nan), dict(min_support=-0.1), dict(min_support=1.5), dict(min_neigh=-1)):
        with pytest.raises(ValueError):
            run([at(*CENTRE)], **bad)


@pytest.fixture(scope="module")
def quality(pkg):
    m = sr.sphere_mixed(pkg)
    s = m["set"]
    args = (m["K"], m["Rp"], m["t"], m["W"], m["H"], s["c"], s["nrm"], s["ref"], s["mask"], s["avg"], 2, 2.0, 3)
    vis = sr.filter_chain(*args, passes=2)
    out = {ms: sr.filter_chain(*args, passes=2, min_support=ms, min_neigh=MIN_NEIGH) for ms in (0.25, 0.5)}
    return s, vis, out


def test_quality_on_the_sphere_chain(quality):
    """filter_reference.mixed_set (true rodrigues_roundtrip rotations): two
    visibility passes (adj_px 2, min_views 3), then one support pass at
    min_support 0.25, min_neigh 1.  At least 98 % of the chain patches are kept
    and at most half as many outliers as the visibility passes alone keep.
    Measured: the visibility passes keep 441/442 chain patches and 8/39 + 7/75
    outliers (15); the support pass at 0.25 removes 8 more and leaves 441/442
    and 7/39 + 0/75 (7); at 0.5 it removes 11 and leaves 441/442 and 4/39 + 0/75
    (4).  A/N of the chain patches: minimum 0.66, median 1.0; of the outliers
    that reach the support pass: median 0.17.  0.25 is PMVS's value and the one
    further from the chain's minimum (0.51 in the experiment the issue quotes)."""
    s, vis, out = quality
    kind = s["kind"]
    (ck, cn), (ok, on), (ik, inn) = quality_counts(kind, vis["keep"])
    print(f"visibility alone: chain {ck}/{cn}, outliers outside {ok}/{on}, inside {ik}/{inn}, removed {vis['removed']}")
    base = ok + ik
    for ms, res in out.items():
        (ck, cn), (ok, on), (ik, inn) = quality_counts(kind, res["keep"])
        live = res["nb"] > 0
        ratio = res["adj"][live] / res["nb"][live]
        print(f"support {ms}: chain {ck}/{cn}, outliers outside {ok}/{on}, inside {ik}/{inn}, removed_support "
              f"{res['removed_support']}; A/N chain min {ratio[kind[live] == 0].min():.3f} median "
              f"{np.median(ratio[kind[live] == 0]):.3f}, outliers median "
              f"{np.median(ratio[kind[live] > 0]) if (kind[live] > 0).any() else float('nan'):.3f}")
    res = out[MIN_SUPPORT]
    (ck, cn), (ok, on), (ik, inn) = quality_counts(kind, res["keep"])
    assert cn > 400 and on + inn > 80 and base > 0
    assert ck >= 0.98 * cn
    assert 2 * (ok + ik) <= base
    # the support pass only removes, and nb, adj cover the input
    assert np.all(res["keep"] <= vis["keep"]) and len(res["removed_support"]) == 1
    assert res["removed_support"][0] == int(vis["keep"].sum()) - int(res["keep"].sum())
    assert np.all(res["adj"] <= res["nb"]) and not res["nb"][vis["keep"] == 0].any()
