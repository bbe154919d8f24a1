"""The restatement of the resumed expansion and of the expand -> filter loop
(tests/loop_reference.py) on its own, without a GPU: the property that makes
resumption testable exactly -- resuming k rounds from the set of R rounds gives
the set of R + k rounds -- and the parent renumbering."""
import numpy as np
import pytest

import expand_reference as er
import loop_reference as lr
import support_reference as sr
import warped_reference as wr

RAD = 0.02
KW = dict(cell=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2)
NOTHING = dict(min_views=0, adj_px=1e9, min_support=0.0, min_neigh=0)     # a filter that removes nothing


def same_set(a, b):
    for k in lr.KEYS + ("occ",):
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape, k
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).astype(np.asarray(a[k]).dtype).tobytes(), k


@pytest.fixture(scope="module")
def chains(pkg):
    m = sr.sphere_mixed(pkg, RAD)
    cam = (m["gray"], m["K"], m["Rp"], m["t"])
    c0, n0, r0, _ = wr.sphere_patches(m["K"], m["R"], m["t"], 4, RAD, np.random.default_rng(1))
    two = er.expand_chain(*cam, c0, n0, r0, 2, scorer=er.score_batch_fast, **KW)
    four = er.expand_chain(*cam, c0, n0, r0, 4, scorer=er.score_batch_fast, **KW)
    return cam, (c0, n0, r0), two, four


def test_resuming_two_rounds_gives_the_four_round_chain(chains):
    cam, _, two, four = chains
    got = lr.resume(*cam, two, 2, scorer=er.score_batch_fast, **KW)
    assert len(four["ref"]) > len(two["ref"]) > 4 and four["round"].max() == 3
    same_set(four, got)
    assert got["max_dist"] == four["max_dist"]
    # one round at a time, and without the set's occ (rebuilt from the rows)
    one = lr.resume(*cam, two, 1, scorer=er.score_batch_fast, **KW)
    same_set(four, lr.resume(*cam, one, 1, scorer=er.score_batch_fast, **KW))
    bare = {k: v for k, v in two.items() if k != "occ"}
    same_set(four, lr.resume(*cam, bare, 2, scorer=er.score_batch_fast, **KW))


def test_zero_rounds_is_the_identity(chains):
    cam, _, two, _ = chains
    same_set(two, lr.resume(*cam, two, 0, scorer=er.score_batch_fast, **KW))
    # max_patches counts the input: no room, no round
    same_set(two, lr.resume(*cam, two, 2, scorer=er.score_batch_fast, max_patches=len(two["ref"]), **KW))
    some = lr.resume(*cam, two, 2, scorer=er.score_batch_fast, max_patches=len(two["ref"]) + 5, **KW)
    assert len(some["ref"]) == len(two["ref"]) + 5


def test_dead_rows_and_cells_outside_the_grid_are_refused(chains):
    cam, _, two, _ = chains
    bad = dict(two, ref=np.where(np.arange(len(two["ref"])) == 1, -1, two["ref"]))
    with pytest.raises(ValueError):
        lr.resume(*cam, bad, 1, scorer=er.score_batch_fast, **KW)
    cell = two["cell"].copy()
    cell[0, 0] = 128 // 2
    with pytest.raises(ValueError):
        lr.resume(*cam, dict(two, cell=cell), 1, scorer=er.score_batch_fast, **KW)


def test_a_loop_whose_filter_removes_nothing_is_the_chain(chains):
    cam, (c0, n0, r0), _, four = chains
    got = lr.reconstruct(*cam, c0, n0, r0, iterations=2, rounds=2, resume_rounds=2, expand=KW, filter=NOTHING,
                         scorer=er.score_batch_fast)
    same_set(four, got)
    assert np.array_equal(got["index"], np.arange(len(four["ref"]))) and got["keep"].all()
    h = got["history"]
    assert [x["removed"] for x in h] == [[0], [0]] and [x["removed_support"] for x in h] == [[0], [0]]
    assert h[0]["resumed"] == len(four["ref"]) == h[1]["patches"] and h[1]["resumed"] is None


def test_parent_renumbering(chains, pkg):
    parent = np.array([-1, 0, 0, 1, 2, -2, 4, -1], np.int64)
    index = np.array([0, 2, 4, 5, 6, 7])
    want = [-1, 0, 1, -2, 2, -1]              # rows 1 and 3 are gone: old rows 2 -> 1, 4 -> 2; an earlier -2 stays
    assert lr.renumber(parent[index], index, 8).tolist() == want
    assert pkg.MvsContext.renumber_parents(parent[index], index, 8).tolist() == want
    # a removed parent
    assert lr.renumber(parent[[3]], [3], 8).tolist() == [-2]
    assert pkg.MvsContext.renumber_parents(parent[[3]], [3], 8).tolist() == [-2]
    # on a chain: every surviving parent still names the same patch
    _, _, _, four = chains
    n = len(four["ref"])
    index = np.flatnonzero(np.arange(n) % 3 != 1)
    new = pkg.MvsContext.renumber_parents(four["parent"][index], index, n)
    assert np.array_equal(new, lr.renumber(four["parent"][index], index, n))
    for k, old in zip(new, four["parent"][index]):
        assert (k == -1 and old == -1) or (k == -2 and old % 3 == 1) or (k >= 0 and index[k] == old)
    assert (new == -2).any() and (new >= 0).any()
