"""The support passes of MvsContext.filter_warped, the resumed expansion
(MvsContext.resume_warped) and the expand -> filter loop
(MvsContext.reconstruct_warped) on the GPU.

Exact comparisons: filter_warped(min_support=...) against the restatement's
chain (tests/support_reference.py); resume_warped(expand_warped(R), k) against
expand_warped(R + k) of the same context, array by array and byte by byte;
the loop with a filter that removes nothing against the uninterrupted chain.
With the real filter the loop is held against tests/loop_reference.py by the
bound tests/test_expand_gpu.py uses for chains (the scorers differ in the last
bits of an ncc, and a differing decision cascades).
"""
import numpy as np
import pytest

import expand_reference as er
import loop_reference as lr
import support_reference as sr
import warped_reference as wr
from test_wfilt_gpu import RAD, Scene

pytestmark = pytest.mark.gpu

KW = dict(cell_size=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2)
KW_CPU = dict(cell=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2)
NOTHING = dict(min_views=0, adj_px=1e9, min_support=0.0, min_neigh=0)      # a filter that removes nothing
REAL = dict(adj_px=2.0, min_views=3, passes=2, min_support=0.25, min_neigh=1)
SET_KEYS = lr.KEYS + ("occ",)


@pytest.fixture(scope="module")
def sphere(pkg):
    m = sr.sphere_mixed(pkg, RAD)
    s = Scene(pkg, m["rgb"], m["K"], m["R"], m["t_raw"])
    assert np.array_equal(s.Rp, m["Rp"])
    s.gray = m["gray"]
    yield s
    s.ctx.close()


@pytest.fixture(scope="module")
def seeds(sphere):
    s = sphere
    c, nrm, ref, _ = wr.sphere_patches(s.K, s.R, s.t, 8, RAD, np.random.default_rng(1))
    return c, nrm, ref


@pytest.fixture(scope="module", params=[0, 2], ids=["unrefined", "refined"])
def chains(request, sphere, seeds):
    """expand_warped for 2 and for 4 rounds, without and with two refinement levels."""
    kw = dict(KW, refine_levels=request.param)
    return kw, sphere.ctx.expand_warped(*seeds, 2, **kw), sphere.ctx.expand_warped(*seeds, 4, **kw)


def same_set(a, b, keys=SET_KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------
# 1. filter_warped with support passes
# ---------------------------------------------------------------------------
def test_filter_with_support_is_the_restatement(pkg, sphere):
    s = sphere
    m = sr.sphere_mixed(pkg, RAD)["set"]
    patches = {k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")}
    for kw in (dict(min_support=0.25), dict(min_support=0.5, min_neigh=30, support_passes=4),
               dict(min_support=1.0, support_passes=0)):
        a = s.ctx.filter_warped(patches, **kw)
        b = pkg.filter_patches_warped(s.ctx, patches, **kw)
        want = sr.filter_chain(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], m["avg"], 2, 2.0, 3, 2, **kw)
        assert a["removed"] == want["removed"] and a["removed_support"] == want["removed_support"], kw
        for k in ("keep", "vis", "conf", "front", "nb", "adj"):
            assert a[k].dtype == want[k].dtype and np.array_equal(a[k], want[k]), (kw, k)
        assert a["zfront"].tobytes() == want["zfront"].tobytes()
        idx = np.flatnonzero(want["keep"])
        assert np.array_equal(a["index"], idx)
        for k in patches:
            assert np.array_equal(a[k], m[k][idx]), k
        assert np.array_equal(a["occ"], lr.occ_of(*s.cam(), m["ref"][idx], m["cell"][idx], m["c"][idx], m["mask"][idx], 2))
        for k in a:                                       # two runs are bit-identical
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), k
            else:
                assert a[k] == b[k], k
        print(f"{kw}: removed {a['removed']}, removed_support {a['removed_support']}, {len(idx)} survive")
    assert len(a["removed_support"]) == 0 and not a["nb"].any()
    many = s.ctx.filter_warped(patches, min_support=0.5, min_neigh=30, support_passes=4)
    assert 1 < len(many["removed_support"]) <= 4 and many["removed_support"][0] > 0


def test_filter_without_support_is_unchanged(pkg, sphere):
    """min_support None: the keys and every value of the call as it was."""
    s = sphere
    m = sr.sphere_mixed(pkg, RAD)["set"]
    patches = {k: m[k] for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")}
    a = s.ctx.filter_warped(patches, cell_size=2, adj_px=2.0, min_views=3, passes=2)
    assert list(a) == ["c", "nrm", "ref", "mask", "avg", "cell", "kind", "keep", "vis", "conf", "front", "zfront",
                       "occ", "index", "removed"]
    want = sr.filter_chain(*s.cam(), m["c"], m["nrm"], m["ref"], m["mask"], m["avg"], 2, 2.0, 3, 2)
    assert a["removed"] == want["removed"]
    for k in ("keep", "vis", "conf", "front"):
        assert np.array_equal(a[k], want[k]), k
    assert a["zfront"].tobytes() == want["zfront"].tobytes()
    # min_neigh and support_passes alone switch nothing on
    b = s.ctx.filter_warped(patches, min_neigh=5, support_passes=3)
    assert list(b) == list(a) and all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------
# 2. the resumed expansion
# ---------------------------------------------------------------------------
def test_resuming_two_rounds_gives_the_four_round_chain(pkg, sphere, chains):
    kw, two, four = chains
    got = sphere.ctx.resume_warped(two, 2, **kw)
    print(f"refine_levels {kw['refine_levels']}: {len(two['ref'])} patches after 2 rounds, {len(four['ref'])} after 4")
    assert len(four["ref"]) > len(two["ref"]) > 8 and four["round"].max() == 3
    same_set(four, got)
    assert got["max_dist"] == four["max_dist"]
    # one round at a time, through the thin wrapper
    one = pkg.resume_patches_warped(sphere.ctx, two, 1, cell_size=2, MIN_NCC=0.7, wid=3, min_cos=0.3, vlb=2,
                                    refine_levels=kw["refine_levels"])
    assert len(two["ref"]) < len(one["ref"]) < len(four["ref"])
    same_set(four, sphere.ctx.resume_warped(one, 1, **kw))


def test_zero_rounds_and_a_set_without_occ(sphere, chains):
    kw, two, four = chains
    same_set(two, sphere.ctx.resume_warped(two, 0, **kw))
    bare = {k: v for k, v in two.items() if k not in ("occ", "max_dist")}
    same_set(two, sphere.ctx.resume_warped(bare, 0, **kw))             # occ rebuilt from the rows
    got = sphere.ctx.resume_warped(bare, 2, max_dist=two["max_dist"], **kw)
    same_set(four, got)
    # max_dist by expand_warped's rule on the first row: the chain's when that row is the unrefined first seed
    guess = sphere.ctx.resume_warped(bare, 0, **kw)["max_dist"]
    assert 0.5 * two["max_dist"] < guess < 2 * two["max_dist"]


def test_max_patches_counts_the_input(sphere, chains):
    kw, two, four = chains
    n2 = len(two["ref"])
    same_set(two, sphere.ctx.resume_warped(two, 2, max_patches=n2, **kw))
    same_set(two, sphere.ctx.resume_warped(two, 2, max_patches=n2 - 3, **kw))
    some = sphere.ctx.resume_warped(two, 2, max_patches=n2 + 5, **kw)
    assert len(some["ref"]) == n2 + 5
    if kw["refine_levels"] == 0:
        for k in lr.KEYS:
            assert some[k].tobytes() == four[k][:n2 + 5].tobytes(), k


def test_refused_sets(sphere, chains):
    kw, two, _ = chains
    ref = two["ref"].copy()
    ref[1] = -1
    with pytest.raises(RuntimeError, match="dead"):
        sphere.ctx.resume_warped(dict(two, ref=ref), 1, **kw)
    ref[1] = sphere.V
    with pytest.raises(RuntimeError, match="dead"):
        sphere.ctx.resume_warped(dict(two, ref=ref), 1, **kw)
    for i, j in ((sphere.W // 2, 0), (0, sphere.H // 2), (-1, 0)):
        cell = two["cell"].copy()
        cell[0] = (i, j)
        with pytest.raises(RuntimeError, match="outside the grid"):
            sphere.ctx.resume_warped(dict(two, cell=cell), 1, **kw)
    with pytest.raises(RuntimeError, match="no 'parent'"):
        sphere.ctx.resume_warped({k: v for k, v in two.items() if k != "parent"}, 1, **kw)


# ---------------------------------------------------------------------------
# 3. the loop
# ---------------------------------------------------------------------------
def test_a_loop_whose_filter_removes_nothing_is_the_chain(pkg, sphere, seeds, chains):
    kw, _, four = chains
    got = pkg.reconstruct_patches_warped(sphere.ctx, *seeds, iterations=2, rounds=2, resume_rounds=2, expand=kw,
                                         filter=NOTHING)
    same_set(four, got)
    assert np.array_equal(got["index"], np.arange(len(four["ref"]))) and got["keep"].all()
    h = got["history"]
    assert [x["removed"] for x in h] == [[0], [0]] and [x["removed_support"] for x in h] == [[0], [0]]
    assert h[0]["resumed"] == len(four["ref"]) == h[1]["patches"] and h[1]["resumed"] is None
    # three iterations of one round each: 2 + 1 + 1 rounds
    got = sphere.ctx.reconstruct_warped(*seeds, iterations=3, rounds=2, resume_rounds=1, expand=kw, filter=NOTHING)
    same_set(four, got)


def test_the_loop_on_a_set_with_planted_outliers(pkg, sphere):
    """The chain of the quality experiment with 114 of its patches moved 2 mm
    off the surface, two iterations with one resumed round between them: the
    filter removes wrong patches and the resumption refills freed cells.  The
    GPU loop is deterministic, keeps one patch per (ref, cell), returns the
    occupancy of its rows and shares at least 98 % of its (ref, cell) set with
    the restatement's loop."""
    s = sphere
    start, src = lr.planted_set(pkg, RAD)
    runs = [s.ctx.reconstruct_warped(None, None, None, iterations=2, resume_rounds=1, expand=KW, filter=REAL,
                                     start=start) for _ in range(2)]
    a, b = runs
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k
    owners = {(int(r), int(i), int(j)) for r, (i, j) in zip(a["ref"], a["cell"])}
    assert len(owners) == len(a["ref"])
    assert np.array_equal(a["occ"], lr.occ_of(*s.cam(), a["ref"], a["cell"], a["c"], a["mask"], 2))
    h = a["history"]
    assert h[0]["patches"] == len(start["ref"]) and sum(h[0]["removed"]) + sum(h[0]["removed_support"]) > 0
    assert h[0]["resumed"] > h[0]["patches"] - sum(h[0]["removed"]) - sum(h[0]["removed_support"])
    assert ((a["parent"] >= -2) & (a["parent"] < len(a["ref"]))).all()
    cpu = lr.reconstruct(s.gray, s.K, s.Rp, s.t, None, None, None, iterations=2, resume_rounds=1, expand=KW_CPU,
                         filter=REAL, scorer=er.score_batch_fast, start=start)
    r = {(int(x), int(i), int(j)) for x, (i, j) in zip(cpu["ref"], cpu["cell"])}
    share = len(owners & r) / max(len(owners), len(r))
    print(f"GPU loop {len(owners)} patches, restatement loop {len(r)}, shared {len(owners & r)} = {share:.4f} of the "
          f"larger set; history GPU {h}, restatement {cpu['history']}; {len(src)} planted")
    assert share >= 0.98
