"""The host-pointer calls share one staging arena per context (csrc/mvs_host.h,
Staging): every call must give what it gives on a context nothing else has
used, whatever family's bytes the arena holds when it starts.

One context (the subject) runs the calls back to back; each result is compared,
bit for bit, with the same call on a context created for it alone (the
witness).  The row counts are odd (1, 3, 5, 257, 4099), so the 4-byte and 1-byte
arrays end off an 8-byte boundary.  On the 24 x 96 x 128 sphere scene the front
grids of cell size 2 hold 73,728 cells: mvs_wfilt_front stages 894,720 B
(256-B slots), the most of any call before the last, and the last
(mvs_score_warped at n = 4099 with per-view ncc) 1,149,440 B: it grows the
arena in the middle of the sequence."""
import numpy as np
import pytest

from test_support_gpu import gpu_support
from test_wfilt_gpu import RAD, Scene, sphere_set
import support_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene_args(pkg):
    return pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=RAD)[:4]


@pytest.fixture(scope="module")
def subject(pkg, scene_args):
    s = Scene(pkg, *scene_args)
    yield s
    s.ctx.close()


def same(got, want, label):
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (label, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (label, k)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (label, k)


def test_back_to_back_families(pkg, scene_args, subject):
    s = subject

    def fresh(call):
        """call on a context of its own."""
        with pkg.MvsContext(*scene_args, device=0) as ctx:
            return call(ctx)

    _, c, nrm, ref, mask = sphere_set(s, 257, 41)
    rng = np.random.default_rng(42)
    avg = rng.uniform(0.5, 1.0, 257)
    nci, ncj = s.ctx.cell_grid(2)
    # inputs that are outputs of other calls come from contexts of their own
    ncc = fresh(lambda x: x.score_warped(c, nrm, ref, want_ncc=True))[4]
    views5, dstep5 = fresh(lambda x: x.refine_lists(ncc[:5], c[:5], ref[:5]))
    front = fresh(lambda x: x.wfilt_front(c, ref, mask, 2))[0]
    front3 = fresh(lambda x: x.wfilt_front(c[:3], ref[:3], mask[:3], 2))[0]
    xy4, mask4 = fresh(lambda x: x.score(c[:4], ref[:4], 0.7, 5))[:2]
    jobs = np.stack([np.arange(257), rng.integers(0, s.V, 257), rng.integers(0, 8, 257), rng.integers(0, 8, 257)],
                    axis=1).astype(np.int32)                      # 64 cells per view: contested claims
    accept = (rng.random(257) < 0.8).astype(np.uint8)
    score = rng.uniform(0.0, 1.0, 257)
    sel = rng.integers(0, 257, 57)
    _, cL, nrmL, refL, _ = sphere_set(s, 4099, 43)

    calls = [
        ("score_warped 257", lambda x: x.score_warped(c, nrm, ref, want_ncc=True)),
        ("refine_warped_level 5", lambda x: x.refine_warped_level(c[:5], nrm[:5], ref[:5], views5, dstep5,
                                                                  want_scores=True)),
        ("wfilt_front 257", lambda x: x.wfilt_front(c, ref, mask, 2)),
        ("wfilt_test 257", lambda x: x.wfilt_test(c, nrm, ref, mask, avg, 2, 2.0, 1, front)),
        ("wfilt_support 3", lambda x: x.wfilt_support(c[:3], nrm[:3], ref[:3], mask[:3], 2, 2.0, 0.25, 1, front3)),
        ("wexp_claim 1", lambda x: (x.wexp_claim_checked(jobs[:1], accept[:1], score[:1], nci, ncj),)),
        ("wexp_claim 257", lambda x: (x.wexp_claim_checked(jobs, accept, score, nci, ncj),)),
        ("refine_lists sel dstep", lambda x: x.refine_lists(ncc, c, ref, sel)),
        ("refine_lists plain", lambda x: x.refine_lists(ncc)),
        ("score 4", lambda x: x.score(c[:4], ref[:4], 0.7, 5)),
        ("exact_avg 4", lambda x: (x.exact_avg(ref[:4], xy4, mask4, 5),)),
        ("score_warped 1", lambda x: x.score_warped(c[:1], nrm[:1], ref[:1], want_ncc=True)),
        ("score_warped 4099", lambda x: x.score_warped(cL, nrmL, refL, want_ncc=True)),
    ]
    got = [(label, call(s.ctx)) for label, call in calls]      # back to back on the one context
    for (label, g), (_, call) in zip(got, calls):
        same(g, fresh(call), label)
    # the calls did something: claims were contested, views passed, patches were kept
    by = dict(got)
    assert 0 < by["wexp_claim 257"][0].sum() < accept.sum()
    assert by["score_warped 4099"][2].max() > 0 and by["wfilt_test 257"][2].any()
    assert (by["refine_lists sel dstep"][0] >= 0).any() and by["refine_lists plain"][1] is None


def test_side_stream_beside_the_arena(subject):
    """score_warped through the arena, the support test on device pointers and
    a side stream, score_warped again: the scores agree and the support result
    is the restatement's."""
    import torch
    s = subject
    _, c, nrm, ref, mask = sphere_set(s, 257, 44)
    front = s.ctx.wfilt_front(c, ref, mask, 2)[0]
    want = sr.support(*s.cam(), c, nrm, ref, mask, 2, 2.0, 0.25, 1, front)
    side = torch.cuda.Stream(torch.device("cuda:0"))
    first = s.ctx.score_warped(c, nrm, ref, want_ncc=True)
    got = gpu_support(s, c, nrm, ref, mask, 2, 2.0, 0.25, 1, front, stream=side)
    again = s.ctx.score_warped(c, nrm, ref, want_ncc=True)
    same(again, first, "score_warped around the side stream")
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
