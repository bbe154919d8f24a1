"""k_score_tab's exact-length K passes: batches whose
units fall into every span class, WID + 1 to WID + 4 K-steps (kspan_cases.py;
what they reach is asserted by test_kspan_host.py), at every window size, one
and three view blocks, the fast and the binary64 decision, through the runs
and through the atomic tile buckets.  Every case against the oracle: xy, masks
and counts bit-exact, avg within AVG_TOL; records pre-filled with -1."""
import os

import numpy as np
import pytest

import kspan_cases as kc

pytestmark = pytest.mark.gpu

AVG_TOL = 1e-12


def _context(pkg, scene, binning):
    """A fresh context created under MVS_BIN = binning (None: unset) and no
    MVS_SCORE_KERNEL, the environment as it was afterwards."""
    env = {"MVS_SCORE_KERNEL": None, "MVS_BIN": binning}
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return pkg.MvsContext(*scene, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _score_rec(cx, c, ref, thr, wid):
    """score_device_rec into xy and records pre-filled with -1: a record or a
    projection left unwritten shows."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ref)
    tc, tr = torch.from_numpy(c).to(dev), torch.from_numpy(ref).to(dev)
    xy = torch.full((n, 2), -1.0, dtype=torch.float64, device=dev)
    rec = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cx.score_device_rec(tc, tr, xy, rec, thr, wid)
    torch.cuda.synchronize()
    return xy.cpu().numpy(), rec.cpu().numpy()


def _check_rec(got, want, tag):
    xy, rec = got
    mask = rec[:, 0].view(np.uint64)
    got4 = (xy, mask.reshape(-1, 1), np.bitwise_count(mask).astype(np.int32), rec[:, 1].view(np.float64))
    for name, g, e in zip(("xy", "mask", "count"), got4[:3], want[:3]):
        assert np.array_equal(g, e), (tag, name, np.nonzero(np.asarray(g != e).reshape(len(e), -1).any(1))[0][:8])
    assert np.allclose(got4[3], want[3], rtol=0, atol=AVG_TOL), tag


@pytest.mark.parametrize("binning", [None, "atomic"], ids=["runs", "atomic"])
@pytest.mark.parametrize("V", kc.VIEWS)
@pytest.mark.parametrize("H,W", kc.SCENES)
def test_every_span_class(pkg, orc, H, W, V, binning):
    case = kc.case(orc, H, W, V)
    ntiles = -(-W // 16) * -(-H // 8)
    assert kc.N >= 2048 and kc.N >= 64 * ntiles   # tiled, and dense enough for the runs
    cx = _context(pkg, case.scene, binning)
    try:
        cx.kernel_timing(True)
        for wid in kc.WIDS:
            for pair, thr in kc.runs(wid):
                want = case.want(pair, wid, thr)
                before = cx.bin_runs_batches()
                got = _score_rec(cx, *case.batch[pair], thr, wid)
                assert cx.timed_kernel() == "k_score_tab", (pair, wid, thr)
                assert cx.bin_runs_batches() - before == int(binning is None), (pair, wid, thr)
                _check_rec(got, want, (pair, wid, thr))
    finally:
        cx.close()
