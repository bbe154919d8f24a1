"""What the K-span batches (kspan_cases.py) reach, from the oracle and the
CPU recount (tools/kstep_count.py) alone: passing candidates in every case,
the rows they were aimed at, and units of the intended span class."""
import importlib.util
import os

import numpy as np
import pytest

import kspan_cases as kc
import shapes_scene as ss
from conftest import REPO


def _tool():
    spec = importlib.util.spec_from_file_location("kstep_count", os.path.join(REPO, "tools", "kstep_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("V", kc.VIEWS)
@pytest.mark.parametrize("H,W", kc.SCENES)
def test_batches_pass_and_span(orc, H, W, V):
    ks = _tool()
    case = kc.case(orc, H, W, V)
    for wid in kc.WIDS:
        for pair, thr in kc.runs(wid):
            xy, _, count, _ = case.want(pair, wid, thr)
            tag = (pair, wid, thr)
            assert (count >= 1).sum() >= kc.MIN_PASSING, (tag, int((count >= 1).sum()))
            rp = (np.floor(xy[:, 1]).astype(int) % ss.TILE_H) >> 1
            assert set(np.unique(rp)) == set(pair), tag
            hist = ks.span_histogram(xy, case.batch[pair][1], case.gray, wid)
            assert hist[kc.span_class(pair, wid)] > 0, (tag, hist)
            assert sum(n for s, n in hist.items() if s > kc.span_class(pair, wid)) == 0, (tag, hist)


def test_split_and_rules():
    """The tool's block split covers every block once, at most 8 per wave;
    the pass rules' step counts."""
    ks = _tool()
    for nblk in range(65):
        size = np.diff(ks.wave_bounds(nblk))
        assert size.sum() == nblk and size.min() >= nblk // 8 and size.max() <= -(-nblk // 8)
    assert ks.wave_bounds(21) == [0, 2, 5, 7, 10, 13, 15, 18, 21]
    for wid in kc.WIDS:
        span = np.arange(wid + 1, wid + 5)
        assert list(ks.steps_of(span, wid, "exact")) == list(span)
        assert list(ks.steps_of(span, wid, "parent")) == [wid + 1, wid + 2, 2 * wid + 2, 2 * wid + 2]
        assert list(ks.steps_of(span, wid, "one")) == [wid + 1, wid + 2, wid + 4, wid + 4]
