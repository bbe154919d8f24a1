"""Batches that force k_score_tab's units into every K-span class
(test_kspan_host.py, test_kspan_gpu.py).  No GPU.

A unit's span is WID + 1 + the distance in row pairs ((y mod 8) >> 1) between
its first and last candidate.  Here the candidates' pixel rows are restricted
to two row pairs p0 <= p1 of the 8-row tiles, so a wave's sorted list holds
those two pairs alone and its units span WID + 1 (one pair) or
WID + 1 + p1 - p0 K-steps -- every class from one pair to all four, also in
the clamped first and last tile rows.  The scenes are shapes_scene's noisy
copies of one image (candidates pass anywhere), 3 x 5 and 3 x 6 tiles."""
import numpy as np

import shapes_scene as ss

SCENES = [(40, 45), (43, 45)]   # (H, W): H a multiple of the tile's 8 rows, and not
VIEWS = (5, 48)                 # one view block, three
PAIRS = [(p0, p1) for p0 in range(4) for p1 in range(p0, 4)]
WIDS = (1, 2, 3, 4, 5)
N = 4096                        # above the direct path's cutoff; 64 per tile and more: binned into runs
THR = 0.7
# the FAST = false instantiation (thr 0): one pair per window size, spans WID + 1 .. WID + 4
THR0_PAIR = {1: (0, 0), 2: (0, 1), 3: (1, 3), 4: (0, 3), 5: (2, 3)}
MIN_PASSING = 100               # candidates with |V| >= 1 in every case (test_kspan_host.py)


def span_class(pair, wid):
    return wid + 1 + pair[1] - pair[0]


def runs(wid):
    """(pair, thr) of every scoring call at one window size."""
    return [(p, THR) for p in PAIRS] + [(THR0_PAIR[wid], 0.0)]


class Case:
    """A scene, its ten batches and the oracle's answers, computed once."""

    def __init__(self, orc, H, W, V):
        self.H, self.W, self.V = H, W, V
        self.scene = ss.copies_scene(V, H, W, seed=1, amp_shift=5 if V == 5 else 0)
        self.gray = orc.gray_from_rgb(self.scene[0])
        self.oracle = orc.Scene(*self.scene)
        self.batch = {p: self._candidates(p) for p in PAIRS}
        self._want = {}

    def _candidates(self, pair):
        rng = np.random.default_rng([7, self.H, self.V, *pair])
        rows = np.array([y for y in range(self.H) if ((y % ss.TILE_H) >> 1) in pair])
        y = rng.choice(rows, N) + rng.uniform(0.1, 0.9, N)
        x = rng.integers(0, self.W, N) + rng.uniform(0.1, 0.9, N)
        ref = rng.integers(0, self.V, N).astype(np.int32)
        _, K, R, t = self.scene
        V = self.V
        return ss.at_pixels(x, y, ref, np.asarray(K, np.float64).reshape(V, 3, 3),
                            np.asarray(R, np.float64).reshape(V, 3, 3), np.asarray(t, np.float64).reshape(V, 3))

    def want(self, pair, wid, thr):
        if (pair, wid, thr) not in self._want:
            self._want[pair, wid, thr] = self.oracle.score_batch(*self.batch[pair], thr, wid, nthreads=16)
        return self._want[pair, wid, thr]


_cases = {}


def case(orc, H, W, V):
    if (H, W, V) not in _cases:
        _cases[H, W, V] = Case(orc, H, W, V)
    return _cases[H, W, V]
