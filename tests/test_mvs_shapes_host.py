"""Coverage of the odd-image-size scoring cases (shapes_scene.py), from the
oracle alone: the GPU tests of test_mvs_shapes_gpu.py only mean something if
passing candidates really lie in the partial edge tiles, the counts vary, and
non-passing and invalid candidates are there too.  The floors are asserted
at the highest threshold the GPU tests use, 0.7, and every window size.  The
uniform part of the candidates alone (n = 6000, wid 5) gives 294 / 56 / 19
passing candidates in the last tile column / row / corner tile at 23 x 29 x
16 and 198 / 40 / 3 at 55 x 77 x 130; the aimed candidates lift every scene
over the floors, and where the default inputs do not (16 x 16, 41 x 2061) the
inputs change (shapes_scene.SCENE_INPUTS), not the floor.  Run with -s for
the table (profiles/r13/host_coverage.txt)."""
import pytest

import shapes_scene as ss

FLOOR_COL, FLOOR_ROW, FLOOR_CORNER = 100, 50, 10
FLOOR_COUNTS, FLOOR_ZERO, FLOOR_INVALID = 8, 50, 50


@pytest.mark.parametrize("H,W,V", ss.SCENES)
def test_edge_tiles_are_reached(orc, H, W, V):
    (rgb, K, R, t), (c, ref) = ss.scene_and_candidates(H, W, V)
    assert len(ref) >= 6000 + 768
    scene = orc.Scene(rgb, K, R, t)
    for wid in ss.WIDS:
        xy, _, count, _ = scene.score_batch(c, ref, 0.7, wid, nthreads=16)
        cv = ss.coverage(xy, count, H, W, wid)
        print(f"{H}x{W}x{V} wid {wid}: " + " ".join(f"{k}={v}" for k, v in cv.items()))
        if cv["col_has_centre"]:
            assert cv["col"] >= FLOOR_COL, (wid, cv)
        if cv["row_has_centre"]:
            assert cv["row"] >= FLOOR_ROW, (wid, cv)
        if cv["col_has_centre"] and cv["row_has_centre"]:
            assert cv["corner"] >= FLOOR_CORNER, (wid, cv)
        if V >= 16:
            assert cv["counts"] >= FLOOR_COUNTS, (wid, cv)
        assert cv["zero_inside"] >= FLOOR_ZERO, (wid, cv)
        assert cv["invalid"] >= FLOOR_INVALID, (wid, cv)


def test_shapes_reach_the_partial_blocks():
    """The image sizes themselves: a partial 16 x 8 tile column and row, a
    partial 32 x 16 moments block each way, widths that are no multiple of 4
    or 16 (k_build_scene's byte branch and partial quads), view counts that
    leave a partial block of 16, and the minimum size."""
    sizes = [(H, W) for H, W, _ in ss.SCENES if (H, W) != (16, 16)]
    assert all(W % 16 and H % 8 and W % 4 and W % 32 and H % 16 for H, W in sizes)
    assert (16, 16) in [(H, W) for H, W, _ in ss.SCENES]
    assert any(W > 2048 for _, W in sizes)
    # a partial quad of the last column alone, and one with a column that windows use
    assert any(W % 4 == 1 for _, W in sizes) and any(W % 4 == 3 for _, W in sizes)
    assert any(H % 8 == 1 for H, _ in sizes) and any(H % 8 == 7 for H, _ in sizes)
    views = [V for _, _, V in ss.SCENES]
    assert any(V % 16 == 1 for V in views) and any(64 < V <= 128 for V in views) and any(V > 128 for V in views)
