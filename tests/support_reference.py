"""Float64 restatement of the neighbour-support test (mvs_wfilt_support_device,
include/mvs_amd.h) and of MvsContext.filter_warped with min_support, built on
filter_reference (placements, the front grid, adjacency and the visibility
chain), which stays as it is.  N and A are Python integers and the decision is
one binary64 product, so every output can be compared exactly.  A plain module
(the tests import it); the definition in the header is the specification.
"""
import math

import numpy as np

import filter_reference as fr

NEIGHBOURS = tuple((di, dj) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (di, dj) != (0, 0))


def check_scalars(min_support, min_neigh):
    if not (math.isfinite(min_support) and 0.0 <= min_support <= 1.0) or min_neigh < 0:
        raise ValueError("min_support must be finite and in [0, 1], min_neigh >= 0")


def decide(N, A, min_support, min_neigh):
    """keep of a live row: N >= min_neigh and (double)A >= min_support * (double)N."""
    return int(N) >= min_neigh and float(int(A)) >= float(min_support) * float(int(N))


def support(K, Rp, t, W, H, c, nrm, ref, mask, cell, adj_px, min_support, min_neigh, front):
    """mvs_wfilt_support_device on a front grid as given (an entry outside
    -1..n-1 reads as -1) -> nb (n,) int32, adj (n,) int32, keep (n,) uint8."""
    check_scalars(min_support, min_neigh)
    n = len(ref)
    _, ncj, nci = front.shape
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    cl = [[float(x) for x in row] for row in c]
    nl = [[float(x) for x in row] for row in nrm]
    nb, adj, keep = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for p, row in enumerate(fr.placements(K, Rp, t, W, H, c, ref, mask, cell)):
        if row is None:
            continue
        N = A = 0
        for v, (i, j), z in row:
            for di, dj in NEIGHBOURS:
                a, b = i + di, j + dj
                if not (0 <= a < nci and 0 <= b < ncj):
                    continue
                q = int(front[v, b, a])
                if q < 0 or q >= n or q == p:
                    continue
                N += 1
                A += bool(fr.adjacent(cl[p], nl[p], cl[q], nl[q], float(adj_px), z, float(K[v][0, 0]),
                                      float(K[v][1, 1])))
        nb[p], adj[p] = N, A
        keep[p] = decide(N, A, min_support, min_neigh)
    return nb, adj, keep


def filter_chain(K, Rp, t, W, H, c, nrm, ref, mask, avg, cell=2, adj_px=2.0, min_views=3, passes=2,
                 min_support=None, min_neigh=1, support_passes=1):
    """MvsContext.filter_warped on the CPU: filter_reference.filter_chain, then
    with min_support up to support_passes passes of front grid, support test and
    ref = -1 for the removed rows, stopping when a pass removes nothing; the
    grids are rebuilt from the survivors.  -> filter_reference's dict, with
    min_support also nb, adj (the last support pass) and removed_support."""
    V = len(K)
    ref = np.array(ref, np.int32).reshape(-1)
    out = fr.filter_chain(K, Rp, t, W, H, c, nrm, ref, mask, avg, cell, adj_px, min_views, passes)
    if min_support is None:
        return out
    check_scalars(min_support, min_neigh)
    n = len(ref)
    ref[out["keep"] == 0] = -1
    nb, adj, removed = np.zeros(n, np.int32), np.zeros(n, np.int32), []
    for _ in range(support_passes):
        alive = int(((ref >= 0) & (ref < V)).sum())
        front, _ = fr.front_grid(K, Rp, t, W, H, c, ref, mask, cell)
        nb, adj, keep = support(K, Rp, t, W, H, c, nrm, ref, mask, cell, adj_px, min_support, min_neigh, front)
        ref[keep == 0] = -1
        removed.append(alive - int(keep.sum()))
        if removed[-1] == 0:
            break
    out["keep"] = ((ref >= 0) & (ref < V)).astype(np.uint8)
    out["front"], out["zfront"] = fr.front_grid(K, Rp, t, W, H, c, ref, mask, cell)
    out.update(nb=nb, adj=adj, removed_support=removed)
    return out


_MIXED = {}


def sphere_mixed(pkg, rad=0.02):
    """The sphere scene (V 24, 96 x 128) with true rodrigues_roundtrip rotations
    and filter_reference.mixed_set on it, computed once per process and shared
    by the test modules; nothing of it is to be modified.
    -> dict rgb, K, R, t_raw, t, Rp, W, H and set (mixed_set's dict)."""
    if rad not in _MIXED:
        import warped_reference as wr
        rgb, K, R, t_raw = pkg.synthetic.sphere_scene(V=24, H=96, W=128, rad=rad)[:4]
        Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
        t = np.asarray(t_raw, np.float64).reshape(-1, 3)
        gray = wr.gray_stack(rgb)
        _MIXED[rad] = {"rgb": rgb, "gray": gray, "K": K, "R": R, "t_raw": t_raw, "t": t, "Rp": Rp, "W": 128, "H": 96,
                       "set": fr.mixed_set(gray, K, R, t, Rp, rad)}
    return _MIXED[rad]
