"""Float64 restatement of the visibility-consistency filter (mvs_wfilt_front_device,
mvs_wfilt_test_device, include/mvs_amd.h) and of the chain around them
(MvsContext.filter_warped), built on expand_reference.cell_of / mask_views,
which stay as they are.  The geometry is written in Python floats, product by
product and sum by sum in the header's order (left to right, unfused), and the
weights are Python integers, so every output can be compared exactly.  A plain
module (the tests import it); the definition in the header is the specification.
"""
import math

import numpy as np

import expand_reference as er


def weight(avg):
    """w = floor(clamp(avg, 0, 2) 2^32 + 0.5), 0 when avg is not finite."""
    a = float(avg)
    if not math.isfinite(a):
        return 0
    a = 0.0 if a < 0.0 else 2.0 if a > 2.0 else a
    return int(math.floor(a * 4294967296.0 + 0.5))


def views_of(ref, mask_row, V):
    """T(p): {ref} + the mask's views, those in 0..V-1, ascending; None for a dead row."""
    r = int(ref)
    if not 0 <= r < V:
        return None
    return sorted(set(er.mask_views(mask_row, V)) | {r})


def depth_in(Rp, t, v, c):
    """z_p(v), left to right."""
    R9 = [float(x) for x in np.asarray(Rp[v]).reshape(9)]
    X, Y, Z = (float(x) for x in c)
    return R9[6] * X + R9[7] * Y + R9[8] * Z + float(np.asarray(t[v]).reshape(3)[2])


def placements(K, Rp, t, W, H, c, ref, mask, cell):
    """Per patch the list of (view, (i, j), z) of its placed views; None for a dead row."""
    V = len(K)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    mask = np.asarray(mask).reshape(len(c), (V + 63) // 64)
    out = []
    for p in range(len(c)):
        views = views_of(ref[p], mask[p], V)
        if views is None:
            out.append(None)
            continue
        row = []
        for v in views:
            ij = er.cell_of(K, Rp, t, v, c[p], W, H, cell)
            if ij is not None:
                row.append((v, ij, depth_in(Rp, t, v, c[p])))
        out.append(row)
    return out


def front_grid(K, Rp, t, W, H, c, ref, mask, cell):
    """front (V, ncj, nci) int32 and zfront float64: the placed patch of least z
    per (view, cell), ties to the lowest index; -1 and +inf in an empty cell."""
    V = len(K)
    nci, ncj = er.grid_shape(W, H, cell)
    front = np.full((V, ncj, nci), -1, np.int32)
    zfront = np.full((V, ncj, nci), np.inf)
    for p, row in enumerate(placements(K, Rp, t, W, H, c, ref, mask, cell)):
        for v, (i, j), z in row or ():
            if front[v, j, i] < 0 or z < zfront[v, j, i]:       # ascending p: a tie keeps the lower index
                front[v, j, i], zfront[v, j, i] = p, z
    return front, zfront


def adjacent(cp, np_, cf, nf, adj_px, z, fx, fy):
    d = [cp[k] - cf[k] for k in range(3)]
    a = abs(d[0] * np_[0] + d[1] * np_[1] + d[2] * np_[2]) + abs(d[0] * nf[0] + d[1] * nf[1] + d[2] * nf[2])
    rho = (adj_px * z) / ((fx + fy) / 2)
    return a < 2.0 * rho                                          # False with a nan anywhere


def vistest(K, Rp, t, W, H, c, nrm, ref, mask, avg, cell, adj_px, min_views, front):
    """mvs_wfilt_test_device on a front grid as given (an entry outside -1..n-1
    reads as -1) -> vis (n, words) uint64, conf (n,) int64, keep (n,) uint8 and
    F, the list of conflict sets."""
    V = len(K)
    n = len(ref)
    words = (V + 63) // 64
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    mask = np.asarray(mask).reshape(n, words)
    cl = [[float(x) for x in row] for row in c]
    nl = [[float(x) for x in row] for row in nrm]
    adj_px = float(adj_px)
    vis = np.zeros((n, words), np.uint64)
    F = [set() for _ in range(n)]
    for p, row in enumerate(placements(K, Rp, t, W, H, c, ref, mask, cell)):
        for v, (i, j), z in row or ():
            f = int(front[v, j, i])
            if f < 0 or f >= n:
                continue
            if f == p or adjacent(cl[p], nl[p], cl[f], nl[f], adj_px, z, float(K[v][0, 0]), float(K[v][1, 1])):
                vis[p, v >> 6] |= np.uint64(1) << np.uint64(v & 63)
            else:
                F[p].add(f)
    w = [weight(a) for a in avg]
    conf = [0] * n
    for p in range(n):
        for f in F[p]:
            conf[p] += w[f]
            conf[f] += w[p]
    keep = np.zeros(n, np.uint8)
    for p in range(n):
        views = views_of(ref[p], mask[p], V)
        if views is None:
            conf[p] = 0
            continue
        seen = sum(bin(int(x)).count("1") for x in vis[p])
        keep[p] = seen >= min_views and len(views) * w[p] >= conf[p]
    return vis, np.array(conf, np.int64).reshape(n), keep, F


def filter_chain(K, Rp, t, W, H, c, nrm, ref, mask, avg, cell=2, adj_px=2.0, min_views=3, passes=2):
    """MvsContext.filter_warped on the CPU: per pass the front grid of the rows
    still alive, the test, and ref = -1 for the removed rows; it stops early when
    a pass removes nothing.  -> dict keep (over the input), removed (per pass),
    vis, conf (last pass), front, zfront (rebuilt from the survivors)."""
    ref = np.array(ref, np.int32).reshape(-1)
    n = len(ref)
    V = len(K)
    vis, conf = np.zeros((n, (V + 63) // 64), np.uint64), np.zeros(n, np.int64)
    removed = []
    for _ in range(passes):
        alive = int(((ref >= 0) & (ref < V)).sum())
        front, _ = front_grid(K, Rp, t, W, H, c, ref, mask, cell)
        vis, conf, keep, _ = vistest(K, Rp, t, W, H, c, nrm, ref, mask, avg, cell, adj_px, min_views, front)
        ref[keep == 0] = -1
        removed.append(alive - int(keep.sum()))
        if removed[-1] == 0:
            break
    keep = ((ref >= 0) & (ref < V)).astype(np.uint8)
    front, zfront = front_grid(K, Rp, t, W, H, c, ref, mask, cell)
    return {"keep": keep, "removed": removed, "vis": vis, "conf": conf, "front": front, "zfront": zfront}


def mixed_set(gray, K, R, t, Rp, rad, n_out=300, shift=0.002):
    """The quality experiment's input on the sphere scene: the restatement's
    chain (4 seeds of sphere_patches(default_rng(1)), 3 rounds, wid 3, cell 2,
    min_ncc 0.7, min_cos 0.3, vlb 2, score_batch_fast) followed by the outliers:
    n_out chain patches chosen by default_rng(7).permutation, moved alternately
    +shift and -shift along the radius and re-scored; those with count >= 2.
    -> dict c, nrm, ref, mask, avg, cell (the outliers' cell is (-1, -1)) and
    kind: 0 = chain, 1 = outlier outside the surface, 2 = inside."""
    import warped_reference as wr
    c0, n0, r0, _ = wr.sphere_patches(K, R, t, 4, rad, np.random.default_rng(1))
    kw = dict(cell=2, wid=3, min_ncc=0.7, min_cos=0.3, vlb=2, scorer=er.score_batch_fast)
    ch = er.expand_chain(gray, K, Rp, t, c0, n0, r0, 3, **kw)
    P = len(ch["ref"])
    pick = np.random.default_rng(7).permutation(P)[:n_out]
    sign = np.where(np.arange(len(pick)) % 2 == 0, 1.0, -1.0)
    radial = ch["c"][pick] / np.linalg.norm(ch["c"][pick], axis=1, keepdims=True)
    oc = ch["c"][pick] + (sign * shift)[:, None] * radial
    on, orf = ch["nrm"][pick], ch["ref"][pick]
    m, k, a, _ = er.score_batch_fast(gray, K, Rp, t, oc, on, orf, 3, 0.7, 0.3)
    ok = k >= 2
    return {"c": np.concatenate([ch["c"], oc[ok]]), "nrm": np.concatenate([ch["nrm"], on[ok]]),
            "ref": np.concatenate([ch["ref"], orf[ok]]).astype(np.int32),
            "mask": np.concatenate([ch["mask"], m[ok]]).astype(np.uint64),
            "avg": np.concatenate([ch["avg"], a[ok]]),
            "cell": np.concatenate([ch["cell"], np.full((int(ok.sum()), 2), -1)]).astype(np.int32),
            "kind": np.concatenate([np.zeros(P, np.int32), np.where(sign[ok] > 0, 1, 2).astype(np.int32)])}
