"""Float64 restatement of the warped expansion's three primitives
(mvs_wexp_children_device, mvs_wexp_claim_device, mvs_wexp_mark_device,
include/mvs_amd.h) and of the chain around them (MvsContext.expand_warped),
built on warped_reference and refine_reference, which stay as they are.  The
geometry is written in Python floats, product by product and sum by sum in the
header's order (left to right, unfused), so the integer decisions derived from
it can be compared exactly.  A plain module (the tests import it); the
definition in the header is the specification.
"""
import math

import numpy as np

import refine_reference as rr
import warped_reference as wr

NEIGHBOURS = ((1, 0), (-1, 0), (0, 1), (0, -1))


def grid_shape(W, H, cell):
    """(nci, ncj): whole cells only."""
    return W // cell, H // cell


def _cam(K, Rp, t, v):
    return ([float(x) for x in np.asarray(Rp[v]).reshape(9)], [float(x) for x in np.asarray(t[v]).reshape(3)],
            float(K[v][0, 0]), float(K[v][1, 1]), float(K[v][0, 2]), float(K[v][1, 2]))


def centre_of(Rp9, t3):
    """O = -Rp^T t, each component a left-to-right sum of three products."""
    return [-(Rp9[k] * t3[0] + Rp9[3 + k] * t3[1] + Rp9[6 + k] * t3[2]) for k in range(3)]


def cell_of(K, Rp, t, v, c, W, H, cell):
    """The cell (i, j) of the projection of c into view v, or None when the
    depth is not positive, the position is outside [0, W) x [0, H) or the cell
    lies outside the grid."""
    x, y, depth = wr.project_ref(K[v], Rp[v], t[v], c)
    if not (depth > 0 and 0 <= x < W and 0 <= y < H):
        return None
    nci, ncj = grid_shape(W, H, cell)
    i, j = int(x) // cell, int(y) // cell
    if i >= nci or j >= ncj:
        return None
    return i, j


def mask_views(mask_row, V):
    """Views 0..V-1 whose bit is set in the uint64 words of one mask row."""
    words = [int(w) for w in np.asarray(mask_row).reshape(-1).view(np.uint64)]
    return [v for v in range(V) if words[v >> 6] >> (v & 63) & 1]


def children(K, Rp, t, W, H, c, nrm, ref, mask, cell, occ, max_dist):
    """Primitive 1 over n frontier patches -> jobs (m, 4) int32, cc (m, 3), cn
    (m, 3), cref (m,) int32 in the sequential order (patch, view, neighbour)."""
    V = len(K)
    nci, ncj = grid_shape(W, H, cell)
    half = (cell - 1) / 2.0
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    mask = np.asarray(mask).reshape(len(c), -1)
    jobs, cc, cn, cref = [], [], [], []
    for p in range(len(c)):
        cp = [float(x) for x in c[p]]
        n = [float(x) for x in nrm[p]]
        views = set(mask_views(mask[p], V))
        if 0 <= int(ref[p]) < V:
            views.add(int(ref[p]))
        for v in sorted(views):
            ij = cell_of(K, Rp, t, v, cp, W, H, cell)
            if ij is None:
                continue
            R9, t3, fx, fy, cx, cy = _cam(K, Rp, t, v)
            O = centre_of(R9, t3)
            e = [cp[k] - O[k] for k in range(3)]
            h = n[0] * e[0] + n[1] * e[1] + n[2] * e[2]
            for di, dj in NEIGHBOURS:
                a, b = ij[0] + di, ij[1] + dj
                if not (0 <= a < nci and 0 <= b < ncj) or occ[v, b, a]:
                    continue
                u = ((a * cell + half) - cx) / fx
                w = ((b * cell + half) - cy) / fy
                d = [R9[k] * u + R9[3 + k] * w + R9[6 + k] for k in range(3)]
                den = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
                if den == 0.0:
                    continue
                s = h / den
                if not (s > 0 and math.isfinite(s)):
                    continue
                X = [O[k] + d[k] * s for k in range(3)]
                q = [X[k] - cp[k] for k in range(3)]
                if not math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) <= max_dist:
                    continue
                jobs.append((p, v, a, b))
                cc.append(X)
                cn.append(nrm[p])
                cref.append(v)
    return (np.array(jobs, np.int32).reshape(-1, 4), np.array(cc, np.float64).reshape(-1, 3),
            np.array(cn, np.float64).reshape(-1, 3), np.array(cref, np.int32))


def claim(jobs, accept, score, V, nci, ncj):
    """Primitive 2: among the contenders (accept != 0, finite score) of one
    (view, cell) inside the grid the highest score wins, ties to the lowest job
    index -> win (m,) uint8."""
    best = {}
    for k in range(len(jobs)):
        _, v, i, j = (int(x) for x in jobs[k])
        s = float(score[k])
        if not accept[k] or not math.isfinite(s):
            continue
        if not (0 <= v < V and 0 <= i < nci and 0 <= j < ncj):
            continue
        if (v, i, j) not in best or s > best[(v, i, j)][0]:    # -0.0 > 0.0 is False: numeric
            best[(v, i, j)] = (s, k)
    win = np.zeros(len(jobs), np.uint8)
    for _, k in best.values():
        win[k] = 1
    return win


def mark(K, Rp, t, W, H, jobs, win, cc, cref, mask, cell, occ):
    """Primitive 3, in place on occ (V, ncj, nci) uint8."""
    V = len(K)
    nci, ncj = grid_shape(W, H, cell)
    mask = np.asarray(mask).reshape(len(jobs), -1)
    for k in np.flatnonzero(np.asarray(win)):
        _, _, i, j = (int(x) for x in jobs[k])
        r = int(cref[k])
        if 0 <= r < V and 0 <= i < nci and 0 <= j < ncj and not occ[r, j, i]:
            occ[r, j, i] = 1
        for v in mask_views(mask[k], V):
            ij = cell_of(K, Rp, t, v, cc[k], W, H, cell)
            if ij is not None and not occ[v, ij[1], ij[0]]:     # a nonzero byte stays as it is
                occ[v, ij[1], ij[0]] = 1
    return occ


def score_batch(gray, K, Rp, t, c, nrm, ref, wid, min_ncc, min_cos):
    """warped_reference over a batch -> mask (n, words) uint64, count, avg, ncc (n, V)."""
    V = len(K)
    words = (V + 63) // 64
    n = len(ref)
    mask = np.zeros((n, words), np.uint64)
    count = np.zeros(n, np.int32)
    avg = np.zeros(n)
    ncc = np.full((n, V), np.nan)
    for i in range(n):
        o = wr.warped_reference(gray, K, Rp, t, c[i], nrm[i], ref[i], wid, min_cos)
        ncc[i] = o["ncc"]
        with np.errstate(invalid="ignore"):
            ps = np.flatnonzero(o["ncc"] > min_ncc)
        for v in ps:
            mask[i, v >> 6] |= np.uint64(1) << np.uint64(v & 63)
        count[i] = len(ps)
        avg[i] = float(o["ncc"][ps].sum() / len(ps)) if len(ps) else 0.0
    return mask, count, avg, ncc


def score_batch_fast(gray, K, Rp, t, c, nrm, ref, wid, min_ncc, min_cos):
    """score_batch with the candidates of a batch taken together, view by view:
    the same definition and the same pieces (ray-plane points, difference-form
    bilinear samples, the sums on g - 128), but sums and products run through
    numpy over the whole batch, so an ncc may differ from warped_reference's in
    its last bits.  For the long chains; test_expand_host.py holds it against
    score_batch."""
    gray = np.asarray(gray)
    V, H, W = gray.shape
    K = np.asarray(K, np.float64).reshape(V, 3, 3)
    Rp = np.asarray(Rp, np.float64).reshape(V, 3, 3)
    t = np.asarray(t, np.float64).reshape(V, 3)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    r = np.asarray(ref, np.int64).reshape(-1)
    n = len(r)
    S = 2 * wid + 1
    N = S * S
    words = (V + 63) // 64
    ncc = np.full((n, V), np.nan)
    if n == 0:
        return np.zeros((0, words), np.uint64), np.zeros(0, np.int32), np.zeros(0), ncc
    g = gray.astype(np.float64) - 128.0
    O = wr.centres(Rp, t)
    Rr, tr = Rp[r], t[r]
    with np.errstate(all="ignore"):
        # the projection into the reference view, in project_ref's order
        x = Rr[:, 0, 0] * c[:, 0] + Rr[:, 0, 1] * c[:, 1] + Rr[:, 0, 2] * c[:, 2] + tr[:, 0]
        y = Rr[:, 1, 0] * c[:, 0] + Rr[:, 1, 1] * c[:, 1] + Rr[:, 1, 2] * c[:, 2] + tr[:, 1]
        z = Rr[:, 2, 0] * c[:, 0] + Rr[:, 2, 1] * c[:, 1] + Rr[:, 2, 2] * c[:, 2] + tr[:, 2]
        w = np.where(z != 0.0, 1.0 / z, 1.0)
        x = x * w * K[r, 0, 0] + K[r, 0, 2]
        y = y * w * K[r, 1, 1] + K[r, 1, 2]
        valid = (z > 0) & (x >= 0) & (y >= 0) & (np.abs(x) < 1e9) & (np.abs(y) < 1e9)
        x0 = np.where(valid, x, 0.0).astype(np.int64)
        y0 = np.where(valid, y, 0.0).astype(np.int64)
        valid &= (x0 - wid >= 0) & (x0 + wid <= W - 1) & (y0 - wid >= 0) & (y0 + wid <= H - 1)
        e = O[None, :, :] - c[:, None, :]                                   # (n, V, 3)
        cosm = np.einsum("nvk,nk->nv", e, nrm) - min_cos * np.sqrt((e * e).sum(2))
        valid &= cosm[np.arange(n), r] > 0
        x0, y0 = np.where(valid, x0, wid), np.where(valid, y0, wid)
        dy, dx = np.mgrid[-wid:wid + 1, -wid:wid + 1]
        qx = (x0[:, None] + dx.ravel()[None, :]).astype(np.float64)         # (n, N)
        qy = (y0[:, None] + dy.ravel()[None, :]).astype(np.float64)
        a = g[r[:, None], y0[:, None] + dy.ravel()[None, :], x0[:, None] + dx.ravel()[None, :]]
        Sa = a.sum(1)
        Da = N * (a * a).sum(1) - Sa * Sa
        valid &= Da > 0
        ray = np.stack([(qx - K[r, 0, 2][:, None]) / K[r, 0, 0][:, None],
                        (qy - K[r, 1, 2][:, None]) / K[r, 1, 1][:, None], np.ones_like(qx)], 2)
        d = np.einsum("nki,nij->nkj", ray, Rr)                              # rows Rp_r^T ray
        Or = O[r]
        s = ((nrm * (c - Or)).sum(1))[:, None] / np.einsum("nkj,nj->nk", d, nrm)
        X = Or[:, None, :] + d * s[:, :, None]                              # (n, N, 3)
        for v in range(V):
            rows = np.flatnonzero(valid & (r != v) & (cosm[:, v] > 0))
            if len(rows) == 0:
                continue
            P = X[rows] @ Rp[v].T + t[v]
            sx = P[:, :, 0] / P[:, :, 2] * K[v, 0, 0] + K[v, 0, 2]
            sy = P[:, :, 1] / P[:, :, 2] * K[v, 1, 1] + K[v, 1, 2]
            ok = np.all(P[:, :, 2] > 0, 1) & np.all(np.isfinite(sx) & np.isfinite(sy), 1)
            ok &= np.all((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1), 1)
            rows, sx, sy = rows[ok], sx[ok], sy[ok]
            if len(rows) == 0:
                continue
            b = wr.bilinear(g[v], sx.ravel(), sy.ravel()).reshape(sx.shape)
            Sb = b.sum(1)
            Db = N * (b * b).sum(1) - Sb * Sb
            val = (N * (a[rows] * b).sum(1) - Sa[rows] * Sb) / np.sqrt(Da[rows] * Db) * N / (N - 1)
            ncc[rows, v] = np.where(Db > 0, val, np.nan)
        ps = ncc > min_ncc
    count = ps.sum(1).astype(np.int32)
    avg = np.where(count > 0, np.where(ps, ncc, 0.0).sum(1) / np.maximum(count, 1), 0.0)
    mask = np.zeros((n, words), np.uint64)
    for v in range(V):
        mask[:, v >> 6] |= ps[:, v].astype(np.uint64) << np.uint64(v & 63)
    return mask, count, avg, ncc


def seed_jobs(K, Rp, t, W, H, c, ref, cell):
    """Round 0: job (-1, ref, cell of the seed's projection into ref) and
    in-grid flags (a seed outside the grid gets the cell (-1, -1))."""
    jobs = np.full((len(ref), 4), -1, np.int32)
    inside = np.zeros(len(ref), bool)
    for k in range(len(ref)):
        jobs[k, 1] = ref[k]
        ij = cell_of(K, Rp, t, int(ref[k]), c[k], W, H, cell)
        if ij is not None:
            jobs[k, 2:] = ij
            inside[k] = True
    return jobs, inside


def default_max_dist(K, Rp, t, c0, r0, cell):
    """2 cell_size pixels at the first seed's depth in its reference view."""
    return 2.0 * cell * float(rr.depth_steps(K, Rp, t, np.asarray(c0).reshape(1, 3), np.array([r0]), 1.0)[0])


def refine_winners(gray, K, Rp, t, cc, cn, cref, ncc, wid, min_ncc, min_cos, levels, max_views, depth_px, vlb,
                   avg, scorer=score_batch):
    """Step 4 of a round on the winners' arrays: refine, re-score and keep the
    refined patch when its count >= vlb and its avg >= the winner's ->
    (kept flags, c', nrm', mask', count', avg') of the refined patches."""
    lists = rr.view_lists(ncc, min_ncc, max_views)
    ds = rr.depth_steps(K, Rp, t, cc, cref, depth_px)
    c2, n2, _ = rr.refine_reference(gray, K, Rp, t, cc, cn, cref, lists, ds, wid, min_cos, levels, 2, 1)
    m2, k2, a2, _ = scorer(gray, K, Rp, t, c2, n2, cref, wid, min_ncc, min_cos)
    kept = (k2 >= vlb) & (a2 >= avg)
    return kept, c2, n2, m2, k2, a2


def expand_chain(gray, K, Rp, t, c, nrm, ref, rounds, cell=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2,
                 max_dist=None, refine_levels=0, max_views=8, depth_px=1.0, max_patches=None,
                 scorer=score_batch):
    """The chain of MvsContext.expand_warped on the CPU -> dict of the patch
    arrays (c, nrm, ref, mask, count, avg, round, parent, cell) and occ.
    scorer: score_batch (warped_reference itself) or score_batch_fast."""
    gray = np.asarray(gray)
    V, H, W = gray.shape
    nci, ncj = grid_shape(W, H, cell)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    ref = np.asarray(ref, np.int32).reshape(-1)
    if max_dist is None:
        max_dist = default_max_dist(K, Rp, t, c[0], ref[0], cell)
    occ = np.zeros((V, ncj, nci), np.uint8)
    out = {k: [] for k in ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell")}
    total = 0
    base = 0          # index of the frontier's first patch in the patch set
    front = None
    for rnd in range(rounds):
        if rnd == 0:
            jobs, inside = seed_jobs(K, Rp, t, W, H, c, ref, cell)
            cc, cn, cref = c.copy(), nrm.copy(), ref.copy()
        else:
            jobs, cc, cn, cref = children(K, Rp, t, W, H, front[0], front[1], front[2], front[3], cell, occ, max_dist)
            inside = np.ones(len(jobs), bool)
        if len(jobs) == 0:
            break
        mask, count, avg, ncc = scorer(gray, K, Rp, t, cc, cn, cref, wid, min_ncc, min_cos)
        accept = ((count >= vlb) & inside).astype(np.uint8)
        win = claim(jobs, accept, avg, V, nci, ncj)
        wk = np.flatnonzero(win)
        if max_patches is not None and total + len(wk) > max_patches:
            wk = wk[:max(max_patches - total, 0)]
            win = np.zeros_like(win)
            win[wk] = 1
        if len(wk) == 0:
            break
        if refine_levels > 0:
            kept, c2, n2, m2, k2, a2 = refine_winners(gray, K, Rp, t, cc[wk], cn[wk], cref[wk], ncc[wk], wid, min_ncc,
                                                      min_cos, refine_levels, max_views, depth_px, vlb, avg[wk],
                                                      scorer)
            for a, k in enumerate(wk):
                if kept[a]:
                    cc[k], cn[k], mask[k], count[k], avg[k] = c2[a], n2[a], m2[a], k2[a], a2[a]
        mark(K, Rp, t, W, H, jobs, win, cc, cref, mask, cell, occ)
        front = (cc[wk], cn[wk], cref[wk], mask[wk])
        out["c"].append(cc[wk]); out["nrm"].append(cn[wk]); out["ref"].append(cref[wk]); out["mask"].append(mask[wk])
        out["count"].append(count[wk]); out["avg"].append(avg[wk])
        out["round"].append(np.full(len(wk), rnd, np.int32))
        out["parent"].append(np.where(jobs[wk, 0] >= 0, jobs[wk, 0] + base, -1).astype(np.int64))
        out["cell"].append(jobs[wk, 2:])
        base = total
        total += len(wk)
        if max_patches is not None and total >= max_patches:
            break
    words = (V + 63) // 64
    empty = {"c": (0, 3), "nrm": (0, 3), "ref": (0,), "mask": (0, words), "count": (0,), "avg": (0,), "round": (0,),
             "parent": (0,), "cell": (0, 2)}
    res = {k: np.concatenate(v) if v else np.zeros(empty[k]) for k, v in out.items()}
    res["occ"] = occ
    res["max_dist"] = max_dist
    return res
