"""Restatement of the resumed expansion (MvsContext.resume_warped) and of the
expand -> filter loop (MvsContext.reconstruct_warped), built on
expand_reference (children, claim, mark, the scorers, refine_winners) and on
support_reference.filter_chain, which stay as they are.  A plain module (the
tests import it); the methods' docstrings are the specification.
"""
import numpy as np

import expand_reference as er
import support_reference as sr

KEYS = ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell")


def occ_of(K, Rp, t, W, H, ref, cell_ij, c, mask, cell):
    """The occupancy of a set's rows: expand_reference.mark with the jobs (-1, ref, cell)."""
    nci, ncj = er.grid_shape(W, H, cell)
    jobs = np.column_stack([np.full(len(ref), -1), ref, np.asarray(cell_ij).reshape(-1, 2)]).astype(np.int32)
    return er.mark(K, Rp, t, W, H, jobs, np.ones(len(ref), np.uint8), c, ref, mask, cell,
                   np.zeros((len(K), ncj, nci), np.uint8))


def resume(gray, K, Rp, t, patches, rounds, cell=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2, max_dist=None,
           refine_levels=0, max_views=8, depth_px=1.0, max_patches=None, scorer=er.score_batch):
    """MvsContext.resume_warped on the CPU: every round's frontier is the whole
    current set in row order; no input row is scored again."""
    gray = np.asarray(gray)
    V, H, W = gray.shape
    nci, ncj = er.grid_shape(W, H, cell)
    ps = {k: np.array(patches[k]) for k in KEYS}
    n = len(ps["ref"])
    if n and (ps["ref"].min() < 0 or ps["ref"].max() >= V):
        raise ValueError("a row is dead")
    if n and (ps["cell"].min() < 0 or ps["cell"][:, 0].max() >= nci or ps["cell"][:, 1].max() >= ncj):
        raise ValueError("a cell lies outside the grid")
    occ = patches.get("occ")
    if occ is not None and np.asarray(occ).shape == (V, ncj, nci):
        occ = np.array(occ, np.uint8)
    else:
        occ = occ_of(K, Rp, t, W, H, ps["ref"], ps["cell"], ps["c"], ps["mask"], cell)
    if max_dist is None:
        max_dist = patches.get("max_dist")
    if max_dist is None and n:
        max_dist = er.default_max_dist(K, Rp, t, ps["c"][0], ps["ref"][0], cell)
    rnd = int(ps["round"].max()) + 1 if n else 0
    for _ in range(rounds):
        total = len(ps["ref"])
        if max_patches is not None and total >= max_patches:
            break
        jobs, cc, cn, cref = er.children(K, Rp, t, W, H, ps["c"], ps["nrm"], ps["ref"], ps["mask"], cell, occ, max_dist)
        if len(jobs) == 0:
            break
        mask, count, avg, ncc = scorer(gray, K, Rp, t, cc, cn, cref, wid, min_ncc, min_cos)
        win = er.claim(jobs, (count >= vlb).astype(np.uint8), avg, V, nci, ncj)
        wk = np.flatnonzero(win)
        if max_patches is not None and total + len(wk) > max_patches:
            wk = wk[:max(max_patches - total, 0)]
            win = np.zeros_like(win)
            win[wk] = 1
        if len(wk) == 0:
            break
        if refine_levels > 0:
            kept, c2, n2, m2, k2, a2 = er.refine_winners(gray, K, Rp, t, cc[wk], cn[wk], cref[wk], ncc[wk], wid, min_ncc,
                                                         min_cos, refine_levels, max_views, depth_px, vlb, avg[wk],
                                                         scorer)
            for a, k in enumerate(wk):
                if kept[a]:
                    cc[k], cn[k], mask[k], count[k], avg[k] = c2[a], n2[a], m2[a], k2[a], a2[a]
        er.mark(K, Rp, t, W, H, jobs, win, cc, cref, mask, cell, occ)
        new = {"c": cc[wk], "nrm": cn[wk], "ref": cref[wk], "mask": mask[wk], "count": count[wk], "avg": avg[wk],
               "round": np.full(len(wk), rnd, np.int32), "parent": jobs[wk, 0].astype(np.int64), "cell": jobs[wk, 2:]}
        ps = {k: np.concatenate([ps[k], new[k].astype(ps[k].dtype)]) for k in KEYS}
        rnd += 1
    ps["occ"] = occ
    ps["max_dist"] = max_dist
    return ps


def renumber(parent, index, n):
    """The parents of the surviving rows `index` of an n-row set in the
    survivors' numbering: removed -> -2; -1 (a seed) and -2 stay."""
    new = {int(old): k for k, old in enumerate(index)}
    return np.array([int(p) if p < 0 else new.get(int(p), -2) for p in parent], np.int64)


def filter_step(gray, K, Rp, t, ps, cell, **filt):
    """One filter_warped on a set -> the survivors' dict (parent in the input's
    numbering) with keep, index, removed, removed_support and occ."""
    V, H, W = np.asarray(gray).shape
    res = sr.filter_chain(K, Rp, t, W, H, ps["c"], ps["nrm"], ps["ref"], ps["mask"], ps["avg"], cell, **filt)
    idx = np.flatnonzero(res["keep"])
    out = {k: np.asarray(ps[k])[idx] for k in KEYS}
    out.update(keep=res["keep"], index=idx, removed=res["removed"], removed_support=res.get("removed_support", []))
    out["occ"] = occ_of(K, Rp, t, W, H, out["ref"], out["cell"], out["c"], out["mask"], cell)
    return out


def planted_set(pkg, rad=0.02):
    """A set for the loop with wrong patches in it, from the quality
    experiment's mixed set (support_reference.sphere_mixed): the chain's rows,
    each outlier put in the place of the chain patch it was made from (it takes
    over that row's ref and cell, so the set keeps one patch per (ref, cell)
    and every cell inside the grid).  Every row counts as a seed (round 0,
    parent -1).  -> (set dict with max_dist and kind, rows of the outliers)."""
    m = sr.sphere_mixed(pkg, rad)
    s = m["set"]
    P = int((s["kind"] == 0).sum())
    # filter_reference.mixed_set's choice, to find each outlier's source row
    pick = np.random.default_rng(7).permutation(P)[:300]
    sign = np.where(np.arange(len(pick)) % 2 == 0, 1.0, -1.0)
    radial = s["c"][pick] / np.linalg.norm(s["c"][pick], axis=1, keepdims=True)
    moved = {(s["c"][pick] + (sign * 0.002)[:, None] * radial)[k].tobytes(): int(pick[k]) for k in range(len(pick))}
    src = np.array([moved[row.tobytes()] for row in s["c"][P:]])
    out = {k: s[k][:P].copy() for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")}
    for k in ("c", "nrm", "mask", "avg", "kind"):
        out[k][src] = s[k][P:]
    assert np.array_equal(out["ref"][src], s["ref"][P:])
    out["count"] = np.array([sum(bin(int(w)).count("1") for w in row) for row in out["mask"]], np.int32)
    out["round"] = np.zeros(P, np.int32)
    out["parent"] = np.full(P, -1, np.int64)
    out["max_dist"] = er.default_max_dist(m["K"], m["Rp"], m["t"], out["c"][0], out["ref"][0], 2)
    return out, src


def reconstruct(gray, K, Rp, t, c, nrm, ref, iterations=3, rounds=4, resume_rounds=2, expand=None, filter=None,
                scorer=er.score_batch, start=None):
    """MvsContext.reconstruct_warped on the CPU.  expand: cell, wid, min_ncc,
    min_cos, vlb, max_dist, refine_levels, max_views, depth_px, max_patches in
    expand_reference's names; filter: support_reference.filter_chain's
    keywords without cell.  start: a set to begin from in place of the
    expansion of the seeds (the tests plant outliers in it)."""
    expand, filt = dict(expand or {}), dict(filter or {})
    cell = expand.get("cell", 2)
    ps = start if start is not None else er.expand_chain(gray, K, Rp, t, c, nrm, ref, rounds, scorer=scorer, **expand)
    grow = dict(expand, max_dist=ps["max_dist"])
    history = []
    for it in range(iterations):
        before = len(ps["ref"])
        ps = filter_step(gray, K, Rp, t, ps, cell, **filt)
        ps["parent"] = renumber(ps["parent"], ps["index"], before)
        history.append({"patches": before, "removed": ps["removed"], "removed_support": ps["removed_support"],
                        "resumed": None})
        if it + 1 < iterations:
            ps = resume(gray, K, Rp, t, ps, resume_rounds, scorer=scorer, **grow)
            history[-1]["resumed"] = len(ps["ref"])
    ps["max_dist"] = grow["max_dist"]
    ps["history"] = history
    return ps
