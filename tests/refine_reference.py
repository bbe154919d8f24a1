"""Float64 numpy restatement of one level of the fixed-grid depth and normal
refinement (mvs_refine_warped, include/mvs_amd.h), one patch at a time, and of
the wrapper around it (MvsContext.refine_warped): the view-list rule and the
level loop.  Built from warped_reference's pieces, which stay as they are; the
definition in the header is the specification.
"""
import math

import numpy as np

import warped_reference as wr


def tangent_basis(nrm):
    """e1, e2 of the definition: m = index of the smallest |nrm_m| (lowest on
    ties), e1 = (nrm x axis_m) / |.|, e2 = nrm x e1."""
    nrm = np.asarray(nrm, np.float64)
    m = int(np.argmin(np.abs(nrm)))            # first minimum
    axis = np.zeros(3)
    axis[m] = 1.0
    e1 = np.cross(nrm, axis)
    e1 = e1 / math.sqrt(float(e1 @ e1))
    return e1, np.cross(nrm, e1)


def tangents(ka, astep, step_scale):
    """tan(i alpha), i = -ka..ka, alpha = astep * step_scale."""
    alpha = float(astep) * float(step_scale)
    return [math.tan(i * alpha) for i in range(-ka, ka + 1)]


def grid(c, nrm, O_r, dstep, kd, ka, astep, step_scale):
    """-> c_k (H, 3), n_ij (H, 3) in hypothesis order h = ((k+kd) A + (j+ka)) A + (i+ka).
    The unperturbed normal (i = j = 0) is nrm as given."""
    c = np.asarray(c, np.float64)
    nrm = np.asarray(nrm, np.float64)
    e = c - O_r
    u = e / math.sqrt(float(e @ e))
    e1, e2 = tangent_basis(nrm)
    tn = tangents(ka, astep, step_scale)
    ck, nij = [], []
    for k in range(-kd, kd + 1):
        cc = c + (k * float(dstep) * float(step_scale)) * u
        for j in range(-ka, ka + 1):
            for i in range(-ka, ka + 1):
                if i == 0 and j == 0:
                    n = nrm.copy()
                else:
                    n = nrm + tn[i + ka] * e1 + tn[j + ka] * e2
                    n = n / math.sqrt(float(n @ n))
                ck.append(cc)
                nij.append(n)
    return np.array(ck), np.array(nij)


def list_ok(views, V, r):
    """The list rule: entries in -1..V-1, none equal to r, none repeated, -1 only at the end."""
    views = [int(v) for v in views]
    T = sum(v >= 0 for v in views)
    head = views[:T]
    return (all(-1 <= v < V for v in views) and all(v >= 0 for v in head) and r not in head
            and len(set(head)) == T)


def refine_level_reference(gray, K, Rp, t, c, nrm, ref, views, dstep, wid=5, min_cos=0.0, kd=2, ka=1,
                           astep=math.radians(8), step_scale=1.0):
    """One level for one patch.  Returns a dict:
      valid     the candidate passed step 1 (and its list and dstep are usable)
      scores    (H,) nan where the hypothesis is invalid
      ck, nij   (H, 3) geometry of every hypothesis
      sigma_b   (H, T) population std of the warped window per list view (nan where none was sampled)
      border    (H,) smallest margin of a sample to the image border over the list (-inf: no positive depth)
      cosm      (H,) smallest |margin| of the facing tests (reference camera and list views)
      cand_cosm the candidate's own min_cos margin
      best, score_best, c_out, nrm_out   the choice (step 4)"""
    gray = np.asarray(gray)
    V, Hh, W = gray.shape
    K = np.asarray(K, np.float64).reshape(V, 3, 3)
    Rp = np.asarray(Rp, np.float64).reshape(V, 3, 3)
    t = np.asarray(t, np.float64).reshape(V, 3)
    c = np.asarray(c, np.float64).reshape(3)
    nrm = np.asarray(nrm, np.float64).reshape(3)
    r = int(ref)
    A = 2 * ka + 1
    H = (2 * kd + 1) * A * A
    S = 2 * wid + 1
    N = S * S
    out = {"valid": False, "scores": np.full(H, np.nan), "best": -1, "score_best": np.nan,
           "c_out": c.copy(), "nrm_out": nrm.copy(), "cand_cosm": np.nan, "H": H}
    O = wr.centres(Rp, t)
    if not (0 <= r < V) or not list_ok(views, V, r) or not float(dstep) > 0:
        return out
    lst = [int(v) for v in views if v >= 0]
    T = len(lst)
    out["ck"], out["nij"] = grid(c, nrm, O[r], dstep, kd, ka, astep, step_scale)
    out["sigma_b"] = np.full((H, T), np.nan)
    out["border"] = np.full(H, np.nan)
    out["cosm"] = np.full(H, np.nan)
    # step 1: the candidate test of mvs_score_warped, window and a fixed
    e = O[r] - c
    out["cand_cosm"] = float(e @ nrm - min_cos * math.sqrt(float(e @ e)))
    x, y, depth = wr.project_ref(K[r], Rp[r], t[r], c)
    if not (depth > 0 and x >= 0 and y >= 0 and abs(x) < 1e9 and abs(y) < 1e9):
        return out
    x0, y0 = int(x), int(y)
    if not (x0 - wid >= 0 and x0 + wid <= W - 1 and y0 - wid >= 0 and y0 + wid <= Hh - 1):
        return out
    if not out["cand_cosm"] > 0 or T < 1:
        return out
    a = gray[r, y0 - wid:y0 + wid + 1, x0 - wid:x0 + wid + 1].astype(np.float64).ravel() - 128.0
    Sa = a.sum()
    Da = N * (a * a).sum() - Sa * Sa
    if not Da > 0:
        return out
    out["valid"] = True
    q = wr.window_pixels(x0, y0, wid)
    g = {v: gray[v].astype(np.float64) - 128.0 for v in lst}
    for h in range(H):
        ck, n = out["ck"][h], out["nij"][h]
        ee = O[[r] + lst] - ck
        cosm = ee @ n - min_cos * np.sqrt((ee * ee).sum(1))
        out["cosm"][h] = np.abs(cosm).min()
        ok = bool(np.all(cosm > 0))
        border, total = np.inf, 0.0
        for k, v in enumerate(lst):
            pos, z = wr.positions_rayplane(K, Rp, t, ck, n, r, v, q)
            sx, sy = pos[:, 0], pos[:, 1]
            if not np.all(z > 0) or not np.all(np.isfinite(pos)):
                border = -np.inf
                ok = False
                continue
            m = min(sx.min(), (W - 1 - sx).min(), sy.min(), (Hh - 1 - sy).min())
            border = min(border, m)
            if m < 0:
                ok = False
                continue
            b = wr.bilinear(g[v], sx, sy)
            Sb = b.sum()
            Db = N * (b * b).sum() - Sb * Sb
            out["sigma_b"][h, k] = math.sqrt(max(Db, 0.0)) / N
            if not Db > 0:
                ok = False
                continue
            total = total + (N * (a * b).sum() - Sa * Sb) / math.sqrt(Da * Db) * N / (N - 1)
        out["border"][h] = border
        if ok:
            out["scores"][h] = total / T
    out.update(choose(out["scores"], out["ck"], out["nij"], c, nrm))
    return out


def choose(scores, ck, nij, c, nrm):
    """Step 4: the centre is kept unless another valid hypothesis scores
    strictly higher; among the others the highest wins, ties to the lowest index."""
    H = len(scores)
    hc = (H - 1) // 2
    best = -1
    for h in range(H):
        if h == hc or np.isnan(scores[h]):
            continue
        if best < 0 or scores[h] > scores[best]:
            best = h
    if not np.isnan(scores[hc]) and (best < 0 or not scores[best] > scores[hc]):
        best = hc
    if best < 0:
        return {"best": -1, "score_best": np.nan, "c_out": np.array(c, np.float64), "nrm_out": np.array(nrm, np.float64)}
    if best == hc:
        return {"best": hc, "score_best": float(scores[hc]), "c_out": np.array(c, np.float64),
                "nrm_out": np.array(nrm, np.float64)}
    return {"best": best, "score_best": float(scores[best]), "c_out": ck[best].copy(), "nrm_out": nij[best].copy()}


def second_best(scores, best):
    """The highest valid score among the hypotheses other than best (nan if none)."""
    s = np.array(scores, np.float64)
    if best >= 0:
        s[best] = np.nan
    return np.nan if np.all(np.isnan(s)) else float(np.nanmax(s))


def view_lists(ncc, min_ncc=0.7, max_views=8):
    """The wrapper's list rule on score_warped's ncc (n, V): the max_views
    passing views (ncc > min_ncc) with the highest ncc, ties to the lower view
    index, in ascending view order, padded with -1 -> (n, max_views) int32."""
    ncc = np.asarray(ncc, np.float64)
    n, V = ncc.shape
    out = np.full((n, max_views), -1, np.int32)
    idx = np.arange(V)
    for i in range(n):
        with np.errstate(invalid="ignore"):
            ok = ncc[i] > min_ncc
        cand = idx[ok]
        order = np.lexsort((cand, -ncc[i, cand]))
        keep = np.sort(cand[order[:max_views]])
        out[i, :len(keep)] = keep
    return out


def depth_steps(K, Rp, t, c, ref, depth_px=1.5):
    """dstep = depth_px * depth in ref / ((fx_r + fy_r) / 2)."""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    Rp = np.asarray(Rp, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    c = np.asarray(c, np.float64).reshape(-1, 3)
    ref = np.asarray(ref)
    depth = Rp[ref, 2, 0] * c[:, 0] + Rp[ref, 2, 1] * c[:, 1] + Rp[ref, 2, 2] * c[:, 2] + t[ref, 2]
    return depth_px * depth / ((K[ref, 0, 0] + K[ref, 1, 1]) / 2)


def perturbed_sphere_patches(K, R, t, Rp, n, rng, rad=0.02, depth_mm=1.5, angles=(5.0, 15.0)):
    """n patches of the sphere (warped_reference.sphere_patches, true centres
    and normals), each moved by U(-depth_mm, depth_mm) mm along its reference
    ray and tilted by U(angles) degrees about a random tangent direction.
    -> c_true, nrm_true, ref, c, nrm."""
    c0, n0, ref, _ = wr.sphere_patches(K, R, t, n, rad, rng)
    O = wr.centres(Rp, t)
    c, nrm = c0.copy(), n0.copy()
    for i in range(n):
        u = c0[i] - O[ref[i]]
        u /= math.sqrt(float(u @ u))
        c[i] = c0[i] + rng.uniform(-depth_mm, depth_mm) * 1e-3 * u
        e1, e2 = tangent_basis(n0[i])
        th, ph = math.radians(rng.uniform(*angles)), rng.uniform(0, 2 * math.pi)
        v = math.cos(th) * n0[i] + math.sin(th) * (math.cos(ph) * e1 + math.sin(ph) * e2)
        nrm[i] = v / math.sqrt(float(v @ v))
    return c0, n0, ref, c, nrm


def patch_errors(c, nrm, c_true, nrm_true):
    """Depth error |c - c_true| (both lie on the reference ray) in metres and
    the angle between nrm and nrm_true in degrees, per patch."""
    d = np.sqrt(((np.asarray(c) - c_true) ** 2).sum(1))
    cosv = np.clip((np.asarray(nrm) * nrm_true).sum(1) / np.sqrt((np.asarray(nrm) ** 2).sum(1)), -1.0, 1.0)
    return d, np.degrees(np.arccos(cosv))


def refine_reference(gray, K, Rp, t, c, nrm, ref, views, dstep, wid=5, min_cos=0.0, levels=4, kd=2, ka=1,
                     astep=math.radians(8)):
    """The level loop over a batch: level l runs with step_scale = 2^-l from
    the output of level l-1 -> c', nrm', best (levels, n)."""
    c = np.array(c, np.float64).reshape(-1, 3)
    nrm = np.array(nrm, np.float64).reshape(-1, 3)
    best = np.empty((levels, len(c)), np.int32)
    for lev in range(levels):
        for i in range(len(c)):
            o = refine_level_reference(gray, K, Rp, t, c[i], nrm[i], ref[i], views[i], dstep[i], wid, min_cos,
                                       kd, ka, astep, 2.0 ** -lev)
            c[i], nrm[i], best[lev, i] = o["c_out"], o["nrm_out"], o["best"]
    return c, nrm, best
