"""Float64 numpy restatement of one sweep of the per-pixel plane propagation
(mvs_wprop_sweep, include/mvs_amd.h), built on warped_reference
(positions_rayplane, bilinear), refine_reference's normal rule (tangent_basis,
tangents) and depth_reference.pixel_ray, which stay as they are.  The
definition in the header is the specification.

pixel_reference is the definition one pixel at a time, in the order of the
header's text.  sweep_view takes the pixels of a view together (the larger maps
need it); test_wprop_host.py holds it against pixel_reference.  Both return, per
(pixel, hypothesis), the score, the per-view ncc, sigma_b, the border margin and
the min_cos margins, as refine_level_reference does.  chain() is
MvsContext.densify_depth's sweep loop on the CPU.
"""
import math

import numpy as np

import depth_reference as dr
import expand_reference as er
import refine_reference as rr
import warped_reference as wr

SCHEDULE = tuple((st, 1, 1, 1.0 if k < 4 else 0.5) for k, st in enumerate((1, 3, 1, 5, 1, 3, 1, 1, 1, 1, 1, 1)))
ASTEP = math.radians(8)
DEPTH_PX = 1.0
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1))   # h = 1..4: (dx, dy) in units of step


def n_hyp(kd, ka):
    return 5 + (2 * kd + 1) * (2 * ka + 1) ** 2


def holds(z, n):
    """A pixel holds a plane: a finite depth > 0 and no nan in the normal."""
    z = np.asarray(z, np.float64)
    n = np.asarray(n, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0) & ~np.isnan(n).any(-1)


def list_of(row):
    return [int(u) for u in row if u >= 0]


def topk_score(ncc, min_ncc, top_k):
    """Step 3's rule on one hypothesis's ncc (T,) in list order -> (score or nan,
    the chosen entries in the order they are added)."""
    with np.errstate(invalid="ignore"):
        passing = [k for k in range(len(ncc)) if ncc[k] > min_ncc]
    if len(passing) < top_k:
        return np.nan, []
    order = sorted(passing, key=lambda k: (-float(ncc[k]), k))[:top_k]
    total = 0.0
    for k in order:
        total = total + float(ncc[k])
    return total / top_k, order


def choose(scores):
    """Step 4: h = 0 is kept unless another valid hypothesis scores strictly
    higher; among the others the highest wins, ties to the lowest h."""
    best = -1
    for h in range(1, len(scores)):
        if np.isnan(scores[h]):
            continue
        if best < 0 or scores[h] > scores[best]:
            best = h
    if not np.isnan(scores[0]) and (best < 0 or not scores[best] > scores[0]):
        best = 0
    return best


def pixel_planes(K, Rp, t, zmap_v, nmap_v, v, qx, qy, step, kd, ka, astep, depth_px, step_scale):
    """Step 2 for one pixel -> zh (HY,), nh (HY,3), exists (HY,) in Python floats."""
    Hh, W = zmap_v.shape
    HY = n_hyp(kd, ka)
    cam = er._cam(K, Rp, t, v)
    R9, t3, fx, fy, cx, cy = cam
    dq = dr.pixel_ray(R9, fx, fy, cx, cy, qx, qy)
    zh = np.full(HY, np.nan)
    nh = np.full((HY, 3), np.nan)
    exists = np.zeros(HY, bool)
    own = bool(holds(zmap_v[qy, qx], nmap_v[qy, qx]))
    if own:
        zh[0], nh[0], exists[0] = zmap_v[qy, qx], nmap_v[qy, qx], True
    for h, (ox, oy) in enumerate(OFFSETS, 1):
        nx, ny = qx + ox * step, qy + oy * step
        if not (0 <= nx < W and 0 <= ny < Hh) or not holds(zmap_v[ny, nx], nmap_v[ny, nx]):
            continue
        zn = float(zmap_v[ny, nx])
        n = [float(x) for x in nmap_v[ny, nx]]
        dn = dr.pixel_ray(R9, fx, fy, cx, cy, nx, ny)
        num = zn * (n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2])
        den = n[0] * dq[0] + n[1] * dq[1] + n[2] * dq[2]
        if den == 0.0:
            continue
        z = num / den
        if not (math.isfinite(z) and z > 0):
            continue
        zh[h], nh[h], exists[h] = z, nmap_v[ny, nx], True
    if own:
        z0 = float(zmap_v[qy, qx])
        n0 = np.array(nmap_v[qy, qx], np.float64)
        dz = (depth_px * z0) / ((fx + fy) / 2)
        e1, e2 = rr.tangent_basis(n0)
        tn = rr.tangents(ka, astep, step_scale)
        h = 5
        for k in range(-kd, kd + 1):
            for j in range(-ka, ka + 1):
                for i in range(-ka, ka + 1):
                    if not (k == 0 and i == 0 and j == 0):
                        if i == 0 and j == 0:
                            n = n0.copy()
                        else:
                            n = n0 + tn[i + ka] * e1 + tn[j + ka] * e2
                            n = n / math.sqrt(float(n @ n))
                        zh[h], nh[h], exists[h] = z0 + (float(k) * dz) * step_scale, n, True
                    h += 1
    return zh, nh, exists


def pixel_reference(gray, K, Rp, t, zmap_v, nmap_v, v, qx, qy, lst, wid=5, min_cos=0.3, min_ncc=0.7, top_k=2, step=1,
                    kd=1, ka=1, astep=ASTEP, depth_px=DEPTH_PX, step_scale=1.0):
    """One pixel of view v against the list lst (entries >= 0).  Returns a dict:
      ok        the pixel test passed
      zh, nh, exists   the hypotheses' geometry
      scores    (HY,) nan where the hypothesis does not exist or is invalid
      ncc, sigma_b, border   (HY, T) per list view (border: -inf with a sample of no positive depth)
      cosm      (HY, T + 1) margins of the facing tests: the own camera, then the list views
      chosen    per hypothesis the list positions whose ncc are averaged
      best, score, z_out, n_out   the choice"""
    gray = np.asarray(gray)
    V, Hh, W = gray.shape
    K = np.asarray(K, np.float64).reshape(V, 3, 3)
    Rp = np.asarray(Rp, np.float64).reshape(V, 3, 3)
    t = np.asarray(t, np.float64).reshape(V, 3)
    HY, T = n_hyp(kd, ka), len(lst)
    S = 2 * wid + 1
    N = S * S
    out = {"ok": False, "scores": np.full(HY, np.nan), "best": -1, "score": np.nan, "z_out": np.inf,
           "n_out": np.full(3, np.nan), "ncc": np.full((HY, T), np.nan), "sigma_b": np.full((HY, T), np.nan),
           "border": np.full((HY, T), np.nan), "cosm": np.full((HY, T + 1), np.nan), "chosen": [[] for _ in range(HY)]}
    out["zh"], out["nh"], out["exists"] = pixel_planes(K, Rp, t, zmap_v, nmap_v, v, qx, qy, step, kd, ka, astep,
                                                       depth_px, step_scale)
    if not (qx - wid >= 0 and qx + wid <= W - 1 and qy - wid >= 0 and qy + wid <= Hh - 1):
        return out
    a = gray[v, qy - wid:qy + wid + 1, qx - wid:qx + wid + 1].astype(np.float64).ravel() - 128.0
    Sa = a.sum()
    Da = N * (a * a).sum() - Sa * Sa
    if not Da > 0:
        return out
    out["ok"] = True
    R9, t3, fx, fy, cx, cy = er._cam(K, Rp, t, v)
    O = np.array(er.centre_of(R9, t3))
    dq = np.array(dr.pixel_ray(R9, fx, fy, cx, cy, qx, qy))
    Os = wr.centres(Rp, t)
    q = wr.window_pixels(qx, qy, wid)
    g = {u: gray[u].astype(np.float64) - 128.0 for u in lst}
    for h in range(HY):
        if not out["exists"][h]:
            continue
        n = out["nh"][h]
        X = O + out["zh"][h] * dq
        ee = np.concatenate([[O], Os[lst]]).reshape(-1, 3) - X
        out["cosm"][h] = (ee * n).sum(1) - min_cos * np.sqrt((ee * ee).sum(1))
        for k, u in enumerate(lst):
            if not out["cosm"][h, k + 1] > 0:
                continue
            pos, z = wr.positions_rayplane(K, Rp, t, X, n, v, u, q)
            sx, sy = pos[:, 0], pos[:, 1]
            if not np.all(z > 0) or not np.all(np.isfinite(pos)):
                out["border"][h, k] = -np.inf
                continue
            m = min(sx.min(), (W - 1 - sx).min(), sy.min(), (Hh - 1 - sy).min())
            out["border"][h, k] = m
            if m < 0:
                continue
            b = wr.bilinear(g[u], sx, sy)
            Sb = b.sum()
            Db = N * (b * b).sum() - Sb * Sb
            out["sigma_b"][h, k] = math.sqrt(max(Db, 0.0)) / N
            if not Db > 0:
                continue
            out["ncc"][h, k] = (N * (a * b).sum() - Sa * Sb) / math.sqrt(Da * Db) * N / (N - 1)
        if out["cosm"][h, 0] > 0:
            out["scores"][h], out["chosen"][h] = topk_score(out["ncc"][h], min_ncc, top_k)
    best = choose(out["scores"])
    if best >= 0:
        out.update(best=best, score=float(out["scores"][best]), z_out=float(out["zh"][best]),
                   n_out=np.array(out["nh"][best]))
    return out


# ---- a view's pixels together ----

def _rays(cam, xs, ys):
    """dr.pixel_ray elementwise: (..., 3)."""
    R9, t3, fx, fy, cx, cy = cam
    u = (np.asarray(xs, np.float64) - cx) / fx
    w = (np.asarray(ys, np.float64) - cy) / fy
    return np.stack([R9[k] * u + R9[3 + k] * w + R9[6 + k] for k in range(3)], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def view_planes(cam, zmap_v, nmap_v, step, kd, ka, astep, depth_px, step_scale):
    """Step 2 for every pixel of a view -> zh (H,W,HY), nh (H,W,HY,3), exists (H,W,HY)."""
    Hh, W = zmap_v.shape
    HY = n_hyp(kd, ka)
    R9, t3, fx, fy, cx, cy = cam
    ys, xs = np.mgrid[0:Hh, 0:W]
    dq = _rays(cam, xs, ys)
    zh = np.full((Hh, W, HY), np.nan)
    nh = np.full((Hh, W, HY, 3), np.nan)
    exists = np.zeros((Hh, W, HY), bool)
    own = holds(zmap_v, nmap_v)
    zh[..., 0] = np.where(own, zmap_v, np.nan)
    nh[..., 0, :] = np.where(own[..., None], nmap_v, np.nan)
    exists[..., 0] = own
    with np.errstate(all="ignore"):
        for h, (ox, oy) in enumerate(OFFSETS, 1):
            nx, ny = xs + ox * step, ys + oy * step
            inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < Hh)
            cx_, cy_ = np.clip(nx, 0, W - 1), np.clip(ny, 0, Hh - 1)
            zn, nn = zmap_v[cy_, cx_], nmap_v[cy_, cx_]
            dn = _rays(cam, nx, ny)
            num = zn * _dot(nn, dn)
            den = _dot(nn, dq)
            z = num / den
            e = inside & holds(zn, nn) & (den != 0.0) & np.isfinite(z) & (z > 0)
            zh[..., h] = np.where(e, z, np.nan)
            nh[..., h, :] = np.where(e[..., None], nn, np.nan)
            exists[..., h] = e
        n0 = nmap_v
        dz = (depth_px * zmap_v) / ((fx + fy) / 2)
        ab = np.abs(n0)
        m = np.where((ab[..., 0] <= ab[..., 1]) & (ab[..., 0] <= ab[..., 2]), 0, np.where(ab[..., 1] <= ab[..., 2], 1, 2))
        zero = np.zeros_like(zmap_v)
        vx = np.where(m == 1, -n0[..., 2], np.where(m == 2, n0[..., 1], zero))
        vy = np.where(m == 0, n0[..., 2], np.where(m == 2, -n0[..., 0], zero))
        vz = np.where(m == 0, -n0[..., 1], np.where(m == 1, n0[..., 0], zero))
        v = np.stack([vx, vy, vz], -1)
        e1 = v / np.sqrt(_dot(v, v))[..., None]
        e2 = np.stack([n0[..., 1] * e1[..., 2] - n0[..., 2] * e1[..., 1], n0[..., 2] * e1[..., 0] - n0[..., 0] * e1[..., 2],
                       n0[..., 0] * e1[..., 1] - n0[..., 1] * e1[..., 0]], -1)
        tn = rr.tangents(ka, astep, step_scale)
        h = 5
        for k in range(-kd, kd + 1):
            for j in range(-ka, ka + 1):
                for i in range(-ka, ka + 1):
                    if not (k == 0 and i == 0 and j == 0):
                        if i == 0 and j == 0:
                            n = n0
                        else:
                            w = n0 + tn[i + ka] * e1 + tn[j + ka] * e2
                            n = w / np.sqrt(_dot(w, w))[..., None]
                        zh[..., h] = np.where(own, zmap_v + (float(k) * dz) * step_scale, np.nan)
                        nh[..., h, :] = np.where(own[..., None], n, np.nan)
                        exists[..., h] = own
                    h += 1
    return zh, nh, exists


def sweep_view(gray, K, Rp, t, zmap_v, nmap_v, v, lst, wid=5, min_cos=0.3, min_ncc=0.7, top_k=2, step=1, kd=1, ka=1,
               astep=ASTEP, depth_px=DEPTH_PX, step_scale=1.0, details=True):
    """Every pixel of view v -> dict of arrays: z_out (H,W), n_out (H,W,3), score,
    best, scores (H,W,HY), zh, nh, exists and, with details, ncc, sigma_b, border
    (H,W,HY,T), cosm (H,W,HY,T+1) and chosen (H,W,HY,T) bool."""
    gray = np.asarray(gray)
    V, Hh, W = gray.shape
    K = np.asarray(K, np.float64).reshape(V, 3, 3)
    Rp = np.asarray(Rp, np.float64).reshape(V, 3, 3)
    t = np.asarray(t, np.float64).reshape(V, 3)
    zmap_v = np.asarray(zmap_v, np.float64).reshape(Hh, W)
    nmap_v = np.asarray(nmap_v, np.float64).reshape(Hh, W, 3)
    HY, T = n_hyp(kd, ka), len(lst)
    S = 2 * wid + 1
    N = S * S
    cam = er._cam(K, Rp, t, v)
    O = np.array(er.centre_of(cam[0], cam[1]))
    zh, nh, exists = view_planes(cam, zmap_v, nmap_v, step, kd, ka, astep, depth_px, step_scale)
    out = {"zh": zh, "nh": nh, "exists": exists, "scores": np.full((Hh, W, HY), np.nan)}
    ncc_all = np.full((Hh, W, HY, T), np.nan)
    if details:
        out["ncc"] = ncc_all
        out["sigma_b"] = np.full((Hh, W, HY, T), np.nan)
        out["border"] = np.full((Hh, W, HY, T), np.nan)
        out["cosm"] = np.full((Hh, W, HY, T + 1), np.nan)
        out["chosen"] = np.zeros((Hh, W, HY, T), bool)
    # the pixel test
    gv = gray[v].astype(np.float64) - 128.0
    ok = np.zeros((Hh, W), bool)
    if Hh > 2 * wid and W > 2 * wid:
        win = np.lib.stride_tricks.sliding_window_view(gv, (S, S)).reshape(Hh - 2 * wid, W - 2 * wid, N)
        Sa_m = win.sum(-1)
        Da_m = N * (win * win).sum(-1) - Sa_m * Sa_m
        ok[wid:Hh - wid, wid:W - wid] = Da_m > 0
    out["ok"] = ok
    dyw, dxw = np.mgrid[-wid:wid + 1, -wid:wid + 1]
    dyw, dxw = dyw.ravel(), dxw.ravel()
    Os = wr.centres(Rp, t)
    g = {u: gray[u].astype(np.float64) - 128.0 for u in lst}
    with np.errstate(all="ignore"):
        for h in range(HY):
            qy, qx = np.nonzero(ok & exists[..., h])
            P = len(qy)
            if P == 0:
                continue
            n = nh[qy, qx, h]                                   # (P,3)
            z = zh[qy, qx, h]
            dq = _rays(cam, qx, qy)
            X = O + z[:, None] * dq
            e = O - X
            cos0 = _dot(n, e) - min_cos * np.sqrt(_dot(e, e))
            a = gv[qy[:, None] + dyw, qx[:, None] + dxw]        # (P,N)
            Sa = a.sum(1)
            Da = N * (a * a).sum(1) - Sa * Sa
            dwin = _rays(cam, qx[:, None] + dxw, qy[:, None] + dyw)   # (P,N,3)
            nd = _dot(n[:, None, :], dwin)
            hh = _dot(n, X - O)
            s = hh[:, None] / nd
            Xs = O + dwin * s[..., None]
            ncc = np.full((P, T), np.nan)
            if details:
                out["cosm"][qy, qx, h, 0] = cos0
            for k, u in enumerate(lst):
                eu = Os[u] - X
                cosu = _dot(n, eu) - min_cos * np.sqrt(_dot(eu, eu))
                Pc = Xs @ Rp[u].T + t[u]
                sx = Pc[..., 0] / Pc[..., 2] * K[u, 0, 0] + K[u, 0, 2]
                sy = Pc[..., 1] / Pc[..., 2] * K[u, 1, 1] + K[u, 1, 2]
                front = np.all(Pc[..., 2] > 0, 1) & np.all(np.isfinite(sx), 1) & np.all(np.isfinite(sy), 1)
                border = np.minimum(np.minimum(sx.min(1), (W - 1 - sx).min(1)), np.minimum(sy.min(1), (Hh - 1 - sy).min(1)))
                border = np.where(front, border, -np.inf)
                inside = front & (border >= 0)
                sxc = np.where(inside[:, None], sx, 0.0)
                syc = np.where(inside[:, None], sy, 0.0)
                b = wr.bilinear(g[u], sxc.ravel(), syc.ravel()).reshape(P, N)
                Sb = b.sum(1)
                Db = N * (b * b).sum(1) - Sb * Sb
                val = (N * (a * b).sum(1) - Sa * Sb) / np.sqrt(Da * Db) * N / (N - 1)
                tested = cosu > 0
                good = tested & inside & (Db > 0)
                ncc[:, k] = np.where(good, val, np.nan)
                if details:
                    out["cosm"][qy, qx, h, k + 1] = cosu
                    out["border"][qy, qx, h, k] = np.where(tested, border, np.nan)
                    out["sigma_b"][qy, qx, h, k] = np.where(tested & inside, np.sqrt(np.maximum(Db, 0.0)) / N, np.nan)
            ncc_all[qy, qx, h] = ncc
            # step 3: the top_k largest passing ncc, descending, equal values in list order
            key = np.where(ncc > min_ncc, ncc, -np.inf)
            order = np.argsort(-key, axis=1, kind="stable")[:, :top_k]
            total = np.zeros(P) if T >= top_k else np.full(P, -np.inf)   # a list shorter than top_k: nothing is valid
            for r in range(min(top_k, T)):
                total = total + np.take_along_axis(key, order[:, r:r + 1], 1)[:, 0]
            valid = (cos0 > 0) & np.isfinite(total)
            out["scores"][qy, qx, h] = np.where(valid, total / top_k, np.nan)
            if details:
                ch = np.zeros((P, T), bool)
                np.put_along_axis(ch, order, True, 1)
                out["chosen"][qy, qx, h] = ch & valid[:, None]
    sc = out["scores"]
    others = np.where(np.isnan(sc), -np.inf, sc)
    others[..., 0] = -np.inf
    bo = np.argmax(others, -1)                                   # the first maximum: the lowest h
    so = np.take_along_axis(others, bo[..., None], -1)[..., 0]
    s0 = sc[..., 0]
    with np.errstate(invalid="ignore"):
        keep0 = ~np.isnan(s0) & ~(so > s0)
    best = np.where(keep0, 0, np.where(so > -np.inf, bo, -1)).astype(np.int32)
    bi = np.maximum(best, 0)[..., None]
    out["best"] = best
    out["score"] = np.where(best >= 0, np.take_along_axis(sc, bi, -1)[..., 0], np.nan)
    out["z_out"] = np.where(best >= 0, np.take_along_axis(zh, bi, -1)[..., 0], np.inf)
    out["n_out"] = np.where((best >= 0)[..., None], np.take_along_axis(nh, bi[..., None], 2)[..., 0, :], np.nan)
    return out


def sweep(gray, K, Rp, t, zmap, nmap, v0, lists, details=False, **kw):
    """mvs_wprop_sweep over the view range v0 .. v0 + len(lists) - 1 -> dict of
    stacked arrays (z, normal, score, best, scores and, with details, the rest)."""
    outs = [sweep_view(gray, K, Rp, t, zmap[k], nmap[k], v0 + k, list_of(lists[k]), details=details, **kw)
            for k in range(len(lists))]
    res = {"z": np.stack([o["z_out"] for o in outs]), "normal": np.stack([o["n_out"] for o in outs]),
           "score": np.stack([o["score"] for o in outs]), "best": np.stack([o["best"] for o in outs]),
           "scores": np.stack([o["scores"] for o in outs]), "views": outs}
    return res


def chain(gray, K, Rp, t, zmap, nmap, v0, lists, schedule=SCHEDULE, wid=5, min_cos=0.3, min_ncc=0.7, top_k=2):
    """densify_depth's sweep loop -> z, normal, score, best of the last sweep and history (sweeps, 2)."""
    z, n = np.asarray(zmap, np.float64), np.asarray(nmap, np.float64)
    hist = []
    res = {"z": z, "normal": n}
    for step, kd, ka, scale in schedule:
        res = sweep(gray, K, Rp, t, z, n, v0, lists, wid=wid, min_cos=min_cos, min_ncc=min_ncc, top_k=top_k, step=step,
                    kd=kd, ka=ka, astep=ASTEP, depth_px=DEPTH_PX, step_scale=scale)
        z, n = res["z"], res["normal"]
        hist.append((int((res["best"] >= 0).sum()), int((res["best"] > 0).sum())))
    res["history"] = np.array(hist, np.int64).reshape(-1, 2)
    return res
