"""Float64 restatement of the seed matcher and the patch colours
(mvs_wseed_match_device, mvs_wpatch_color_device, include/mvs_amd.h), and the
planted feature set the seed tests share.  The geometry is written in Python
floats, product by product and sum by sum in the header's order (left to right,
unfused); the colour sums are Python integers.  Every output can be compared
exactly.  A plain module (the tests import it); the definition in the header is
the specification.
"""
import math

import numpy as np

import expand_reference as er
import warped_reference as wr


def check_scalars(epi_px, min_sin2, cap=0):
    if not (math.isfinite(epi_px) and epi_px > 0.0) or not (0.0 <= min_sin2 < 1.0) or cap < 0:
        raise ValueError("epi_px must be finite and > 0, min_sin2 in [0, 1), cap >= 0")


def check_tables(V, feat_off, pairs):
    feat_off = [int(x) for x in feat_off]
    if len(feat_off) != V + 1 or feat_off[0] != 0 or any(b < a for a, b in zip(feat_off, feat_off[1:])):
        raise ValueError("feat_off must be V + 1 offsets from 0, not decreasing")
    for r, v in pairs:
        if not (0 <= r < V and 0 <= v < V) or r == v:
            raise ValueError("a pair needs two different views of 0..V-1")


def pixel_ray(R9, fx, fy, cx, cy, x, y):
    """d = Rp^T ((x - cx) / fx, (y - cy) / fy, 1)."""
    u = (float(x) - cx) / fx
    w = (float(y) - cy) / fy
    return [R9[m] * u + R9[3 + m] * w + R9[6 + m] for m in range(3)]


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def match(K, Rp, t, feat, feat_off, pairs, epi_px, min_sin2):
    """Every candidate in the order (pair, a, b) -> dict c (n,3), nrm (n,3), ref
    (n,) int32, cand (n,4) int32 [pair, a, b, v], err (n,).  The call's first
    cap rows are the first cap of these; its total is n."""
    V = len(K)
    check_scalars(epi_px, min_sin2)
    pairs = [(int(r), int(v)) for r, v in np.asarray(pairs).reshape(-1, 2)]
    check_tables(V, feat_off, pairs)
    feat = np.asarray(feat).reshape(-1, 2)
    epi2 = float(epi_px) * float(epi_px)
    min_sin2 = float(min_sin2)
    cams = [er._cam(K, Rp, t, v) for v in range(V)]
    O = [er.centre_of(cm[0], cm[1]) for cm in cams]
    rays = {}

    def view_rays(v):
        if v not in rays:
            R9, _, fx, fy, cx, cy = cams[v]
            rays[v] = [pixel_ray(R9, fx, fy, cx, cy, int(q[0]), int(q[1]))
                       for q in feat[int(feat_off[v]):int(feat_off[v + 1])]]
        return rays[v]

    c, nrm, ref, cand, err = [], [], [], [], []
    for k, (r, v) in enumerate(pairs):
        Or, Ov = O[r], O[v]
        w = [Or[m] - Ov[m] for m in range(3)]
        R9, t3, fx, fy, cx, cy = cams[v]
        qb = [(float(int(q[0])), float(int(q[1]))) for q in feat[int(feat_off[v]):int(feat_off[v + 1])]]
        tb = [(db, dot3(db, db), dot3(db, w)) for db in view_rays(v)]
        for a, da in enumerate(view_rays(r)):
            A = dot3(da, da)
            D = dot3(da, w)
            for b, (db, C, E) in enumerate(tb):
                B = dot3(da, db)
                AC = A * C
                den = AC - B * B
                if not den > min_sin2 * AC:
                    continue
                s = (B * E - C * D) / den
                u = (A * E - B * D) / den
                if not (s > 0.0 and math.isfinite(s) and u > 0.0 and math.isfinite(u)):
                    continue
                X = [Or[m] + s * da[m] for m in range(3)]
                x = R9[0] * X[0] + R9[1] * X[1] + R9[2] * X[2] + t3[0]
                y = R9[3] * X[0] + R9[4] * X[1] + R9[5] * X[2] + t3[1]
                z = R9[6] * X[0] + R9[7] * X[1] + R9[8] * X[2] + t3[2]
                iz = 1.0 / z if z != 0.0 else 1.0
                px = x * iz * fx + cx
                py = y * iz * fy + cy
                ex = px - qb[b][0]
                ey = py - qb[b][1]
                e2 = ex * ex + ey * ey
                if not (z > 0.0 and e2 <= epi2):
                    continue
                e = [Or[m] - X[m] for m in range(3)]
                ln = math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
                c.append(X)
                nrm.append([e[m] / ln if ln != 0.0 or e[m] != 0.0 else math.nan for m in range(3)])
                ref.append(r)
                cand.append((k, a, b, v))
                err.append(e2)
    return {"c": np.array(c, np.float64).reshape(-1, 3), "nrm": np.array(nrm, np.float64).reshape(-1, 3),
            "ref": np.array(ref, np.int32), "cand": np.array(cand, np.int32).reshape(-1, 4),
            "err": np.array(err, np.float64)}


def select(res, epi_px):
    """The rows of match(..., a larger epi_px, ...) that a call at epi_px
    keeps: step 5 is the last decision and err does not depend on epi_px."""
    keep = res["err"] <= float(epi_px) * float(epi_px)
    return {k: v[keep] for k, v in res.items()}


def color(rgb, K, Rp, t, c, ref, mask):
    """mvs_wpatch_color_device -> color (n,3) float64, nviews (n,) int32."""
    V, H, W = rgb.shape[:3]
    c = np.asarray(c, np.float64).reshape(-1, 3)
    n = len(c)
    mask = np.asarray(mask).reshape(n, (V + 63) // 64)
    out, nv = np.zeros((n, 3)), np.zeros(n, np.int32)
    for p in range(n):
        views = set(er.mask_views(mask[p], V))
        if 0 <= int(ref[p]) < V:
            views.add(int(ref[p]))
        sums, m = [0, 0, 0], 0
        for v in sorted(views):
            x, y, depth = wr.project_ref(K[v], Rp[v], t[v], c[p])
            if not (depth > 0.0 and 0.0 <= x <= float(W - 1) and 0.0 <= y <= float(H - 1)):
                continue
            m += 1
            ix, iy = int(x), int(y)
            ax, ay = x - float(ix), y - float(iy)
            ix1, iy1 = min(ix + 1, W - 1), min(iy + 1, H - 1)
            for ch in range(3):
                g00, g01 = float(rgb[v, iy, ix, ch]), float(rgb[v, iy, ix1, ch])
                g10, g11 = float(rgb[v, iy1, ix, ch]), float(rgb[v, iy1, ix1, ch])
                top = g00 + ax * (g01 - g00)
                bot = g10 + ax * (g11 - g10)
                S = top + ay * (bot - top)
                sums[ch] += int(math.floor(S * 256.0 + 0.5))
        nv[p] = m
        if m:
            out[p] = [float(sums[ch]) / float(256 * m) for ch in range(3)]
    return out, nv


# ---------------------------------------------------------------------------
# the planted set: features that are projections of known sphere points
# ---------------------------------------------------------------------------
_PLANTED = {}


def ring_pairs(V):
    """(r, r+1), (r, r-1), (r, r+2) mod V, r-major."""
    return np.array([(r, (r + d) % V) for r in range(V) for d in (1, -1, 2)], np.int32)


def planted(pkg, rad=0.02, n_points=400, margin=6):
    """sphere_scene(V 24, 96 x 128) with rodrigues_roundtrip rotations, 400
    points on the sphere (default_rng(1) normals x rad) and, per view, the
    points facing the camera (n.(O - P) > 0.3 rad |O - P|) projected and rounded
    to integer pixels, `margin` px inside the image.  Computed once per process
    and shared; nothing of it is to be modified.  -> dict rgb, K, R, t_raw, t,
    Rp, W, H, rad, P (points), feats (list of (n_v,2) int32), ids (list of the
    points' indices, in feature order), feat, feat_off, pairs."""
    key = (rad, n_points, margin)
    if key not in _PLANTED:
        V, H, W = 24, 96, 128
        rgb, K, R, t_raw = pkg.synthetic.sphere_scene(V=V, H=H, W=W, rad=rad)[:4]
        Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
        t = np.asarray(t_raw, np.float64).reshape(-1, 3)
        rng = np.random.default_rng(1)
        nr = rng.normal(size=(n_points, 3))
        nr /= np.linalg.norm(nr, axis=1, keepdims=True)
        P = nr * rad
        feats, ids = [], []
        for v in range(V):
            O = np.array(er.centre_of([float(x) for x in Rp[v].reshape(9)], [float(x) for x in t[v]]))
            f, idv = [], []
            for i in range(n_points):
                e = O - P[i]
                if not nr[i] @ e * rad > 0.3 * rad * np.linalg.norm(e):
                    continue
                x, y, depth = wr.project_ref(K[v], Rp[v], t[v], P[i])
                qx, qy = int(round(x)), int(round(y))
                if depth > 0 and margin <= qx <= W - 1 - margin and margin <= qy <= H - 1 - margin:
                    f.append((qx, qy))
                    idv.append(i)
            feats.append(np.array(f, np.int32).reshape(-1, 2))
            ids.append(np.array(idv, np.int64))
        feat_off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
        _PLANTED[key] = {"rgb": rgb, "K": K, "R": R, "t_raw": t_raw, "t": t, "Rp": Rp, "W": W, "H": H, "rad": rad,
                         "P": P, "feats": feats, "ids": ids, "feat": np.concatenate(feats), "feat_off": feat_off,
                         "pairs": ring_pairs(V)}
    return _PLANTED[key]


def planted_match(pkg, epi_px=2.0):
    """match() of the planted set at epi_px 2 (select() gives the smaller
    ones), computed once per process."""
    s = planted(pkg)
    if "match" not in s:
        s["match"] = match(s["K"], s["Rp"], s["t"], s["feat"], s["feat_off"], s["pairs"], 2.0, 1e-4)
    return select(s["match"], epi_px)


def true_rows(s, res):
    """Rows of res whose two features come from one planted point."""
    k, a, b, v = res["cand"].T
    r = res["ref"]
    ida = np.array([s["ids"][int(rr)][int(aa)] for rr, aa in zip(r, a)], np.int64)
    idb = np.array([s["ids"][int(vv)][int(bb)] for vv, bb in zip(v, b)], np.int64)
    return ida == idb
