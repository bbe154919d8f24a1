"""Float64 numpy restatement of the plane-warped photo test (mvs_score_warped,
include/mvs_amd.h), one candidate at a time, in the ray-plane form: every
pixel of the reference window is sent along its ray to the patch plane and the
plane point is projected into each tested view.  A plain module (the tests
import it); there is no reference code for this test, the definition in the
header is the specification.

Cameras: Rp = the projection rotations (ctx.rproj() on the GPU tests,
pkg.rodrigues_roundtrip(R) on the CPU tests), t, and fx fy cx cy = K[0,0],
K[1,1], K[0,2], K[1,2] (no skew).  Gray: OpenCV's BGR2GRAY fixed-point formula
applied to the RGB bytes, as the library's gray stack.
"""
import math

import numpy as np


def gray_stack(rgb):
    """(V,H,W,3) uint8 RGB -> (V,H,W) uint8, the library's gray images."""
    p = np.asarray(rgb).astype(np.uint32)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def centres(Rp, t):
    """O_v = -Rp_v^T t_v."""
    return -np.einsum("vji,vj->vi", np.asarray(Rp, np.float64), np.asarray(t, np.float64).reshape(-1, 3))


def project_ref(K, Rp, t, c):
    """cv2.projectPoints without distortion in the library's operation order
    (Python floats: the same binary64 operations) -> x, y, depth."""
    X, Y, Z = (float(v) for v in c)
    Rp = [float(v) for v in np.asarray(Rp).reshape(9)]
    t = [float(v) for v in np.asarray(t).reshape(3)]
    x = Rp[0] * X + Rp[1] * Y + Rp[2] * Z + t[0]
    y = Rp[3] * X + Rp[4] * Y + Rp[5] * Z + t[1]
    z = Rp[6] * X + Rp[7] * Y + Rp[8] * Z + t[2]
    depth = z
    z = 1.0 / z if z != 0.0 else 1.0
    x *= z
    y *= z
    return x * float(K[0, 0]) + float(K[0, 2]), y * float(K[1, 1]) + float(K[1, 2]), depth


def window_pixels(x0, y0, wid):
    """Integer pixels of the window, row-major: (N, 2) float64 [x, y]."""
    dy, dx = np.mgrid[-wid:wid + 1, -wid:wid + 1]
    return np.stack([x0 + dx.ravel(), y0 + dy.ravel()], 1).astype(np.float64)


def plane_points(K, Rp, t, c, nrm, r, q):
    """Ray-plane form: the points X of the patch plane seen at pixels q of view r."""
    O = -Rp[r].T @ t[r]
    ray = np.stack([(q[:, 0] - K[r, 0, 2]) / K[r, 0, 0], (q[:, 1] - K[r, 1, 2]) / K[r, 1, 1],
                    np.ones(len(q))], 1)
    d = ray @ Rp[r]                      # rows Rp_r^T ray
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (nrm @ (c - O)) / (d @ nrm)
    return O + d * s[:, None]


def positions_rayplane(K, Rp, t, c, nrm, r, v, q):
    """Sample positions (N, 2) in view v and the samples' depths there."""
    X = plane_points(K, Rp, t, c, nrm, r, q)
    P = X @ Rp[v].T + t[v]
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = P[:, 0] / P[:, 2] * K[v, 0, 0] + K[v, 0, 2]
        sy = P[:, 1] / P[:, 2] * K[v, 1, 1] + K[v, 1, 2]
    return np.stack([sx, sy], 1), P[:, 2]


def homography(K, Rp, t, c, nrm, r, v):
    """H = K_v [(Rp_v O_r + t_v)(A^T nrm)^T + (nrm.(c - O_r)) Rp_v A], A = Rp_r^T K_r^-1
    (K without skew): H (q.x, q.y, 1) ~ the position of pixel q of view r in view v."""
    def kmat(k):
        return np.array([[k[0, 0], 0.0, k[0, 2]], [0.0, k[1, 1], k[1, 2]], [0.0, 0.0, 1.0]])
    O = -Rp[r].T @ t[r]
    A = Rp[r].T @ np.linalg.inv(kmat(K[r]))
    return kmat(K[v]) @ (np.outer(Rp[v] @ O + t[v], A.T @ nrm) + (nrm @ (c - O)) * (Rp[v] @ A))


def positions_homography(K, Rp, t, c, nrm, r, v, q):
    h = np.concatenate([q, np.ones((len(q), 1))], 1) @ homography(K, Rp, t, c, nrm, r, v).T
    return h[:, :2] / h[:, 2:3]


def bilinear(g, sx, sy):
    """Difference-form bilinear samples of image g (H, W) float64 at in-image
    positions: exact on a constant neighbourhood."""
    H, W = g.shape
    ix = np.floor(sx).astype(np.int64)
    iy = np.floor(sy).astype(np.int64)
    ax, ay = sx - ix, sy - iy
    ix1 = np.minimum(ix + 1, W - 1)
    iy1 = np.minimum(iy + 1, H - 1)
    g00, g01, g10, g11 = g[iy, ix], g[iy, ix1], g[iy1, ix], g[iy1, ix1]
    top = g00 + ax * (g01 - g00)
    bot = g10 + ax * (g11 - g10)
    return top + ay * (bot - top)


def warped_reference(gray, K, Rp, t, c, nrm, ref, wid=5, min_cos=0.0):
    """One candidate.  Returns a dict:
      xy       projection of c into view ref (x, y)
      valid    the candidate passed step 2 of the definition
      ncc      (V,) float64, nan for ref, culled and failed views
      sigma_b  (V,) population std of the warped window (nan where no window was sampled)
      border   (V,) margin of the samples to the image border in px (min over the
               samples of min(sx, W-1-sx, sy, H-1-sy); -inf when a sample has no
               positive depth); nan for views that are not tested
      cosm     (V,) margin of the min_cos test, nrm.(O_v - c) - min_cos |O_v - c|
               (every view, ref included)
    The sums are taken on g - 128 (NCC is shift-invariant)."""
    gray = np.asarray(gray)
    V, H, W = gray.shape
    K = np.asarray(K, np.float64).reshape(V, 3, 3)
    Rp = np.asarray(Rp, np.float64).reshape(V, 3, 3)
    t = np.asarray(t, np.float64).reshape(V, 3)
    c = np.asarray(c, np.float64).reshape(3)
    nrm = np.asarray(nrm, np.float64).reshape(3)
    r = int(ref)
    S = 2 * wid + 1
    N = S * S
    out = {"ncc": np.full(V, np.nan), "sigma_b": np.full(V, np.nan), "border": np.full(V, np.nan),
           "valid": False}
    O = centres(Rp, t)
    e = O - c
    out["cosm"] = e @ nrm - min_cos * np.sqrt((e * e).sum(1))
    x, y, depth = project_ref(K[r], Rp[r], t[r], c)
    out["xy"] = (x, y)
    if not (depth > 0 and x >= 0 and y >= 0 and abs(x) < 1e9 and abs(y) < 1e9):
        return out
    x0, y0 = int(x), int(y)
    if not (x0 - wid >= 0 and x0 + wid <= W - 1 and y0 - wid >= 0 and y0 + wid <= H - 1):
        return out
    if not out["cosm"][r] > 0:
        return out
    a = gray[r, y0 - wid:y0 + wid + 1, x0 - wid:x0 + wid + 1].astype(np.float64).ravel() - 128.0
    Sa = a.sum()
    Da = N * (a * a).sum() - Sa * Sa
    if not Da > 0:
        return out
    out["valid"] = True
    q = window_pixels(x0, y0, wid)
    for v in range(V):
        if v == r or not out["cosm"][v] > 0:
            continue
        pos, z = positions_rayplane(K, Rp, t, c, nrm, r, v, q)
        sx, sy = pos[:, 0], pos[:, 1]
        if not np.all(z > 0) or not np.all(np.isfinite(pos)):
            out["border"][v] = -np.inf
            continue
        out["border"][v] = min(sx.min(), (W - 1 - sx).min(), sy.min(), (H - 1 - sy).min())
        if out["border"][v] < 0:
            continue
        b = bilinear(gray[v].astype(np.float64) - 128.0, sx, sy)
        Sb = b.sum()
        Db = N * (b * b).sum() - Sb * Sb
        out["sigma_b"][v] = math.sqrt(max(Db, 0.0)) / N
        if not Db > 0:
            continue
        out["ncc"][v] = (N * (a * b).sum() - Sa * Sb) / math.sqrt(Da * Db) * N / (N - 1)
    return out


def warped_batch(gray, K, Rp, t, c, nrm, ref, wid=5, min_cos=0.0):
    """warped_reference over a batch -> dict of stacked arrays."""
    rs = [warped_reference(gray, K, Rp, t, c[i], nrm[i], ref[i], wid, min_cos) for i in range(len(ref))]
    return {k: np.array([r[k] for r in rs]) for k in ("xy", "valid", "ncc", "sigma_b", "border", "cosm")}


def sphere_patches(K, R, t, n, rad, rng, shifts=(0.0,), H=96, W=128, min_facing=0.5, margin=8):
    """n patches of the sphere |X| = rad facing their reference camera: a random
    view, a random pixel (at least margin px from the border) whose ray
    (par-file rotation R) hits the sphere, the first hit, kept when the outward normal and the direction to the camera
    make a cosine above min_facing.  Patch k is moved by shifts[k % len(shifts)]
    along its normal.  -> c (n,3), nrm (n,3) true normals, ref (n,), shift (n,)."""
    V = len(K)
    c, nr, ref, sh = [], [], [], []
    while len(c) < n:
        v = int(rng.integers(0, V))
        x, y = rng.uniform(margin, W - margin), rng.uniform(margin, H - margin)
        d = R[v].T @ (np.linalg.inv(K[v]) @ np.array([x, y, 1.0]))
        d /= np.linalg.norm(d)
        O = -R[v].T @ t[v]
        b = d @ O
        disc = b * b - (O @ O - rad * rad)
        if disc <= 0:
            continue
        X = O + (-b - math.sqrt(disc)) * d
        nn = X / np.linalg.norm(X)
        to_cam = (O - X) / np.linalg.norm(O - X)
        if nn @ to_cam <= min_facing:
            continue
        s = shifts[len(c) % len(shifts)]
        c.append(X + s * nn)
        nr.append(nn)
        ref.append(v)
        sh.append(s)
    return np.array(c), np.array(nr), np.array(ref, np.int32), np.array(sh)
