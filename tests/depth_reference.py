"""Float64 restatement of the depth maps of a warped patch set
(mvs_wdepth_splat_device, mvs_wdepth_consist_device, mvs_wdepth_points_device,
include/mvs_amd.h) and of the fusion rule of MvsContext.depth_maps, built on
expand_reference's projection helpers and filter_reference.views_of / depth_in,
which stay as they are.  The geometry is written in Python floats, product by
product and sum by sum in the header's order (left to right, unfused), so every
output can be compared exactly.  consist_fast is the same count with the pixels
of a view taken together through numpy's elementwise binary64 operations, in
the same order: the same bits, for maps too large for the Python loop;
test_wdepth_host.py holds it against consist.  A plain module (the tests import
it); the definition in the header is the specification.
"""
import math

import numpy as np

import expand_reference as er
import filter_reference as fr
import warped_reference as wr


def pixel_ray(R9, fx, fy, cx, cy, qx, qy):
    """d = Rp^T ((qx - cx) / fx, (qy - cy) / fy, 1) of the integer pixel (qx, qy)."""
    u = (float(qx) - cx) / fx
    w = (float(qy) - cy) / fy
    return [R9[k] * u + R9[3 + k] * w + R9[6 + k] for k in range(3)]


def nearest(a):
    """int(a + 0.5) of a coordinate >= 0; None when it is not finite."""
    a = a + 0.5
    return int(a) if math.isfinite(a) else None


def splat(K, Rp, t, W, H, c, nrm, ref, mask, radius, slope, v0=0, nv=None):
    """mvs_wdepth_splat_device -> zmap (nv, H, W) float64 (+inf = empty) and idmap
    int32 (-1 = empty).  Patches in ascending order: a tie keeps the lower index."""
    V = len(K)
    nv = V - v0 if nv is None else nv
    c = np.asarray(c, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    mask = np.asarray(mask).reshape(len(c), (V + 63) // 64)
    slope = float(slope)
    zmap = np.full((nv, H, W), np.inf)
    idmap = np.full((nv, H, W), -1, np.int32)
    cams = {}
    for p in range(len(c)):
        views = fr.views_of(ref[p], mask[p], V)
        if views is None:
            continue
        cp = [float(x) for x in c[p]]
        n = [float(x) for x in nrm[p]]
        for v in views:
            if not v0 <= v < v0 + nv:
                continue
            x, y, depth = wr.project_ref(K[v], Rp[v], t[v], cp)
            if not (depth > 0 and 0 <= x < W and 0 <= y < H):
                continue
            z = fr.depth_in(Rp, t, v, cp)
            if v not in cams:
                cams[v] = er._cam(K, Rp, t, v)
            R9, t3, fx, fy, cx, cy = cams[v]
            O = er.centre_of(R9, t3)
            e = [O[k] - cp[k] for k in range(3)]
            if not n[0] * e[0] + n[1] * e[1] + n[2] * e[2] > 0:
                continue
            f = [cp[k] - O[k] for k in range(3)]
            h = n[0] * f[0] + n[1] * f[1] + n[2] * f[2]
            x0, y0 = int(x + 0.5), int(y + 0.5)
            for qy in range(max(y0 - radius, 0), min(y0 + radius, H - 1) + 1):
                for qx in range(max(x0 - radius, 0), min(x0 + radius, W - 1) + 1):
                    d = pixel_ray(R9, fx, fy, cx, cy, qx, qy)
                    den = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
                    if den == 0.0 or den != den:
                        continue
                    s = h / den
                    if not (s > 0 and math.isfinite(s)):
                        continue
                    m = max(abs(qx - x0), abs(qy - y0))
                    if not abs(s - z) <= slope * float(m + 1) * z / ((fx + fy) / 2):
                        continue
                    if s < zmap[v - v0, qy, qx]:                 # ascending p: a tie keeps the lower index
                        zmap[v - v0, qy, qx], idmap[v - v0, qy, qx] = s, p
    return zmap, idmap


def world_point(cam, qx, qy, z):
    """X = O + z d, each component one product and one sum."""
    R9, t3, fx, fy, cx, cy = cam
    O = er.centre_of(R9, t3)
    d = pixel_ray(R9, fx, fy, cx, cy, qx, qy)
    return [O[k] + z * d[k] for k in range(3)]


def consist(K, Rp, t, W, H, zmap, v0, nv, rel_tol):
    """mvs_wdepth_consist_device in Python floats -> cons, viol (nv, H, W) uint8."""
    zmap = np.asarray(zmap, np.float64).reshape(nv, H, W)
    rel_tol = float(rel_tol)
    cons = np.zeros((nv, H, W), np.uint8)
    viol = np.zeros((nv, H, W), np.uint8)
    cams = [er._cam(K, Rp, t, v0 + k) for k in range(nv)]
    for vi in range(nv):
        for qy, qx in np.argwhere(np.isfinite(zmap[vi]) & (zmap[vi] > 0)):
            X = world_point(cams[vi], int(qx), int(qy), float(zmap[vi, qy, qx]))
            for ui in range(nv):
                if ui == vi:
                    continue
                x, y, depth = wr.project_ref(K[v0 + ui], Rp[v0 + ui], t[v0 + ui], X)
                if not (depth > 0 and x >= 0 and y >= 0):
                    continue
                xi, yi = nearest(x), nearest(y)
                if xi is None or yi is None or not (xi < W and yi < H):
                    continue
                zu = float(zmap[ui, yi, xi])
                if not math.isfinite(zu):
                    continue
                tol = rel_tol * depth
                if abs(zu - depth) <= tol:
                    cons[vi, qy, qx] += 1
                elif zu - depth > tol:
                    viol[vi, qy, qx] += 1
    return cons, viol


def consist_fast(K, Rp, t, W, H, zmap, v0, nv, rel_tol):
    """consist with a view's pixels taken together: the same binary64 operations
    in the same order through numpy's elementwise arithmetic."""
    zmap = np.asarray(zmap, np.float64).reshape(nv, H, W)
    rel_tol = float(rel_tol)
    cons = np.zeros((nv, H, W), np.uint8)
    viol = np.zeros((nv, H, W), np.uint8)
    cams = [er._cam(K, Rp, t, v0 + k) for k in range(nv)]
    with np.errstate(all="ignore"):
        for vi in range(nv):
            qy, qx = np.nonzero(np.isfinite(zmap[vi]) & (zmap[vi] > 0))
            if len(qy) == 0:
                continue
            R9, t3, fx, fy, cx, cy = cams[vi]
            O = er.centre_of(R9, t3)
            z = zmap[vi, qy, qx]
            u = (qx.astype(np.float64) - cx) / fx
            w = (qy.astype(np.float64) - cy) / fy
            X = [O[k] + z * (R9[k] * u + R9[3 + k] * w + R9[6 + k]) for k in range(3)]
            for ui in range(nv):
                if ui == vi:
                    continue
                A9, a3, gx, gy, ax, ay = cams[ui]
                x = A9[0] * X[0] + A9[1] * X[1] + A9[2] * X[2] + a3[0]
                y = A9[3] * X[0] + A9[4] * X[1] + A9[5] * X[2] + a3[1]
                depth = A9[6] * X[0] + A9[7] * X[1] + A9[8] * X[2] + a3[2]
                r = np.where(depth != 0.0, 1.0 / depth, 1.0)
                x = x * r * gx + ax
                y = y * r * gy + ay
                xr, yr = x + 0.5, y + 0.5
                ok = (depth > 0) & (x >= 0) & (y >= 0) & (xr < W) & (yr < H)
                xi = np.where(ok, xr, 0.0).astype(np.int64)
                yi = np.where(ok, yr, 0.0).astype(np.int64)
                zu = zmap[ui, yi, xi]
                ok &= np.isfinite(zu)
                tol = rel_tol * depth
                agree = ok & (np.abs(zu - depth) <= tol)
                through = ok & ~agree & (zu - depth > tol)
                cons[vi, qy, qx] += agree.astype(np.uint8)
                viol[vi, qy, qx] += through.astype(np.uint8)
    return cons, viol


def points(K, Rp, t, W, H, rgb, zmap, v0, nv, pix):
    """mvs_wdepth_points_device -> xyz (m, 3) float64 and rgb (m, 3) uint8; nan
    and 0 where the pixel's depth is not finite and > 0."""
    zmap = np.asarray(zmap, np.float64).reshape(nv, H, W)
    pix = np.asarray(pix, np.int32).reshape(-1, 3)
    xyz = np.full((len(pix), 3), np.nan)
    col = np.zeros((len(pix), 3), np.uint8)
    for k, (v, qx, qy) in enumerate(pix.tolist()):
        assert v0 <= v < v0 + nv and 0 <= qx < W and 0 <= qy < H
        z = float(zmap[v - v0, qy, qx])
        if z > 0 and math.isfinite(z):
            xyz[k] = world_point(er._cam(K, Rp, t, v), qx, qy, z)
            col[k] = rgb[v][qy, qx]
    return xyz, col


def fuse(idmap, cons, viol, ref, v0, min_consistent=2, max_violations=0):
    """The fusion rule: pixel (v, q) is emitted when id >= 0, ref[id] = v, cons >=
    min_consistent and viol <= max_violations -> pix (m, 3) int32 rows (v, q.x,
    q.y) in the maps' order (view, row, column)."""
    ref = np.asarray(ref, np.int32).reshape(-1)
    idmap = np.asarray(idmap)
    nv = idmap.shape[0]
    owner = np.where(idmap >= 0, ref[np.maximum(idmap, 0)] if len(ref) else -1, -1)
    here = (v0 + np.arange(nv))[:, None, None]
    sel = (idmap >= 0) & (owner == here) & (cons >= min_consistent) & (viol <= max_violations)
    vi, qy, qx = np.nonzero(sel)
    return np.stack([vi + v0, qx, qy], 1).astype(np.int32).reshape(-1, 3)


def depth_chain(K, Rp, t, W, H, rgb, patches, radius=1, slope=4.0, views=None, rel_tol=0.01, min_consistent=2,
                max_violations=0, consist_fn=consist_fast):
    """MvsContext.depth_maps on the CPU -> dict z, id, cons, viol, normal and the
    fused cloud points, normals, colors, pix.  views: None or (v0, nv)."""
    V = len(K)
    v0, nv = (0, V) if views is None else (int(views[0]), int(views[1]))
    c, nrm, ref, mask = patches["c"], patches["nrm"], patches["ref"], patches["mask"]
    z, idm = splat(K, Rp, t, W, H, c, nrm, ref, mask, radius, slope, v0, nv)
    cons, viol = consist_fn(K, Rp, t, W, H, z, v0, nv, rel_tol)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    normal = np.full((nv, H, W, 3), np.nan)
    normal[idm >= 0] = nrm[idm[idm >= 0]]
    pix = fuse(idm, cons, viol, ref, v0, min_consistent, max_violations)
    xyz, col = points(K, Rp, t, W, H, rgb, z, v0, nv, pix)
    return {"z": z, "id": idm, "cons": cons, "viol": viol, "normal": normal, "points": xyz,
            "normals": normal[pix[:, 0] - v0, pix[:, 2], pix[:, 1]].reshape(-1, 3), "colors": col, "pix": pix}


def sphere_depth(K, Rp, t, W, H, v, rad):
    """Analytic depth of the sphere |X| = rad in every integer pixel of view v
    (H, W), nan where the pixel's ray misses it: the first root of |O + s d| =
    rad along d = pixel_ray, whose camera z is 1."""
    R9, t3, fx, fy, cx, cy = er._cam(K, Rp, t, v)
    O = np.array(er.centre_of(R9, t3))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    u, w = (xs - cx) / fx, (ys - cy) / fy
    d = np.stack([R9[k] * u + R9[3 + k] * w + R9[6 + k] for k in range(3)], -1)
    a = (d * d).sum(-1)
    b = d @ O
    disc = b * b - a * (O @ O - rad * rad)
    with np.errstate(invalid="ignore"):
        s = (-b - np.sqrt(np.where(disc > 0, disc, np.nan))) / a
    return np.where(s > 0, s, np.nan)
