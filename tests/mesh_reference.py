"""Float64 restatement of the volumetric fusion and the surface extraction of
the warped pipeline (mvs_wtsdf_integrate_device, mvs_wmesh_extract_device,
include/mvs_amd.h) and of the chain MvsContext.mesh_depth.  The geometry is
written in Python floats, product by product and sum by sum in the header's
order (left to right, unfused), so every output can be compared exactly.
integrate_fast is integrate with the lattice points taken together through
numpy's elementwise binary64 operations in the same order: the same bits, for
lattices too large for the Python loop; test_wmesh_host.py holds it against
integrate.  A plain module (the tests import it); this text is normative.
"""
import itertools
import math

import numpy as np

import depth_reference as dr
import expand_reference as er

PERMS = tuple(itertools.permutations(range(3)))


def tet_corners(perm):
    """The four cube corners (bit m of a corner = its offset along axis m) of the
    Kuhn tetrahedron of `perm`: c0 = 0, c1 = c0 + e_perm[0], c2 = c1 + e_perm[1], c3 = 7."""
    c1 = 1 << perm[0]
    return (0, c1, c1 | (1 << perm[1]), 7)


def base_triangles(case):
    """The triangles of a 4-bit inside mask before winding, as pairs (p, q), p < q,
    of tetrahedron corners (the lattice edge between them)."""
    ins = [k for k in range(4) if case >> k & 1]
    out = [k for k in range(4) if not case >> k & 1]
    e = lambda p, q: (min(p, q), max(p, q))
    if len(ins) == 1:
        return [[e(ins[0], o) for o in out]]
    if len(ins) == 3:
        return [[e(i, out[0]) for i in ins]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        return [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
    return []


def _corner_xyz(corner):
    return [corner >> m & 1 for m in range(3)]


def _derive_flips():
    """flip[perm index] bit `case`: the base triangles of the case are listed
    against the winding rule and have p1 and p2 swapped.  Derived with corner
    values -1 (inside) and +1, vertices at the edge midpoints, in integers
    (coordinates doubled): every triangle of a case gets the same answer."""
    flips = []
    for perm in PERMS:
        cc = [_corner_xyz(c) for c in tet_corners(perm)]
        word = 0
        for case in range(1, 15):
            ins = [k for k in range(4) if case >> k & 1]
            out = [k for k in range(4) if not case >> k & 1]
            # (mean of the outside corners - mean of the inside corners) times len(ins) len(out)
            g = [len(ins) * sum(cc[k][m] for k in out) - len(out) * sum(cc[k][m] for k in ins) for m in range(3)]
            signs = set()
            for tri in base_triangles(case):
                p = [[cc[a][m] + cc[b][m] for m in range(3)] for a, b in tri]
                u = [p[1][m] - p[0][m] for m in range(3)]
                w = [p[2][m] - p[0][m] for m in range(3)]
                n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
                s = n[0] * g[0] + n[1] * g[1] + n[2] * g[2]
                assert s != 0
                signs.add(s < 0)
            assert len(signs) == 1
            if signs.pop():
                word |= 1 << case
        flips.append(word)
    return tuple(flips)


FLIPS = _derive_flips()


def lattice_point(origin, voxel, i, j, k):
    """P(i, j, k) = origin + (i, j, k) voxel: one product and one sum per coordinate."""
    return [origin[0] + float(i) * voxel, origin[1] + float(j) * voxel, origin[2] + float(k) * voxel]


def integrate(K, Rp, t, W, H, rgb, zmap, v0, nv, dims, origin, voxel, trunc, min_weight):
    """mvs_wtsdf_integrate_device in Python floats -> tsdf (nz+1, ny+1, nx+1)
    float64, weight int32, rgb (.., 3) uint8, cnt uint8."""
    nx, ny, nz = dims
    zmap = np.asarray(zmap, np.float64).reshape(nv, H, W)
    origin = [float(x) for x in origin]
    voxel, trunc = float(voxel), float(trunc)
    cams = [er._cam(K, Rp, t, v0 + k) for k in range(nv)]
    shape = (nz + 1, ny + 1, nx + 1)
    tsdf = np.full(shape, np.nan)
    weight = np.zeros(shape, np.int32)
    col = np.zeros(shape + (3,), np.uint8)
    cnt = np.zeros(shape, np.uint8)
    for k, j, i in itertools.product(range(nz + 1), range(ny + 1), range(nx + 1)):
        X, Y, Z = lattice_point(origin, voxel, i, j, k)
        D, Wt, c, s = 0.0, 0, 0, [0, 0, 0]
        for ui in range(nv):
            R9, t3, fx, fy, cx, cy = cams[ui]
            x = R9[0] * X + R9[1] * Y + R9[2] * Z + t3[0]
            y = R9[3] * X + R9[4] * Y + R9[5] * Z + t3[1]
            z = R9[6] * X + R9[7] * Y + R9[8] * Z + t3[2]
            r = 1.0 / z if z != 0.0 else 1.0
            x = x * r * fx + cx
            y = y * r * fy + cy
            xr, yr = x + 0.5, y + 0.5
            if not (z > 0 and x >= 0 and y >= 0 and xr < W and yr < H):
                continue
            xi, yi = int(xr), int(yr)
            zu = float(zmap[ui, yi, xi])
            if not (math.isfinite(zu) and zu > 0):
                continue
            sdf = zu - z
            if sdf < -trunc:
                continue
            q = sdf / trunc
            D += q if q < 1.0 else 1.0
            Wt += 1
            if abs(sdf) <= trunc:
                px = rgb[v0 + ui][yi, xi]
                for m in range(3):
                    s[m] += int(px[m])
                c += 1
        weight[k, j, i] = Wt
        if Wt >= min_weight:
            tsdf[k, j, i] = D / float(Wt)
        if c:
            col[k, j, i] = [(2 * s[m] + c) // (2 * c) for m in range(3)]
        cnt[k, j, i] = min(c, 255)
    return tsdf, weight, col, cnt


def integrate_fast(K, Rp, t, W, H, rgb, zmap, v0, nv, dims, origin, voxel, trunc, min_weight):
    """integrate with the lattice points taken together: the same binary64
    operations in the same order through numpy's elementwise arithmetic."""
    nx, ny, nz = dims
    zmap = np.asarray(zmap, np.float64).reshape(nv, H, W)
    origin = [float(x) for x in origin]
    voxel, trunc = float(voxel), float(trunc)
    shape = (nz + 1, ny + 1, nx + 1)
    kk, jj, ii = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    X = origin[0] + ii.astype(np.float64) * voxel
    Y = origin[1] + jj.astype(np.float64) * voxel
    Z = origin[2] + kk.astype(np.float64) * voxel
    D = np.zeros(shape)
    Wt = np.zeros(shape, np.int64)
    c = np.zeros(shape, np.int64)
    s = np.zeros(shape + (3,), np.int64)
    with np.errstate(all="ignore"):
        for ui in range(nv):
            R9, t3, fx, fy, cx, cy = er._cam(K, Rp, t, v0 + ui)
            x = R9[0] * X + R9[1] * Y + R9[2] * Z + t3[0]
            y = R9[3] * X + R9[4] * Y + R9[5] * Z + t3[1]
            z = R9[6] * X + R9[7] * Y + R9[8] * Z + t3[2]
            r = np.where(z != 0.0, 1.0 / z, 1.0)
            x = x * r * fx + cx
            y = y * r * fy + cy
            xr, yr = x + 0.5, y + 0.5
            ok = (z > 0) & (x >= 0) & (y >= 0) & (xr < W) & (yr < H)
            xi = np.where(ok, xr, 0.0).astype(np.int64)
            yi = np.where(ok, yr, 0.0).astype(np.int64)
            zu = zmap[ui, yi, xi]
            ok &= np.isfinite(zu) & (zu > 0)
            sdf = zu - z
            ok &= ~(sdf < -trunc)
            q = sdf / trunc
            D = np.where(ok, D + np.where(q < 1.0, q, 1.0), D)
            Wt += ok
            near = ok & (np.abs(sdf) <= trunc)
            s += np.where(near[..., None], rgb[v0 + ui][yi, xi].astype(np.int64), 0)
            c += near
        tsdf = np.where(Wt >= min_weight, D / Wt.astype(np.float64), np.nan)
    c3 = c[..., None]
    col = np.where(c3 > 0, (2 * s + c3) // np.maximum(2 * c3, 1), 0).astype(np.uint8)
    return tsdf, Wt.astype(np.int32), col, np.minimum(c, 255).astype(np.uint8)


def extract(tsdf, rgb, cnt, origin, voxel):
    """mvs_wmesh_extract_device in Python floats: marching tetrahedra over the
    lattice tsdf (nz+1, ny+1, nx+1) -> vertices (n, 3) float64, colors (n, 3)
    uint8, faces (m, 3) int32.  Vertices are ordered by (owner point's linear
    index, edge type delta.x + 2 delta.y + 4 delta.z - 1), triangles by (cube's
    linear index, tetrahedron, triangle)."""
    tsdf = np.asarray(tsdf, np.float64)
    nz, ny, nx = (n - 1 for n in tsdf.shape)
    rgb = np.asarray(rgb, np.uint8).reshape(tsdf.shape + (3,))
    cnt = np.asarray(cnt, np.uint8).reshape(tsdf.shape)
    origin = [float(x) for x in origin]
    voxel = float(voxel)
    tets = [tet_corners(p) for p in PERMS]
    tris = []          # triples of edge keys (owner linear index, edge type)
    for k, j, i in itertools.product(range(nz), range(ny), range(nx)):
        f = [float(tsdf[k + (c >> 2 & 1), j + (c >> 1 & 1), i + (c & 1)]) for c in range(8)]
        lin = [((k + (c >> 2 & 1)) * (ny + 1) + j + (c >> 1 & 1)) * (nx + 1) + i + (c & 1) for c in range(8)]
        for tp, cc in enumerate(tets):
            g = [f[c] for c in cc]
            if not all(math.isfinite(x) for x in g):
                continue
            case = sum(1 << m for m in range(4) if g[m] < 0)
            for tri in base_triangles(case):
                keys = [(lin[cc[p]], (cc[q] ^ cc[p]) - 1) for p, q in tri]
                if FLIPS[tp] >> case & 1:
                    keys[1], keys[2] = keys[2], keys[1]
                tris.append(keys)
    used = sorted({key for tri in tris for key in tri})
    index = {key: n for n, key in enumerate(used)}
    vert = np.zeros((len(used), 3))
    col = np.zeros((len(used), 3), np.uint8)
    for n, (lin, e) in enumerate(used):
        i, r = lin % (nx + 1), lin // (nx + 1)
        j, k = r % (ny + 1), r // (ny + 1)
        d = _corner_xyz(e + 1)
        a, b = (k, j, i), (k + d[2], j + d[1], i + d[0])
        fa, fb = float(tsdf[a]), float(tsdf[b])
        tt = fa / (fa - fb)
        Pa = lattice_point(origin, voxel, i, j, k)
        Pb = lattice_point(origin, voxel, i + d[0], j + d[1], k + d[2])
        vert[n] = [Pa[m] + tt * (Pb[m] - Pa[m]) for m in range(3)]
        first, other = (a, b) if tt < 0.5 else (b, a)
        col[n] = rgb[first] if cnt[first] else rgb[other]
    faces = np.array([[index[key] for key in tri] for tri in tris], np.int32).reshape(-1, 3)
    return vert, col, faces


def percentile(values, q):
    """The q-th percentile of a sequence by linear interpolation between the
    order statistics, in Python floats: position (n - 1) q / 100, weight t of the
    upper neighbour, a + (b - a) t below t = 0.5 and b - (b - a)(1 - t) from there
    (numpy's default rule, restated so that the lattice is worked out twice)."""
    a = sorted(float(x) for x in values)
    pos = (len(a) - 1) * (q / 100.0)
    lo = int(math.floor(pos))
    hi = min(lo + 1, len(a) - 1)
    t = pos - lo
    d = a[hi] - a[lo]
    return a[hi] - d * (1.0 - t) if t >= 0.5 else a[lo] + d * t


def mesh_grid(points, bounds, resolution, trunc_voxels):
    """The lattice of MvsContext.mesh_depth, in Python floats -> origin (3,)
    float64, voxel, dims (nx, ny, nz), trunc.  bounds = (lo, hi) is taken as
    given: voxel = its longest side / resolution.  bounds None: the per-axis 0.5
    to 99.5 percentile box of `points` gives the voxel the same way and is then
    grown by 2 trunc on every side.  dims = ceil(side / voxel), at least 1, per axis."""
    if bounds is None:
        pts = np.zeros((0, 3)) if points is None else np.asarray(points, np.float64).reshape(-1, 3)
        if len(pts) == 0:
            raise RuntimeError("mesh_depth: no points to take the bounds from")
        lo = [percentile(pts[:, m], 0.5) for m in range(3)]
        hi = [percentile(pts[:, m], 99.5) for m in range(3)]
    else:
        lo, hi = ([float(x) for x in np.asarray(b).reshape(3)] for b in bounds)
    voxel = max(hi[m] - lo[m] for m in range(3)) / float(resolution)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise RuntimeError("mesh_depth: the bounds must be finite with a positive longest side")
    trunc = float(trunc_voxels) * voxel
    if bounds is None:
        grow = 2.0 * trunc
        lo, hi = [x - grow for x in lo], [x + grow for x in hi]
    dims = tuple(max(1, int(math.ceil((hi[m] - lo[m]) / voxel))) for m in range(3))
    return np.array(lo, np.float64), voxel, dims, trunc


def mesh_chain(K, Rp, t, W, H, rgb, maps, views=None, bounds=None, resolution=256, trunc_voxels=3.0, min_weight=1,
               rel_tol=0.01, min_consistent=2, max_violations=0, integrate_fn=integrate_fast):
    """MvsContext.mesh_depth on the CPU -> dict vertices, colors, faces, tsdf,
    weight, origin, voxel, dims."""
    V = len(K)
    v0, nv = (0, V) if views is None else (int(views[0]), int(views[1]))
    z = np.asarray(maps["z"], np.float64).reshape(nv, H, W)
    cons, viol = dr.consist_fast(K, Rp, t, W, H, z, v0, nv, rel_tol)
    keep = np.isfinite(z) & (cons >= min_consistent) & (viol <= max_violations)
    z = np.where(keep, z, np.inf)
    origin, voxel, dims, trunc = mesh_grid(maps.get("points"), bounds, resolution, trunc_voxels)
    tsdf, weight, col, cnt = integrate_fn(K, Rp, t, W, H, rgb, z, v0, nv, dims, origin, voxel, trunc, min_weight)
    vert, vcol, faces = extract(tsdf, col, cnt, origin, voxel)
    return {"vertices": vert, "colors": vcol, "faces": faces, "tsdf": tsdf, "weight": weight, "origin": origin,
            "voxel": voxel, "dims": np.array(dims, np.int32)}


# ---------------------------------------------------------------------------
# what the tests measure on a mesh
# ---------------------------------------------------------------------------
def edge_uses(faces):
    """{(a, b): number of triangles that run the directed edge a -> b}."""
    uses = {}
    for tri in np.asarray(faces).reshape(-1, 3).tolist():
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            uses[(a, b)] = uses.get((a, b), 0) + 1
    return uses


def manifold_report(faces):
    """-> (worst number of triangles on one undirected edge, worst number of
    uses of one directed edge, number of boundary edges, number of undirected edges)."""
    uses = edge_uses(faces)
    und = {}
    for (a, b), n in uses.items():
        und[(min(a, b), max(a, b))] = und.get((min(a, b), max(a, b)), 0) + n
    boundary = sum(1 for n in und.values() if n == 1)
    return max(und.values(), default=0), max(uses.values(), default=0), boundary, len(und)


def areas2(vert, faces):
    """Twice the area of every triangle."""
    p = np.asarray(vert)[np.asarray(faces).reshape(-1, 3)]
    return np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def enclosed_volume(vert, faces):
    """The signed volume inside a closed mesh whose triangles face outward."""
    p = np.asarray(vert)[np.asarray(faces).reshape(-1, 3)]
    return float(np.einsum("ni,ni->n", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def look_at_cameras(centres, H, W):
    """Cameras at `centres` looking at the origin, K = dinoRing's scaled to W x H
    (synthetic.ring_cameras' convention; a camera on the z axis takes up = x)."""
    f = 3310.4 * W / 640.0
    V = len(centres)
    K = np.tile(np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]), (V, 1, 1))
    R, t = np.empty((V, 3, 3)), np.empty((V, 3))
    for v, C in enumerate(np.asarray(centres, np.float64)):
        z = -C / np.linalg.norm(C)
        up = np.array([0, 0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0, 0])
        x = np.cross(up, z)
        x /= np.linalg.norm(x)
        R[v] = np.stack([x, np.cross(z, x), z])
        t[v] = -R[v] @ C
    return K, R, t


def sphere14(H=48, W=64, dist=0.33):
    """The 14 centres of the closed sphere scene: 6 on the axes and 8 on the
    cube diagonals, at `dist` from the origin -> K, R, t."""
    axes = [np.eye(3)[m] * s for m in range(3) for s in (1.0, -1.0)]
    corners = [np.array(c, np.float64) / math.sqrt(3.0) for c in itertools.product((1.0, -1.0), repeat=3)]
    return look_at_cameras(np.array(axes + corners) * dist, H, W)
