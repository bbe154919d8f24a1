"""The mesh of the depth maps: signed-distance fusion and marching tetrahedra (csrc/mvs_mesh_warp.hip)."""
import math

import numpy as np

from ._abi import _c, _dp, _i32p, _i64p, _p, _u8p, check, load
from ._context import _need


def mesh_grid(points, bounds, resolution, trunc_voxels):
    """The lattice of MvsContext.mesh_depth -> origin (3,) float64, voxel, dims
    (nx, ny, nz), trunc.  bounds = (lo, hi) is taken as given: voxel = its longest
    side / resolution.  bounds None: the per-axis 0.5 to 99.5 percentile box of
    `points` gives the voxel the same way and is then grown by 2 trunc on every
    side.  dims = ceil(side / voxel), at least 1, per axis."""
    if bounds is None:
        pts = np.zeros((0, 3)) if points is None else np.asarray(points, np.float64).reshape(-1, 3)
        if len(pts) == 0:
            raise RuntimeError("mesh_depth: no points to take the bounds from")
        lo, hi = np.percentile(pts, 0.5, axis=0), np.percentile(pts, 99.5, axis=0)
    else:
        lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
    if int(resolution) < 1:
        raise RuntimeError("mesh_depth: resolution must be >= 1")
    voxel = float((hi - lo).max()) / float(resolution)
    if not (voxel > 0 and math.isfinite(voxel) and float(trunc_voxels) > 0):
        raise RuntimeError("mesh_depth: the bounds must be finite with a positive longest side, trunc_voxels > 0")
    trunc = float(trunc_voxels) * voxel
    if bounds is None:
        lo, hi = lo - 2.0 * trunc, hi + 2.0 * trunc
    dims = tuple(max(1, int(math.ceil(float(s) / voxel))) for s in hi - lo)
    return np.ascontiguousarray(lo, np.float64), voxel, dims, trunc


class _Wmesh:
    @staticmethod
    def _lattice(dims, origin):
        """(nx, ny, nz) as ints, the lattice's shape (nz+1, ny+1, nx+1) and origin as 3 contiguous doubles."""
        nx, ny, nz = (int(d) for d in dims)
        origin = _c(origin, np.float64).reshape(-1)
        if len(origin) != 3:
            raise RuntimeError("origin must hold 3 values")
        return (nx, ny, nz), (nz + 1, ny + 1, nx + 1), origin

    def wtsdf_integrate_device(self, zmap, v0, nv, dims, origin, voxel, trunc, min_weight, tsdf, weight, rgb, cnt,
                               stream=None):
        """mvs_wtsdf_integrate_device on torch device tensors (contiguous: zmap
        float64 (nv,H,W); over the lattice (nz+1,ny+1,nx+1) of dims = (nx, ny,
        nz): tsdf float64, weight int32, rgb uint8 (..,3), cnt uint8, all written
        whole); origin: 3 host doubles; stream-ordered."""
        (nx, ny, nz), shape, origin = self._lattice(dims, origin)
        _need("wtsdf_integrate_device", [("zmap", zmap, 8, (int(nv), self.H, self.W)), ("tsdf", tsdf, 8, shape),
                                         ("weight", weight, 4, shape), ("rgb", rgb, 1, shape + (3,)),
                                         ("cnt", cnt, 1, shape)])
        rc = load().mvs_wtsdf_integrate_device(self._h, zmap.data_ptr(), int(v0), int(nv), nx, ny, nz, _p(origin, _dp),
                                               float(voxel), float(trunc), int(min_weight), tsdf.data_ptr(),
                                               weight.data_ptr(), rgb.data_ptr(), cnt.data_ptr(), stream)
        check(rc, self._h, "mvs_wtsdf_integrate_device")

    def wtsdf_integrate(self, zmap, dims, origin, voxel, trunc, min_weight=1, views=None):
        """The signed-distance lattice of depth maps (mvs_wtsdf_integrate, host
        pointers) -> tsdf (nz+1,ny+1,nx+1) float64 (nan below min_weight), weight
        int32, rgb (..,3) uint8, cnt uint8."""
        v0, nv = self._view_range(views)
        (nx, ny, nz), shape, origin = self._lattice(dims, origin)
        if min(nx, ny, nz) < 0 or (nx + 1) * (ny + 1) * (nz + 1) > 1 << 27:
            raise RuntimeError("wtsdf_integrate: more than 2^27 lattice points")
        zmap = _c(zmap, np.float64).reshape(nv, self.H, self.W)
        tsdf = np.empty(shape, np.float64)
        weight = np.empty(shape, np.int32)
        rgb = np.empty(shape + (3,), np.uint8)
        cnt = np.empty(shape, np.uint8)
        rc = load().mvs_wtsdf_integrate(self._h, _p(zmap, _dp), v0, nv, nx, ny, nz, _p(origin, _dp), float(voxel),
                                        float(trunc), int(min_weight), _p(tsdf, _dp), _p(weight, _i32p),
                                        _p(rgb, _u8p), _p(cnt, _u8p))
        check(rc, self._h, "mvs_wtsdf_integrate")
        return tsdf, weight, rgb, cnt

    def wmesh_extract_device(self, dims, origin, voxel, tsdf, rgb, cnt, vert, vcol, tri, total, stream=None):
        """mvs_wmesh_extract_device on torch device tensors (contiguous: over the
        lattice (nz+1,ny+1,nx+1) of dims: tsdf float64, rgb uint8 (..,3), cnt
        uint8; vert float64 (cap_v,3), vcol uint8 (cap_v,3), tri int32 (cap_t,3),
        each may be None for a cap of 0 (vert and vcol together); total int64
        (2,): vertices, triangles); stream-ordered."""
        (nx, ny, nz), shape, origin = self._lattice(dims, origin)
        if (vert is None) != (vcol is None):
            raise RuntimeError("wmesh_extract_device: vert and vcol come together")
        cap_v = 0 if vert is None else int(vert.shape[0])
        cap_t = 0 if tri is None else int(tri.shape[0])
        _need("wmesh_extract_device", [("tsdf", tsdf, 8, shape), ("rgb", rgb, 1, shape + (3,)), ("cnt", cnt, 1, shape),
                                       ("vert", vert, 8, (cap_v, 3)), ("vcol", vcol, 1, (cap_v, 3)),
                                       ("tri", tri, 4, (cap_t, 3)), ("total", total, 8, (2,))])
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        rc = load().mvs_wmesh_extract_device(self._h, nx, ny, nz, _p(origin, _dp), float(voxel), tsdf.data_ptr(),
                                             rgb.data_ptr(), cnt.data_ptr(), cap_v, cap_t, ptr(vert), ptr(vcol),
                                             ptr(tri), total.data_ptr(), stream)
        check(rc, self._h, "mvs_wmesh_extract_device")

    def wmesh_extract(self, tsdf, rgb, cnt, origin, voxel, cap_v=None, cap_t=None):
        """Marching tetrahedra over a lattice (mvs_wmesh_extract, host pointers):
        tsdf (nz+1,ny+1,nx+1) float64, rgb (..,3) uint8, cnt uint8 -> vertices
        (n,3) float64, colors (n,3) uint8, faces (m,3) int32 and total (2,) int64,
        the full counts.  cap_v, cap_t None: a counting call first, then the exact
        sizes; given: the first min(cap, total) entries."""
        tsdf = _c(tsdf, np.float64)
        if tsdf.ndim != 3 or min(tsdf.shape) < 2:
            raise RuntimeError("wmesh_extract: tsdf must be (nz+1, ny+1, nx+1) with at least 2 points per axis")
        nz, ny, nx = (n - 1 for n in tsdf.shape)
        _, shape, origin = self._lattice((nx, ny, nz), origin)
        rgb = _c(rgb, np.uint8).reshape(shape + (3,))
        cnt = _c(cnt, np.uint8).reshape(shape)
        total = np.zeros(2, np.int64)

        def call(cv, ct):
            vert = np.zeros((max(cv, 1), 3))
            vcol = np.zeros((max(cv, 1), 3), np.uint8)
            tri = np.zeros((max(ct, 1), 3), np.int32)
            rc = load().mvs_wmesh_extract(self._h, nx, ny, nz, _p(origin, _dp), float(voxel), _p(tsdf, _dp),
                                          _p(rgb, _u8p), _p(cnt, _u8p), cv, ct, _p(vert, _dp), _p(vcol, _u8p),
                                          _p(tri, _i32p), _p(total, _i64p))
            check(rc, self._h, "mvs_wmesh_extract")
            nv_, nt_ = min(cv, int(total[0])), min(ct, int(total[1]))
            return vert[:nv_], vcol[:nv_], tri[:nt_]

        if cap_v is None or cap_t is None:
            call(0, 0)
            cap_v = int(total[0]) if cap_v is None else cap_v
            cap_t = int(total[1]) if cap_t is None else cap_t
        vert, vcol, tri = call(int(cap_v), int(cap_t))
        return vert, vcol, tri, total

    def mesh_depth(self, maps, views=None, bounds=None, resolution=256, trunc_voxels=3.0, min_weight=1, rel_tol=0.01,
                   min_consistent=2, max_violations=0, timer=None):
        """A triangle mesh from the depth maps that depth_maps or densify_depth
        returns (`maps` needs z; the definitions are in include/mvs_amd.h).
        wdepth_consist_device counts the agreeing views of the maps as given;
        a pixel that fails the fusion rule of those calls (a finite depth, cons
        >= min_consistent, viol <= max_violations) is set to +inf, so an
        unconfirmed depth neither votes nor carves.  The lattice (mesh_grid):
        bounds = (lo, hi) as given with voxel = its longest side / resolution;
        by default the per-axis 0.5 to 99.5 percentile box of maps["points"],
        which gives the voxel the same way and is then grown by 2 trunc; trunc =
        trunc_voxels voxel.  wtsdf_integrate_device fuses the maps and
        wmesh_extract_device meshes the lattice, once to count and once to
        write.  Everything runs on the context's torch side stream.

        Returns a dict of numpy arrays: vertices (n,3) float64, colors (n,3)
        uint8, faces (m,3) int32, tsdf (nz+1,ny+1,nx+1) float64 (nan = unseen),
        weight int32, origin (3,) float64, voxel (a float) and dims (3,) int32
        (nx, ny, nz).  timer: an optional callable timer(phase, 0) called on the
        chain's stream before each phase ("consist", "mask", "integrate",
        "count", "extract") and with "end" after the last."""
        import torch
        if "z" not in maps:
            raise RuntimeError("mesh_depth: maps has no 'z'")
        v0, nv = self._view_range(views)
        H, W = self.H, self.W
        z0 = _c(maps["z"], np.float64).reshape(nv, H, W)
        origin, voxel, dims, trunc = mesh_grid(maps.get("points"), bounds, resolution, trunc_voxels)
        nx, ny, nz = dims
        shape = (nz + 1, ny + 1, nx + 1)
        if shape[0] * shape[1] * shape[2] > 1 << 27:
            raise RuntimeError("mesh_depth: more than 2^27 lattice points; lower the resolution")
        dev, st, sh, tick = self._chain(timer)
        with torch.cuda.stream(st):
            z = torch.from_numpy(z0).to(dev)
            cons = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            tick("consist", 0)
            self.wdepth_consist_device(z, v0, nv, rel_tol, cons, viol, stream=sh)
            tick("mask", 0)
            keep = torch.isfinite(z) & (cons >= int(min_consistent)) & (viol <= int(max_violations))
            z = torch.where(keep, z, torch.full((), float("inf"), dtype=torch.float64, device=dev)).contiguous()
            tsdf = torch.empty(shape, dtype=torch.float64, device=dev)
            weight = torch.empty(shape, dtype=torch.int32, device=dev)
            rgb = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
            cnt = torch.empty(shape, dtype=torch.uint8, device=dev)
            total = torch.zeros(2, dtype=torch.int64, device=dev)
            tick("integrate", 0)
            self.wtsdf_integrate_device(z, v0, nv, dims, origin, voxel, trunc, min_weight, tsdf, weight, rgb, cnt,
                                        stream=sh)
            tick("count", 0)
            self.wmesh_extract_device(dims, origin, voxel, tsdf, rgb, cnt, None, None, None, total, stream=sh)
            n, m = (int(x) for x in total.cpu().numpy())
            if n >= 1 << 31 or m >= 1 << 31:
                raise RuntimeError("mesh_depth: 2^31 or more vertices or triangles; lower the resolution")
            vert = torch.empty((n, 3), dtype=torch.float64, device=dev)
            vcol = torch.empty((n, 3), dtype=torch.uint8, device=dev)
            tri = torch.empty((m, 3), dtype=torch.int32, device=dev)
            tick("extract", 0)
            if n or m:
                self.wmesh_extract_device(dims, origin, voxel, tsdf, rgb, cnt, vert, vcol, tri, total, stream=sh)
            tick("end", 0)
            out = {"vertices": vert.cpu().numpy(), "colors": vcol.cpu().numpy(), "faces": tri.cpu().numpy(),
                   "tsdf": tsdf.cpu().numpy(), "weight": weight.cpu().numpy(), "origin": origin, "voxel": voxel,
                   "dims": np.array(dims, np.int32)}
        st.synchronize()
        return out
