"""Depth maps of a warped patch set, densified by plane propagation (csrc/mvs_depth_warp.hip, mvs_prop_warp.hip)."""
import math

import numpy as np

from ._abi import _c, _dp, _i32p, _p, _u8p, _u64p, check, load
from ._context import _need, seed_view_pairs


def wprop_view_lists(Rp, tv=4, min_axis_cos=0.5, v0=0, nv=None):
    """The view lists of the propagation sweep for the views v0 .. v0 + nv - 1
    -> (nv, tv) int32: the rows of seed_view_pairs(Rp, tv, min_axis_cos) grouped
    by their first view, in that order, padded with -1."""
    Rp = np.asarray(Rp, np.float64).reshape(-1, 3, 3)
    nv = len(Rp) - v0 if nv is None else int(nv)
    out = np.full((nv, int(tv)), -1, np.int32)
    fill = [0] * nv
    for r, v in seed_view_pairs(Rp, int(tv), min_axis_cos).tolist():
        if v0 <= r < v0 + nv:
            out[r - v0, fill[r - v0]] = v
            fill[r - v0] += 1
    return out


class _Wdepth:
    def wdepth_splat_device(self, c, nrm, ref, mask, radius, slope, v0, nv, zmap, idmap, stream=None):
        """mvs_wdepth_splat_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), zmap float64 and
        idmap int32 (nv,H,W), both written whole); stream-ordered."""
        n = int(ref.numel())
        maps = (int(nv), self.H, self.W)
        _need("wdepth_splat_device",
              self._patch_rows(n, c, nrm, ref, mask) + [("zmap", zmap, 8, maps), ("idmap", idmap, 4, maps)])
        rc = load().mvs_wdepth_splat_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                            int(radius), float(slope), int(v0), int(nv), zmap.data_ptr(),
                                            idmap.data_ptr(), stream)
        check(rc, self._h, "mvs_wdepth_splat_device")

    def wdepth_consist_device(self, zmap, v0, nv, rel_tol, cons, viol=None, stream=None):
        """mvs_wdepth_consist_device on torch device tensors (contiguous: zmap
        float64, cons and viol uint8 (nv,H,W); viol may be None); stream-ordered."""
        maps = (int(nv), self.H, self.W)
        _need("wdepth_consist_device", [("zmap", zmap, 8, maps), ("cons", cons, 1, maps), ("viol", viol, 1, maps)])
        rc = load().mvs_wdepth_consist_device(self._h, zmap.data_ptr(), int(v0), int(nv), float(rel_tol),
                                              cons.data_ptr(), viol.data_ptr() if viol is not None else None, stream)
        check(rc, self._h, "mvs_wdepth_consist_device")

    def wdepth_points_device(self, pix, zmap, v0, nv, xyz, rgb, stream=None):
        """mvs_wdepth_points_device on torch device tensors (contiguous: pix int32
        (m,3) rows (view, x, y), zmap float64 (nv,H,W), xyz float64 (m,3), rgb
        uint8 (m,3)); stream-ordered."""
        m = int(pix.shape[0])
        _need("wdepth_points_device", [("pix", pix, 4, (m, 3)), ("zmap", zmap, 8, (int(nv), self.H, self.W)),
                                       ("xyz", xyz, 8, (m, 3)), ("rgb", rgb, 1, (m, 3))])
        rc = load().mvs_wdepth_points_device(self._h, m, pix.data_ptr(), zmap.data_ptr(), int(v0), int(nv),
                                             xyz.data_ptr(), rgb.data_ptr(), stream)
        check(rc, self._h, "mvs_wdepth_points_device")

    def wdepth_splat(self, c, nrm, ref, mask, radius=1, slope=4.0, views=None):
        """Depth and patch-index maps of a patch set (mvs_wdepth_splat, host
        pointers): zmap (nv,H,W) float64 (+inf = empty) and idmap int32 (-1)."""
        v0, nv = self._view_range(views)
        n, c, nrm, ref, mask = self._rows(c, nrm, ref, mask)
        zmap = np.empty((nv, self.H, self.W), np.float64)
        idmap = np.empty((nv, self.H, self.W), np.int32)
        rc = load().mvs_wdepth_splat(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(mask, _u64p),
                                     int(radius), float(slope), v0, nv, _p(zmap, _dp), _p(idmap, _i32p))
        check(rc, self._h, "mvs_wdepth_splat")
        return zmap, idmap

    def wdepth_consist(self, zmap, rel_tol=0.01, views=None):
        """The cross-view consistency count of depth maps (mvs_wdepth_consist,
        host pointers) -> cons, viol (nv,H,W) uint8."""
        v0, nv = self._view_range(views)
        zmap = _c(zmap, np.float64).reshape(nv, self.H, self.W)
        cons = np.empty((nv, self.H, self.W), np.uint8)
        viol = np.empty((nv, self.H, self.W), np.uint8)
        rc = load().mvs_wdepth_consist(self._h, _p(zmap, _dp), v0, nv, float(rel_tol), _p(cons, _u8p), _p(viol, _u8p))
        check(rc, self._h, "mvs_wdepth_consist")
        return cons, viol

    def wdepth_points(self, pix, zmap, views=None):
        """World points and colours of listed pixels (mvs_wdepth_points, host
        pointers; a pixel outside the range or the image raises) -> xyz (m,3)
        float64 and rgb (m,3) uint8."""
        v0, nv = self._view_range(views)
        pix = _c(pix, np.int32).reshape(-1, 3)
        m = len(pix)
        zmap = _c(zmap, np.float64).reshape(nv, self.H, self.W)
        xyz = np.zeros((max(m, 1), 3))
        rgb = np.zeros((max(m, 1), 3), np.uint8)
        rc = load().mvs_wdepth_points(self._h, m, _p(pix, _i32p), _p(zmap, _dp), v0, nv, _p(xyz, _dp), _p(rgb, _u8p))
        check(rc, self._h, "mvs_wdepth_points")
        return xyz[:m], rgb[:m]

    def depth_maps(self, patches, radius=1, slope=4.0, views=None, rel_tol=0.01, min_consistent=2, max_violations=0,
                   timer=None):
        """Per-view depth and normal maps of a warped patch set and the dense
        cloud fused from them (the definitions are in include/mvs_amd.h).
        `patches` is the dict expand_warped, filter_warped or reconstruct_warped
        returns; it needs c, nrm, ref and mask.  views: None (every view) or
        (v0, nv).  The maps are splatted (wdepth_splat_device), the other views
        that agree with or see through each pixel are counted
        (wdepth_consist_device), and a pixel (v, q) is fused when id >= 0,
        ref[id] = v, cons >= min_consistent and viol <= max_violations: the ref
        rule emits a surface point once, in its patch's reference view.  The
        fused points and colours come from wdepth_points_device; selection and
        gathers are torch indexing on the device.  Everything runs on the
        context's torch side stream.

        Returns a dict of numpy arrays: z (nv,H,W) float64 (+inf = empty), id
        int32 (-1), cons and viol uint8, normal (nv,H,W,3) float64 (nan where
        empty), and the fused cloud points (m,3), normals (m,3), colors (m,3)
        uint8 and pix (m,3) int32 rows (view, x, y) in the maps' order.
        timer: an optional callable timer(phase, 0) called on the chain's stream
        before each phase ("splat", "consist", "select", "points") and with
        phase "end" after the last."""
        import torch
        for k in ("c", "nrm", "ref", "mask"):
            if k not in patches:
                raise RuntimeError(f"depth_maps: patches has no '{k}'")
        v0, nv = self._view_range(views)
        n, c0, n0, ref0, m0 = self._rows(patches["c"], patches["nrm"], patches["ref"], patches["mask"])
        dev, st, sh, tick = self._chain(timer)
        H, W = self.H, self.W
        with torch.cuda.stream(st):
            c, nrm, ref, mask = (self._dev_tensor(x, None, x.shape) for x in (c0, n0, ref0, m0))
            z = torch.empty((nv, H, W), dtype=torch.float64, device=dev)
            idm = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
            cons = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            tick("splat", 0)
            self.wdepth_splat_device(c, nrm, ref, mask, radius, slope, v0, nv, z, idm, stream=sh)
            tick("consist", 0)
            self.wdepth_consist_device(z, v0, nv, rel_tol, cons, viol, stream=sh)
            tick("select", 0)
            drawn = idm >= 0
            row = idm.clamp(min=0).long()
            if n:
                owner = ref[row.reshape(-1)].reshape(nv, H, W)
                normal = torch.where(drawn.unsqueeze(-1), nrm[row.reshape(-1)].reshape(nv, H, W, 3),
                                     torch.full((), float("nan"), dtype=torch.float64, device=dev))
            else:
                owner = torch.full((nv, H, W), -1, dtype=torch.int32, device=dev)
                normal = torch.full((nv, H, W, 3), float("nan"), dtype=torch.float64, device=dev)
            here = torch.arange(v0, v0 + nv, dtype=torch.int32, device=dev).reshape(nv, 1, 1)
            sel = drawn & (owner == here) & (cons >= int(min_consistent)) & (viol <= int(max_violations))
            at = sel.nonzero()                                   # (view of the range, row, column), in the maps' order
            pix = torch.stack([at[:, 0] + v0, at[:, 2], at[:, 1]], 1).to(torch.int32).contiguous()
            m = int(pix.shape[0])
            xyz = torch.empty((m, 3), dtype=torch.float64, device=dev)
            rgb = torch.empty((m, 3), dtype=torch.uint8, device=dev)
            tick("points", 0)
            self.wdepth_points_device(pix, z, v0, nv, xyz, rgb, stream=sh)
            normals = normal[at[:, 0], at[:, 1], at[:, 2]]
            tick("end", 0)
            out = {"z": z.cpu().numpy(), "id": idm.cpu().numpy(), "cons": cons.cpu().numpy(),
                   "viol": viol.cpu().numpy(), "normal": normal.cpu().numpy(), "points": xyz.cpu().numpy(),
                   "normals": normals.cpu().numpy().reshape(m, 3), "colors": rgb.cpu().numpy(),
                   "pix": pix.cpu().numpy()}
        st.synchronize()
        return out

    # the default schedule of densify_depth: (step, kd, ka, step_scale) per sweep
    DENSIFY_SCHEDULE = tuple((st, 1, 1, 1.0 if k < 4 else 0.5)
                             for k, st in enumerate((1, 3, 1, 5, 1, 3, 1, 1, 1, 1, 1, 1)))
    DENSIFY_ASTEP = math.radians(8)
    DENSIFY_DEPTH_PX = 1.0

    @staticmethod
    def wprop_hypotheses(kd, ka):
        """HY = 5 + (2 kd + 1)(2 ka + 1)^2: the hypotheses of a pixel in one sweep."""
        return 5 + (2 * int(kd) + 1) * (2 * int(ka) + 1) ** 2

    def wprop_view_lists(self, tv=4, min_axis_cos=0.5, views=None):
        """The view lists a sweep is fed -> (nv, tv) int32: the rows of
        seed_view_pairs(rproj(), tv, min_axis_cos) grouped by their first view
        (in that order) and padded with -1: one rule for neighbour views in the
        whole warped family.  views: None (every view) or (v0, nv)."""
        v0, nv = self._view_range(views)
        return wprop_view_lists(self.rproj(), tv, min_axis_cos, v0, nv)

    def _wprop_lists(self, lists, nv):
        lists = _c(lists, np.int32)
        if lists.ndim != 2 or lists.shape[0] != nv or not 1 <= lists.shape[1] <= 32:
            raise RuntimeError(f"wprop_sweep: lists must be ({nv}, tv) with tv in 1..32")
        return lists

    def wprop_sweep_device(self, zmap, nmap, lists, v0, nv, z_out, n_out, score, best, scores=None, wid=5,
                           min_cos=0.3, min_ncc=0.7, top_k=2, step=1, kd=1, ka=1, astep=math.radians(8),
                           depth_px=1.0, step_scale=1.0, stream=None):
        """mvs_wprop_sweep_device on torch device tensors (contiguous: zmap,
        z_out, score float64 (nv,H,W), nmap, n_out float64 (nv,H,W,3), best int32
        (nv,H,W), scores float64 (nv,H,W,HY) or None; every output written whole);
        lists is a host int32 array (nv, tv).  Stream-ordered."""
        nv = int(nv)
        lists = self._wprop_lists(lists, nv)
        maps = (nv, self.H, self.W)
        hy = self.wprop_hypotheses(kd, ka)
        _need("wprop_sweep_device", [("zmap", zmap, 8, maps), ("nmap", nmap, 8, maps + (3,)), ("z_out", z_out, 8, maps),
                                     ("n_out", n_out, 8, maps + (3,)), ("score", score, 8, maps),
                                     ("best", best, 4, maps), ("scores", scores, 8, maps + (hy,))])
        rc = load().mvs_wprop_sweep_device(self._h, int(v0), nv, zmap.data_ptr(), nmap.data_ptr(), _p(lists, _i32p),
                                           lists.shape[1], int(wid), float(min_cos), float(min_ncc), int(top_k),
                                           int(step), int(kd), int(ka), float(astep), float(depth_px),
                                           float(step_scale), z_out.data_ptr(), n_out.data_ptr(), score.data_ptr(),
                                           best.data_ptr(), scores.data_ptr() if scores is not None else None, stream)
        check(rc, self._h, "mvs_wprop_sweep_device")

    def wprop_sweep(self, zmap, nmap, lists, views=None, wid=5, min_cos=0.3, min_ncc=0.7, top_k=2, step=1, kd=1, ka=1,
                    astep=math.radians(8), depth_px=1.0, step_scale=1.0, want_scores=False):
        """One propagation sweep on numpy maps (mvs_wprop_sweep, host pointers)
        -> dict z (nv,H,W), normal (nv,H,W,3), score, best int32 and, with
        want_scores, scores (nv,H,W,HY)."""
        v0, nv = self._view_range(views)
        lists = self._wprop_lists(lists, nv)
        maps = (nv, self.H, self.W)
        zmap = _c(zmap, np.float64).reshape(maps)
        nmap = _c(nmap, np.float64).reshape(maps + (3,))
        z = np.empty(maps)
        n = np.empty(maps + (3,))
        score = np.empty(maps)
        best = np.empty(maps, np.int32)
        scores = np.empty(maps + (self.wprop_hypotheses(kd, ka),)) if want_scores else None
        rc = load().mvs_wprop_sweep(self._h, v0, nv, _p(zmap, _dp), _p(nmap, _dp), _p(lists, _i32p), lists.shape[1],
                                    int(wid), float(min_cos), float(min_ncc), int(top_k), int(step), int(kd), int(ka),
                                    float(astep), float(depth_px), float(step_scale), _p(z, _dp), _p(n, _dp),
                                    _p(score, _dp), _p(best, _i32p), _p(scores, _dp) if want_scores else None)
        check(rc, self._h, "mvs_wprop_sweep")
        out = {"z": z, "normal": n, "score": score, "best": best}
        if want_scores:
            out["scores"] = scores
        return out

    def densify_depth(self, maps, views=None, lists=None, tv=4, wid=5, min_ncc=0.7, min_cos=0.3, top_k=2,
                      schedule=None, rel_tol=0.01, min_consistent=2, max_violations=0, timer=None):
        """Densify the maps depth_maps returns (`maps` needs z and normal) by
        per-pixel plane propagation (mvs_wprop_sweep, include/mvs_amd.h) and fuse
        them.  Two sets of device maps are ping-ponged through the sweeps of
        `schedule`, a list of (step, kd, ka, step_scale) (default
        DENSIFY_SCHEDULE: 12 sweeps, steps 1,3,1,5,1,3,1,1,1,1,1,1, a 3 x 3 x 3
        grid of 1 px in depth and 8 degrees, halved after the fourth sweep);
        lists: the (nv, tv) view lists (default wprop_view_lists(tv)).  Then
        wdepth_consist_device counts the agreeing views and a pixel is fused
        when it holds a depth, cons >= min_consistent and viol <=
        max_violations.  There is no ref rule here -- a densified pixel has no
        owner patch -- so a surface point is emitted in every view that holds
        it; the cloud is not de-duplicated across views.  Everything runs on
        the context's torch side stream.

        Returns a dict of numpy arrays: z (nv,H,W) float64 (+inf = empty),
        normal (nv,H,W,3) (nan where empty), score float64, best int32 (of the
        last sweep), cons and viol uint8, the fused cloud points (m,3), normals
        (m,3), colors (m,3) uint8, pix (m,3) int32 rows (view, x, y) in the
        maps' order, and history (sweeps, 2) int64: per sweep the pixels that
        hold a depth after it and the pixels whose best > 0 (gathered on the
        device, copied once at the end).  timer: an optional callable
        timer(phase, k) called on the chain's stream before sweep k ("sweep"),
        before "consist", "select" and "points", and with "end" after the last."""
        import torch
        v0, nv = self._view_range(views)
        H, W = self.H, self.W
        if lists is None:
            lists = self.wprop_view_lists(tv, views=(v0, nv))
        lists = self._wprop_lists(lists, nv)
        schedule = list(self.DENSIFY_SCHEDULE if schedule is None else schedule)
        z0 = _c(maps["z"], np.float64).reshape(nv, H, W)
        n0 = _c(maps["normal"], np.float64).reshape(nv, H, W, 3)
        dev, st, sh, tick = self._chain(timer)
        with torch.cuda.stream(st):
            z = [torch.from_numpy(z0).to(dev), torch.empty((nv, H, W), dtype=torch.float64, device=dev)]
            nm = [torch.from_numpy(n0).to(dev), torch.empty((nv, H, W, 3), dtype=torch.float64, device=dev)]
            score = torch.full((nv, H, W), float("nan"), dtype=torch.float64, device=dev)
            best = torch.full((nv, H, W), -1, dtype=torch.int32, device=dev)
            hist = torch.zeros((max(len(schedule), 1), 2), dtype=torch.int64, device=dev)
            cur = 0
            for k, (step, kd, ka, scale) in enumerate(schedule):
                tick("sweep", k)
                self.wprop_sweep_device(z[cur], nm[cur], lists, v0, nv, z[1 - cur], nm[1 - cur], score, best, None,
                                        wid, min_cos, min_ncc, top_k, step, kd, ka, self.DENSIFY_ASTEP,
                                        self.DENSIFY_DEPTH_PX, scale, stream=sh)
                cur = 1 - cur
                hist[k, 0] = (best >= 0).sum()
                hist[k, 1] = (best > 0).sum()
            zf, nf = z[cur], nm[cur]
            if not schedule:   # no sweep: the maps as given
                zf = torch.where(torch.isfinite(zf) & (zf > 0), zf, torch.full((), float("inf"), dtype=torch.float64,
                                                                               device=dev))
            cons = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            viol = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            tick("consist", 0)
            self.wdepth_consist_device(zf, v0, nv, rel_tol, cons, viol, stream=sh)
            tick("select", 0)
            sel = torch.isfinite(zf) & (zf > 0) & (cons >= int(min_consistent)) & (viol <= int(max_violations))
            at = sel.nonzero()                                   # (view of the range, row, column), in the maps' order
            pix = torch.stack([at[:, 0] + v0, at[:, 2], at[:, 1]], 1).to(torch.int32).contiguous()
            m = int(pix.shape[0])
            xyz = torch.empty((m, 3), dtype=torch.float64, device=dev)
            rgb = torch.empty((m, 3), dtype=torch.uint8, device=dev)
            tick("points", 0)
            self.wdepth_points_device(pix, zf, v0, nv, xyz, rgb, stream=sh)
            normals = nf[at[:, 0], at[:, 1], at[:, 2]]
            tick("end", 0)
            out = {"z": zf.cpu().numpy(), "normal": nf.cpu().numpy(), "score": score.cpu().numpy(),
                   "best": best.cpu().numpy(), "cons": cons.cpu().numpy(), "viol": viol.cpu().numpy(),
                   "points": xyz.cpu().numpy(), "normals": normals.cpu().numpy().reshape(m, 3),
                   "colors": rgb.cpu().numpy(), "pix": pix.cpu().numpy(),
                   "history": hist.cpu().numpy()[:len(schedule)]}
        st.synchronize()
        return out
