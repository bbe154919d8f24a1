"""The plane-warped photo test and the patch refinement against it (csrc/mvs_warp.hip, mvs_refine.hip)."""
import math

import numpy as np

from ._abi import _c, _dp, _i32p, _i64p, _p, _u64p, check, load
from ._context import _need


class _Warp:
    def score_warped(self, c, nrm, ref, min_ncc=0.7, wid=5, min_cos=0.0, want_ncc=False):
        """Plane-warped, per-view reprojected photo test (mvs_score_warped) on
        host arrays: the reference window of patch (c, nrm) in view ref is
        carried through the patch plane into every other view whose camera the
        normal faces (cosine > min_cos), sampled bilinearly and compared with
        ctNcc's scaling.  nrm: unit normals pointing towards the cameras (not
        checked).  Call it where the patch normal is known and the views differ
        enough that windows at one pixel no longer show the same surface;
        `score` is the reference's test.

        Returns xy (n,2), mask (n,words) uint64, count (n,), avg (n,) and, with
        want_ncc, ncc (n,V) float64 (nan for ref, culled and failed views)."""
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        if len(c) != n or len(nrm) != n:
            raise RuntimeError("c, nrm and ref lengths differ")
        xy = np.empty((n, 2))
        mask = np.empty((n, self.words), np.uint64)
        count = np.empty(n, np.int32)
        avg = np.empty(n)
        ncc = np.empty((n, self.V)) if want_ncc else None
        rc = load().mvs_score_warped(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), int(wid),
                                     float(min_ncc), float(min_cos), _p(xy, _dp), _p(mask, _u64p),
                                     _p(count, _i32p), _p(avg, _dp), _p(ncc, _dp) if want_ncc else None)
        check(rc, self._h, "mvs_score_warped")
        return (xy, mask, count, avg, ncc) if want_ncc else (xy, mask, count, avg)

    def score_warped_device(self, c, nrm, ref, xy, mask, count, avg=None, ncc=None, min_ncc=0.7, wid=5,
                            min_cos=0.0, stream=None):
        """score_warped on torch device tensors (contiguous: c, nrm float64
        (n,3), ref int32 (n,), xy float64 (n,2), mask int64 (n,words), count
        int32 (n,), avg float64 (n,) or None, ncc float64 (n,V) or None);
        stream-ordered (stream = a hipStream_t handle, None = the context's)."""
        n = int(ref.numel())
        _need("score_warped_device", self._patch_rows(n, c, nrm, ref, None) + [
            ("xy", xy, 8, (n, 2)), ("mask", mask, 8, (n, self.words)), ("count", count, 4, (n,)),
            ("avg", avg, 8, (n,)), ("ncc", ncc, 8, (n, self.V))])
        rc = load().mvs_score_warped_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), int(wid),
                                            float(min_ncc), float(min_cos), xy.data_ptr(), mask.data_ptr(),
                                            count.data_ptr(), avg.data_ptr() if avg is not None else None,
                                            ncc.data_ptr() if ncc is not None else None, stream)
        check(rc, self._h, "mvs_score_warped_device")

    @staticmethod
    def refine_hypotheses(kd, ka):
        """H = (2 kd + 1)(2 ka + 1)^2, the grid size of one refinement level."""
        return (2 * int(kd) + 1) * (2 * int(ka) + 1) ** 2

    def refine_warped_level(self, c, nrm, ref, views, dstep, wid=5, min_cos=0.0, kd=2, ka=1,
                            astep=math.radians(8), step_scale=1.0, want_scores=False):
        """One level of the fixed-grid depth and normal refinement
        (mvs_refine_warped) on host arrays: the H = (2 kd + 1)(2 ka + 1)^2
        plane hypotheses around patch (c, nrm) -- depths k dstep step_scale
        along the reference ray, normals tilted by tan(i astep step_scale) along
        two tangents -- are scored by the mean warped ncc over the patch's view
        list views[i] (int32 (n, tv), -1 padded at the end), and the best is
        chosen; the input patch is kept unless another scores strictly higher.

        Returns c_out (n,3), nrm_out (n,3), best (n,) int32 (-1: nothing valid),
        score_best (n,) and, with want_scores, scores (n, H)."""
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        views = _c(views, np.int32)
        if views.ndim != 2 or len(views) != n:
            raise RuntimeError("views must be (n, tv) int32")
        tv = views.shape[1]
        dstep = _c(dstep, np.float64).reshape(-1)
        if len(c) != n or len(nrm) != n or len(dstep) != n:
            raise RuntimeError("c, nrm, ref, views and dstep lengths differ")
        c_out = np.empty((n, 3))
        nrm_out = np.empty((n, 3))
        best = np.empty(n, np.int32)
        score_best = np.empty(n)
        scores = np.empty((n, self.refine_hypotheses(kd, ka))) if want_scores and 0 <= kd <= 3 and 0 <= ka <= 2 \
            else None
        rc = load().mvs_refine_warped(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(views, _i32p),
                                      int(tv), _p(dstep, _dp), int(wid), float(min_cos), int(kd), int(ka),
                                      float(astep), float(step_scale), _p(c_out, _dp), _p(nrm_out, _dp),
                                      _p(best, _i32p), _p(score_best, _dp),
                                      _p(scores, _dp) if scores is not None else None)
        check(rc, self._h, "mvs_refine_warped")
        return (c_out, nrm_out, best, score_best, scores) if want_scores else (c_out, nrm_out, best, score_best)

    def refine_warped_level_device(self, c, nrm, ref, views, dstep, c_out, nrm_out, best, score_best, scores=None,
                                   wid=5, min_cos=0.0, kd=2, ka=1, astep=math.radians(8), step_scale=1.0,
                                   stream=None):
        """refine_warped_level on torch device tensors (contiguous: c, nrm,
        c_out, nrm_out float64 (n,3), ref, best int32 (n,), views int32 (n,tv),
        dstep, score_best float64 (n,), scores float64 (n,H) or None);
        stream-ordered (stream = a hipStream_t handle, None = the context's).
        c_out / nrm_out must be other tensors than c / nrm."""
        n = int(ref.numel())
        tv = int(views.shape[1]) if views.dim() == 2 else 0
        _need("refine_warped_level_device", self._patch_rows(n, c, nrm, ref, None) + [
            ("views", views, 4, (n, tv)), ("dstep", dstep, 8, (n,)), ("c_out", c_out, 8, (n, 3)),
            ("nrm_out", nrm_out, 8, (n, 3)), ("best", best, 4, (n,)), ("score_best", score_best, 8, (n,)),
            ("scores", scores, 8, (n, self.refine_hypotheses(kd, ka)))])
        rc = load().mvs_refine_warped_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(),
                                             views.data_ptr(), tv, dstep.data_ptr(), int(wid), float(min_cos),
                                             int(kd), int(ka), float(astep), float(step_scale), c_out.data_ptr(),
                                             nrm_out.data_ptr(), best.data_ptr(), score_best.data_ptr(),
                                             scores.data_ptr() if scores is not None else None, stream)
        check(rc, self._h, "mvs_refine_warped_device")

    @staticmethod
    def refine_view_lists(ncc, min_ncc=0.7, max_views=8):
        """The view lists refine_warped builds from score_warped's ncc (n, V):
        per patch the max_views passing views (ncc > min_ncc) with the highest
        ncc, ties to the lower view index, in ascending view order, padded with
        -1 -> int32 (n, max_views)."""
        ncc = np.asarray(ncc, np.float64)
        n, V = ncc.shape
        with np.errstate(invalid="ignore"):
            key = np.where(ncc > min_ncc, ncc, -np.inf)      # nan and failing views last
        order = np.argsort(-key, axis=1, kind="stable")[:, :max_views]   # stable: ties keep the lower view first
        keep = np.take_along_axis(key, order, 1) > -np.inf
        lists = np.where(keep, order, V)                     # V sorts after every view
        lists.sort(axis=1)
        lists[lists == V] = -1
        out = np.full((n, max_views), -1, np.int32)
        out[:, :lists.shape[1]] = lists
        return out

    def refine_depth_steps(self, c, ref, depth_px=1.5):
        """dstep = depth_px * (depth of c in its reference view) / ((fx + fy) / 2):
        the world size of depth_px pixels at the patch."""
        c = _c(c, np.float64).reshape(-1, 3)
        ref = np.asarray(ref).reshape(-1)
        Rp, t, K = self.rproj(), self._t, self._K
        depth = Rp[ref, 2, 0] * c[:, 0] + Rp[ref, 2, 1] * c[:, 1] + Rp[ref, 2, 2] * c[:, 2] + t[ref, 2]
        return depth_px * depth / ((K[ref, 0, 0] + K[ref, 1, 1]) / 2)

    def refine_lists_device(self, ncc, c, ref, views, dstep, sel=None, min_ncc=0.7, max_views=8, depth_px=1.5,
                            stream=None):
        """refine_view_lists and refine_depth_steps on the device
        (mvs_refine_lists_device), bit for bit, on torch device tensors
        (contiguous): ncc float64 (rows,V) as score_warped_device writes it, c
        float64 (rows,3), ref int32 (rows,), views int32 (n,max_views) and dstep
        float64 (n,) the outputs, sel int64 (n,) or None -- output row k is made
        from source row sel[k] (None: row k, n <= rows).  dstep None: lists
        only, c and ref may then be None.  A sel entry outside 0..rows-1 gives
        an all -1 list and dstep nan; a ref outside 0..V-1 gives dstep nan.
        Stream-ordered (stream = a hipStream_t handle, None = the context's);
        the call keeps no state and may run on several streams at once."""
        rows = int(ncc.shape[0]) if ncc.dim() == 2 else 0
        n = int(views.shape[0]) if views.dim() == 2 else 0
        want = [("ncc", ncc, 8, (rows, self.V)), ("views", views, 4, (n, int(max_views)))]
        if dstep is not None:
            if c is None or ref is None:
                raise RuntimeError("refine_lists_device: dstep needs c and ref")
            want += [("c", c, 8, (rows, 3)), ("ref", ref, 4, (rows,)), ("dstep", dstep, 8, (n,))]
        _need("refine_lists_device", want + [("sel", sel, 8, (n,))], floating=("ncc", "c", "dstep"))
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = load().mvs_refine_lists_device(self._h, n, rows, ptr(sel), ncc.data_ptr(),
                                            ptr(c) if dstep is not None else None,
                                            ptr(ref) if dstep is not None else None, float(min_ncc), int(max_views),
                                            float(depth_px), views.data_ptr(), ptr(dstep), stream)
        check(rc, self._h, "mvs_refine_lists_device")

    def refine_lists(self, ncc, c=None, ref=None, sel=None, min_ncc=0.7, max_views=8, depth_px=1.5):
        """refine_lists_device on host arrays (mvs_refine_lists, synchronous):
        ncc (rows,V), c (rows,3) and ref (rows,) or both None (lists only), sel
        (n,) int64 or None.  A sel entry outside 0..rows-1 or a ref outside
        0..V-1 raises.  Returns views (n,max_views) int32 and dstep (n,) float64
        (None without c and ref)."""
        ncc = _c(ncc, np.float64)
        if ncc.ndim != 2 or ncc.shape[1] != self.V:
            raise RuntimeError(f"refine_lists: ncc must be (rows, {self.V})")
        rows = len(ncc)
        if (c is None) != (ref is None):
            raise RuntimeError("refine_lists: c and ref go together")
        if c is not None:
            c = _c(c, np.float64).reshape(-1, 3)
            ref = _c(ref, np.int32).reshape(-1)
            if len(c) != rows or len(ref) != rows:
                raise RuntimeError("refine_lists: ncc, c and ref lengths differ")
        if sel is not None:
            sel = _c(sel, np.int64).reshape(-1)
        n = len(sel) if sel is not None else rows
        mv = int(max_views)
        views = np.empty((n, mv if 1 <= mv <= 32 else 1), np.int32)
        dstep = np.empty(n) if c is not None else None
        rc = load().mvs_refine_lists(self._h, n, rows, _p(sel, _i64p) if sel is not None else None, _p(ncc, _dp),
                                     _p(c, _dp) if c is not None else None,
                                     _p(ref, _i32p) if c is not None else None, float(min_ncc), mv, float(depth_px),
                                     _p(views, _i32p), _p(dstep, _dp) if dstep is not None else None)
        check(rc, self._h, "mvs_refine_lists")
        return views, dstep

    def refine_warped(self, c, nrm, ref, wid=5, min_ncc=0.7, min_cos=0.0, max_views=8, levels=4, kd=2, ka=1,
                      depth_px=1.5, astep=math.radians(8)):
        """Coarse-to-fine depth and normal refinement of patches against the
        plane-warped photo test, one upload, one chain on the context's side
        stream, one download:
          1. score_warped_device with per-view ncc;
          2. refine_lists_device: per patch the view list of refine_view_lists
             (the max_views best passing views) and
          3. dstep = the world size of depth_px pixels at the patch
             (refine_depth_steps);
          4. `levels` level calls (refine_warped_level_device) with step_scale
             = 2^-level, c / nrm ping-ponging between two device buffers, no
             host synchronisation in between;
          5. score_warped_device of the refined patches.
        A patch with no passing view, or invalid in its reference view, comes
        back unchanged (best -1 at every level).

        Returns c' (n,3), nrm' (n,3), (xy, mask, count, avg) of the final test
        and an info dict: views (n, max_views), best (levels, n), score_first
        (n,) the first level's centre score, score_last (n,) the last level's
        best score."""
        import torch
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        levels = int(levels)
        if levels < 1:
            raise RuntimeError("refine_warped: levels must be >= 1")
        if not 1 <= int(max_views) <= 32:
            raise RuntimeError("refine_warped: max_views must be in 1..32")
        if len(c) != n or len(nrm) != n:
            raise RuntimeError("c, nrm and ref lengths differ")
        if n and (ref.min() < 0 or ref.max() >= self.V):
            raise RuntimeError("refine_warped: ref view out of range")
        H = self.refine_hypotheses(kd, ka)
        dev, st, sh, _ = self._chain()   # the context's torch side stream carries the whole chain
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        with torch.cuda.stream(st):
            cur = [torch.from_numpy(c).to(dev), torch.from_numpy(nrm).to(dev)]
            nxt = [torch.empty((n, 3), **f64), torch.empty((n, 3), **f64)]
            t_ref = torch.from_numpy(ref).to(dev)
            xy = torch.empty((n, 2), **f64)
            mask = torch.empty((n, self.words), dtype=torch.int64, device=dev)
            count = torch.empty(n, **i32)
            avg = torch.empty(n, **f64)
            ncc = torch.empty((n, self.V), **f64)
            self.score_warped_device(cur[0], cur[1], t_ref, xy, mask, count, None, ncc, min_ncc, wid, min_cos,
                                     stream=sh)
            t_views = torch.empty((n, int(max_views)), **i32)
            t_dstep = torch.empty(n, **f64)
            self.refine_lists_device(ncc, cur[0], t_ref, t_views, t_dstep, None, min_ncc, int(max_views), depth_px,
                                     stream=sh)
            best = torch.empty((levels, n), **i32)
            sbest = torch.empty(n, **f64)
            first = torch.empty((n, H), **f64)
            for lev in range(levels):
                self.refine_warped_level_device(cur[0], cur[1], t_ref, t_views, t_dstep, nxt[0], nxt[1], best[lev],
                                                sbest, first if lev == 0 else None, wid, min_cos, kd, ka, astep,
                                                2.0 ** -lev, stream=sh)
                cur, nxt = nxt, cur
            self.score_warped_device(cur[0], cur[1], t_ref, xy, mask, count, avg, None, min_ncc, wid, min_cos,
                                     stream=sh)
            info = {"views": t_views.cpu().numpy(), "best": best.cpu().numpy(),
                    "score_first": first[:, (H - 1) // 2].cpu().numpy(), "score_last": sbest.cpu().numpy()}
            out = (cur[0].cpu().numpy(), cur[1].cpu().numpy(),
                   (xy.cpu().numpy(), mask.cpu().numpy().view(np.uint64), count.cpu().numpy(), avg.cpu().numpy()),
                   info)
        st.synchronize()
        return out
