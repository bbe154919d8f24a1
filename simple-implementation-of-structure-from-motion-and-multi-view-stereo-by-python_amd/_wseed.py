"""Seeds from image features and patch colours (csrc/mvs_seed_warp.hip)."""
import numpy as np

from ._abi import _c, _dp, _i32p, _i64p, _p, _u64p, check, load
from ._context import _need, seed_view_pairs


class _Wseed:
    def wseed_pairs(self, neighbours=4, min_axis_cos=0.5):
        """The view pairs the seed matcher is fed (seed_view_pairs on the
        context's rotations): (np, 2) int32, r-major."""
        return seed_view_pairs(self.rproj(), neighbours, min_axis_cos)

    def _seed_tables(self, feat_off, pairs):
        feat_off = _c(feat_off, np.int64).reshape(-1)
        if len(feat_off) != self.V + 1:
            raise RuntimeError(f"wseed_match: feat_off must have V + 1 = {self.V + 1} entries")
        pairs = _c(pairs, np.int32).reshape(-1, 2)
        return feat_off, pairs

    def wseed_match_device(self, feat, feat_off, pairs, epi_px, min_sin2, c, nrm, ref, cand, err, total, stream=None):
        """mvs_wseed_match_device: feat a torch device tensor (contiguous int32
        (F,2) [col, row]), feat_off (V+1,) and pairs (np,2) host arrays, the
        outputs torch device tensors (contiguous: c, nrm float64 (cap,3), ref
        int32 (cap,), cand int32 (cap,4), err float64 (cap,), total int64 (1,))
        or, to count only, c = nrm = ref = cand = err = None; stream-ordered."""
        feat_off, pairs = self._seed_tables(feat_off, pairs)
        F = int(feat.shape[0])
        if feat.dtype.itemsize != 4 or tuple(feat.shape) != (F, 2) or not feat.is_contiguous():
            raise RuntimeError("wseed_match_device: feat must be contiguous int32 (F, 2)")
        if len(feat_off) and int(feat_off[-1]) > F:
            raise RuntimeError("wseed_match_device: feat_off names more features than feat holds")
        outs = [c, nrm, ref, cand, err]
        cap = 0
        if any(x is not None for x in outs):
            cap = int(ref.numel())
            _need("wseed_match_device", [("c", c, 8, (cap, 3)), ("nrm", nrm, 8, (cap, 3)), ("ref", ref, 4, (cap,)),
                                         ("cand", cand, 4, (cap, 4)), ("err", err, 8, (cap,))], optional=False)
        if total.dtype.itemsize != 8 or tuple(total.shape) != (1,):
            raise RuntimeError("wseed_match_device: total must be int64 (1,)")
        ptr = (lambda x: x.data_ptr() if cap else None)
        rc = load().mvs_wseed_match_device(self._h, feat.data_ptr(), _p(feat_off, _i64p), len(pairs), _p(pairs, _i32p),
                                           float(epi_px), float(min_sin2), cap, ptr(c), ptr(nrm), ptr(ref), ptr(cand),
                                           ptr(err), total.data_ptr(), stream)
        check(rc, self._h, "mvs_wseed_match_device")

    def wseed_match(self, feat, feat_off, pairs, epi_px=1.5, min_sin2=1e-4, cap=None):
        """Seed candidates from features (mvs_wseed_match, host pointers): every
        pair (feature a of view r, feature b of view v) of the ordered view
        pairs whose rays pass each other in front of both cameras, with the point
        on a's ray within epi_px pixels of b in v, triangulated into a patch
        (centre on a's ray, normal towards r's camera); the definition is in
        include/mvs_amd.h.  feat (F,2) int32 [col, row] of all views, feat_off
        (V+1,), pairs (np,2).  cap None: a counting call first, then room for
        every candidate.  Returns c (k,3), nrm (k,3), ref (k,) int32, cand (k,4)
        int32 [pair, a, b, v], err (k,) and the total found (k = min(total, cap))."""
        feat_off, pairs = self._seed_tables(feat_off, pairs)
        feat = _c(feat, np.int32).reshape(-1, 2)
        if len(feat_off) and int(feat_off[-1]) > len(feat):
            raise RuntimeError("wseed_match: feat_off names more features than feat holds")
        lib = load()
        total = np.zeros(1, np.int64)

        def call(cap, c, nrm, ref, cand, err):
            opt = (lambda x, t: _p(x, t) if cap else None)
            rc = lib.mvs_wseed_match(self._h, _p(feat, _i32p), _p(feat_off, _i64p), len(pairs), _p(pairs, _i32p),
                                     float(epi_px), float(min_sin2), int(cap), opt(c, _dp), opt(nrm, _dp),
                                     opt(ref, _i32p), opt(cand, _i32p), opt(err, _dp), _p(total, _i64p))
            check(rc, self._h, "mvs_wseed_match")

        if cap is None:
            call(0, None, None, None, None, None)
            cap = int(total[0])
        cap = int(cap)
        c, nrm = np.empty((max(cap, 1), 3)), np.empty((max(cap, 1), 3))
        ref, cand = np.empty(max(cap, 1), np.int32), np.empty((max(cap, 1), 4), np.int32)
        err = np.empty(max(cap, 1))
        total[0] = 0
        call(cap, c, nrm, ref, cand, err)
        k = min(int(total[0]), cap)
        return c[:k], nrm[:k], ref[:k], cand[:k], err[:k], int(total[0])

    def seed_features(self, border):
        """harris_points of every view without the points closer than `border`
        pixels to an image edge: a list of (n_v, 2) int32 [col, row]."""
        b = int(border)
        out = []
        for v in range(self.V):
            p = self.harris_points(v)
            out.append(p[(p[:, 0] >= b) & (p[:, 0] <= self.W - 1 - b) & (p[:, 1] >= b) & (p[:, 1] <= self.H - 1 - b)])
        return out

    def seed_warped(self, feats=None, pairs=None, epi_px=1.5, min_sin2=1e-4, border=None, wid=5):
        """Seed candidates of the warped pipeline from image features (PMVS's
        match step): feats None: harris_points per view; the features closer
        than border (None: wid + 1) to an image edge are dropped; pairs None:
        wseed_pairs(); then one counting and one emitting wseed_match_device
        call on the context's side stream.  feats: a list of V arrays (n_v, 2)
        [col, row].  Returns c (n,3), nrm (n,3), ref (n,) int32, cand (n,4) int32
        [pair, a, b, v] (a, b index the features kept) and err (n,) as numpy;
        the counts are left in self.last_seed (features, pairs, tests, candidates)."""
        import torch
        border = int(wid) + 1 if border is None else int(border)
        if feats is None:
            feats = self.seed_features(border)
        else:
            if len(feats) != self.V:
                raise RuntimeError("seed_warped: feats must hold one array per view")
            feats = [_c(f, np.int32).reshape(-1, 2) for f in feats]
            feats = [f[(f[:, 0] >= border) & (f[:, 0] <= self.W - 1 - border) & (f[:, 1] >= border)
                       & (f[:, 1] <= self.H - 1 - border)] for f in feats]
        pairs = self.wseed_pairs() if pairs is None else _c(pairs, np.int32).reshape(-1, 2)
        nv = np.array([len(f) for f in feats], np.int64)
        feat_off = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
        feat = np.concatenate(feats) if len(feats) else np.empty((0, 2), np.int32)
        tests = int(sum(int(nv[r]) * int(nv[v]) for r, v in pairs)) if len(pairs) and pairs.min() >= 0 \
            and pairs.max() < self.V else 0
        self.last_seed = {"features": int(nv.sum()), "pairs": len(pairs), "tests": tests, "candidates": 0,
                          "feats": feats}
        dev, st, sh, _ = self._chain()
        with torch.cuda.stream(st):
            t_feat = torch.from_numpy(_c(feat, np.int32).reshape(-1, 2)).to(dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            self.wseed_match_device(t_feat, feat_off, pairs, epi_px, min_sin2, None, None, None, None, None, total,
                                    stream=sh)
            n = int(total.item())
            c = torch.empty((n, 3), dtype=torch.float64, device=dev)
            nrm = torch.empty((n, 3), dtype=torch.float64, device=dev)
            ref = torch.empty(n, dtype=torch.int32, device=dev)
            cand = torch.empty((n, 4), dtype=torch.int32, device=dev)
            err = torch.empty(n, dtype=torch.float64, device=dev)
            if n:
                self.wseed_match_device(t_feat, feat_off, pairs, epi_px, min_sin2, c, nrm, ref, cand, err, total,
                                        stream=sh)
            out = tuple(x.cpu().numpy() for x in (c, nrm, ref, cand, err))
        st.synchronize()
        self.last_seed["candidates"] = n
        return out

    def wpatch_color_device(self, c, ref, mask, color, nviews, stream=None):
        """mvs_wpatch_color_device on torch device tensors (contiguous: c float64
        (n,3), ref int32 (n,), mask int64 (n,words), color float64 (n,3), nviews
        int32 (n,)); stream-ordered."""
        n = int(ref.numel())
        _need("wpatch_color_device",
              self._patch_rows(n, c, None, ref, mask) + [("color", color, 8, (n, 3)), ("nviews", nviews, 4, (n,))])
        rc = load().mvs_wpatch_color_device(self._h, n, c.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                            color.data_ptr(), nviews.data_ptr(), stream)
        check(rc, self._h, "mvs_wpatch_color_device")

    def wpatch_color(self, c, ref, mask):
        """The colour of patches (mvs_wpatch_color, host pointers): per channel
        the mean over the views of {ref} + mask that see the centre of the
        bilinear sample of the resident RGB image there, in steps of 1/256.
        Returns color (n,3) float64 (0 where no view sees it) and nviews (n,) int32."""
        n, c, _, ref, mask = self._rows(c, None, ref, mask)
        color = np.zeros((max(n, 1), 3))
        nviews = np.zeros(max(n, 1), np.int32)
        rc = load().mvs_wpatch_color(self._h, n, _p(c, _dp), _p(ref, _i32p), _p(mask, _u64p), _p(color, _dp),
                                     _p(nviews, _i32p))
        check(rc, self._h, "mvs_wpatch_color")
        return color[:n], nviews[:n]
