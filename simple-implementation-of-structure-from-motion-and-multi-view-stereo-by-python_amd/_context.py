"""The core of MvsContext (csrc/mvs_context.cpp, mvs_engine.cpp, mvs_geometry.cpp): the live contexts and their
atexit hook, lifetime, scorers, SfM front-end, the helpers the families' wrappers share, the context-free calls."""
import atexit
import ctypes
import weakref

import numpy as np

from ._abi import _c, _dp, _fp, _i32p, _i64p, _p, _u8p, _u64p, _vp, check, load


def rodrigues_roundtrip(R):
    """R' = Rodrigues(Rodrigues(R)) -- the rotation cv2.projectPoints applies (utils.py:242-243)."""
    R = _c(R, np.float64).reshape(9)
    out = np.empty(9)
    check(load().mvs_rodrigues_roundtrip(_p(R, _dp), _p(out, _dp)), what="rodrigues")
    return out.reshape(3, 3)


def sfm_pair(KA, RA, tA, KB, RB, tB, q, tr, max_err):
    """One pair of StructureFromMotion's loop (SFM.py:60-80), host C++:
    (float32 points (n, 3), keep (n,) bool)."""
    mats = [_c(m, np.float64).reshape(-1) for m in (KA, RA, tA, KB, RB, tB)]
    q = _c(q, np.float32).reshape(-1, 2)
    tr = _c(tr, np.float32).reshape(-1, 2)
    n = len(q)
    if len(tr) != n:
        raise RuntimeError("query and train correspondences differ in length")
    pt = np.empty((max(n, 1), 3), np.float32)
    keep = np.empty(max(n, 1), np.uint8)
    check(load().mvs_sfm_pair(*[_p(m, _dp) for m in mats], n, _p(q, _fp), _p(tr, _fp),
                              float(max_err), _p(pt, _fp), _p(keep, _u8p)), None, "mvs_sfm_pair")
    return pt[:n], keep[:n].astype(bool)


def filter_outliers(cell, mask, count, avg, c, nrm, nci, ncj):
    """CellTable.filter_out_outlier (MVS2.py:132-158) on the host over accepted
    patches in fill order (mvs_filter_outliers): -> (alive bool (n,), removed,
    "remove a outlier" lines).  Raises ZeroDivisionError where the reference does."""
    cell = _c(cell, np.int32).reshape(-1, 2)
    n = len(cell)
    mask = _c(mask, np.uint64).reshape(n, -1)
    count = _c(count, np.int32).reshape(n)
    avg = _c(avg, np.float64).reshape(n)
    c = _c(c, np.float64).reshape(n, 3)
    nrm = _c(nrm, np.float64).reshape(n, 3)
    alive = np.empty(max(n, 1), np.uint8)
    stats = np.zeros(2, np.int64)
    check(load().mvs_filter_outliers(n, mask.shape[1], int(nci), int(ncj), _p(cell, _i32p), _p(mask, _u64p),
                                     _p(count, _i32p), _p(avg, _dp), _p(c, _dp), _p(nrm, _dp),
                                     _p(alive, _u8p), _p(stats, _i64p)), None, "mvs_filter_outliers")
    return alive[:n].astype(bool), int(stats[0]), int(stats[1])


def triangulate(P1, P2, x1, x2):
    """cv2.triangulatePoints for one correspondence (utils.py:238-239), homogeneous 4-vector."""
    P1 = _c(P1, np.float64).reshape(12)
    P2 = _c(P2, np.float64).reshape(12)
    x1 = _c(x1, np.float64).reshape(2)
    x2 = _c(x2, np.float64).reshape(2)
    out = np.empty(4)
    check(load().mvs_triangulate(_p(P1, _dp), _p(P2, _dp), _p(x1, _dp), _p(x2, _dp), _p(out, _dp)),
          what="triangulate")
    return out


def seed_view_pairs(Rp, neighbours=4, min_axis_cos=0.5):
    """The ordered view pairs (r, v) the seed matcher is fed, from the
    rotations Rp (V,3,3) alone: per r the views v != r ranked by the descending
    dot product of the optical axes (the third rows of Rp; Python floats, left
    to right), ties to the lower v; those with a dot >= min_axis_cos; the first
    `neighbours` of them.  (np, 2) int32, r-major."""
    ax = [[float(x) for x in row] for row in np.asarray(Rp, np.float64).reshape(-1, 3, 3)[:, 2, :]]
    V = len(ax)
    out = []
    for r in range(V):
        dots = [(ax[r][0] * ax[v][0] + ax[r][1] * ax[v][1] + ax[r][2] * ax[v][2], v) for v in range(V) if v != r]
        keep = sorted((d, v) for d, v in dots if d >= float(min_axis_cos))
        keep.sort(key=lambda dv: (-dv[0], dv[1]))
        out += [(r, v) for _, v in keep[:max(int(neighbours), 0)]]
    return np.array(out, np.int32).reshape(-1, 2)


# live contexts: a retiring caller stream is announced to each of them
# (stream_retiring), and the ones still open at interpreter exit are closed by
# an atexit hook, before the HIP runtime's own teardown
_LIVE = weakref.WeakSet()


def stream_retiring(stream):
    """A caller stream (a hipStream_t handle) is about to be destroyed: every
    live context waits for its work there now (mvs_stream_retiring)."""
    for cx in list(_LIVE):
        h = getattr(cx, "_h", None)
        if h:
            check(load().mvs_stream_retiring(h, stream), h, "mvs_stream_retiring")


@atexit.register
def _close_live_contexts():
    for cx in list(_LIVE):
        try:
            cx.close()
        except Exception:
            pass


def _need(who, rows, floating=None, optional=True):
    """The *_device wrappers' tensor check: every (name, tensor, itemsize, shape) of rows must be contiguous with
    that element size and shape -- the kernels index rows at a fixed pitch.  A None tensor (an optional argument) is
    skipped unless optional is False.  floating: the names whose dtype must be floating point, no other row's."""
    for name, x, size, shape in rows:
        if x is None and optional:
            continue
        if x is None or x.dtype.itemsize != size or tuple(x.shape) != shape or not x.is_contiguous() or \
                (floating is not None and x.dtype.is_floating_point != (name in floating)):
            raise RuntimeError(f"{who}: {name} must be contiguous, {size}-byte elements, {shape}")


class _Core:
    def __init__(self, imgs, K, R, t, device=0, Rp=None):
        lib = load()
        rgb = _c(np.stack(imgs) if isinstance(imgs, (list, tuple)) else imgs, np.uint8)
        if rgb.ndim != 4 or rgb.shape[-1] != 3:
            raise RuntimeError(f"images must be (V,H,W,3) uint8 RGB, got {rgb.shape}")
        self.V, self.H, self.W = (int(x) for x in rgb.shape[:3])
        self.words = (self.V + 63) // 64
        K = _c(K, np.float64).reshape(self.V, 9)
        R = _c(R, np.float64).reshape(self.V, 9)
        t = _c(t, np.float64).reshape(self.V, 3)
        rp = _c(Rp, np.float64).reshape(self.V, 9) if Rp is not None else None
        h = _vp()
        rc = lib.mvs_ctx_create(int(device), self.V, self.H, self.W, _p(rgb, _u8p), _p(K, _dp),
                                _p(R, _dp), _p(t, _dp), _p(rp, _dp) if rp is not None else None,
                                ctypes.byref(h))
        check(rc, None, "mvs_ctx_create")
        self._h = h
        self.device = device
        self._K = K.reshape(self.V, 3, 3).copy()   # refine_depth_steps
        self._t = t.copy()
        self._refine_stream = None   # refine_warped's torch side stream
        self._stages = weakref.WeakSet()
        _LIVE.add(self)

    def close(self):
        if getattr(self, "_h", None):
            # stepped stages hold the context: they go first
            for st in list(getattr(self, "_stages", ())):
                st.close()
            load().mvs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def rproj(self):
        out = np.empty((self.V, 9))
        check(load().mvs_ctx_rproj(self._h, _p(out, _dp)), self._h, "mvs_ctx_rproj")
        return out.reshape(self.V, 3, 3)

    def exact_hits(self):
        return int(load().mvs_exact_hits(self._h))

    def scorer_stats(self):
        """{'direct': candidates the direct path re-scored (guard band +
        bucket overflow), 'overflow': of them bucket overflow, 'batches':
        tiled batches} since the context was created (mvs_scorer_stats)."""
        out = np.zeros(3, np.int64)
        check(load().mvs_scorer_stats(self._h, _p(out, _i64p)), self._h, "mvs_scorer_stats")
        return {"direct": int(out[0]), "overflow": int(out[1]), "batches": int(out[2])}

    def bin_runs_batches(self):
        """Tiled batches since the context was created that were binned into
        workgroup-private sorted runs (mvs_bin_runs_batches); the others used
        the atomic tile buckets."""
        return int(load().mvs_bin_runs_batches(self._h))

    def rebuild(self, stream=None):
        """Rebuild the device gray stack / view-major copy from the resident
        RGB images (stream-ordered; for cold-sweep timing)."""
        check(load().mvs_ctx_rebuild(self._h, stream), self._h, "mvs_ctx_rebuild")

    def set_images(self, first_view, imgs):
        """Replace the resident RGB images of views first_view, first_view + 1,
        ... by imgs (k, H, W, 3) uint8 (mvs_ctx_set_images, synchronous).  The
        gray stack and the moment tables follow at the next rebuild()."""
        rgb = _c(imgs, np.uint8)
        if rgb.ndim != 4 or rgb.shape[1:] != (self.H, self.W, 3):
            raise RuntimeError(f"images must be (k,{self.H},{self.W},3) uint8 RGB, got {rgb.shape}")
        check(load().mvs_ctx_set_images(self._h, int(first_view), len(rgb), _p(rgb, _u8p)), self._h,
              "mvs_ctx_set_images")

    def kernel_timing(self, enable=True, every=1):
        """Start (reset) or stop HIP-event timing of the dominant scoring kernel;
        every = k times every k-th scoring call."""
        check(load().mvs_kernel_timing(self._h, int(every) if enable else 0), self._h, "mvs_kernel_timing")

    def kernel_time(self):
        """-> (total kernel milliseconds, timed launches) since kernel_timing(True)."""
        ms = ctypes.c_double(0.0)
        k = ctypes.c_int64(0)
        check(load().mvs_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(k)), self._h,
              "mvs_kernel_time")
        return ms.value, int(k.value)

    def timed_kernel(self):
        """Name of the kernel the last timed event pair bracketed."""
        name = load().mvs_timed_kernel(self._h)
        return name.decode() if name else ""

    def score(self, c, ref, min_ncc=0.7, wid=5):
        """Batched photo_consistenecy_test (MVS2.py:62-77) on host arrays.

        Returns xy (n,2), mask (n,words) uint64, count (n,), avg (n,)."""
        c = _c(c, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        if len(c) != n:
            raise RuntimeError("c and ref lengths differ")
        xy = np.empty((n, 2))
        mask = np.empty((n, self.words), np.uint64)
        count = np.empty(n, np.int32)
        avg = np.empty(n)
        rc = load().mvs_score(self._h, n, _p(c, _dp), _p(ref, _i32p), int(wid), float(min_ncc),
                              _p(xy, _dp), _p(mask, _u64p), _p(count, _i32p), _p(avg, _dp))
        check(rc, self._h, "mvs_score")
        return xy, mask, count, avg

    def exact_avg(self, ref, xy, mask, wid=5):
        """avg_ncc_score in the reference's arithmetic (numpy-order ctNcc, summed in
        view order) for candidates scored by `score`: bit-exact, where score's avg
        is within 1e-12."""
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        xy = _c(xy, np.float64).reshape(n, 2)
        mask = _c(mask, np.uint64).reshape(n, self.words)
        out = np.empty(n)
        check(load().mvs_exact_avg(self._h, n, _p(ref, _i32p), _p(xy, _dp), _p(mask, _u64p), int(wid),
                                   _p(out, _dp)), self._h, "mvs_exact_avg")
        return out

    def score_device(self, c, ref, xy, mask, count, avg, min_ncc=0.7, wid=5, stream=None):
        """Same on device tensors (torch: pass .data_ptr() ints); stream-ordered."""
        n = int(ref.numel()) if hasattr(ref, "numel") else int(len(ref))
        ptr = (lambda x: x.data_ptr()) if hasattr(ref, "data_ptr") else (lambda x: int(x))
        rc = load().mvs_score_device(self._h, n, ptr(c), ptr(ref), int(wid), float(min_ncc),
                                     ptr(xy), ptr(mask), ptr(count),
                                     ptr(avg) if avg is not None else None,
                                     stream)
        check(rc, self._h, "mvs_score_device")

    def score_device_rec(self, c, ref, xy, rec, min_ncc=0.7, wid=5, stream=None):
        """The photo test into records (device int64 tensor (n, words + 1): mask
        words, avg bits; |V| = popcount), stream-ordered."""
        n = int(ref.numel())
        if rec.dtype.itemsize != 8 or tuple(rec.shape) != (n, self.words + 1) or not rec.is_contiguous():
            raise RuntimeError(f"score_device_rec: rec must be contiguous int64 ({n}, {self.words + 1})")
        rc = load().mvs_score_device_rec(self._h, n, c.data_ptr(), ref.data_ptr(), int(wid), float(min_ncc),
                                         xy.data_ptr(), rec.data_ptr(), stream)
        check(rc, self._h, "mvs_score_device_rec")

    def cell_grid(self, cell_size):
        """(nci, ncj) of the expansion's cell grid: whole cells only."""
        s = int(cell_size)
        if not 1 <= s <= 16:
            raise RuntimeError("cell_size must be in 1..16")
        return self.W // s, self.H // s

    def _dev_tensor(self, x, dtype, shape):
        """numpy array or torch tensor -> contiguous tensor of dtype on the context's device."""
        # dtype None: the array's own (uint64 as int64).  An array that already
        # fits costs one copy on the current stream, as torch.from_numpy(x).to(dev)
        import torch
        dev = torch.device(f"cuda:{self.device}")
        if not isinstance(x, torch.Tensor):
            a = np.ascontiguousarray(x)
            if a.dtype == np.uint64:
                a = a.view(np.int64)
            x = torch.from_numpy(a)
        return x.to(device=dev, dtype=dtype).reshape(shape).contiguous()

    def _side_stream(self):
        """The context's torch side stream (the handle of torch's default stream
        is 0, which the C-ABI reads as "the context's own stream")."""
        import torch
        if self._refine_stream is None:
            self._refine_stream = torch.cuda.Stream(torch.device(f"cuda:{self.device}"))
        return self._refine_stream

    def _chain(self, timer=None):
        """What a chain on the side stream opens with -> (torch device, side stream, its handle, timer or a no-op)."""
        import torch
        st = self._side_stream()
        tick = timer if timer is not None else (lambda phase, k: None)
        return torch.device(f"cuda:{self.device}"), st, st.cuda_stream, tick

    def _rows(self, c, nrm, ref, mask):
        """The host arrays of n = len(ref) patches, contiguous -> (n, c, nrm float64 (n,3), ref int32 (n,), mask uint64
        (n,words)); a None nrm stays None.  An array of another length is numpy's ValueError, c's first."""
        ref = _c(ref, np.int32).reshape(-1)
        n = len(ref)
        c = _c(c, np.float64).reshape(n, 3)
        nrm = _c(nrm, np.float64).reshape(n, 3) if nrm is not None else nrm
        return n, c, nrm, ref, _c(mask, np.uint64).reshape(n, self.words)

    def _patch_rows(self, n, c, nrm, ref, mask):
        """_need's rows of n patches on the device, in the order every wrapper checks them; a None is skipped there."""
        return [("c", c, 8, (n, 3)), ("nrm", nrm, 8, (n, 3)), ("ref", ref, 4, (n,)), ("mask", mask, 8, (n, self.words))]

    def _view_range(self, views):
        """(v0, nv) of a view range given as None (every view) or (v0, nv)."""
        v0, nv = (0, self.V) if views is None else (int(views[0]), int(views[1]))
        if v0 < 0 or nv < 1 or v0 + nv > self.V:
            raise RuntimeError("the view range (v0, nv) must lie inside 0..V-1, nv >= 1")
        return v0, nv

    def pack_accepted(self, offset, count, mask, vlb, out, stream=None, c=None):
        """mvs_pack_accepted: the accepted candidates (count >= vlb) of a scored
        slice as exchange rows of out (device int64 tensor (cap + 1, width):
        row 0 = [accepted, n, 0...], then rows
        [offset + i, mask words(, x y z bits with c)]: each 8,192-candidate
        chunk in index order, the chunks in any order -- sort_rows() orders
        them); c = the
        slice's (n, 3) float64 centres or None (width 1 + words [+ 3]);
        stream-ordered, no host sync.  count None: mask is score_device_rec's
        records and |V| their popcount."""
        n = int(count.numel()) if count is not None else int(mask.shape[0])
        # the kernel indexes rows at a fixed pitch: strided views would give wrong rows
        if count is None and (mask.dtype.itemsize != 8 or mask.dim() != 2 or mask.shape[1] != self.words + 1
                              or not mask.is_contiguous()):
            raise RuntimeError("pack_accepted: records must be contiguous int64 (n, words + 1)")
        if count is not None and (count.dtype.itemsize != 4 or not count.is_contiguous()
                                  or mask.dtype.itemsize != 8 or tuple(mask.shape) != (n, self.words)
                                  or not mask.is_contiguous()):
            raise RuntimeError(f"pack_accepted: count must be contiguous int32 (n,) and mask contiguous "
                               f"int64 (n, {self.words})")
        cap = int(out.shape[0]) - 1
        width = 1 + self.words + (3 if c is not None else 0)
        if out.dtype.itemsize != 8 or out.shape[1] != width or not out.is_contiguous():
            raise RuntimeError(f"pack_accepted: out must be contiguous int64 (cap + 1, {width})")
        if c is not None and (c.dtype.itemsize != 8 or tuple(c.shape) != (n, 3) or not c.is_contiguous()):
            raise RuntimeError("pack_accepted: c must be contiguous float64 (n, 3)")
        rc = load().mvs_pack_accepted(self._h, n, int(offset), count.data_ptr() if count is not None else None,
                                      mask.data_ptr(),
                                      c.data_ptr() if c is not None else None,
                                      int(vlb), cap, out.data_ptr(),
                                      stream)
        check(rc, self._h, "mvs_pack_accepted")

    def set_scorer_grid(self, workgroups=0):
        """Hold the persistent scorers to `workgroups` workgroups (0: default,
        two per CU): the grid for a CU-masked scoring stream."""
        check(load().mvs_set_scorer_grid(self._h, int(workgroups)), self._h, "mvs_set_scorer_grid")

    def harris_points(self, view):
        """getHarrisPoints(imgs[view]) (HarrisFeatures.py:135-161) on the GPU:
        int32 (n, 2) [col, row] in np.where's row-major order."""
        lib = load()
        n = ctypes.c_int64(0)
        check(lib.mvs_harris_points(self._h, int(view), None, 0, ctypes.byref(n)), self._h,
              "mvs_harris_points")
        out = np.empty((max(n.value, 1), 2), np.int32)
        check(lib.mvs_harris_points(self._h, int(view), _p(out, _i32p), n.value, ctypes.byref(n)),
              self._h, "mvs_harris_points")
        return out[:n.value]

    def match_two_sided(self, view_a, pts_a, view_b, pts_b, thr=0.5, wid=5):
        """MatchTwoSided over getDescFeatures windows (HarrisFeatures.py:15-67) on the
        GPU; pts_* [row, col] inside getDescFeatures' bounds.
        Returns (m12, best12, best21) int32 (-1 = none)."""
        a = _c(pts_a, np.int32).reshape(-1, 2)
        b = _c(pts_b, np.int32).reshape(-1, 2)
        m12 = np.empty(max(len(a), 1), np.int32)
        b12 = np.empty(max(len(a), 1), np.int32)
        b21 = np.empty(max(len(b), 1), np.int32)
        check(load().mvs_match_two_sided(self._h, int(view_a), _p(a, _i32p), len(a), int(view_b),
                                         _p(b, _i32p), len(b), int(wid), float(thr), _p(m12, _i32p),
                                         _p(b12, _i32p), _p(b21, _i32p)),
              self._h, "mvs_match_two_sided")
        return m12[:len(a)], b12[:len(a)], b21[:len(b)]

    def expand_candidates(self, pc, pn, pxy, job_parent, job_view, job_di, cell_size=2,
                          scale=10.0, wid=5, min_ncc=0.7):
        """patch_expansion candidates (MVS2.py:329-369) for explicit jobs (see mvs_amd.h)."""
        pc = _c(pc, np.float64).reshape(-1, 3)
        pn = _c(pn, np.float64).reshape(-1, 3)
        pxy = _c(pxy, np.float64).reshape(-1, 2)
        jp = _c(job_parent, np.int32)
        jv = _c(job_view, np.int32)
        jd = _c(job_di, np.int32)
        n = len(jp)
        X, nX, xy = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 2))
        color = np.empty((n, 3), np.uint8)
        mask = np.empty((n, self.words), np.uint64)
        count = np.empty(n, np.int32)
        acc = np.empty(n, np.uint8)
        rc = load().mvs_expand_candidates(self._h, len(pc), _p(pc, _dp), _p(pn, _dp), _p(pxy, _dp),
                                          n, _p(jp, _i32p), _p(jv, _i32p), _p(jd, _i32p),
                                          int(cell_size), float(scale), int(wid), float(min_ncc),
                                          _p(X, _dp), _p(nX, _dp), _p(color, _u8p), _p(xy, _dp),
                                          _p(mask, _u64p), _p(count, _i32p), _p(acc, _u8p))
        check(rc, self._h, "mvs_expand_candidates")
        return X, nX, color, xy, mask, count, acc


def proxy_copy(dst, src, nbytes, workgroups, stream=None):
    """Measurement only: copy nbytes between device tensors with a kernel of
    `workgroups` workgroups on `stream` (a collective's CU footprint)."""
    check(load().mvs_proxy_copy(dst.data_ptr(), src.data_ptr(), int(nbytes), int(workgroups), stream),
          None, "mvs_proxy_copy")


def ncc_windows(a, b, thr, force_exact=False, stream=None):
    """ctNcc on device window pairs (torch uint8 tensors (n, npx)); returns (ncc, pass) tensors."""
    import torch
    n, npx = a.shape
    ncc = torch.empty(n, dtype=torch.float64, device=a.device)
    ok = torch.empty(n, dtype=torch.uint8, device=a.device)
    rc = load().mvs_ncc_windows(n, npx, a.data_ptr(), b.data_ptr(), float(thr), int(force_exact),
                                ncc.data_ptr(), ok.data_ptr(), stream)
    check(rc, None, "mvs_ncc_windows")
    return ncc, ok
