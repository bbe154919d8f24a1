"""The visibility-consistency filter of a warped patch set, the expand -> filter loop (csrc/mvs_filter_warp.hip)."""
import numpy as np

from ._abi import _c, _dp, _i32p, _i64p, _p, _u8p, _u64p, check, load
from ._context import _need


class _Wfilt:
    def wfilt_front_device(self, c, ref, mask, cell_size, front, zfront, stream=None):
        """mvs_wfilt_front_device on torch device tensors (contiguous: c float64
        (n,3), ref int32 (n,), mask int64 (n,words), front int32 and zfront
        float64 (V,ncj,nci), both written whole); stream-ordered."""
        n = int(ref.numel())
        nci, ncj = self.cell_grid(cell_size)
        _need("wfilt_front_device", self._patch_rows(n, c, None, ref, mask) + [
            ("front", front, 4, (self.V, ncj, nci)), ("zfront", zfront, 8, (self.V, ncj, nci))])
        rc = load().mvs_wfilt_front_device(self._h, n, c.data_ptr(), ref.data_ptr(), mask.data_ptr(), int(cell_size),
                                           front.data_ptr(), zfront.data_ptr(), stream)
        check(rc, self._h, "mvs_wfilt_front_device")

    def wfilt_test_device(self, c, nrm, ref, mask, avg, cell_size, adj_px, min_views, front, vis, conf, keep,
                          stream=None):
        """mvs_wfilt_test_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), avg float64 (n,),
        front int32 (V,ncj,nci), vis int64 (n,words), conf int64 (n,), keep uint8
        (n,)); stream-ordered."""
        n = int(ref.numel())
        nci, ncj = self.cell_grid(cell_size)
        _need("wfilt_test_device", self._patch_rows(n, c, nrm, ref, mask) + [
            ("avg", avg, 8, (n,)), ("front", front, 4, (self.V, ncj, nci)), ("vis", vis, 8, (n, self.words)),
            ("conf", conf, 8, (n,)), ("keep", keep, 1, (n,))])
        rc = load().mvs_wfilt_test_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                          avg.data_ptr(), int(cell_size), float(adj_px), int(min_views),
                                          front.data_ptr(), vis.data_ptr(), conf.data_ptr(), keep.data_ptr(), stream)
        check(rc, self._h, "mvs_wfilt_test_device")

    def wfilt_front(self, c, ref, mask, cell_size):
        """The front grid of a patch set (mvs_wfilt_front, host pointers): per
        (view, cell) the placed patch of least depth, ties to the lowest index.
        Returns front (V,ncj,nci) int32 (-1 = empty) and zfront float64 (+inf)."""
        nci, ncj = self.cell_grid(cell_size)
        n, c, _, ref, mask = self._rows(c, None, ref, mask)
        front = np.empty((self.V, ncj, nci), np.int32)
        zfront = np.empty((self.V, ncj, nci), np.float64)
        rc = load().mvs_wfilt_front(self._h, n, _p(c, _dp), _p(ref, _i32p), _p(mask, _u64p), int(cell_size),
                                    _p(front, _i32p), _p(zfront, _dp))
        check(rc, self._h, "mvs_wfilt_front")
        return front, zfront

    def wfilt_test(self, c, nrm, ref, mask, avg, cell_size, adj_px, min_views, front):
        """The visibility and conflict test of a patch set against a front grid
        (mvs_wfilt_test, host pointers; a front entry outside -1..n-1 raises).
        Returns vis (n,words) uint64, conf (n,) int64 and keep (n,) uint8."""
        nci, ncj = self.cell_grid(cell_size)
        n, c, nrm, ref, mask = self._rows(c, nrm, ref, mask)
        avg = _c(avg, np.float64).reshape(n)
        front = _c(front, np.int32).reshape(self.V, ncj, nci)
        vis = np.zeros((max(n, 1), self.words), np.uint64)
        conf = np.zeros(max(n, 1), np.int64)
        keep = np.zeros(max(n, 1), np.uint8)
        rc = load().mvs_wfilt_test(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(mask, _u64p),
                                   _p(avg, _dp), int(cell_size), float(adj_px), int(min_views), _p(front, _i32p),
                                   _p(vis, _u64p), _p(conf, _i64p), _p(keep, _u8p))
        check(rc, self._h, "mvs_wfilt_test")
        return vis[:n], conf[:n], keep[:n]

    def wfilt_support_device(self, c, nrm, ref, mask, cell_size, adj_px, min_support, min_neigh, front, nb, adj, keep,
                             stream=None):
        """mvs_wfilt_support_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), front int32
        (V,ncj,nci), nb and adj int32 (n,), keep uint8 (n,)); stream-ordered."""
        n = int(ref.numel())
        nci, ncj = self.cell_grid(cell_size)
        _need("wfilt_support_device", self._patch_rows(n, c, nrm, ref, mask) + [
            ("front", front, 4, (self.V, ncj, nci)), ("nb", nb, 4, (n,)), ("adj", adj, 4, (n,)),
            ("keep", keep, 1, (n,))])
        rc = load().mvs_wfilt_support_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(), mask.data_ptr(),
                                             int(cell_size), float(adj_px), float(min_support), int(min_neigh),
                                             front.data_ptr(), nb.data_ptr(), adj.data_ptr(), keep.data_ptr(), stream)
        check(rc, self._h, "mvs_wfilt_support_device")

    def wfilt_support(self, c, nrm, ref, mask, cell_size, adj_px, min_support, min_neigh, front):
        """The neighbour-support test of a patch set against a front grid
        (mvs_wfilt_support, host pointers; a front entry outside -1..n-1 raises).
        Returns nb (n,) int32, adj (n,) int32 and keep (n,) uint8."""
        nci, ncj = self.cell_grid(cell_size)
        n, c, nrm, ref, mask = self._rows(c, nrm, ref, mask)
        front = _c(front, np.int32).reshape(self.V, ncj, nci)
        nb = np.zeros(max(n, 1), np.int32)
        adj = np.zeros(max(n, 1), np.int32)
        keep = np.zeros(max(n, 1), np.uint8)
        rc = load().mvs_wfilt_support(self._h, n, _p(c, _dp), _p(nrm, _dp), _p(ref, _i32p), _p(mask, _u64p),
                                      int(cell_size), float(adj_px), float(min_support), int(min_neigh),
                                      _p(front, _i32p), _p(nb, _i32p), _p(adj, _i32p), _p(keep, _u8p))
        check(rc, self._h, "mvs_wfilt_support")
        return nb[:n], adj[:n], keep[:n]

    def filter_warped(self, patches, cell_size=2, adj_px=2.0, min_views=3, passes=2, timer=None, min_support=None,
                      min_neigh=1, support_passes=1):
        """Remove the patches of a warped patch set that contradict the
        visibility of the rest (the definition is in include/mvs_amd.h).
        `patches` is the dict expand_warped returns; it needs c, nrm, ref, mask,
        avg and cell.  Each pass builds the front grid of the rows still alive
        (wfilt_front_device), runs the test (wfilt_test_device) and sets the
        removed rows' ref to -1 on the device; nothing is compacted between
        passes.  It stops after `passes` passes or when a pass removes nothing.
        Everything runs on the context's torch side stream; the host reads one
        counter per pass, the survivors.

        min_support not None: after the visibility passes, up to support_passes
        passes of the neighbour-support test (wfilt_support_device with adj_px,
        min_support and min_neigh) in the same way: the front grid of the rows
        still alive, the test, ref = -1 for the removed rows, one counter read;
        they stop when a pass removes nothing.  The dict then also holds nb and
        adj (int32, the last support pass over the input; zeros when none ran)
        and removed_support (per support pass).  The timer's phases of a
        support pass are "sfront", "support" and "ssync".

        Returns a dict of numpy arrays: the surviving rows of every per-patch
        array of the input (parent keeps the input's numbering), index (their
        rows in the input), keep (over the input), vis (words uint64) and conf
        (int64) of the last pass over the input, removed (per pass), front and
        zfront (V,ncj,nci) rebuilt from the survivors, and occ (V,ncj,nci): the
        survivors' cells through wexp_mark_device with the jobs (-1, ref, cell).
        timer: an optional callable timer(phase, pass) called on the chain's
        stream before each phase and with phase "end" after the last."""
        import torch
        for k in ("c", "nrm", "ref", "mask", "avg", "cell"):
            if k not in patches:
                raise RuntimeError(f"filter_warped: patches has no '{k}'")
        ref0 = _c(patches["ref"], np.int32).reshape(-1)
        n = len(ref0)
        V, words = self.V, self.words
        s = int(cell_size)
        nci, ncj = self.cell_grid(s)
        passes = int(passes)
        if passes < 0:
            raise RuntimeError("filter_warped: passes < 0")
        support_passes = int(support_passes) if min_support is not None else 0
        if support_passes < 0:
            raise RuntimeError("filter_warped: support_passes < 0")
        c0 = _c(patches["c"], np.float64).reshape(n, 3)
        n0 = _c(patches["nrm"], np.float64).reshape(n, 3)
        m0 = _c(patches["mask"], np.uint64).reshape(n, words)
        a0 = _c(patches["avg"], np.float64).reshape(n)
        cell0 = _c(patches["cell"], np.int32).reshape(n, 2)
        dev, st, sh, tick = self._chain(timer)
        removed = []
        alive = int(((ref0 >= 0) & (ref0 < V)).sum())
        with torch.cuda.stream(st):
            c, nrm, ref, avg, mask = (self._dev_tensor(x, None, x.shape) for x in (c0, n0, ref0.copy(), a0, m0))
            front = torch.empty((V, ncj, nci), dtype=torch.int32, device=dev)
            zfront = torch.empty((V, ncj, nci), dtype=torch.float64, device=dev)
            vis = torch.zeros((n, words), dtype=torch.int64, device=dev)
            conf = torch.zeros(n, dtype=torch.int64, device=dev)
            keep = torch.empty(n, dtype=torch.uint8, device=dev)
            for k in range(passes):
                tick("front", k)
                self.wfilt_front_device(c, ref, mask, s, front, zfront, stream=sh)
                tick("test", k)
                self.wfilt_test_device(c, nrm, ref, mask, avg, s, adj_px, min_views, front, vis, conf, keep, stream=sh)
                ref.masked_fill_(keep == 0, -1)
                tick("sync", k)
                left = int(keep.sum().item())   # the pass's one read
                removed.append(alive - left)
                alive = left
                if removed[-1] == 0:
                    break
            if min_support is not None:
                removed_support = []
                nb = torch.zeros(n, dtype=torch.int32, device=dev)
                adj = torch.zeros(n, dtype=torch.int32, device=dev)
                if support_passes == 0 or n == 0:   # no pass runs the call: its scalar checks all the same
                    self.wfilt_support_device(c[:0], nrm[:0], ref[:0], mask[:0], s, adj_px, min_support, min_neigh,
                                              front, nb[:0], adj[:0], keep[:0], stream=sh)
                for k in range(support_passes):
                    tick("sfront", k)
                    self.wfilt_front_device(c, ref, mask, s, front, zfront, stream=sh)
                    tick("support", k)
                    self.wfilt_support_device(c, nrm, ref, mask, s, adj_px, min_support, min_neigh, front, nb, adj,
                                              keep, stream=sh)
                    ref.masked_fill_(keep == 0, -1)
                    tick("ssync", k)
                    left = int(keep.sum().item())   # the pass's one read
                    removed_support.append(alive - left)
                    alive = left
                    if removed_support[-1] == 0:
                        break
            tick("rebuild", passes)
            self.wfilt_front_device(c, ref, mask, s, front, zfront, stream=sh)
            tick("occ", passes)
            live = ((ref >= 0) & (ref < V)).to(torch.uint8)
            job = torch.cat([torch.full((n, 1), -1, dtype=torch.int32, device=dev), ref.reshape(n, 1),
                             torch.from_numpy(cell0).to(dev)], 1).contiguous()
            occ = torch.zeros((V, ncj, nci), dtype=torch.uint8, device=dev)
            self.wexp_mark_device(job, live, c, ref, mask, s, occ, stream=sh)
            tick("end", passes)
            h_keep = live.cpu().numpy()
            res = {"keep": h_keep, "vis": vis.cpu().numpy().view(np.uint64), "conf": conf.cpu().numpy(),
                   "front": front.cpu().numpy(), "zfront": zfront.cpu().numpy(), "occ": occ.cpu().numpy()}
            if min_support is not None:
                res.update({"nb": nb.cpu().numpy(), "adj": adj.cpu().numpy(), "removed_support": removed_support})
        st.synchronize()
        index = np.flatnonzero(h_keep).astype(np.int64)
        out = {k: np.asarray(v)[index] for k, v in patches.items()
               if k not in ("occ", "trace") and isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n}
        out.update(res)
        out["index"] = index
        out["removed"] = removed
        return out

    @staticmethod
    def renumber_parents(parent, index, n):
        """The parents of the rows `index` (ascending) of an n-row set in the
        numbering of those rows alone: a removed parent becomes -2, a seed's -1
        and an earlier -2 stay."""
        parent = np.asarray(parent, np.int64)
        new = np.full(n + 1, -2, np.int64)        # the last element serves the negative parents
        new[np.asarray(index, np.int64)] = np.arange(len(index))
        return np.where(parent >= 0, new[np.where(parent >= 0, parent, n)], parent)

    def reconstruct_warped(self, c, nrm, ref, iterations=3, rounds=4, resume_rounds=2, expand=None, filter=None,
                           start=None, timer=None):
        """PMVS's expand -> filter loop on the warped pipeline: expand_warped of
        the seeds (c, nrm, ref) for `rounds` rounds, then `iterations` times
        filter_warped and, unless it was the last filter, resume_warped for
        resume_rounds rounds from the survivors and their occ.  `expand` holds
        the keywords of expand_warped and resume_warped, `filter` those of
        filter_warped; cell_size is shared (give it in `expand`).  After every
        filter the survivors' parent is renumbered through index
        (renumber_parents).  start: an existing set (a dict as resume_warped
        takes it, with max_dist) to loop on in place of the seeds' expansion;
        c, nrm, ref and rounds are then unused.  timer: an optional callable
        timer(stage, iteration, phase, k) that receives the phase marks of every
        stage ("expand", "filter", "resume") as that stage's own timer would.

        Returns the last filter_warped's dict with parent renumbered, max_dist,
        and history: per iteration a dict of patches (the set's size before the
        filter), removed, removed_support and resumed (the size after the
        resumption, None after the last filter)."""
        expand, filt = dict(expand or {}), dict(filter or {})
        for k in ("trace", "timer"):
            if k in expand or k in filt:
                raise RuntimeError(f"reconstruct_warped: '{k}' belongs to the single calls")

        def stage(name, it):   # the stages' phase marks, told apart
            return None if timer is None else (lambda phase, k: timer(name, it, phase, k))

        if filt.setdefault("cell_size", expand.get("cell_size", 2)) != expand.get("cell_size", 2):
            raise RuntimeError("reconstruct_warped: expand and filter disagree on cell_size")
        iterations = int(iterations)
        if iterations < 1:
            raise RuntimeError("reconstruct_warped: iterations < 1")
        ps = start if start is not None else self.expand_warped(c, nrm, ref, rounds, timer=stage("expand", 0),
                                                                **expand)
        grow = dict(expand, max_dist=ps["max_dist"])
        history = []
        for it in range(iterations):
            before = len(ps["ref"])
            ps = self.filter_warped(ps, timer=stage("filter", it), **filt)
            ps["parent"] = self.renumber_parents(ps["parent"], ps["index"], before)
            history.append({"patches": before, "removed": ps["removed"],
                            "removed_support": ps.get("removed_support", []), "resumed": None})
            if it + 1 < iterations:
                ps = self.resume_warped(ps, resume_rounds, timer=stage("resume", it), **grow)
                history[-1]["resumed"] = len(ps["ref"])
        ps["max_dist"] = grow["max_dist"]
        ps["history"] = history
        return ps
