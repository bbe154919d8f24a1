"""The level-synchronous expansion driven by the warped test (csrc/mvs_expand_warp.hip)."""
import math

import numpy as np

from ._abi import _c, _dp, _i32p, _p, _u8p, check, load
from ._context import _need


class _Wexp:
    def wexp_children_device(self, c, nrm, ref, mask, cell_size, occ, max_dist, job, cc, cn, cref, total,
                             stream=None):
        """mvs_wexp_children_device on torch device tensors (contiguous: c, nrm
        float64 (n,3), ref int32 (n,), mask int64 (n,words), occ uint8
        (V,ncj,nci), job int32 (cap,4), cc, cn float64 (cap,3), cref int32
        (cap,), total int64 (1,)); stream-ordered."""
        n, cap = int(ref.numel()), int(cref.numel())
        nci, ncj = self.cell_grid(cell_size)
        _need("wexp_children_device", self._patch_rows(n, c, nrm, ref, mask) + [
            ("occ", occ, 1, (self.V, ncj, nci)), ("job", job, 4, (cap, 4)), ("cc", cc, 8, (cap, 3)),
            ("cn", cn, 8, (cap, 3)), ("cref", cref, 4, (cap,)), ("total", total, 8, (1,))])
        rc = load().mvs_wexp_children_device(self._h, n, c.data_ptr(), nrm.data_ptr(), ref.data_ptr(),
                                             mask.data_ptr(), int(cell_size), occ.data_ptr(), float(max_dist), cap,
                                             job.data_ptr(), cc.data_ptr(), cn.data_ptr(), cref.data_ptr(),
                                             total.data_ptr(), stream)
        check(rc, self._h, "mvs_wexp_children_device")

    def wexp_claim_device(self, job, accept, score, nci, ncj, win, stream=None):
        """mvs_wexp_claim_device on torch device tensors (contiguous: job int32
        (m,4), accept, win uint8 (m,), score float64 (m,)); stream-ordered."""
        m = int(accept.numel())
        _need("wexp_claim_device", [("job", job, 4, (m, 4)), ("accept", accept, 1, (m,)), ("score", score, 8, (m,)),
                                    ("win", win, 1, (m,))])
        rc = load().mvs_wexp_claim_device(self._h, m, job.data_ptr(), accept.data_ptr(), score.data_ptr(), int(nci),
                                          int(ncj), win.data_ptr(), stream)
        check(rc, self._h, "mvs_wexp_claim_device")

    def wexp_mark_device(self, job, win, cc, cref, mask, cell_size, occ, stream=None):
        """mvs_wexp_mark_device on torch device tensors (contiguous: job int32
        (m,4), win uint8 (m,), cc float64 (m,3), cref int32 (m,), mask int64
        (m,words), occ uint8 (V,ncj,nci), updated in place); stream-ordered."""
        m = int(win.numel())
        nci, ncj = self.cell_grid(cell_size)
        _need("wexp_mark_device", [("job", job, 4, (m, 4)), ("win", win, 1, (m,)), ("cc", cc, 8, (m, 3)),
                                   ("cref", cref, 4, (m,)), ("mask", mask, 8, (m, self.words)),
                                   ("occ", occ, 1, (self.V, ncj, nci))])
        rc = load().mvs_wexp_mark_device(self._h, m, job.data_ptr(), win.data_ptr(), cc.data_ptr(), cref.data_ptr(),
                                         mask.data_ptr(), int(cell_size), occ.data_ptr(), stream)
        check(rc, self._h, "mvs_wexp_mark_device")

    def wexp_children(self, c, nrm, ref, mask, cell_size, occ, max_dist, cap=None):
        """Child jobs and geometry of frontier patches (mvs_wexp_children_device)
        from numpy arrays or torch tensors, through torch device tensors: per
        patch and per view of {ref} + mask, the up to four vacant neighbour cells
        of the patch's cell in that view whose centre ray meets the parent's
        tangent plane within max_dist of the parent.  cap None: room for every
        job.  Returns jobs (k,4) int32 [parent, view, cell i, cell j], cc (k,3),
        cn (k,3), cref (k,) and the total found (k = min(total, cap)), as numpy."""
        import torch
        n = int(np.asarray(ref.cpu() if isinstance(ref, torch.Tensor) else ref).size)
        nci, ncj = self.cell_grid(cell_size)
        dev, st, sh, _ = self._chain()
        t_c = self._dev_tensor(c, torch.float64, (n, 3))
        t_n = self._dev_tensor(nrm, torch.float64, (n, 3))
        t_r = self._dev_tensor(ref, torch.int32, (n,))
        t_m = self._dev_tensor(mask, torch.int64, (n, self.words))
        t_o = self._dev_tensor(occ, torch.uint8, (self.V, ncj, nci))
        cap = 4 * self.V * n if cap is None else int(cap)
        job = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        cc = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        cn = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        cref = torch.empty(cap, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # the inputs' copies, before the side stream reads them
        self.wexp_children_device(t_c, t_n, t_r, t_m, cell_size, t_o, max_dist, job, cc, cn, cref, total, stream=sh)
        st.synchronize()
        tot = int(total.item())
        k = min(tot, cap)
        return job[:k].cpu().numpy(), cc[:k].cpu().numpy(), cn[:k].cpu().numpy(), cref[:k].cpu().numpy(), tot

    def wexp_claim(self, jobs, accept, score, nci, ncj):
        """One winner per (view, cell) (mvs_wexp_claim_device) from numpy arrays or
        torch tensors: among the jobs with accept != 0 and a finite score that
        name one cell, the highest score wins, ties to the lowest index.
        Returns win (m,) uint8 as numpy."""
        import torch
        dev, st, sh, _ = self._chain()
        t_a = self._dev_tensor(accept, torch.uint8, (-1,))
        m = int(t_a.numel())
        t_j = self._dev_tensor(jobs, torch.int32, (m, 4))
        t_s = self._dev_tensor(score, torch.float64, (m,))
        win = torch.zeros(m, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.wexp_claim_device(t_j, t_a, t_s, nci, ncj, win, stream=sh)
        st.synchronize()
        return win.cpu().numpy()

    def wexp_claim_checked(self, jobs, accept, score, nci, ncj):
        """The host-pointer claim (mvs_wexp_claim): as wexp_claim on numpy
        arrays, but a job whose (view, cell) lies outside the grid raises."""
        jobs = _c(jobs, np.int32).reshape(-1, 4)
        m = len(jobs)
        accept = _c(accept, np.uint8).reshape(m)
        score = _c(score, np.float64).reshape(m)
        win = np.zeros(max(m, 1), np.uint8)
        rc = load().mvs_wexp_claim(self._h, m, _p(jobs, _i32p), _p(accept, _u8p), _p(score, _dp), int(nci), int(ncj),
                                   _p(win, _u8p))
        check(rc, self._h, "mvs_wexp_claim")
        return win[:m]

    def wexp_mark(self, jobs, win, cc, cref, mask, cell_size, occ):
        """Fill the cells of the winners (mvs_wexp_mark_device) from numpy arrays
        or torch tensors: the job's own cell in its reference view and the cell
        of the centre's projection in every view of its mask.  Returns the new
        occupancy (V, ncj, nci) uint8 as numpy; the input is not modified."""
        import torch
        dev, st, sh, _ = self._chain()
        nci, ncj = self.cell_grid(cell_size)
        t_w = self._dev_tensor(win, torch.uint8, (-1,))
        m = int(t_w.numel())
        t_j = self._dev_tensor(jobs, torch.int32, (m, 4))
        t_c = self._dev_tensor(cc, torch.float64, (m, 3))
        t_r = self._dev_tensor(cref, torch.int32, (m,))
        t_m = self._dev_tensor(mask, torch.int64, (m, self.words))
        t_o = self._dev_tensor(occ, torch.uint8, (self.V, ncj, nci)).clone()
        torch.cuda.current_stream(dev).synchronize()
        self.wexp_mark_device(t_j, t_w, t_c, t_r, t_m, cell_size, t_o, stream=sh)
        st.synchronize()
        return t_o.cpu().numpy()

    def expand_warped(self, c, nrm, ref, rounds, cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2, max_dist=None,
                      refine_levels=0, max_views=8, depth_px=1.0, max_patches=None, trace=False, timer=None):
        """Grow a patch set from seed patches (c, nrm, ref) by `rounds` rounds of a
        level-synchronous expansion driven by the plane-warped photo test:

          round 0: the seeds are the candidates, job (-1, ref, cell of the
            seed's projection into ref); a seed outside the grid is not accepted;
          every round: score_warped_device of the candidates; accept = count >=
            vlb; one winner per (view, cell) by the highest avg (wexp_claim);
            with refine_levels > 0 the winners are refined (refine_lists_device:
            the rule of refine_view_lists and refine_depth_steps(depth_px) on the
            device; refine_levels level calls at step_scale
            2^-level, kd 2, ka 1) and re-scored, and the refined patch replaces
            the winner when its count >= vlb and its avg >= the winner's; the
            winners' cells are filled (wexp_mark) with their final masks; the
            winners join the patch set and are the next frontier;
          later rounds: the candidates are the frontier's children (wexp_children).

        It stops after `rounds` rounds, when a round has no winner, or at
        max_patches (the last round's winners truncated in job order).
        max_dist None: 2 cell_size pixels at the first seed's depth in its
        reference view.  Everything runs on one torch side stream; the host
        reads two counters once per round (the next round's job total and this
        round's winners) and, with refinement, the winners' number once more
        (it sizes their buffers); no array crosses to the host inside a round.

        Returns a dict of numpy arrays over the patch set: c, nrm (P,3), ref
        (P,), mask (P,words) uint64, count, avg, round, parent (index into the
        patch set, -1 for seeds), cell (P,2) and occ (V,ncj,nci), max_dist.  With
        trace=True also "trace": per round a dict of jobs, cc, cn, cref, xy,
        mask, count, avg, ncc (as scored), accept, win, lists (nw, max_views)
        and dstep (nw,) fed to the level calls, kept (winners whose refined
        patch replaced them), refined (c, nrm, count, avg of the
        winners' refined patches, in winner order) and occ after marking.
        timer: an optional callable timer(phase, round) called on the chain's
        stream before each phase and with phase "end" after the last."""
        c = _c(c, np.float64).reshape(-1, 3)
        nrm = _c(nrm, np.float64).reshape(-1, 3)
        ref = _c(ref, np.int32).reshape(-1)
        n0 = len(ref)
        if len(c) != n0 or len(nrm) != n0:
            raise RuntimeError("c, nrm and ref lengths differ")
        if n0 and (ref.min() < 0 or ref.max() >= self.V):
            raise RuntimeError("expand_warped: ref view out of range")
        rounds, refine_levels, vlb = int(rounds), int(refine_levels), int(vlb)
        s = int(cell_size)
        nci, ncj = self.cell_grid(s)
        if refine_levels and not 1 <= int(max_views) <= 32:
            raise RuntimeError("expand_warped: max_views must be in 1..32")
        Rp, K, t = self.rproj(), self._K, self._t
        if max_dist is None and n0:
            max_dist = 2.0 * s * float(self.refine_depth_steps(c[:1], ref[:1], 1.0)[0])
        # round 0 on the host: the seeds' cells (the library's projection, in Python floats)
        jobs0 = np.full((n0, 4), -1, np.int32)
        inside0 = np.zeros(n0, np.uint8)
        for k in range(n0):
            r = int(ref[k])
            jobs0[k, 1] = r
            X, Y, Z = (float(x) for x in c[k])
            R9 = [float(x) for x in Rp[r].reshape(9)]
            x = R9[0] * X + R9[1] * Y + R9[2] * Z + float(t[r, 0])
            y = R9[3] * X + R9[4] * Y + R9[5] * Z + float(t[r, 1])
            z = R9[6] * X + R9[7] * Y + R9[8] * Z + float(t[r, 2])
            w = 1.0 / z if z != 0.0 else 1.0
            x = x * w * float(K[r, 0, 0]) + float(K[r, 0, 2])
            y = y * w * float(K[r, 1, 1]) + float(K[r, 1, 2])
            if z > 0 and 0 <= x < self.W and 0 <= y < self.H and int(x) // s < nci and int(y) // s < ncj:
                jobs0[k, 2:] = (int(x) // s, int(y) // s)
                inside0[k] = 1
        return self._wexp_chain(rounds, (c, nrm, ref, jobs0, inside0), None, s, wid, min_ncc, min_cos, vlb, max_dist,
                                refine_levels, max_views, depth_px, max_patches, trace, timer)

    def _wexp_chain(self, rounds, seeds, start, s, wid, min_ncc, min_cos, vlb, max_dist, refine_levels, max_views,
                    depth_px, max_patches, trace, timer):
        """The rounds of expand_warped (seeds = (c, nrm, ref, jobs, inside) of
        round 0, start None) and of resume_warped (seeds None, start = the host
        arrays of an existing set and its occ or None).  From a set, the
        frontier of every round is the whole current set in row order and the
        first round's children cost one more counter read."""
        import torch
        V, words = self.V, self.words
        nci, ncj = self.cell_grid(s)
        dev, st, sh, tick = self._chain(timer)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        want_ncc = trace or refine_levels > 0
        keys = ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell")
        out = {k: [] for k in keys}
        traces = []
        total, base, r0 = 0, 0, 0
        S = None   # from a set: its c, nrm, ref and mask on the device, every round's winners appended
        with torch.cuda.stream(st):
            counters = torch.zeros(2, **i64)   # [the next round's job total, this round's winners]

            def children(F, cap):
                nb = [torch.empty((cap, 4), **i32), torch.empty((cap, 3), **f64), torch.empty((cap, 3), **f64),
                      torch.empty(cap, **i32)]
                self.wexp_children_device(F[0], F[1], F[2], F[3], s, occ, max_dist, nb[0], nb[1], nb[2], nb[3],
                                          counters[:1], stream=sh)
                return nb

            if start is None:
                c, nrm, ref, jobs0, inside0 = seeds
                occ = torch.zeros((V, ncj, nci), **u8)
                job = torch.from_numpy(jobs0).to(dev)
                cc, cn, cref = (torch.from_numpy(x).to(dev) for x in (c, nrm, ref))
                inside = torch.from_numpy(inside0).to(dev)
                m = len(ref)
            else:
                host, occ0 = start
                for k in keys:
                    out[k].append(self._dev_tensor(host[k], None, host[k].shape))
                S = [out[k][0] for k in ("c", "nrm", "ref", "mask")]
                total = len(host["ref"])
                r0 = int(host["round"].max()) + 1 if total else 0
                if occ0 is not None:
                    occ = torch.from_numpy(occ0).to(dev)
                else:   # the set's cells, as filter_warped marks them
                    occ = torch.zeros((V, ncj, nci), **u8)
                    job = torch.cat([torch.full((total, 1), -1, **i32), S[2].reshape(total, 1), out["cell"][0]],
                                    1).contiguous()
                    self.wexp_mark_device(job, torch.ones(total, **u8), S[0], S[2], S[3], s, occ, stream=sh)
                inside = None
                m = 0
                if rounds > 0 and total and (max_patches is None or total < int(max_patches)):
                    tick("children", r0 - 1)
                    cap = min(4 * V * total, max(1 << 20, 16 * total))
                    nb = children(S, cap)
                    tot = int(counters[0].item())   # the first round's job total
                    if tot > cap:
                        cap = tot
                        nb = children(S, cap)
                    m = min(tot, cap)
                    job, cc, cn, cref = (x[:m].contiguous() for x in nb)
            for rnd in range(r0, r0 + rounds):
                if m == 0:
                    break
                tick("score", rnd)
                xy = torch.empty((m, 2), **f64)
                mask = torch.empty((m, words), **i64)
                count = torch.empty(m, **i32)
                avg = torch.empty(m, **f64)
                ncc = torch.empty((m, V), **f64) if want_ncc else None
                self.score_warped_device(cc, cn, cref, xy, mask, count, avg, ncc, min_ncc, wid, min_cos, stream=sh)
                tick("claim", rnd)
                accept = (count >= vlb).to(torch.uint8)
                if inside is not None:
                    accept = accept * inside
                win = torch.empty(m, **u8)
                self.wexp_claim_device(job, accept, avg, nci, ncj, win, stream=sh)
                if max_patches is not None:
                    room = max(int(max_patches) - total, 0)
                    win = win * (torch.cumsum(win.to(torch.int64), 0) <= room).to(torch.uint8)
                tr = None
                if trace:
                    tr = {"jobs": job, "cc": cc.clone(), "cn": cn.clone(), "cref": cref, "xy": xy, "mask": mask.clone(),
                          "count": count.clone(), "avg": avg.clone(), "ncc": ncc, "accept": accept, "win": win}
                if refine_levels > 0:
                    tick("refine", rnd)
                    # the winners' view lists and depth steps, from the round's ncc on the device
                    idx = torch.nonzero(win).reshape(-1)   # sizes the winners' buffers: the phase's one read
                    nw = int(idx.numel())
                    if nw:
                        wc, wn, wr_ = cc[idx].contiguous(), cn[idx].contiguous(), cref[idx].contiguous()
                        t_lists, t_dstep = torch.empty((nw, int(max_views)), **i32), torch.empty(nw, **f64)
                        self.refine_lists_device(ncc, cc, cref, t_lists, t_dstep, idx, min_ncc, int(max_views),
                                                 depth_px, stream=sh)
                        cur, nxt = [wc, wn], [torch.empty((nw, 3), **f64), torch.empty((nw, 3), **f64)]
                        best, sbest = torch.empty(nw, **i32), torch.empty(nw, **f64)
                        for lev in range(refine_levels):
                            self.refine_warped_level_device(cur[0], cur[1], wr_, t_lists, t_dstep, nxt[0], nxt[1],
                                                            best, sbest, None, wid, min_cos, 2, 1, math.radians(8),
                                                            2.0 ** -lev, stream=sh)
                            cur, nxt = nxt, cur
                        xy2 = torch.empty((nw, 2), **f64)
                        mask2 = torch.empty((nw, words), **i64)
                        count2 = torch.empty(nw, **i32)
                        avg2 = torch.empty(nw, **f64)
                        self.score_warped_device(cur[0], cur[1], wr_, xy2, mask2, count2, avg2, None, min_ncc, wid,
                                                 min_cos, stream=sh)
                        kept = (count2 >= vlb) & (avg2 >= avg[idx])
                        ki = idx[kept]
                        cc[ki], cn[ki] = cur[0][kept], cur[1][kept]
                        mask[ki], count[ki], avg[ki] = mask2[kept], count2[kept], avg2[kept]
                        if trace:
                            tr["lists"], tr["dstep"] = t_lists, t_dstep
                            tr["kept"] = kept.to(torch.uint8)
                            tr["refined"] = {"c": cur[0], "nrm": cur[1], "count": count2, "avg": avg2}
                tick("mark", rnd)
                self.wexp_mark_device(job, win, cc, cref, mask, s, occ, stream=sh)
                if trace:
                    tr["occ"] = occ.clone()
                    traces.append(tr)
                # the next round's children from every job: a job that did not win gets
                # no view (ref -1, empty mask), so the order is the winners' order
                last = rnd + 1 >= r0 + rounds
                winb = win.bool()
                counters[1] = win.sum()
                if not last:
                    tick("children", rnd)
                    f_ref = torch.where(winb, cref, torch.full_like(cref, -1))
                    f_mask = mask * winb.to(torch.int64)[:, None]
                    F = [cc, cn, f_ref, f_mask]
                    if S is not None:   # the whole set first, then this round's jobs
                        F = [torch.cat([x, y]) for x, y in zip(S, F)]
                    nf = int(F[2].numel())
                    cap = min(4 * V * nf, max(1 << 20, 16 * nf))
                    nb = children(F, cap)
                tick("sync", rnd)
                tot, nw = (int(x) for x in counters.cpu())   # the round's one read
                if not last and tot > cap and nw and (max_patches is None or total + nw < max_patches):
                    # more jobs than the first guess holds: the same call again with room for all
                    cap = tot
                    nb = children(F, cap)
                tick("append", rnd)
                if nw == 0:
                    break
                rank = torch.cumsum(win.to(torch.int64), 0) - 1   # a job's index among the round's winners
                out["c"].append(cc[winb]); out["nrm"].append(cn[winb]); out["ref"].append(cref[winb])
                out["mask"].append(mask[winb]); out["count"].append(count[winb]); out["avg"].append(avg[winb])
                out["round"].append(torch.full((nw,), rnd, **i32))
                par = job[winb, 0].to(torch.int64)
                # from a set the parent already is a row of the set (the remapping below)
                out["parent"].append(torch.where(par >= 0, par + base, par) if S is None else par)
                out["cell"].append(job[winb, 2:])
                base, total = total, total + nw
                if last or (max_patches is not None and total >= int(max_patches)):
                    break
                m = min(tot, cap)
                job, cc, cn, cref = (x[:m].contiguous() for x in nb)
                j0 = job[:, 0].long()
                if S is None:
                    job[:, 0] = rank[j0].to(torch.int32)   # parent: job index -> index among the winners
                else:
                    # parent: a row of the set as it is, a job index -> the winner's row behind the set
                    job[:, 0] = torch.where(j0 < base, j0, base + rank[(j0 - base).clamp(min=0)]).to(torch.int32)
                    S = [torch.cat([x, out[k][-1]]) for x, k in zip(S, ("c", "nrm", "ref", "mask"))]
                inside = None
            tick("end", r0 + rounds)
            empty = {"c": torch.empty((0, 3), **f64), "nrm": torch.empty((0, 3), **f64), "ref": torch.empty(0, **i32),
                     "mask": torch.empty((0, words), **i64), "count": torch.empty(0, **i32),
                     "avg": torch.empty(0, **f64), "round": torch.empty(0, **i32), "parent": torch.empty(0, **i64),
                     "cell": torch.empty((0, 2), **i32)}
            res = {k: (torch.cat(v) if v else empty[k]).cpu().numpy() for k, v in out.items()}
            res["mask"] = res["mask"].view(np.uint64)
            res["occ"] = occ.cpu().numpy()
            res["max_dist"] = max_dist
            if trace:
                def host(x):
                    if isinstance(x, dict):
                        return {k: host(v) for k, v in x.items()}
                    x = x.cpu().numpy()
                    return x.view(np.uint64) if x.dtype == np.int64 and x.ndim == 2 and x.shape[1] == words else x
                res["trace"] = [host(tr) for tr in traces]
        st.synchronize()
        return res

    def resume_warped(self, patches, rounds, cell_size=2, wid=5, min_ncc=0.7, min_cos=0.3, vlb=2, max_dist=None,
                      refine_levels=0, max_views=8, depth_px=1.0, max_patches=None, trace=False, timer=None):
        """Grow an existing patch set by `rounds` more rounds of expand_warped's
        expansion.  `patches` is a dict as expand_warped or filter_warped
        returns it; it needs c, nrm, ref, mask, count, avg, round, parent and
        cell.  Every row must be alive (ref in 0..V-1) and every cell inside the
        grid of cell_size.  occ is patches["occ"] when that has the shape
        (V,ncj,nci); otherwise it is rebuilt from the rows (wexp_mark_device
        with the jobs (-1, ref, cell), as filter_warped does).  max_dist: the
        argument, else patches["max_dist"], else expand_warped's rule on the
        first row.

        No row of the input is scored again.  The frontier of every round is
        the whole current set in row order, the input first; its children
        (wexp_children_device) are the round's candidates, and the round is an
        expand_warped round from there: score, accept, claim, optional
        refinement, mark.  An older patch's vacant neighbours are the candidates
        that failed before; they fail again and compete for nothing, so
        resuming k rounds from the set of R rounds gives the set of R + k
        rounds.  The host reads the same two counters once per round, and the
        first round's job total once more.  It stops after `rounds` rounds, at
        a round with no job or no winner, or at max_patches, which counts the
        input.

        Returns expand_warped's dict: the input rows unchanged, then the new
        rows (parent indexes the returned set, round continues from the
        input's highest + 1), occ and max_dist.  rounds = 0 returns the input
        with its occ."""
        keys = ("c", "nrm", "ref", "mask", "count", "avg", "round", "parent", "cell")
        for k in keys:
            if k not in patches:
                raise RuntimeError(f"resume_warped: patches has no '{k}'")
        rounds, refine_levels, vlb = int(rounds), int(refine_levels), int(vlb)
        if rounds < 0:
            raise RuntimeError("resume_warped: rounds < 0")
        if refine_levels and not 1 <= int(max_views) <= 32:
            raise RuntimeError("resume_warped: max_views must be in 1..32")
        s = int(cell_size)
        nci, ncj = self.cell_grid(s)
        ref = _c(patches["ref"], np.int32).reshape(-1)
        n = len(ref)
        host = {"c": _c(patches["c"], np.float64).reshape(n, 3), "nrm": _c(patches["nrm"], np.float64).reshape(n, 3),
                "ref": ref, "mask": _c(patches["mask"], np.uint64).reshape(n, self.words),
                "count": _c(patches["count"], np.int32).reshape(n), "avg": _c(patches["avg"], np.float64).reshape(n),
                "round": _c(patches["round"], np.int32).reshape(n),
                "parent": _c(patches["parent"], np.int64).reshape(n),
                "cell": _c(patches["cell"], np.int32).reshape(n, 2)}
        if n and (ref.min() < 0 or ref.max() >= self.V):
            raise RuntimeError("resume_warped: a row is dead (ref outside 0..V-1)")
        cell = host["cell"]
        if n and (cell.min() < 0 or cell[:, 0].max() >= nci or cell[:, 1].max() >= ncj):
            raise RuntimeError("resume_warped: a cell lies outside the grid")
        occ = patches.get("occ")
        if occ is not None:
            occ = np.asarray(occ)
            occ = _c(occ, np.uint8) if occ.shape == (self.V, ncj, nci) else None
        if max_dist is None:
            max_dist = patches.get("max_dist")
        if max_dist is None and n:
            max_dist = 2.0 * s * float(self.refine_depth_steps(host["c"][:1], ref[:1], 1.0)[0])
        return self._wexp_chain(rounds, None, (host, occ), s, wid, min_ncc, min_cos, vlb, max_dist, refine_levels,
                                max_views, depth_px, max_patches, trace, timer)
