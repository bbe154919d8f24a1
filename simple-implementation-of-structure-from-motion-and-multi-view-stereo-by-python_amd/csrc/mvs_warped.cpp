// The warped family's C-ABI of libmvs_amd.so: the plane-warped photo test,
// the refinement level and its view lists, the warped expansion's primitives,
// the visibility-consistency filter, the neighbour-support test, the seeds and
// colours, the depth maps, and the propagation sweep on them.
#include <cmath>

#include "mvs_host.h"

// The checks every family repeats, each under the family's own name `who`
// (0, or the error's code with the message recorded).
static int bad_arg(mvs_ctx* ctx, const char* who, const std::string& what) {
    return set_err(ctx, Fail{MVS_E_ARG, std::string(who) + ": " + what});
}
static int need_nonneg(mvs_ctx* ctx, const char* who, const char* name, int64_t v) {
    return v < 0 ? bad_arg(ctx, who, std::string(name) + " < 0") : 0;
}
// a row count: 2^31 itself passes here (the filter family refuses it, in wfilt_check)
static int need_count(mvs_ctx* ctx, const char* who, const char* name, int64_t n) {
    if (int rc = need_nonneg(ctx, who, name, n)) return rc;
    return n > ((int64_t)1 << 31) ? bad_arg(ctx, who, std::string(name) + " above 2^31") : 0;
}
static int need_wid(mvs_ctx* ctx, const char* who, int wid) {
    return wid < 1 || wid > MVS_MAX_WID ? bad_arg(ctx, who, "wid must be in 1..5") : 0;
}
static int need_min_cos(mvs_ctx* ctx, const char* who, double min_cos) {
    return !(min_cos >= 0.0 && min_cos < 1.0) ? bad_arg(ctx, who, "min_cos must be in [0, 1)") : 0;
}
static int need_cell_size(mvs_ctx* ctx, const char* who, int cell_size) {
    return cell_size < 1 || cell_size > 16 ? bad_arg(ctx, who, "cell_size must be in 1..16") : 0;
}

extern "C" {

// argument checks shared by the two entry points of the plane-warped test
static int warp_check(mvs_ctx* ctx, int64_t n, bool ptrs_ok, int wid, double min_cos) {
    if (int rc = need_count(ctx, "mvs_score_warped", "n", n)) return rc;
    if (int rc = need_wid(ctx, "mvs_score_warped", wid)) return rc;
    if (int rc = need_min_cos(ctx, "mvs_score_warped", min_cos)) return rc;
    if (n > 0 && !ptrs_ok) return set_err(ctx, Fail{MVS_E_ARG, "mvs_score_warped: null pointer (only avg and ncc may be NULL)"});
    return 0;
}

static void warp_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                        int wid, double min_ncc, double min_cos, double* d_xy, uint64_t* d_mask, int32_t* d_count,
                        double* d_avg, double* d_ncc, hipStream_t s) {
    WarpArgs a{};
    a.n = n;
    a.c = d_c;
    a.nrm = d_nrm;
    a.ref = d_ref;
    a.min_ncc = min_ncc;
    a.min_cos = min_cos;
    a.xy = d_xy;
    a.mask = d_mask;
    a.count = d_count;
    a.avg = d_avg;
    a.ncc = d_ncc;
    if (mvs_launch_score_warp(&ctx->sc, &a, wid, s) != 0) throw Fail{MVS_E_HIP, "score_warp launch failed"};
}

int mvs_score_warped_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                            int wid, double min_ncc, double min_cos, double* d_xy, uint64_t* d_mask,
                            int32_t* d_count, double* d_avg, double* d_ncc, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = warp_check(ctx, n, d_c && d_nrm && d_ref && d_xy && d_mask && d_count, wid, min_cos)) return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        warp_launch(ctx, n, d_c, d_nrm, d_ref, wid, min_ncc, min_cos, d_xy, d_mask, d_count, d_avg, d_ncc, s);
        return 0;
    });
}

int mvs_score_warped(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref, int wid,
                     double min_ncc, double min_cos, double* xy, uint64_t* mask, int32_t* count, double* avg,
                     double* ncc) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = warp_check(ctx, n, c && nrm && ref && xy && mask && count, wid, min_cos)) return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        for (int64_t i = 0; i < n; ++i)
            if (ref[i] < 0 || ref[i] >= ctx->V) throw Fail{MVS_E_ARG, "mvs_score_warped: ref view out of range"};
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_nrm = st.in(nrm, n * 3);
        const auto d_ref = st.in(ref, n);
        const auto d_xy = st.out(xy, n * 2);
        const auto d_mask = st.out(mask, n * ctx->words());
        const auto d_count = st.out(count, n);
        const auto d_avg = st.out(avg, n);
        const auto d_ncc = st.out(ncc, n * ctx->V);
        st.upload();
        warp_launch(ctx, n, d_c, d_nrm, d_ref, wid, min_ncc, min_cos, d_xy, d_mask, d_count, d_avg, d_ncc, s);
        st.finish();
        return 0;
    });
}

// argument checks shared by the two entry points of the refinement level
static int refine_check(mvs_ctx* ctx, int64_t n, bool ptrs_ok, int tv, int wid, double min_cos, int kd, int ka,
                        double astep, double step_scale) {
    if (int rc = need_count(ctx, "mvs_refine_warped", "n", n)) return rc;
    if (int rc = need_wid(ctx, "mvs_refine_warped", wid)) return rc;
    if (int rc = need_min_cos(ctx, "mvs_refine_warped", min_cos)) return rc;
    if (tv < 1 || tv > 32) return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_warped: tv must be in 1..32"});
    if (kd < 0 || kd > 3) return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_warped: kd must be in 0..3"});
    if (ka < 0 || ka > 2) return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_warped: ka must be in 0..2"});
    if (!(step_scale > 0.0) || !std::isfinite(step_scale))
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_warped: step_scale must be > 0"});
    if (!(astep >= 0.0) || !((double)ka * astep * step_scale <= 1.2))
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_warped: ka * astep * step_scale must be in [0, 1.2]"});
    if (n > 0 && !ptrs_ok)
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_warped: null pointer (only scores may be NULL)"});
    return 0;
}

static void refine_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                          const int32_t* d_views, int tv, const double* d_dstep, int wid, double min_cos, int kd,
                          int ka, double astep, double step_scale, double* d_c_out, double* d_nrm_out,
                          int32_t* d_best, double* d_score_best, double* d_scores, hipStream_t s) {
    RefineArgs a{};
    a.n = n;
    a.c = d_c;
    a.nrm = d_nrm;
    a.ref = d_ref;
    a.views = d_views;
    a.dstep = d_dstep;
    a.tv = tv;
    a.kd = kd;
    a.ka = ka;
    a.min_cos = min_cos;
    a.step_scale = step_scale;
    // the grid's tangents from the host's libm (what a caller's own tan() gives)
    const double alpha = astep * step_scale;
    for (int i = -ka; i <= ka; ++i) a.tans[i + ka] = std::tan((double)i * alpha);
    a.c_out = d_c_out;
    a.nrm_out = d_nrm_out;
    a.best = d_best;
    a.score_best = d_score_best;
    a.scores = d_scores;
    if (mvs_launch_refine_warp(&ctx->sc, &a, wid, s) != 0) throw Fail{MVS_E_HIP, "refine_warp launch failed"};
}

int mvs_refine_warped_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                             const int32_t* d_views, int tv, const double* d_dstep, int wid, double min_cos, int kd,
                             int ka, double astep, double step_scale, double* d_c_out, double* d_nrm_out,
                             int32_t* d_best, double* d_score_best, double* d_scores, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = refine_check(ctx, n, d_c && d_nrm && d_ref && d_views && d_dstep && d_c_out && d_nrm_out && d_best &&
                                          d_score_best, tv, wid, min_cos, kd, ka, astep, step_scale))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        refine_launch(ctx, n, d_c, d_nrm, d_ref, d_views, tv, d_dstep, wid, min_cos, kd, ka, astep, step_scale,
                      d_c_out, d_nrm_out, d_best, d_score_best, d_scores, s);
        return 0;
    });
}

int mvs_refine_warped(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                      const int32_t* views, int tv, const double* dstep, int wid, double min_cos, int kd, int ka,
                      double astep, double step_scale, double* c_out, double* nrm_out, int32_t* best,
                      double* score_best, double* scores) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = refine_check(ctx, n, c && nrm && ref && views && dstep && c_out && nrm_out && best && score_best,
                              tv, wid, min_cos, kd, ka, astep, step_scale))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        const int V = ctx->V;
        for (int64_t i = 0; i < n; ++i) {
            if (ref[i] < 0 || ref[i] >= V) throw Fail{MVS_E_ARG, "mvs_refine_warped: ref view out of range"};
            const int32_t* l = views + i * tv;
            bool ended = false;
            for (int j = 0; j < tv; ++j) {
                if (l[j] < -1 || l[j] >= V) throw Fail{MVS_E_ARG, "mvs_refine_warped: list view out of range"};
                if (l[j] < 0) { ended = true; continue; }
                if (ended) throw Fail{MVS_E_ARG, "mvs_refine_warped: list view after a -1"};
                if (l[j] == ref[i]) throw Fail{MVS_E_ARG, "mvs_refine_warped: list view equal to ref"};
                for (int k = 0; k < j; ++k)
                    if (l[k] == l[j]) throw Fail{MVS_E_ARG, "mvs_refine_warped: list view repeated"};
            }
        }
        hipStream_t s = ctx->stream;
        const int A = 2 * ka + 1;
        const int64_t H = (int64_t)(2 * kd + 1) * A * A;
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_nrm = st.in(nrm, n * 3);
        const auto d_dstep = st.in(dstep, n);
        const auto d_ref = st.in(ref, n);
        const auto d_views = st.in(views, n * tv);
        const auto d_co = st.out(c_out, n * 3);
        const auto d_no = st.out(nrm_out, n * 3);
        const auto d_sb = st.out(score_best, n);
        const auto d_best = st.out(best, n);
        const auto d_scores = st.out(scores, n * H);
        st.upload();
        refine_launch(ctx, n, d_c, d_nrm, d_ref, d_views, tv, d_dstep, wid, min_cos, kd, ka, astep, step_scale, d_co,
                      d_no, d_best, d_sb, d_scores, s);
        st.finish();
        return 0;
    });
}

// argument checks shared by the two entry points of the list builder
static int lists_check(mvs_ctx* ctx, int64_t n, int64_t rows, bool has_sel, bool ptrs_ok, double min_ncc,
                       int max_views, double depth_px) {
    if (int rc = need_nonneg(ctx, "mvs_refine_lists", "n", n)) return rc;
    if (int rc = need_nonneg(ctx, "mvs_refine_lists", "rows", rows)) return rc;
    if (n > ((int64_t)1 << 31) || rows > ((int64_t)1 << 31))
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_lists: n or rows above 2^31"});
    if (max_views < 1 || max_views > 32)
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_lists: max_views must be in 1..32"});
    if (std::isnan(min_ncc)) return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_lists: min_ncc is nan"});
    if (!std::isfinite(depth_px) || !(depth_px > 0.0))
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_lists: depth_px must be finite and > 0"});
    if (!has_sel && n > rows) return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_lists: n > rows without sel"});
    if (n > 0 && !ptrs_ok)
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_refine_lists: null pointer (only sel and dstep, and c and ref "
                                            "without dstep, may be NULL)"});
    return 0;
}

static void lists_launch(mvs_ctx* ctx, int64_t n, int64_t rows, const int64_t* d_sel, const double* d_ncc,
                         const double* d_c, const int32_t* d_ref, double min_ncc, int max_views, double depth_px,
                         int32_t* d_views, double* d_dstep, hipStream_t s) {
    ListArgs a{};
    a.n = n;
    a.rows = rows;
    a.sel = d_sel;
    a.ncc = d_ncc;
    a.c = d_c;
    a.ref = d_ref;
    a.min_ncc = min_ncc;
    a.depth_px = depth_px;
    a.max_views = max_views;
    a.views = d_views;
    a.dstep = d_dstep;
    if (mvs_launch_refine_lists(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "refine_lists launch failed"};
}

int mvs_refine_lists_device(mvs_ctx* ctx, int64_t n, int64_t rows, const int64_t* d_sel, const double* d_ncc,
                            const double* d_c, const int32_t* d_ref, double min_ncc, int max_views, double depth_px,
                            int32_t* d_views, double* d_dstep, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = lists_check(ctx, n, rows, d_sel != nullptr, d_ncc && d_views && (!d_dstep || (d_c && d_ref)),
                             min_ncc, max_views, depth_px))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        lists_launch(ctx, n, rows, d_sel, d_ncc, d_c, d_ref, min_ncc, max_views, depth_px, d_views, d_dstep, s);
        return 0;
    });
}

int mvs_refine_lists(mvs_ctx* ctx, int64_t n, int64_t rows, const int64_t* sel, const double* ncc, const double* c,
                     const int32_t* ref, double min_ncc, int max_views, double depth_px, int32_t* views,
                     double* dstep) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = lists_check(ctx, n, rows, sel != nullptr, ncc && views && (!dstep || (c && ref)), min_ncc,
                             max_views, depth_px))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        const int V = ctx->V;
        for (int64_t k = 0; sel && k < n; ++k)
            if (sel[k] < 0 || sel[k] >= rows) throw Fail{MVS_E_ARG, "mvs_refine_lists: sel row out of range"};
        for (int64_t k = 0; dstep && k < n; ++k) {
            const int32_t r = ref[sel ? sel[k] : k];
            if (r < 0 || r >= V) throw Fail{MVS_E_ARG, "mvs_refine_lists: ref view out of range"};
        }
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_ncc = st.in(ncc, rows * V);
        // c and ref are read for dstep alone: not copied without it
        const auto d_c = st.in(dstep ? c : nullptr, rows * 3);
        const auto d_ref = st.in(dstep ? ref : nullptr, rows);
        const auto d_sel = st.in(sel, n);
        const auto d_views = st.out(views, n * max_views);
        const auto d_dstep = st.out(dstep, n);
        st.upload();
        lists_launch(ctx, n, rows, sel ? (int64_t*)d_sel : nullptr, d_ncc, d_c, d_ref, min_ncc, max_views, depth_px,
                     d_views, d_dstep, s);
        st.finish();
        return 0;
    });
}

// ---- the warped expansion's primitives (mvs_expand_warp.hip) ----

int mvs_wexp_children_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                             const uint64_t* d_mask, int cell_size, const uint8_t* d_occ, double max_dist,
                             int64_t cap, int32_t* d_job, double* d_cc, double* d_cn, int32_t* d_cref,
                             int64_t* d_total, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = need_count(ctx, "mvs_wexp_children", "n", n)) return rc;
    if (int rc = need_cell_size(ctx, "mvs_wexp_children", cell_size)) return rc;
    if (!(max_dist > 0.0)) return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_children: max_dist must be > 0"});
    if (int rc = need_nonneg(ctx, "mvs_wexp_children", "cap", cap)) return rc;
    if (n == 0) return MVS_OK;
    if (!d_c || !d_nrm || !d_ref || !d_mask || !d_occ || !d_total ||
        (cap > 0 && (!d_job || !d_cc || !d_cn || !d_cref)))
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_children: null pointer (the outputs may be NULL when cap is 0)"});
    if ((uintptr_t)d_job % 16) return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_children: d_job must be 16-B aligned"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        ctx->wexp_order.acquire(s);
        ctx->x_cnt.ensure(n);
        ctx->x_offs.ensure(n + 1);
        WexpArgs a{};
        a.n = n;
        a.c = d_c;
        a.nrm = d_nrm;
        a.ref = d_ref;
        a.mask = d_mask;
        a.cell_size = cell_size;
        a.occ = d_occ;
        a.max_dist = max_dist;
        a.cap = cap;
        a.cnt = ctx->x_cnt.p;
        a.offs = ctx->x_offs.p;
        a.job = (int4*)d_job;
        a.cc = d_cc;
        a.cn = d_cn;
        a.cref = d_cref;
        a.total = d_total;
        if (mvs_launch_wexp_children(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wexp_children launch failed"};
        ctx->wexp_order.release(s);
        return 0;
    });
}

static int claim_check(mvs_ctx* ctx, int64_t m, bool ptrs_ok, int nci, int ncj) {
    if (int rc = need_count(ctx, "mvs_wexp_claim", "m", m)) return rc;
    if (nci < 1 || ncj < 1 || nci > 65536 || ncj > 65536)
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_claim: nci and ncj must be in 1..65536"});
    if (m > 0 && !ptrs_ok) return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_claim: null pointer"});
    return 0;
}

// the claim on device pointers; the caller holds wexp_order
static void claim_launch(mvs_ctx* ctx, int64_t m, const int32_t* d_job, const uint8_t* d_accept,
                         const double* d_score, int nci, int ncj, uint8_t* d_win, hipStream_t s) {
    const size_t cells = (size_t)ctx->V * nci * ncj;
    if (cells > ctx->x_key.n || cells > ctx->x_ticket.n) {
        // new grids start clean; every call leaves them clean (hipFree of the old ones waits for their users)
        ctx->x_key.alloc(cells);
        ctx->x_ticket.alloc(cells);
        HIPCHK(hipMemsetAsync(ctx->x_key.p, 0, ctx->x_key.n * sizeof(uint64_t), s));
        HIPCHK(hipMemsetAsync(ctx->x_ticket.p, 0, ctx->x_ticket.n * sizeof(uint32_t), s));
    }
    ClaimArgs a{};
    a.m = m;
    a.job = (const int4*)d_job;
    a.accept = d_accept;
    a.score = d_score;
    a.V = ctx->V;
    a.nci = nci;
    a.ncj = ncj;
    a.key = ctx->x_key.p;
    a.ticket = ctx->x_ticket.p;
    a.win = d_win;
    if (mvs_launch_wexp_claim(&a, s) != 0) throw Fail{MVS_E_HIP, "wexp_claim launch failed"};
}

int mvs_wexp_claim_device(mvs_ctx* ctx, int64_t m, const int32_t* d_job, const uint8_t* d_accept,
                          const double* d_score, int nci, int ncj, uint8_t* d_win, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = claim_check(ctx, m, d_job && d_accept && d_score && d_win, nci, ncj)) return rc;
    if (m == 0) return MVS_OK;
    if ((uintptr_t)d_job % 16) return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_claim: d_job must be 16-B aligned"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        ctx->wexp_order.acquire(s);
        claim_launch(ctx, m, d_job, d_accept, d_score, nci, ncj, d_win, s);
        ctx->wexp_order.release(s);
        return 0;
    });
}

int mvs_wexp_claim(mvs_ctx* ctx, int64_t m, const int32_t* job, const uint8_t* accept, const double* score, int nci,
                   int ncj, uint8_t* win) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = claim_check(ctx, m, job && accept && score && win, nci, ncj)) return rc;
    if (m == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        for (int64_t k = 0; k < m; ++k) {
            const int32_t* j = job + 4 * k;
            if (j[1] < 0 || j[1] >= ctx->V || j[2] < 0 || j[2] >= nci || j[3] < 0 || j[3] >= ncj)
                throw Fail{MVS_E_ARG, "mvs_wexp_claim: job (view, cell) outside the grid"};
        }
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_job = st.in(job, 4 * m);
        const auto d_accept = st.in(accept, m);
        const auto d_score = st.in(score, m);
        const auto d_win = st.out(win, m);
        ctx->wexp_order.acquire(s);
        st.upload();
        claim_launch(ctx, m, d_job, d_accept, d_score, nci, ncj, d_win, s);
        ctx->wexp_order.release(s);
        st.finish();
        return 0;
    });
}

int mvs_wexp_mark_device(mvs_ctx* ctx, int64_t m, const int32_t* d_job, const uint8_t* d_win, const double* d_cc,
                         const int32_t* d_cref, const uint64_t* d_mask, int cell_size, uint8_t* d_occ,
                         void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = need_count(ctx, "mvs_wexp_mark", "m", m)) return rc;
    if (int rc = need_cell_size(ctx, "mvs_wexp_mark", cell_size)) return rc;
    if (m == 0) return MVS_OK;
    if (!d_job || !d_win || !d_cc || !d_cref || !d_mask || !d_occ)
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_mark: null pointer"});
    if ((uintptr_t)d_job % 16) return set_err(ctx, Fail{MVS_E_ARG, "mvs_wexp_mark: d_job must be 16-B aligned"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        MarkArgs a{};
        a.m = m;
        a.job = (const int4*)d_job;
        a.win = d_win;
        a.cc = d_cc;
        a.cref = d_cref;
        a.mask = d_mask;
        a.cell_size = cell_size;
        a.occ = d_occ;
        if (mvs_launch_wexp_mark(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wexp_mark launch failed"};
        return 0;
    });
}

// ---- the visibility-consistency filter (mvs_filter_warp.hip) ----

static int wfilt_check(mvs_ctx* ctx, const char* who, int64_t n, int cell_size, double adj_px, int min_views,
                       bool grids_ok, bool rows_ok) {
    if (int rc = need_nonneg(ctx, who, "n", n)) return rc;
    if (n >= ((int64_t)1 << 31)) return bad_arg(ctx, who, "n must be below 2^31");
    if (int rc = need_cell_size(ctx, who, cell_size)) return rc;
    if (!(adj_px >= 0.0 && adj_px < HUGE_VAL)) return bad_arg(ctx, who, "adj_px must be finite and >= 0");
    if (int rc = need_nonneg(ctx, who, "min_views", min_views)) return rc;
    if (!grids_ok || (n > 0 && !rows_ok)) return bad_arg(ctx, who, "null pointer");
    return 0;
}

static void wfilt_front_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref,
                               const uint64_t* d_mask, int cell_size, int32_t* d_front, double* d_zfront,
                               hipStream_t s) {
    WfiltArgs a{};
    a.n = n;
    a.c = d_c;
    a.ref = d_ref;
    a.mask = d_mask;
    a.cell_size = cell_size;
    a.front = d_front;
    a.zfront = (uint64_t*)d_zfront;
    if (mvs_launch_wfilt_front(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wfilt_front launch failed"};
}

static void wfilt_test_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                              const uint64_t* d_mask, const double* d_avg, int cell_size, double adj_px,
                              int min_views, const int32_t* d_front, uint64_t* d_vis, int64_t* d_conf,
                              uint8_t* d_keep, hipStream_t s) {
    WfiltArgs a{};
    a.n = n;
    a.c = d_c;
    a.nrm = d_nrm;
    a.ref = d_ref;
    a.mask = d_mask;
    a.avg = d_avg;
    a.cell_size = cell_size;
    a.adj_px = adj_px;
    a.min_views = min_views;
    a.front = const_cast<int32_t*>(d_front);   // read only by the test's kernels
    a.vis = d_vis;
    a.conf = d_conf;
    a.keep = d_keep;
    if (mvs_launch_wfilt_test(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wfilt_test launch failed"};
}

int mvs_wfilt_front_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, const uint64_t* d_mask,
                           int cell_size, int32_t* d_front, double* d_zfront, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wfilt_check(ctx, "mvs_wfilt_front", n, cell_size, 0.0, 0, d_front && d_zfront,
                             d_c && d_ref && d_mask))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wfilt_front_launch(ctx, n, d_c, d_ref, d_mask, cell_size, d_front, d_zfront, s);
        return 0;
    });
}

int mvs_wfilt_test_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                          const uint64_t* d_mask, const double* d_avg, int cell_size, double adj_px, int min_views,
                          const int32_t* d_front, uint64_t* d_vis, int64_t* d_conf, uint8_t* d_keep, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wfilt_check(ctx, "mvs_wfilt_test", n, cell_size, adj_px, min_views, true,
                             d_c && d_nrm && d_ref && d_mask && d_avg && d_front && d_vis && d_conf && d_keep))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wfilt_test_launch(ctx, n, d_c, d_nrm, d_ref, d_mask, d_avg, cell_size, adj_px, min_views, d_front, d_vis,
                          d_conf, d_keep, s);
        return 0;
    });
}

int mvs_wfilt_front(mvs_ctx* ctx, int64_t n, const double* c, const int32_t* ref, const uint64_t* mask,
                    int cell_size, int32_t* front, double* zfront) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wfilt_check(ctx, "mvs_wfilt_front", n, cell_size, 0.0, 0, front && zfront, c && ref && mask))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        const int64_t cells = (int64_t)ctx->V * (ctx->H / cell_size) * (ctx->W / cell_size);
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_ref = st.in(ref, n);
        const auto d_mask = st.in(mask, n * ctx->words());
        const auto d_front = st.out(front, cells);
        const auto d_zfront = st.out(zfront, cells);
        st.upload();
        wfilt_front_launch(ctx, n, d_c, d_ref, d_mask, cell_size, d_front, d_zfront, s);
        st.finish();
        return 0;
    });
}

int mvs_wfilt_test(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                   const uint64_t* mask, const double* avg, int cell_size, double adj_px, int min_views,
                   const int32_t* front, uint64_t* vis, int64_t* conf, uint8_t* keep) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wfilt_check(ctx, "mvs_wfilt_test", n, cell_size, adj_px, min_views, true,
                             c && nrm && ref && mask && avg && front && vis && conf && keep))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        const int64_t cells = (int64_t)ctx->V * (ctx->H / cell_size) * (ctx->W / cell_size);
        for (int64_t k = 0; k < cells; ++k)
            if (front[k] < -1 || front[k] >= n) throw Fail{MVS_E_ARG, "mvs_wfilt_test: front entry outside -1..n-1"};
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_nrm = st.in(nrm, n * 3);
        const auto d_avg = st.in(avg, n);
        const auto d_ref = st.in(ref, n);
        const auto d_mask = st.in(mask, n * ctx->words());
        const auto d_front = st.in(front, cells);
        const auto d_vis = st.out(vis, n * ctx->words());
        const auto d_conf = st.out(conf, n);
        const auto d_keep = st.out(keep, n);
        st.upload();
        wfilt_test_launch(ctx, n, d_c, d_nrm, d_ref, d_mask, d_avg, cell_size, adj_px, min_views, d_front, d_vis,
                          d_conf, d_keep, s);
        st.finish();
        return 0;
    });
}

// ---- the neighbour-support test (k_wfilt_support) ----

static int wsup_check(mvs_ctx* ctx, int64_t n, int cell_size, double adj_px, double min_support, int min_neigh,
                      bool rows_ok) {
    if (int rc = wfilt_check(ctx, "mvs_wfilt_support", n, cell_size, adj_px, 0, true, rows_ok)) return rc;
    if (!(min_support >= 0.0 && min_support <= 1.0))
        return set_err(ctx, Fail{MVS_E_ARG, "mvs_wfilt_support: min_support must be in 0..1"});
    if (int rc = need_nonneg(ctx, "mvs_wfilt_support", "min_neigh", min_neigh)) return rc;
    return 0;
}

static void wsup_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                        const uint64_t* d_mask, int cell_size, double adj_px, double min_support, int min_neigh,
                        const int32_t* d_front, int32_t* d_nb, int32_t* d_adj, uint8_t* d_keep, hipStream_t s) {
    WsupArgs a{};
    a.n = n;
    a.c = d_c;
    a.nrm = d_nrm;
    a.ref = d_ref;
    a.mask = d_mask;
    a.cell_size = cell_size;
    a.min_neigh = min_neigh;
    a.adj_px = adj_px;
    a.min_support = min_support;
    a.front = d_front;
    a.nb = d_nb;
    a.adj = d_adj;
    a.keep = d_keep;
    if (mvs_launch_wfilt_support(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wfilt_support launch failed"};
}

int mvs_wfilt_support_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                             const uint64_t* d_mask, int cell_size, double adj_px, double min_support,
                             int min_neigh, const int32_t* d_front, int32_t* d_nb, int32_t* d_adj, uint8_t* d_keep,
                             void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wsup_check(ctx, n, cell_size, adj_px, min_support, min_neigh,
                            d_c && d_nrm && d_ref && d_mask && d_front && d_nb && d_adj && d_keep))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wsup_launch(ctx, n, d_c, d_nrm, d_ref, d_mask, cell_size, adj_px, min_support, min_neigh, d_front, d_nb,
                    d_adj, d_keep, s);
        return 0;
    });
}

int mvs_wfilt_support(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                      const uint64_t* mask, int cell_size, double adj_px, double min_support, int min_neigh,
                      const int32_t* front, int32_t* nb, int32_t* adj, uint8_t* keep) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wsup_check(ctx, n, cell_size, adj_px, min_support, min_neigh,
                            c && nrm && ref && mask && front && nb && adj && keep))
        return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        const int64_t cells = (int64_t)ctx->V * (ctx->H / cell_size) * (ctx->W / cell_size);
        for (int64_t k = 0; k < cells; ++k)
            if (front[k] < -1 || front[k] >= n)
                throw Fail{MVS_E_ARG, "mvs_wfilt_support: front entry outside -1..n-1"};
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_nrm = st.in(nrm, n * 3);
        const auto d_mask = st.in(mask, n * ctx->words());
        const auto d_ref = st.in(ref, n);
        const auto d_front = st.in(front, cells);
        const auto d_nb = st.out(nb, n);
        const auto d_adj = st.out(adj, n);
        const auto d_keep = st.out(keep, n);
        st.upload();
        wsup_launch(ctx, n, d_c, d_nrm, d_ref, d_mask, cell_size, adj_px, min_support, min_neigh, d_front, d_nb,
                    d_adj, d_keep, s);
        st.finish();
        return 0;
    });
}

// ---- seeds from features and patch colours (mvs_seed_warp.hip) ----

// the checks of both entry points; *F = the feature total.  0, or the error's code
static int wseed_check(mvs_ctx* ctx, const int64_t* feat_off, int64_t np, const int32_t* pairs, double epi_px,
                       double min_sin2, int64_t cap, int64_t* F) {
    const char* who = "mvs_wseed_match";
    if (int rc = need_nonneg(ctx, who, "np", np)) return rc;
    if (np >= ((int64_t)1 << 31)) return bad_arg(ctx, who, "np must be below 2^31");
    if (int rc = need_nonneg(ctx, who, "cap", cap)) return rc;
    if (!(epi_px > 0.0 && epi_px < HUGE_VAL)) return bad_arg(ctx, who, "epi_px must be finite and > 0");
    if (!(min_sin2 >= 0.0 && min_sin2 < 1.0)) return bad_arg(ctx, who, "min_sin2 must be in [0, 1)");
    *F = 0;
    if (np == 0) return 0;
    if (!feat_off || !pairs) return bad_arg(ctx, who, "null pointer (feat_off, pairs)");
    const int V = ctx->V;
    if (feat_off[0] != 0) return bad_arg(ctx, who, "feat_off[0] must be 0");
    for (int v = 0; v < V; ++v)
        if (feat_off[v + 1] < feat_off[v]) return bad_arg(ctx, who, "feat_off decreases");
    if (feat_off[V] >= ((int64_t)1 << 31)) return bad_arg(ctx, who, "more than 2^31 - 1 features");
    for (int64_t k = 0; k < np; ++k) {
        const int32_t r = pairs[2 * k], v = pairs[2 * k + 1];
        if (r < 0 || r >= V || v < 0 || v >= V) return bad_arg(ctx, who, "pair view out of range");
        if (r == v) return bad_arg(ctx, who, "pair of a view with itself");
    }
    *F = feat_off[V];
    return 0;
}

// the call on device pointers (F > 0, np > 0, arguments checked)
static void wseed_launch(mvs_ctx* ctx, const int32_t* d_feat, const int64_t* feat_off, int64_t np,
                         const int32_t* pairs, double epi_px, double min_sin2, int64_t cap, double* d_c,
                         double* d_nrm, int32_t* d_ref, int32_t* d_cand, double* d_err, int64_t* d_total,
                         hipStream_t s) {
    int64_t rows = 0, nblocks = 0;
    for (int64_t k = 0; k < np; ++k) {
        const int64_t na = feat_off[pairs[2 * k] + 1] - feat_off[pairs[2 * k]];
        rows += na;
        nblocks += (na + MVS_SEED_BLOCK - 1) / MVS_SEED_BLOCK;
    }
    if (rows >= ((int64_t)1 << 31) || nblocks >= ((int64_t)1 << 31))
        throw Fail{MVS_E_ARG, "mvs_wseed_match: the pairs' reference features sum to 2^31 or more"};
    ctx->wexp_order.acquire(s);
    const size_t bytes = (size_t)np * sizeof(SeedPair) + (size_t)nblocks * sizeof(int2);
    unsigned char* h = ctx->s_tab_h.fill(bytes);
    SeedPair* hp = (SeedPair*)h;
    int2* hb = (int2*)(h + (size_t)np * sizeof(SeedPair));
    int64_t row = 0, blk = 0;
    for (int64_t k = 0; k < np; ++k) {
        const int32_t r = pairs[2 * k], v = pairs[2 * k + 1];
        SeedPair p{};
        p.r = r;
        p.v = v;
        p.a0 = (int32_t)feat_off[r];
        p.na = (int32_t)(feat_off[r + 1] - feat_off[r]);
        p.b0 = (int32_t)feat_off[v];
        p.nb = (int32_t)(feat_off[v + 1] - feat_off[v]);
        p.row0 = row;
        hp[k] = p;
        row += p.na;
        for (int32_t a0 = 0; a0 < p.na; a0 += MVS_SEED_BLOCK) hb[blk++] = make_int2((int)k, a0);
    }
    ctx->s_tab.ensure(bytes);
    ctx->x_cnt.ensure((size_t)rows);
    ctx->x_offs.ensure((size_t)rows + 1);
    ctx->s_tab_h.upload(ctx->s_tab.p, bytes, s);
    WseedArgs a{};
    a.feat = d_feat;
    a.pairs = (const SeedPair*)ctx->s_tab.p;
    a.blocks = (const int2*)(ctx->s_tab.p + (size_t)np * sizeof(SeedPair));
    a.nblocks = nblocks;
    a.rows = rows;
    a.epi2 = epi_px * epi_px;
    a.min_sin2 = min_sin2;
    a.cap = cap;
    a.cnt = ctx->x_cnt.p;
    a.offs = ctx->x_offs.p;
    a.c = d_c;
    a.nrm = d_nrm;
    a.ref = d_ref;
    a.cand = d_cand;
    a.err = d_err;
    a.total = d_total;
    if (mvs_launch_wseed_match(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wseed_match launch failed"};
    ctx->wexp_order.release(s);
}

int mvs_wseed_match_device(mvs_ctx* ctx, const int32_t* d_feat, const int64_t* feat_off, int64_t np,
                           const int32_t* pairs, double epi_px, double min_sin2, int64_t cap, double* d_c,
                           double* d_nrm, int32_t* d_ref, int32_t* d_cand, double* d_err, int64_t* d_total,
                           void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    int64_t F = 0;
    if (int rc = wseed_check(ctx, feat_off, np, pairs, epi_px, min_sin2, cap, &F)) return rc;
    if (np == 0 || F == 0) return MVS_OK;
    if (!d_feat || !d_total || (cap > 0 && (!d_c || !d_nrm || !d_ref || !d_cand || !d_err)))
        return bad_arg(ctx, "mvs_wseed_match", "null pointer (the outputs may be NULL when cap is 0)");
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wseed_launch(ctx, d_feat, feat_off, np, pairs, epi_px, min_sin2, cap, d_c, d_nrm, d_ref, d_cand, d_err,
                     d_total, s);
        return 0;
    });
}

int mvs_wseed_match(mvs_ctx* ctx, const int32_t* feat, const int64_t* feat_off, int64_t np, const int32_t* pairs,
                    double epi_px, double min_sin2, int64_t cap, double* c, double* nrm, int32_t* ref,
                    int32_t* cand, double* err, int64_t* total) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    int64_t F = 0;
    if (int rc = wseed_check(ctx, feat_off, np, pairs, epi_px, min_sin2, cap, &F)) return rc;
    if (np == 0 || F == 0) return MVS_OK;
    if (!feat || !total || (cap > 0 && (!c || !nrm || !ref || !cand || !err)))
        return bad_arg(ctx, "mvs_wseed_match", "null pointer (the outputs may be NULL when cap is 0)");
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_feat = st.in(feat, F * 2);
        const auto d_c = st.out(cap ? c : nullptr, cap * 3);
        const auto d_nrm = st.out(cap ? nrm : nullptr, cap * 3);
        const auto d_err = st.out(cap ? err : nullptr, cap);
        const auto d_total = st.out(total, 1);
        const auto d_ref = st.out(cap ? ref : nullptr, cap);
        const auto d_cand = st.out(cap ? cand : nullptr, cap * 4);
        st.upload();
        wseed_launch(ctx, d_feat, feat_off, np, pairs, epi_px, min_sin2, cap, d_c, d_nrm, d_ref, d_cand, d_err,
                     d_total, s);
        st.finish();
        return 0;
    });
}

static int wcol_check(mvs_ctx* ctx, int64_t n, bool ptrs_ok) {
    if (int rc = need_nonneg(ctx, "mvs_wpatch_color", "n", n)) return rc;
    if (n >= ((int64_t)1 << 31)) return bad_arg(ctx, "mvs_wpatch_color", "n must be below 2^31");
    if (n > 0 && !ptrs_ok) return bad_arg(ctx, "mvs_wpatch_color", "null pointer");
    return 0;
}

static void wcol_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, const uint64_t* d_mask,
                        double* d_color, int32_t* d_nviews, hipStream_t s) {
    WcolArgs a{};
    a.n = n;
    a.c = d_c;
    a.ref = d_ref;
    a.mask = d_mask;
    a.color = d_color;
    a.nviews = d_nviews;
    if (mvs_launch_wpatch_color(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wpatch_color launch failed"};
}

int mvs_wpatch_color_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, const uint64_t* d_mask,
                            double* d_color, int32_t* d_nviews, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wcol_check(ctx, n, d_c && d_ref && d_mask && d_color && d_nviews)) return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wcol_launch(ctx, n, d_c, d_ref, d_mask, d_color, d_nviews, s);
        return 0;
    });
}

int mvs_wpatch_color(mvs_ctx* ctx, int64_t n, const double* c, const int32_t* ref, const uint64_t* mask,
                     double* color, int32_t* nviews) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wcol_check(ctx, n, c && ref && mask && color && nviews)) return rc;
    if (n == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_mask = st.in(mask, n * ctx->words());
        const auto d_ref = st.in(ref, n);
        const auto d_color = st.out(color, n * 3);
        const auto d_nviews = st.out(nviews, n);
        st.upload();
        wcol_launch(ctx, n, d_c, d_ref, d_mask, d_color, d_nviews, s);
        st.finish();
        return 0;
    });
}

// ---- depth maps of a warped patch set (mvs_depth_warp.hip) ----

static int need_views(mvs_ctx* ctx, const char* who, int v0, int nv) {
    return v0 < 0 || nv < 1 || (int64_t)v0 + nv > ctx->V
               ? bad_arg(ctx, who, "the view range v0 .. v0 + nv - 1 must lie inside 0..V-1, nv >= 1")
               : 0;
}

static int wsplat_check(mvs_ctx* ctx, int64_t n, int radius, double slope, int v0, int nv, bool maps_ok,
                        bool rows_ok) {
    const char* who = "mvs_wdepth_splat";
    if (int rc = need_nonneg(ctx, who, "n", n)) return rc;
    if (n >= ((int64_t)1 << 31)) return bad_arg(ctx, who, "n must be below 2^31");
    if (radius < 0 || radius > 3) return bad_arg(ctx, who, "radius must be in 0..3");
    if (!(slope > 0.0 && slope < HUGE_VAL)) return bad_arg(ctx, who, "slope must be finite and > 0");
    if (int rc = need_views(ctx, who, v0, nv)) return rc;
    if (!maps_ok || (n > 0 && !rows_ok)) return bad_arg(ctx, who, "null pointer");
    return 0;
}

static void wsplat_launch(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                          const uint64_t* d_mask, int radius, double slope, int v0, int nv, double* d_zmap,
                          int32_t* d_idmap, hipStream_t s) {
    WdepthArgs a{};
    a.n = n;
    a.c = d_c;
    a.nrm = d_nrm;
    a.ref = d_ref;
    a.mask = d_mask;
    a.radius = radius;
    a.v0 = v0;
    a.nv = nv;
    a.slope = slope;
    a.zmap = (uint64_t*)d_zmap;
    a.idmap = d_idmap;
    if (mvs_launch_wdepth_splat(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wdepth_splat launch failed"};
}

int mvs_wdepth_splat_device(mvs_ctx* ctx, int64_t n, const double* d_c, const double* d_nrm, const int32_t* d_ref,
                            const uint64_t* d_mask, int radius, double slope, int v0, int nv, double* d_zmap,
                            int32_t* d_idmap, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wsplat_check(ctx, n, radius, slope, v0, nv, d_zmap && d_idmap, d_c && d_nrm && d_ref && d_mask))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wsplat_launch(ctx, n, d_c, d_nrm, d_ref, d_mask, radius, slope, v0, nv, d_zmap, d_idmap, s);
        return 0;
    });
}

int mvs_wdepth_splat(mvs_ctx* ctx, int64_t n, const double* c, const double* nrm, const int32_t* ref,
                     const uint64_t* mask, int radius, double slope, int v0, int nv, double* zmap, int32_t* idmap) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wsplat_check(ctx, n, radius, slope, v0, nv, zmap && idmap, c && nrm && ref && mask)) return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        const int64_t pixels = (int64_t)nv * ctx->H * ctx->W;
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_nrm = st.in(nrm, n * 3);
        const auto d_mask = st.in(mask, n * ctx->words());
        const auto d_ref = st.in(ref, n);
        const auto d_zmap = st.out(zmap, pixels);
        const auto d_idmap = st.out(idmap, pixels);
        st.upload();
        wsplat_launch(ctx, n, d_c, d_nrm, d_ref, d_mask, radius, slope, v0, nv, d_zmap, d_idmap, s);
        st.finish();
        return 0;
    });
}

static int wcons_check(mvs_ctx* ctx, int v0, int nv, double rel_tol, bool ptrs_ok) {
    const char* who = "mvs_wdepth_consist";
    if (!(rel_tol >= 0.0 && rel_tol < HUGE_VAL)) return bad_arg(ctx, who, "rel_tol must be finite and >= 0");
    if (int rc = need_views(ctx, who, v0, nv)) return rc;
    if (!ptrs_ok) return bad_arg(ctx, who, "null pointer (only viol may be NULL)");
    return 0;
}

static void wcons_launch(mvs_ctx* ctx, const double* d_zmap, int v0, int nv, double rel_tol, uint8_t* d_cons,
                         uint8_t* d_viol, hipStream_t s) {
    WconsArgs a{};
    a.zmap = d_zmap;
    a.v0 = v0;
    a.nv = nv;
    a.rel_tol = rel_tol;
    a.cons = d_cons;
    a.viol = d_viol;
    if (mvs_launch_wdepth_consist(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wdepth_consist launch failed"};
}

int mvs_wdepth_consist_device(mvs_ctx* ctx, const double* d_zmap, int v0, int nv, double rel_tol, uint8_t* d_cons,
                              uint8_t* d_viol, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wcons_check(ctx, v0, nv, rel_tol, d_zmap && d_cons)) return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wcons_launch(ctx, d_zmap, v0, nv, rel_tol, d_cons, d_viol, s);
        return 0;
    });
}

int mvs_wdepth_consist(mvs_ctx* ctx, const double* zmap, int v0, int nv, double rel_tol, uint8_t* cons,
                       uint8_t* viol) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wcons_check(ctx, v0, nv, rel_tol, zmap && cons)) return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        const int64_t pixels = (int64_t)nv * ctx->H * ctx->W;
        Staging& st = ctx->staging.begin(s);
        const auto d_zmap = st.in(zmap, pixels);
        const auto d_cons = st.out(cons, pixels);
        const auto d_viol = st.out(viol, pixels);
        st.upload();
        wcons_launch(ctx, d_zmap, v0, nv, rel_tol, d_cons, d_viol, s);
        st.finish();
        return 0;
    });
}

static int wpoints_check(mvs_ctx* ctx, int64_t m, int v0, int nv, bool map_ok, bool rows_ok) {
    const char* who = "mvs_wdepth_points";
    if (int rc = need_nonneg(ctx, who, "m", m)) return rc;
    if (m >= ((int64_t)1 << 31)) return bad_arg(ctx, who, "m must be below 2^31");
    if (int rc = need_views(ctx, who, v0, nv)) return rc;
    if (!map_ok || (m > 0 && !rows_ok)) return bad_arg(ctx, who, "null pointer");
    return 0;
}

static void wpoints_launch(mvs_ctx* ctx, int64_t m, const int32_t* d_pix, const double* d_zmap, int v0, int nv,
                           double* d_xyz, uint8_t* d_rgb, hipStream_t s) {
    WpointsArgs a{};
    a.m = m;
    a.pix = d_pix;
    a.zmap = d_zmap;
    a.v0 = v0;
    a.nv = nv;
    a.xyz = d_xyz;
    a.rgb = d_rgb;
    if (mvs_launch_wdepth_points(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wdepth_points launch failed"};
}

int mvs_wdepth_points_device(mvs_ctx* ctx, int64_t m, const int32_t* d_pix, const double* d_zmap, int v0, int nv,
                             double* d_xyz, uint8_t* d_rgb, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wpoints_check(ctx, m, v0, nv, d_zmap != nullptr, d_pix && d_xyz && d_rgb)) return rc;
    if (m == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wpoints_launch(ctx, m, d_pix, d_zmap, v0, nv, d_xyz, d_rgb, s);
        return 0;
    });
}

int mvs_wdepth_points(mvs_ctx* ctx, int64_t m, const int32_t* pix, const double* zmap, int v0, int nv, double* xyz,
                      uint8_t* rgb) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (int rc = wpoints_check(ctx, m, v0, nv, zmap != nullptr, pix && xyz && rgb)) return rc;
    if (m == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        for (int64_t k = 0; k < m; ++k) {
            const int32_t* q = pix + 3 * k;
            if (q[0] < v0 || q[0] >= v0 + nv || q[1] < 0 || q[1] >= ctx->W || q[2] < 0 || q[2] >= ctx->H)
                throw Fail{MVS_E_ARG, "mvs_wdepth_points: listed pixel outside the view range or the image"};
        }
        hipStream_t s = ctx->stream;
        const int64_t pixels = (int64_t)nv * ctx->H * ctx->W;
        Staging& st = ctx->staging.begin(s);
        const auto d_zmap = st.in(zmap, pixels);
        const auto d_xyz = st.out(xyz, m * 3);
        const auto d_pix = st.in(pix, m * 3);
        const auto d_rgb = st.out(rgb, m * 3);
        st.upload();
        wpoints_launch(ctx, m, d_pix, d_zmap, v0, nv, d_xyz, d_rgb, s);
        st.finish();
        return 0;
    });
}

// ---- per-pixel plane propagation on the depth maps (mvs_prop_warp.hip) ----

struct WpropCall {
    int v0, nv, tv, wid, top_k, step, kd, ka;
    double min_cos, min_ncc, astep, depth_px, step_scale;
    const int32_t* lists;
};

// byte ranges [p, p + n) and [q, q + m) share a byte
static bool overlaps(const void* p, size_t n, const void* q, size_t m) {
    const char* a = (const char*)p;
    const char* b = (const char*)q;
    return p && q && n && m && a < b + m && b < a + n;
}

// the checks of both entry points (0, or the error's code with the message recorded)
static int wprop_check(mvs_ctx* ctx, const WpropCall& k, const void* zmap, const void* nmap, const void* z_out,
                       const void* n_out, const void* score, const void* best, const void* scores) {
    const char* who = "mvs_wprop_sweep";
    if (k.v0 < 0 || k.nv < 0 || (int64_t)k.v0 + k.nv > ctx->V)
        return bad_arg(ctx, who, "the view range v0 .. v0 + nv - 1 must lie inside 0..V-1");
    if (int rc = need_wid(ctx, who, k.wid)) return rc;
    if (int rc = need_min_cos(ctx, who, k.min_cos)) return rc;
    if (std::isnan(k.min_ncc)) return bad_arg(ctx, who, "min_ncc is nan");
    if (k.tv < 1 || k.tv > 32) return bad_arg(ctx, who, "tv must be in 1..32");
    if (k.top_k < 1 || k.top_k > k.tv) return bad_arg(ctx, who, "top_k must be in 1..tv");
    if (k.step < 1 || k.step > 64) return bad_arg(ctx, who, "step must be in 1..64");
    if (k.kd < 0 || k.kd > 3) return bad_arg(ctx, who, "kd must be in 0..3");
    if (k.ka < 0 || k.ka > 2) return bad_arg(ctx, who, "ka must be in 0..2");
    if (!(k.depth_px > 0.0 && k.depth_px < HUGE_VAL)) return bad_arg(ctx, who, "depth_px must be finite and > 0");
    if (!(k.step_scale > 0.0) || !std::isfinite(k.step_scale)) return bad_arg(ctx, who, "step_scale must be > 0");
    if (!(k.astep >= 0.0) || !((double)k.ka * k.astep * k.step_scale <= 1.2))
        return bad_arg(ctx, who, "ka * astep * step_scale must be in [0, 1.2]");
    if (k.nv > 0 && !k.lists) return bad_arg(ctx, who, "null pointer (lists)");
    const int V = ctx->V;
    for (int r = 0; r < k.nv; ++r) {
        const int32_t* l = k.lists + (size_t)r * k.tv;
        bool ended = false;
        for (int j = 0; j < k.tv; ++j) {
            if (l[j] < -1 || l[j] >= V) return bad_arg(ctx, who, "list view out of range");
            if (l[j] < 0) { ended = true; continue; }
            if (ended) return bad_arg(ctx, who, "list view after a -1");
            if (l[j] == k.v0 + r) return bad_arg(ctx, who, "list view equal to the row's own view");
            for (int i = 0; i < j; ++i)
                if (l[i] == l[j]) return bad_arg(ctx, who, "list view repeated");
        }
    }
    const size_t px = (size_t)k.nv * ctx->H * ctx->W;
    if (px == 0) return 0;
    if (!zmap || !nmap || !z_out || !n_out || !score || !best)
        return bad_arg(ctx, who, "null pointer (only scores may be NULL)");
    const int A = 2 * k.ka + 1;
    const size_t HY = 5 + (size_t)(2 * k.kd + 1) * A * A;
    const void* in[2] = {zmap, nmap};
    const size_t in_b[2] = {px * 8, px * 24};
    const void* out[5] = {z_out, n_out, score, best, scores};
    const size_t out_b[5] = {px * 8, px * 24, px * 8, px * 4, px * HY * 8};
    for (int o = 0; o < 5; ++o) {
        for (int i = 0; i < 2; ++i)
            if (overlaps(out[o], out_b[o], in[i], in_b[i])) return bad_arg(ctx, who, "an output overlaps an input");
        for (int i = 0; i < o; ++i)
            if (overlaps(out[o], out_b[o], out[i], out_b[i])) return bad_arg(ctx, who, "two outputs overlap");
    }
    return 0;
}

// one launch per view: the view's list travels in the kernel's arguments
static void wprop_launch(mvs_ctx* ctx, const WpropCall& k, const double* d_zmap, const double* d_nmap, double* d_z_out,
                         double* d_n_out, double* d_score, int32_t* d_best, double* d_scores, hipStream_t s) {
    const size_t hw = (size_t)ctx->H * ctx->W;
    const int A = 2 * k.ka + 1;
    const size_t HY = 5 + (size_t)(2 * k.kd + 1) * A * A;
    WpropArgs a{};
    a.top_k = k.top_k;
    a.step = k.step;
    a.kd = k.kd;
    a.ka = k.ka;
    a.min_cos = k.min_cos;
    a.min_ncc = k.min_ncc;
    a.depth_px = k.depth_px;
    a.step_scale = k.step_scale;
    // the grid's tangents from the host's libm, as mvs_refine_warped's
    const double alpha = k.astep * k.step_scale;
    for (int i = -k.ka; i <= k.ka; ++i) a.tans[i + k.ka] = std::tan((double)i * alpha);
    for (int r = 0; r < k.nv; ++r) {
        a.v = k.v0 + r;
        a.T = 0;
        for (int j = 0; j < 32; ++j) {
            a.views[j] = j < k.tv ? k.lists[(size_t)r * k.tv + j] : -1;
            if (a.views[j] >= 0) ++a.T;
        }
        a.zmap = d_zmap + r * hw;
        a.nmap = d_nmap + r * hw * 3;
        a.z_out = d_z_out + r * hw;
        a.n_out = d_n_out + r * hw * 3;
        a.score = d_score + r * hw;
        a.best = d_best + r * hw;
        a.scores = d_scores ? d_scores + r * hw * HY : nullptr;
        if (mvs_launch_wprop_sweep(&ctx->sc, &a, k.wid, s) != 0) throw Fail{MVS_E_HIP, "wprop_sweep launch failed"};
    }
}

int mvs_wprop_sweep_device(mvs_ctx* ctx, int v0, int nv, const double* d_zmap, const double* d_nmap,
                           const int32_t* lists, int tv, int wid, double min_cos, double min_ncc, int top_k, int step,
                           int kd, int ka, double astep, double depth_px, double step_scale, double* d_z_out,
                           double* d_n_out, double* d_score, int32_t* d_best, double* d_scores, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    const WpropCall k{v0, nv, tv, wid, top_k, step, kd, ka, min_cos, min_ncc, astep, depth_px, step_scale, lists};
    if (int rc = wprop_check(ctx, k, d_zmap, d_nmap, d_z_out, d_n_out, d_score, d_best, d_scores)) return rc;
    if ((int64_t)nv * ctx->H * ctx->W == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wprop_launch(ctx, k, d_zmap, d_nmap, d_z_out, d_n_out, d_score, d_best, d_scores, s);
        return 0;
    });
}

int mvs_wprop_sweep(mvs_ctx* ctx, int v0, int nv, const double* zmap, const double* nmap, const int32_t* lists,
                    int tv, int wid, double min_cos, double min_ncc, int top_k, int step, int kd, int ka, double astep,
                    double depth_px, double step_scale, double* z_out, double* n_out, double* score, int32_t* best,
                    double* scores) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    const WpropCall k{v0, nv, tv, wid, top_k, step, kd, ka, min_cos, min_ncc, astep, depth_px, step_scale, lists};
    if (int rc = wprop_check(ctx, k, zmap, nmap, z_out, n_out, score, best, scores)) return rc;
    const int64_t px = (int64_t)nv * ctx->H * ctx->W;
    if (px == 0) return MVS_OK;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        const int A = 2 * ka + 1;
        const int64_t HY = 5 + (int64_t)(2 * kd + 1) * A * A;
        Staging& st = ctx->staging.begin(s);
        const auto d_zmap = st.in(zmap, px);
        const auto d_nmap = st.in(nmap, px * 3);
        const auto d_zo = st.out(z_out, px);
        const auto d_no = st.out(n_out, px * 3);
        const auto d_sc = st.out(score, px);
        const auto d_best = st.out(best, px);
        const auto d_scores = st.out(scores, px * HY);
        st.upload();
        wprop_launch(ctx, k, d_zmap, d_nmap, d_zo, d_no, d_sc, d_best, d_scores, s);
        st.finish();
        return 0;
    });
}

// ---- the signed-distance lattice and its mesh (mvs_mesh_warp.hip) ----

// the lattice's checks; *points = the number of lattice points.  0, or the error's code
static int lattice_check(mvs_ctx* ctx, const char* who, int nx, int ny, int nz, const double* origin, double voxel,
                         int64_t* points) {
    if (nx < 1 || ny < 1 || nz < 1) return bad_arg(ctx, who, "nx, ny and nz must be >= 1");
    const int64_t limit = (int64_t)1 << 27;
    // factor by factor: the product of three ints can pass 2^63
    if (nx >= limit || ny >= limit || nz >= limit || ((int64_t)nx + 1) * ((int64_t)ny + 1) > limit ||
        ((int64_t)nx + 1) * ((int64_t)ny + 1) * ((int64_t)nz + 1) > limit)
        return bad_arg(ctx, who, "more than 2^27 lattice points");
    if (!origin) return bad_arg(ctx, who, "null pointer (origin)");
    for (int m = 0; m < 3; ++m)
        if (!std::isfinite(origin[m])) return bad_arg(ctx, who, "origin must be finite");
    if (!(voxel > 0.0 && voxel < HUGE_VAL)) return bad_arg(ctx, who, "voxel must be finite and > 0");
    *points = ((int64_t)nx + 1) * ((int64_t)ny + 1) * ((int64_t)nz + 1);
    return 0;
}

static int wtsdf_check(mvs_ctx* ctx, int v0, int nv, int nx, int ny, int nz, const double* origin, double voxel,
                       double trunc, int min_weight, bool ptrs_ok, int64_t* points) {
    const char* who = "mvs_wtsdf_integrate";
    if (int rc = lattice_check(ctx, who, nx, ny, nz, origin, voxel, points)) return rc;
    if (!(trunc > 0.0 && trunc < HUGE_VAL)) return bad_arg(ctx, who, "trunc must be finite and > 0");
    if (min_weight < 1) return bad_arg(ctx, who, "min_weight must be >= 1");
    if (int rc = need_views(ctx, who, v0, nv)) return rc;
    if (!ptrs_ok) return bad_arg(ctx, who, "null pointer");
    return 0;
}

static void wtsdf_launch(mvs_ctx* ctx, const double* d_zmap, int v0, int nv, int nx, int ny, int nz,
                         const double* origin, double voxel, double trunc, int min_weight, double* d_tsdf,
                         int32_t* d_weight, uint8_t* d_rgb, uint8_t* d_cnt, hipStream_t s) {
    WtsdfArgs a{};
    a.zmap = d_zmap;
    a.v0 = v0;
    a.nv = nv;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    for (int m = 0; m < 3; ++m) a.origin[m] = origin[m];
    a.voxel = voxel;
    a.trunc = trunc;
    a.min_weight = min_weight;
    a.tsdf = d_tsdf;
    a.weight = d_weight;
    a.rgb = d_rgb;
    a.cnt = d_cnt;
    if (mvs_launch_wtsdf_integrate(&ctx->sc, &a, s) != 0) throw Fail{MVS_E_HIP, "wtsdf_integrate launch failed"};
}

int mvs_wtsdf_integrate_device(mvs_ctx* ctx, const double* d_zmap, int v0, int nv, int nx, int ny, int nz,
                               const double* origin, double voxel, double trunc, int min_weight, double* d_tsdf,
                               int32_t* d_weight, uint8_t* d_rgb, uint8_t* d_cnt, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    int64_t points = 0;
    if (int rc = wtsdf_check(ctx, v0, nv, nx, ny, nz, origin, voxel, trunc, min_weight,
                             d_zmap && d_tsdf && d_weight && d_rgb && d_cnt, &points))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wtsdf_launch(ctx, d_zmap, v0, nv, nx, ny, nz, origin, voxel, trunc, min_weight, d_tsdf, d_weight, d_rgb,
                     d_cnt, s);
        return 0;
    });
}

int mvs_wtsdf_integrate(mvs_ctx* ctx, const double* zmap, int v0, int nv, int nx, int ny, int nz,
                        const double* origin, double voxel, double trunc, int min_weight, double* tsdf,
                        int32_t* weight, uint8_t* rgb, uint8_t* cnt) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    int64_t points = 0;
    if (int rc = wtsdf_check(ctx, v0, nv, nx, ny, nz, origin, voxel, trunc, min_weight,
                             zmap && tsdf && weight && rgb && cnt, &points))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_zmap = st.in(zmap, (int64_t)nv * ctx->H * ctx->W);
        const auto d_tsdf = st.out(tsdf, points);
        const auto d_weight = st.out(weight, points);
        const auto d_rgb = st.out(rgb, points * 3);
        const auto d_cnt = st.out(cnt, points);
        st.upload();
        wtsdf_launch(ctx, d_zmap, v0, nv, nx, ny, nz, origin, voxel, trunc, min_weight, d_tsdf, d_weight, d_rgb,
                     d_cnt, s);
        st.finish();
        return 0;
    });
}

static int wmesh_check(mvs_ctx* ctx, int nx, int ny, int nz, const double* origin, double voxel, int64_t cap_v,
                       int64_t cap_t, bool in_ok, bool vert_ok, bool tri_ok, int64_t* points) {
    const char* who = "mvs_wmesh_extract";
    if (int rc = lattice_check(ctx, who, nx, ny, nz, origin, voxel, points)) return rc;
    if (int rc = need_nonneg(ctx, who, "cap_v", cap_v)) return rc;
    if (int rc = need_nonneg(ctx, who, "cap_t", cap_t)) return rc;
    if (cap_v >= ((int64_t)1 << 31) || cap_t >= ((int64_t)1 << 31))
        return bad_arg(ctx, who, "cap_v and cap_t must be below 2^31");
    if (!in_ok || (cap_v > 0 && !vert_ok) || (cap_t > 0 && !tri_ok))
        return bad_arg(ctx, who, "null pointer (vert and vcol may be NULL when cap_v is 0, tri when cap_t is 0)");
    return 0;
}

static void wmesh_launch(mvs_ctx* ctx, int nx, int ny, int nz, const double* origin, double voxel,
                         const double* d_tsdf, const uint8_t* d_rgb, const uint8_t* d_cnt, int64_t cap_v,
                         int64_t cap_t, double* d_vert, uint8_t* d_vcol, int32_t* d_tri, int64_t* d_total,
                         hipStream_t s) {
    const int64_t points = ((int64_t)nx + 1) * (ny + 1) * (nz + 1), cubes = (int64_t)nx * ny * nz;
    const int64_t nbv = (points + MVS_MESH_BLOCK - 1) / MVS_MESH_BLOCK;
    const int64_t nbt = (cubes + MVS_MESH_BLOCK - 1) / MVS_MESH_BLOCK;
    ctx->wmesh_order.acquire(s);
    ctx->m_mask.ensure((size_t)((points + 3) / 4));
    ctx->m_voff.ensure((size_t)points);
    ctx->m_sums.ensure((size_t)(nbv + nbt + 2));
    WmeshArgs a{};
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    for (int m = 0; m < 3; ++m) a.origin[m] = origin[m];
    a.voxel = voxel;
    a.tsdf = d_tsdf;
    a.rgb = d_rgb;
    a.cnt = d_cnt;
    a.cap_v = cap_v;
    a.cap_t = cap_t;
    a.vert = d_vert;
    a.vcol = d_vcol;
    a.tri = d_tri;
    a.total = d_total;
    a.mask = ctx->m_mask.p;
    a.voff = ctx->m_voff.p;
    a.vsum = ctx->m_sums.p;
    a.tsum = ctx->m_sums.p + nbv + 1;
    // s uses the scratch from here on, also when a later pass fails to launch after earlier ones were queued
    ctx->wmesh_order.release(s);
    if (mvs_launch_wmesh_extract(&a, s) != 0) throw Fail{MVS_E_HIP, "wmesh_extract launch failed"};
}

int mvs_wmesh_extract_device(mvs_ctx* ctx, int nx, int ny, int nz, const double* origin, double voxel,
                             const double* d_tsdf, const uint8_t* d_rgb, const uint8_t* d_cnt, int64_t cap_v,
                             int64_t cap_t, double* d_vert, uint8_t* d_vcol, int32_t* d_tri, int64_t* d_total,
                             void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    int64_t points = 0;
    if (int rc = wmesh_check(ctx, nx, ny, nz, origin, voxel, cap_v, cap_t, d_tsdf && d_rgb && d_cnt && d_total,
                             d_vert && d_vcol, d_tri != nullptr, &points))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        wmesh_launch(ctx, nx, ny, nz, origin, voxel, d_tsdf, d_rgb, d_cnt, cap_v, cap_t, d_vert, d_vcol, d_tri,
                     d_total, s);
        return 0;
    });
}

int mvs_wmesh_extract(mvs_ctx* ctx, int nx, int ny, int nz, const double* origin, double voxel, const double* tsdf,
                      const uint8_t* rgb, const uint8_t* cnt, int64_t cap_v, int64_t cap_t, double* vert,
                      uint8_t* vcol, int32_t* tri, int64_t* total) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    int64_t points = 0;
    if (int rc = wmesh_check(ctx, nx, ny, nz, origin, voxel, cap_v, cap_t, tsdf && rgb && cnt && total, vert && vcol,
                             tri != nullptr, &points))
        return rc;
    return guarded(ctx, [&]() {
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_tsdf = st.in(tsdf, points);
        const auto d_rgb = st.in(rgb, points * 3);
        const auto d_cnt = st.in(cnt, points);
        const auto d_vert = st.out(cap_v ? vert : nullptr, cap_v * 3);
        const auto d_vcol = st.out(cap_v ? vcol : nullptr, cap_v * 3);
        const auto d_tri = st.out(cap_t ? tri : nullptr, cap_t * 3);
        const auto d_total = st.out(total, 2);
        st.upload();
        wmesh_launch(ctx, nx, ny, nz, origin, voxel, d_tsdf, d_rgb, d_cnt, cap_v, cap_t, d_vert, d_vcol, d_tri,
                     d_total, s);
        st.finish();
        return 0;
    });
}

}  // extern "C"
