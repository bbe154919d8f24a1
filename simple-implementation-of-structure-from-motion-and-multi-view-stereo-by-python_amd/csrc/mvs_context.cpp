// The scene context of libmvs_amd.so and what runs on it apart from the
// stage: create / destroy / rebuild, the camera table, the scorer dispatch
// (score_device: direct or tiled matrix-core kernels), the scorers' and the
// exchange helpers' C-ABI and the SfM front-end calls.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "mvs_host.h"

namespace {

thread_local std::string g_err;   // mvs_last_error(NULL): the one copy of the library

void build_cameras(mvs_ctx* ctx, const double* K, const double* R, const double* t, const double* Rp) {
    ctx->cams.resize(ctx->V);
    for (int v = 0; v < ctx->V; ++v) {
        CamDev& c = ctx->cams[v];
        std::memset(&c, 0, sizeof c);
        const double* Kv = K + 9 * v;
        const double* Rv = R + 9 * v;
        const double* tv = t + 3 * v;
        if (Rp)
            std::memcpy(c.Rp, Rp + 9 * v, sizeof c.Rp);
        else
            rodrigues_roundtrip(Rv, c.Rp);
        std::memcpy(c.t, tv, sizeof c.t);
        std::memcpy(c.R, Rv, sizeof c.R);
        c.fx = Kv[0];
        c.fy = Kv[4];
        c.cx = Kv[2];
        c.cy = Kv[5];
        c.fbar = (Kv[0] + Kv[4]) / 2;
        for (int j = 0; j < 3; ++j) {
            // camera_pos = -(R^T @ t) (MVS2.py:189); C = (-R^T) @ t (MVS2.py:351)
            c.O[j] = -fma_dot3(Rv[j], Rv[3 + j], Rv[6 + j], tv[0], tv[1], tv[2]);
            c.C[j] = fma_dot3(-Rv[j], -Rv[3 + j], -Rv[6 + j], tv[0], tv[1], tv[2]);
        }
    }
}

}  // namespace

int set_err(mvs_ctx* ctx, const Fail& f) {
    if (ctx) ctx->err = f.msg;
    g_err = f.msg;
    return f.code;
}

// d_count == null: d_mask holds records [mask words, avg bits] of words + 1
// int64 each (mvs_score_device_rec), d_avg is ignored
void score_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, int wid,
                  double thr, double* d_xy, uint64_t* d_mask, int32_t* d_count, double* d_avg,
                  hipStream_t s) {
    if (wid < 1 || wid > MVS_MAX_WID) throw Fail{MVS_E_UNSUPPORTED, "wid must be in 1..5"};
    ScoreArgs a{};
    a.n = n;
    a.c = d_c;
    a.ref = d_ref;
    a.thr = thr;
    a.xy = d_xy;
    a.mask = d_mask;
    a.count = d_count;
    a.avg = d_avg;
    a.exact_hits = ctx->d_exact.p;
    a.mstride = ctx->words();
    a.astride = 1;
    a.rec = 0;
    if (!d_count) {
        a.rec = 1;
        a.mstride = a.astride = ctx->words() + 1;
        a.avg = (double*)(d_mask + ctx->words());
    }
    // the tiled matrix-core scorer (k_score_mma, any V <= 256) for batches of
    // >= 2048 candidates; the direct k_score for small batches
    const bool grouped = ctx->V > MVS_GROUP_VIEWS;
    const bool tiled = ctx->kernel_mode == 2 || (ctx->kernel_mode == 0 && n >= 2048);
    // an empty batch launches nothing: the counter sets and their parity stay
    // as they are (the launcher returns before k_bin, which would have zeroed
    // the other set)
    if (tiled && n == 0) return;
    if (tiled) {
        TiledArgs t{};
        t.tw = MVS_TILE_W;
        t.th = MVS_TILE_H;
        t.ntx = (ctx->W + MVS_TILE_W - 1) / MVS_TILE_W;
        t.nty = (ctx->H + MVS_TILE_H - 1) / MVS_TILE_H;
        const int ntiles = t.ntx * t.nty;
        const int32_t* tiles_before = ctx->t_tiles.p;
        const int64_t set_words = tc_words(ntiles);
        ctx->t_tiles.ensure((size_t)(2 * set_words));   // two counter sets (parities)
        if (ctx->t_tiles.p != tiles_before) ctx->tiles_clean_ntiles = -1;
        const int groups = grouped ? (ctx->V + MVS_GROUP_VIEWS - 1) / MVS_GROUP_VIEWS : 1;
        // tile buckets of cap candidates (16x the mean load, at least 1024:
        // expansion sweeps crowd onto the object's tiles; the rest of a tile
        // goes to the direct path), and the direct path's list (int4 entries).
        // Only the filled part of a bucket is ever touched.
        const int64_t mean = (n + ntiles - 1) / ntiles;
        int64_t cap = std::min<int64_t>(std::max<int64_t>(16 * mean, 1024), std::max<int64_t>(n, 64));
        cap = (cap + 63) & ~(int64_t)63;
        if ((int64_t)ntiles * cap >= ((int64_t)1 << 31)) cap = (((int64_t)1 << 31) - 1) / ntiles & ~(int64_t)63;
        if (cap < 64) throw Fail{MVS_E_UNSUPPORTED, "image too large for the tile buckets"};
        ctx->t_cand.ensure((size_t)2 * ntiles * cap + 4 * (size_t)n);
        t.ntiles = ntiles;
        t.cap = (int)cap;
        t.chunk = grouped ? MVS_GROUP_CHUNK : MVS_MMA_CHUNK;
        t.groups = groups;
        // this batch's counter set; k_bin zeroes the other (the previous
        // batch's) for the next batch
        int32_t* set = ctx->t_tiles.p + ctx->tiles_parity * set_words;
        t.tile_count = set;
        int32_t* ctl = set + (int64_t)ntiles * kTcStride;   // one 128-B line per counter
        t.head = ctl;
        t.fix_count = ctl + 32;
        t.n_items = ctl + 96;
        t.zero_blk = ctx->t_tiles.p + (1 - ctx->tiles_parity) * set_words;
        t.zero_words = set_words;
        t.sorted = (int2*)ctx->t_cand.p;
        t.fix_list = (int4*)(ctx->t_cand.p + 2 * (size_t)ntiles * cap);
        // at most one partial chunk per tile beyond the full ones, in any one
        // of the kItemSegs segments
        t.item_seg = (int)(n / std::max(t.chunk, 1) + ntiles + 2);
        ctx->t_items.ensure((size_t)kItemSegs * t.item_seg);
        t.items = ctx->t_items.p;
        t.zero_first = ctx->tiles_clean_ntiles != ntiles ? 1 : 0;
        t.grid = ctx->scorer_wgs;
        t.stats = ctx->d_stats.p;
        // the runs path's buffers, where the batch is small enough for it (the
        // launcher decides; every element read is written by k_bin)
        const int64_t nbin = (n + MVS_BIN_CHUNK - 1) / MVS_BIN_CHUNK;
        t.runs_max = std::min(ctx->runs_max, kRunsLimit);
        if (nbin <= t.runs_max) {
            ctx->t_runs.ensure((size_t)nbin * MVS_BIN_CHUNK);
            ctx->t_offs.ensure((size_t)nbin * (ntiles + 1));
            t.runs = ctx->t_runs.p;
            t.offs = ctx->t_offs.p;
        }
        ctx->tiles_clean_ntiles = -1;            // dirty until the sequence is queued
        hipEvent_t e0, e1;
        ctx->next_events(&e0, &e1);
        ctx->scratch_acquire(s);
        const bool tab = ctx->ensure_moments(wid, s);
        const MomentsDev mt = ctx->moments(wid);
        if (mvs_tiled_uses_runs(&ctx->sc, &a, &t, tab ? &mt : nullptr)) ++ctx->runs_batches;
        const int rc = mvs_launch_score_tiled(&ctx->sc, &a, &t, wid, tab ? &mt : nullptr, s, e0, e1);
        if (rc != 0) throw Fail{rc == -3 ? MVS_E_UNSUPPORTED : MVS_E_HIP, "tiled score launch failed"};
        ctx->scratch_release(s);
        if (e0) ctx->timed_name = mvs_timed_kernel_name(ctx->V, wid, tab && !grouped ? 2 : 1);
        ctx->tiles_clean_ntiles = ntiles;        // the next batch's set was zeroed by this k_bin
        ctx->tiles_parity ^= 1;
        return;
    }
    hipEvent_t e0, e1;
    ctx->next_events(&e0, &e1);
    if (mvs_launch_score(&ctx->sc, &a, wid, s, e0, e1) != 0) throw Fail{MVS_E_HIP, "score launch failed"};
    if (e0) ctx->timed_name = mvs_timed_kernel_name(ctx->V, wid, 0);
}

extern "C" {

const char* mvs_version(void) { return "mvs_amd 0.1 (gfx950)"; }

const char* mvs_last_error(const mvs_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_err.c_str();
}

int mvs_ctx_create(int device, int V, int H, int W, const uint8_t* rgb, const double* K,
                   const double* R, const double* t, const double* Rp, mvs_ctx** out) {
    if (!out || !rgb || !K || !R || !t) return set_err(nullptr, Fail{MVS_E_ARG, "null argument"});
    *out = nullptr;
    if (V < 1 || V > MVS_MAX_VIEWS || H < 16 || W < 16 || H > 65536 || W > 65536)
        return set_err(nullptr, Fail{MVS_E_UNSUPPORTED, "need 1 <= V <= 256 and 16 <= H, W <= 65536"});
    std::unique_ptr<mvs_ctx> ctx(new mvs_ctx());
    ctx->device = device;
    int rc = guarded(ctx.get(), [&]() {
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) throw Fail{MVS_E_ARG, "no such HIP device"};
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->V = V; ctx->H = H; ctx->W = W;
        ctx->Wq = (W + 3) / 4 + 1;   // +1 zero quad: the last aligned dword read of a row
        const int64_t npx = (int64_t)V * H * W;
        ctx->h_rgb.assign(rgb, rgb + npx * 3);
        ctx->d_rgb.alloc(npx * 3);
        HIPCHK(hipMemcpyAsync(ctx->d_rgb.p, rgb, npx * 3, hipMemcpyHostToDevice, ctx->stream));
        const int64_t stack_bytes = (int64_t)H * ctx->Wq * V * 4;
        ctx->d_stack.alloc(stack_bytes + 64);
        HIPCHK(hipMemsetAsync(ctx->d_stack.p, 0, stack_bytes + 64, ctx->stream));
        // view-major copy: 8 zero bytes left of column 0, >= 24 right of W-1,
        // pitch a multiple of 16 (SceneDev)
        ctx->sc.Wp = (W + 32 + 15) & ~15;
        const int64_t gv_bytes = (int64_t)V * H * ctx->sc.Wp + 64;
        ctx->d_gv.alloc(gv_bytes);
        HIPCHK(hipMemsetAsync(ctx->d_gv.p, 0, gv_bytes, ctx->stream));
        ctx->sc.V = V; ctx->sc.H = H; ctx->sc.W = W; ctx->sc.Wq = ctx->Wq;
        ctx->sc.row_bytes = (int64_t)ctx->Wq * V * 4;
        ctx->sc.stack = ctx->d_stack.p;
        ctx->sc.rgb = ctx->d_rgb.p;
        ctx->sc.gv = ctx->d_gv.p + 8;
        if (mvs_launch_build_scene(&ctx->sc, ctx->d_rgb.p, ctx->d_stack.p, ctx->d_gv.p, ctx->stream) != 0)
            throw Fail{MVS_E_HIP, "build_scene launch failed"};
        build_cameras(ctx.get(), K, R, t, Rp);
        ctx->K.assign(K, K + 9 * V);
        ctx->d_cams.alloc(V);
        HIPCHK(hipMemcpyAsync(ctx->d_cams.p, ctx->cams.data(), V * sizeof(CamDev), hipMemcpyHostToDevice, ctx->stream));
        ctx->d_exact.alloc(1);
        HIPCHK(hipMemsetAsync(ctx->d_exact.p, 0, sizeof(int32_t), ctx->stream));
        ctx->d_stats.alloc(4);
        HIPCHK(hipMemsetAsync(ctx->d_stats.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->sc.cams = ctx->d_cams.p;
        if (const char* km = std::getenv("MVS_SCORE_KERNEL")) {
            if (!std::strcmp(km, "direct")) ctx->kernel_mode = 1;
            else if (!std::strcmp(km, "tiled")) ctx->kernel_mode = 2;
            else if (!std::strcmp(km, "mma")) ctx->tab_mode = 1;   // tiled, in-kernel moments
            else if (!std::strcmp(km, "tab")) ctx->tab_mode = 2;   // tiled, tables at every V
        }
        if (const char* sw = std::getenv("MVS_SCORER_WGS")) ctx->scorer_wgs = std::max(0, std::atoi(sw));
        if (const char* tl = std::getenv("MVS_TAB_LIMIT")) ctx->tab_limit = std::max<int64_t>(1, std::atoll(tl));
        // the binning path: MVS_BIN=atomic keeps the atomic tile buckets
        // everywhere; MVS_BIN_RUNS_MAX: the most runs (binning workgroups)
        // the runs path is taken for
        if (const char* rm = std::getenv("MVS_BIN_RUNS_MAX")) ctx->runs_max = std::min(std::max(0, std::atoi(rm)), kRunsLimit);
        if (const char* bm = std::getenv("MVS_BIN"))
            if (!std::strcmp(bm, "atomic")) ctx->runs_max = 0;
        return 0;
    });
    if (rc != 0) {
        g_err = ctx->err;
        return rc;
    }
    *out = ctx.release();
    return 0;
}

void mvs_ctx_destroy(mvs_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // the scratch's last users may be any streams (some perhaps destroyed by now)
    if (ctx->scratch_order.used || ctx->pack_order.used || ctx->wexp_order.used || ctx->wmesh_order.used)
        (void)hipDeviceSynchronize();
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
    if (ctx->scratch_order.ev) (void)hipEventDestroy(ctx->scratch_order.ev);
    if (ctx->pack_order.ev) (void)hipEventDestroy(ctx->pack_order.ev);
    if (ctx->wexp_order.ev) (void)hipEventDestroy(ctx->wexp_order.ev);
    if (ctx->wmesh_order.ev) (void)hipEventDestroy(ctx->wmesh_order.ev);
    delete ctx;
}

int mvs_kernel_timing(mvs_ctx* ctx, int enable) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    return guarded(ctx, [&]() {
        if (enable < 0) throw Fail{MVS_E_ARG, "timing period must be >= 0"};
        ctx->timing = enable != 0;
        if (ctx->timing) {
            ctx->ev_used = 0;   // disabling keeps the record readable
            ctx->timing_period = enable;
            ctx->timing_count = 0;
        }
        return 0;
    });
}

int mvs_kernel_time(mvs_ctx* ctx, double* total_ms, int64_t* launches) {
    if (!ctx || !total_ms || !launches) return set_err(ctx, Fail{MVS_E_ARG, "bad arguments"});
    return guarded(ctx, [&]() {
        double tot = 0.0;
        for (size_t k = 0; k + 1 < ctx->ev_used; k += 2) {
            HIPCHK(hipEventSynchronize(ctx->ev[k + 1]));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ctx->ev[k], ctx->ev[k + 1]));
            tot += ms;
        }
        *total_ms = tot;
        *launches = (int64_t)(ctx->ev_used / 2);
        return 0;
    });
}

const char* mvs_timed_kernel(const mvs_ctx* ctx) { return ctx ? ctx->timed_name : ""; }

int mvs_ctx_rebuild(mvs_ctx* ctx, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        if (mvs_launch_build_scene(&ctx->sc, ctx->d_rgb.p, ctx->d_stack.p, ctx->d_gv.p, s) != 0)
            throw Fail{MVS_E_HIP, "build_scene launch failed"};
        // the window-moment tables built so far follow the scene
        for (int w = 1; w <= MVS_MAX_WID; ++w)
            if (ctx->mom_ok[w]) {
                const MomentsDev m = ctx->moments(w);
                if (mvs_launch_moments(&ctx->sc, &m, s) != 0) throw Fail{MVS_E_HIP, "moments launch failed"};
            }
        return 0;
    });
}

int mvs_ctx_set_images(mvs_ctx* ctx, int first_view, int n_views, const uint8_t* rgb) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    return guarded(ctx, [&]() {
        if (first_view < 0 || n_views < 0 || first_view > ctx->V - n_views) throw Fail{MVS_E_ARG, "views out of range"};
        if (n_views == 0) return 0;
        if (!rgb) throw Fail{MVS_E_ARG, "null argument"};
        const int64_t per = (int64_t)ctx->H * ctx->W * 3;
        HIPCHK(hipMemcpyAsync(ctx->d_rgb.p + first_view * per, rgb, n_views * per, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->h_rgb.data() + first_view * per, rgb, (size_t)(n_views * per));
        return 0;
    });
}

int mvs_ctx_rproj(const mvs_ctx* ctx, double* Rp) {
    if (!ctx || !Rp) return MVS_E_ARG;
    for (int v = 0; v < ctx->V; ++v) std::memcpy(Rp + 9 * v, ctx->cams[v].Rp, 9 * sizeof(double));
    return 0;
}

int mvs_score_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, int wid,
                     double min_ncc, double* d_xy, uint64_t* d_mask, int32_t* d_count,
                     double* d_avg, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (n < 0) return set_err(ctx, Fail{MVS_E_ARG, "n < 0"});
    if (n > 0 && (!d_c || !d_ref || !d_xy || !d_mask || !d_count))
        return set_err(ctx, Fail{MVS_E_ARG, "null device pointer"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        score_device(ctx, n, d_c, d_ref, wid, min_ncc, d_xy, d_mask, d_count, d_avg, s);
        return 0;
    });
}

int mvs_score_device_rec(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, int wid,
                         double min_ncc, double* d_xy, int64_t* d_rec, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (n < 0 || (n > 0 && (!d_c || !d_ref || !d_xy || !d_rec)) || ((uintptr_t)d_rec & 15) != 0)
        return set_err(ctx, Fail{MVS_E_ARG, "bad arguments (records must be 16-B aligned)"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        score_device(ctx, n, d_c, d_ref, wid, min_ncc, d_xy, (uint64_t*)d_rec, nullptr, nullptr, s);
        return 0;
    });
}

int mvs_pack_accepted(mvs_ctx* ctx, int64_t n, int64_t offset, const int32_t* d_count, const uint64_t* d_mask,
                      const double* d_c, int vlb, int64_t cap, int64_t* d_out, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (n < 0 || cap < 0 || !d_out || (n > 0 && !d_mask))
        return set_err(ctx, Fail{MVS_E_ARG, "bad arguments"});
    return guarded(ctx, [&]() {
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        // the pack's own scratch (counter, ticket): ordered against the
        // previous pack only, so that a pack on a communication stream does
        // not order the next sweep's scoring behind it
        ctx->pack_order.acquire(s);
        if (!ctx->p_ctl.p) {
            ctx->p_ctl.ensure(32);
            HIPCHK(hipMemsetAsync(ctx->p_ctl.p, 0, 32 * sizeof(unsigned long long), s));
        }
        if (mvs_launch_pack_accepted(n, offset, d_count, d_mask, d_c, ctx->words(), vlb, cap, ctx->p_ctl.p, d_out,
                                     s) != 0)
            throw Fail{MVS_E_HIP, "pack launch failed"};
        ctx->pack_order.release(s);
        return 0;
    });
}

int mvs_proxy_copy(void* d_dst, const void* d_src, int64_t bytes, int workgroups, void* stream) {
    if (bytes < 0 || (bytes % 16) != 0 || workgroups < 1 || (bytes > 0 && (!d_dst || !d_src)))
        return set_err(nullptr, Fail{MVS_E_ARG, "bad arguments"});
    if (mvs_launch_proxy_copy(d_dst, d_src, bytes, workgroups, (hipStream_t)stream) != 0)
        return set_err(nullptr, Fail{MVS_E_HIP, "proxy copy launch failed"});
    return 0;
}

int mvs_set_scorer_grid(mvs_ctx* ctx, int workgroups) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (workgroups < 0) return set_err(ctx, Fail{MVS_E_ARG, "workgroups must be >= 0"});
    ctx->scorer_wgs = workgroups;
    return 0;
}

int mvs_score(mvs_ctx* ctx, int64_t n, const double* c, const int32_t* ref, int wid, double min_ncc,
              double* xy, uint64_t* mask, int32_t* count, double* avg) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (n < 0 || (n > 0 && (!c || !ref || !xy || !mask || !count || !avg)))
        return set_err(ctx, Fail{MVS_E_ARG, "bad arguments"});
    return guarded(ctx, [&]() {
        for (int64_t i = 0; i < n; ++i)
            if (ref[i] < 0 || ref[i] >= ctx->V) throw Fail{MVS_E_ARG, "ref view out of range"};
        if (n == 0) return 0;
        hipStream_t s = ctx->stream;
        const int words = ctx->words();
        Staging& st = ctx->staging.begin(s);
        const auto d_c = st.in(c, n * 3);
        const auto d_ref = st.in(ref, n);
        const auto d_xy = st.out(xy, n * 2);
        const auto d_mask = st.out(mask, n * words);
        const auto d_count = st.out(count, n);
        const auto d_avg = st.out(avg, n);
        st.upload();
        score_device(ctx, n, d_c, d_ref, wid, min_ncc, d_xy, d_mask, d_count, d_avg, s);
        st.finish();
        return 0;
    });
}

int64_t mvs_exact_hits(mvs_ctx* ctx) {
    if (!ctx) return MVS_E_ARG;
    int32_t h = 0;
    int rc = guarded(ctx, [&]() {
        HIPCHK(hipMemcpyAsync(&h, ctx->d_exact.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return 0;
    });
    return rc ? rc : h;
}

int mvs_stream_retiring(mvs_ctx* ctx, void* stream) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (!stream) return 0;   // the library's own stream is never retired by a caller
    return guarded(ctx, [&]() {
        ctx->scratch_order.retire((hipStream_t)stream);
        ctx->pack_order.retire((hipStream_t)stream);
        ctx->wexp_order.retire((hipStream_t)stream);
        ctx->wmesh_order.retire((hipStream_t)stream);
        return 0;
    });
}

int mvs_scorer_stats(mvs_ctx* ctx, int64_t* out) {
    if (!ctx || !out) return set_err(ctx, Fail{MVS_E_ARG, "null argument"});
    return guarded(ctx, [&]() {
        unsigned long long h[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(h, ctx->d_stats.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int k = 0; k < 3; ++k) out[k] = (int64_t)h[k];
        return 0;
    });
}

int64_t mvs_bin_runs_batches(mvs_ctx* ctx) { return ctx ? ctx->runs_batches : 0; }

int mvs_ncc_windows(int64_t n, int npx, const uint8_t* d_a, const uint8_t* d_b, double thr,
                    int force_exact, double* d_ncc, uint8_t* d_pass, void* stream) {
    if (npx < 1 || npx > 128) return set_err(nullptr, Fail{MVS_E_UNSUPPORTED, "npx must be in 1..128"});
    int rc = mvs_launch_ncc_windows(n, npx, d_a, d_b, thr, force_exact, d_ncc, d_pass, (hipStream_t)stream);
    if (rc) return set_err(nullptr, Fail{MVS_E_HIP, "ncc_windows launch failed"});
    return 0;
}

int mvs_exact_avg(mvs_ctx* ctx, int64_t n, const int32_t* ref, const double* xy, const uint64_t* mask, int wid,
                  double* avg) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    if (n < 0 || (n > 0 && (!ref || !xy || !mask || !avg))) return set_err(ctx, Fail{MVS_E_ARG, "bad arguments"});
    if (wid != 3 && wid != 5) return set_err(ctx, Fail{MVS_E_UNSUPPORTED, "exact avg supports wid 3 or 5"});
    return guarded(ctx, [&]() {
        const int words = ctx->words();
        for (int64_t i = 0; i < n; ++i) {
            if (ref[i] < 0 || ref[i] >= ctx->V) throw Fail{MVS_E_ARG, "ref view out of range"};
            // a V list names other views (MVS2.py:66-67) inside the scene; a
            // non-empty one needs a valid window (HarrisFeatures.py:128)
            bool any = false;
            for (int w = 0; w < words; ++w) {
                uint64_t m = mask[i * words + w];
                const int nv = ctx->V - 64 * w;
                if (nv < 64 && (m >> nv)) throw Fail{MVS_E_ARG, "mask names a view >= V"};
                if (ref[i] / 64 == w && ((m >> (ref[i] % 64)) & 1ull))
                    throw Fail{MVS_E_ARG, "mask names the reference view itself"};
                any |= m != 0;
            }
            if (any) {
                const double x = xy[2 * i], y = xy[2 * i + 1];
                if (!(x > -1e9 && x < 1e9 && y > -1e9 && y < 1e9)) throw Fail{MVS_E_ARG, "non-finite projection"};
                const int q = (int)x, r = (int)y;
                if (!(r - wid >= 0 && r + wid + 1 < ctx->H && q - wid > 0 && q + wid + 1 < ctx->W))
                    throw Fail{MVS_E_ARG, "mask bits set for a window outside the image"};
            }
        }
        if (n == 0) return 0;
        hipStream_t s = ctx->stream;
        Staging& st = ctx->staging.begin(s);
        const auto d_ref = st.in(ref, n);
        const auto d_xy = st.in(xy, n * 2);
        const auto d_mask = st.in(mask, n * words);
        const auto d_avg = st.out(avg, n);
        st.upload();
        RecordsDev rec{};
        rec.R = d_ref;
        rec.xy = d_xy;
        rec.mask = d_mask;
        if (mvs_launch_exact_avg(&ctx->sc, rec, wid, nullptr, n, d_avg, s) != 0)
            throw Fail{MVS_E_HIP, "exact_avg launch failed"};
        st.finish();
        return 0;
    });
}

// ---- SfM front-end (HarrisFeatures.py, SFM.py) ----

int mvs_harris_points(mvs_ctx* ctx, int view, int32_t* out, int64_t cap, int64_t* n_out) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    return guarded(ctx, [&]() -> int {
        if (!n_out || (cap > 0 && !out)) throw Fail{MVS_E_ARG, "null output"};
        if (view < 0 || view >= ctx->V) throw Fail{MVS_E_ARG, "view out of range"};
        // BORDER_REFLECT_101 of a 3x3 Sobel needs two pixels per axis
        if (ctx->H < 2 || ctx->W < 2) throw Fail{MVS_E_UNSUPPORTED, "Harris needs images of at least 2x2"};
        const int64_t npx = (int64_t)ctx->H * ctx->W;
        ctx->f_resp.ensure(npx);
        ctx->f_dil.ensure(npx);
        ctx->f_key.ensure(1);
        ctx->f_rows.ensure(2 * (size_t)ctx->H + 1);
        hipStream_t s = ctx->stream;
        int32_t* rowcnt = ctx->f_rows.p;
        int32_t* rowoff = ctx->f_rows.p + ctx->H;
        if (mvs_launch_harris(&ctx->sc, view, 0.04, ctx->f_resp.p, ctx->f_dil.p, ctx->f_key.p, rowcnt,
                              rowoff, s) != 0)
            throw Fail{MVS_E_HIP, "harris launch failed"};
        int32_t total = 0;
        HIPCHK(hipMemcpyAsync(&total, rowoff + ctx->H, sizeof total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        *n_out = total;
        const int64_t m = std::min<int64_t>(total, cap);
        if (m > 0) {
            ctx->f_pts.ensure(2 * (size_t)total);
            if (mvs_launch_harris_write(&ctx->sc, ctx->f_dil.p, ctx->f_key.p, rowoff, ctx->f_pts.p, total,
                                        s) != 0)
                throw Fail{MVS_E_HIP, "harris write launch failed"};
            HIPCHK(hipMemcpyAsync(out, ctx->f_pts.p, 2 * m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        return 0;
    });
}

int mvs_match_two_sided(mvs_ctx* ctx, int view_a, const int32_t* pts_a, int64_t n_a, int view_b,
                        const int32_t* pts_b, int64_t n_b, int wid, double thr, int32_t* m12,
                        int32_t* best12, int32_t* best21) {
    if (!ctx) return set_err(nullptr, Fail{MVS_E_ARG, "null context"});
    return guarded(ctx, [&]() -> int {
        if (n_a < 0 || n_b < 0 || (n_a && (!pts_a || !m12)) || (n_b && !pts_b))
            throw Fail{MVS_E_ARG, "bad point arrays"};
        if (view_a < 0 || view_a >= ctx->V || view_b < 0 || view_b >= ctx->V)
            throw Fail{MVS_E_ARG, "view out of range"};
        if (wid < 1 || (2 * wid + 1) * (2 * wid + 1) > 128) throw Fail{MVS_E_UNSUPPORTED, "wid must be 1..5"};
        // getDescFeatures keeps only windows inside these bounds (HarrisFeatures.py:128)
        for (int side = 0; side < 2; ++side) {
            const int32_t* p = side ? pts_b : pts_a;
            const int64_t n = side ? n_b : n_a;
            for (int64_t i = 0; i < n; ++i) {
                const int r = p[2 * i], c = p[2 * i + 1];
                if (!(r - wid >= 0 && r + wid + 1 < ctx->H && c - wid > 0 && c + wid + 1 < ctx->W))
                    throw Fail{MVS_E_ARG, "point outside getDescFeatures' bounds"};
            }
        }
        if (n_a == 0) {
            // no A row: every B row's dist row is empty, so no match
            if (best21) std::fill(best21, best21 + n_b, -1);
            return 0;
        }
        const int npx = (2 * wid + 1) * (2 * wid + 1);
        constexpr int DW = 32;   // descriptor dwords (kDescWords)
        const int64_t n = n_a + n_b;
        ctx->f_pts.ensure(2 * (size_t)n);
        ctx->f_desc.ensure((size_t)DW * n + 4);
        ctx->f_mom.ensure(2 * (size_t)n);
        ctx->f_best.ensure((size_t)n);
        hipStream_t s = ctx->stream;
        HIPCHK(hipMemcpyAsync(ctx->f_pts.p, pts_a, 2 * n_a * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (n_b)
            HIPCHK(hipMemcpyAsync(ctx->f_pts.p + 2 * n_a, pts_b, 2 * n_b * sizeof(int32_t),
                                  hipMemcpyHostToDevice, s));
        uint32_t* dA = ctx->f_desc.p;
        uint32_t* dB = ctx->f_desc.p + (size_t)DW * n_a;
        int32_t* S = ctx->f_mom.p;
        int32_t* SS = ctx->f_mom.p + n;
        if (mvs_launch_gather_desc(&ctx->sc, view_a, ctx->f_pts.p, n_a, wid, dA, S, SS, s) != 0 ||
            mvs_launch_gather_desc(&ctx->sc, view_b, ctx->f_pts.p + 2 * n_a, n_b, wid, dB, S + n_a,
                                   SS + n_a, s) != 0)
            throw Fail{MVS_E_HIP, "descriptor launch failed"};
        int32_t* b12 = ctx->f_best.p;
        int32_t* b21 = ctx->f_best.p + n_a;
        if (mvs_launch_match_rows(dA, S, SS, n_a, dB, S + n_a, SS + n_a, n_b, npx, thr, b12, s) != 0 ||
            mvs_launch_match_rows(dB, S + n_a, SS + n_a, n_b, dA, S, SS, n_a, npx, thr, b21, s) != 0)
            throw Fail{MVS_E_HIP, "match launch failed"};
        std::vector<int32_t> h12(n_a), h21(n_b);
        HIPCHK(hipMemcpyAsync(h12.data(), b12, n_a * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (n_b) HIPCHK(hipMemcpyAsync(h21.data(), b21, n_b * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        // MatchTwoSided's symmetric check (HarrisFeatures.py:60-64)
        for (int64_t i = 0; i < n_a; ++i) {
            const int32_t j = h12[i];
            m12[i] = (j >= 0 && h21[j] == (int32_t)i) ? j : -1;
        }
        if (best12) std::copy(h12.begin(), h12.end(), best12);
        if (best21) std::copy(h21.begin(), h21.end(), best21);
        return 0;
    });
}


}  // extern "C"
