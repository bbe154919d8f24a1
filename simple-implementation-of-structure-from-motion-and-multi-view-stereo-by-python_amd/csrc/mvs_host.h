// What the host sources of libmvs_amd.so share: the error type, the device
// buffer, the host-pointer calls' staging arena, the context and the helpers
// defined in one source and called from another.  None of it is part of the
// library's dynamic interface: every declaration has hidden visibility.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/mvs_amd.h"
#include "mvs_internal.h"

#pragma GCC visibility push(hidden)

struct Fail {
    int code;
    std::string msg;
};

#define HIPCHK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess)                                                             \
            throw Fail{MVS_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)};        \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        HIPCHK(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
    }
    void ensure(size_t count) {
        if (count > n) alloc(std::max(count, n * 2));
    }
    // grow preserving the first `keep` elements
    void grow(size_t count, size_t keep, hipStream_t s) {
        if (count <= n) return;
        T* q = nullptr;
        size_t nn = std::max(count, n * 2);
        HIPCHK(hipMalloc((void**)&q, nn * sizeof(T)));
        if (p && keep) HIPCHK(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        release();
        p = q;
        n = nn;
    }
};

// The device copies of one host-pointer call: a bump allocator over one
// buffer.  A call names its arrays (in, out, tmp), then upload() sizes the
// buffer once for all of them and queues the copies in; a Slot gives its
// device pointer only after that, so no pointer outlives a growth.  finish()
// queues the copies out and synchronises.  Such calls run on ctx->stream, one
// at a time, and end synchronised: they share the buffer and its high-water mark.
struct Staging {
    static constexpr size_t kAlign = 256, kNone = ~(size_t)0;   // k_wexp_claim reads its jobs as int4
    template <class T>
    struct Slot {
        const Staging* st;
        size_t off;
        operator T*() const { return off == kNone ? nullptr : (T*)(st->base() + off); }
    };
    struct Copy {
        size_t off;
        void* host;
        size_t bytes;
    };
    DevBuf<unsigned char> buf;
    hipStream_t s = nullptr;
    size_t total = 0;
    bool placed = false;
    std::vector<Copy> ins, outs;

    Staging& begin(hipStream_t stream) {
        s = stream;
        total = 0;
        placed = false;
        ins.clear();
        outs.clear();
        return *this;
    }
    unsigned char* base() const {
        if (!placed) throw Fail{MVS_E_ARG, "staging slot used before upload"};
        return buf.p;
    }
    template <class T>
    Slot<T> tmp(size_t count) {
        if (placed) throw Fail{MVS_E_ARG, "staging slot reserved after upload"};
        const size_t off = total;
        total += (count * sizeof(T) + kAlign - 1) & ~(kAlign - 1);
        return Slot<T>{this, off};
    }
    // a null host array is not copied: its slot holds whatever the buffer does
    template <class T>
    Slot<T> in(const T* host, size_t count) {
        const Slot<T> r = tmp<T>(count);
        if (host && count) ins.push_back(Copy{r.off, const_cast<T*>(host), count * sizeof(T)});
        return r;
    }
    // a null host array (an optional output) gets no slot: a null device pointer
    template <class T>
    Slot<T> out(T* host, size_t count) {
        if (!host) return Slot<T>{this, kNone};
        const Slot<T> r = tmp<T>(count);
        if (count) outs.push_back(Copy{r.off, host, count * sizeof(T)});
        return r;
    }
    void upload() {
        buf.ensure(total);
        placed = true;
        for (const Copy& c : ins) HIPCHK(hipMemcpyAsync(buf.p + c.off, c.host, c.bytes, hipMemcpyHostToDevice, s));
    }
    void finish() {
        for (const Copy& c : outs) HIPCHK(hipMemcpyAsync(c.host, buf.p + c.off, c.bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
};

// Small host tables a stream-ordered *_device call hands to its kernels (the
// seed matcher's pairs and blocks): a pinned host copy, so the upload is a true
// asynchronous copy, and the event of the last upload, which the next fill
// waits for before it rewrites the host copy.
struct PinnedTable {
    unsigned char* p = nullptr;
    size_t n = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    PinnedTable() = default;
    PinnedTable(const PinnedTable&) = delete;
    PinnedTable& operator=(const PinnedTable&) = delete;
    ~PinnedTable() {
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
    }
    // room for `bytes`, the previous upload complete
    unsigned char* fill(size_t bytes) {
        if (pending) HIPCHK(hipEventSynchronize(ev));
        pending = false;
        if (bytes > n) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            n = 0;
            HIPCHK(hipHostMalloc((void**)&p, std::max(bytes, (size_t)4096), hipHostMallocDefault));
            n = std::max(bytes, (size_t)4096);
        }
        return p;
    }
    void upload(void* dst, size_t bytes, hipStream_t s) {
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHK(hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(ev, s));
        pending = true;
    }
};

// OpenCV-order geometry (mvs_geometry.cpp)
void rodrigues_roundtrip(const double* Rin, double* Rout);
void triangulate(const double* P1, const double* P2, const double* x1, const double* x2, double* X4);

inline double fma_dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    // numpy 3-element dot / matvec row as OpenBLAS 0.3.29 evaluates it
    return std::fma(a2, b2, std::fma(a1, b1, a0 * b0));
}

inline int py_wrap(long i, long n) { return (int)(i < 0 ? i + n : i); }

// ---------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------

// the public header's opaque type: default visibility, as its declaration there
#pragma GCC visibility pop
struct mvs_ctx {
    int device = 0;
    int stage_flags = 0;   // mvs_stage_set_options
    int V = 0, H = 0, W = 0, Wq = 0;
    hipStream_t stream = nullptr;
    std::vector<CamDev> cams;
    std::vector<double> K;   // V*9 as given (getProjectionMatrix uses all of K)
    std::vector<uint8_t> h_rgb;
    DevBuf<uint8_t> d_rgb, d_stack, d_gv;
    DevBuf<CamDev> d_cams;
    DevBuf<int32_t> d_exact;
    DevBuf<unsigned long long> d_stats;   // mvs_scorer_stats (k_score_fix)
    SceneDev sc{};
    // every host-pointer call's device copies (on `stream` only; the *_device
    // calls of the warped test, refinement, lists and filter keep no state)
    Staging staging;
    // the warped expansion's scratch (ordered by wexp_order): the children's
    // per-patch counts and offsets and the claim's per-(view, cell) key and
    // ticket grids (zero between calls)
    DevBuf<int32_t> x_cnt;
    DevBuf<int64_t> x_offs;
    DevBuf<uint64_t> x_key;
    DevBuf<uint32_t> x_ticket;
    // the seed matcher's pair and block tables (mvs_wseed_match; it shares
    // x_cnt, x_offs and wexp_order with the expansion)
    PinnedTable s_tab_h;
    DevBuf<unsigned char> s_tab;
    // the mesh extraction's scratch (mvs_wmesh_extract, ordered by wmesh_order):
    // the points' used-edge masks and first vertices, the workgroups' vertex and
    // triangle counts
    DevBuf<uint32_t> m_mask;
    DevBuf<int32_t> m_voff;
    DevBuf<int64_t> m_sums;
    // tiled scorer scratch
    DevBuf<int32_t> t_tiles, t_cand;
    // mvs_pack_accepted: the pack's row counter and chunk ticket (k_acc_pack
    // leaves both zero)
    DevBuf<unsigned long long> p_ctl;
    DevBuf<int4> t_items;
    // the runs path's scratch (mvs_internal.h) and the most binning
    // workgroups it is taken for (env MVS_BIN=atomic: 0; MVS_BIN_RUNS_MAX)
    DevBuf<int2> t_runs;
    DevBuf<uint16_t> t_offs;
    int runs_max = kRunsLimit;
    int64_t runs_batches = 0;   // tiled batches binned into runs (mvs_bin_runs_batches)
    // SfM front-end scratch (Harris maps, descriptors, match rows)
    DevBuf<float> f_resp, f_dil;
    DevBuf<uint32_t> f_key, f_desc;
    DevBuf<int32_t> f_rows, f_pts, f_mom, f_best;
    int kernel_mode = 0;   // 0 auto, 1 direct, 2 tiled (env MVS_SCORE_KERNEL)
    // the tiled scorer's window moments: per wid, built on first use
    // (k_moments), rebuilt with the scene; tab_mode 0 = tables when they fit
    // (ring256 with tile-order items: 1.52 ms per 2^20 against 1.67-1.69 ms
    // for the in-kernel Q table), 1 = never (in-kernel moments; env
    // MVS_SCORE_KERNEL=mma), 2 = tables (env MVS_SCORE_KERNEL=tab)
    int tab_mode = 0;
    int scorer_wgs = 0;   // env MVS_SCORER_WGS: k_score_tab's grid (0 = every CU, twice)
    DevBuf<int16_t> mom_sb[MVS_MAX_WID + 1];
    DevBuf<double> mom_w[MVS_MAX_WID + 1];     // V <= 64
    DevBuf<int32_t> mom_d[MVS_MAX_WID + 1];    // V > 64 (moments_dtab)
    DevBuf<uint16_t> mom_flat[MVS_MAX_WID + 1];   // constant-window bits (MomentsDev.flat)
    bool mom_ok[MVS_MAX_WID + 1] = {};
    int moments_vp() const { return V > MVS_GROUP_VIEWS ? 64 * ((V + 63) / 64) : 16 * ((V + 15) / 16); }
    MomentsDev moments(int wid) const {
        MomentsDev m{};
        m.sb = mom_sb[wid].p;
        m.w = mom_w[wid].p;
        m.d = mom_d[wid].p;
        m.flat = mom_flat[wid].p;
        m.VP = moments_vp();
        m.wid = wid;
        return m;
    }
    // the tables of wid (10 B per (pixel, view) at V <= 64: S_b and w; 6 B at
    // V > 64: S_b and D), built on stream s if needed; false when they do not
    // apply (disabled, or more than 2^31 elements).  One row of 16 pixels
    // past the end: k_score_tab stages a tile's rows whole (16 pixels x VP),
    // also where the last tile column runs past W
    // Memory: (H W + 16) VP elements per wid, 10 B each at V <= 64 (S_b int16
    // + w binary64) or 6 B at V > 64
    // (S_b + D int32): 147 MB per wid at dinoRing, 3.2 GB at 256 x 1920 x 1080.  A scene past tab_limit elements (2^31;
    // env MVS_TAB_LIMIT lowers it, for tests) or whose tables cannot be
    // allocated is scored with the in-kernel moments instead (same results).
    int64_t tab_limit = (int64_t)1 << 31;
    bool ensure_moments(int wid, hipStream_t s) {
        if (tab_mode == 1) return false;
        const int64_t elems = ((int64_t)H * W + 16) * moments_vp();
        if (elems >= tab_limit) return false;
        if (!mom_ok[wid]) {
            try {
                mom_sb[wid].alloc((size_t)elems);
                if (moments_dtab(V)) mom_d[wid].alloc((size_t)elems);
                else mom_w[wid].alloc((size_t)elems);
                mom_flat[wid].alloc((size_t)(elems / 16));
            } catch (const Fail&) {
                mom_sb[wid].release();
                mom_d[wid].release();
                mom_w[wid].release();
                mom_flat[wid].release();
                (void)hipGetLastError();   // the failed hipMalloc's error is not this call's
                return false;
            }
            HIPCHK(hipMemsetAsync(mom_sb[wid].p, 0, (size_t)elems * sizeof(int16_t), s));
            HIPCHK(hipMemsetAsync(mom_flat[wid].p, 0, (size_t)(elems / 16) * sizeof(uint16_t), s));
            if (moments_dtab(V))
                HIPCHK(hipMemsetAsync(mom_d[wid].p, 0, (size_t)elems * sizeof(int32_t), s));
            else
                HIPCHK(hipMemsetAsync(mom_w[wid].p, 0, (size_t)elems * sizeof(double), s));
            const MomentsDev m = moments(wid);
            if (mvs_launch_moments(&sc, &m, s) != 0) throw Fail{MVS_E_HIP, "moments launch failed"};
            mom_ok[wid] = true;
        }
        return true;
    }
    int tiles_clean_ntiles = -1;   // the next batch's counter set known zero for this tile count (-1: unknown)
    int tiles_parity = 0;          // the counter set the next tiled batch uses
    // kernel timing (mvs_kernel_timing): one event pair per `timing_period`-th
    // scoring launch (an event record between two kernels costs a few us of
    // stream time, so a timed loop samples)
    bool timing = false;
    int timing_period = 1;
    int64_t timing_count = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    const char* timed_name = "";   // the kernel the last timed pair bracketed
    // The context's scratch (tiled-scorer counters and lists), the exchange
    // pack's status words and the warped expansion's grids may be used on any stream
    // a *_device call names: a call waits for the previous use when the
    // stream changes.  The event is recorded then, lazily, on the stream that
    // used the area last (its later work is waited for too): consecutive
    // calls on one stream enqueue nothing, where an event record after every
    // call cost the stream ~5 us of idle time before the next call's first
    // kernel (profiles/r05/r5d_kernel_trace.csv).  A stream destroyed since
    // its use cannot take the record: the whole device is synchronised then.
    struct StreamOrder {
        hipEvent_t ev = nullptr;
        hipStream_t s = nullptr;
        bool used = false;
        void acquire(hipStream_t cur) {
            if (!used || s == cur) return;
            if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            if (hipEventRecord(ev, s) != hipSuccess) {
                (void)hipGetLastError();
                HIPCHK(hipDeviceSynchronize());
                return;
            }
            HIPCHK(hipStreamWaitEvent(cur, ev, 0));
        }
        void release(hipStream_t cur) {
            s = cur;
            used = true;
        }
        // the stream st is about to be destroyed: its work on the area is
        // waited for now, so no later acquire records an event on it
        void retire(hipStream_t st) {
            if (!used || s != st) return;
            HIPCHK(hipStreamSynchronize(st));
            used = false;
            s = nullptr;
        }
    } scratch_order, pack_order, wexp_order, wmesh_order;
    std::string err;
    void scratch_acquire(hipStream_t s) { scratch_order.acquire(s); }
    void scratch_release(hipStream_t s) { scratch_order.release(s); }
    // next event pair while timing is on, else nulls
    void next_events(hipEvent_t* e0, hipEvent_t* e1) {
        *e0 = *e1 = nullptr;
        if (!timing) return;
        if (timing_count++ % timing_period) return;
        if (ev_used + 2 > ev.size()) {
            for (int k = 0; k < 2; ++k) {
                hipEvent_t e;
                // no system-scope fence at the record: no L2 writeback between
                // the timed kernels (the timestamps need none)
                HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
                ev.push_back(e);
            }
        }
        *e0 = ev[ev_used];
        *e1 = ev[ev_used + 1];
        ev_used += 2;
    }
    int words() const { return (V + 63) / 64; }
};
#pragma GCC visibility push(hidden)

// f becomes the context's and the thread's last error; returns f.code (mvs_context.cpp)
int set_err(mvs_ctx* ctx, const Fail& f);

template <class Fn>
int guarded(mvs_ctx* ctx, Fn&& fn) {
    try {
        if (ctx) HIPCHK(hipSetDevice(ctx->device));
        return fn();
    } catch (const Fail& f) {
        return set_err(ctx, f);
    } catch (const std::bad_alloc&) {
        return set_err(ctx, Fail{MVS_E_NOMEM, "host allocation failed"});
    } catch (const std::exception& e) {
        return set_err(ctx, Fail{MVS_E_ARG, e.what()});
    }
}

// the photo test of n candidates on stream s (mvs_context.cpp)
void score_device(mvs_ctx* ctx, int64_t n, const double* d_c, const int32_t* d_ref, int wid, double thr,
                  double* d_xy, uint64_t* d_mask, int32_t* d_count, double* d_avg, hipStream_t s);

#pragma GCC visibility pop
