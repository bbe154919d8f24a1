// HIP kernels of the direct path (gfx950 / CDNA4): scene build, the direct photo
// test, the tiled scorers' guard-band fix-up and expansion, which share the wave
// core below.  The tiled path: mvs_bin.hip, mvs_score_tab.hip, mvs_score_mma*.hip.
//
// Reference path (MarvinChung/simple-implementation-of-structure-from-motion-
// and-multi-view-stereo-by-python):
//   MyPatch.photo_consistenecy_test   MVS2.py:62-77   -> k_score_mma / k_score
//   projectPoint                      utils.py:241-244 -> project()
//   getDescFeatures                   HarrisFeatures.py:116-133 -> window gather
//   ctNcc                             MVS2.py:39-43   -> integer moments + exact_ncc_*
//   patch_expansion candidate geometry + accept test MVS2.py:329-369 -> k_expand*
//
// Numerics.  Window sums are exact integers (S_a, S_aa, S_b, S_bb, S_ab) and
// the NCC is n (n S_ab - S_a S_b) / ((n-1) sqrt((n S_aa - S_a^2)(n S_bb - S_b^2))).
// Every decision close to the threshold is taken again on the numpy-order
// ctNcc (exact_ncc_*), so every accept/reject is the reference's.  Geometry is
// binary64 in the reference's order; this file is compiled with
// -ffp-contract=off (products that numpy/OpenBLAS fuse are written as fma()).
#include <algorithm>

#include "mvs_device.h"

namespace {

// ctNcc of view R's and view v's windows at (q, r) in numpy's operation order
// (the guard-band path: rare).  Both windows' rows come in with every load in
// flight at once (one memory round trip), aligned to the window's first
// column (alignbyte) and held as packed bytes; the numpy-order arithmetic
// then reads every pixel from a register (constant indices: fully unrolled).
// Reading pixel by pixel from memory in the serial loops cost ~20 us per call
// (one dependent load per pixel and pass): a single such pair in a sweep set
// the whole k_score_fix launch (26 us at wid 3, profiles/r06/).
template <int WID>
__device__ __noinline__ double exact_ncc_stack(const SceneDev sc, int R, int v, int q, int r) {
    constexpr int NB = 2 * WID + 1, NPX = NB * NB;
    constexpr int NW = (NB + 3) / 4, ND = NW + 1;   // aligned dwords per row, dwords loaded per row
    const int64_t vstride = (int64_t)sc.V * 4;
    const int o = (q - WID) & 3;
    const uint8_t* p0 = sc.stack + (int64_t)(r - WID) * sc.row_bytes + (int64_t)((q - WID) >> 2) * vstride;
    // one window's rows, every load in flight, aligned to column q - WID
    auto window = [&](int view, uint32_t (&w)[NB][NW]) {
        uint32_t d[NB][ND];
#pragma unroll
        for (int row = 0; row < NB; ++row)
#pragma unroll
            for (int j = 0; j < ND; ++j)
                d[row][j] = *(const uint32_t*)(p0 + (int64_t)row * sc.row_bytes + j * vstride + view * 4);
#pragma unroll
        for (int row = 0; row < NB; ++row)
#pragma unroll
            for (int j = 0; j < NW; ++j) w[row][j] = __builtin_amdgcn_alignbyte(d[row][j + 1], d[row][j], o);
    };
    uint32_t wa[NB][NW], wb[NB][NW];
    window(R, wa);
    __builtin_amdgcn_sched_barrier(0);   // the second window's loads after: fewer registers in flight
    window(v, wb);
    // pixel i as a double, re-extracted at every use (opaque): kept as packed
    // bytes, not as NPX live doubles per window
    auto px = [&](const uint32_t (&w)[NB][NW], int i) -> double {
        const uint32_t word = (uint32_t)opaque((int)w[i / NB][(i % NB) >> 2]);
        return (double)((word >> (8 * ((i % NB) & 3))) & 255u);
    };
    int sa = 0, sb = 0;
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        sa += (int)((wa[i / NB][(i % NB) >> 2] >> (8 * ((i % NB) & 3))) & 255u);
        sb += (int)((wb[i / NB][(i % NB) >> 2] >> (8 * ((i % NB) & 3))) & 255u);
    }
    const double ma = (double)sa / NPX, mb = (double)sb / NPX;
    // numpy's pairwise sum of (x - mean)^2 for 8 <= n <= 128: 8 accumulators,
    // combined pairwise, the remainder added in order (as pairwise_sq)
    static_assert(NPX >= 8 && NPX <= 128, "numpy pairwise summation restated for 8 <= n <= 128");
    auto pw = [&](const uint32_t (&w)[NB][NW], double m) -> double {
        double acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { const double x = px(w, j) - m; acc[j] = x * x; }
#pragma unroll
        for (int i = 8; i < NPX - (NPX % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const double x = px(w, i + j) - m; acc[j] += x * x; }
        double res = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
        for (int i = NPX - (NPX % 8); i < NPX; ++i) { const double x = px(w, i) - m; res += x * x; }
        return res;
    };
    const double stda = sqrt(pw(wa, ma) / NPX), stdb = sqrt(pw(wb, mb) / NPX);
    // sum(d1 * d2) with Python's sequential sum (MVS2.py:43)
    double acc = 0;
#pragma unroll
    for (int i = 0; i < NPX; ++i) acc = acc + ((px(wa, i) - ma) / stda) * ((px(wb, i) - mb) / stdb);
    return acc / (NPX - 1);
}

// ---------------------------------------------------------------------------
// Direct photo test: one wave per candidate, lane l handles views l, l+64, ...
// (NS slots); window rows gathered from the stack.  Used for small batches,
// for the guard-band re-score of the tiled scorer (k_score_fix) and for the
// children of small expansion sweeps.
// ---------------------------------------------------------------------------
// One wave scores one candidate whose window sits at (q, r) of every view
// (the reference samples all views at view R's pixel, MVS2.py:68).
// fetch(s, row, j) returns the j-th dword (4 pixels of this lane's view of
// slot s) of window row `row`, counted from the quad holding column q - WID;
// o = (q - WID) & 3.  Lane 0 of the wave writes mask/count/avg.
// Decision without sqrt/div: for thr >= 0.01, ncc > thr  <=>  L > 0 and
// L^2 > thr^2 (n-1)^2 da db  with L = n*num (exact in binary64); a relative band
// of 1e-11 around it (5e-12 relative on the NCC) goes to the numpy-order
// path.  The comparison itself is exact to ~6e-16 relative (L is an exact
// integer, rhs three roundings); the reference's numpy-order NCC differs from
// the exact value by < 1e-14 relative (121 terms, std from pairwise sums), so
// the band covers every pair whose reference decision could differ from the
// exact one with a margin of ~500.  (It was 1e-8: 104 numpy-order
// evaluations per wid-3 sweep then, most of k_score_fix's 26 us.)
template <int WID, int NS, class Fetch>
DEV void wave_score_core(const SceneDev& sc, int R, int q, int r, double thr, Fetch&& fetch,
                         uint64_t* mask_out, int32_t* count_out, double* avg_out, int32_t* exact_hits) {
    constexpr int NB = 2 * WID + 1;
    constexpr int NPX = NB * NB;
    constexpr int NW = (NB + 3) / 4;
    constexpr int ND = NW + 1;
    constexpr uint32_t LASTMASK = (NB % 4 == 0) ? 0xffffffffu : ((1u << (8 * (NB % 4))) - 1u);
    const int lane = threadIdx.x & 63;
    const int o = (q - WID) & 3;
    const int V = sc.V;
    const int Rs = R >> 6, Rl = R & 63;

    uint32_t Sb[NS], Sbb[NS], Sab[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) Sb[s] = Sbb[s] = Sab[s] = 0;
    // one view slot: every row's loads in flight at once (a latency-bound
    // wave per candidate); more slots: one row at a time (registers)
    constexpr int ROW_UNROLL = NS == 1 ? NB : 1;
#pragma unroll ROW_UNROLL
    for (int row = 0; row < NB; ++row) {
        uint32_t w[NS][NW];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int v = lane + 64 * s;
            uint32_t d[ND];
            if (NS == 1 || v < V) {
#pragma unroll
                for (int j = 0; j < ND; ++j) d[j] = fetch(s, row, j);
            } else {
#pragma unroll
                for (int j = 0; j < ND; ++j) d[j] = 0;
            }
#pragma unroll
            for (int j = 0; j < NW; ++j) w[s][j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], o);
            w[s][NW - 1] &= LASTMASK;
        }
        uint32_t a[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            uint32_t src = w[0][j];
#pragma unroll
            for (int s = 1; s < NS; ++s) src = (Rs == s) ? w[s][j] : src;
            a[j] = __builtin_amdgcn_readlane(src, Rl);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                Sab[s] = __builtin_amdgcn_udot4(a[j], w[s][j], Sab[s], false);
                Sbb[s] = __builtin_amdgcn_udot4(w[s][j], w[s][j], Sbb[s], false);
                Sb[s] = __builtin_amdgcn_sad_u8(w[s][j], 0u, Sb[s]);
            }
        }
    }

    uint32_t sa_src = Sb[0], saa_src = Sbb[0];
#pragma unroll
    for (int s = 1; s < NS; ++s) {
        sa_src = (Rs == s) ? Sb[s] : sa_src;
        saa_src = (Rs == s) ? Sbb[s] : saa_src;
    }
    const int64_t Sa = __builtin_amdgcn_readlane(sa_src, Rl);
    const int64_t Saa = __builtin_amdgcn_readlane(saa_src, Rl);
    const int64_t da = (int64_t)NPX * Saa - Sa * Sa;

    double acc = 0.0;
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int v = lane + 64 * s;
        const int64_t sb = Sb[s];
        const int64_t db = (int64_t)NPX * (int64_t)Sbb[s] - sb * sb;
        const int64_t num = (int64_t)NPX * (int64_t)Sab[s] - Sa * sb;
        bool pass = false;
        double ncc = 0.0;
        const bool live = v < V && v != R && da > 0 && db > 0;   // da/db == 0: ctNcc nan -> reject
        if (live) {
            if (thr >= 0.01) {
                const double L = (double)((int64_t)NPX * num);
                if (L > 0.0) {
                    const double tk = thr * (double)(NPX - 1);
                    const double rhs = (tk * tk) * ((double)da * (double)db);
                    const double diff = L * L - rhs;
                    if (fabs(diff) <= 1e-11 * rhs) {
                        ncc = exact_ncc_stack<WID>(sc, R, v, q, r);
                        atomicAdd(exact_hits, 1);
                        pass = ncc > thr;
                    } else {
                        pass = diff > 0.0;
                        if (pass && avg_out) {
                            // avg_ncc_score value only: rsq + two Newton steps
                            const double D = (double)da * (double)db;
                            double y = __builtin_amdgcn_rsq(D);
                            y = y * (1.5 - 0.5 * D * y * y);
                            y = y * (1.5 - 0.5 * D * y * y);
                            ncc = L * y * (1.0 / (double)(NPX - 1));
                        }
                    }
                }
            } else {
                ncc = (double)((int64_t)NPX * num) / ((double)(NPX - 1) * sqrt((double)da * (double)db));
                if (fabs(ncc - thr) <= kGuard) {
                    ncc = exact_ncc_stack<WID>(sc, R, v, q, r);
                    atomicAdd(exact_hits, 1);
                }
                pass = ncc > thr;
            }
        }
        const uint64_t m = __ballot(pass);
        // NS slots can exceed the candidate's ceil(V/64) mask words (NS = 4 for
        // 128 < V <= 192): only the words that exist are written
        if (lane == 0 && 64 * s < V) mask_out[s] = m;
        cnt += __popcll(m);
        acc += pass ? ncc : 0.0;
    }
    if (!avg_out || cnt == 0) {
        if (lane == 0) {
            if (count_out) *count_out = cnt;
            if (avg_out) *avg_out = 0.0;
        }
        return;
    }
    const double tot = wave_sum(acc);
    if (lane == 0) {
        if (count_out) *count_out = cnt;
        *avg_out = tot / cnt;
    }
}

template <int WID, int NS>
DEV void wave_score(const SceneDev& sc, int R, int q, int r, double thr, uint64_t* mask_out,
                    int32_t* count_out, double* avg_out, int32_t* exact_hits) {
    const int lane = threadIdx.x & 63;
    const int k0 = (q - WID) >> 2;
    const int64_t vstride = (int64_t)sc.V * 4;
    const uint8_t* p0 = sc.stack + (int64_t)(r - WID) * sc.row_bytes + (int64_t)k0 * vstride;
    auto fetch = [&](int s, int row, int j) -> uint32_t {
        return *(const uint32_t*)(p0 + (int64_t)row * sc.row_bytes + j * vstride + (lane + 64 * s) * 4);
    };
    wave_score_core<WID, NS>(sc, R, q, r, thr, fetch, mask_out, count_out, avg_out, exact_hits);
}

template <int NS>
DEV void wave_score_empty(uint64_t* mask_out, int32_t* count_out, double* avg_out, int words) {
    const int lane = threadIdx.x & 63;
    if (lane < NS && lane < words) mask_out[lane] = 0;
    if (lane == 0) {
        if (count_out) *count_out = 0;
        if (avg_out) *avg_out = 0.0;
    }
}

// ---------------------------------------------------------------------------
// Scene setup: RGB (V, H, W, 3) -> gray (OpenCV BGR2GRAY fixed point applied to
// the RGB data, HarrisFeatures.py:125 on main.py:18's RGB images), written in
// both layouts.  A block takes one image row, a 64-pixel strip and 16 views at
// a time: the RGB bytes come in as whole 16-byte pieces, gv rows leave as 64-B
// runs per view and stack quads as 64-B runs per quad (16 views).
// ---------------------------------------------------------------------------
constexpr int kSceneStrip = 64, kSceneViews = 16;

__global__ __launch_bounds__(256) void k_build_scene(const SceneDev sc, const uint8_t* __restrict__ rgb,
                                                     uint8_t* __restrict__ stack, uint8_t* __restrict__ gv) {
    __shared__ __attribute__((aligned(16))) uint8_t srgb[kSceneViews][kSceneStrip * 3];
    __shared__ uint32_t squad[kSceneStrip / 4][kSceneViews];
    const int y = blockIdx.y;
    const int x0 = blockIdx.x * kSceneStrip;
    const int nx = min(kSceneStrip, sc.W - x0);
    const int tid = threadIdx.x;
    const bool vec = (sc.W & 15) == 0;          // every strip is whole 16-byte pieces
    for (int v0 = 0; v0 < sc.V; v0 += kSceneViews) {
        const int nv = min(kSceneViews, sc.V - v0);
        if (vec) {
            const int cpv = nx * 3 / 16;
            for (int k = tid; k < nv * cpv; k += 256) {
                const int vv = k / cpv, c = k - vv * cpv;
                *(uint4*)(&srgb[vv][16 * c]) =
                    *(const uint4*)(rgb + (((int64_t)(v0 + vv) * sc.H + y) * sc.W + x0) * 3 + 16 * c);
            }
        } else {
            for (int k = tid; k < nv * nx * 3; k += 256) {
                const int vv = k / (nx * 3), b = k - vv * (nx * 3);
                srgb[vv][b] = rgb[(((int64_t)(v0 + vv) * sc.H + y) * sc.W + x0) * 3 + b];
            }
        }
        __syncthreads();
        {
            const int vv = tid >> 4, qd = tid & 15;
            if (vv < nv && 4 * qd < nx) {
                uint32_t word = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int x = 4 * qd + b;
                    if (x < nx) {
                        const uint8_t* p = &srgb[vv][3 * x];
                        const uint32_t g = (p[0] * 1868u + p[1] * 9617u + p[2] * 4899u + 8192u) >> 14;
                        word |= g << (8 * b);
                    }
                }
                squad[qd][vv] = word;
                // gv: signed bytes s = g - 128 (the tiled scorer's operands)
                *(uint32_t*)(gv + ((int64_t)(v0 + vv) * sc.H + y) * sc.Wp + x0 + 4 * qd) = word ^ 0x80808080u;
            }
        }
        __syncthreads();
        {
            const int qd = tid >> 4, vv = tid & 15;
            if (vv < nv && 4 * qd < nx)
                *(uint32_t*)(stack + (int64_t)y * sc.row_bytes + ((int64_t)(x0 / 4 + qd) * sc.V + v0 + vv) * 4) =
                    squad[qd][vv];
        }
        __syncthreads();
    }
}

template <int WID, int NS>
__global__ __launch_bounds__(256) void k_score(const SceneDev sc, const ScoreArgs a) {
    const int64_t cand = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cand >= a.n) return;
    const int words = (sc.V + 63) >> 6;
    const int R = __builtin_amdgcn_readfirstlane(a.ref[cand]);
    double c[3] = {a.c[3 * cand], a.c[3 * cand + 1], a.c[3 * cand + 2]};
    double px, py;
    project(sc.cams[R], c, px, py);
    const int lane = threadIdx.x & 63;
    if (lane == 0) { a.xy[2 * cand] = px; a.xy[2 * cand + 1] = py; }
    int q, r;
    if (!window_ok(sc, px, py, WID, &q, &r)) {
        wave_score_empty<NS>(a.mask + cand * a.mstride, a.count ? a.count + cand : nullptr,
                             a.avg ? a.avg + cand * a.astride : nullptr, words);
        return;
    }
    q = __builtin_amdgcn_readfirstlane(q);
    r = __builtin_amdgcn_readfirstlane(r);
    wave_score<WID, NS>(sc, R, q, r, a.thr, a.mask + cand * a.mstride, a.count ? a.count + cand : nullptr,
                        a.avg ? a.avg + cand * a.astride : nullptr, a.exact_hits);
}

// Guard-band candidates of the tiled scorer and bucket overflow, re-scored
// whole by the direct path (whose own guard band leads to the numpy-order
// ctNcc).  Last kernel of a batch.  It zeroes nothing: the tile counters and
// the control block come in two parity sets, and the next batch's k_bin
// zeroes this batch's set (no done ticket here: a kernel with a short list
// is a launch and one load: 6.8 -> 4.7 us with 30 guard-band entries,
// profiles/r06/r6p_*).  The grid has kFixBase workgroups plus, for large batches, more that take
// part only when the list is long (a skewed batch whose tiles overflow their
// buckets): a guard-band list of a few hundred entries costs no extra
// workgroups' atomics, a long overflow list gets up to 4x the workgroups.
constexpr int kFixBase = 64, kFixSmall = kFixBase * 4 * 8;

template <int WID, int NS>
__global__ __launch_bounds__(256) void k_score_fix(const SceneDev sc, const ScoreArgs a,
                                                   const TiledArgs t) {
    const int nfix = *t.fix_count;
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.stats) {
        t.stats[0] += (unsigned long long)nfix;
        t.stats[2] += 1ull;
    }
    const int active = nfix > kFixSmall ? (int)gridDim.x : kFixBase;   // uniform over the grid
    if ((int)blockIdx.x >= active) return;
    for (int k = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); k < nfix;
         k += active * 4) {
        const int4 f = t.fix_list[k];
        const int64_t cand = __builtin_amdgcn_readfirstlane(f.x);
        const int tile = __builtin_amdgcn_readfirstlane(f.y);
        const int pk = __builtin_amdgcn_readfirstlane(f.z);
        const int ty = tile / t.ntx, tx = tile - ty * t.ntx;
        const int q = tx * MVS_TILE_W + (pk & 15), r = ty * MVS_TILE_H + ((pk >> 4) & 7), R = pk >> 7;
        wave_score<WID, NS>(sc, R, q, r, a.thr, a.mask + cand * a.mstride, a.count ? a.count + cand : nullptr,
                            a.avg ? a.avg + cand * a.astride : nullptr, a.exact_hits);
    }
}

// ---------------------------------------------------------------------------
// patch_expansion children (MVS2.py:329-369)
// ---------------------------------------------------------------------------
DEV double dot3(const double* a, const double* b) {
    // np.dot of two float64 3-vectors as OpenBLAS 0.3.29 evaluates it.
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]));
}

DEV int py_wrap(int i, int n) { return i < 0 ? i + n : i; }

// Geometry of child k: ray through the (buggy) cell centre, intersection
// with the parent's plane, normal, colour, projection into the child's own
// view and its cell; written into the child's record row `out`.
DEV void child_geometry(const SceneDev& sc, const RecordsDev& rec, const ExpandArgs& a, const ChildJob job,
                        int64_t out, double* X, double* nX, double* pxo, double* pyo) {
    const int64_t par = job.parent;
    const int v = job.view;
    const int di = job.di;
    const CamDev& cm = sc.cams[v];
    const double pc[3] = {rec.c[3 * par], rec.c[3 * par + 1], rec.c[3 * par + 2]};
    const double pn[3] = {rec.n[3 * par], rec.n[3 * par + 1], rec.n[3 * par + 2]};
    const double cs = (double)a.cell_size;
    // which_cell of the parent's hit (MVS2.py:330): every V entry carries the
    // parent's projection into its own reference view (MVS2.py:68, 74).
    const double ci = floor(rec.xy[2 * par] / cs), cj = floor(rec.xy[2 * par + 1] / cs);
    // cell_center(ci+i, cj+i): the second index reuses i (MVS2.py:334)
    const double cc0 = cs * ((ci + di) + 0.5);
    const double cc1 = cs * ((cj + di) + 0.5);
    const double w[3] = {cc0 - cm.cx, cc1 - cm.cy, cm.fbar};
    double Pw[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)   // R^T @ w + C (MVS2.py:353)
        Pw[j] = fma(cm.R[6 + j], w[2], fma(cm.R[3 + j], w[1], cm.R[j] * w[0])) + cm.C[j];
    const double nrm = sqrt((Pw[0] * Pw[0] + Pw[1] * Pw[1]) + Pw[2] * Pw[2]);   // vector_norm
    const double d[3] = {Pw[0] / nrm, Pw[1] / nrm, Pw[2] / nrm};
    // ray_plane_intersection(camera_pos[v], d, parent.c, parent.n) (MVS2.py:302-306)
    const double dot_out = dot3(d, pn);
    const double cmo[3] = {pc[0] - cm.O[0], pc[1] - cm.O[1], pc[2] - cm.O[2]};
    const double tt = dot3(cmo, pn) / dot_out;
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = cm.O[j] + tt * d[j];
    const double e0 = X[0] - cm.O[0], e1 = X[1] - cm.O[1], e2 = X[2] - cm.O[2];
    const double dist = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
#pragma unroll
    for (int j = 0; j < 3; ++j) nX[j] = (cm.O[j] - X[j]) / dist;
    double px, py;
    project(cm, X, px, py);
    *pxo = px;
    *pyo = py;
}

DEV void child_write(const SceneDev& sc, const RecordsDev& rec, const ExpandArgs& a, const ChildJob job,
                     int64_t out, const double* X, const double* nX, double px, double py) {
    const int v = job.view;
    const double cs = (double)a.cell_size;
    const int64_t par = job.parent;
    const double ci = floor(rec.xy[2 * par] / cs), cj = floor(rec.xy[2 * par + 1] / cs);
    const double cc0 = cs * ((ci + job.di) + 0.5);
    const double cc1 = cs * ((cj + job.di) + 0.5);
#pragma unroll
    for (int j = 0; j < 3; ++j) { rec.c[3 * out + j] = X[j]; rec.n[3 * out + j] = nX[j]; }
    rec.xy[2 * out] = px;
    rec.xy[2 * out + 1] = py;
    rec.R[out] = v;
    // get_color(imgs[v], cc0, cc1) = img[int(cc1)][int(cc0)] (MVS2.py:119-120, 358)
    int yy = 0, xx = 0;
    py_trunc(cc1, &yy);
    py_trunc(cc0, &xx);
    yy = py_wrap(yy, sc.H);
    xx = py_wrap(xx, sc.W);
    uint8_t rgbv[3] = {0, 0, 0};
    if (yy >= 0 && yy < sc.H && xx >= 0 && xx < sc.W) {
        const uint8_t* p = sc.rgb + (((int64_t)v * sc.H + yy) * sc.W + xx) * 3;
        rgbv[0] = p[0]; rgbv[1] = p[1]; rgbv[2] = p[2];
    }
    rec.color[4 * out] = rgbv[0]; rec.color[4 * out + 1] = rgbv[1];
    rec.color[4 * out + 2] = rgbv[2]; rec.color[4 * out + 3] = 0;
    rec.cell[2 * out] = (int32_t)floor(px / cs);
    rec.cell[2 * out + 1] = (int32_t)floor(py / cs);
}

// accept test (MVS2.py:369) with is_patch_neighbor (MVS2.py:298-299)
DEV uint8_t child_accept(const RecordsDev& rec, const ExpandArgs& a, int64_t par, const double* X,
                         const double* nX, int cnt) {
    const double pc[3] = {rec.c[3 * par], rec.c[3 * par + 1], rec.c[3 * par + 2]};
    const double pn[3] = {rec.n[3 * par], rec.n[3 * par + 1], rec.n[3 * par + 2]};
    const double pm[3] = {pc[0] - X[0], pc[1] - X[1], pc[2] - X[2]};
    const double nb = fabs(dot3(pm, pn) + dot3(pm, nX));
    const double g0 = pc[0] - X[0], g1 = pc[1] - X[1], g2 = pc[2] - X[2];
    const double dd = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
    return (cnt >= a.vlb && nb < 0.1 && dd < a.dist_thr) ? 1 : 0;
}

// one wave per child: geometry, direct photo test, accept test (small sweeps)
template <int WID, int NS>
__global__ __launch_bounds__(256) void k_expand(const SceneDev sc, RecordsDev rec, const ExpandArgs a) {
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= a.n) return;
    const int lane = threadIdx.x & 63;
    const int words = (sc.V + 63) >> 6;
    const ChildJob job = a.jobs[k];
    const int v = __builtin_amdgcn_readfirstlane((int)job.view);
    const int64_t out = a.first_out + k;
    double X[3], nX[3], px, py;
    child_geometry(sc, rec, a, job, out, X, nX, &px, &py);
    if (lane == 0) child_write(sc, rec, a, job, out, X, nX, px, py);
    int q, r;
    if (!window_ok(sc, px, py, WID, &q, &r)) {
        wave_score_empty<NS>(rec.mask + out * words, rec.count + out, nullptr, words);
        if (lane == 0) rec.accept[out] = 0;
        return;
    }
    q = __builtin_amdgcn_readfirstlane(q);
    r = __builtin_amdgcn_readfirstlane(r);
    wave_score<WID, NS>(sc, v, q, r, a.thr, rec.mask + out * words, rec.count + out, nullptr,
                        a.exact_hits);
    if (lane == 0) rec.accept[out] = child_accept(rec, a, job.parent, X, nX, rec.count[out]);
}

// large sweeps: one thread per child for the geometry ...
__global__ void k_expand_geom(const SceneDev sc, RecordsDev rec, const ExpandArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n;
         k += (int64_t)gridDim.x * blockDim.x) {
        const ChildJob job = a.jobs[k];
        const int64_t out = a.first_out + k;
        double X[3], nX[3], px, py;
        child_geometry(sc, rec, a, job, out, X, nX, &px, &py);
        child_write(sc, rec, a, job, out, X, nX, px, py);
    }
}

// ... and, after the tiled photo test of the children, the accept test
__global__ void k_expand_accept(RecordsDev rec, const ExpandArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n;
         k += (int64_t)gridDim.x * blockDim.x) {
        const ChildJob job = a.jobs[k];
        const int64_t out = a.first_out + k;
        const double X[3] = {rec.c[3 * out], rec.c[3 * out + 1], rec.c[3 * out + 2]};
        const double nX[3] = {rec.n[3 * out], rec.n[3 * out + 1], rec.n[3 * out + 2]};
        rec.accept[out] = child_accept(rec, a, job.parent, X, nX, rec.count[out]);
    }
}

// Batched ctNcc on explicit window pairs: the function-level check of the NCC
// core (integer moments + guard + exact fallback), one thread per pair.
__global__ void k_ncc_windows(int64_t n, int npx, const uint8_t* __restrict__ A,
                              const uint8_t* __restrict__ B, double thr, int force_exact,
                              double* ncc_out, uint8_t* pass_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t* a = A + i * npx;
        const uint8_t* b = B + i * npx;
        int64_t sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
        for (int k = 0; k < npx; ++k) {
            const int x = a[k], y = b[k];
            sa += x; sb += y; saa += x * x; sbb += y * y; sab += x * y;
        }
        const int64_t da = npx * saa - sa * sa, db = npx * sbb - sb * sb;
        const int64_t num = npx * sab - sa * sb;
        double ncc;
        bool in_guard = false;
        if (da <= 0 || db <= 0) {
            ncc = __builtin_nan("");
        } else {
            ncc = (double)(npx * num) / ((double)(npx - 1) * sqrt((double)da * (double)db));
            in_guard = fabs(ncc - thr) <= kGuard;
        }
        if ((force_exact || in_guard) && da > 0 && db > 0)
            ncc = exact_ncc_generic([&](int k) -> int { return a[k]; },
                                    [&](int k) -> int { return b[k]; }, npx);
        ncc_out[i] = ncc;
        pass_out[i] = ncc > thr ? 1 : 0;
    }
}

// Sharded sweep, ingest side: every rank computed the whole sweep's child
// geometry (k_expand_geom) and received the other ranks' photo-test masks,
// so a child's count (|V| = popcount of its mask, MVS2.py:72-74) and its
// accept test (MVS2.py:369) follow here.
__global__ void k_expand_ingest(RecordsDev rec, const ExpandArgs a, int words) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n;
         k += (int64_t)gridDim.x * blockDim.x) {
        const ChildJob job = a.jobs[k];
        const int64_t out = a.first_out + k;
        int cnt = 0;
        for (int q = 0; q < words; ++q) cnt += __popcll(rec.mask[out * words + q]);
        rec.count[out] = cnt;
        const double X[3] = {rec.c[3 * out], rec.c[3 * out + 1], rec.c[3 * out + 2]};
        const double nX[3] = {rec.n[3 * out], rec.n[3 * out + 1], rec.n[3 * out + 2]};
        rec.accept[out] = child_accept(rec, a, job.parent, X, nX, cnt);
    }
}

// reconstruct_from_Q (MVS2.py:159-173): an accepted patch is appended under
// key (u, cell) for every view u of its V list, with one cell for all entries
// (every V entry carries the projection into the patch's own view), so its
// first sight in the lexicographic key walk is (min u, cell)
__global__ void k_event_keys(RecordsDev rec, int words, const int32_t* __restrict__ events, int64_t n,
                             int nci, int ncj, uint64_t* __restrict__ keys) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = events[e];
        int minv = -1;
        for (int w = 0; w < words && minv < 0; ++w) {
            const uint64_t mk = rec.mask[r * words + w];
            if (mk) minv = 64 * w + __ffsll((long long)mk) - 1;
        }
        const int cx = rec.cell[2 * r], cy = rec.cell[2 * r + 1];
        keys[e] = (minv < 0 || cx < 0 || cx >= nci || cy < 0 || cy >= ncj)
                      ? ~0ull
                      : (uint64_t)(((int64_t)minv * nci + cx) * ncj + cy);
    }
}

// the PLY rows [x y z r g b] (utils.py:249-250) of records idx[i]
__global__ void k_gather_rows(RecordsDev rec, const int32_t* __restrict__ idx, int64_t n,
                              double* __restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx[i];
        double* o = rows + 6 * i;
        o[0] = rec.c[3 * r];
        o[1] = rec.c[3 * r + 1];
        o[2] = rec.c[3 * r + 2];
        o[3] = rec.color[4 * r];
        o[4] = rec.color[4 * r + 1];
        o[5] = rec.color[4 * r + 2];
    }
}

// avg_ncc_score of accepted patches in the reference's own arithmetic
// (MVS2.py:62-76, for filter_out_outlier): every view of the V list in view
// order, ctNcc in numpy's order (exact_ncc_stack), summed left to right from
// 0 (`self.avg_ncc_score += ncc_score`), then divided by |V|.  One wave per
// record: the lanes score the views, lane 0 sums them in order.  ids == null:
// records 0..n-1 (a scored batch's ref / xy / mask arrays as the records).
template <int WID, int NS>
__global__ __launch_bounds__(256) void k_exact_avg(const SceneDev sc, const RecordsDev rec,
                                                   const int32_t* __restrict__ ids, int64_t n,
                                                   double* __restrict__ out) {
    __shared__ double s_ncc[4][64 * NS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + w;
    if (k >= n) return;   // uniform per wave; no block-level barrier below
    const int64_t r = ids ? ids[k] : k;
    const int words = (sc.V + 63) >> 6;
    const int R = rec.R[r];
    int q = 0, rr = 0;
    // a window outside the image has no passing views (its V list is empty);
    // masked views of such a record read a defined NaN, never the stack
    const bool ok = window_ok(sc, rec.xy[2 * r], rec.xy[2 * r + 1], WID, &q, &rr);
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int v = lane + 64 * sl;
        if (v < sc.V && ((rec.mask[r * words + (v >> 6)] >> (v & 63)) & 1ull))
            s_ncc[w][v] = ok ? exact_ncc_stack<WID>(sc, R, v, q, rr) : __builtin_nan("");
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        double sum = 0.0;
        int cnt = 0;
        for (int v = 0; v < sc.V; ++v)
            if ((rec.mask[r * words + (v >> 6)] >> (v & 63)) & 1ull) {
                sum = sum + s_ncc[w][v];
                ++cnt;
            }
        out[k] = cnt ? sum / (double)cnt : 0.0;
    }
}

template <int WID>
int launch_score_w(const SceneDev* sc, const ScoreArgs* a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    const int64_t blocks = (a->n + 3) / 4;
    if (blocks == 0) return 0;
    TimedLaunch tl(s, ev0, ev1);
    if (sc->V <= 64)
        hipLaunchKernelGGL((k_score<WID, 1>), dim3((unsigned)blocks), dim3(256), 0, s, *sc, *a);
    else if (sc->V <= 128)
        hipLaunchKernelGGL((k_score<WID, 2>), dim3((unsigned)blocks), dim3(256), 0, s, *sc, *a);
    else
        hipLaunchKernelGGL((k_score<WID, 4>), dim3((unsigned)blocks), dim3(256), 0, s, *sc, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int WID>
int launch_expand_w(const SceneDev* sc, RecordsDev rec, const ExpandArgs* a, hipStream_t s) {
    const int64_t blocks = (a->n + 3) / 4;
    if (blocks == 0) return 0;
    if (sc->V <= 64)
        hipLaunchKernelGGL((k_expand<WID, 1>), dim3((unsigned)blocks), dim3(256), 0, s, *sc, rec, *a);
    else if (sc->V <= 128)
        hipLaunchKernelGGL((k_expand<WID, 2>), dim3((unsigned)blocks), dim3(256), 0, s, *sc, rec, *a);
    else
        hipLaunchKernelGGL((k_expand<WID, 4>), dim3((unsigned)blocks), dim3(256), 0, s, *sc, rec, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int grid_for(int64_t n, int block, int cap) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, cap));
}

}  // namespace

extern "C" int mvs_launch_build_scene(const SceneDev* sc, const uint8_t* d_rgb, uint8_t* d_stack,
                                      uint8_t* d_gv_base, hipStream_t s) {
    (void)d_gv_base;
    const dim3 grid((unsigned)((sc->W + kSceneStrip - 1) / kSceneStrip), (unsigned)sc->H);
    hipLaunchKernelGGL(k_build_scene, grid, dim3(256), 0, s, *sc, d_rgb, d_stack, (uint8_t*)sc->gv);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mvs_launch_score(const SceneDev* sc, const ScoreArgs* a, int wid, hipStream_t s,
                                hipEvent_t ev0, hipEvent_t ev1) {
    return dispatch_wid(wid, -2, [&](auto w) { return launch_score_w<decltype(w)::value>(sc, a, s, ev0, ev1); });
}

extern "C" int mvs_launch_score_fix(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t, int wid,
                                    hipStream_t s) {
    // 256 waves (one candidate each at a time) for the guard band; up to 4x as many for a long overflow list
    const int kFixBlocks = (int)std::min<int64_t>(std::max<int64_t>(a->n / 4096, kFixBase), 4 * kFixBase);
    return dispatch_wid(wid, -2, [&](auto w) {
        constexpr int WID = decltype(w)::value;
        if (sc->V <= MVS_GROUP_VIEWS)
            hipLaunchKernelGGL((k_score_fix<WID, 1>), dim3(kFixBlocks), dim3(256), 0, s, *sc, *a, *t);
        else if (sc->V <= 128)
            hipLaunchKernelGGL((k_score_fix<WID, 2>), dim3(kFixBlocks), dim3(256), 0, s, *sc, *a, *t);
        else
            hipLaunchKernelGGL((k_score_fix<WID, 4>), dim3(kFixBlocks), dim3(256), 0, s, *sc, *a, *t);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

extern "C" int mvs_launch_expand(const SceneDev* sc, RecordsDev rec, const ExpandArgs* a, int wid,
                                 hipStream_t s) {
    return dispatch_wid(wid, -2, [&](auto w) {   // wid 3 and 5 only
        constexpr int WID = decltype(w)::value;
        if constexpr (WID == 3 || WID == 5) return launch_expand_w<WID>(sc, rec, a, s);
        else return -2;
    });
}

extern "C" int mvs_launch_expand_geom(const SceneDev* sc, RecordsDev rec, const ExpandArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_expand_geom, dim3(grid_for(a->n, 256, 4096)), dim3(256), 0, s, *sc, rec, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mvs_launch_expand_accept(RecordsDev rec, const ExpandArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_expand_accept, dim3(grid_for(a->n, 256, 4096)), dim3(256), 0, s, rec, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mvs_launch_expand_ingest(RecordsDev rec, const ExpandArgs* a, int words, hipStream_t s) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_expand_ingest, dim3(grid_for(a->n, 256, 4096)), dim3(256), 0, s, rec, *a, words);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int mvs_launch_ncc_windows(int64_t n, int npx, const uint8_t* a, const uint8_t* b,
                                      double thr, int force_exact, double* ncc, uint8_t* pass,
                                      hipStream_t s) {
    if (npx <= 0 || npx > 128) return -2;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_ncc_windows, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, n, npx, a, b, thr,
                       force_exact, ncc, pass);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mvs_launch_event_keys(RecordsDev rec, int words, const int32_t* events, int64_t n_events,
                                     int nci, int ncj, uint64_t* keys, hipStream_t s) {
    if (n_events <= 0) return 0;
    hipLaunchKernelGGL(k_event_keys, dim3(grid_for(n_events, 256, 4096)), dim3(256), 0, s, rec, words, events,
                       n_events, nci, ncj, keys);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int WID>
int launch_exact_avg_w(const SceneDev* sc, RecordsDev rec, const int32_t* ids, int64_t n, double* out,
                       hipStream_t s) {
    const dim3 grid((unsigned)((n + 3) / 4));
    if (sc->V <= 64) hipLaunchKernelGGL((k_exact_avg<WID, 1>), grid, dim3(256), 0, s, *sc, rec, ids, n, out);
    else if (sc->V <= 128) hipLaunchKernelGGL((k_exact_avg<WID, 2>), grid, dim3(256), 0, s, *sc, rec, ids, n, out);
    else hipLaunchKernelGGL((k_exact_avg<WID, 4>), grid, dim3(256), 0, s, *sc, rec, ids, n, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mvs_launch_exact_avg(const SceneDev* sc, RecordsDev rec, int wid, const int32_t* ids, int64_t n,
                                    double* out, hipStream_t s) {
    if (n <= 0) return 0;
    if (sc->V > MVS_MAX_VIEWS) return -3;
    return dispatch_wid(wid, -2, [&](auto w) {   // wid 3 and 5 only
        constexpr int WID = decltype(w)::value;
        if constexpr (WID == 3 || WID == 5) return launch_exact_avg_w<WID>(sc, rec, ids, n, out, s);
        else return -2;
    });
}

extern "C" int mvs_launch_gather_rows(RecordsDev rec, const int32_t* idx, int64_t n, double* rows, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, rec, idx, n, rows);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
