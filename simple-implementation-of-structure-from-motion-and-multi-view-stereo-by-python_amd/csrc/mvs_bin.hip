// Binning and the launcher that orders a tiled batch: k_bin, k_item_scan, the
// scene's scorer (k_score_tab, k_score_mma or k_score_mma_v) and k_score_fix,
// each in a unit of its own, through its extern "C" launcher.
#include <algorithm>

#include "mvs_mma.h"
#include "mvs_stamps.h"

namespace {

// ---------------------------------------------------------------------------
// Tiled scorer, stage 1: candidates binned by the 16x8 pixel tile of their
// window centre.  k_bin projects (binary64, reference order), tests the
// window and ranks the candidate inside its tile -- through an LDS histogram
// per block (one global atomic per non-empty (block, tile) pair) when the tile
// counters fit in LDS, else through one global atomic per candidate -- and
// writes it into the tile's bucket.  k_item_scan then writes the work items
// (tile, chunk j: candidates [j chunk, (j+1) chunk) of its bucket) in tile
// order; the scorers read the tile's final count when they take the item
// (item_desc).
// ---------------------------------------------------------------------------
// MVS_BIN_PER (mvs_internal.h): candidates per k_bin thread (A/B switch)
constexpr int kBinBlock = MVS_BIN_BLOCK, kBinPer = MVS_BIN_PER, kBinLdsTiles = 16384;
static_assert(kBinBlock * kBinPer == MVS_BIN_CHUNK, "MVS_BIN_CHUNK candidates per k_bin workgroup");
static_assert(kBinBlock * kBinPer <= 4096, "k_bin_count packs a rank inside the workgroup into 12 bits");
#ifndef MVS_IMPLICIT_MEAN
#define MVS_IMPLICIT_MEAN 64   // A/B switch (a huge value keeps k_item_scan everywhere)
#endif
constexpr int64_t kImplicitMean = MVS_IMPLICIT_MEAN;

// The work items in tile order: one workgroup reads every tile's count, scans
// the tiles' chunk counts (chunk j of a tile: bucket entries [j chunk,
// (j+1) chunk) below min(count, cap)) and writes (tile, j) for each chunk into
// segment 0 (the other segments' counts to 0).  Measured against items in the
// order k_bin's workgroups opened them (same box): k_score_mma_v at ring256
// 1.67-1.72 vs 1.86-1.87 ms per 2^20, k_score_tab at dinoRing 105.5-107.2 vs
// 111.1-111.6 us (profiles/r04/r4r_*, r4s_*).
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_item_scan(const TiledArgs t) {
    __shared__ int s_w[kScanThreads / 64 + 1];
    const int per = (t.ntiles + kScanThreads - 1) / kScanThreads;   // tiles per thread, contiguous
    const int t0 = min((int)threadIdx.x * per, t.ntiles), t1 = min(t0 + per, t.ntiles);
    int mine = 0;
    for (int k = t0; k < t1; ++k) {
        const int c = min(t.tile_count[k * kTcStride], t.cap);
        mine += (c + t.chunk - 1) / t.chunk;
    }
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if ((threadIdx.x & 63) >= d) incl += o;
    }
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) { const int c = s_w[w]; s_w[w] = run; run += c; }
        s_w[kScanThreads / 64] = run;
    }
    __syncthreads();
    int slot = s_w[threadIdx.x >> 6] + incl - mine;
    for (int k = t0; k < t1; ++k) {
        const int c = min(t.tile_count[k * kTcStride], t.cap);
        for (int j = 0; j * t.chunk < c; ++j) t.items[slot++] = make_int4(k, j, 0, 0);
    }
    if (threadIdx.x < kItemSegs) t.n_items[32 * threadIdx.x] = threadIdx.x == 0 ? s_w[kScanThreads / 64] : 0;
}

// RUNS (with LDSHIST): the runs path (mvs_internal.h) -- the workgroup's
// candidates sorted by tile into its own run, from an exclusive scan of its LDS
// histogram; no global atomic, no tile_count, no implicit-item appends, no
// fix_list entries (k_score_tab's gather pushes the ranks past cap)
template <bool LDSHIST, bool RUNS = false>
__global__ __launch_bounds__(kBinBlock) void k_bin(const SceneDev sc, const ScoreArgs a,
                                                   const TiledArgs t, int wid, const MomentsDev mt) {
    extern __shared__ int32_t hist[];      // [ntiles] local counts, then global bases
    // the cameras' projection constants (R', t, fx fy cx cy) in LDS: every
    // candidate reads its reference camera's 16 values there instead of by
    // per-lane global loads.  Field-major ([value][view]): the lanes of a
    // read (one value of 64 random views) fall in distinct banks; view-major
    // rows of 128 B put them all in two banks (81 % of k_bin's LDS cycles
    // were bank conflicts, profiles/r06/pmc_r6e_w5_scorer.csv)
    __shared__ double s_cam[16][MVS_MAX_VIEWS];
    const int words = (sc.V + 63) >> 6;
    const int64_t base = (int64_t)blockIdx.x * kBinBlock * kBinPer;
    // every candidate's inputs in flight at once (one memory round trip, not
    // one per candidate), issued before the camera table's loads: the two
    // round trips overlap (k_bin 27.4 vs 28.5 us, profiles/r06/r6k_*)
    int Rk[kBinPer];
    double ck[kBinPer][3];
#pragma unroll
    for (int k = 0; k < kBinPer; ++k) {
        const int64_t i = base + (int64_t)k * kBinBlock + threadIdx.x;
        const int64_t ii = i < a.n ? i : 0;
        Rk[k] = a.ref[ii];
        ck[k][0] = a.c[3 * ii];
        ck[k][1] = a.c[3 * ii + 1];
        ck[k][2] = a.c[3 * ii + 2];
    }
    for (int k = threadIdx.x; k < sc.V * 16; k += blockDim.x) {
        const int v = k >> 4, f = k & 15;
        const CamDev& cm = sc.cams[v];
        s_cam[f][v] = f < 9 ? cm.Rp[f] : f < 12 ? cm.t[f - 9] : f == 12 ? cm.fx : f == 13 ? cm.fy : f == 14 ? cm.cx : cm.cy;
    }
    STAMP(t0);
    // the previous batch's counter set (the other parity; its k_score_fix
    // has finished, stream order) back to zero for the batch after this one
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < t.zero_words; k += (int64_t)gridDim.x * blockDim.x)
        t.zero_blk[k] = 0;
    if (LDSHIST)
        for (int b = threadIdx.x; b < t.ntiles; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    int tl[kBinPer], lr[kBinPer], pk[kBinPer];
    // a candidate whose reference window is constant (D_a = 0: ctNcc's std is
    // 0, every view's NCC nan, MVS2.py:41-42) passes no view: its outputs are
    // written here (V = [], avg 0) and it is not binned, so the scorers never
    // see it.  Decided from the scene's constant-window bits (MomentsDev.flat,
    // 2 B per pixel and 16 views: an L2 hit), one gather per candidate, all of
    // a thread's in flight
    const uint16_t* __restrict__ flat = mt.flat;
    int fk[kBinPer];
    int qk[kBinPer], rk[kBinPer];
    // V = [], avg 0.  Records (a.rec, V <= 64): one 16-B store.  No loop
    // with a run-time trip count here: the compiler's wait-count tracking
    // then stays exact, where a loop made it wait for every store of the
    // thread (vmcnt(0)) before the first (workgroup, tile) atomic
    auto settle = [&](int64_t i) {
        if (a.rec && words == 1) {
            *(uint4*)(a.mask + 2 * i) = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
#pragma unroll
        for (int w = 0; w < MVS_MAX_VIEWS / 64; ++w)
            if (w < words) a.mask[i * a.mstride + w] = 0;
        if (a.count) a.count[i] = 0;
        if (a.avg) a.avg[i * a.astride] = 0.0;
    };
    // Every load of these two loops is issued and consumed on every path
    // (past the batch: candidate 0's values; invalid window: pixel (0, 0)'s
    // bits), so that no path leaves a load pending at the loops' joins: the
    // compiler's wait counting then stays exact, where a conditionally
    // consumed load made it wait for every memory operation of the thread
    // (vmcnt(0): the xy and settled stores included) ahead of the barrier
#pragma unroll
    for (int k = 0; k < kBinPer; ++k) {
        const int64_t i = base + (int64_t)k * kBinBlock + threadIdx.x;
        const int R = Rk[k];
        const double c[3] = {ck[k][0], ck[k][1], ck[k][2]};
        double px, py;
        project_vals([&](int f) { return s_cam[f][R]; }, c, px, py);
        int q = 0, r = 0;
        const bool inb = i < a.n, ok = inb && window_ok(sc, px, py, wid, &q, &r);
        if (!ok) q = r = 0;
        tl[k] = ok ? 0 : inb ? -1 : -2;   // -2: past the batch
        qk[k] = q;
        rk[k] = r;
        // the stores ahead of the bit load: the wait for the last load then
        // waits for nothing behind it
        if (inb) {
            a.xy[2 * i] = px;
            a.xy[2 * i + 1] = py;
        }
        if (inb && !ok) settle(i);
        fk[k] = flat ? flat[((int64_t)r * sc.W + q) * (mt.VP >> 4) + (R >> 4)] : 0;
    }
#pragma unroll
    for (int k = 0; k < kBinPer; ++k) {
        const bool cst = (fk[k] >> (Rk[k] & 15)) & 1;
        if (tl[k] < 0) continue;
        const int64_t i = base + (int64_t)k * kBinBlock + threadIdx.x;
        if (cst) {
            tl[k] = -1;
            settle(i);
            continue;
        }
        const int R = Rk[k], q = qk[k], r = rk[k];
        const int tx = q / MVS_TILE_W, ty = r / MVS_TILE_H;
        const int tile = ty * t.ntx + tx;
        tl[k] = tile;
        pk[k] = (q - tx * MVS_TILE_W) | ((r - ty * MVS_TILE_H) << 4) | (R << 7);
        if (LDSHIST) {
            lr[k] = atomicAdd(&hist[tile], 1);
        } else {
            lr[k] = atomicAdd(&t.tile_count[tile * kTcStride], 1);
            // implicit items: the candidate that opens chunk j >= 1 appends it
            if (t.implicit && lr[k] > 0 && lr[k] < t.cap && lr[k] % t.chunk == 0)
                t.items[t.item_seg + atomicAdd(&t.n_items[32], 1)] = make_int4(tile, lr[k] / t.chunk, 0, 0);
        }
    }
    STAMP(t1);
    if constexpr (RUNS) {
        static_assert(LDSHIST, "the runs come from the LDS histogram");
        // exclusive scan of hist[0, ntiles): a thread sums its contiguous
        // tiles, wave scans, one cross-wave step
        __shared__ int s_w[kBinBlock / 64];
        __syncthreads();
        const int per = (t.ntiles + kBinBlock - 1) / kBinBlock;
        const int k0 = min((int)threadIdx.x * per, t.ntiles), k1 = min(k0 + per, t.ntiles);
        int mine = 0;
        for (int k = k0; k < k1; ++k) mine += hist[k];
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if ((threadIdx.x & 63) >= d) incl += o;
        }
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        int run = incl - mine, total = 0;
#pragma unroll
        for (int w = 0; w < kBinBlock / 64; ++w) {
            const int c = s_w[w];
            if (w < (int)(threadIdx.x >> 6)) run += c;
            total += c;
        }
        for (int k = k0; k < k1; ++k) {
            const int c = hist[k];
            hist[k] = run;   // start[tile]
            run += c;
        }
        __syncthreads();
        STAMP(t2);
        uint16_t* orow = t.offs + (int64_t)blockIdx.x * (t.ntiles + 1);
        for (int k = threadIdx.x; k <= t.ntiles; k += kBinBlock) orow[k] = (uint16_t)(k < t.ntiles ? hist[k] : total);
        int2* myrun = t.runs + (int64_t)blockIdx.x * MVS_BIN_CHUNK;
#pragma unroll
        for (int k = 0; k < kBinPer; ++k) {
            const int64_t i = base + (int64_t)k * kBinBlock + threadIdx.x;
            if (tl[k] < 0) continue;
            myrun[hist[tl[k]] + lr[k]] = make_int2((int32_t)i, pk[k]);
        }
        STAMP(t3);
        STAMP_ADD_ROW(2048 + blockIdx.x, 0, 1);
        STAMP_ADD_ROW(2048 + blockIdx.x, 1, t1 - t0);
        STAMP_ADD_ROW(2048 + blockIdx.x, 2, t2 - t1);
        STAMP_ADD_ROW(2048 + blockIdx.x, 3, t3 - t2);
        return;
    }
    if (LDSHIST) {
        // the workgroup's base in every tile it touched: every thread's
        // returning atomics in flight together (ntiles <= 16 x 1024)
        __syncthreads();
        int bs[kBinLdsTiles / kBinBlock];
#pragma unroll
        for (int j = 0; j < kBinLdsTiles / kBinBlock; ++j) {
            const int b = threadIdx.x + j * kBinBlock;
            const int c = b < t.ntiles ? hist[b] : 0;
            bs[j] = c ? atomicAdd(&t.tile_count[b * kTcStride], c) : 0;
        }
        auto bs_tile = [&](int jj) { return (int)threadIdx.x + jj * kBinBlock; };
        if (t.implicit) {
            // implicit items: the workgroup whose share of a tile's bucket
            // holds the first entry of chunk j >= 1 (below cap) appends (tile, j)
#pragma unroll
            for (int j = 0; j < kBinLdsTiles / kBinBlock; ++j) {
                const int b = bs_tile(j);
                const int c = b < t.ntiles ? hist[b] : 0;
                const int end = min(bs[j] + c, t.cap);
                for (int q = max((bs[j] + t.chunk - 1) / t.chunk, 1); c > 0 && q * t.chunk < end; ++q)
                    t.items[t.item_seg + atomicAdd(&t.n_items[32], 1)] = make_int4(b, q, 0, 0);
            }
        }
        __syncthreads();   // every thread has read the counts it needs
#pragma unroll
        for (int j = 0; j < kBinLdsTiles / kBinBlock; ++j) {
            const int b = bs_tile(j);
            if (b < t.ntiles) hist[b] = bs[j];
        }
        __syncthreads();
    }
    STAMP(t2);
    // straight into the tile's bucket (no separate scatter pass); past the
    // bucket's capacity to the direct path's list (counted: mvs_scorer_stats)
    int over = 0;
#pragma unroll
    for (int k = 0; k < kBinPer; ++k) {
        const int64_t i = base + (int64_t)k * kBinBlock + threadIdx.x;
        if (tl[k] < 0) continue;
        const int rank = (LDSHIST ? hist[tl[k]] : 0) + lr[k];
        if (rank < t.cap) {
            t.sorted[(int64_t)tl[k] * t.cap + rank] = make_int2((int32_t)i, pk[k]);
        } else {
            t.fix_list[atomicAdd(t.fix_count, 1)] = make_int4((int32_t)i, tl[k], pk[k], 0);
            ++over;
        }
    }
    if (t.stats && __ballot(over != 0)) {
        over = wave_sum(over);
        if ((threadIdx.x & 63) == 0) atomicAdd(&t.stats[1], (unsigned long long)over);
    }
    STAMP(t3);
    STAMP_ADD_ROW(2048 + blockIdx.x, 0, 1);
    STAMP_ADD_ROW(2048 + blockIdx.x, 1, t1 - t0);
    STAMP_ADD_ROW(2048 + blockIdx.x, 2, t2 - t1);
    STAMP_ADD_ROW(2048 + blockIdx.x, 3, t3 - t2);
}

}  // namespace

MVS_STAMPS_READER(mvs_read_stamps_bin)

extern "C" int mvs_tiled_uses_runs(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t, const MomentsDev* mt) {
    const int64_t nbin = (a->n + MVS_BIN_CHUNK - 1) / MVS_BIN_CHUNK;
    const bool dense = sc->V <= kGroupViews && mt && a->n >= (int64_t)kImplicitMean * t->ntiles;
    const bool fits = t->ntiles <= kBinLdsTiles && nbin <= std::min(t->runs_max, kRunsLimit);
    return dense && a->n > 0 && fits && t->runs && t->offs ? 1 : 0;
}

extern "C" const char* mvs_timed_kernel_name(int V, int wid, int tiled) {
    (void)wid;
    if (!tiled) return "k_score";
    if (tiled == 2) return "k_score_tab";
    return V > kGroupViews ? "k_score_mma_v" : "k_score_mma";
}

extern "C" int mvs_launch_score_tiled(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t, int wid,
                                      const MomentsDev* mt, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (wid < 1 || wid > MVS_MAX_WID) return -2;
    if (a->n == 0) return 0;
    const bool grouped = sc->V > kGroupViews;
    if (t->tw != MVS_TILE_W || t->th != MVS_TILE_H || t->items == nullptr ||
        t->chunk != (grouped ? kGroupChunk : kMmaChunk) || t->groups != (grouped ? (sc->V + 63) / 64 : 1) ||
        sc->V > MVS_MAX_VIEWS)
        return -3;
    // tile counters and the control block (queue heads, fix_count, n_items)
    // of this parity: zeroed by the previous batch's k_bin, unless
    // zero_first (both sets)
    if (t->zero_first &&
        (hipMemsetAsync(t->tile_count, 0, sizeof(int32_t) * tc_words(t->ntiles), s) != hipSuccess ||
         hipMemsetAsync(t->zero_blk, 0, sizeof(int32_t) * t->zero_words, s) != hipSuccess))
        return -1;
    const int64_t per_block = (int64_t)kBinBlock * kBinPer;
    const int nbin = (int)((a->n + per_block - 1) / per_block);
    // k_score_tab on a dense batch (>= kImplicitMean candidates per tile on
    // average: every tile holds some, so an empty item is rare) takes the
    // tiles themselves as its items, in tile order, and needs no k_item_scan
    TiledArgs tv = *t;
    tv.implicit = (!grouped && mt && a->n >= (int64_t)kImplicitMean * t->ntiles) ? 1 : 0;
    // the runs path: k_score_tab on a dense batch of few enough binning
    // workgroups (one run per gathering lane); everything else keeps the
    // atomic tile buckets
    tv.nbin = nbin;
    tv.use_runs = mvs_tiled_uses_runs(sc, a, t, mt);
    // with the scene's moment tables k_bin also settles the candidates whose
    // reference window is constant (they pass no view) without binning them
    const MomentsDev mflat = mt ? *mt : MomentsDev{};
    if (tv.use_runs)
        hipLaunchKernelGGL((k_bin<true, true>), dim3(nbin), dim3(kBinBlock), (size_t)t->ntiles * 4, s, *sc, *a, tv, wid, mflat);
    else if (t->ntiles <= kBinLdsTiles)
        hipLaunchKernelGGL(k_bin<true>, dim3(nbin), dim3(kBinBlock), (size_t)t->ntiles * 4, s, *sc, *a, tv, wid, mflat);
    else
        hipLaunchKernelGGL(k_bin<false>, dim3(nbin), dim3(kBinBlock), 0, s, *sc, *a, tv, wid, mflat);
    // the work items in tile order (the scorers' workgroups in flight then
    // share image rows -- and at V > 64 table rows -- in L2)
    if (!tv.implicit) hipLaunchKernelGGL(k_item_scan, dim3(1), dim3(kScanThreads), 0, s, tv);
    t = &tv;
    int rc = 0;
    {
        TimedLaunch tl(s, ev0, ev1);
        if (grouped) rc = mvs_launch_score_mma_v(sc, a, t, mt, wid, s);
        else if (mt) rc = mvs_launch_score_tab(sc, a, t, mt, s);   // window moments from the scene's tables
        else rc = mvs_launch_score_mma(sc, a, t, wid, s);
    }
    if (rc) return rc;
    return mvs_launch_score_fix(sc, a, t, wid, s);
}
