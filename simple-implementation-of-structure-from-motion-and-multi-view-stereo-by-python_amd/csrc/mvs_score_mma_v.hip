// ---------------------------------------------------------------------------
// k_score_mma_v (64 < V <= 256): the views in groups of 64 (one mask word
// each).  A workgroup takes one work item (the candidates of one 16x8 tile,
// at most kGroupChunk of them) from the queue and scores it against every
// view group in turn:
//   0. (per item) the candidate list is sorted by the candidate's row in the
//      tile (counting sort over 8 rows), so that an M-block of 16 candidates
//      spans few region rows and its K-loop skips the K-steps none of its
//      windows reaches;
//   1. (per item) each candidate's own reference window rows go to LDS by
//      LDS-DMA (its view is usually in another group); behind group 0's
//      phase 2 they are masked in place to the window's columns (the A
//      operands need no masking afterwards), S_a and S_aa summed per row by
//      every thread, and the decision constants derived;
//   2. (per group) Q = S_bb of every (pixel, view) of the group (int32; -1
//      past V): one thread per (pixel column, view) sums its column's window
//      rows straight from the staged region (masked v_dot4_i32_i8) and slides
//      them down the tile;
//   3. (per group) wave tasks (M-block of 16 candidates, 32 views): C = sum
//      s_R s_v and S_b = sum s_v over the window, both by
//      v_mfma_i32_16x16x64_i8 (S_b with the window's 0/1 indicator row as A,
//      from a 16-entry table by the window's column); D = n Q - S_b^2 and
//      num = n C - S_a S_b (24-bit multiplies: |S_b| < 2^14, Q < 2^21); the
//      decision num w_b > T in binary32 with w_b = v_rsq_f32(D) (guard band
//      2e-6 |T| as in k_score_mma; D = 0, a constant window, gives
//      0 * inf = nan and never passes), the sum of the passing num w_b with
//      w_b refined in binary64 (one Newton step);
//   4. (per group) each candidate's mask word, count, sum and guard flag
//      accumulate in its thread's registers; written after the last group
//      (guard-band candidates to k_score_fix).
// The regions are double-buffered: group k+1's (after an item's last group,
// the next item's first) lands by LDS-DMA while group k is scored, as do the
// next item's candidate list and, behind group 0's phase 2, an item's
// reference rows.  Every LDS-DMA target is a static LDS array of its own, so
// that the compiler sees no aliasing with the tables phases 2-4 read and
// write.  Work items come in tile order (k_item_scan): the workgroups in flight
// share image rows, so TLB and L2 reach over 256 views of a large image.
// ---------------------------------------------------------------------------
#include "mvs_mma.h"
#include "mvs_stamps.h"

namespace {

constexpr int kVTab = 68;   // Q-table row pitch (int32): the per-column writes are conflict free

// a candidate's constants (LDS, per item)
struct alignas(16) CandInfoV {
    int32_t px, R, Sa, pk;    // Q-table row of its pixel (px * kVTab), reference view, -S_a, packed pixel
    float T, gT;              // decision threshold on num w_b and its guard band
    double ca;                // n / (n-1) * w_a
};

// dynamic LDS of k_score_mma_v (the LDS-DMA targets are static arrays)
struct VLds {
    int qtab, ci, rmask, rguard, rsum, total;
};

template <bool TAB>
__host__ __device__ constexpr VLds v_lds() {
    VLds L{};
    L.qtab = 0;                                                 // [128 px][kVTab] int32 (TAB: none)
    L.ci = L.qtab + (TAB ? 0 : 128 * kVTab * 4);
    L.rmask = L.ci + kGroupChunk * (int)sizeof(CandInfoV);      // [cand][4 view blocks] u16 (item start:
                                                                // [cand] {S_a, S_aa} int32 sums)
    L.rguard = L.rmask + kGroupChunk * 4 * 2;                   // [cand][2 halves] u16
    L.rsum = L.rguard + kGroupChunk * 2 * 2 + 8;                // [cand][2 halves] double (8-B aligned)
    L.total = L.rsum + kGroupChunk * 2 * 8;
    return L;
}

template <int WID>
__host__ __device__ constexpr int v_static_lds() {
    return 2 * 64 * MmaGeom<WID>::VS + 2 * kGroupChunk * 8 + kGroupChunk * MmaGeom<WID>::NB * 32 + 16 +
           16 * 32 + 16 + 16 + 16 * 4;
}


// byte masks of a window of NB bytes starting at byte b0 over the 4 dwords
// from dword b0 >> 2
template <int NB>
DEV void window_dword_masks(int b0, uint32_t (&mk)[4]) {
    const int e = b0 + NB;   // one past the last byte
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int base = 4 * ((b0 >> 2) + j);
        const int lo = max(b0 - base, 0), n = min(e - base, 4) - lo;   // bytes [lo, lo + n) of dword j
        mk[j] = n > 0 ? (uint32_t)(((1ull << (8 * n)) - 1ull) << (8 * lo)) : 0u;
    }
}

// 1/sqrt(D) in binary64: v_rsq_f64 + one Newton step (max relative error
// 4.1e-15 over 4M values of D < 2^31, tools/ubench/rsq_acc.hip); nan for D <= 0
DEV double rsqrt_nr(int D) {
    double w = __builtin_nan("");
    if (D > 0) {
        const double x = (double)D;
        w = __builtin_amdgcn_rsq(x);
        w = w * (1.5 - 0.5 * x * w * w);
    }
    return w;
}

template <int WID, bool FAST, bool TAB>
__global__ __launch_bounds__(kMmaThreads) void k_score_mma_v(const SceneDev sc, const ScoreArgs a, const TiledArgs t,
                                                             const MomentsDev mt, const int4* __restrict__ items,
                                                             const int2* __restrict__ sorted) {
    using G = MmaGeom<WID>;
    constexpr int NB = G::NB, NPX = G::NPX, ROWS = G::ROWS, VS = G::VS, C0 = G::C0;
    constexpr int RPV = VS / 32;
    constexpr int NPIECE = 64 * RPV * 2;                                              // 16-B pieces of a region
    constexpr int RPIECE = (NPIECE + kMmaThreads - 1) / kMmaThreads;                  // ... per thread
    constexpr int APIECE = (kGroupChunk * NB * 2 + kMmaThreads - 1) / kMmaThreads;   // reference-row pieces
    constexpr int AROW = (kGroupChunk * NB + kMmaThreads - 1) / kMmaThreads;         // reference rows per thread
    static_assert(kGroupChunk <= 128, "one phase-3 task per wave; the sort ranks two waves");
    // LDS-DMA targets: two regions, the candidate list as it lands (s_cd0) and
    // sorted by row (s_cd1), the reference rows
    __shared__ __attribute__((aligned(16))) uint8_t s_rg0[64 * VS], s_rg1[64 * VS];
    __shared__ __attribute__((aligned(16))) uint8_t s_cd0[kGroupChunk * 8], s_cd1[kGroupChunk * 8];
    // the reference rows, then 16 zero bytes (never an LDS-DMA target): phase
    // 3 reads a row or the zeros through an offset select inside the one
    // array, so that the read carries the array's alias scope and waits for
    // no LDS-DMA in flight (a select between two arrays would wait for all)
    constexpr int AZERO = kGroupChunk * NB * 32;
    __shared__ __attribute__((aligned(16))) uint8_t s_areg[AZERO + 16];
    // the window indicator rows by window column (0/1 bytes), then 16 zeros
    __shared__ __attribute__((aligned(16))) uint8_t s_ind[16 * 32 + 16];
    __shared__ int s_item;
    __shared__ __attribute__((aligned(16))) int32_t s_cnt[16];   // the sort's per-wave row counts
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr VLds L = v_lds<TAB>();
    const int16_t* __restrict__ tsb = mt.sb;   // TAB: S_b and D = n S_bb - S_b^2 per (pixel, view)
    const int32_t* __restrict__ tdd = mt.d;
    const int VPt = mt.VP;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int V = sc.V;
    const int NG = t.groups;
    int32_t* qtab = (int32_t*)(smem + L.qtab);
    CandInfoV* ci = (CandInfoV*)(smem + L.ci);
    uint16_t* rmask = (uint16_t*)(smem + L.rmask);
    int32_t* asums = (int32_t*)(smem + L.rmask);   // item start only: {S_a, S_aa} per candidate
    uint16_t* rguard = (uint16_t*)(smem + L.rguard);
    double* rsum = (double*)(smem + L.rsum);
    const double kn = (double)NPX / (double)(NPX - 1);
    const float tqf = (float)(a.thr / kn);
    ItemMap im;
    im.load(t);
    const int n_items = im.total();
    int32_t* head = t.head;

    // region piece k (view k / 2RPV, row, half) of view group g at a tile: its
    // gv address; rows outside the image are clamped (their pixels are never
    // in a valid window), views past V repeat the last (never used)
    auto region_src = [&](int tile, int g, int k) -> const uint8_t* {
        const int ty = tile / t.ntx, tx = tile - ty * t.ntx;
        const int v = k / (2 * RPV), r2 = k - v * (2 * RPV);
        const int y = min(max(ty * MVS_TILE_H - WID + (r2 >> 1), 0), sc.H - 1);
        const int view = min(g * 64 + v, V - 1);
        return sc.gv + ((int64_t)view * sc.H + y) * sc.Wp + (tx * MVS_TILE_W - 8) + 16 * (r2 & 1);
    };
    auto stage_region = [&](int tile, int g, auto bufc) {
        uint8_t* dst = decltype(bufc)::value ? s_rg1 : s_rg0;
        const int tv = opaque(tid);   // per-lane addressing recomputed here, not held across the loop
#pragma unroll
        for (int p = 0; p < RPIECE; ++p) {
            const int k = tv + p * kMmaThreads;
            if (k < NPIECE)
                __builtin_amdgcn_global_load_lds((const void*)region_src(tile, g, k),
                                                 (void __attribute__((address_space(3)))*)(dst + (p * kMmaThreads + wave * 64) * 16),
                                                 16, 0, 0);
        }
    };
    // an item's candidate list always lands in s_cd0 (free once sorted into s_cd1)
    auto stage_cands = [&](const int4 d) {
        const int32_t* csrc = (const int32_t*)(sorted + d.y);
        if (tid < 2 * d.z)
            __builtin_amdgcn_global_load_lds((const void*)(csrc + tid),
                                             (void __attribute__((address_space(3)))*)(s_cd0 + wave * 64 * 4),
                                             4, 0, 0);
    };

    // the items in contiguous bands of tiles, band x claimed first by the
    // workgroups b = x mod kBandHeads (one band per XCD under round-robin
    // dispatch: an XCD's workgroups in flight take neighbouring tiles and
    // share their regions' lines in its L2; ring256 0.498 vs 0.506 ms with
    // one queue, profiles/r06/r6n_*)
    const int ob = (int)blockIdx.x % kBandHeads;
    int cb = ob;   // thread 0's current band
    auto claim_item = [&]() -> int {
        return band_claim(head + (3 + kItemSegs) * 32, cb, ob, kBandHeads, n_items, [](int) { return 0; });
    };
    // the first item: its candidates and group 0's region; the indicator rows
    if (tid == 0) s_item = claim_item();
    if (tid < 16 * 8) {   // indicator row q: bytes [q + C0, q + C0 + NB) are 1
        const int q = tid >> 3, j = tid & 7;
        const uint32_t wm = ((1u << NB) - 1u) << (q + C0);
        ((uint32_t*)s_ind)[tid] = byte_mask((wm >> (4 * j)) & 15u) & 0x01010101u;
    } else if (tid < 16 * 8 + 4) {
        ((uint32_t*)(s_ind + 16 * 32))[tid - 16 * 8] = 0u;
        ((uint32_t*)(s_areg + AZERO))[tid - 16 * 8] = 0u;
    }
    __syncthreads();
    int item = __builtin_amdgcn_readfirstlane(s_item);
    if (item >= n_items) return;
    int4 d = item_desc(t, items, im, item);
    stage_cands(d);
    stage_region(d.x, 0, std::integral_constant<int, 0>{});
    __syncthreads();
    int kpar = 0;    // region buffer of this group (groups alternate across items)

    for (;;) {
        const int tile = d.x, nc = d.z;
        const int ty = tile / t.ntx;
        const int x0 = (tile - ty * t.ntx) * MVS_TILE_W;
        const int2* cand = (const int2*)s_cd1;
        // ---- 0. the candidates sorted by row (counting sort, two waves) ----
        {
            const int2 e = tid < nc ? ((const int2*)s_cd0)[tid] : make_int2(0, 0);
            const int key = (e.y >> 4) & 7;
            int rank = 0;
            if (wave < 2) {
                int cntv = 0;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const uint64_t m = __ballot(tid < nc && key == r);
                    if ((tid & 63) == r) cntv = __popcll(m);
                    if (key == r) rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                }
                if ((tid & 63) < 8) s_cnt[wave * 8 + (tid & 63)] = cntv;
            }
            if (tid < 2 * kGroupChunk) asums[tid] = 0;
            lds_barrier();
            if (tid < nc) {
                int pos = rank;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int c0 = s_cnt[r], c1 = s_cnt[8 + r];
                    pos += (r < key ? c0 + c1 : 0) + (r == key && wave == 1 ? c0 : 0);
                }
                ((int2*)s_cd1)[pos] = e;
            }
            lds_barrier();
        }
        const int my_idx = tid < nc ? cand[tid].x : 0;
        // ---- 1. the candidates' reference rows (they land behind phase 2) ----
        // (the candidate entries are read first: an LDS read between two
        // LDS-DMA issues would wait for the first)
        const int tv = opaque(tid);
        int pks[APIECE];
#pragma unroll
        for (int p = 0; p < APIECE; ++p) {
            const int k = tv + p * kMmaThreads;
            pks[p] = k < nc * NB * 2 ? cand[k / (2 * NB)].y : 0;
        }
#pragma unroll
        for (int p = 0; p < APIECE; ++p) {
            const int k = tv + p * kMmaThreads;
            if (k < nc * NB * 2) {
                const int kk = k / (2 * NB), r2 = k - kk * (2 * NB);
                const int pk = pks[p];
                const int y = ty * MVS_TILE_H + ((pk >> 4) & 7) - WID + (r2 >> 1);   // inside: the window is valid
                const uint8_t* src = sc.gv + ((int64_t)(pk >> 7) * sc.H + y) * sc.Wp + (x0 - 8) + 16 * (r2 & 1);
                __builtin_amdgcn_global_load_lds((const void*)src,
                                                 (void __attribute__((address_space(3)))*)(s_areg + (p * kMmaThreads + wave * 64) * 16),
                                                 16, 0, 0);
            }
        }

        int next = n_items;
        int4 dn = make_int4(0, 0, 0, 0);
        int acnt = 0;
        double asum = 0.0;
        uint32_t aguard = 0;
        uint64_t pend = 0;   // the previous group's mask word, stored during this group's phase 2

        // one view group; its region is in s_rg<buf>
        auto group = [&](const int g, auto bufc) {
            constexpr int buf = decltype(bufc)::value;
            // the per-lane maps, recomputed per group rather than held in
            // registers across the item loop
            const int tid = opaque(threadIdx.x), lane = tid & 63;
            const int m = lane & 15, kh = lane >> 4;
            // phase 2 map: thread = (pixel column mx, view mv); 16 columns x 4 views per wave
            const int mx = tid & 15, mv = tid >> 4;
            uint32_t cmk[4];
            window_dword_masks<NB>(mx + C0, cmk);
            const int cd0 = (mx + C0) >> 2;
            const uint8_t* reg = buf ? s_rg1 : s_rg0;
            STAMP(t0);
            const int vb = g * 64;
            const int GV = min(64, V - vb);
            const bool last = g + 1 == NG;
            // the next region (group g+1, or the next item's group 0) and, after
            // the last group, the next item's candidates land during phases 3-4
            auto prefetch = [&]() {
                if (!last) {
                    stage_region(tile, g + 1, std::integral_constant<int, buf ^ 1>{});
                } else if (next < n_items) {
                    stage_cands(dn);
                    stage_region(dn.x, 0, std::integral_constant<int, buf ^ 1>{});
                }
            };
            // group 0: thread 0 claims the next item; the result is in by the
            // barrier after phase 2, which waits for the reference rows anyway
            // (claimed inside the group loop: a VGPR loaded before the loop and
            // read in it would make the compiler drain every load at loop entry)
            int claim = 0;
            if (g == 0 && tid == 0) claim = claim_item();
            // ---- 2. Q = S_bb of every (pixel, view) of the group ----
            // (TAB: none, the scene's tables hold S_b and D)
            if (TAB) {
            } else if (mv < GV) {
                // rows in order, the window sliding down as they come: at most
                // NB + 1 row sums live
                int Q[ROWS];
                const uint8_t* col = reg + mv * VS + 4 * cd0;
                int q = 0;
#pragma unroll
                for (int rho = 0; rho < ROWS; ++rho) {
                    int qr = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int dm = (int)(*(const uint32_t*)(col + rho * 32 + 4 * j) & cmk[j]);
                        qr = __builtin_amdgcn_sdot4(dm, dm, qr, false);
                    }
                    Q[rho] = qr;
                    q += qr;
                    if (rho >= NB) q -= Q[rho - NB];
                    if (rho >= NB - 1) qtab[((rho - (NB - 1)) * 16 + mx) * kVTab + mv] = q;
                }
            } else {
#pragma unroll
                for (int y = 0; y < MVS_TILE_H; ++y) qtab[(y * 16 + mx) * kVTab + mv] = -1;   // D < 0: nan
            }
            (void)mx; (void)mv; (void)cmk; (void)cd0;
            STAMP(t0a);
            // (and, group 0, the reference rows have landed; nothing else is in
            // flight, so the LDS reads of phases 3-4 need no waits)
            __syncthreads();
            STAMP(t0b);
            if (g == 0) {
                if (tid == 0) s_item = claim;   // published by the barriers below
                // the reference rows masked in place to their window's columns,
                // and their sums: one thread per (candidate, row)
#pragma unroll
                for (int p = 0; p < AROW; ++p) {
                    const int k = tid + p * kMmaThreads;
                    if (k < nc * NB) {
                        const int qrel = cand[k / NB].y & 15;
                        const uint32_t wm = ((1u << NB) - 1u) << (qrel + C0);
                        uint4* row = (uint4*)(s_areg + k * 32);
                        uint4 h0 = row[0], h1 = row[1];
                        h0.x &= byte_mask(wm & 15u);
                        h0.y &= byte_mask((wm >> 4) & 15u);
                        h0.z &= byte_mask((wm >> 8) & 15u);
                        h0.w &= byte_mask((wm >> 12) & 15u);
                        h1.x &= byte_mask((wm >> 16) & 15u);
                        h1.y &= byte_mask((wm >> 20) & 15u);
                        h1.z &= byte_mask((wm >> 24) & 15u);
                        h1.w &= byte_mask(wm >> 28);
                        row[0] = h0;
                        row[1] = h1;
                        int s = 0, q = 0;
                        const uint32_t dw[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            s = __builtin_amdgcn_sdot4((int)dw[j], 0x01010101, s, false);
                            q = __builtin_amdgcn_sdot4((int)dw[j], (int)dw[j], q, false);
                        }
                        atomicAdd(&asums[2 * (k / NB)], s);
                        atomicAdd(&asums[2 * (k / NB) + 1], q);
                    }
                }
                lds_barrier();
                // the candidates' constants
                if (tid < nc) {
                    const int pk = cand[tid].y;
                    const int s = asums[2 * tid], q = asums[2 * tid + 1];
                    const double wa = rsqrt_nr(NPX * q - s * s);
                    CandInfoV c;
                    // the pixel's row: of the Q table, or (TAB) of the scene's tables
                    c.px = TAB ? ((ty * MVS_TILE_H + ((pk >> 4) & 7)) * sc.W + x0 + (pk & 15)) * VPt
                               : (pk & 127) * kVTab;
                    c.R = pk >> 7;
                    c.Sa = -s;
                    c.pk = pk;
                    c.T = tqf * __builtin_amdgcn_rcpf((float)wa);   // nan for a constant window
                    c.gT = 2e-6f * fabsf(c.T);
                    c.ca = kn * wa;
                    ci[tid] = c;
                }
                lds_barrier();
                next = __builtin_amdgcn_readfirstlane(s_item);
                if (next < n_items) dn = item_desc(t, items, im, next);
            }
            STAMP(t1);
            prefetch();
            // the previous group's mask word: its store has phases 3-4 to complete
            // (the barrier after phase 4 waits for it with the region's LDS-DMA)
            if (g > 0 && tid < nc) a.mask[(int64_t)my_idx * a.mstride + g - 1] = pend;
            asm volatile("" ::: "memory");   // the LDS-DMA issues stay ahead of phase 3
            STAMP(tpf);

            // ---- 3. wave task (M-block b, views 32 h + [0, 32)) ----
            const int nblk = (nc + 15) >> 4;
            if (wave < nblk * 2) {
                const int b = wave >> 1, h = wave & 1;
                const int kk = b * 16 + m;
                const bool valid = kk < nc;
                const int pk = valid ? ci[kk].pk : 0;
                const int qrel = pk & 15, rrel = (pk >> 4) & 7;
                // the block's rows (sorted): K-steps s0..s1 hold every window row
                const int r_lo = __builtin_amdgcn_readfirstlane((ci[b * 16].pk >> 4) & 7);
                const int r_hi = __builtin_amdgcn_readfirstlane((ci[min(b * 16 + 15, nc - 1)].pk >> 4) & 7);
                const int s0 = r_lo >> 1, s1 = (r_hi + NB - 1) >> 1;
                const int lofs = 32 * (kh >> 1) + 16 * (kh & 1);
                // region row 2s + (kh >> 1) = window row 2s + (kh >> 1) - rrel of the candidate
                const int aoff = (min(kk, nc - 1) * NB - rrel) * 32 + 16 * (kh & 1);
                const int ioff = qrel * 32 + 16 * (kh & 1);
                const uint8_t* bptr0 = reg + min(32 * h + m, GV - 1) * VS + lofs;
                const uint8_t* bptr1 = reg + min(32 * h + 16 + m, GV - 1) * VS + lofs;
                v4i C0v = {0, 0, 0, 0}, C1v = {0, 0, 0, 0}, S0v = {0, 0, 0, 0}, S1v = {0, 0, 0, 0};
                auto kstep = [&](const int s) {
                    const int row = 2 * s + (kh >> 1);
                    const bool rv = valid && row >= rrel && row < rrel + NB;
                    // rows outside the window read 16 zero bytes: an offset select
                    // instead of a branch around the load
                    const uint4 av = *(const uint4*)(s_areg + (rv ? aoff + row * 32 : AZERO));
                    const uint4 iv = *(const uint4*)(s_ind + (rv ? ioff : 16 * 32));
                    const v4i AI = {(int)iv.x, (int)iv.y, (int)iv.z, (int)iv.w};
                    const v4i A = {(int)av.x, (int)av.y, (int)av.z, (int)av.w};
                    const uint4 b0 = *(const uint4*)(bptr0 + 64 * s);
                    const uint4 b1 = *(const uint4*)(bptr1 + 64 * s);
                    const v4i B0 = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w};
                    const v4i B1 = {(int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
                    C0v = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B0, C0v, 0, 0, 0);
                    C1v = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B1, C1v, 0, 0, 0);
                    if constexpr (!TAB) {
                        S0v = __builtin_amdgcn_mfma_i32_16x16x64_i8(AI, B0, S0v, 0, 0, 0);
                        S1v = __builtin_amdgcn_mfma_i32_16x16x64_i8(AI, B1, S1v, 0, 0, 0);
                    } else {
                        (void)AI;
                    }
                };
                // every window takes KMIN K-steps: those unrolled from sb (loads
                // issued ahead of the MFMAs), the block's further ones after
                constexpr int KMIN = (NB + 2) / 2;
                const int sb = min(s0, G::KS - KMIN);
#pragma unroll
                for (int u = 0; u < KMIN; ++u) kstep(sb + u);
                for (int s = sb + KMIN; s <= s1; ++s) kstep(s);
                // lane (kh, m) holds candidate 16 b + 4 kh + i, views vb + 32 h + 16 j + m
                uint32_t pmv = 0, gdv = 0;
                double sacc[4];
                // TAB: S_b and D of candidate 4 kh + i's pixel at views vb + 32 h +
                // 16 j + m from the tables, one candidate step ahead of their use
                int tsbv[2][2], tdv[2][2];
                auto tfetch = [&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    if constexpr (TAB) {
                        const int px = ci[min(b * 16 + 4 * kh + i, nc - 1)].px + vb + 32 * h + m;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            tsbv[i & 1][j] = tsb[px + 16 * j];
                            tdv[i & 1][j] = tdd[px + 16 * j];
                        }
                    }
                };
                tfetch(std::integral_constant<int, 0>{});
                static_for<4>([&](auto Ic) {
                    constexpr int i = Ic;
                    if constexpr (i < 3) tfetch(std::integral_constant<int, i + 1>{});
                    const CandInfoV c = ci[min(b * 16 + 4 * kh + i, nc - 1)];
                    double sa = 0.0;
                    uint64_t gacc = 0;
                    static_for<2>([&](auto Jc) {
                        constexpr int j = Jc;
                        const int vl = 32 * h + 16 * j + m;
                        const int Sb = TAB ? tsbv[i & 1][j] : (j ? S1v[i] : S0v[i]);
                        const int D = TAB ? tdv[i & 1][j]
                                          : __mul24(NPX, qtab[c.px + vl]) - __mul24(Sb, Sb);   // < 0 past V: nan
                        const float wf = __builtin_amdgcn_rsqf((float)D);
                        const int num = __mul24(c.Sa, Sb) + __mul24(NPX, j ? C1v[i] : C0v[i]);
                        const uint64_t liv = __builtin_amdgcn_uicmp((uint32_t)(vb + vl), (uint32_t)c.R, 33);
                        // w_b in binary64: one Newton step from the binary32 estimate
                        double w = (double)wf;
                        w = w * (1.5 - 0.5 * (double)D * w * w);
                        uint64_t P, Gd;
                        if constexpr (FAST) {
                            const float x = fmaf((float)num, wf, -c.T);
                            P = __builtin_amdgcn_fcmpf(x, 0.0f, 2) & liv;
                            Gd = __builtin_amdgcn_fcmpf(fabsf(x), c.gT, 4) & liv;
                        } else {
                            const double ncc = (double)num * w * c.ca;
                            P = __ballot(vb + vl != c.R && ncc > a.thr);
                            Gd = __ballot(vb + vl != c.R && fabs(ncc - a.thr) <= kGuard);
                        }
                        pmv = writelane<2 * (2 * i + j)>(pmv, (uint32_t)P);
                        pmv = writelane<2 * (2 * i + j) + 1>(pmv, (uint32_t)(P >> 32));
                        gacc |= Gd;
                        sa = fma_f64_lanes(sa, num, w, P);
                    });
                    gdv = writelane<2 * i>(gdv, (uint32_t)gacc);
                    gdv = writelane<2 * i + 1>(gdv, (uint32_t)(gacc >> 32));
                    sacc[i] = sa;
                    __builtin_amdgcn_sched_barrier(0);   // one candidate row at a time: register pressure
                });
                // candidate 16 b + l (l = 4 q + i): 16-bit piece q of ballot (i, j)
                {
                    const int l = lane & 15, i = l & 3, q = l >> 2;
                    const int cc = b * 16 + l;
                    uint32_t pc[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const uint32_t lo = __builtin_amdgcn_ds_bpermute(4 * (2 * (2 * i + j)), (int)pmv);
                        const uint32_t hi = __builtin_amdgcn_ds_bpermute(4 * (2 * (2 * i + j) + 1), (int)pmv);
                        pc[j] = (uint32_t)(((((uint64_t)hi << 32) | lo) >> (16 * q)) & 0xffffu);
                    }
                    const uint32_t glo = __builtin_amdgcn_ds_bpermute(4 * (2 * i), (int)gdv);
                    const uint32_t ghi = __builtin_amdgcn_ds_bpermute(4 * (2 * i + 1), (int)gdv);
                    const uint32_t gq = (uint32_t)(((((uint64_t)ghi << 32) | glo) >> (16 * q)) & 0xffffu);
                    if (lane < 16 && cc < nc) {
                        ((uint32_t*)rmask)[cc * 2 + h] = pc[0] | (pc[1] << 16);
                        rguard[cc * 2 + h] = (uint16_t)gq;
                    }
                }
                if (a.avg != nullptr) {
                    const double mine = row_sum16_x4(sacc, m);
                    const int cc = b * 16 + 4 * kh + m;
                    if (m < 4 && cc < nc) rsum[cc * 2 + h] = mine;
                }
            }
            STAMP(t1a);
            lds_barrier();
            STAMP(t2);
            // ---- 4. the group's mask word, count, sum and guard accumulate ----
            if (tid < nc) {
                const uint64_t mk = *(const uint64_t*)(rmask + tid * 4);   // views 16 nb + [0, 16) at bits 16 nb
                aguard |= rguard[tid * 2] | rguard[tid * 2 + 1];
                pend = mk;
                acnt += __popcll(mk);
                if (a.avg != nullptr && mk) asum += (rsum[tid * 2] + rsum[tid * 2 + 1]) * ci[tid].ca;
            }
            __syncthreads();   // the next region has landed
            STAMP(t3);
            STAMP_ADD(0, 1);
            STAMP_ADD(1, t1 - t0);
            STAMP_ADD(2, t2 - t1);
            STAMP_ADD(3, t3 - t2);
            STAMP_ADD(4, t0a - t0);    // wave 0: phase 2 own work
            STAMP_ADD(5, t0b - t0a);   // barrier after phase 2 (group 0: the reference rows)
            STAMP_ADD(6, t1 - t0b);    // group 0: the candidate constants
            STAMP_ADD(7, t1a - t1);    // wave 0: prefetch issue + its phase-3 task
            if (g == 0) STAMP_ADD(8, t0b - t0a);                     // barrier after phase 2, group 0 only
            STAMP_ADD_LANE0(9, t0a - t0);                            // every wave's own phase-2 work
            STAMP_ADD(10, tpf - t1);                                 // wave 0: prefetch + mask-store issue
            if (wave < ((nc + 15) >> 4) * 2) {
                STAMP_ADD_LANE0(11, t1a - tpf);                      // a task's phase-3 time (waves with tasks)
                STAMP_ADD_LANE0(12, 1);                              // tasks
            }
        };
        for (int g = 0; g < NG; ++g) {
            if (kpar) group(g, std::integral_constant<int, 1>{});
            else group(g, std::integral_constant<int, 0>{});
            kpar ^= 1;
        }
        if (tid < nc) {
            a.mask[(int64_t)my_idx * a.mstride + NG - 1] = pend;
            if (a.count) a.count[my_idx] = acnt;
            if (a.avg) a.avg[(int64_t)my_idx * a.astride] = acnt ? asum * (1.0 / (double)acnt) : 0.0;
            if (aguard) t.fix_list[atomicAdd(t.fix_count, 1)] = make_int4(my_idx, tile, cand[tid].y, 0);
        }
        if (next >= n_items) break;
        item = next;
        d = dn;
    }
}

template <int WID>
int launch_mma_v(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t, const MomentsDev* mt, hipStream_t s) {
    // (mt: the scene's S_b / D tables, or null: the Q table per item and group)
    const MomentsDev m = mt ? *mt : MomentsDev{};
    const bool fast = fabs(a->thr) >= 0.01;
#define MVS_V_LAUNCH(FAST_, TAB_)                                                                              \
    do {                                                                                                       \
        static std::atomic<uint64_t> done{0};                                                                  \
        constexpr int lds = v_lds<TAB_>().total;                                                               \
        if (set_dyn_lds_once((const void*)k_score_mma_v<WID, FAST_, TAB_>, done, lds) != 0) return -1;         \
        hipLaunchKernelGGL((k_score_mma_v<WID, FAST_, TAB_>), dim3(kMmaGrid), dim3(kMmaThreads), lds, s, *sc, \
                           *a, *t, m, (const int4*)t->items, (const int2*)t->sorted);                          \
    } while (0)
    if (mt) { if (fast) MVS_V_LAUNCH(true, true); else MVS_V_LAUNCH(false, true); }
    else { if (fast) MVS_V_LAUNCH(true, false); else MVS_V_LAUNCH(false, false); }
#undef MVS_V_LAUNCH
    return 0;
}

}  // namespace

MVS_STAMPS_READER(mvs_read_stamps_mma_v)

extern "C" int mvs_launch_score_mma_v(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t,
                                      const MomentsDev* mt, int wid, hipStream_t s) {
    return dispatch_wid(wid, -2, [&](auto w) { return launch_mma_v<decltype(w)::value>(sc, a, t, mt, s); });
}

extern "C" size_t mvs_mma_v_lds_bytes(int wid) {
    return dispatch_wid(wid, (size_t)0, [&](auto w) { return (size_t)(v_lds<false>().total + v_static_lds<decltype(w)::value>()); });
}
