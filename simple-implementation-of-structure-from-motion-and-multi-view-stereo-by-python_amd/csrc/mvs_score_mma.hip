// k_score_mma: V <= 64 without the scene's moment tables (with them: k_score_tab).
// ---------------------------------------------------------------------------
// Tiled scorer, stage 2: the candidates of a 16x8 pixel tile against every
// view on the matrix cores (v_mfma_i32_16x16x64_i8 over the tile's window
// region), one workgroup of 16 waves per CU taking work items from a dynamic
// queue: k_score_mma for V <= 64 (every view staged), k_score_mma_v for V > 64
// (64-view groups).  Both decide each (candidate, view) pair from exact
// integer window products and moments (see k_score_mma).
// ---------------------------------------------------------------------------
#include "mvs_mma.h"
#include "mvs_stamps.h"

namespace {

// ---------------------------------------------------------------------------
// k_score_mma (V <= 64).  A workgroup (16 waves) takes one work item (the
// candidates of one 16x8 pixel tile, at most kMmaChunk) from a dynamic queue:
//   1. the item's window region of every view (signed bytes s = g - 128,
//      [view][ROWS rows][32 columns], two aligned 16-B loads of gv per view
//      row) and its candidate list go to LDS; the NEXT item's region is
//      loaded into registers meanwhile (issued after this item is staged,
//      written to LDS at the top of the next iteration), so the global
//      latency hides behind phases 2-3;
//   2. per (pixel, view) of the tile: S_b and w = 1/sqrt(n S_bb - S_b^2) in
//      binary64 (NaN for a constant window: ctNcc's nan, never passes), from
//      horizontal v_dot4_i32_i8 prefix sums and vertical sums;
//   3. 16 candidates per wave and M-block: C[m][v] = sum over the window of
//      s_R s_v by v_mfma_i32_16x16x64_i8 (A = the reference window masked to
//      candidate m's window, B = view v's region), exact;
//   4. per (candidate, view): num = n C - S_a S_b (the n S_ab - S_a S_b of
//      ctNcc, shift invariant), ncc = n/(n-1) num w_a w_b, so
//      ncc > thr  <=>  num w_b > T = thr (n-1)/(n w_a): one binary32 fma,
//      with a relative guard band of 2e-6 |T| (the binary32 roundings add
//      < 3e-7 |T|); a candidate with any pair in the band is re-scored by
//      k_score_fix (numpy-order ctNcc).  avg_ncc_score = n/(n-1) w_a
//      sum(num w_b) / cnt in binary64.
// ---------------------------------------------------------------------------
// a candidate's constants in phase 3 (per wave, 32 slots: the two M-blocks
// of its unit)
struct alignas(16) CandInfo {
    int32_t osb;              // LDS byte offset of its pixel's S_b table row (the w row follows from it)
    int32_t Sa;               // -S_a
    int32_t R;                // reference view (-1: no candidate)
    float T;                  // decision threshold on num w_b (FAST: binary32; else thr)
};

// LDS layout: region | S_b table, w table (binary64), [w table (binary32)]
// (the tables alias the horizontal sums of phase 2) | per-wave candidate
// slots | the item's candidates | 32 zero bytes
struct MmaLds {
    int reg, regsz, sb, w, wf, ci, wp, cand, zero, total;
};

// Dynamic LDS of k_score_mma.  DB: the two region buffers and the two
// candidate buffers are static LDS arrays of the kernel (the next item's
// region and candidates land by LDS-DMA during this item's candidates), so
// the dynamic part holds only the tables and slots; otherwise one region and
// one candidate buffer come first.  WF: a binary32 copy of the w table.
template <int WID, int NBLK, bool WF, bool DB>
__host__ __device__ constexpr MmaLds mma_lds(int V) {
    using G = MmaGeom<WID>;
    constexpr int VP = 16 * NBLK;
    MmaLds L{};
    L.reg = 0;
    L.regsz = V * G::VS;                               // VS is a multiple of 32
    L.sb = DB ? 0 : L.regsz;
    L.w = L.sb + 128 * VP * 4;
    L.wf = L.w + 128 * VP * 8;
    const int htmp = G::ROWS * 16 * VP * 4, tab = 128 * VP * (WF ? 16 : 12);
    L.ci = L.sb + (htmp > tab ? htmp : tab);
    L.wp = L.ci + kMmaWaves * 32 * (int)sizeof(CandInfo);
    L.cand = L.wp;
    L.zero = L.cand + (DB ? 0 : kMmaChunk * 8);
    L.total = L.zero + 32;
    return L;
}

// static LDS of k_score_mma: region and candidate buffers (DB) + small slots
template <int WID, int NBLK, bool DB>
__host__ __device__ constexpr int mma_static_lds() {
    return (DB ? 2 * (16 * NBLK * MmaGeom<WID>::VS + 16 + kMmaChunk * 8) : 64) + 8 + 4 + 65 * 8 + 64 +
           kSortBins * kMmaWaves * 3;   // the row sort's counts and offsets
}

// what fits in 160 KiB beside the rest at this NBLK (1 workgroup of 16 waves
// per CU): double buffering first, then the binary32 w copy
template <int WID, int NBLK>
__host__ __device__ constexpr bool mma_db() {
    return mma_lds<WID, NBLK, false, true>(16 * NBLK).total + mma_static_lds<WID, NBLK, true>() <= 160 * 1024;
}
template <int WID, int NBLK>
__host__ __device__ constexpr bool mma_wf() {
    return mma_lds<WID, NBLK, true, mma_db<WID, NBLK>()>(16 * NBLK).total +
               mma_static_lds<WID, NBLK, mma_db<WID, NBLK>()>() <= 160 * 1024;
}
template <int WID, int NBLK>
__host__ __device__ constexpr MmaLds mma_layout(int V) {
    return mma_lds<WID, NBLK, mma_wf<WID, NBLK>(), mma_db<WID, NBLK>()>(V);
}

template <int WID, int NBLK, bool FAST>
__global__ __launch_bounds__(kMmaThreads) void k_score_mma(const SceneDev sc, const ScoreArgs a, const TiledArgs t,
                                                           const int4* __restrict__ items,
                                                           const int2* __restrict__ sorted) {
    using G = MmaGeom<WID>;
    constexpr int NB = G::NB, NPX = G::NPX, ROWS = G::ROWS, KS = G::KS, VS = G::VS, C0 = G::C0;
    constexpr int VP = 16 * NBLK;                         // views per table row
    constexpr bool WF = mma_wf<WID, NBLK>(), DB = mma_db<WID, NBLK>();
    constexpr int RPV = VS / 32;                          // region rows per view incl. the pad row
    constexpr int PF = (VP * RPV * 2 + kMmaThreads - 1) / kMmaThreads;   // 16-B pieces per thread
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // DB: the two region and candidate buffers are distinct LDS objects, so
    // that the compiler sees that reads of one do not alias the LDS-DMA into
    // the other (no vmcnt wait for the prefetch before them)
    // (DB) each region buffer ends in 16 zero bytes, never an LDS-DMA target:
    // phase 3 reads a window row or the zeros by an offset select inside the
    // one buffer, so that the read keeps the buffer's alias scope and does not
    // wait for the other buffer's LDS-DMA (a select between two LDS objects
    // would wait for every LDS-DMA in flight)
    constexpr int RB = DB ? VP * VS : 16, CB = DB ? kMmaChunk * 8 : 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_reg0[RB + 16], s_reg1[RB + 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_cand0[CB], s_cand1[CB];
    __shared__ int s_ids[2];
    __shared__ int s_simd_n[4];
    __shared__ int s_V;
    __shared__ double s_recip[65];
    // the item's candidates are reordered by pixel row inside the tile (a
    // counting sort in LDS): per (wave, row) counts and destination offsets
#ifdef MVS_STAMPS
    __shared__ unsigned s_maxown;
    if (threadIdx.x == 0) s_maxown = 0;
#endif
    __shared__ __attribute__((aligned(16))) uint8_t s_rcnt[kSortBins][kMmaWaves];
    __shared__ __attribute__((aligned(16))) int16_t s_roff[kSortBins][kMmaWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int V = sc.V;
    const int npiece = V * RPV * 2;
    // k / V as umulhi(k, ceil(2^32 / V)): exact for k V < 2^32 (uniform, once)
    const uint32_t vmagic = __builtin_amdgcn_readfirstlane(0xffffffffu / (uint32_t)V + 1u);
    if (tid <= 64) s_recip[tid] = c_recip.r[tid];
    if (tid == 0) s_V = V;
    const MmaLds L = mma_layout<WID, NBLK>(V);
    uint32_t* htmp = (uint32_t*)(smem + L.sb);
    int32_t* tsb = (int32_t*)(smem + L.sb);
    double* tw = (double*)(smem + L.w);
    float* twf = (float*)(smem + L.wf);
    CandInfo* ci = (CandInfo*)(smem + L.ci) + wave * 32;
    if (tid < 8) ((uint32_t*)(smem + L.zero))[tid] = 0u;
    if (DB && tid >= 8 && tid < 16) ((uint32_t*)((tid < 12 ? s_reg0 : s_reg1) + RB))[tid & 3] = 0u;
    const int zoff = DB ? RB : L.zero - L.reg;   // the zero row, relative to a region buffer

    const double kn = (double)NPX / (double)(NPX - 1);
    const float tqf = (float)(a.thr / kn);
    ItemMap im;
    im.load(t);
    const int n_units = im.total();
    int32_t* head = t.head;

    // The region of an item (gv rows, signed bytes) goes to LDS by LDS-DMA
    // (global_load_lds_dwordx4: 64 lanes x 16 B land contiguously), 32 B per
    // region row and RPV rows per view including one pad row, so that the
    // image is linear in the piece index; rows outside the image are clamped
    // (their pixels are never inside a valid window).
    auto region_buf = [&](int buf) -> uint8_t* { return DB ? (buf ? s_reg1 : s_reg0) : smem + L.reg; };
    auto cand_buf = [&](int buf) -> uint8_t* { return DB ? (buf ? s_cand1 : s_cand0) : smem + L.cand; };
    auto stage = [&](const int4 d, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        const int ty = d.x / t.ntx, tx = d.x - ty * t.ntx;
        const int x0 = tx * MVS_TILE_W, yr0 = ty * MVS_TILE_H - WID;
        uint8_t* base = region_buf(buf);
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int k = tid + p * kMmaThreads;
            if (k < npiece) {
                const int v = k / (2 * RPV), r2 = k - v * (2 * RPV);
                const int y = min(max(yr0 + (r2 >> 1), 0), sc.H - 1);
                const uint8_t* src = sc.gv + ((int64_t)v * sc.H + y) * sc.Wp + (x0 - 8) + 16 * (r2 & 1);
                __builtin_amdgcn_global_load_lds((const void*)src,
                                                 (void __attribute__((address_space(3)))*)(base + (p * kMmaThreads + wave * 64) * 16),
                                                 16, 0, 0);
            }
        }
        // the item's sorted (id, pk) entries, one dword per lane
        uint8_t* cbase = cand_buf(buf);
        const int32_t* csrc = (const int32_t*)(sorted + d.y);
#pragma unroll
        for (int p = 0; p < 2 * kMmaChunk / kMmaThreads; ++p) {
            const int k = tid + p * kMmaThreads;
            if (k < 2 * d.z)
                __builtin_amdgcn_global_load_lds((const void*)(csrc + k),
                                                 (void __attribute__((address_space(3)))*)(cbase + (p * kMmaThreads + wave * 64) * 4),
                                                 4, 0, 0);
        }
    };

    // Work items flow through a pipeline: while item k is scored, item k+1's
    // region (DB) and candidate list, item k+2's descriptor and thread 0's
    // claim of item k+3 are in flight; the barrier that ends item k retires them.
    if (tid == 0) {
        s_ids[0] = atomicAdd(head, 1);
        s_ids[1] = atomicAdd(head, 1);
    }
    // The 16 waves sit 4 to a SIMD, which shares its issue among them: work is
    // split by SIMD (virtual wave vw = 4 SIMD + rank on it) where it does not
    // divide evenly over the waves.  vw = wave unless every SIMD holds 4 waves.
    if (tid < 4) s_simd_n[tid] = 0;
    __syncthreads();
    const int simd = __builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4);   // HW_ID.SIMD_ID
    int srank = 0;
    if (lane == 0) srank = atomicAdd(&s_simd_n[simd & 3], 1);
    srank = __builtin_amdgcn_readfirstlane(srank);
    __syncthreads();
    const bool simd_ok = s_simd_n[0] == 4 && s_simd_n[1] == 4 && s_simd_n[2] == 4 && s_simd_n[3] == 4;
    const int vw = __builtin_amdgcn_readfirstlane(simd_ok ? 4 * (simd & 3) + srank : wave);
    int cur = __builtin_amdgcn_readfirstlane(s_ids[0]);
    int nx1 = __builtin_amdgcn_readfirstlane(s_ids[1]);
    if (cur >= n_units) return;
    int4 dcur = item_desc(t, items, im, cur);
    dcur = make_int4(__builtin_amdgcn_readfirstlane(dcur.x), __builtin_amdgcn_readfirstlane(dcur.y),
                     __builtin_amdgcn_readfirstlane(dcur.z), 0);
    stage(dcur, std::integral_constant<int, 0>{});
    // item nx1's descriptor (uniform, scalar loads) and thread 0's claim of
    // the item after it
    int4 dnx1 = nx1 < n_units ? item_desc(t, items, im, nx1) : make_int4(0, 0, 0, 0);
    int pend = 0;
    if (tid == 0) pend = atomicAdd(head, 1);
    __syncthreads();   // everyone has read s_ids before they are rewritten

    // one round per work item; the rounds alternate the buffers (DB), with the
    // buffer index a compile-time constant in each
    auto round = [&](auto bufc) -> bool {
        constexpr int buf = decltype(bufc)::value;
        STAMP(t0);
        const int nc = dcur.z;
            const uint8_t* reg = region_buf(buf);
            const int2* cand = (const int2*)cand_buf(buf);
            // ---- 1. this item's region and candidates are staged ----
            if (tid == 0) s_ids[0] = pend;
            __syncthreads();
            const int nx2 = __builtin_amdgcn_readfirstlane(s_ids[0]);
            STAMP(t1);
            // thread -> (row, view) maps of phase 2, from a V read after the
            // barrier (not hoisted: no registers held across phase 3)
            const int Vl = s_V;
            // tasks split into four contiguous SIMD segments (vw = 4 SIMD + rank):
            // each SIMD issues a quarter of them whatever the task count
            const int ploc = (vw & 3) * 64 + lane, pseg = vw >> 2;
            const int hq = (Vl * ROWS + 3) >> 2, vq = (Vl * 16 + 3) >> 2;   // per-SIMD quotas
            const int vtask = pseg * vq + ploc;
            const int h_rho0 = (int)__umulhi((uint32_t)vtask, vmagic), h_v0 = vtask - h_rho0 * Vl;   // vertical: (column, view)
            const bool m2 = ploc < vq && vtask < Vl * 16;
            // sort of the candidates by pixel row pair (rrel >> 1: a K-step's two
            // region rows), stable: thread k holds candidate k; its rank among
            // the wave's candidates of its row pair now, the destination after
            // the offsets are known (phase 2 barriers)
            int2 my_c = make_int2(0, 0);
            int my_row = kSortBins, my_rank = 0;
            if (tid < nc) {
                my_c = ((const int2*)cand_buf(buf))[tid];
                my_row = (my_c.y >> 5) & 3;
            }
            int my_cnt = 0;   // lane y < kSortBins: the wave's count of bin y
            static_for<kSortBins>([&](auto Yc) {
                constexpr int y = Yc;
                const uint64_t bm = __ballot(my_row == y);
                if (my_row == y) my_rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
                my_cnt = writelane<y>((uint32_t)my_cnt, (uint32_t)__popcll(bm));
            });
            if (lane < kSortBins) s_rcnt[lane][wave] = (uint8_t)my_cnt;
            // ---- 2. S_b and w of every view at the tile's pixels ----
            // horizontal sums of each region row on the unsigned bytes g = s + 128
            // (the moments are shift invariant): prefix sums by v_sad_u8 and
            // v_dot4_u32_u8, packed as (sum g^2) << 12 | sum g
            for (int j = 0; ploc + 256 * j < hq; ++j) {
                const int k = pseg * hq + ploc + 256 * j;
                if (k < V * ROWS) {
                    const int rho = (int)__umulhi((uint32_t)k, vmagic), v = k - rho * Vl;
                    const uint4 lo = *(const uint4*)(reg + v * VS + rho * 32);
                    const uint4 hi = *(const uint4*)(reg + v * VS + rho * 32 + 16);
                    const uint32_t d[8] = {lo.x ^ 0x80808080u, lo.y ^ 0x80808080u, lo.z ^ 0x80808080u,
                                           lo.w ^ 0x80808080u, hi.x ^ 0x80808080u, hi.y ^ 0x80808080u,
                                           hi.z ^ 0x80808080u, hi.w ^ 0x80808080u};
                    uint32_t PS[33], PQ[33];
                    PS[0] = 0;
                    PQ[0] = 0;
    #pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const uint32_t m1 = d[k] & 0xffu, m2b = d[k] & 0xffffu, m3 = d[k] & 0xffffffu;
                        PS[4 * k + 1] = __builtin_amdgcn_sad_u8(m1, 0u, PS[4 * k]);
                        PS[4 * k + 2] = __builtin_amdgcn_sad_u8(m2b, 0u, PS[4 * k]);
                        PS[4 * k + 3] = __builtin_amdgcn_sad_u8(m3, 0u, PS[4 * k]);
                        PS[4 * k + 4] = __builtin_amdgcn_sad_u8(d[k], 0u, PS[4 * k]);
                        PQ[4 * k + 1] = __builtin_amdgcn_udot4(m1, d[k], PQ[4 * k], false);
                        PQ[4 * k + 2] = __builtin_amdgcn_udot4(m2b, d[k], PQ[4 * k], false);
                        PQ[4 * k + 3] = __builtin_amdgcn_udot4(m3, d[k], PQ[4 * k], false);
                        PQ[4 * k + 4] = __builtin_amdgcn_udot4(d[k], d[k], PQ[4 * k], false);
                    }
                    uint32_t* hrow = htmp + rho * 16 * VP + v;
    #pragma unroll
                    for (int x = 0; x < 16; ++x)
                        hrow[x * VP] = ((PQ[x + C0 + NB] - PQ[x + C0]) << 12) | (PS[x + C0 + NB] - PS[x + C0]);
                }
            }
            __syncthreads();
            STAMP(t1a);
            // destination offsets of the row sort: row y's candidates start after
            // every candidate of rows < y, then by wave (lane y of the last wave:
            // the row's 16 wave counts in one read, prefix sums in registers)
            if (wave == kMmaWaves - 1 && lane < kSortBins) {
                const uint4 q4 = *(const uint4*)&s_rcnt[lane][0];
                const uint32_t qw[4] = {q4.x, q4.y, q4.z, q4.w};
                int pre[kMmaWaves];
                int tot = 0;
    #pragma unroll
                for (int w = 0; w < kMmaWaves; ++w) {
                    pre[w] = tot;
                    tot += (qw[w >> 2] >> (8 * (w & 3))) & 0xff;
                }
                int ex = tot;
    #pragma unroll
                for (int off = 1; off < kSortBins; off <<= 1) {
                    const int yv = __shfl_up(ex, off, 64);
                    if (lane >= off) ex += yv;
                }
                const int base = ex - tot;
                uint32_t pk[kMmaWaves / 2];
    #pragma unroll
                for (int w = 0; w < kMmaWaves / 2; ++w)
                    pk[w] = (uint32_t)(base + pre[2 * w]) | ((uint32_t)(base + pre[2 * w + 1]) << 16);
                *(uint4*)&s_roff[lane][0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                *(uint4*)&s_roff[lane][8] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            }
            // vertical sums -> (S_b of s, w) per (pixel, view); the table overwrites
            // the horizontal sums, so every thread reads first
            int ms[MVS_TILE_H];
            double mw[MVS_TILE_H];
            const int m2x = h_rho0, m2v = h_v0;   // thread -> (pixel column, view)
            if (m2) {
                int S[ROWS], Q[ROWS];
    #pragma unroll
                for (int rho = 0; rho < ROWS; ++rho) {
                    const uint32_t h = htmp[(rho * 16 + m2x) * VP + m2v];
                    S[rho] = (int)(h & 0xfffu);
                    Q[rho] = (int)(h >> 12);
                }
                int sg = 0, q = 0;
    #pragma unroll
                for (int rho = 0; rho < NB; ++rho) {
                    sg += S[rho];
                    q += Q[rho];
                }
    #pragma unroll
                for (int y = 0; y < MVS_TILE_H; ++y) {
                    if (y > 0) {
                        sg += S[y + NB - 1] - S[y - 1];
                        q += Q[y + NB - 1] - Q[y - 1];
                    }
                    const int db = NPX * q - sg * sg;   // < 2^31: n * sum g^2 <= 121 * 121 * 255^2
                    // v_rsq_f64 + one Newton step: max relative error 4.1e-15 over
                    // 4M values of D < 2^31 (tools/ubench/rsq_acc.hip; 5.2e-8 without).
                    // A constant window (D = 0) gets rsq = inf and then nan from the
                    // Newton step: ctNcc's nan, which never passes (no select)
                    const double D = (double)db;
                    double w = __builtin_amdgcn_rsq(D);
                    w = w * (1.5 - 0.5 * D * w * w);
                    ms[y] = sg - 128 * NPX;             // S_b of s = g - 128
                    mw[y] = w;
                }
            }
            __syncthreads();
            STAMP(t1b);
            if (tid < nc) ((int2*)cand_buf(buf))[s_roff[my_row][wave] + my_rank] = my_c;
            if (m2)
    #pragma unroll
                for (int y = 0; y < MVS_TILE_H; ++y) {
                    const int o = (y * 16 + m2x) * VP + m2v;
                    tsb[o] = ms[y];
                    tw[o] = mw[y];
                    if constexpr (WF) twf[o] = (float)mw[y];
                }
            if (VP > V)   // views V..VP-1 of the last 16-view block: never pass
                for (int k = tid; k < 128 * (VP - V); k += kMmaThreads) {
                    const int px = k / (VP - V), v = V + (k - px * (VP - V));
                    tsb[px * VP + v] = 0;
                    tw[px * VP + v] = __builtin_nan("");
                    if constexpr (WF) twf[px * VP + v] = __builtin_nanf("");
                }
            __syncthreads();
            STAMP(t2);
            // the next items' loads, in flight during phase 3 (phase 2's register
            // spills would otherwise wait for them: vmcnt retires in order): item
            // nx1's region and candidates (DB), item nx2's descriptor (scalar
            // loads) and thread 0's claim of the item after it
            if (nx1 < n_units) {
                if constexpr (DB) stage(dnx1, std::integral_constant<int, buf ^ 1>{});
            }
            int4 dnx2 = make_int4(0, 0, 0, 0);
            if (nx2 < n_units) {
                dnx2 = item_desc(t, items, im, nx2);
                if (tid == 0) pend = atomicAdd(head, 1);
            }
    
            // ---- 3. + 4. the candidates: units of two M-blocks of 16 (32
            // consecutive candidates of the row-sorted list), which share their
            // K-steps and B operands and give the epilogue two independent
            // chains.  The SIMDs share the issue of their waves, so the blocks
            // are split into four contiguous SIMD segments of equal size; a
            // segment's waves take its units (the last one may be a single
            // block) ----
            const int nblk = (nc + 15) >> 4;
            const int sg = vw >> 2, sr = vw & 3;           // SIMD segment, wave rank in it
            const int seg_b = (nblk * sg) >> 2, seg_e = (nblk * (sg + 1)) >> 2;
    #ifdef MVS_STAMPS
            unsigned long long w0blk = 0;
    #endif
            for (int fb = seg_b + 2 * sr; fb < seg_e; fb += 8) {
              const int nh = min(2, seg_e - fb);
    #ifdef MVS_STAMPS
              w0blk += nh;
    #endif
              auto unit = [&](auto nhc) {
                constexpr int NH = decltype(nhc)::value;
                // lane constants recomputed per unit (hoisted, they would hold
                // registers through phase 2)
                const int ol = opaque(lane);
                const int m = ol & 15, kh = ol >> 4;
                int2 e[NH];
                bool valid[NH];
                int qrel[NH], rrel[NH], Rv[NH];
    #pragma unroll
                for (int h = 0; h < NH; ++h) {
                    const int kk = (fb + h) * 16 + m;
                    valid[h] = kk < nc;
                    e[h] = valid[h] ? cand[kk] : make_int2(-1, 0);
                    qrel[h] = e[h].y & 15;
                    rrel[h] = (e[h].y >> 4) & 7;
                    Rv[h] = e[h].y >> 7;
                }
                // the candidates' constants (row 0 of the wave computes them for
                // both blocks, before the K-loop: they do not depend on it), shared
                // through LDS
                double my_wa[NH];
    #pragma unroll
                for (int h = 0; h < NH; ++h) my_wa[h] = 0.0;
                if (kh == 0) {
    #pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        CandInfo c;
                        const int px = e[h].y & 127;          // rrel * 16 + qrel
                        const int o = px * VP + Rv[h];
                        const double wa = tw[o];
                        c.osb = L.sb + px * VP * 4;
                        c.Sa = -tsb[o];                       // -S_a: num = n C + (-S_a) S_b
                        c.R = valid[h] ? Rv[h] : -1;
                        // FAST: T = thr (n-1)/n sqrt(da) in binary32 (1-ulp reciprocal,
                        // well inside the guard band); else the decision is on ncc
                        c.T = FAST ? (valid[h] ? tqf * __builtin_amdgcn_rcpf((float)wa) : __builtin_nanf("")) : 0.0f;
                        ci[16 * h + m] = c;
                        my_wa[h] = wa;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                // the unit's candidates are sorted by row pair: its window rows lie
                // in candidate 0's pair to the last valid candidate's pair + NB - 1
                const int last = min(16 * NH - 1, nc - 1 - fb * 16);
                const int r_lo = __builtin_amdgcn_readlane(rrel[0], 0) & ~1;
                const int r_hi = (last >= 16 ? __builtin_amdgcn_readlane(rrel[NH - 1], last - 16)
                                             : __builtin_amdgcn_readlane(rrel[0], last)) | 1;
                constexpr int KSK = WID + 1;     // K-steps of one row's windows
                const int s_lo = r_lo >> 1, s_hi = (r_hi + NB - 1) >> 1;
                const int span = s_hi - s_lo + 1;
                // A: the reference windows, masked to each candidate's window
                // columns (this lane's 16 columns) and rows (bit 2s: K-step s holds
                // a window row of this lane's row parity)
                uint32_t cm[NH][4], rb[NH];
    #pragma unroll
                for (int h = 0; h < NH; ++h) {
                    const uint32_t wm = valid[h] ? (((1u << NB) - 1u) << (qrel[h] + C0)) : 0u;
                    const uint32_t hm = wm >> (16 * (kh & 1));
    #pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4) cm[h][k4] = byte_mask((hm >> (4 * k4)) & 15u);
                    rb[h] = valid[h] ? (((1u << NB) - 1u) << rrel[h]) >> (kh >> 1) : 0u;
                }
                const int lofs = 32 * (kh >> 1) + 16 * (kh & 1);
                v4i C[NH][NBLK];
    #pragma unroll
                for (int h = 0; h < NH; ++h)
    #pragma unroll
                    for (int nb = 0; nb < NBLK; ++nb) C[h][nb] = (v4i){0, 0, 0, 0};
                // NST K-steps from sb; steps below sd are done (their A rows read zeros)
                // steps [SAFE_LO, SAFE_HI] of the pass hold window rows of every
                // candidate of the unit (no row test there)
                auto kpass = [&](auto nstc, auto safe_lo_c, auto safe_hi_c, int sb, int sd) {
                    constexpr int NST = decltype(nstc)::value;
                    constexpr int SAFE_LO = decltype(safe_lo_c)::value, SAFE_HI = decltype(safe_hi_c)::value;
                    uint32_t rbp[NH];
                    int aoff[NH];
    #pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        rbp[h] = (rb[h] & ~((1u << (2 * sd)) - 1u)) >> (2 * sb);
                        aoff[h] = Rv[h] * VS + lofs + 64 * sb;
                    }
                    const uint8_t* bptr[NBLK];
    #pragma unroll
                    for (int nb = 0; nb < NBLK; ++nb) bptr[nb] = reg + min(16 * nb + m, V - 1) * VS + lofs + 64 * sb;
                    // operands of step st + 1 load while step st's MFMAs run; the
                    // schedule barrier keeps the compiler from hoisting more loads
                    // (their registers would spill)
                    uint4 av[2][NH], bv[2][NBLK];
                    auto load = [&](int st, int slot) {
    #pragma unroll
                        for (int h = 0; h < NH; ++h)
                            // rows outside the window read 16 zero bytes: an offset
                            // select instead of a branch around the load
                            av[slot][h] = *(const uint4*)(reg + ((st >= SAFE_LO && st <= SAFE_HI) ||
                                                                         ((rbp[h] >> (2 * st)) & 1u)
                                                                     ? aoff[h] + 64 * st : zoff));
    #pragma unroll
                        for (int nb = 0; nb < NBLK; ++nb) bv[slot][nb] = *(const uint4*)(bptr[nb] + 64 * st);
                    };
                    load(0, 0);
    #pragma unroll
                    for (int st = 0; st < NST; ++st) {
                        const int cur = st & 1;
                        if (st + 1 < NST) load(st + 1, cur ^ 1);
                        v4i A[NH];
    #pragma unroll
                        for (int h = 0; h < NH; ++h)
                            A[h] = (v4i){(int)(av[cur][h].x & cm[h][0]), (int)(av[cur][h].y & cm[h][1]),
                                         (int)(av[cur][h].z & cm[h][2]), (int)(av[cur][h].w & cm[h][3])};
    #pragma unroll
                        for (int nb = 0; nb < NBLK; ++nb) {
                            const v4i B = {(int)bv[cur][nb].x, (int)bv[cur][nb].y, (int)bv[cur][nb].z, (int)bv[cur][nb].w};
    #pragma unroll
                            for (int h = 0; h < NH; ++h)
                                C[h][nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[h], B, C[h][nb], 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                // one row pair (span KSK, from s_lo <= KS - KSK): steps 1 .. KSK-2
                // hold rows of every window; two (span KSK+1): steps 2 .. KSK-2
                using I = std::integral_constant<int, 0>;
                if (span <= KSK) {
                    kpass(std::integral_constant<int, KSK>{}, std::integral_constant<int, 1>{},
                          std::integral_constant<int, KSK - 2>{}, min(s_lo, KS - KSK), 0);
                } else if (span == KSK + 1) {
                    kpass(std::integral_constant<int, KSK + 1>{}, std::integral_constant<int, 2>{},
                          std::integral_constant<int, KSK - 2>{}, min(s_lo, KS - KSK - 1), 0);
                } else {
                    for (int sd = s_lo; sd <= s_hi; sd += KSK)
                        kpass(std::integral_constant<int, KSK>{}, std::integral_constant<int, KSK>{}, I{},
                              min(sd, KS - KSK), sd);
                }
                // lane (kh, m) holds C[h][nb][i] = block h's candidate 4 kh + i, view 16 nb + m
                uint32_t pmv[NH], gdv[NH];
    #pragma unroll
                for (int h = 0; h < NH; ++h) pmv[h] = gdv[h] = 0u;
                double sacc[NH][4];
                static_for<4>([&](auto Ic) {
                    constexpr int i = Ic;
    #pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        const CandInfo c = ci[16 * h + 4 * kh + i];
                        const int32_t* sbp = (const int32_t*)(smem + c.osb) + m;
                        const double* twp = (const double*)(smem + L.w + 2 * (c.osb - L.sb)) + m;
                        const float* twfp = (const float*)(smem + c.osb + (L.wf - L.sb)) + m;   // WF only
                        const float gT = 2e-6f * fabsf(c.T);
                        // slow path: n/(n-1) w_a from the pixel's w row
                        double ca = 0.0;
                        if constexpr (!FAST) ca = kn * twp[(c.R < 0 ? 0 : c.R) - m];
                        double sa = 0.0;
                        uint64_t g = 0;
                        float ax[NBLK];   // FAST: the decision values, for the guard test
                        static_for<NBLK>([&](auto Nc) {
                            constexpr int nb = Nc;
                            const int vl = 16 * nb + m;
                            const int num = __mul24(c.Sa, sbp[16 * nb]) + __mul24(NPX, C[h][nb][i]);
                            const double w = twp[16 * nb];
                            uint64_t P;
                            if constexpr (FAST) {
                                // ncc > thr <=> num w_b > T; a constant window (w_b = 0 here)
                                // never passes.  The candidate's own view R passes (its ncc
                                // is n/(n-1) > thr): its mask bit and its term of the sum
                                // are taken out once per candidate, not tested per pair
                                const float x = fmaf((float)num, WF ? twfp[16 * nb] : (float)w, -c.T);
                                P = __builtin_amdgcn_fcmpf(x, 0.0f, 2);                         // ogt
                                ax[nb] = x;
                                // the sum's term in the passing lanes only
                                sa = fma_f64_lanes(sa, num, w, P);
                            } else {
                                const double ncc = (double)num * w * ca;
                                const bool pass = vl != c.R && ncc > a.thr;
                                P = __ballot(pass);
                                g |= __ballot(vl != c.R && fabs(ncc - a.thr) <= kGuard);
                                sa = fma((double)num, pass ? w : 0.0, sa);
                            }
                            pmv[h] = writelane<2 * (i * NBLK + nb)>(pmv[h], (uint32_t)P);
                            pmv[h] = writelane<2 * (i * NBLK + nb) + 1>(pmv[h], (uint32_t)(P >> 32));
                        });
                        if constexpr (FAST) {
                            // guard band: min over the views of |x| < gT (one compare)
                            float mn = fabsf(ax[0]);
    #pragma unroll
                            for (int nb = 1; nb < NBLK; ++nb) mn = fminf(mn, fabsf(ax[nb]));
                            g = __builtin_amdgcn_fcmpf(mn, gT, 4);                               // olt
                        }
                        gdv[h] = writelane<2 * i>(gdv[h], (uint32_t)g);
                        gdv[h] = writelane<2 * i + 1>(gdv[h], (uint32_t)(g >> 32));
                        sacc[h][i] = sa;
                    }
                });
                // owner lane c = 4 j + i (row 0) of each block's candidate c: its mask
                // bits, guard bits and sum from the lanes that hold them (crossbar
                // permutes, no LDS storage)
                const int jj = m >> 2, ii = m & 3;
    #pragma unroll
                for (int h = 0; h < NH; ++h) {
                    uint64_t mk = 0;
    #pragma unroll
                    for (int nb = 0; nb < NBLK; ++nb) {
                        const uint32_t d = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (2 * (ii * NBLK + nb) + (jj >> 1)), (int)pmv[h]);
                        mk |= (uint64_t)((d >> (16 * (jj & 1))) & 0xffffu) << (16 * nb);
                    }
                    const uint32_t gw = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * (2 * ii + (jj >> 1)), (int)gdv[h]);
                    const bool gg = ((gw >> (16 * (jj & 1))) & 0xffffu) != 0u;
                    double mine = 0.0;
                    if (a.avg != nullptr) {
                        const double rs = row_sum16_x4(sacc[h], m);
                        const int src = 4 * (16 * jj + ii);   // lane 16 j + i holds candidate 4 j + i's sum
                        const unsigned long long rb64 = __double_as_longlong(rs);
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)rb64);
                        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(rb64 >> 32));
                        mine = __longlong_as_double(((unsigned long long)hi << 32) | lo);
                    }
                    if (kh == 0 && valid[h]) {
                        // the reference view itself is no V entry (MVS2.py:66-67)
                        const uint64_t self = (mk >> Rv[h]) & 1ull;
                        mk &= ~(1ull << Rv[h]);
                        const int cnt = __popcll(mk);
                        const int64_t idx = e[h].x;
                        a.mask[idx * a.mstride] = mk;
                        if (a.count) a.count[idx] = cnt;
                        if (a.avg) {
                            // its own term num_RR w_a = D_a w_a = sqrt(D_a) = 1 / w_a (to
                            // the rsq + Newton accuracy of w_a, 4e-15) leaves the sum
                            double inv = __builtin_amdgcn_rcp(my_wa[h]);
                            inv = inv * (2.0 - my_wa[h] * inv);
                            const double sum = self ? mine - inv : mine;
                            a.avg[idx * a.astride] = cnt ? sum * (kn * my_wa[h]) * s_recip[cnt] : 0.0;
                        }
                        if (gg) {
                            t.fix_list[atomicAdd(t.fix_count, 1)] = make_int4((int32_t)idx, dcur.x, e[h].y, 0);
                            STAMP_ADD_ANY(11, 1);
                        }
                    }
                }
    #ifdef MVS_STAMPS
                STAMP_ADD_LANE0(12, span > KSK ? 1 : 0);
                STAMP_ADD_LANE0(13, 1);
    #endif
              };
              if (nh == 2) unit(std::integral_constant<int, 2>{});
              else unit(std::integral_constant<int, 1>{});
            }
            STAMP(t3);
    #ifdef MVS_STAMPS
            // slowest wave's own phase-3 time (per item: slot 9), every wave's (10)
            if (lane == 0) atomicMax(&s_maxown, (unsigned)(t3 - t2));
            STAMP_ADD_LANE0(10, t3 - t2);
    #endif
            __syncthreads();
            STAMP(t4);
            STAMP_ADD(0, 1);
            STAMP_ADD(1, t1 - t0);
            STAMP_ADD(2, t2 - t1);
            STAMP_ADD(3, t4 - t2);
            STAMP_ADD_W0(4, t3 - t2);
            STAMP_ADD_W0(5, w0blk);
            STAMP_ADD(6, t1a - t1);
            STAMP_ADD(7, t1b - t1a);
            STAMP_ADD_W0(8, t4 - t3);
    #ifdef MVS_STAMPS
            if (tid == 0) {
                STAMP_ADD_ANY(9, s_maxown);
                s_maxown = 0;
            }
    #endif
        if (nx1 >= n_units) return false;
        if constexpr (!DB) stage(dnx1, std::integral_constant<int, 0>{});   // the buffer is free now; lands by the next barrier
        cur = nx1;
        dcur = dnx1;
        nx1 = nx2;
        dnx1 = dnx2;
        return true;
    };
    for (;;) {
        if (!round(std::integral_constant<int, 0>{})) break;
        if (!round(std::integral_constant<int, DB ? 1 : 0>{})) break;
    }
}

template <int WID, int NBLK>
int launch_mma(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t, hipStream_t s) {
    // the largest table is sized for V = 16 NBLK; every V of this NBLK fits in it
    const int lds = mma_layout<WID, NBLK>(16 * NBLK).total, used = mma_layout<WID, NBLK>(sc->V).total;
#define MVS_MMA_LAUNCH(FAST_)                                                                                   \
    do {                                                                                                        \
        static std::atomic<uint64_t> done{0};                                                                   \
        if (set_dyn_lds_once((const void*)k_score_mma<WID, NBLK, FAST_>, done, lds) != 0) return -1;            \
        hipLaunchKernelGGL((k_score_mma<WID, NBLK, FAST_>), dim3(kMmaGrid), dim3(kMmaThreads), used, s, *sc, *a, \
                           *t, (const int4*)t->items, (const int2*)t->sorted);                                  \
    } while (0)
    if (fabs(a->thr) >= 0.01) MVS_MMA_LAUNCH(true);
    else MVS_MMA_LAUNCH(false);
#undef MVS_MMA_LAUNCH
    return 0;
}

}  // namespace

MVS_STAMPS_READER(mvs_read_stamps_mma)

extern "C" int mvs_launch_score_mma(const SceneDev* sc, const ScoreArgs* a, const TiledArgs* t, int wid,
                                    hipStream_t s) {
    return dispatch_wid(wid, -2, [&](auto w) {
        constexpr int WID = decltype(w)::value;
        switch ((sc->V + 15) / 16) {
            case 1: return launch_mma<WID, 1>(sc, a, t, s);
            case 2: return launch_mma<WID, 2>(sc, a, t, s);
            case 3: return launch_mma<WID, 3>(sc, a, t, s);
            default: return launch_mma<WID, 4>(sc, a, t, s);
        }
    });
}

extern "C" size_t mvs_mma_lds_bytes(int V, int wid) {
    if (V > kGroupViews) return mvs_mma_v_lds_bytes(wid);
    return dispatch_wid(wid, (size_t)0, [&](auto w) {
        constexpr int WID = decltype(w)::value;
        switch ((V + 15) / 16) {
            case 1: return (size_t)mma_layout<WID, 1>(V).total;
            case 2: return (size_t)mma_layout<WID, 2>(V).total;
            case 3: return (size_t)mma_layout<WID, 3>(V).total;
            default: return (size_t)mma_layout<WID, 4>(V).total;
        }
    });
}
