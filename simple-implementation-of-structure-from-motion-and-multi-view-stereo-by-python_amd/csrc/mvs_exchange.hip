// The multi-GPU sweep's exchange: the pack of a slice's accepted candidates
// (k_acc_pack) and the measurement-only stand-in for a collective (k_proxy_copy).
#include <algorithm>

#include "mvs_device.h"

namespace {

// ---------------------------------------------------------------------------
// The multi-GPU sweep's exchange record set (parallel.PointsExchange): the
// accepted candidates of a rank's slice (|V| >= vlb, MVS2.py:256/369) as rows
// [global index, mask words..., (c) x, y, z as binary64 bits] of a
// fixed-capacity buffer whose row 0 is the header [accepted, n, 0...].  No
// host synchronisation: the accepted total travels in the header, and a slice
// with more than cap accepted candidates keeps cap of them (the receiver sees
// accepted > cap).
// One workgroup per chunk of kAccChunk = 8,192 candidates (thread t holds
// candidates chunk + t + 1024 j, j < kAccPer: coalesced loads).  A chunk's
// rows are its accepted candidates in index order; the chunks reserve their
// row ranges by one returning atomic each on the pack's counter, in whatever
// order they get there -- no chunk waits for another (round 5's decoupled
// look-back kept the rows in index order across chunks and cost ~18 us per
// 2^20 sweep); the receiver orders rows by their index column if it needs
// to (PointsExchange.result).  The workgroup that takes the last ticket
// writes the header and returns the counter and the ticket to zero for the
// next call.
// ---------------------------------------------------------------------------
constexpr int kAccThreads = 1024, kAccPer = MVS_ACC_PER, kAccChunk = kAccThreads * kAccPer, kAccWaves = kAccThreads / 64;
constexpr int kAccE = kAccPer * kAccWaves;          // (j, wave) counts of a chunk
constexpr int kAccEpl = (kAccE + 63) / 64;          // of them per lane of wave 0's scan
// 16-B accesses at 8-B alignment (global_load/store_dwordx4 allow it)
typedef double acc_d2v __attribute__((ext_vector_type(2)));
typedef acc_d2v acc_d2 __attribute__((aligned(8)));
typedef long long acc_l2v __attribute__((ext_vector_type(2)));
typedef acc_l2v acc_l2 __attribute__((aligned(8)));
static_assert(kAccChunk == MVS_ACC_CHUNK, "the host sizes the pack's grid by MVS_ACC_CHUNK");
static_assert(kAccE <= 128, "wave 0 scans at most two (j, wave) counts per lane");

// a chunk's ticket, taken after its reservation (base) has returned; the last
// one writes the header and returns the counter and the ticket to zero
DEV void acc_ticket(unsigned long long* __restrict__ ctl, unsigned long long base, int64_t nch, int64_t n, int width,
                    int64_t* __restrict__ out) {
    // the ticket's address depends on the reservation's result (always 0 +
    // 16; opaque to the compiler), so it issues after the return
    const int dep = opaque((int)(base >> 63));
    const unsigned long long tk = atomicAdd(&ctl[16 + dep], 1ull);
    if ((int64_t)tk == nch - 1) {
        const int64_t total = (int64_t)__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[0] = total;
        out[1] = n;
        for (int q = 2; q < width; ++q) out[q] = 0;
        __hip_atomic_store(&ctl[0], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&ctl[16], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ctl: [0] the row counter, [16] the chunk ticket (128 B apart), both zero
// between calls
__global__ __launch_bounds__(kAccThreads) void k_acc_pack(int64_t n, int64_t offset, const int32_t* __restrict__ count,
                                                          const uint64_t* __restrict__ mask, const double* __restrict__ cpt,
                                                          int words, int vlb, int64_t cap,
                                                          unsigned long long* __restrict__ ctl,
                                                          int64_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int32_t s_cnt[kAccE];   // accepted per (j, wave), then their exclusive prefix
    __shared__ int64_t s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int width = 1 + words + (cpt ? 3 : 0);
    // count == null: the scorer's records [mask words, avg], |V| = popcount
    const int64_t ms = count ? words : words + 1;
    const int64_t nch = max((n + kAccChunk - 1) / kAccChunk, (int64_t)1);   // an empty slice still writes the header
    const int64_t b = blockIdx.x;
    // every load of the chunk in flight at once: the first mask words and the
    // counts (records: popcounts of the words)
    uint64_t m[kAccPer], w0[kAccPer];
    int c[kAccPer];
    double px[kAccPer], py[kAccPer], pz[kAccPer];
#pragma unroll
    for (int j = 0; j < kAccPer; ++j) {
        const int64_t i = b * kAccChunk + j * kAccThreads + threadIdx.x;
        w0[j] = i < n ? mask[i * ms] : 0ull;
        c[j] = i < n && count ? count[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < kAccPer; ++j) {
        const int64_t i = b * kAccChunk + j * kAccThreads + threadIdx.x;
        if (i < n && !count) {
            c[j] = __popcll(w0[j]);
            for (int q = 1; q < words; ++q) c[j] += __popcll(mask[i * ms + q]);
        }
    }
    // the accepted candidates' points, in flight across the scan and the
    // reservation (LDS-only barriers)
#pragma unroll
    for (int j = 0; j < kAccPer; ++j) {
        const int64_t i = b * kAccChunk + j * kAccThreads + threadIdx.x;
        const bool acc = i < n && c[j] >= vlb;
        m[j] = __ballot(acc);
        px[j] = py[j] = pz[j] = 0.0;
        if (cpt && acc) {
            // (every candidate's point loaded with the mask words instead --
            // coalesced, but 25 MB instead of the accepted ones' 6 MB:
            // 12.26 vs 11.18 us, profiles/r06/r6u_*)
            // x, y as one 16-B load (8-B aligned), z beside it
            const acc_d2 xy = *(const acc_d2*)(cpt + 3 * i);
            px[j] = xy.x;
            py[j] = xy.y;
            pz[j] = cpt[3 * i + 2];
        }
        if (lane == 0) s_cnt[j * kAccWaves + wave] = __popcll(m[j]);
    }
    lds_barrier();
    if (wave == 0) {
        // exclusive scan of the (j, wave) counts in index order, kAccEpl
        // consecutive ones per lane
        int x[kAccEpl], tot = 0;
#pragma unroll
        for (int q = 0; q < kAccEpl; ++q) {
            const int e = lane * kAccEpl + q;
            x[q] = e < kAccE ? s_cnt[e] : 0;
            tot += x[q];
        }
        int incl = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        int ex = incl - tot;
#pragma unroll
        for (int q = 0; q < kAccEpl; ++q) {
            const int e = lane * kAccEpl + q;
            if (e < kAccE) s_cnt[e] = ex;
            ex += x[q];
        }
        const unsigned long long T = (unsigned)__shfl(incl, 63, 64);   // this chunk's accepted
        if (lane == 0) {
            // this chunk's rows, then its ticket (after the reservation has
            // returned: the last ticket sees every chunk's rows counted)
            const unsigned long long base = T ? atomicAdd(&ctl[0], T) : 0ull;
            s_base = (int64_t)base;
        }
    }
    lds_barrier();
    const int64_t base = s_base;
    // the ticket is taken here, off the rows' critical path (11.07 vs 11.43
    // us with the ticket before the barrier, profiles/r06/r6m_*)
    if (threadIdx.x == 0) acc_ticket(ctl, (unsigned long long)base, nch, n, width, out);
#pragma unroll
    for (int j = 0; j < kAccPer; ++j) {
        if ((m[j] >> lane) & 1ull) {
            const int64_t i = b * kAccChunk + j * kAccThreads + threadIdx.x;
            const int64_t pos = base + s_cnt[j * kAccWaves + wave] +
                                __builtin_amdgcn_mbcnt_hi((uint32_t)(m[j] >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)m[j], 0u));
            if (pos < cap && words == 1 && cpt) {
                // the 40-B row as 16 + 16 + 8 B (8-B aligned stores)
                int64_t* o = out + (1 + pos) * width;
                *(acc_l2*)o = acc_l2{offset + i, (int64_t)w0[j]};
                *(acc_l2*)(o + 2) = acc_l2{__double_as_longlong(px[j]), __double_as_longlong(py[j])};
                o[4] = __double_as_longlong(pz[j]);
            } else if (pos < cap) {
                int64_t* o = out + (1 + pos) * width;
                o[0] = offset + i;
                o[1] = (int64_t)w0[j];
                for (int q = 1; q < words; ++q) o[1 + q] = (int64_t)mask[i * ms + q];
                if (cpt) {
                    // the accepted 3D point itself (binary64 bits)
                    o[1 + words] = __double_as_longlong(px[j]);
                    o[2 + words] = __double_as_longlong(py[j]);
                    o[3 + words] = __double_as_longlong(pz[j]);
                }
            }
        }
    }
}

// Measurement only (bench.py exchange.overlap_proxy): a copy of n 16-B pieces
// by a fixed number of workgroups -- the footprint of an RCCL all-gather's
// kernel (a few CUs streaming bytes) -- to run beside the scoring kernels.
// Eight pieces per thread in flight, as a collective's copy loop keeps them
// (one at a time makes the copy latency-bound: 3x slower beside the scorer,
// profiles/r05/r5a_overlap_probe_timeline_old_proxy.txt).
__global__ __launch_bounds__(256) void k_proxy_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n) {
    constexpr int U = 8;
    // one contiguous range per workgroup, U coalesced 4-KiB pieces in flight
    const int64_t per = (n + gridDim.x - 1) / gridDim.x;
    const int64_t b0 = (int64_t)blockIdx.x * per, b1 = min(n, b0 + per);
    for (int64_t i = b0 + threadIdx.x; i < b1; i += 256 * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = i + 256 * u < b1 ? src[i + 256 * u] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i + 256 * u < b1) dst[i + 256 * u] = v[u];
    }
}

}  // namespace

extern "C" int mvs_launch_pack_accepted(int64_t n, int64_t offset, const int32_t* count, const uint64_t* mask,
                                        const double* c, int words, int vlb, int64_t cap, unsigned long long* ctl,
                                        int64_t* out, hipStream_t s) {
    const int64_t nchunk = (n + kAccChunk - 1) / kAccChunk;
    if (nchunk >= ((int64_t)1 << 31)) return -3;
    const int grid = (int)std::max<int64_t>(1, nchunk);   // one workgroup per chunk
    // n == 0 still writes the header (chunk 0 of an empty slice)
    hipLaunchKernelGGL(k_acc_pack, dim3(grid), dim3(kAccThreads), 0, s, n, offset, count, mask, c, words, vlb, cap,
                       ctl, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mvs_launch_proxy_copy(void* dst, const void* src, int64_t bytes, int workgroups, hipStream_t s) {
    if (bytes <= 0) return 0;
    hipLaunchKernelGGL(k_proxy_copy, dim3(std::max(workgroups, 1)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst,
                       bytes / 16);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
