// Visibility-consistency filter for warped patch sets (mvs_wfilt_front /
// mvs_wfilt_test, include/mvs_amd.h): which patch is in front in every (view,
// cell), and which patches contradict the visibility of the rest of the set.
// No reference counterpart (the reference's filter_out_outlier knows neither
// normals nor depth order).
//
// k_wfilt_fill: one thread per (view, cell): zfront = +inf's bits, front = -1.
// k_wfilt_front<INDEX>: one wave per patch, four patches per workgroup, lane =
//   view (groups of 64 at V > 64), the layout of k_wexp_mark.  The depth pass
//   (INDEX = false) does a 64-bit vector atomic min of the depth's bit pattern
//   (positive doubles order as unsigned integers); the index pass repeats the
//   arithmetic and the holders of the cell's minimum do an unsigned 32-bit
//   atomic min of their index (-1 reads as 0xFFFFFFFF).  Minimum and minimum
//   among the holders are order-free, as in k_wexp_claim_*.
// k_wfilt_conflict<G>: the same layout.  A lane places the patch in its view,
//   gathers the cell's front patch and, when that is another patch, its centre
//   and normal for the adjacency test.  The vis words are ballots.  The distinct
//   conflicting front patches are found inside the wave: a lane's patch counts
//   when no earlier (group, lane) holds the same one (the set bits of the
//   conflict ballots are walked with v_readlane, as in k_refine_lists).  Every
//   counted lane adds w(p) onto conf[f] (64-bit vector atomic add); the wave's
//   sum of w(f) goes onto conf[p] by one more.  Integer sums: order-free.
// k_wfilt_decide: one thread per patch, after the conflict kernel.
// k_wfilt_support (mvs_wfilt_support): the same layout, a runtime loop over the
//   groups of 64 views.  A lane places the patch in its view, gathers the front
//   patches of the eight cells around that cell and their centres and normals,
//   and counts the neighbours (N) and the adjacent ones (A); the wave's sums
//   come from shuffles and one lane writes nb, adj and keep.  No atomics, no
//   LDS, no barrier.
// Binary64 in the library's operation order, compiled with -ffp-contract=off.
#include <algorithm>

#include "mvs_device.h"

namespace {

constexpr uint64_t kInfBits = 0x7ff0000000000000ull;

// the cell (i, j) of the patch centre in view v and its depth there; false when the patch is not placed
DEV bool place_ij(const SceneDev& sc, int v, const double* c, int cs, int nci, int ncj, int* i, int* j, double* depth) {
    const CamDev& cv = sc.cams[v];
    double px, py;
    project(cv, c, px, py);
    const double z = cv.Rp[6] * c[0] + cv.Rp[7] * c[1] + cv.Rp[8] * c[2] + cv.t[2];
    // x < W and y < H leave out nan and inf
    if (!(z > 0.0 && px >= 0.0 && px < (double)sc.W && py >= 0.0 && py < (double)sc.H)) return false;
    const int ci = (int)px / cs, cj = (int)py / cs;
    if (ci >= nci || cj >= ncj) return false;
    *i = ci;
    *j = cj;
    *depth = z;
    return true;
}

// the same with the cell as its index in the (V, ncj, nci) grids
DEV bool place(const SceneDev& sc, int v, const double* c, int cs, int nci, int ncj, int64_t* cell, double* depth) {
    int ci, cj;
    if (!place_ij(sc, v, c, cs, nci, ncj, &ci, &cj, depth)) return false;
    *cell = ((int64_t)v * ncj + cj) * nci + ci;
    return true;
}

// w = floor(clamp(avg, 0, 2) 2^32 + 0.5); 0 for nan and +-inf
DEV int64_t weight(double avg) {
    if (!(avg > -__builtin_inf() && avg < __builtin_inf())) return 0;
    const double x = avg < 0.0 ? 0.0 : avg > 2.0 ? 2.0 : avg;
    return (int64_t)floor(x * 4294967296.0 + 0.5);
}

__global__ __launch_bounds__(256) void k_wfilt_fill(int64_t cells, int32_t* front, uint64_t* zfront) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cells; k += step) {
        zfront[k] = kInfBits;
        front[k] = -1;
    }
}

template <bool INDEX>
__global__ __launch_bounds__(256) void k_wfilt_front(const SceneDev sc, const WfiltArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p >= a.n) return;
    const int V = sc.V, words = (V + 63) >> 6;
    const int cs = a.cell_size, nci = sc.W / cs, ncj = sc.H / cs;
    const int R = __builtin_amdgcn_readfirstlane(a.ref[p]);
    if (R < 0 || R >= V) return;   // a dead row takes no part
    const double c[3] = {a.c[3 * p], a.c[3 * p + 1], a.c[3 * p + 2]};
    for (int g0 = 0; g0 < V; g0 += 64) {
        const int v = g0 + lane;
        const uint64_t word = a.mask[p * words + (g0 >> 6)];
        if (v >= V || !(v == R || ((word >> lane) & 1))) continue;
        int64_t cell;
        double z;
        if (!place(sc, v, c, cs, nci, ncj, &cell, &z)) continue;
        const uint64_t zb = (uint64_t)__double_as_longlong(z);
        if (!INDEX)
            atomicMin((unsigned long long*)a.zfront + cell, (unsigned long long)zb);
        else if (a.zfront[cell] == zb)
            atomicMin((unsigned int*)a.front + cell, (unsigned int)p);
    }
}

DEV int64_t wave_sum64(int64_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += (int64_t)__shfl_xor((long long)x, off, 64);
    return x;
}

template <int G>
__global__ __launch_bounds__(256) void k_wfilt_conflict(const SceneDev sc, const WfiltArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p >= a.n) return;
    const int V = sc.V, words = (V + 63) >> 6;
    const int cs = a.cell_size, nci = sc.W / cs, ncj = sc.H / cs;
    const int R = __builtin_amdgcn_readfirstlane(a.ref[p]);
    uint64_t* const vis = a.vis + p * words;
    if (R < 0 || R >= V) {   // a dead row: no view, no conflict (k_wfilt_decide writes its conf and keep)
        if (lane < words) vis[lane] = 0;
        return;
    }
    const double c[3] = {a.c[3 * p], a.c[3 * p + 1], a.c[3 * p + 2]};
    const double n[3] = {a.nrm[3 * p], a.nrm[3 * p + 1], a.nrm[3 * p + 2]};
    int fg[G];   // view 64 g + lane: the front patch that hides p there, -1 = none
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int v = 64 * g + lane;
        bool seen = false;
        int f = -1;
        if (64 * g < V) {   // (uniform: the last word of a V <= 64 (G - 1) scene does not exist)
            const uint64_t word = a.mask[p * words + g];
            int64_t cell;
            double z;
            if (v < V && (v == R || ((word >> lane) & 1)) && place(sc, v, c, cs, nci, ncj, &cell, &z)) {
                int fr = a.front[cell];
                if (fr < -1 || fr >= a.n) fr = -1;   // reads nothing
                if (fr == p) {
                    seen = true;
                } else if (fr >= 0) {
                    const double* const cf = a.c + 3 * (int64_t)fr;
                    const double* const nf = a.nrm + 3 * (int64_t)fr;
                    const double d[3] = {c[0] - cf[0], c[1] - cf[1], c[2] - cf[2]};
                    const double dp = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
                    const double df = d[0] * nf[0] + d[1] * nf[1] + d[2] * nf[2];
                    const double rho = (a.adj_px * z) / ((sc.cams[v].fx + sc.cams[v].fy) / 2);
                    if (fabs(dp) + fabs(df) < 2.0 * rho)   // nan: not adjacent
                        seen = true;
                    else
                        f = fr;
                }
            }
            const uint64_t b = __ballot(seen);
            if (lane == 0) vis[g] = b;
        }
        fg[g] = f;
    }
    // F(p) as a set: a lane's patch counts when no earlier (group, lane) holds the same one
    bool first[G];
#pragma unroll
    for (int g = 0; g < G; ++g) first[g] = fg[g] >= 0;
#pragma unroll
    for (int gu = 0; gu < G; ++gu) {
        for (uint64_t pm = __ballot(fg[gu] >= 0); pm; pm &= pm - 1) {
            const int l = __builtin_ctzll(pm);
            const int fu = __builtin_amdgcn_readlane(fg[gu], l);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool later = gu < g || (gu == g && l < lane);
                if (later && fg[g] == fu) first[g] = false;
            }
        }
    }
    const int64_t wp = weight(a.avg[p]);
    int64_t own = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!first[g]) continue;
        own += weight(a.avg[fg[g]]);
        if (wp) atomicAdd((unsigned long long*)a.conf + fg[g], (unsigned long long)wp);
    }
    own = wave_sum64(own);
    if (lane == 0 && own) atomicAdd((unsigned long long*)a.conf + p, (unsigned long long)own);
}

__global__ __launch_bounds__(256) void k_wfilt_decide(int V, const WfiltArgs a) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const int words = (V + 63) >> 6;
    const int R = a.ref[p];
    if (R < 0 || R >= V) {
        a.conf[p] = 0;
        a.keep[p] = 0;
        return;
    }
    int tv = 0, seen = 0;
    for (int g = 0; g < words; ++g) {
        uint64_t m = a.mask[p * words + g];
        if (64 * g + 64 > V) m &= (1ull << (V & 63)) - 1;   // bits >= V name no view
        if ((R >> 6) == g) m |= 1ull << (R & 63);
        tv += __popcll(m);
        seen += __popcll(a.vis[p * words + g]);
    }
    a.keep[p] = seen >= a.min_views && (int64_t)tv * weight(a.avg[p]) >= a.conf[p];
}

DEV int wave_sum32(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// The neighbour-support test: a lane places the patch in its view and walks the
// eight cells around that cell.  Every neighbour cell whose front patch q is
// another patch is one incidence (N); it supports p (A) when p and q are
// adjacent in that view.  No state survives a group of 64 views but the two
// counts, so the groups are a runtime loop.  The gathers are latency-bound:
// eight waves per SIMD (at most 64 VGPRs) is asked for, the family's occupancy.
__global__ __launch_bounds__(256, 8) void k_wfilt_support(const SceneDev sc, const WsupArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p >= a.n) return;
    const int V = sc.V, words = (V + 63) >> 6;
    const int cs = a.cell_size, nci = sc.W / cs, ncj = sc.H / cs;
    const int R = __builtin_amdgcn_readfirstlane(a.ref[p]);
    if (R < 0 || R >= V) {   // a dead row: no neighbour, not kept
        if (lane == 0) {
            a.nb[p] = 0;
            a.adj[p] = 0;
            a.keep[p] = 0;
        }
        return;
    }
    const double c[3] = {a.c[3 * p], a.c[3 * p + 1], a.c[3 * p + 2]};
    const double n[3] = {a.nrm[3 * p], a.nrm[3 * p + 1], a.nrm[3 * p + 2]};
    int N = 0, A = 0;
    for (int g0 = 0; g0 < V; g0 += 64) {
        const int v = g0 + lane;
        const uint64_t word = a.mask[p * words + (g0 >> 6)];
        if (v >= V || !(v == R || ((word >> lane) & 1))) continue;
        int ci, cj;
        double z;
        if (!place_ij(sc, v, c, cs, nci, ncj, &ci, &cj, &z)) continue;
        const double rho = (a.adj_px * z) / ((sc.cams[v].fx + sc.cams[v].fy) / 2);
        const double lim = 2.0 * rho;
        // a row of the neighbourhood at a time: its three front entries first (independent
        // 4-byte gathers), then the rows they name.  A skipped neighbour reads p's own row
        // (in cache), so the loads need no branch and overlap.
#pragma unroll 1
        for (int dj = -1; dj <= 1; ++dj) {
            const int j = cj + dj;
            if (j < 0 || j >= ncj) continue;
            const int32_t* const row = a.front + ((int64_t)v * ncj + j) * nci;
            int q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int i = ci + k - 1;
                int f = -1;
                if (i >= 0 && i < nci && !(dj == 0 && k == 1)) f = row[i];
                if (f < -1 || f >= a.n || f == p) f = -1;   // reads nothing; p itself is no neighbour
                q[k] = f;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int64_t r = q[k] < 0 ? p : (int64_t)q[k];
                const double* const cf = a.c + 3 * r;
                const double* const nf = a.nrm + 3 * r;
                const double d[3] = {c[0] - cf[0], c[1] - cf[1], c[2] - cf[2]};
                const double dp = d[0] * n[0] + d[1] * n[1] + d[2] * n[2];
                const double df = d[0] * nf[0] + d[1] * nf[1] + d[2] * nf[2];
                N += q[k] >= 0;
                A += q[k] >= 0 && fabs(dp) + fabs(df) < lim;   // nan: not adjacent
            }
        }
    }
    N = wave_sum32(N);
    A = wave_sum32(A);
    if (lane == 0) {
        a.nb[p] = N;
        a.adj[p] = A;
        a.keep[p] = N >= a.min_neigh && (double)A >= a.min_support * (double)N;
    }
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" int mvs_launch_wfilt_front(const SceneDev* sc, const WfiltArgs* a, hipStream_t s) {
    const int64_t cells = (int64_t)sc->V * (sc->H / a->cell_size) * (sc->W / a->cell_size);
    if (cells > 0) {
        const int64_t blocks = std::min<int64_t>((cells + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_wfilt_fill, dim3((unsigned)blocks), dim3(256), 0, s, cells, a->front, a->zfront);
        if (!launched()) return -1;
    }
    if (a->n <= 0 || cells <= 0) return 0;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    hipLaunchKernelGGL(k_wfilt_front<false>, grid, block, 0, s, *sc, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wfilt_front<true>, grid, block, 0, s, *sc, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wfilt_test(const SceneDev* sc, const WfiltArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    if (hipMemsetAsync(a->conf, 0, a->n * sizeof(int64_t), s) != hipSuccess) return -1;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    switch ((sc->V + 63) / 64) {
        case 1: hipLaunchKernelGGL(k_wfilt_conflict<1>, grid, block, 0, s, *sc, *a); break;
        case 2: hipLaunchKernelGGL(k_wfilt_conflict<2>, grid, block, 0, s, *sc, *a); break;
        case 3: hipLaunchKernelGGL(k_wfilt_conflict<3>, grid, block, 0, s, *sc, *a); break;
        case 4: hipLaunchKernelGGL(k_wfilt_conflict<4>, grid, block, 0, s, *sc, *a); break;
        default: return -1;
    }
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wfilt_decide, dim3((unsigned)((a->n + 255) / 256)), dim3(256), 0, s, sc->V, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wfilt_support(const SceneDev* sc, const WsupArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_wfilt_support, dim3((unsigned)((a->n + 3) / 4)), dim3(256), 0, s, *sc, *a);
    return launched() ? 0 : -1;
}
static_assert(MVS_MAX_VIEWS == 256, "k_wfilt_conflict holds at most four front patches per lane");
