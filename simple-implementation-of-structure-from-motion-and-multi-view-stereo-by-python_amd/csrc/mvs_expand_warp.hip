// Level-synchronous patch expansion driven by the plane-warped photo test
// (mvs_wexp_children / mvs_wexp_claim / mvs_wexp_mark, include/mvs_amd.h): the
// three device primitives a caller runs between score_warped and refine_warped
// calls to grow a patch set one wavefront at a time.  No reference counterpart
// (the reference's expansion ignores the normal and never refines).
//
// k_wexp_children<EMIT>: one wave per frontier patch, four patches per
//   workgroup, lane = view (groups of 64 at V > 64).  A lane keeps its camera
//   in registers, projects the patch centre, gathers the four neighbour cells'
//   occupancy bytes and intersects the four cell-centre rays with the parent's
//   tangent plane.  The in-patch order (view, then neighbour k) comes from four
//   ballots and mbcnt.  The order across patches comes from a count pass
//   (EMIT = false: cnt[p]), k_wexp_scan (one workgroup: exclusive int64 offsets
//   and the total) and the emit pass (EMIT = true), which repeats the count
//   pass's arithmetic operation for operation -- no atomics anywhere.
// k_wexp_claim_max / _min / _win / _reset: one thread per job on a per-(view,
//   cell) grid of 64-bit keys and 32-bit tickets that is zero between calls:
//   64-bit vector atomic max of an order-preserving image of the score, atomic
//   max of ~index among the jobs that hold the cell's maximum (= the lowest
//   index), the winners' flags, then the touched cells back to zero.  Maximum
//   and minimum are order-free, so the result does not depend on scheduling.
// k_wexp_mark: one wave per job, lane = view of the winner's mask; byte stores
//   of 1 (a set: order-free).
// Binary64 in the library's operation order, compiled with -ffp-contract=off.
#include "mvs_device.h"

namespace {

constexpr int kScanThreads = 1024;

template <bool EMIT>
__global__ __launch_bounds__(256) void k_wexp_children(const SceneDev sc, const WexpArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p >= a.n) return;
    const int V = sc.V, words = (V + 63) >> 6;
    const int cs = a.cell_size, nci = sc.W / cs, ncj = sc.H / cs;
    const double half = (double)(cs - 1) / 2.0;
    const int R = __builtin_amdgcn_readfirstlane(a.ref[p]);
    const double c[3] = {a.c[3 * p], a.c[3 * p + 1], a.c[3 * p + 2]};
    const double n[3] = {a.nrm[3 * p], a.nrm[3 * p + 1], a.nrm[3 * p + 2]};
    const int64_t base = EMIT ? a.offs[p] : 0;
    int run = 0;   // jobs of the groups before this one
    for (int g0 = 0; g0 < V; g0 += 64) {
        const int v = g0 + lane;
        const uint64_t word = a.mask[p * words + (g0 >> 6)];
        const bool active = v < V && (v == R || ((word >> lane) & 1));
        bool ok[4] = {false, false, false, false};
        double X[4][3];
        int ci = 0, cj = 0;
        if (active) {
            const CamDev& cv = sc.cams[v];
            double Rp[9], t[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp[k] = cv.Rp[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = cv.t[k];
            const double fx = cv.fx, fy = cv.fy, cx = cv.cx, cy = cv.cy;
            double px, py;
            project(cv, c, px, py);
            const double z = Rp[6] * c[0] + Rp[7] * c[1] + Rp[8] * c[2] + t[2];
            // x < W and y < H leave out nan and inf
            if (z > 0.0 && px >= 0.0 && px < (double)sc.W && py >= 0.0 && py < (double)sc.H) {
                ci = (int)px / cs;
                cj = (int)py / cs;
                if (ci < nci && cj < ncj) {
                    double O[3], e[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        O[k] = -(Rp[k] * t[0] + Rp[3 + k] * t[1] + Rp[6 + k] * t[2]);
                        e[k] = c[k] - O[k];
                    }
                    const double h = n[0] * e[0] + n[1] * e[1] + n[2] * e[2];
                    const uint8_t* occ = a.occ + (int64_t)v * ncj * nci;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int ai = ci + (k == 0) - (k == 1), bj = cj + (k == 2) - (k == 3);
                        if (ai < 0 || ai >= nci || bj < 0 || bj >= ncj) continue;
                        if (occ[(int64_t)bj * nci + ai]) continue;
                        const double u = (((double)(ai * cs) + half) - cx) / fx;
                        const double w = (((double)(bj * cs) + half) - cy) / fy;
                        double d[3];
#pragma unroll
                        for (int m = 0; m < 3; ++m) d[m] = Rp[m] * u + Rp[3 + m] * w + Rp[6 + m];
                        const double den = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
                        if (den == 0.0) continue;
                        const double s = h / den;
                        if (!(s > 0.0 && s < __builtin_inf())) continue;
                        double q[3];
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
                            X[k][m] = O[m] + d[m] * s;
                            q[m] = X[k][m] - c[m];
                        }
                        ok[k] = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) <= a.max_dist;
                    }
                }
            }
        }
        // (view, k) order inside the group: the jobs of the lanes below, then the lane's own lower k
        int below = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t b = __ballot(ok[k]);
            below += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0));
            total += __popcll(b);
        }
        if (EMIT) {
            int64_t at = base + run + below;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!ok[k]) continue;
                if (at < a.cap) {
                    const int ai = ci + (k == 0) - (k == 1), bj = cj + (k == 2) - (k == 3);
                    a.job[at] = make_int4((int)p, v, ai, bj);
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        a.cc[3 * at + m] = X[k][m];
                        a.cn[3 * at + m] = n[m];
                    }
                    a.cref[at] = v;
                }
                ++at;
            }
        }
        run += total;
    }
    if (!EMIT && lane == 0) a.cnt[p] = run;
}

// offs[k] = cnt[0] + ... + cnt[k-1] (int64), offs[n] and total[0] = the sum; one workgroup
__global__ __launch_bounds__(kScanThreads) void k_wexp_scan(const int32_t* cnt, int64_t n, int64_t* offs,
                                                            int64_t* total) {
    __shared__ int64_t part[kScanThreads];
    const int tid = threadIdx.x;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads;
    const int64_t b = min((int64_t)tid * per, n), e = min(b + per, n);
    int64_t s = 0;
    for (int64_t k = b; k < e; ++k) s += cnt[k];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int64_t v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t r = tid ? part[tid - 1] : 0;
    for (int64_t k = b; k < e; ++k) {
        offs[k] = r;
        r += cnt[k];
    }
    if (tid == kScanThreads - 1) {
        offs[n] = part[tid];
        total[0] = part[tid];
    }
}

// Order-preserving image of a finite score (-0.0 as +0.0), never 0; 0 for a
// job that does not contend.
DEV uint64_t claim_key(const ClaimArgs& a, int64_t k, int64_t* cell) {
    const int4 j = a.job[k];
    *cell = -1;
    if (j.y < 0 || j.y >= a.V || j.z < 0 || j.z >= a.nci || j.w < 0 || j.w >= a.ncj) return 0;
    *cell = ((int64_t)j.y * a.ncj + j.w) * a.nci + j.z;
    double s = a.score[k];
    if (!a.accept[k] || !(s > -__builtin_inf() && s < __builtin_inf())) return 0;
    s = s + 0.0;   // -0.0 + 0.0 = +0.0 (round to nearest)
    const uint64_t u = (uint64_t)__double_as_longlong(s);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void k_wexp_claim_max(const ClaimArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m) return;
    int64_t cell;
    const uint64_t key = claim_key(a, k, &cell);
    if (key) atomicMax((unsigned long long*)a.key + cell, (unsigned long long)key);
}

// among the holders of the cell's maximum, the lowest index: max of ~k (never 0: k < 2^31)
__global__ void k_wexp_claim_min(const ClaimArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m) return;
    int64_t cell;
    const uint64_t key = claim_key(a, k, &cell);
    if (key && a.key[cell] == key) atomicMax(a.ticket + cell, ~(uint32_t)k);
}

__global__ void k_wexp_claim_win(const ClaimArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m) return;
    int64_t cell;
    const uint64_t key = claim_key(a, k, &cell);
    a.win[k] = key && a.key[cell] == key && a.ticket[cell] == ~(uint32_t)k;
}

// the cells the jobs name back to zero (every writer stores the same value)
__global__ void k_wexp_claim_reset(const ClaimArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m) return;
    int64_t cell;
    (void)claim_key(a, k, &cell);
    if (cell >= 0) {
        a.key[cell] = 0;
        a.ticket[cell] = 0;
    }
}

__global__ __launch_bounds__(256) void k_wexp_mark(const SceneDev sc, const MarkArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    if (k >= a.m || !a.win[k]) return;
    const int V = sc.V, words = (V + 63) >> 6;
    const int cs = a.cell_size, nci = sc.W / cs, ncj = sc.H / cs;
    const int4 j = a.job[k];
    const int R = a.cref[k];
    // the winner's own cell, as the job names it (no reprojection)
    // (a byte that is nonzero already stays as it is: every writer of this call stores 1 into a zero byte)
    if (lane == 0 && R >= 0 && R < V && j.z >= 0 && j.z < nci && j.w >= 0 && j.w < ncj) {
        uint8_t* o = a.occ + ((int64_t)R * ncj + j.w) * nci + j.z;
        if (!*o) *o = 1;
    }
    const double c[3] = {a.cc[3 * k], a.cc[3 * k + 1], a.cc[3 * k + 2]};
    for (int g0 = 0; g0 < V; g0 += 64) {
        const int v = g0 + lane;
        const uint64_t word = a.mask[k * words + (g0 >> 6)];
        if (v >= V || !((word >> lane) & 1)) continue;
        const CamDev& cv = sc.cams[v];
        double px, py;
        project(cv, c, px, py);
        const double z = cv.Rp[6] * c[0] + cv.Rp[7] * c[1] + cv.Rp[8] * c[2] + cv.t[2];
        if (!(z > 0.0 && px >= 0.0 && px < (double)sc.W && py >= 0.0 && py < (double)sc.H)) continue;
        const int ci = (int)px / cs, cj = (int)py / cs;
        if (ci < nci && cj < ncj) {
            uint8_t* o = a.occ + ((int64_t)v * ncj + cj) * nci + ci;
            if (!*o) *o = 1;
        }
    }
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" int mvs_launch_wexp_children(const SceneDev* sc, const WexpArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    hipLaunchKernelGGL(k_wexp_children<false>, grid, block, 0, s, *sc, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wexp_scan, dim3(1), dim3(kScanThreads), 0, s, a->cnt, a->n, a->offs, a->total);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wexp_children<true>, grid, block, 0, s, *sc, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wexp_claim(const ClaimArgs* a, hipStream_t s) {
    if (a->m <= 0) return 0;
    const dim3 grid((unsigned)((a->m + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_wexp_claim_max, grid, block, 0, s, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wexp_claim_min, grid, block, 0, s, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wexp_claim_win, grid, block, 0, s, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wexp_claim_reset, grid, block, 0, s, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wexp_mark(const SceneDev* sc, const MarkArgs* a, hipStream_t s) {
    if (a->m <= 0) return 0;
    const dim3 grid((unsigned)((a->m + 3) / 4)), block(256);
    hipLaunchKernelGGL(k_wexp_mark, grid, block, 0, s, *sc, *a);
    return launched() ? 0 : -1;
}
