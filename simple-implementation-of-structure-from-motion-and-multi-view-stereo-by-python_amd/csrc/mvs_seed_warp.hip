// Seeds of the warped pipeline from image features (mvs_wseed_match) and the
// colours of a patch set (mvs_wpatch_color), include/mvs_amd.h.  No reference
// counterpart: the reference seeds from SfM tracks (MVS2.py:196-262).
//
// k_wseed_pairs<EMIT>: one workgroup of 256 threads per (view pair, block of
//   256 features a of the reference view r), thread = feature a.  A thread
//   keeps its ray d_a, A = d_a.d_a and D = d_a.w in registers; the cameras of r
//   and v are wave-uniform.  The features b of view v come in LDS tiles of
//   MVS_SEED_TILE: every thread prepares one b per tile (its ray d_b, C =
//   d_b.d_b, E = d_b.w and the pixel), then walks the tile -- every lane reads
//   the same LDS address, a broadcast -- and tests (a, b): the two rays' closest
//   points, the point on a's ray projected into v, the distance to b.  The
//   thread's loop over b is the order inside a row (pair, a); the order across
//   rows comes from a count pass (EMIT = false: cnt[row]), k_wseed_scan (one
//   workgroup: exclusive int64 offsets and the total) and the emit pass (EMIT =
//   true), which repeats the count pass's arithmetic operation for operation --
//   no atomics anywhere, as k_wexp_children / k_wexp_scan.
// k_wpatch_color: one wave per patch, four patches per workgroup, lane = view
//   (a runtime loop over the groups of 64 views), the layout of k_wfilt_front.
//   A lane projects the centre into its view and samples the three channels of
//   the resident RGB image bilinearly; the samples become integers (1/256 of a
//   gray level), so the wave's sums do not depend on the order of the shuffles.
// Binary64 in the library's operation order, compiled with -ffp-contract=off.
#include "mvs_device.h"

namespace {

constexpr int kScanThreads = 1024;
constexpr int kBlock = MVS_SEED_BLOCK, kTile = MVS_SEED_TILE;

// O = -Rp^T t, the order of k_wexp_children
DEV void centre(const CamDev& cm, double* O) {
#pragma unroll
    for (int k = 0; k < 3; ++k) O[k] = -(cm.Rp[k] * cm.t[0] + cm.Rp[3 + k] * cm.t[1] + cm.Rp[6 + k] * cm.t[2]);
}

// d = Rp^T ((x - cx) / fx, (y - cy) / fy, 1) of the integer pixel (x, y)
DEV void pixel_ray(const CamDev& cm, int x, int y, double* d) {
    const double u = ((double)x - cm.cx) / cm.fx, w = ((double)y - cm.cy) / cm.fy;
#pragma unroll
    for (int m = 0; m < 3; ++m) d[m] = cm.Rp[m] * u + cm.Rp[3 + m] * w + cm.Rp[6 + m];
}

DEV double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void k_wseed_pairs(const SceneDev sc, const WseedArgs a) {
    // per feature b of the tile: d_b (3), C, E, pixel x, y
    __shared__ double sb[7][kTile];
    const int tid = threadIdx.x;
    const int2 blk = a.blocks[blockIdx.x];
    const int k = __builtin_amdgcn_readfirstlane(blk.x);
    const SeedPair P = a.pairs[k];
    const int r = __builtin_amdgcn_readfirstlane(P.r), v = __builtin_amdgcn_readfirstlane(P.v);
    const int na = __builtin_amdgcn_readfirstlane(P.na), nb = __builtin_amdgcn_readfirstlane(P.nb);
    const int b0 = __builtin_amdgcn_readfirstlane(P.b0);
    const int ia = __builtin_amdgcn_readfirstlane(blk.y) + tid;
    const bool active = ia < na;
    const CamDev& cr = sc.cams[r];
    const CamDev& cv = sc.cams[v];
    double Or[3], Ov[3], w[3];
    centre(cr, Or);
    centre(cv, Ov);
#pragma unroll
    for (int m = 0; m < 3; ++m) w[m] = Or[m] - Ov[m];
    double da[3] = {0, 0, 0};
    if (active) {
        const int32_t* q = a.feat + 2 * ((int64_t)P.a0 + ia);
        pixel_ray(cr, q[0], q[1], da);
    }
    const double A = dot3(da, da), D = dot3(da, w);
    const int64_t row = P.row0 + ia;
    int64_t at = EMIT && active ? a.offs[row] : 0;
    int count = 0;
    for (int t0 = 0; t0 < nb; t0 += kTile) {
        const int m = min(kTile, nb - t0);
        __syncthreads();   // the tile before this one has been read
        for (int j = tid; j < m; j += kBlock) {
            const int32_t* q = a.feat + 2 * ((int64_t)b0 + t0 + j);
            const int qx = q[0], qy = q[1];
            double db[3];
            pixel_ray(cv, qx, qy, db);
            sb[0][j] = db[0];
            sb[1][j] = db[1];
            sb[2][j] = db[2];
            sb[3][j] = dot3(db, db);
            sb[4][j] = dot3(db, w);
            sb[5][j] = (double)qx;
            sb[6][j] = (double)qy;
        }
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < m; ++j) {
            const double db[3] = {sb[0][j], sb[1][j], sb[2][j]};
            const double C = sb[3][j], E = sb[4][j];
            const double B = dot3(da, db);
            const double AC = A * C;
            const double den = AC - B * B;
            if (!(den > a.min_sin2 * AC)) continue;   // parallel rays, nan
            const double s = (B * E - C * D) / den, u = (A * E - B * D) / den;
            if (!(s > 0.0 && s < __builtin_inf() && u > 0.0 && u < __builtin_inf())) continue;
            const double X[3] = {Or[0] + s * da[0], Or[1] + s * da[1], Or[2] + s * da[2]};
            double px, py;
            project(cv, X, px, py);
            const double z = cv.Rp[6] * X[0] + cv.Rp[7] * X[1] + cv.Rp[8] * X[2] + cv.t[2];
            const double ex = px - sb[5][j], ey = py - sb[6][j];
            const double e2 = ex * ex + ey * ey;
            if (!(z > 0.0 && e2 <= a.epi2)) continue;
            if (EMIT) {
                if (at < a.cap) {
                    const double e[3] = {Or[0] - X[0], Or[1] - X[1], Or[2] - X[2]};
                    const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        a.c[3 * at + i] = X[i];
                        a.nrm[3 * at + i] = e[i] / len;
                    }
                    a.ref[at] = r;
                    int32_t* cd = a.cand + 4 * at;
                    cd[0] = k;
                    cd[1] = ia;
                    cd[2] = t0 + j;
                    cd[3] = v;
                    a.err[at] = e2;
                }
                ++at;
            }
            ++count;
        }
    }
    if (!EMIT && active) a.cnt[row] = count;
}

// offs[k] = cnt[0] + ... + cnt[k-1] (int64), offs[n] and total[0] = the sum; one workgroup (k_wexp_scan's scheme)
__global__ __launch_bounds__(kScanThreads) void k_wseed_scan(const int32_t* cnt, int64_t n, int64_t* offs,
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

DEV int64_t wave_sum64(int64_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += (int64_t)__shfl_xor((long long)x, off, 64);
    return x;
}

__global__ __launch_bounds__(256) void k_wpatch_color(const SceneDev sc, const WcolArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p >= a.n) return;
    const int V = sc.V, words = (V + 63) >> 6;
    const int W = sc.W, H = sc.H;
    const double Wm1 = (double)(W - 1), Hm1 = (double)(H - 1);
    const int R = __builtin_amdgcn_readfirstlane(a.ref[p]);
    const double c[3] = {a.c[3 * p], a.c[3 * p + 1], a.c[3 * p + 2]};
    int64_t sum[3] = {0, 0, 0};
    int m = 0;
    for (int g0 = 0; g0 < V; g0 += 64) {
        const int v = g0 + lane;
        const uint64_t word = a.mask[p * words + (g0 >> 6)];
        bool counted = false;
        int64_t K[3] = {0, 0, 0};
        if (v < V && (v == R || ((word >> lane) & 1))) {
            const CamDev& cv = sc.cams[v];
            double x, y;
            project(cv, c, x, y);
            const double z = cv.Rp[6] * c[0] + cv.Rp[7] * c[1] + cv.Rp[8] * c[2] + cv.t[2];
            // x <= W - 1 and y <= H - 1 leave out nan and inf
            if (z > 0.0 && x >= 0.0 && x <= Wm1 && y >= 0.0 && y <= Hm1) {
                counted = true;
                const int ix = (int)x, iy = (int)y;
                const double ax = x - (double)ix, ay = y - (double)iy;
                const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
                const uint8_t* img = sc.rgb + (int64_t)v * H * W * 3;
                const uint8_t* r0 = img + (int64_t)iy * W * 3;
                const uint8_t* r1 = img + (int64_t)iy1 * W * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double g00 = (double)r0[3 * ix + ch], g01 = (double)r0[3 * ix1 + ch];
                    const double g10 = (double)r1[3 * ix + ch], g11 = (double)r1[3 * ix1 + ch];
                    const double top = g00 + ax * (g01 - g00);
                    const double bot = g10 + ax * (g11 - g10);
                    const double S = top + ay * (bot - top);
                    K[ch] = (int64_t)floor(S * 256.0 + 0.5);
                }
            }
        }
        m += __popcll(__ballot(counted));
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sum[ch] += wave_sum64(K[ch]);
    }
    if (lane == 0) {
        const double den = (double)(256 * (int64_t)m);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.color[3 * p + ch] = m ? (double)sum[ch] / den : 0.0;
        a.nviews[p] = m;
    }
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" int mvs_launch_wseed_match(const SceneDev* sc, const WseedArgs* a, hipStream_t s) {
    const dim3 grid((unsigned)a->nblocks), block(kBlock);
    if (a->nblocks > 0) {
        hipLaunchKernelGGL(k_wseed_pairs<false>, grid, block, 0, s, *sc, *a);
        if (!launched()) return -1;
    }
    hipLaunchKernelGGL(k_wseed_scan, dim3(1), dim3(kScanThreads), 0, s, a->cnt, a->rows, a->offs, a->total);
    if (!launched()) return -1;
    if (a->nblocks > 0 && a->cap > 0) {
        hipLaunchKernelGGL(k_wseed_pairs<true>, grid, block, 0, s, *sc, *a);
        if (!launched()) return -1;
    }
    return 0;
}

extern "C" int mvs_launch_wpatch_color(const SceneDev* sc, const WcolArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    hipLaunchKernelGGL(k_wpatch_color, dim3((unsigned)((a->n + 3) / 4)), dim3(256), 0, s, *sc, *a);
    return launched() ? 0 : -1;
}
