// Per-view depth maps of a warped patch set (mvs_wdepth_splat / _consist /
// _points, include/mvs_amd.h): a z-buffer splat of the oriented patches into
// the views, the cross-view depth consistency count of the maps, and the world
// points and colours of listed pixels.  No reference counterpart.
//
// k_wdepth_fill: one thread per pixel of the range: zmap = +inf's bits, idmap = -1.
// k_wdepth_splat<INDEX>: one wave per patch, four patches per workgroup, in two
//   phases per group of 64 views.  Phase A, lane = view: the patch centre's
//   projection, depth and facing test (one projection per view); the lanes
//   whose view takes the patch write (view, x0, y0, z, h) into the wave's own
//   LDS rows, compacted by their rank in the ballot.  Phase B flattens the
//   (taken view, footprint pixel) pairs over the lanes, 64 per pass: pair k is
//   pixel k % F of taken view k / F, F = (2 R + 1)^2, so a patch of 10 views
//   fills 90 of 128 lanes at R = 1, 250 of 256 at R = 2 and 490 of 512 at
//   R = 3 (a lane = view layout would fill 10 of 64).  A lane intersects its
//   pixel's ray with the patch plane and, inside the slope bound, does the
//   depth pass's 64-bit vector atomic min of s's bit pattern (positive doubles
//   order as unsigned integers) or, in the index pass, repeats the arithmetic
//   and the holders of the pixel's minimum do an unsigned 32-bit atomic min of
//   their index: k_wfilt_front's idiom.  Minimum and minimum among the holders
//   are order-free.
// k_wdepth_consist: one thread per pixel, blockIdx.y = view of the range, so
//   the pixel's own camera and, in the uniform loop over the other views, the
//   tested camera are wave-uniform (scalar loads); neighbouring pixels gather
//   neighbouring addresses of the other view's map.  No atomics, no LDS.
// k_wdepth_points: one thread per listed pixel.
// Binary64 in the library's operation order, compiled with -ffp-contract=off.
#include <algorithm>

#include "mvs_planes.h"

namespace {

constexpr uint64_t kInfBits = 0x7ff0000000000000ull;

DEV bool finite(double x) { return x > -__builtin_inf() && x < __builtin_inf(); }

__global__ __launch_bounds__(256) void k_wdepth_fill(int64_t pixels, uint64_t* zmap, int32_t* idmap) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < pixels; k += step) {
        zmap[k] = kInfBits;
        idmap[k] = -1;
    }
}

template <bool INDEX>
__global__ __launch_bounds__(256) void k_wdepth_splat(const SceneDev sc, const WdepthArgs a) {
    // a wave's taken views of one group of 64: rows of its own, no workgroup barrier
    __shared__ int s_v[4][64], s_x[4][64], s_y[4][64];
    __shared__ double s_z[4][64], s_h[4][64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave;
    if (p >= a.n) return;
    const int V = sc.V, words = (V + 63) >> 6, W = sc.W, H = sc.H;
    const int R = __builtin_amdgcn_readfirstlane(a.ref[p]);
    if (R < 0 || R >= V) return;   // a dead row draws nothing
    const double c[3] = {a.c[3 * p], a.c[3 * p + 1], a.c[3 * p + 2]};
    const double n[3] = {a.nrm[3 * p], a.nrm[3 * p + 1], a.nrm[3 * p + 2]};
    const int rad = a.radius, side = 2 * rad + 1, F = side * side;
    const int vend = a.v0 + a.nv;
    for (int g0 = a.v0 & ~63; g0 < vend; g0 += 64) {
        // ---- phase A, lane = view ----
        const int v = g0 + lane;
        const uint64_t word = a.mask[p * words + (g0 >> 6)];
        bool take = false;
        int x0 = 0, y0 = 0;
        double z = 0.0, h = 0.0;
        if (v >= a.v0 && v < vend && (v == R || ((word >> lane) & 1))) {
            const CamDev& cv = sc.cams[v];
            double px, py;
            project(cv, c, px, py);
            z = cv.Rp[6] * c[0] + cv.Rp[7] * c[1] + cv.Rp[8] * c[2] + cv.t[2];
            // x < W and y < H leave out nan and inf
            if (z > 0.0 && px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H) {
                double O[3];
                centre(cv, O);
                const double e[3] = {O[0] - c[0], O[1] - c[1], O[2] - c[2]};
                if (n[0] * e[0] + n[1] * e[1] + n[2] * e[2] > 0.0) {
                    const double f[3] = {c[0] - O[0], c[1] - O[1], c[2] - O[2]};
                    h = n[0] * f[0] + n[1] * f[1] + n[2] * f[2];
                    x0 = (int)(px + 0.5);
                    y0 = (int)(py + 0.5);
                    take = true;
                }
            }
        }
        const uint64_t b = __ballot(take);
        const int taken = __popcll(b);
        if (taken == 0) continue;   // (uniform)
        if (take) {
            const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0));
            s_v[wave][r] = v;
            s_x[wave][r] = x0;
            s_y[wave][r] = y0;
            s_z[wave][r] = z;
            s_h[wave][r] = h;
        }
        wave_lds_publish();
        // ---- phase B, lane = (taken view, footprint pixel) ----
        const int pairs = taken * F;
        for (int k0 = 0; k0 < pairs; k0 += 64) {
            const int k = k0 + lane;
            if (k >= pairs) continue;
            const int j = k / F, f = k - j * F;
            const int dy = f / side - rad, dx = f - (f / side) * side - rad;
            const int qx = s_x[wave][j] + dx, qy = s_y[wave][j] + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const int vj = s_v[wave][j];
            const double zj = s_z[wave][j];
            const CamDev& cv = sc.cams[vj];
            double d[3];
            pixel_ray(cv, qx, qy, d);
            const double den = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
            if (den == 0.0) continue;
            const double s = s_h[wave][j] / den;
            if (!(s > 0.0 && s < __builtin_inf())) continue;
            const int cheb = max(abs(dx), abs(dy));
            const double lim = a.slope * (double)(cheb + 1) * zj / ((cv.fx + cv.fy) / 2);
            if (!(fabs(s - zj) <= lim)) continue;
            const int64_t at = ((int64_t)(vj - a.v0) * H + qy) * W + qx;
            const uint64_t sb = (uint64_t)__double_as_longlong(s);
            if (!INDEX)
                atomicMin((unsigned long long*)a.zmap + at, (unsigned long long)sb);
            else if (a.zmap[at] == sb)
                atomicMin((unsigned int*)a.idmap + at, (unsigned int)p);
        }
        wave_lds_publish();   // the rows are rewritten by the next group
    }
}

__global__ __launch_bounds__(256) void k_wdepth_consist(const SceneDev sc, const WconsArgs a) {
    const int W = sc.W, H = sc.H;
    const int64_t hw = (int64_t)H * W;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= hw) return;
    const int vi = blockIdx.y, v = a.v0 + vi;   // uniform
    const int64_t at = (int64_t)vi * hw + q;
    const double z = a.zmap[at];
    int cons = 0, viol = 0;
    if (z > 0.0 && finite(z)) {
        const CamDev& cv = sc.cams[v];
        const int qy = (int)(q / W), qx = (int)(q - (int64_t)qy * W);
        double O[3], d[3], X[3];
        centre(cv, O);
        pixel_ray(cv, qx, qy, d);
#pragma unroll
        for (int m = 0; m < 3; ++m) X[m] = O[m] + z * d[m];
        for (int ui = 0; ui < a.nv; ++ui) {
            if (ui == vi) continue;
            const CamDev& cu = sc.cams[a.v0 + ui];
            double x, y;
            project(cu, X, x, y);
            const double depth = cu.Rp[6] * X[0] + cu.Rp[7] * X[1] + cu.Rp[8] * X[2] + cu.t[2];
            // int(x + 0.5) < W is x + 0.5 < W for x >= 0 (W an integer); nan and inf fail a comparison
            const double xr = x + 0.5, yr = y + 0.5;
            if (!(depth > 0.0 && x >= 0.0 && y >= 0.0 && xr < (double)W && yr < (double)H)) continue;
            const double zu = a.zmap[(int64_t)ui * hw + (int64_t)(int)yr * W + (int)xr];
            if (!finite(zu)) continue;   // a hole: unknown
            const double tol = a.rel_tol * depth;
            if (fabs(zu - depth) <= tol)
                ++cons;
            else if (zu - depth > tol)
                ++viol;
        }
    }
    a.cons[at] = (uint8_t)cons;
    if (a.viol) a.viol[at] = (uint8_t)viol;
}

__global__ __launch_bounds__(256) void k_wdepth_points(const SceneDev sc, const WpointsArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m) return;
    const int W = sc.W, H = sc.H;
    const int v = a.pix[3 * k], qx = a.pix[3 * k + 1], qy = a.pix[3 * k + 2];
    const double nan = __builtin_nan("");
    double X[3] = {nan, nan, nan};
    uint8_t rgb[3] = {0, 0, 0};
    // a pixel outside the range or the image reads nothing
    if (v >= a.v0 && v < a.v0 + a.nv && qx >= 0 && qx < W && qy >= 0 && qy < H) {
        const double z = a.zmap[((int64_t)(v - a.v0) * H + qy) * W + qx];
        if (z > 0.0 && finite(z)) {
            const CamDev& cv = sc.cams[v];
            double O[3], d[3];
            centre(cv, O);
            pixel_ray(cv, qx, qy, d);
            const uint8_t* px = sc.rgb + (((int64_t)v * H + qy) * W + qx) * 3;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                X[m] = O[m] + z * d[m];
                rgb[m] = px[m];
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        a.xyz[3 * k + m] = X[m];
        a.rgb[3 * k + m] = rgb[m];
    }
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" int mvs_launch_wdepth_splat(const SceneDev* sc, const WdepthArgs* a, hipStream_t s) {
    const int64_t pixels = (int64_t)a->nv * sc->H * sc->W;
    if (pixels > 0) {
        const int64_t blocks = std::min<int64_t>((pixels + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_wdepth_fill, dim3((unsigned)blocks), dim3(256), 0, s, pixels, a->zmap, a->idmap);
        if (!launched()) return -1;
    }
    if (a->n <= 0 || pixels <= 0) return 0;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    hipLaunchKernelGGL(k_wdepth_splat<false>, grid, block, 0, s, *sc, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wdepth_splat<true>, grid, block, 0, s, *sc, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wdepth_consist(const SceneDev* sc, const WconsArgs* a, hipStream_t s) {
    const int64_t hw = (int64_t)sc->H * sc->W;
    if (a->nv <= 0 || hw <= 0) return 0;
    const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)a->nv), block(256);
    hipLaunchKernelGGL(k_wdepth_consist, grid, block, 0, s, *sc, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wdepth_points(const SceneDev* sc, const WpointsArgs* a, hipStream_t s) {
    if (a->m <= 0) return 0;
    hipLaunchKernelGGL(k_wdepth_points, dim3((unsigned)((a->m + 255) / 256)), dim3(256), 0, s, *sc, *a);
    return launched() ? 0 : -1;
}
static_assert(MVS_MAX_VIEWS <= 65535, "k_wdepth_consist puts the view of the range in blockIdx.y");
