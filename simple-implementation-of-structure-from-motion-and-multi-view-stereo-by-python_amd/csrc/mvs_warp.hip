// Plane-warped photo-consistency test (mvs_score_warped, include/mvs_amd.h):
// the reference window of a patch, taken at integer pixels of its reference
// view, is carried through the patch plane (centre c, unit normal nrm) into
// every other view, sampled there bilinearly and compared with ctNcc's
// scaling.  No reference counterpart: the reference's test cuts every view's
// window at the reference view's pixel (MVS2.py:68) and never uses the normal.
//
// k_score_warp: one wave per candidate, four candidates per workgroup.
//   1. the wave projects c into its reference view r (the projection of
//      mvs_score, bit for bit) and tests the candidate;
//   2. lane = sample: the plane point X of every window pixel (ray of the
//      pixel through view r meets the patch plane) and the pixel's gray value
//      go to LDS, 32 B per sample; sum a and D_a by a wave reduction of
//      exact integers;
//   3. lane = view (groups of 64 at V > 64): the lane keeps its camera in
//      registers, walks the N samples (X and a are LDS broadcasts), projects,
//      gathers its four bytes from the view-major plane gv[v][y][x], and keeps
//      sum b, sum b^2, sum a b to itself -- no cross-lane traffic inside the
//      loop; the mask word is a ballot, avg a wave sum in a fixed order.
// All arithmetic on positions, samples and sums is binary64 on s = g - 128
// (NCC is shift-invariant).  Compiled with -ffp-contract=off: fused products
// are the ones written as fma().
#include "mvs_device.h"

namespace {

struct WarpSample {
    double X, Y, Z;   // plane point of the window pixel
    double a;         // reference gray value - 128
};

template <int WID>
__global__ __launch_bounds__(256) void k_score_warp(const SceneDev sc, const WarpArgs a) {
    constexpr int S = 2 * WID + 1, N = S * S;
    __shared__ WarpSample smp[4][N];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t cand = (int64_t)blockIdx.x * 4 + wave;
    if (cand >= a.n) return;   // no workgroup barrier below: a wave works on its own LDS rows
    const int V = sc.V, words = (V + 63) >> 6;
    const double nan = __builtin_nan("");
    uint64_t* const mask = a.mask + cand * words;
    double* const ncc_out = a.ncc ? a.ncc + cand * V : nullptr;

    const int R = __builtin_amdgcn_readfirstlane(a.ref[cand]);
    const double c[3] = {a.c[3 * cand], a.c[3 * cand + 1], a.c[3 * cand + 2]};
    const double n[3] = {a.nrm[3 * cand], a.nrm[3 * cand + 1], a.nrm[3 * cand + 2]};
    bool valid = R >= 0 && R < V;
    double px = nan, py = nan;
    double Or[3] = {0, 0, 0}, h = 0;   // O_r and nrm . (c - O_r)
    int x0 = 0, y0 = 0;
    if (valid) {
        const CamDev& cr = sc.cams[R];
        project(cr, c, px, py);
        const double z = cr.Rp[6] * c[0] + cr.Rp[7] * c[1] + cr.Rp[8] * c[2] + cr.t[2];
        valid = z > 0.0 && px >= 0.0 && py >= 0.0 && py_trunc(px, &x0) && py_trunc(py, &y0);
        valid = valid && x0 - WID >= 0 && x0 + WID <= sc.W - 1 && y0 - WID >= 0 && y0 + WID <= sc.H - 1;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Or[k] = -(cr.Rp[k] * cr.t[0] + cr.Rp[3 + k] * cr.t[1] + cr.Rp[6 + k] * cr.t[2]);
        const double e[3] = {Or[0] - c[0], Or[1] - c[1], Or[2] - c[2]};
        const double ne = n[0] * e[0] + n[1] * e[1] + n[2] * e[2];
        valid = valid && ne > a.min_cos * sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        h = -ne;
    }
    if (lane == 0) { a.xy[2 * cand] = px; a.xy[2 * cand + 1] = py; }

    double Sa = 0, Da = 0;
    if (valid) {
        // lane = sample: plane points and reference pixels into LDS
        const CamDev& cr = sc.cams[R];
        const int8_t* gr = (const int8_t*)sc.gv + (int64_t)R * sc.H * sc.Wp;
        int sa = 0, saa = 0;
        for (int i = lane; i < N; i += 64) {
            const int dy = i / S - WID, dx = i % S - WID;
            const double u = ((double)(x0 + dx) - cr.cx) / cr.fx, w = ((double)(y0 + dy) - cr.cy) / cr.fy;
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = cr.Rp[k] * u + cr.Rp[3 + k] * w + cr.Rp[6 + k];
            const double s = h / (n[0] * d[0] + n[1] * d[1] + n[2] * d[2]);
            const int g = gr[(int64_t)(y0 + dy) * sc.Wp + x0 + dx];   // window inside the image (tested above)
            WarpSample sm;
            sm.X = Or[0] + d[0] * s;
            sm.Y = Or[1] + d[1] * s;
            sm.Z = Or[2] + d[2] * s;
            sm.a = (double)g;
            smp[wave][i] = sm;
            sa += g;
            saa += g * g;
        }
        sa = wave_sum(sa);
        saa = wave_sum(saa);
        Sa = (double)sa;
        Da = (double)(N * saa - sa * sa);   // exact: |.| < 2^31 at N <= 121, |g| <= 128
        valid = Da > 0.0;
    }
    if (!valid) {
        if (lane < words) mask[lane] = 0;
        if (lane == 0) {
            a.count[cand] = 0;
            if (a.avg) a.avg[cand] = 0.0;
        }
        if (ncc_out)
            for (int v = lane; v < V; v += 64) ncc_out[v] = nan;
        return;
    }
    wave_lds_publish();

    const double Wm1 = (double)(sc.W - 1), Hm1 = (double)(sc.H - 1);
    const double scale = (double)N / (double)(N - 1);
    int count = 0;
    double sum = 0.0;
    for (int g0 = 0; g0 < V; g0 += 64) {
        const int v = g0 + lane;
        double ncc = nan;
        bool tested = v < V && v != R;
        double Rp[9], t[3], fx = 0, fy = 0, cx = 0, cy = 0;
        if (tested) {
            const CamDev& cv = sc.cams[v];
#pragma unroll
            for (int k = 0; k < 9; ++k) Rp[k] = cv.Rp[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = cv.t[k];
            fx = cv.fx; fy = cv.fy; cx = cv.cx; cy = cv.cy;
            double e[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) e[k] = -(Rp[k] * t[0] + Rp[3 + k] * t[1] + Rp[6 + k] * t[2]) - c[k];
            tested = n[0] * e[0] + n[1] * e[1] + n[2] * e[2] >
                     a.min_cos * sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        }
        if (tested) {
            const int8_t* gvv = (const int8_t*)sc.gv + (int64_t)v * sc.H * sc.Wp;
            const int Wp = sc.Wp, W1 = sc.W - 1, H1 = sc.H - 1;
            bool ok = true;
            double Sb = 0, Sbb = 0, Sab = 0;
            for (int i = 0; i < N; ++i) {
                const WarpSample sm = smp[wave][i];
                const double x = fma(Rp[0], sm.X, fma(Rp[1], sm.Y, fma(Rp[2], sm.Z, t[0])));
                const double y = fma(Rp[3], sm.X, fma(Rp[4], sm.Y, fma(Rp[5], sm.Z, t[1])));
                const double z = fma(Rp[6], sm.X, fma(Rp[7], sm.Y, fma(Rp[8], sm.Z, t[2])));
                const double rz = recip(z);
                const double sx = fma(x * rz, fx, cx), sy = fma(y * rz, fy, cy);
                ok = ok && z > 0.0 && sx >= 0.0 && sx <= Wm1 && sy >= 0.0 && sy <= Hm1;
                // a sample outside the image has failed its view already:
                // its addresses are held inside the image all the same
                const double sxc = fmin(fmax(sx, 0.0), Wm1), syc = fmin(fmax(sy, 0.0), Hm1);
                const int ix = min(max((int)sxc, 0), W1), iy = min(max((int)syc, 0), H1);
                const double ax = sxc - (double)ix, ay = syc - (double)iy;
                const int ix1 = min(ix + 1, W1), iy1 = min(iy + 1, H1);
                const int8_t* r0 = gvv + (int64_t)iy * Wp;
                const int8_t* r1 = gvv + (int64_t)iy1 * Wp;
                const double g00 = (double)r0[ix], g01 = (double)r0[ix1];
                const double g10 = (double)r1[ix], g11 = (double)r1[ix1];
                const double top = fma(ax, g01 - g00, g00);
                const double bot = fma(ax, g11 - g10, g10);
                const double b = fma(ay, bot - top, top);
                Sb += b;
                Sbb = fma(b, b, Sbb);
                Sab = fma(sm.a, b, Sab);
            }
            const double Db = fma((double)N, Sbb, -(Sb * Sb));
            if (ok && Db > 0.0) ncc = fma((double)N, Sab, -(Sa * Sb)) / sqrt(Da * Db) * scale;
        }
        const bool pass = ncc > a.min_ncc;
        const uint64_t m = __ballot(pass);
        if (lane == 0) mask[g0 >> 6] = m;
        count += __popcll(m);
        sum += wave_sum(pass ? ncc : 0.0);
        if (ncc_out && v < V) ncc_out[v] = ncc;
    }
    if (lane == 0) {
        a.count[cand] = count;
        if (a.avg) a.avg[cand] = count ? sum / (double)count : 0.0;
    }
}

}  // namespace

extern "C" int mvs_launch_score_warp(const SceneDev* sc, const WarpArgs* a, int wid, hipStream_t s) {
    if (a->n <= 0) return 0;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    return dispatch_wid(wid, -1, [&](auto w) {
        hipLaunchKernelGGL(k_score_warp<decltype(w)::value>, grid, block, 0, s, *sc, *a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}
