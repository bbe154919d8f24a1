// One sweep of the per-pixel plane propagation on depth and normal maps
// (mvs_wprop_sweep, include/mvs_amd.h): every pixel of a view scores its own
// plane, the planes of four neighbours `step` pixels away extended to it, and a
// small depth x normal grid around its own plane against the plane-warped photo
// test over the view's short list, and takes the best.  Jacobi style: one set
// of maps is read, another written.  No reference counterpart.
//
// k_wprop_sweep: one launch per view of the range (the view, its list and the
// scalars are kernel arguments: no table in memory, no context state).  A wave
// owns 16 consecutive pixels of the view, four waves per workgroup.
//   A. lane = (pixel, source): the border ring and whether the pixel or one of
//      its four neighbours holds a plane -- a few map loads.  The pixels that
//      fail (the background and everything away from the frontier) get their
//      empty outputs by coalesced stores and cost nothing more: no LDS write,
//      no camera load.  A wave with no pixel left ends here.
//   B. the wave walks its remaining pixels one at a time, as k_refine_warp
//      walks a candidate: lane = sample sums the window (a constant window
//      leaves before any LDS write), then the window's rays and gray values go
//      to the wave's own LDS rows; lane = (hypothesis, list view) in segments
//      of S = the next power of two >= |T| lanes, 64 / S hypotheses per pass.
//      A lane keeps its view's camera and base = Rp_u O_v + t_u for the whole
//      wave (the list is the launch's).  Per pass it forms its hypothesis
//      (z_h, n_h), the facing tests, and walks the N samples in k_refine_warp's
//      homogeneous form.  The top_k largest passing ncc of a segment are
//      brought into rank order by one ds_permute and summed in that order on
//      every lane of the segment; the arg-max runs across passes in registers,
//      then across segments by a fixed butterfly.  Lane 0 writes the pixel.
// A wave keeps to its own LDS rows: no workgroup barrier, no scratch buffer in
// memory, no atomics.  Binary64 throughout on s = g - 128; compiled with
// -ffp-contract=off (fused products are the ones written as fma()).
#include "mvs_planes.h"

namespace {

struct RaySample {
    double dx, dy, dz;   // ray direction of the window pixel (world frame, camera z = 1)
    double a;            // the view's gray value - 128
};

constexpr int kPix = 16;   // pixels per wave

DEV bool holds(double z, double n0, double n1, double n2) {
    return z > 0.0 && z < __builtin_inf() && n0 == n0 && n1 == n1 && n2 == n2;
}

// What the hypotheses of one pixel are built from (wave-uniform).
struct PixelFrame {
    int qx, qy;
    double O[3], dq[3];
    double z0, n0[3], dz;
    bool own;
};

// Hypothesis h of the pixel: false when it does not exist.  h may differ from
// lane to lane; the same h gives the same bits on every lane.
DEV bool plane_of(const SceneDev& sc, const WpropArgs& a, const CamDev& cv, const PixelFrame& f, const GridFrame& g,
                  int h, int gc, double& zh, double* nh) {
    if (h == 0) {
        zh = f.z0;
#pragma unroll
        for (int m = 0; m < 3; ++m) nh[m] = f.n0[m];
        return f.own;
    }
    if (h < 5) {
        const int nx = f.qx + (h == 1 ? -a.step : h == 2 ? a.step : 0);
        const int ny = f.qy + (h == 3 ? -a.step : h == 4 ? a.step : 0);
        if (nx < 0 || nx >= sc.W || ny < 0 || ny >= sc.H) return false;
        const int64_t at = (int64_t)ny * sc.W + nx;
        const double zn = a.zmap[at];
#pragma unroll
        for (int m = 0; m < 3; ++m) nh[m] = a.nmap[3 * at + m];
        if (!holds(zn, nh[0], nh[1], nh[2])) return false;
        double dn[3];
        pixel_ray(cv, nx, ny, dn);
        const double num = zn * (nh[0] * dn[0] + nh[1] * dn[1] + nh[2] * dn[2]);
        const double den = nh[0] * f.dq[0] + nh[1] * f.dq[1] + nh[2] * f.dq[2];
        if (den == 0.0) return false;
        zh = num / den;
        return zh > 0.0 && zh < __builtin_inf();
    }
    const int hg = h - 5;
    if (!f.own || hg == gc) return false;
    const int A = 2 * a.ka + 1;
    const int k = hg / (A * A) - a.kd;
    zh = f.z0 + ((double)k * f.dz) * a.step_scale;
    double ck[3];
    hypothesis(g, hg, ck, nh);
    return true;
}

template <int WID>
__global__ __launch_bounds__(256) void k_wprop_sweep(const SceneDev sc, const WpropArgs a) {
    constexpr int SW = 2 * WID + 1, N = SW * SW;
    __shared__ RaySample smp[4][N];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int W = sc.W, H = sc.H;
    const int64_t HW = (int64_t)H * W;
    const int64_t q0 = ((int64_t)blockIdx.x * 4 + wave) * kPix;
    if (q0 >= HW) return;   // no workgroup barrier below: a wave works on its own LDS rows
    const int A = 2 * a.ka + 1, G = (2 * a.kd + 1) * A * A, HY = 5 + G, gc = (G - 1) >> 1;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const int npx = (int)(HW - q0 < kPix ? HW - q0 : kPix);

    // ---- A. lane = (pixel p, source): which pixels have anything to score ----
    uint32_t act;
    {
        const int p = lane & (kPix - 1), src = lane >> 4;
        const int64_t q = q0 + p;
        const bool inb = p < npx;
        int qy = 0, qx = 0;
        if (inb) {
            qy = (int)(q / W);
            qx = (int)(q - (int64_t)qy * W);
        }
        const bool ring = inb && qx - WID >= 0 && qx + WID <= W - 1 && qy - WID >= 0 && qy + WID <= H - 1;
        const int nx = qx + (src == 0 ? -a.step : src == 1 ? a.step : 0);
        const int ny = qy + (src == 2 ? -a.step : src == 3 ? a.step : 0);
        bool e = false;
        if (ring && nx >= 0 && nx < W && ny >= 0 && ny < H) {
            const int64_t at = (int64_t)ny * W + nx;
            e = holds(a.zmap[at], a.nmap[3 * at], a.nmap[3 * at + 1], a.nmap[3 * at + 2]);
        }
        if (ring && src == 0 && !e) e = holds(a.zmap[q], a.nmap[3 * q], a.nmap[3 * q + 1], a.nmap[3 * q + 2]);
        const uint64_t m = __ballot(e);
        act = (uint32_t)((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffu);
    }
    {
        const uint32_t idle = ((1u << npx) - 1u) & ~act;
        if (idle) {   // (uniform)
            if (lane < kPix && ((idle >> lane) & 1)) {
                a.z_out[q0 + lane] = inf;
                a.score[q0 + lane] = nan;
                a.best[q0 + lane] = -1;
            }
            if (lane < 3 * kPix && ((idle >> (lane / 3)) & 1)) a.n_out[3 * q0 + lane] = nan;
            if (a.scores)
                for (int i = lane; i < npx * HY; i += 64)
                    if ((idle >> (i / HY)) & 1) a.scores[q0 * HY + i] = nan;
        }
    }
    if (act == 0) return;

    // ---- per wave: the view's camera, the lane's list view ----
    const CamDev& cv = sc.cams[a.v];
    const int T = a.T;
    int S = 1;
    while (S < T) S <<= 1;
    S = __builtin_amdgcn_readfirstlane(S);
    const int HP = 64 / S;
    const int j = lane & (S - 1), seg0 = lane & ~(S - 1), seg = seg0 / S;
    const bool has_view = j < T;
    int u = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) u = j == k ? a.views[k] : u;   // selects: no lane-indexed argument array
    PixelFrame f = {};
    centre(cv, f.O);
    double Rp[9], base[3], Ou[3] = {0, 0, 0}, fx = 0, fy = 0, cx = 0, cy = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rp[k] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = 0;
    const int8_t* gvu = (const int8_t*)sc.gv;
    if (has_view) {
        const CamDev& cu = sc.cams[u];
        double t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rp[k] = cu.Rp[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = cu.t[k];
        fx = cu.fx; fy = cu.fy; cx = cu.cx; cy = cu.cy;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Ou[k] = -(Rp[k] * t[0] + Rp[3 + k] * t[1] + Rp[6 + k] * t[2]);
            base[k] = fma(Rp[3 * k], f.O[0], fma(Rp[3 * k + 1], f.O[1], fma(Rp[3 * k + 2], f.O[2], t[k])));
        }
        gvu += (int64_t)u * H * sc.Wp;
    }
    const int8_t* const gr = (const int8_t*)sc.gv + (int64_t)a.v * H * sc.Wp;
    const double Wm1 = (double)(W - 1), Hm1 = (double)(H - 1);
    const int Wp = sc.Wp, W1 = W - 1, H1 = H - 1;
    const double scale = (double)N / (double)(N - 1);
    const int top_k = a.top_k;
    const double Kn = (double)top_k;
    GridFrame g = {};
    g.step_scale = a.step_scale;
#pragma unroll
    for (int k = 0; k < 5; ++k) g.tans[k] = a.tans[k];
    g.kd = a.kd;
    g.ka = a.ka;
    g.dstep = 0.0;

    // ---- B. the wave's pixels, one at a time ----
    for (uint32_t rem = act; rem; rem &= rem - 1) {
        const int64_t q = q0 + __builtin_ctz(rem);
        f.qy = (int)(q / W);
        f.qx = (int)(q - (int64_t)f.qy * W);
        // lane = sample: the window's sums (inside the image: the ring test above)
        int gq[(N + 63) / 64];
        int sa = 0, saa = 0;
#pragma unroll
        for (int r = 0; r < (N + 63) / 64; ++r) {
            const int i = lane + 64 * r;
            gq[r] = 0;
            if (i < N) gq[r] = gr[(int64_t)(f.qy + i / SW - WID) * Wp + f.qx + i % SW - WID];
            sa += gq[r];
            saa += gq[r] * gq[r];
        }
        sa = wave_sum(sa);
        saa = wave_sum(saa);
        const double Sa = (double)sa;
        const double Da = (double)(N * saa - sa * sa);   // exact: |.| < 2^31 at N <= 121, |g| <= 128
        double cs = nan, bs = -inf;   // the own plane's score, the best score among the others
        int bh = -1;
        if (Da > 0.0) {
            pixel_ray(cv, f.qx, f.qy, f.dq);
#pragma unroll
            for (int r = 0; r < (N + 63) / 64; ++r) {
                const int i = lane + 64 * r;
                if (i < N) {
                    double d[3];
                    pixel_ray(cv, f.qx + i % SW - WID, f.qy + i / SW - WID, d);
                    RaySample sm;
                    sm.dx = d[0];
                    sm.dy = d[1];
                    sm.dz = d[2];
                    sm.a = (double)gq[r];
                    smp[wave][i] = sm;
                }
            }
            wave_lds_publish();
            f.z0 = a.zmap[q];
#pragma unroll
            for (int m = 0; m < 3; ++m) f.n0[m] = a.nmap[3 * q + m];
            f.own = holds(f.z0, f.n0[0], f.n0[1], f.n0[2]);
            f.dz = (a.depth_px * f.z0) / ((cv.fx + cv.fy) / 2);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                g.nrm[m] = f.n0[m];
                g.c[m] = f.O[m] + f.z0 * f.dq[m];
            }
            if (f.own && G > 1) grid_frame(g, f.O);

            for (int h0 = 0; h0 < HY; h0 += HP) {
                const int h = h0 + seg;
                const bool act_h = h < HY;
                double zh = 0.0, hn[3] = {0, 0, 0};
                bool facing = false;
                double ncc = nan;
                if (act_h && plane_of(sc, a, cv, f, g, h, gc, zh, hn)) {
                    double X[3];
#pragma unroll
                    for (int m = 0; m < 3; ++m) X[m] = f.O[m] + zh * f.dq[m];
                    const double er[3] = {f.O[0] - X[0], f.O[1] - X[1], f.O[2] - X[2]};
                    const double ner = hn[0] * er[0] + hn[1] * er[1] + hn[2] * er[2];
                    facing = ner > a.min_cos * sqrt(er[0] * er[0] + er[1] * er[1] + er[2] * er[2]);
                    const double ev[3] = {Ou[0] - X[0], Ou[1] - X[1], Ou[2] - X[2]};
                    const double nev = hn[0] * ev[0] + hn[1] * ev[1] + hn[2] * ev[2];
                    if (facing && has_view &&
                        nev > a.min_cos * sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2])) {
                        const double hh = -ner;   // n . (X_h - O_v)
                        bool ok = true;
                        double Sb = 0, Sbb = 0, Sab = 0;
                        for (int i = 0; i < N; ++i) {
                            const RaySample sm = smp[wave][i];
                            const double nd = fma(hn[0], sm.dx, fma(hn[1], sm.dy, hn[2] * sm.dz));
                            const double px = fma(Rp[0], sm.dx, fma(Rp[1], sm.dy, Rp[2] * sm.dz));
                            const double py = fma(Rp[3], sm.dx, fma(Rp[4], sm.dy, Rp[5] * sm.dz));
                            const double pz = fma(Rp[6], sm.dx, fma(Rp[7], sm.dy, Rp[8] * sm.dz));
                            // P (n.d): depth z = zs / nd
                            const double xs = fma(base[0], nd, hh * px);
                            const double ys = fma(base[1], nd, hh * py);
                            const double zs = fma(base[2], nd, hh * pz);
                            const double rz = recip(zs);
                            const double sx = fma(xs * rz, fx, cx), sy = fma(ys * rz, fy, cy);
                            ok = ok && ((zs > 0.0 && nd > 0.0) || (zs < 0.0 && nd < 0.0)) && sx >= 0.0 && sx <= Wm1 &&
                                 sy >= 0.0 && sy <= Hm1;
                            // a sample outside the image has failed its view already:
                            // its addresses are held inside the image all the same
                            const double sxc = fmin(fmax(sx, 0.0), Wm1), syc = fmin(fmax(sy, 0.0), Hm1);
                            const int ix = min(max((int)sxc, 0), W1), iy = min(max((int)syc, 0), H1);
                            const double ax = sxc - (double)ix, ay = syc - (double)iy;
                            const int ix1 = min(ix + 1, W1), iy1 = min(iy + 1, H1);
                            const int8_t* r0 = gvu + (int64_t)iy * Wp;
                            const int8_t* r1 = gvu + (int64_t)iy1 * Wp;
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
                }
                // the segment's passing ncc in rank order: descending, equal values in list order
                const bool pass = ncc > a.min_ncc;
                const double key = pass ? ncc : -inf;
                int rank = 0;
                for (int k = 0; k < S; ++k) {
                    const double ku = __shfl(key, seg0 + k, 64);
                    rank += (ku > key || (ku == key && k < j)) ? 1 : 0;
                }
                const int to = 4 * (seg0 + rank);   // a permutation of the segment's lanes
                const int lo = __builtin_amdgcn_ds_permute(to, __double2loint(key));
                const int hi = __builtin_amdgcn_ds_permute(to, __double2hiint(key));
                const double sorted = __hiloint2double(hi, lo);
                double sum = T >= top_k ? 0.0 : -inf;   // a list shorter than top_k: nothing is valid
                for (int k = 0; k < top_k && k < S; ++k) sum += __shfl(sorted, seg0 + k, 64);   // -inf when fewer than top_k pass
                const double score = (facing && sum > -inf) ? sum / Kn : nan;
                if (act_h) {
                    if (a.scores && j == 0) a.scores[q * HY + h] = score;
                    if (h == 0) cs = score;
                    else if (score > bs) { bs = score; bh = h; }   // strictly: the lowest index of a tie stays
                }
            }
            // across segments: highest score, lowest index on ties (-1 = none, the largest unsigned)
            for (int off = S; off < 64; off <<= 1) {
                const double os = __shfl_xor(bs, off, 64);
                const int oh = __shfl_xor(bh, off, 64);
                if (os > bs || (os == bs && (unsigned)oh < (unsigned)bh)) { bs = os; bh = oh; }
            }
            cs = __shfl(cs, 0, 64);
        } else if (a.scores) {
            for (int h = lane; h < HY; h += 64) a.scores[q * HY + h] = nan;
        }
        int best = -1;
        double sbest = nan;
        if (cs == cs && !(bh >= 0 && bs > cs)) { best = 0; sbest = cs; }
        else if (bh >= 0) { best = bh; sbest = bs; }
        double zo = inf, no[3] = {nan, nan, nan};
        if (best >= 0) (void)plane_of(sc, a, cv, f, g, best, gc, zo, no);
        if (lane == 0) {
            a.best[q] = best;
            a.score[q] = sbest;
            a.z_out[q] = zo;
#pragma unroll
            for (int m = 0; m < 3; ++m) a.n_out[3 * q + m] = no[m];
        }
        wave_lds_publish();   // the rows are rewritten by the next pixel
    }
}

}  // namespace

extern "C" int mvs_launch_wprop_sweep(const SceneDev* sc, const WpropArgs* a, int wid, hipStream_t s) {
    const int64_t hw = (int64_t)sc->H * sc->W;
    if (hw <= 0) return 0;
    const int64_t waves = (hw + kPix - 1) / kPix;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    return dispatch_wid(wid, -1, [&](auto w) {
        hipLaunchKernelGGL(k_wprop_sweep<decltype(w)::value>, grid, block, 0, s, *sc, *a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}
