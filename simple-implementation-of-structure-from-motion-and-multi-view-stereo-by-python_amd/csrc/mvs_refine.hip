// One level of the fixed-grid depth and normal refinement of a patch against
// the plane-warped photo test (mvs_refine_warped, include/mvs_amd.h): H plane
// hypotheses (2 kd + 1 depths along the reference ray x (2 ka + 1)^2 normals)
// of one patch are scored against the patch's own short view list, and the
// best one is chosen.  No reference counterpart (the reference never refines).
//
// k_refine_warp: one wave per candidate, four candidates per workgroup.
//   1. the wave tests the candidate and its list as k_score_warp does;
//   2. lane = sample: the ray direction d = Rp_r^T((q.x-cx)/fx, (q.y-cy)/fy, 1)
//      of every window pixel and the pixel's gray value go to LDS, 32 B per
//      sample -- one ray set per candidate, whatever the hypothesis; sum a and
//      D_a by a wave reduction of exact integers;
//   3. lane = (hypothesis, list view), hypothesis-major: segments of S = the
//      next power of two >= |T| lanes, 64 / S hypotheses per pass.  A lane
//      keeps its view's camera for the whole kernel and, per pass, its
//      hypothesis's normal n and n.(c_k - O_r); it walks the N samples (LDS
//      broadcasts) and keeps sum b, sum b^2, sum a b to itself.  A sample is
//      projected in homogeneous form, without forming the plane point:
//        P (n.d) = (Rp_v O_r + t_v)(n.d) + (n.(c_k - O_r)) (Rp_v d),
//      so the only reciprocal per sample is the one of the depth;
//   4. the score of a hypothesis is the sum of its segment's ncc in list order
//      (shuffles from the segment's first |T| lanes, the same order on every
//      lane) over |T|; the arg-max runs across passes in registers, then
//      across segments by a fixed butterfly.  Lane 0 writes the outputs.
// A wave keeps to its own LDS rows: no workgroup barrier, no scratch buffer
// in memory, no atomics.  Binary64 throughout on s = g - 128; compiled with
// -ffp-contract=off (fused products are the ones written as fma()).
//
// k_refine_lists: what the level kernel is fed, built on the device
// (mvs_refine_lists, include/mvs_amd.h): per row the view list -- the
// max_views best passing views of a row of k_score_warp's ncc, ties to the
// lower view, in ascending view order -- and the depth step.  One wave per
// row, four rows per workgroup, lane = view: a row's 8 V bytes are one
// coalesced load, at V > 64 a lane holds one key per group of 64 views (G of
// them, in registers).  A key's rank is counted in a loop over the passing
// keys (the set bits of their ballot: a handful per scored row), each
// broadcast from its lane (v_readlane, the lane index is uniform); the
// output slot of a selected view is the number of selected lower views (a
// ballot and mbcnt per group, plus the lower groups' popcounts): ascending
// order with no sort.  Lane 0 computes the depth step from the camera table.
// No LDS, no atomics, no scratch: a memory stream of n (8 V + 4 max_views + 44)
// bytes.
#include "mvs_planes.h"

namespace {

struct RaySample {
    double dx, dy, dz;   // ray direction of the window pixel (world frame, not normalised)
    double a;            // reference gray value - 128
};

template <int WID>
__global__ __launch_bounds__(256) void k_refine_warp(const SceneDev sc, const RefineArgs a) {
    constexpr int SW = 2 * WID + 1, N = SW * SW;
    __shared__ RaySample smp[4][N];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t cand = (int64_t)blockIdx.x * 4 + wave;
    if (cand >= a.n) return;   // no workgroup barrier below: a wave works on its own LDS rows
    const int V = sc.V, tv = a.tv;
    const int A = 2 * a.ka + 1, H = (2 * a.kd + 1) * A * A, hc = (H - 1) >> 1;
    const double nan = __builtin_nan("");

    const int R = __builtin_amdgcn_readfirstlane(a.ref[cand]);
    GridFrame g;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.c[k] = a.c[3 * cand + k]; g.nrm[k] = a.nrm[3 * cand + k]; }
    g.dstep = a.dstep[cand];
    g.step_scale = a.step_scale;
#pragma unroll
    for (int k = 0; k < 5; ++k) g.tans[k] = a.tans[k];
    g.kd = a.kd;
    g.ka = a.ka;
    const double* const c = g.c;
    const double* const n0 = g.nrm;

    // the view list: lane l < tv holds entry l
    const int myv = lane < tv ? a.views[cand * tv + lane] : -1;
    const uint64_t present = __ballot(myv >= 0);
    const int T = __builtin_amdgcn_readfirstlane(__popcll(present));
    bool bad = lane < tv && (myv < -1 || myv >= V || myv == R);
    for (int j = 0; j < T; ++j) {
        const int vj = __shfl(myv, j, 64);
        bad = bad || (lane > j && lane < T && myv == vj);
    }
    bool valid = R >= 0 && R < V && T >= 1 && present == ((1ull << T) - 1) && __ballot(bad) == 0 &&
                 g.dstep > 0.0;

    double Or[3] = {0, 0, 0};
    int x0 = 0, y0 = 0;
    if (valid) {
        const CamDev& cr = sc.cams[R];
        double px, py;
        project(cr, c, px, py);
        const double z = cr.Rp[6] * c[0] + cr.Rp[7] * c[1] + cr.Rp[8] * c[2] + cr.t[2];
        valid = z > 0.0 && px >= 0.0 && py >= 0.0 && py_trunc(px, &x0) && py_trunc(py, &y0);
        valid = valid && x0 - WID >= 0 && x0 + WID <= sc.W - 1 && y0 - WID >= 0 && y0 + WID <= sc.H - 1;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Or[k] = -(cr.Rp[k] * cr.t[0] + cr.Rp[3 + k] * cr.t[1] + cr.Rp[6 + k] * cr.t[2]);
        const double e[3] = {Or[0] - c[0], Or[1] - c[1], Or[2] - c[2]};
        const double ne = n0[0] * e[0] + n0[1] * e[1] + n0[2] * e[2];
        valid = valid && ne > a.min_cos * sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    }

    double Sa = 0, Da = 0;
    if (valid) {
        // lane = sample: ray directions and reference pixels into LDS
        const CamDev& cr = sc.cams[R];
        const int8_t* gr = (const int8_t*)sc.gv + (int64_t)R * sc.H * sc.Wp;
        int sa = 0, saa = 0;
        for (int i = lane; i < N; i += 64) {
            const int dy = i / SW - WID, dx = i % SW - WID;
            const double u = ((double)(x0 + dx) - cr.cx) / cr.fx, w = ((double)(y0 + dy) - cr.cy) / cr.fy;
            const int gq = gr[(int64_t)(y0 + dy) * sc.Wp + x0 + dx];   // window inside the image (tested above)
            RaySample sm;
            sm.dx = cr.Rp[0] * u + cr.Rp[3] * w + cr.Rp[6];
            sm.dy = cr.Rp[1] * u + cr.Rp[4] * w + cr.Rp[7];
            sm.dz = cr.Rp[2] * u + cr.Rp[5] * w + cr.Rp[8];
            sm.a = (double)gq;
            smp[wave][i] = sm;
            sa += gq;
            saa += gq * gq;
        }
        sa = wave_sum(sa);
        saa = wave_sum(saa);
        Sa = (double)sa;
        Da = (double)(N * saa - sa * sa);   // exact: |.| < 2^31 at N <= 121, |g| <= 128
        valid = Da > 0.0;
    }
    if (!valid) {
        if (a.scores)
            for (int h = lane; h < H; h += 64) a.scores[cand * H + h] = nan;
        if (lane == 0) {
            a.best[cand] = -1;
            a.score_best[cand] = nan;
        }
        if (lane < 3) {
            a.c_out[3 * cand + lane] = a.c[3 * cand + lane];
            a.nrm_out[3 * cand + lane] = a.nrm[3 * cand + lane];
        }
        return;
    }
    wave_lds_publish();

    grid_frame(g, Or);

    // segments: S = next power of two >= T lanes per hypothesis
    int S = 1;
    while (S < T) S <<= 1;
    S = __builtin_amdgcn_readfirstlane(S);
    const int HP = 64 / S;
    const int j = lane & (S - 1), seg0 = lane & ~(S - 1), seg = seg0 / S;
    const bool has_view = j < T;
    const int v = __shfl(myv, j, 64);   // entry j of the list (j < T: a view in 0..V-1 other than R)

    // the lane's camera, its centre O_v and base = Rp_v O_r + t_v
    double Rp[9], base[3], Ov[3] = {0, 0, 0}, fx = 0, fy = 0, cx = 0, cy = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rp[k] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = 0;
    const int8_t* gvv = (const int8_t*)sc.gv;
    if (has_view) {
        const CamDev& cv = sc.cams[v];
        double t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rp[k] = cv.Rp[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = cv.t[k];
        fx = cv.fx; fy = cv.fy; cx = cv.cx; cy = cv.cy;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Ov[k] = -(Rp[k] * t[0] + Rp[3 + k] * t[1] + Rp[6 + k] * t[2]);
            base[k] = fma(Rp[3 * k], Or[0], fma(Rp[3 * k + 1], Or[1], fma(Rp[3 * k + 2], Or[2], t[k])));
        }
        gvv += (int64_t)v * sc.H * sc.Wp;
    }

    const double Wm1 = (double)(sc.W - 1), Hm1 = (double)(sc.H - 1);
    const int Wp = sc.Wp, W1 = sc.W - 1, H1 = sc.H - 1;
    const double scale = (double)N / (double)(N - 1);
    const double Tn = (double)T;
    double bs = -__builtin_inf(), cs = nan;   // best score among the others, the centre's score
    int bh = -1;
    for (int h0 = 0; h0 < H; h0 += HP) {
        const int h = h0 + seg;
        const bool act = h < H;
        double ncc = nan;
        if (act && has_view) {
            double ck[3], hn[3];
            hypothesis(g, h, ck, hn);
            // facing tests of the hypothesis: the reference camera, then the lane's view
            const double er[3] = {Or[0] - ck[0], Or[1] - ck[1], Or[2] - ck[2]};
            const double ner = hn[0] * er[0] + hn[1] * er[1] + hn[2] * er[2];
            const double ev[3] = {Ov[0] - ck[0], Ov[1] - ck[1], Ov[2] - ck[2]};
            const double nev = hn[0] * ev[0] + hn[1] * ev[1] + hn[2] * ev[2];
            const bool facing = ner > a.min_cos * sqrt(er[0] * er[0] + er[1] * er[1] + er[2] * er[2]) &&
                                nev > a.min_cos * sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
            if (facing) {
                const double hh = -ner;   // n . (c_k - O_r)
                bool ok = true;
                double Sb = 0, Sbb = 0, Sab = 0;
                for (int i = 0; i < N; ++i) {
                    const RaySample sm = smp[wave][i];
                    const double nd = fma(hn[0], sm.dx, fma(hn[1], sm.dy, hn[2] * sm.dz));
                    const double qx = fma(Rp[0], sm.dx, fma(Rp[1], sm.dy, Rp[2] * sm.dz));
                    const double qy = fma(Rp[3], sm.dx, fma(Rp[4], sm.dy, Rp[5] * sm.dz));
                    const double qz = fma(Rp[6], sm.dx, fma(Rp[7], sm.dy, Rp[8] * sm.dz));
                    // P (n.d): depth z = zh / nd
                    const double xh = fma(base[0], nd, hh * qx);
                    const double yh = fma(base[1], nd, hh * qy);
                    const double zh = fma(base[2], nd, hh * qz);
                    const double rz = recip(zh);
                    const double sx = fma(xh * rz, fx, cx), sy = fma(yh * rz, fy, cy);
                    ok = ok && ((zh > 0.0 && nd > 0.0) || (zh < 0.0 && nd < 0.0)) && sx >= 0.0 && sx <= Wm1 &&
                         sy >= 0.0 && sy <= Hm1;
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
        }
        // the hypothesis's score: its segment's ncc in list order, on every lane of the segment
        double sum = 0.0;
        for (int k = 0; k < T; ++k) sum += __shfl(ncc, seg0 + k, 64);
        const double score = sum / Tn;   // nan when any list view failed
        if (act) {
            if (a.scores && j == 0) a.scores[cand * H + h] = score;
            if (h == hc) cs = score;
            else if (score > bs) { bs = score; bh = h; }   // strictly: the lowest index of a tie stays
        }
    }
    // across segments: highest score, lowest index on ties (-1 = none, the largest unsigned)
    for (int off = S; off < 64; off <<= 1) {
        const double os = __shfl_xor(bs, off, 64);
        const int oh = __shfl_xor(bh, off, 64);
        if (os > bs || (os == bs && (unsigned)oh < (unsigned)bh)) { bs = os; bh = oh; }
    }
    cs = __shfl(cs, (hc % HP) * S, 64);
    int best = -1;
    double sbest = nan;
    if (cs == cs && !(bh >= 0 && bs > cs)) { best = hc; sbest = cs; }
    else if (bh >= 0) { best = bh; sbest = bs; }
    // (with no valid hypothesis every scores entry above was written as nan)
    double co[3] = {c[0], c[1], c[2]}, no[3] = {n0[0], n0[1], n0[2]};
    if (best >= 0 && best != hc) hypothesis(g, best, co, no);
    if (lane == 0) {
        a.best[cand] = best;
        a.score_best[cand] = sbest;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.c_out[3 * cand + k] = co[k];
            a.nrm_out[3 * cand + k] = no[k];
        }
    }
}

// x of lane l (wave-uniform) on every lane
DEV double lane_bcast(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

template <int G>
__global__ __launch_bounds__(256) void k_refine_lists(const SceneDev sc, const ListArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    if (k >= a.n) return;
    const int V = sc.V, mv = a.max_views;
    const double nan = __builtin_nan(""), ninf = -__builtin_inf();
    int64_t s = a.sel ? a.sel[k] : k;   // one address per wave
    s = ((int64_t)__builtin_amdgcn_readfirstlane((int)(s >> 32)) << 32) |
        (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    int32_t* const out = a.views + k * mv;
    if (s < 0 || s >= a.rows) {   // nothing of the row is read
        if (lane < mv) out[lane] = -1;
        if (lane == 0 && a.dstep) a.dstep[k] = nan;
        return;
    }
    // view v = 64 g + lane holds key[g]: its ncc when it passes, else -inf (a
    // passing ncc is above min_ncc, so above -inf: -inf never outranks or ties it)
    double key[G];
    const double* const row = a.ncc + s * V;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int v = 64 * g + lane;
        const double x = v < V ? row[v] : nan;
        key[g] = x > a.min_ncc ? x : ninf;   // nan never passes, +inf does
    }
    // rank[g] = the passing views u that go before v: key_u > key_v, or equal
    // and u < v.  Only passing views can go before a passing one, so the loop
    // walks the set bits of their ballot (a scored row passes a handful of
    // its V views, most rows none)
    int rank[G];
#pragma unroll
    for (int g = 0; g < G; ++g) rank[g] = 0;
#pragma unroll
    for (int gu = 0; gu < G; ++gu) {
        for (uint64_t pm = __ballot(key[gu] > ninf); pm; pm &= pm - 1) {
            const int l = __builtin_ctzll(pm);
            const double ku = lane_bcast(key[gu], l);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool lower = gu < g || (gu == g && l < lane);
                rank[g] += (ku > key[g] || (ku == key[g] && lower)) ? 1 : 0;
            }
        }
    }
    int total = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool chosen = key[g] > ninf && rank[g] < mv;
        const uint64_t b = __ballot(chosen);
        const int slot = total + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if (chosen) out[slot] = 64 * g + lane;   // slot < mv: at most mv views have a rank below mv
        total += __popcll(b);
    }
    if (lane >= total && lane < mv) out[lane] = -1;
    if (lane == 0 && a.dstep) {
        const int r = a.ref[s];
        double d = nan;
        if (r >= 0 && r < V) {
            const CamDev& cr = sc.cams[r];
            const double* const c = a.c + 3 * s;
            const double depth = cr.Rp[6] * c[0] + cr.Rp[7] * c[1] + cr.Rp[8] * c[2] + cr.t[2];
            d = (a.depth_px * depth) / ((cr.fx + cr.fy) / 2);
        }
        a.dstep[k] = d;
    }
}

}  // namespace

extern "C" int mvs_launch_refine_lists(const SceneDev* sc, const ListArgs* a, hipStream_t s) {
    if (a->n <= 0) return 0;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    switch ((sc->V + 63) / 64) {
        case 1: hipLaunchKernelGGL(k_refine_lists<1>, grid, block, 0, s, *sc, *a); break;
        case 2: hipLaunchKernelGGL(k_refine_lists<2>, grid, block, 0, s, *sc, *a); break;
        case 3: hipLaunchKernelGGL(k_refine_lists<3>, grid, block, 0, s, *sc, *a); break;
        case 4: hipLaunchKernelGGL(k_refine_lists<4>, grid, block, 0, s, *sc, *a); break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
static_assert(MVS_MAX_VIEWS == 256, "k_refine_lists holds at most four keys per lane");

extern "C" int mvs_launch_refine_warp(const SceneDev* sc, const RefineArgs* a, int wid, hipStream_t s) {
    if (a->n <= 0) return 0;
    const dim3 grid((unsigned)((a->n + 3) / 4)), block(256);
    return dispatch_wid(wid, -1, [&](auto w) {
        hipLaunchKernelGGL(k_refine_warp<decltype(w)::value>, grid, block, 0, s, *sc, *a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}
