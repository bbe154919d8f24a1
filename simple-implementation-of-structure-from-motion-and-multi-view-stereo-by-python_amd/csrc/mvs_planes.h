// Plane geometry shared by the warped family's units: a camera's centre and
// the ray of an integer pixel (k_wdepth_*, k_wprop_*), and the hypothesis grid
// of the depth and normal refinement (k_refine_warp, k_wprop_sweep).  Binary64,
// left to right, unfused (-ffp-contract=off).
#pragma once
#include "mvs_device.h"

namespace {

// O = -Rp^T t, each component a left-to-right sum of three products (k_wexp_children's)
DEV void centre(const CamDev& cv, double* O) {
#pragma unroll
    for (int k = 0; k < 3; ++k) O[k] = -(cv.Rp[k] * cv.t[0] + cv.Rp[3 + k] * cv.t[1] + cv.Rp[6 + k] * cv.t[2]);
}

// d = Rp^T ((qx - cx) / fx, (qy - cy) / fy, 1): the ray of the integer pixel q, camera z = 1
DEV void pixel_ray(const CamDev& cv, int qx, int qy, double* d) {
    const double u = ((double)qx - cv.cx) / cv.fx;
    const double w = ((double)qy - cv.cy) / cv.fy;
#pragma unroll
    for (int m = 0; m < 3; ++m) d[m] = cv.Rp[m] * u + cv.Rp[3 + m] * w + cv.Rp[6 + m];
}

// The candidate's frame of the grid: u along the reference ray, e1 and e2 the
// tangent basis of the definition.
struct GridFrame {
    double c[3], nrm[3], u[3], e1[3], e2[3];
    double dstep, step_scale;
    double tans[5];
    int kd, ka;
};

DEV void grid_frame(GridFrame& g, const double* Or) {
    const double e[3] = {g.c[0] - Or[0], g.c[1] - Or[1], g.c[2] - Or[2]};
    const double len = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) g.u[k] = e[k] / len;
    const double ax = fabs(g.nrm[0]), ay = fabs(g.nrm[1]), az = fabs(g.nrm[2]);
    const int m = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);   // smallest |nrm_m|, lowest index on ties
    // nrm x axis_m
    double v[3];
    v[0] = m == 1 ? -g.nrm[2] : m == 2 ? g.nrm[1] : 0.0;
    v[1] = m == 0 ? g.nrm[2] : m == 2 ? -g.nrm[0] : 0.0;
    v[2] = m == 0 ? -g.nrm[1] : m == 1 ? g.nrm[0] : 0.0;
    const double vl = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) g.e1[k] = v[k] / vl;
    g.e2[0] = g.nrm[1] * g.e1[2] - g.nrm[2] * g.e1[1];
    g.e2[1] = g.nrm[2] * g.e1[0] - g.nrm[0] * g.e1[2];
    g.e2[2] = g.nrm[0] * g.e1[1] - g.nrm[1] * g.e1[0];
}

// Hypothesis h = ((k + kd) A + (j + ka)) A + (i + ka): centre c_k, normal n_ij.
DEV void hypothesis(const GridFrame& g, int h, double* ck, double* n) {
    const int A = 2 * g.ka + 1;
    const int ii = h % A, jj = (h / A) % A;
    const int k = h / (A * A) - g.kd;
    const double sd = ((double)k * g.dstep) * g.step_scale;
#pragma unroll
    for (int m = 0; m < 3; ++m) ck[m] = g.c[m] + sd * g.u[m];
    if (ii == g.ka && jj == g.ka) {
        // the unperturbed normal is the input, as given
#pragma unroll
        for (int m = 0; m < 3; ++m) n[m] = g.nrm[m];
        return;
    }
    double ti = g.tans[0], tj = g.tans[0];
#pragma unroll
    for (int m = 1; m < 5; ++m) {   // selects: a lane-indexed array would live in scratch
        ti = ii == m ? g.tans[m] : ti;
        tj = jj == m ? g.tans[m] : tj;
    }
    double w[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) w[m] = g.nrm[m] + ti * g.e1[m] + tj * g.e2[m];
    const double wl = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int m = 0; m < 3; ++m) n[m] = w[m] / wl;
}

}  // namespace
