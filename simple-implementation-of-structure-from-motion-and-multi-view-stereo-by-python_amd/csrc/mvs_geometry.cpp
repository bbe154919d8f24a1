// Host geometry of libmvs_amd.so: the OpenCV 4.x algorithms the reference
// calls through cv2 (utils.py:234-254), and the C-ABI calls that are geometry
// alone.  Compiled with -ffp-contract=off: the Jacobi SVD, the triangulation
// and the projections follow OpenCV's / numpy's operation order.
#include <cfloat>
#include <cmath>

#include "mvs_host.h"

// cv::JacobiSVDImpl_<double>: one-sided Jacobi on the n rows (length m) of At.
static void jacobi_svd(double* At, double* Wout, double* Vt, int m, int n) {
    double W[16];
    const double eps = DBL_EPSILON * 10, minval = DBL_MIN;
    const int max_iter = std::max(m, 30);
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const double t = At[i * m + k];
            sd += t * t;
        }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double* Ai = At + i * m;
                double* Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = std::hypot(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = std::sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = std::sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                double* Vi = Vt + i * n;
                double* Vj = Vt + j * n;
                for (int k = 0; k < n; k++) {
                    const double t0 = c * Vi[k] + s * Vj[k];
                    const double t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const double t = At[i * m + k];
            sd += t * t;
        }
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (int k = 0; k < m; k++) std::swap(At[i * m + k], At[j * m + k]);
            for (int k = 0; k < n; k++) std::swap(Vt[i * n + k], Vt[j * n + k]);
        }
    }
    for (int i = 0; i < n; i++) Wout[i] = W[i];
    for (int i = 0; i < n; i++) {
        const double s = W[i] > minval ? 1 / W[i] : 0.;
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// cvRodrigues2 3x3 -> 3x1 then 3x1 -> 3x3 (projectPoint, utils.py:242-243).
void rodrigues_roundtrip(const double* Rin, double* Rout) {
    double At[9], W[3], Vt[9], U[9], R[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) At[i * 3 + j] = Rin[j * 3 + i];
    jacobi_svd(At, W, Vt, 3, 3);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) U[i * 3 + j] = At[j * 3 + i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += U[i * 3 + k] * Vt[k * 3 + j];
            R[i * 3 + j] = s;
        }
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = std::acos(c);
    if (s < 1e-5) {
        if (c > 0) {
            rx = ry = rz = 0;
        } else {
            double t = (R[0] + 1) * 0.5;
            rx = std::sqrt(std::max(t, 0.));
            t = (R[4] + 1) * 0.5;
            ry = std::sqrt(std::max(t, 0.)) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5;
            rz = std::sqrt(std::max(t, 0.)) * (R[2] < 0 ? -1. : 1.);
            if (std::fabs(rx) < std::fabs(ry) && std::fabs(rx) < std::fabs(rz) &&
                (R[5] > 0) != (ry * rz > 0))
                rz = -rz;
            theta /= std::sqrt(rx * rx + ry * ry + rz * rz);
            rx *= theta;
            ry *= theta;
            rz *= theta;
        }
    } else {
        double vth = 1 / (2 * s);
        vth *= theta;
        rx *= vth;
        ry *= vth;
        rz *= vth;
    }
    // 3x1 -> 3x3
    const double th = std::sqrt(rx * rx + ry * ry + rz * rz);
    if (th < DBL_EPSILON) {
        for (int i = 0; i < 9; i++) Rout[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    // glibc sincos(): the gcc -O2 lowering of OpenCV's adjacent cos/sin calls
    double ss, cc;
    ::sincos(th, &ss, &cc);
    const double c1 = 1. - cc;
    const double ith = th ? 1. / th : 0.;
    rx *= ith;
    ry *= ith;
    rz *= ith;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int i = 0; i < 9; i++) {
        const double e = (i % 4 == 0) ? 1.0 : 0.0;
        Rout[i] = (cc * e + c1 * rrt[i]) + ss * r_x[i];
    }
}

// cvTriangulatePoints for one correspondence (utils.py:238-239).
void triangulate(const double* P1, const double* P2, const double* x1, const double* x2, double* X4) {
    double A[16];
    const double* P[2] = {P1, P2};
    const double* pt[2] = {x1, x2};
    for (int j = 0; j < 2; j++) {
        const double x = pt[j][0], y = pt[j][1];
        for (int k = 0; k < 4; k++) {
            A[(j * 2 + 0) * 4 + k] = x * P[j][8 + k] - P[j][0 + k];
            A[(j * 2 + 1) * 4 + k] = y * P[j][8 + k] - P[j][4 + k];
        }
    }
    double At[16], W[4], Vt[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) At[i * 4 + j] = A[j * 4 + i];
    jacobi_svd(At, W, Vt, 4, 4);
    for (int k = 0; k < 4; k++) X4[k] = Vt[12 + k];
}

// cv2.projectPoints of one point, no distortion (cvProjectPoints2Internal
// order; the device project() in mvs_kernels.hip is the same expression)
static void project_host(const double* K, const double* Rp, const double* t, const double* M, double* out) {
    double x = Rp[0] * M[0] + Rp[1] * M[1] + Rp[2] * M[2] + t[0];
    double y = Rp[3] * M[0] + Rp[4] * M[1] + Rp[5] * M[2] + t[1];
    double z = Rp[6] * M[0] + Rp[7] * M[1] + Rp[8] * M[2] + t[2];
    z = z != 0.0 ? 1.0 / z : 1.0;
    x *= z;
    y *= z;
    out[0] = x * K[0] + K[2];
    out[1] = y * K[4] + K[5];
}

// getProjectionMatrix(K, R, t) = K @ [R | t] (utils.py:234-236) as OpenBLAS
// evaluates the 3x3 by 3x4 product: an FMA chain per entry
static void projection_matrix(const double* K, const double* R, const double* t, double* P) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const double e0 = c < 3 ? R[c] : t[0], e1 = c < 3 ? R[3 + c] : t[1],
                         e2 = c < 3 ? R[6 + c] : t[2];
            P[4 * r + c] = fma_dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], e0, e1, e2);
        }
}

extern "C" {

int mvs_rodrigues_roundtrip(const double* R, double* Rp) {
    if (!R || !Rp) return MVS_E_ARG;
    rodrigues_roundtrip(R, Rp);
    return 0;
}

int mvs_triangulate(const double* P1, const double* P2, const double* x1, const double* x2, double* X4) {
    if (!P1 || !P2 || !x1 || !x2 || !X4) return MVS_E_ARG;
    triangulate(P1, P2, x1, x2, X4);
    return 0;
}

int mvs_sfm_pair(const double* KA, const double* RA, const double* tA, const double* KB,
                 const double* RB, const double* tB, int64_t n, const float* q, const float* tr,
                 double max_err, float* pt, uint8_t* keep) {
    if (!KA || !RA || !tA || !KB || !RB || !tB || n < 0 || (n && (!q || !tr || !pt || !keep)))
        return set_err(nullptr, Fail{MVS_E_ARG, "null argument"});
    double P1[12], P2[12], RpA[9], RpB[9];
    projection_matrix(KA, RA, tA, P1);
    projection_matrix(KB, RB, tB, P2);
    rodrigues_roundtrip(RA, RpA);
    rodrigues_roundtrip(RB, RpB);
    for (int64_t i = 0; i < n; ++i) {
        // cv2.triangulatePoints on float32 points: double DLT, float32 result
        const double x1[2] = {q[2 * i], q[2 * i + 1]}, x2[2] = {tr[2 * i], tr[2 * i + 1]};
        double X4[4];
        triangulate(P1, P2, x1, x2, X4);
        const float w = (float)X4[3];
        keep[i] = 0;
        pt[3 * i] = pt[3 * i + 1] = pt[3 * i + 2] = 0.f;
        if (w == 0.f) continue;                    // SFM.py:69-72: not added
        float p[3];
        for (int k = 0; k < 3; ++k) p[k] = (float)X4[k] / w;
        for (int k = 0; k < 3; ++k) pt[3 * i + k] = p[k];
        // projectPoint on the float32 point: double projection, float32 result;
        // np.linalg.norm of the float32 residual (SFM.py:75-78)
        const double M[3] = {p[0], p[1], p[2]};
        double oa[2], ob[2];
        project_host(KA, RpA, tA, M, oa);
        project_host(KB, RpB, tB, M, ob);
        const float ra0 = (float)oa[0] - q[2 * i], ra1 = (float)oa[1] - q[2 * i + 1];
        const float rb0 = (float)ob[0] - tr[2 * i], rb1 = (float)ob[1] - tr[2 * i + 1];
        const float ea = std::sqrt(ra0 * ra0 + ra1 * ra1), eb = std::sqrt(rb0 * rb0 + rb1 * rb1);
        keep[i] = ((double)ea > max_err || (double)eb > max_err) ? 0 : 1;
    }
    return 0;
}

}  // extern "C"
