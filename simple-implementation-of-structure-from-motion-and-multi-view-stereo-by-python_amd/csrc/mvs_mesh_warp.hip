// Volumetric fusion of per-view depth maps and the surface mesh of the result
// (mvs_wtsdf_integrate, mvs_wmesh_extract, include/mvs_amd.h).  No reference
// counterpart.
//
// k_wtsdf_integrate: one thread per lattice point, a workgroup owns a brick of
//   16 x 4 x 4 points with i fastest (a wave is a 16 x 4 sheet of one k), so
//   neighbouring lanes project to neighbouring pixels of a view's map.  The
//   loop over the views of the range is wave-uniform: the camera comes through
//   scalar loads, as in k_wdepth_consist.  The sums run in view order in
//   registers; no atomics, no LDS.  Bricks past the lattice's end are cut.
// k_wmesh_mark: one thread per cube.  The six Kuhn tetrahedra of the cube are
//   unrolled (their corners are compile-time constants, so the eight values
//   stay in registers); a tetrahedron's triangles come from a 16-entry table
//   of edge pairs and a winding bit per (tetrahedron, case).  The thread
//   gathers the used-edge bits of the cube's corners in one register and ORs
//   the non-empty bytes into the owner points' masks (an OR does not depend on
//   the order of arrival); the workgroup's triangle count goes to tsum.
// k_wmesh_vcount: one thread per point: the workgroup's vertex count -> vsum.
// k_wmesh_scan: two workgroups, one per array: exclusive int64 offsets in
//   place and the totals (k_wseed_scan's scheme).
// k_wmesh_vertex: one thread per point: an exclusive scan of the mask's
//   popcounts inside the workgroup gives the point's first vertex (kept in
//   voff); the vertices below cap_v are written.
// k_wmesh_tri: one thread per cube, the mark pass's arithmetic again; an
//   exclusive scan inside the workgroup gives the cube's first triangle; a
//   vertex index is voff[owner] + the rank of the edge's bit in the owner's mask.
// Binary64 in the library's operation order, compiled with -ffp-contract=off.
#include <algorithm>

#include "mvs_device.h"

namespace {

constexpr int kBX = 16, kBY = 4, kBZ = 4;
constexpr int kBlock = MVS_MESH_BLOCK;
constexpr int kScanThreads = 1024;
static_assert(kBX * kBY * kBZ == 256 && kBlock == 256, "workgroups of four waves");

DEV bool finite(double x) { return x > -__builtin_inf() && x < __builtin_inf(); }

__global__ __launch_bounds__(256) void k_wtsdf_integrate(const SceneDev sc, const WtsdfArgs a) {
    const int px = a.nx + 1, py = a.ny + 1, pz = a.nz + 1;
    const unsigned bx = (unsigned)(px + kBX - 1) / kBX, by = (unsigned)(py + kBY - 1) / kBY;
    const unsigned b = blockIdx.x, r = b / bx;
    const int tid = threadIdx.x;
    const int i = (int)(b - r * bx) * kBX + (tid & 15);
    const int j = (int)(r % by) * kBY + ((tid >> 4) & 3);
    const int k = (int)(r / by) * kBZ + (tid >> 6);
    if (i >= px || j >= py || k >= pz) return;
    const int W = sc.W, H = sc.H;
    const int64_t hw = (int64_t)H * W;
    const double P[3] = {a.origin[0] + (double)i * a.voxel, a.origin[1] + (double)j * a.voxel,
                         a.origin[2] + (double)k * a.voxel};
    double D = 0.0;
    int Wt = 0, cnt = 0;
    int sum[3] = {0, 0, 0};
    for (int ui = 0; ui < a.nv; ++ui) {
        const CamDev& cu = sc.cams[a.v0 + ui];
        double x, y;
        project(cu, P, x, y);
        const double z = cu.Rp[6] * P[0] + cu.Rp[7] * P[1] + cu.Rp[8] * P[2] + cu.t[2];
        // k_wdepth_consist's nearest pixel: nan and inf fail a comparison before the conversion
        const double xr = x + 0.5, yr = y + 0.5;
        if (!(z > 0.0 && x >= 0.0 && y >= 0.0 && xr < (double)W && yr < (double)H)) continue;
        const int64_t at = (int64_t)(int)yr * W + (int)xr;
        const double zu = a.zmap[(int64_t)ui * hw + at];
        if (!(finite(zu) && zu > 0.0)) continue;
        const double sdf = zu - z;
        if (sdf < -a.trunc) continue;   // hidden behind the surface
        const double q = sdf / a.trunc;
        D += q < 1.0 ? q : 1.0;
        ++Wt;
        if (fabs(sdf) <= a.trunc) {
            const uint8_t* c = sc.rgb + ((int64_t)(a.v0 + ui) * hw + at) * 3;
            sum[0] += c[0];
            sum[1] += c[1];
            sum[2] += c[2];
            ++cnt;
        }
    }
    const int64_t p = ((int64_t)k * py + j) * px + i;
    a.tsdf[p] = Wt >= a.min_weight ? D / (double)Wt : __builtin_nan("");
    a.weight[p] = Wt;
#pragma unroll
    for (int m = 0; m < 3; ++m) a.rgb[3 * p + m] = cnt ? (uint8_t)((2 * sum[m] + cnt) / (2 * cnt)) : (uint8_t)0;
    a.cnt[p] = (uint8_t)min(cnt, 255);
}

// ---- marching tetrahedra ----

// The Kuhn tetrahedron of the permutation tp (itertools.permutations(range(3))
// order): its corners c0..c3 as cube corners (bit m = the offset along axis m),
// a nibble each.
constexpr uint32_t kTetCorners[6] = {0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640};
// bit `case` of kFlip[tp]: the case's triangles are listed against the winding rule
constexpr uint32_t kFlip[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
// The triangles of a 4-bit inside mask: bits 24..25 the count; nibble 3 t + e
// the edge e of triangle t as p | q << 2, p < q tetrahedron corners.  One or
// three inside: the lone corner's three edges; two inside, a < b, outside c < d:
// (ac, ad, bd) and (ac, bd, bc).
__device__ const uint32_t kCaseTris[16] = {0x0,       0x1000c84, 0x1000d94, 0x29d8dc8, 0x1000e98, 0x29e4ec4,
                                           0x28e4ed4, 0x1000edc, 0x1000edc, 0x2de4e84, 0x2ce4e94, 0x1000e98,
                                           0x2cd8d98, 0x1000d94, 0x1000c84, 0x0};

// Exclusive scan of x over the workgroup's 256 threads (all of them call it);
// total = the workgroup's sum.  Integers: the order of the sums does not matter.
DEV int block_excl_scan(int x, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(inc, off, 64);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int v = s_w[w];
        base += w < wave ? v : 0;
        total += v;
    }
    return base + inc - x;
}

struct Cube {
    int i, j, k;
    int lin0;       // the linear index of the cube's corner 0 among the points
    int px, pxy;    // the points' strides along j and k
    bool in;        // the thread has a cube
};

DEV Cube cube_of(const WmeshArgs& a) {
    Cube c;
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t cubes = (int64_t)a.nx * a.ny * a.nz;
    c.in = q < cubes;
    const int64_t qq = c.in ? q : 0;
    const int r = (int)(qq / a.nx);
    c.i = (int)(qq - (int64_t)r * a.nx);
    c.j = r % a.ny;
    c.k = r / a.ny;
    c.px = a.nx + 1;
    c.pxy = c.px * (a.ny + 1);
    c.lin0 = c.k * c.pxy + c.j * c.px + c.i;
    return c;
}

DEV int corner_lin(const Cube& c, int corner) {
    return c.lin0 + (corner & 1) + ((corner >> 1) & 1) * c.px + ((corner >> 2) & 1) * c.pxy;
}

// The cube's tetrahedra in order: emit(tp, case, tris) for each that draws.
template <class F>
DEV void for_tets(const double* f, F&& emit) {
#pragma unroll
    for (int tp = 0; tp < 6; ++tp) {
        const uint32_t cc = kTetCorners[tp];
        const double g[4] = {f[cc & 7], f[(cc >> 4) & 7], f[(cc >> 8) & 7], f[(cc >> 12) & 7]};
        if (!(finite(g[0]) && finite(g[1]) && finite(g[2]) && finite(g[3]))) continue;
        const int cs = (g[0] < 0.0 ? 1 : 0) | (g[1] < 0.0 ? 2 : 0) | (g[2] < 0.0 ? 4 : 0) | (g[3] < 0.0 ? 8 : 0);
        if (cs == 0 || cs == 15) continue;
        emit(tp, cs, kCaseTris[cs]);
    }
}

DEV void load_cube(const WmeshArgs& a, const Cube& c, double* f) {
#pragma unroll
    for (int m = 0; m < 8; ++m) f[m] = a.tsdf[corner_lin(c, m)];
}

__global__ __launch_bounds__(kBlock) void k_wmesh_mark(const WmeshArgs a) {
    __shared__ int s_w[4];
    const Cube c = cube_of(a);
    int count = 0;
    if (c.in) {
        double f[8];
        load_cube(a, c, f);
        uint64_t used = 0;   // byte m: the edge bits that corner m owns
        for_tets(f, [&](int tp, int cs, uint32_t tris) {
            const uint32_t cc = kTetCorners[tp];
            const int n = (int)(tris >> 24);
            count += n;
            for (int e = 0; e < 3 * n; ++e) {
                const uint32_t pq = tris >> (4 * e);
                const uint32_t ca = (cc >> (4 * (pq & 3))) & 7, cb = (cc >> (4 * ((pq >> 2) & 3))) & 7;
                used |= (uint64_t)1 << (8 * ca + ((ca ^ cb) - 1));
            }
        });
#pragma unroll
        for (int m = 0; m < 7; ++m) {   // corner 7 owns no edge
            const uint32_t bits = (uint32_t)(used >> (8 * m)) & 0x7f;
            if (bits) {
                const int lin = corner_lin(c, m);
                atomicOr(a.mask + (lin >> 2), bits << (8 * (lin & 3)));
            }
        }
    }
    int total;
    block_excl_scan(count, s_w, total);
    if (threadIdx.x == 0) a.tsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_wmesh_vcount(const WmeshArgs a, int64_t points) {
    __shared__ int s_w[4];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int n = p < points ? __popc(((const uint8_t*)a.mask)[p]) : 0;
    int total;
    block_excl_scan(n, s_w, total);
    if (threadIdx.x == 0) a.vsum[blockIdx.x] = total;
}

// Workgroup 0: vsum[0..nbv) -> exclusive offsets in place, vsum[nbv] and total[0]
// = the sum; workgroup 1: the same for tsum and total[1] (k_wseed_scan's scheme).
__global__ __launch_bounds__(kScanThreads) void k_wmesh_scan(int64_t* vsum, int64_t nbv, int64_t* tsum, int64_t nbt,
                                                             int64_t* total) {
    __shared__ int64_t part[kScanThreads];
    int64_t* x = blockIdx.x ? tsum : vsum;
    const int64_t n = blockIdx.x ? nbt : nbv;
    const int tid = threadIdx.x;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads;
    const int64_t b = min((int64_t)tid * per, n), e = min(b + per, n);
    int64_t s = 0;
    for (int64_t k = b; k < e; ++k) s += x[k];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int64_t v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t r = tid ? part[tid - 1] : 0;
    for (int64_t k = b; k < e; ++k) {   // a thread rewrites its own chunk only
        const int64_t v = x[k];
        x[k] = r;
        r += v;
    }
    if (tid == kScanThreads - 1) {
        x[n] = part[tid];
        total[blockIdx.x] = part[tid];
    }
}

__global__ __launch_bounds__(kBlock) void k_wmesh_vertex(const WmeshArgs a, int64_t points) {
    __shared__ int s_w[4];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in = p < points;
    const uint32_t bits = in ? ((const uint8_t*)a.mask)[p] : 0;
    int total;
    const int64_t first = a.vsum[blockIdx.x] + block_excl_scan(__popc(bits), s_w, total);
    if (!in) return;
    a.voff[p] = (int32_t)first;
    if (!bits || first >= a.cap_v) return;
    const int px = a.nx + 1, py = a.ny + 1;
    const int r = (int)(p / px);
    const int i = (int)(p - (int64_t)r * px), j = r % py, k = r / py;
    const double fa = a.tsdf[p];
    const double Pa[3] = {a.origin[0] + (double)i * a.voxel, a.origin[1] + (double)j * a.voxel,
                          a.origin[2] + (double)k * a.voxel};
    int64_t at = first;
    for (int e = 0; e < 7; ++e) {
        if (!((bits >> e) & 1)) continue;
        if (at >= a.cap_v) break;
        const int d = e + 1, dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        const int64_t pb = p + dx + (int64_t)dy * px + (int64_t)dz * px * py;
        const double fb = a.tsdf[pb];
        const double t = fa / (fa - fb);
        const double Pb[3] = {a.origin[0] + (double)(i + dx) * a.voxel, a.origin[1] + (double)(j + dy) * a.voxel,
                              a.origin[2] + (double)(k + dz) * a.voxel};
#pragma unroll
        for (int m = 0; m < 3; ++m) a.vert[3 * at + m] = Pa[m] + t * (Pb[m] - Pa[m]);
        // the endpoint nearer the surface, or the other one when it saw no colour
        const int64_t nearer = t < 0.5 ? p : pb, other = t < 0.5 ? pb : p;
        const int64_t src = a.cnt[nearer] ? nearer : other;
#pragma unroll
        for (int m = 0; m < 3; ++m) a.vcol[3 * at + m] = a.rgb[3 * src + m];
        ++at;
    }
}

__global__ __launch_bounds__(kBlock) void k_wmesh_tri(const WmeshArgs a) {
    __shared__ int s_w[4];
    const Cube c = cube_of(a);
    double f[8];
    int count = 0;
    if (c.in) {
        load_cube(a, c, f);
        for_tets(f, [&](int, int, uint32_t tris) { count += (int)(tris >> 24); });
    }
    int total;
    int64_t at = a.tsum[blockIdx.x] + block_excl_scan(count, s_w, total);
    if (!c.in || count == 0 || at >= a.cap_t) return;
    const uint8_t* mask = (const uint8_t*)a.mask;
    for_tets(f, [&](int tp, int cs, uint32_t tris) {
        const uint32_t cc = kTetCorners[tp];
        const bool flip = (kFlip[tp] >> cs) & 1;
        const int n = (int)(tris >> 24);
        for (int t = 0; t < n; ++t, ++at) {
            if (at >= a.cap_t) continue;
            int32_t v[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const uint32_t pq = tris >> (4 * (3 * t + e));
                const uint32_t ca = (cc >> (4 * (pq & 3))) & 7, cb = (cc >> (4 * ((pq >> 2) & 3))) & 7;
                const int lin = corner_lin(c, (int)ca);
                const uint32_t below = ((uint32_t)1 << ((ca ^ cb) - 1)) - 1;
                v[e] = a.voff[lin] + __popc(mask[lin] & below);
            }
            a.tri[3 * at] = v[0];
            a.tri[3 * at + 1] = flip ? v[2] : v[1];
            a.tri[3 * at + 2] = flip ? v[1] : v[2];
        }
    });
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" int mvs_launch_wtsdf_integrate(const SceneDev* sc, const WtsdfArgs* a, hipStream_t s) {
    const int64_t bricks = (int64_t)((a->nx + kBX) / kBX) * ((a->ny + kBY) / kBY) * ((a->nz + kBZ) / kBZ);
    if (bricks <= 0 || bricks >= ((int64_t)1 << 31)) return -1;
    hipLaunchKernelGGL(k_wtsdf_integrate, dim3((unsigned)bricks), dim3(256), 0, s, *sc, *a);
    return launched() ? 0 : -1;
}

extern "C" int mvs_launch_wmesh_extract(const WmeshArgs* a, hipStream_t s) {
    const int64_t points = (int64_t)(a->nx + 1) * (a->ny + 1) * (a->nz + 1);
    const int64_t cubes = (int64_t)a->nx * a->ny * a->nz;
    const int64_t nbv = (points + kBlock - 1) / kBlock, nbt = (cubes + kBlock - 1) / kBlock;
    if (hipMemsetAsync(a->mask, 0, (size_t)((points + 3) / 4) * sizeof(uint32_t), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_wmesh_mark, dim3((unsigned)nbt), dim3(kBlock), 0, s, *a);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wmesh_vcount, dim3((unsigned)nbv), dim3(kBlock), 0, s, *a, points);
    if (!launched()) return -1;
    hipLaunchKernelGGL(k_wmesh_scan, dim3(2), dim3(kScanThreads), 0, s, a->vsum, nbv, a->tsum, nbt, a->total);
    if (!launched()) return -1;
    if (a->cap_v > 0 || a->cap_t > 0) {
        hipLaunchKernelGGL(k_wmesh_vertex, dim3((unsigned)nbv), dim3(kBlock), 0, s, *a, points);
        if (!launched()) return -1;
    }
    if (a->cap_t > 0) {
        hipLaunchKernelGGL(k_wmesh_tri, dim3((unsigned)nbt), dim3(kBlock), 0, s, *a);
        if (!launched()) return -1;
    }
    return 0;
}
