// vfn_icp.hip — the device half of point-to-point ICP (vf_nerf_amd/icp.py): the step between the meshes of vf_nerf_amd/refuse.py and a
// score that evaluation/methods.py:747-801 (metrics_3d_no_vf, icp_align = True) leaves to an external package.
//   transform_points  one lane per point: q' = R q + t in the association of include/vfn.h.
//   nn_radius         the hot path: every query's nearest target within a radius, WITH its index.  One lane per query; the targets are
//                     sorted by the cell of a uniform grid whose edge exceeds the radius, so a query reads the 3 x 3 x 3 cells around
//                     its own as 9 contiguous ranges (the 3 cells along z are neighbours in the sorted order).  Lanes diverge: the
//                     targets come through vector loads.  No LDS.
//   icp_accumulate    the 17 sums a rigid solve needs over the rows with a neighbour, along the fixed tree of vfn_tree.h, lane order
//                     "near": no floating-point atomics, bits a function of n and the data alone.
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.
//
// WHY THE GRID CANNOT CHANGE A BIT.  The result is defined without the grid: the minimum of (d2, original index) in lexicographic order
// over the targets with d2 <= rr, rr = fl(r r).  The minimum of a set does not depend on the order of the visit, so it is enough that
// the 27 cells hold EVERY admissible target.  Per axis, with o = the targets' minimum, e = their maximum, h the cell edge, dim cells:
//   cell(x) = min(max(floor(fl(fl(x - o) / h)), 0), dim - 1),     and a query's coordinate is first clamped: x <- min(max(x, o), e).
// (1) Clamping the query into [o, e] does not increase |x - t| for a target coordinate t, which lies in [o, e].
// (2) An admissible pair has fl(dx dx) <= d2 <= rr: the two further terms of d2 are non-negative and rounding is monotone, so a sum is
//     no smaller than a representable addend.  The host refuses a radius whose square is not a normal number, so either dx dx is
//     subnormal, |dx| < 2^-511 <= r, or dx dx (1 - u) <= rr <= r r (1 + u), |dx| <= r (1 + 2 u); dx = fl(q'x - tx) carries one more
//     rounding: the true |q'x - tx| <= r (1 + 4 u), u = 2^-53.
// (3) For x <= y in [o, e], s = x - o >= 0: fl(fl(s) / h) lies within s / h (1 +- u)^2, so the two real cell coordinates a <= b satisfy
//     b - a <= (y - x) / h + 2.01 u (a + b) <= (y - x) / h + 4.02 u K with K a bound on (e - o) / h.  The host gives h >= r (1 + 2^-20)
//     and at most GRID_CAP = 128 cells an axis (h is enlarged to (e - o) / 128 (1 + 2^-20) when r is smaller), so K <= 129 and
//     b - a <= (1 + 4 u) / (1 + 2^-20) + 519 u < 1 - 2^-21.  Then b <= a + 1 and floor(b) <= floor(a) + 1; the final clamp to
//     [0, dim - 1] is monotone and keeps that.  By symmetry the cells of an admissible pair differ by at most 1 on every axis.
// A bare h = r fails step (3): (1 + 4 u) / 1 + 519 u > 1, and two points exactly r apart can land two cells apart.
// Within a cell the sorted order is the original one (the sort is stable), but nothing relies on it: the comparison carries the index.
#include "vfn_common.h"
#include "vfn_tree.h"
#include <math.h>

namespace {

constexpr int ICP_BLOCK = 256;
constexpr int ACC_N = 17;                                                          // count, sum d2, 3 + 3 first moments, 9 products
constexpr int GRID_CAP = VFN_ICP_GRID_CAP;                                         // cells per axis at most (include/vfn.h)
constexpr double GRID_MARGIN = 1.0 + 1.0 / (double)(1ll << VFN_ICP_GRID_MARGIN_LOG2);     // cell edge over radius at least: 1 + 2^-20

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

struct Xform { double r[9], t[3]; int on; };            // by value in the kernel arguments; on = 0: the identity, no arithmetic
struct Grid { double o[3], e[3], h; int dim[3]; };

__device__ __forceinline__ void apply(const Xform& T, double x, double y, double z, double& px, double& py, double& pz) {
    if (T.on) {
        px = ((T.r[0] * x + T.r[1] * y) + T.r[2] * z) + T.t[0];
        py = ((T.r[3] * x + T.r[4] * y) + T.r[5] * z) + T.t[1];
        pz = ((T.r[6] * x + T.r[7] * y) + T.r[8] * z) + T.t[2];
    } else {
        px = x; py = y; pz = z;
    }
}

__global__ __launch_bounds__(256) void vfn_icp_finite_kernel(const double* __restrict__ q, long long n, const double* __restrict__ t, long long m,
                                                             unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nq = 3 * n, nt = 3 * m;
    bool bad = false;
    if (i < nq) bad = !isfinite(q[i]);
    else if (i < nq + nt) bad = !isfinite(t[i - nq]);
    if (bad) atomicOr(info, 1ull);
}

__global__ __launch_bounds__(ICP_BLOCK) void vfn_transform_points_kernel(const double* __restrict__ q, long long n, Xform T, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double px, py, pz;
    apply(T, q[3 * i], q[3 * i + 1], q[3 * i + 2], px, py, pz);
    out[3 * i] = px; out[3 * i + 1] = py; out[3 * i + 2] = pz;
}

// lane -> query order[lane] (order NULL: the lane's own number).  sorted[m,3] are the targets in cell order, perm[m] their original
// indices, cell_start[cells + 1] the first sorted position of every cell.  Every range is clipped to [0, m] before it is read.
__global__ __launch_bounds__(ICP_BLOCK) void vfn_nn_radius_kernel(const double* __restrict__ q, long long n, Xform T, const double* __restrict__ sorted,
                                                                  const long long* __restrict__ perm, long long m,
                                                                  const int* __restrict__ cell_start, Grid g, double rr,
                                                                  const long long* __restrict__ order, long long* __restrict__ index,
                                                                  double* __restrict__ sqdist) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= n) return;
    long long i = order ? order[lane] : lane;
    if (i < 0 || i >= n) return;
    double px, py, pz;
    apply(T, q[3 * i], q[3 * i + 1], q[3 * i + 2], px, py, pz);
    const int cx = vfn_cell_of(px, g.o[0], g.e[0], g.h, g.dim[0]);              // (vfn_common.h: shared with csrc/vfn_nn.hip)
    const int cy = vfn_cell_of(py, g.o[1], g.e[1], g.h, g.dim[1]);
    const int cz = vfn_cell_of(pz, g.o[2], g.e[2], g.h, g.dim[2]);
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.dim[0] ? cx + 1 : g.dim[0] - 1;
    const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < g.dim[1] ? cy + 1 : g.dim[1] - 1;
    const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < g.dim[2] ? cz + 1 : g.dim[2] - 1;
    double best = __longlong_as_double((long long)INF_BITS);
    long long bi = -1;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy) {
            const long long row = ((long long)ix * g.dim[1] + iy) * g.dim[2];
            long long j = cell_start[row + z0], j1 = cell_start[row + z1 + 1];
            j = j < 0 ? 0 : j;
            j1 = j1 > m ? m : j1;
            for (; j < j1; ++j) {
                const double d2 = vfn_pair_sqdist(px, py, pz, sorted[3 * j], sorted[3 * j + 1], sorted[3 * j + 2]);
                if (d2 <= rr && d2 <= best) {
                    const long long k = perm[j];
                    if (d2 < best || k < bi) { best = d2; bi = k; }
                }
            }
        }
    index[i] = bi;
    sqdist[i] = best;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the 17 sums
// ---------------------------------------------------------------------------------------------------------------------------------
using Acc = TreeSum<ACC_N>;

__device__ __forceinline__ Acc acc_row(long long i, long long n, const double* __restrict__ q, const Xform& T, const double* __restrict__ t, long long m,
                                       const long long* __restrict__ index, const double* __restrict__ sqdist, double ax, double ay, double az,
                                       unsigned long long* __restrict__ info) {
    Acc r;
#pragma unroll
    for (int c = 0; c < ACC_N; ++c) r.v[c] = 0.0;                // a row past n, or without a neighbour, joins as the identity
    if (i >= n) return r;
    const long long j = index[i];
    if (j < 0) return r;
    if (j >= m) { atomicOr(info, 2ull); return r; }
    double px, py, pz;
    apply(T, q[3 * i], q[3 * i + 1], q[3 * i + 2], px, py, pz);
    const double p[3] = {px - ax, py - ay, pz - az};
    const double s[3] = {t[3 * j] - ax, t[3 * j + 1] - ay, t[3 * j + 2] - az};
    r.v[0] = 1.0;
    r.v[1] = sqdist[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.v[2 + a] = p[a];
        r.v[5 + a] = s[a];
#pragma unroll
        for (int b = 0; b < 3; ++b) r.v[8 + 3 * a + b] = p[a] * s[b];
    }
    return r;
}

// first level: block b covers rows [b TREE_TILE, (b + 1) TREE_TILE); lane l takes the rows l + 256 k in the "near" order, then the block
// tree.  The lane tree is not unrolled: sixteen rows' loads in flight at once would need more registers than a lane has.
__global__ __launch_bounds__(TREE_LANES) void vfn_icp_accumulate_kernel(const double* __restrict__ q, long long n, Xform T, const double* __restrict__ t,
                                                                        long long m, const long long* __restrict__ index,
                                                                        const double* __restrict__ sqdist, double ax, double ay, double az,
                                                                        double* __restrict__ partials, unsigned long long* __restrict__ info) {
    __shared__ Acc sh[TREE_LANES];
    const int l = threadIdx.x;
    const long long base = (long long)blockIdx.x * TREE_TILE + l;
    const Acc mine = tree_lane<1, Acc>([&](int k) { return acc_row(base + (long long)k * TREE_LANES, n, q, T, t, m, index, sqdist, ax, ay, az, info); },
                                       TreeAdd());
    tree_block<TREE_LANES>(mine, sh, TreeAdd());
    if (l < ACC_N) partials[(long long)blockIdx.x * ACC_N + l] = sh[0].v[l];
}

// second level over the p partials; the block tree one component after the other through the same 1024 doubles of LDS (1024 Acc would
// be 136 KiB).
__global__ __launch_bounds__(TREE_TOP) void vfn_icp_accumulate_top_kernel(const double* __restrict__ partials, long long p, double* __restrict__ sums) {
    __shared__ double sh[TREE_TOP];
    Acc zero;
#pragma unroll
    for (int c = 0; c < ACC_N; ++c) zero.v[c] = 0.0;
    const Acc s = tree_top_lane(p, zero, [&](long long i) {
        Acc r;
#pragma unroll
        for (int c = 0; c < ACC_N; ++c) r.v[c] = partials[i * ACC_N + c];
        return r;
    }, TreeAdd());
#pragma unroll
    for (int c = 0; c < ACC_N; ++c) {
        const double r = tree_block<TREE_TOP>(s.v[c], sh, TreeAdd());
        if (threadIdx.x == 0) sums[c] = r;
        __syncthreads();                               // the next component overwrites sh
    }
}

// the 12 doubles of a transform (host memory) -> the kernel argument; false when one is not finite
bool load_xform(const double* transform, Xform* T) {
    T->on = transform != nullptr;
    for (int k = 0; k < 9; ++k) T->r[k] = transform ? transform[k] : (k % 4 == 0 ? 1.0 : 0.0);
    for (int k = 0; k < 3; ++k) T->t[k] = transform ? transform[9 + k] : 0.0;
    if (transform)
        for (int k = 0; k < 12; ++k)
            if (!isfinite(transform[k])) return false;
    return true;
}

bool counts_ok(int64_t n, int64_t m) { return n >= 1 && m >= 1 && n < (1ll << 31) && m < (1ll << 31); }

}  // namespace

extern "C" int vfn_transform_points(const double* points, int64_t n, const double* transform, double* out, void* stream) {
    VFN_REQUIRE(n >= 1 && n < (1ll << 31), "vfn_transform_points: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(points && out, "vfn_transform_points: NULL argument");
    Xform T;
    VFN_REQUIRE(load_xform(transform, &T), "vfn_transform_points: a non-finite transform");
    hipLaunchKernelGGL(vfn_transform_points_kernel, dim3(blocks_for(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, (hipStream_t)stream, points, (long long)n, T, out);
    return vfn_check_launch("vfn_transform_points");
}

extern "C" int vfn_nn_radius(const double* queries, int64_t n, const double* transform, const double* sorted_targets, const int64_t* perm,
                             int64_t m, const int32_t* cell_start, const double* box, int32_t nx, int32_t ny, int32_t nz, double radius,
                             const int64_t* order, int32_t check_finite, int64_t* index, double* sqdist, int64_t* info, void* stream) {
    VFN_REQUIRE(counts_ok(n, m), "vfn_nn_radius: n %lld / m %lld outside [1, 2^31)", (long long)n, (long long)m);
    VFN_REQUIRE(queries && sorted_targets && perm && cell_start && box && index && sqdist && info, "vfn_nn_radius: NULL argument");
    const double rr = radius * radius;
    VFN_REQUIRE(isfinite(radius) && radius > 0 && isfinite(rr) && rr >= 2.2250738585072014e-308,
                "vfn_nn_radius: the radius %g is not a positive finite number with a normal square", radius);
    Xform T;
    VFN_REQUIRE(load_xform(transform, &T), "vfn_nn_radius: a non-finite transform");
    VFN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= GRID_CAP && ny <= GRID_CAP && nz <= GRID_CAP, "vfn_nn_radius: grid %d x %d x %d outside [1, %d]^3",
                nx, ny, nz, GRID_CAP);
    Grid g;
    for (int k = 0; k < 3; ++k) { g.o[k] = box[k]; g.e[k] = box[3 + k]; }
    g.h = box[6];
    g.dim[0] = nx; g.dim[1] = ny; g.dim[2] = nz;
    bool box_ok = isfinite(g.h) && g.h >= radius * GRID_MARGIN;
    for (int k = 0; k < 3; ++k) box_ok = box_ok && isfinite(g.o[k]) && isfinite(g.e[k]) && g.o[k] <= g.e[k] && (g.e[k] - g.o[k]) / g.h <= GRID_CAP + 1;
    VFN_REQUIRE(box_ok, "vfn_nn_radius: the box is not finite and ordered, or its cell edge %g is below radius (1 + 2^-20) or (max - min) / %d", g.h, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    // (the sorted targets are a permutation of the targets: their coordinates are the ones to check)
    if (check_finite)
        hipLaunchKernelGGL(vfn_icp_finite_kernel, dim3(blocks_for(3 * ((long long)n + m), 256)), dim3(256), 0, s, queries, (long long)n, sorted_targets,
                       (long long)m, (unsigned long long*)info);
    hipLaunchKernelGGL(vfn_nn_radius_kernel, dim3(blocks_for(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, s, queries, (long long)n, T, sorted_targets,
                       (const long long*)perm, (long long)m, (const int*)cell_start, g, rr, (const long long*)order, (long long*)index, sqdist);
    return vfn_check_launch("vfn_nn_radius");
}

extern "C" int64_t vfn_icp_accumulate_workspace_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) {
        vfn_set_error("vfn_icp_accumulate_workspace_bytes: n %lld outside [1, 2^31)", (long long)n);
        return -1;
    }
    return (int64_t)(tree_tiles(n) * ACC_N * sizeof(double));
}

extern "C" int vfn_icp_accumulate(const double* queries, int64_t n, const double* transform, const double* targets, int64_t m,
                                  const int64_t* index, const double* sqdist, const double* anchor, double* sums, int64_t* info,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    VFN_REQUIRE(counts_ok(n, m), "vfn_icp_accumulate: n %lld / m %lld outside [1, 2^31)", (long long)n, (long long)m);
    const int64_t need = vfn_icp_accumulate_workspace_bytes(n);
    VFN_REQUIRE(queries && targets && index && sqdist && anchor && sums && info && workspace && workspace_bytes >= need,
                "vfn_icp_accumulate: NULL argument or a workspace of %lld bytes < %lld", (long long)workspace_bytes, (long long)need);
    Xform T;
    VFN_REQUIRE(load_xform(transform, &T), "vfn_icp_accumulate: a non-finite transform");
    VFN_REQUIRE(isfinite(anchor[0]) && isfinite(anchor[1]) && isfinite(anchor[2]), "vfn_icp_accumulate: a non-finite anchor");
    hipStream_t s = (hipStream_t)stream;
    const long long p = tree_tiles(n);
    hipLaunchKernelGGL(vfn_icp_accumulate_kernel, dim3((unsigned)p), dim3(TREE_LANES), 0, s, queries, (long long)n, T, targets, (long long)m,
                       (const long long*)index, sqdist, anchor[0], anchor[1], anchor[2], (double*)workspace, (unsigned long long*)info);
    hipLaunchKernelGGL(vfn_icp_accumulate_top_kernel, dim3(1), dim3(TREE_TOP), 0, s, (const double*)workspace, p, sums);
    return vfn_check_launch("vfn_icp_accumulate");
}
