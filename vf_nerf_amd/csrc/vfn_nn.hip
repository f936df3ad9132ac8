// vfn_nn.hip — every query's nearest target over ALL targets, WITH its index (include/vfn.h: vfn_nn_nearest, vfn_nn_nearest_list): the
// unbounded search that vf_nerf_amd/metrics3d.py scores with, on the grid that csrc/vfn_icp.hip searches within a radius.
//   nn_nearest       one lane per query: the cells around the query's own, ring by ring (ring r = the cells at Chebyshev distance exactly
//                    r, clipped to the grid), until a lower bound on every unvisited target's d2 exceeds the best found.  The targets are
//                    sorted by cell and the cells along z are neighbours in that order, so a row of a ring is one contiguous range (a
//                    row on the ring's x or y face) or two single cells (its z faces).  A query that has not stopped after ring
//                    max_rings puts its number on a list.  Lanes diverge: vector loads, no LDS, no lane waits on another.
//   nn_nearest_list  one wave per listed query: 64 lanes stride over all m targets in their ORIGINAL order, then a lexicographic
//                    (d2, index) minimum across the wave by shuffles.  Wave-uniform control flow throughout.
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.
//
// WHY THE GRID CANNOT CHANGE A BIT.  The result is defined without the grid: the minimum of (d2, original index) in lexicographic order
// over all targets, d2 = vfn_pair_sqdist's expression.  The minimum of a set does not depend on the order of the visit, and the list
// kernel visits every target; so it is enough that a query which STOPS after ring r has missed no target that could win or tie: every
// target outside rings 0..r must have d2 > best, strictly.  Notation and steps (1), (3) are those of the argument in csrc/vfn_icp.hip:
// per axis o = the targets' minimum, e = their maximum, h the cell edge, dim cells, u = 2^-53, K = 129 >= (e - o) / h, and
//   a(x) = fl(fl(x' - o) / h) with x' = min(max(x, o), e)   the real cell coordinate (vfn_cell_coord), a >= 0,
//   cell(x) = min(max(floor(a(x)), 0), dim - 1)              (vfn_cell_of).
// For the query: c = cell(x), f = a(x) - c per axis.  c <= a < 130 are both multiples of ulp(a) <= 1, so f is exact and f >= 0; f < 1
// except where the final clamp acted, c = dim - 1 <= a - 1 (the upper face).  s = the minimum over the three axes of
// min(f, max(fl(1 - f), 0)); fl(1 - f) <= (1 - f) (1 + u) when f <= 1.
// The stop rule after ring r: rings 0..r cover the grid (r >= c and r >= dim - 1 - c on every axis: nothing is unvisited), or
//   r + s >= 2^-20  and  lb >= 2^-1022  and  best < lb,    w = fl(fl(r + s) h),  lb = fl(fl(w w) (1 - 2^-20)).
// (a) A target t not visited by rings 0..r has a cell that differs from c by at least r + 1 on some axis; take that axis.
//     High side, cell(t) >= c + r + 1: cell(t) <= floor(a(t)) (the clamps only lower a non-negative floor), so a(t) >= c + r + 1 and
//     a(t) - a(x) >= r + 1 - f.  This needs c + r + 1 <= dim - 1, so c < dim - 1, the final clamp did not act on the query and f < 1;
//     on the upper face (f >= 1) there is no high side, and max(., 0) only keeps s >= 0 there.
//     Low side, cell(t) <= c - r - 1 < dim - 1: the final clamp did not act on t, so a(t) < cell(t) + 1 <= c - r and
//     a(x) - a(t) > r + f.
//     Either way |a(t) - a(x)| >= r + s', s' in {f, 1 - f}, and s <= s' (1 + u).
// (b) The clamped query x' and t both lie in [o, e].  Step (3) there: for two points of [o, e] the real cell coordinates differ by at
//     most |t - x'| / h + 4.02 u K.  Hence |t - x'| >= (r + s' - 519 u) h, and by step (1) the unclamped |t - x| >= |t - x'|.
// (c) With the first guard, 519 u <= 2^-43.9 <= (r + s') 2^-23.9 and (1 + u)^-1 costs another u:
//     |t - x| >= (r + s) h (1 - 2^-23.8).  dx = fl(x - t) has |dx| >= |t - x| (1 - u), and when the real dx dx is at least 2^-1022
//     its rounding costs one more factor (1 - u): fl(dx dx) >= ((r + s) h)^2 (1 - 2^-22.7).
// (d) On the other side w <= (r + s) h (1 + u)^2 (r + s <= 129 and h are normal, r + s >= 2^-20 and w >= 2^-511 follows from the second
//     guard, so both roundings are relative), fl(w w) <= w^2 (1 + u), and lb >= 2^-1022 is the rounding of a real within 2^-1075 of
//     it, again a factor 1 + u: lb <= ((r + s) h)^2 (1 + u)^6 (1 - 2^-20) < ((r + s) h)^2 (1 - 2^-20.1).  The host refuses a cell edge
//     with ((GRID_CAP + 2) h)^2 not finite, so nothing here overflows; and the real dx dx of (c) exceeds lb >= 2^-1022, which is the
//     normality (c) assumed.
// (e) d2 >= fl(dx dx) (the two further terms are non-negative and rounding is monotone: a sum is no smaller than a representable
//     addend) > lb > best.  Strict: an unvisited target can neither win nor tie, whatever its index.
// Without the first guard the absolute term 519 u of (b) could exceed r + s (a query on a cell face in ring 0: s = 0, lb = 0 stops
// nothing; s = 1e-300 must not stop anything either).  Without the second, dx dx could be subnormal and its rounding not relative.
// A NaN or infinite query coordinate cannot reach memory it should not: fmin / fmax drop a NaN, the cell is clamped in double before
// the conversion and every range is clipped to [0, m]; check_finite reports it.
#include "vfn_common.h"
#include <math.h>

namespace {

constexpr int NN_BLOCK = 256;
constexpr int WAVE = 64;                                                            // gfx950: one query per wave in the list kernel
constexpr int LIST_UNROLL = 4;                                                      // targets a lane of the list kernel has in flight
constexpr int GRID_CAP = VFN_ICP_GRID_CAP;                                          // cells per axis at most (include/vfn.h)
constexpr double RING_GUARD = 1.0 / (double)(1ll << VFN_ICP_GRID_MARGIN_LOG2);      // 2^-20: the least r + s at which the bound is used
constexpr double RING_SHAVE = 1.0 - 1.0 / (double)(1ll << VFN_ICP_GRID_MARGIN_LOG2);    // 1 - 2^-20
constexpr double MIN_NORMAL = 2.2250738585072014e-308;                              // 2^-1022

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

struct Grid { double o[3], e[3], h; int dim[3]; };

__global__ __launch_bounds__(256) void vfn_nn_finite_kernel(const double* __restrict__ q, long long n, const double* __restrict__ t, long long m,
                                                            unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nq = 3 * n, nt = 3 * m;
    bool bad = false;
    if (i < nq) bad = !isfinite(q[i]);
    else if (i < nq + nt) bad = !isfinite(t[i - nq]);
    if (bad) atomicOr(info, 1ull);
}

// the sorted positions [j, j1) against one query; the comparison carries the original index, so the order of the visit does not matter
__device__ __forceinline__ void scan_range(long long j, long long j1, long long m, const double* __restrict__ sorted, const long long* __restrict__ perm,
                                           double px, double py, double pz, double& best, long long& bi) {
    j = j < 0 ? 0 : j;
    j1 = j1 > m ? m : j1;
    for (; j < j1; ++j) {
        const double d2 = vfn_pair_sqdist(px, py, pz, sorted[3 * j], sorted[3 * j + 1], sorted[3 * j + 2]);
        if (d2 <= best) {
            const long long k = perm[j];
            if (d2 < best || k < bi) { best = d2; bi = k; }
        }
    }
}

// lane -> query order[lane] (order NULL: the lane's own number); sorted / perm / cell_start as in vfn_nn_radius.  Every loop is bounded
// by the grid's dimensions: r <= min(max_rings, the ring that covers the grid) <= 127.
__global__ __launch_bounds__(NN_BLOCK) void vfn_nn_nearest_kernel(const double* __restrict__ q, long long n, const double* __restrict__ sorted,
                                                                  const long long* __restrict__ perm, long long m,
                                                                  const int* __restrict__ cell_start, Grid g, int max_rings,
                                                                  const long long* __restrict__ order, long long* __restrict__ index,
                                                                  double* __restrict__ sqdist, long long* __restrict__ leftover,
                                                                  unsigned long long* __restrict__ leftover_count) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= n) return;
    const long long i = order ? order[lane] : lane;
    if (i < 0 || i >= n) return;
    const double p[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    int c[3];
    double s = 1.0;
    int cover = 0;                                                   // the first ring after which rings 0..r hold every cell
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = vfn_cell_coord(p[k], g.o[k], g.e[k], g.h);
        c[k] = vfn_cell_of(p[k], g.o[k], g.e[k], g.h, g.dim[k]);
        const double f = a - (double)c[k];
        s = fmin(s, fmin(f, fmax(1.0 - f, 0.0)));
        const int far = c[k] > g.dim[k] - 1 - c[k] ? c[k] : g.dim[k] - 1 - c[k];
        cover = far > cover ? far : cover;
    }
    const int last = cover < max_rings ? cover : max_rings;
    double best = __longlong_as_double((long long)INF_BITS);
    long long bi = -1;
    bool stopped = false;
    for (int r = 0; r <= last && !stopped; ++r) {
        const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < g.dim[0] ? c[0] + r : g.dim[0] - 1;
        const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < g.dim[1] ? c[1] + r : g.dim[1] - 1;
        const int zl = c[2] - r, zh = c[2] + r;
        const int z0 = zl > 0 ? zl : 0, z1 = zh < g.dim[2] ? zh : g.dim[2] - 1;
        for (int ix = x0; ix <= x1; ++ix) {
            const bool x_face = ix - c[0] == r || c[0] - ix == r;
            for (int iy = y0; iy <= y1; ++iy) {
                const long long row = ((long long)ix * g.dim[1] + iy) * g.dim[2];
                if (x_face || iy - c[1] == r || c[1] - iy == r) {    // the whole run of the row along z belongs to the ring (all of ring 0)
                    scan_range(cell_start[row + z0], cell_start[row + z1 + 1], m, sorted, perm, p[0], p[1], p[2], best, bi);
                } else {                                             // an inner row: the ring's two z faces, where the grid has them
                    if (zl >= 0) scan_range(cell_start[row + zl], cell_start[row + zl + 1], m, sorted, perm, p[0], p[1], p[2], best, bi);
                    if (zh < g.dim[2]) scan_range(cell_start[row + zh], cell_start[row + zh + 1], m, sorted, perm, p[0], p[1], p[2], best, bi);
                }
            }
        }
        if (r >= cover) {
            stopped = true;
        } else {
            const double rs = (double)r + s;
            const double w = rs * g.h;
            const double lb = (w * w) * RING_SHAVE;
            stopped = rs >= RING_GUARD && lb >= MIN_NORMAL && best < lb;
        }
    }
    if (stopped) {
        index[i] = bi;
        sqdist[i] = best;
    } else {
        const unsigned long long slot = atomicAdd(leftover_count, 1ull);
        if (slot < (unsigned long long)n) leftover[slot] = i;        // (an order that repeats a query could count past n: never write there)
    }
}

// wave w serves the query leftover[w]; lane l takes the targets l, l + 64, ... in ascending order and keeps its FIRST strict minimum,
// so a lane's (d2, j) is its lexicographic minimum; the butterfly then joins the 64 of them.  A lane without a target below +inf holds
// (+inf, -1), which loses to every finite d2.  Nothing diverges between the loop and the shuffles: the bounds are wave-uniform.
__global__ __launch_bounds__(NN_BLOCK) void vfn_nn_nearest_list_kernel(const double* __restrict__ q, long long n, const double* __restrict__ t, long long m,
                                                                       const long long* __restrict__ leftover, long long count,
                                                                       long long* __restrict__ index, double* __restrict__ sqdist) {
    const long long wave = ((long long)blockIdx.x * NN_BLOCK + threadIdx.x) / WAVE;
    const int l = threadIdx.x % WAVE;
    if (wave >= count) return;                                       // (the whole wave)
    const long long i = leftover[wave];
    if (i < 0 || i >= n) return;                                     // (the whole wave)
    const double px = q[3 * i], py = q[3 * i + 1], pz = q[3 * i + 2];
    double best = __longlong_as_double((long long)INF_BITS);
    long long bj = -1;
    long long base = 0;
    for (; base + LIST_UNROLL * WAVE <= m; base += LIST_UNROLL * WAVE) {         // whole batches: the loads of four targets in flight at once
        double d2[LIST_UNROLL];
#pragma unroll
        for (int k = 0; k < LIST_UNROLL; ++k) {
            const long long j = base + k * WAVE + l;
            d2[k] = vfn_pair_sqdist(px, py, pz, t[3 * j], t[3 * j + 1], t[3 * j + 2]);
        }
#pragma unroll
        for (int k = 0; k < LIST_UNROLL; ++k)                                    // still in ascending j
            if (d2[k] < best) { best = d2[k]; bj = base + k * WAVE + l; }
    }
    for (; base < m; base += WAVE) {
        const long long j = base + l;
        if (j < m) {
            const double d2 = vfn_pair_sqdist(px, py, pz, t[3 * j], t[3 * j + 1], t[3 * j + 2]);
            if (d2 < best) { best = d2; bj = j; }
        }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const double ob = __shfl_xor(best, d, WAVE);
        const long long oj = __shfl_xor(bj, d, WAVE);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (l == 0) {
        index[i] = bj;
        sqdist[i] = best;
    }
}

bool counts_ok(int64_t n, int64_t m) { return n >= 1 && m >= 1 && n < (1ll << 31) && m < (1ll << 31); }

}  // namespace

extern "C" int vfn_nn_nearest(const double* queries, int64_t n, const double* sorted_targets, const int64_t* perm, int64_t m,
                              const int32_t* cell_start, const double* box, int32_t nx, int32_t ny, int32_t nz, int32_t max_rings,
                              const int64_t* order, int32_t check_finite, int64_t* index, double* sqdist, int64_t* leftover,
                              int64_t* leftover_count, int64_t* info, void* stream) {
    VFN_REQUIRE(counts_ok(n, m), "vfn_nn_nearest: n %lld / m %lld outside [1, 2^31)", (long long)n, (long long)m);
    VFN_REQUIRE(queries && sorted_targets && perm && cell_start && box && index && sqdist && leftover && leftover_count && info,
                "vfn_nn_nearest: NULL argument");
    VFN_REQUIRE(max_rings >= 0, "vfn_nn_nearest: max_rings %d is negative", max_rings);
    VFN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= GRID_CAP && ny <= GRID_CAP && nz <= GRID_CAP, "vfn_nn_nearest: grid %d x %d x %d outside [1, %d]^3",
                nx, ny, nz, GRID_CAP);
    Grid g;
    for (int k = 0; k < 3; ++k) { g.o[k] = box[k]; g.e[k] = box[3 + k]; }
    g.h = box[6];
    g.dim[0] = nx; g.dim[1] = ny; g.dim[2] = nz;
    const double reach = (GRID_CAP + 2) * g.h;
    bool box_ok = isfinite(g.h) && g.h >= MIN_NORMAL && isfinite(reach * reach);
    for (int k = 0; k < 3; ++k) box_ok = box_ok && isfinite(g.o[k]) && isfinite(g.e[k]) && g.o[k] <= g.e[k] && (g.e[k] - g.o[k]) / g.h <= GRID_CAP + 1;
    VFN_REQUIRE(box_ok, "vfn_nn_nearest: the box is not finite and ordered, or its cell edge %g is not normal, below (max - min) / %d, or (%d h)^2 overflows",
                g.h, GRID_CAP, GRID_CAP + 2);
    hipStream_t s = (hipStream_t)stream;
    if (check_finite)
        hipLaunchKernelGGL(vfn_nn_finite_kernel, dim3(blocks_for(3 * ((long long)n + m), 256)), dim3(256), 0, s, queries, (long long)n, sorted_targets,
                           (long long)m, (unsigned long long*)info);
    hipLaunchKernelGGL(vfn_nn_nearest_kernel, dim3(blocks_for(n, NN_BLOCK)), dim3(NN_BLOCK), 0, s, queries, (long long)n, sorted_targets,
                       (const long long*)perm, (long long)m, (const int*)cell_start, g, (int)max_rings, (const long long*)order, (long long*)index,
                       sqdist, (long long*)leftover, (unsigned long long*)leftover_count);
    return vfn_check_launch("vfn_nn_nearest");
}

extern "C" int vfn_nn_nearest_list(const double* queries, int64_t n, const double* targets, int64_t m, const int64_t* leftover, int64_t count,
                                   int64_t* index, double* sqdist, void* stream) {
    VFN_REQUIRE(counts_ok(n, m), "vfn_nn_nearest_list: n %lld / m %lld outside [1, 2^31)", (long long)n, (long long)m);
    VFN_REQUIRE(count >= 1 && count <= n, "vfn_nn_nearest_list: count %lld outside [1, n = %lld]", (long long)count, (long long)n);
    VFN_REQUIRE(queries && targets && leftover && index && sqdist, "vfn_nn_nearest_list: NULL argument");
    hipLaunchKernelGGL(vfn_nn_nearest_list_kernel, dim3(blocks_for(count, NN_BLOCK / WAVE)), dim3(NN_BLOCK), 0, (hipStream_t)stream, queries,
                       (long long)n, targets, (long long)m, (const long long*)leftover, (long long)count, (long long*)index, sqdist);
    return vfn_check_launch("vfn_nn_nearest_list");
}
