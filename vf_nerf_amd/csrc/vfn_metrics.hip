// vfn_metrics.hip — scoring a mesh against a mesh on the device: the geometry half of evaluation/methods.py:747-801
// (metrics_3d_no_vf) with utils/utils.py:327-367 (get_chamfer_distance).  The reference samples points on both surfaces
// (trimesh.sample.sample_surface), finds every point's nearest neighbour in the other set with a KD-tree and takes statistics of the
// distances.  Here:
//   tri_areas       one lane per face: 0.5 |e1 x e2|.
//   cumsum          a deterministic inclusive scan of the areas (fixed blocks of 1024, a scan of the block totals, an add-back pass):
//                   the bits of every prefix are a function of the data alone, so equal uniforms always pick equal faces.
//   sample_surface  one lane per point: binary search of u0 x total in the cumulative table, then the folded-square barycentric point.
//   nn_sqdist       the hot path: all pairs, exact.  One lane holds NN_QPL queries in registers; the targets of a slice are read at
//                   wave-uniform addresses (scalar loads, no LDS), 9 fp64 vector instructions per pair, no index; the slices of one
//                   query merge with a 64-bit integer atomicMin on the bits of the non-negative double (order-independent).
//   reduce_stats    sum / min / max / count(x < threshold) along the fixed tree of vfn_tree.h, lane order "far".
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.
#include "vfn_common.h"
#include "vfn_tree.h"
#include <math.h>

namespace {

constexpr int NN_BLOCK = 256;                 // lanes per workgroup
constexpr int NN_QPL = 4;                     // queries per lane: four independent chains per target
constexpr int NN_QBLOCK = NN_BLOCK * NN_QPL;  // queries per workgroup
constexpr int NN_TB = 8;                      // targets per unrolled batch (24 doubles at uniform addresses)
constexpr int NN_MIN_SLICE = 256;             // fewest targets per slice
constexpr long long NN_WANT_BLOCKS = 16384;   // workgroups aimed at: many rounds of 256 CUs, so the last round's idle share stays small

constexpr int SCAN_BLOCK = 256, SCAN_PER = 4, SCAN_TILE = SCAN_BLOCK * SCAN_PER;   // 1024 values per scan block

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------------------------------------------------------------------------
// nearest neighbour
// ---------------------------------------------------------------------------------------------------------------------------------
// best[i] = +inf bits for i < n; info[0] |= 1 when one of the 3 n + 3 m coordinates is not finite
__global__ __launch_bounds__(256) void vfn_nn_prepare_kernel(const double* __restrict__ q, long long n, const double* __restrict__ t, long long m,
                                                             unsigned long long* __restrict__ best, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) best[i] = INF_BITS;
    const long long nq = 3 * n, nt = 3 * m;
    bool bad = false;
    if (i < nq) bad = !isfinite(q[i]);
    else if (i < nq + nt) bad = !isfinite(t[i - nq]);
    if (bad) atomicOr(info, 1ull);
}

// grid (query blocks, target slices); slice s covers targets [s slice_len, min((s + 1) slice_len, m)); slice_len is a multiple of NN_TB
__global__ __launch_bounds__(NN_BLOCK) void vfn_nn_sqdist_kernel(const double* __restrict__ q, long long n, const double* __restrict__ t,
                                                                 long long m, long long slice_len, unsigned long long* __restrict__ best) {
    const long long q0 = (long long)blockIdx.x * NN_QBLOCK + threadIdx.x;
    double qx[NN_QPL], qy[NN_QPL], qz[NN_QPL], b[NN_QPL];
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        long long i = q0 + (long long)k * NN_BLOCK;
        i = i < n ? i : n - 1;                       // lanes past the end repeat the last query and skip the merge
        qx[k] = q[3 * i]; qy[k] = q[3 * i + 1]; qz[k] = q[3 * i + 2];
        b[k] = __longlong_as_double((long long)INF_BITS);
    }
    const long long j0 = (long long)blockIdx.y * slice_len;
    const long long j1 = j0 + slice_len < m ? j0 + slice_len : m;
    long long j = j0;
    for (; j + NN_TB <= j1; j += NN_TB) {
        const double* __restrict__ tp = t + 3 * j;   // wave-uniform: the 24 doubles come through the scalar cache
        double tv[3 * NN_TB];
#pragma unroll
        for (int u = 0; u < 3 * NN_TB; ++u) tv[u] = tp[u];
#pragma unroll
        for (int u = 0; u < NN_TB; ++u)
#pragma unroll
            for (int k = 0; k < NN_QPL; ++k) b[k] = fmin(b[k], vfn_pair_sqdist(qx[k], qy[k], qz[k], tv[3 * u], tv[3 * u + 1], tv[3 * u + 2]));
    }
    for (; j < j1; ++j) {
        const double tx = t[3 * j], ty = t[3 * j + 1], tz = t[3 * j + 2];
#pragma unroll
        for (int k = 0; k < NN_QPL; ++k) b[k] = fmin(b[k], vfn_pair_sqdist(qx[k], qy[k], qz[k], tx, ty, tz));
    }
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const long long i = q0 + (long long)k * NN_BLOCK;
        // a non-negative double orders as its bits do: the slices of one query merge in any order to the same minimum
        if (i < n) atomicMin(best + i, (unsigned long long)__double_as_longlong(b[k]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// areas, scan, sampling
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vfn_tri_areas_kernel(const double* __restrict__ v, long long nv, const long long* __restrict__ f, long long nf,
                                                            double* __restrict__ areas, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const long long a = f[3 * i], b = f[3 * i + 1], c = f[3 * i + 2];
    if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) {
        atomicOr(info, 2ull);
        areas[i] = 0.0;
        return;
    }
    const double e1x = v[3 * b] - v[3 * a], e1y = v[3 * b + 1] - v[3 * a + 1], e1z = v[3 * b + 2] - v[3 * a + 2];
    const double e2x = v[3 * c] - v[3 * a], e2y = v[3 * c + 1] - v[3 * a + 1], e2z = v[3 * c + 2] - v[3 * a + 2];
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    if (!isfinite(area)) atomicOr(info, 1ull);
    areas[i] = area;
}

// One block scans SCAN_TILE consecutive values: lane l adds its SCAN_PER values serially (3 additions), a Kogge-Stone scan over the 256
// lane totals (8 levels), one more addition for the exclusive lane prefix: every local prefix is at most 12 additions deep, a block
// total at most 11.  x and out may be the same array (a lane reads its four values before it writes them).
__global__ __launch_bounds__(SCAN_BLOCK) void vfn_scan_tile_kernel(const double* x, long long n, double* out, double* totals) {
    __shared__ double sh[2][SCAN_BLOCK];
    const int l = threadIdx.x;
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)l * SCAN_PER;
    double s[SCAN_PER];
    double run = 0.0;
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) {
        const double val = base + k < n ? x[base + k] : 0.0;
        run = k == 0 ? val : run + val;
        s[k] = run;
    }
    int cur = 0;
    sh[0][l] = run;
    __syncthreads();
    for (int d = 1; d < SCAN_BLOCK; d <<= 1) {
        const double mine = sh[cur][l];
        sh[cur ^ 1][l] = l >= d ? sh[cur][l - d] + mine : mine;
        cur ^= 1;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k)
        if (base + k < n) out[base + k] = l == 0 ? s[k] : sh[cur][l - 1] + s[k];
    if (totals && l == SCAN_BLOCK - 1) totals[blockIdx.x] = sh[cur][l];
}

// out[i] += prefix[i / SCAN_TILE - 1] for i >= SCAN_TILE: one more addition per level
__global__ __launch_bounds__(256) void vfn_scan_add_kernel(double* __restrict__ out, long long n, const double* __restrict__ prefix) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x + SCAN_TILE;
    if (i < n) out[i] = prefix[i / SCAN_TILE - 1] + out[i];
}

__global__ __launch_bounds__(256) void vfn_sample_surface_kernel(const double* __restrict__ v, long long nv, const long long* __restrict__ f,
                                                                 long long nf, const double* __restrict__ cum, const double* __restrict__ u,
                                                                 long long count, double* __restrict__ points, long long* __restrict__ face_index,
                                                                 unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double t = u[3 * i] * cum[nf - 1];
    long long lo = 0, hi = nf;                      // the smallest index with cum[index] > t
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    const long long face = lo < nf ? lo : nf - 1;
    face_index[i] = face;
    const long long ia = f[3 * face], ib = f[3 * face + 1], ic = f[3 * face + 2];
    if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) {
        atomicOr(info, 2ull);
        points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = 0.0;
        return;
    }
    double a = u[3 * i + 1], b = u[3 * i + 2];
    if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v0 = v[3 * ia + c];
        const double e1 = v[3 * ib + c] - v0, e2 = v[3 * ic + c] - v0;
        points[3 * i + c] = (v0 + a * e1) + b * e2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// statistics
// ---------------------------------------------------------------------------------------------------------------------------------
struct Stats { double sum, mn, mx; long long cnt; };

__device__ __forceinline__ Stats stats_join(const Stats& a, const Stats& b) {
    return Stats{a.sum + b.sum, fmin(a.mn, b.mn), fmax(a.mx, b.mx), a.cnt + b.cnt};
}

__device__ __forceinline__ Stats stats_empty() {
    return Stats{0.0, __longlong_as_double((long long)INF_BITS), -__longlong_as_double((long long)INF_BITS), 0};
}

// first level: block b covers x[b TREE_TILE, (b + 1) TREE_TILE); lane l holds the values l + 256 k in its slots k and joins them in the
// "far" order, then the block tree.  Fully unrolled, the 16 loads issued before the first join: the lane tree is register moves.
__global__ __launch_bounds__(TREE_LANES) void vfn_reduce_stats_kernel(const double* __restrict__ x, long long n, double threshold,
                                                                      Stats* __restrict__ partials) {
    __shared__ Stats sh[TREE_LANES];
    const long long base = (long long)blockIdx.x * TREE_TILE + threadIdx.x;
    Stats s[TREE_PER];
#pragma unroll
    for (int k = 0; k < TREE_PER; ++k) {
        const long long i = base + (long long)k * TREE_LANES;
        if (i < n) {
            const double val = x[i];
            s[k] = Stats{val, val, val, val < threshold ? 1ll : 0ll};
        } else {
            s[k] = stats_empty();
        }
    }
    const Stats mine = tree_lane<TREE_PER, Stats>([&](int k) { return s[tree_far_slot(k)]; }, stats_join);
    const Stats r = tree_block<TREE_LANES>(mine, sh, stats_join);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// second level over the p partials.  stats[4] = sum, min, max, count (as a double: exact below 2^53).
__global__ __launch_bounds__(TREE_TOP) void vfn_reduce_stats_top_kernel(const Stats* __restrict__ partials, long long p, double* __restrict__ stats) {
    __shared__ Stats sh[TREE_TOP];
    const Stats s = tree_top_lane(p, stats_empty(), [&](long long i) { return partials[i]; }, stats_join);
    const Stats r = tree_block<TREE_TOP>(s, sh, stats_join);
    if (threadIdx.x == 0) {
        stats[0] = r.sum; stats[1] = r.mn; stats[2] = r.mx; stats[3] = (double)r.cnt;
    }
}

int scan_levels(long long n, long long* sizes) {
    int k = 0;
    sizes[0] = n;
    while (sizes[k] > SCAN_TILE) { sizes[k + 1] = (sizes[k] + SCAN_TILE - 1) / SCAN_TILE; ++k; }
    return k + 1;
}

}  // namespace

extern "C" int vfn_nn_sqdist(const double* queries, int64_t n, const double* targets, int64_t m, double* best, int64_t* info, void* stream) {
    VFN_REQUIRE(n >= 1 && m >= 1 && n < (1ll << 31) && m < (1ll << 31), "vfn_nn_sqdist: n %lld / m %lld outside [1, 2^31)", (long long)n,
                (long long)m);
    VFN_REQUIRE(queries && targets && best && info, "vfn_nn_sqdist: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const long long coords = 3 * ((long long)n + m);
    hipLaunchKernelGGL(vfn_nn_prepare_kernel, dim3(blocks_for(coords, 256)), dim3(256), 0, s, queries, (long long)n, targets, (long long)m,
                       (unsigned long long*)best, (unsigned long long*)info);
    const long long qblocks = (n + NN_QBLOCK - 1) / NN_QBLOCK;
    long long slices = (NN_WANT_BLOCKS + qblocks - 1) / qblocks;
    const long long most = (m + NN_MIN_SLICE - 1) / NN_MIN_SLICE;
    if (slices > most) slices = most;
    if (slices > 65535) slices = 65535;
    if (slices < 1) slices = 1;
    long long slice_len = (m + slices - 1) / slices;
    slice_len = (slice_len + NN_TB - 1) / NN_TB * NN_TB;
    slices = (m + slice_len - 1) / slice_len;
    hipLaunchKernelGGL(vfn_nn_sqdist_kernel, dim3((unsigned)qblocks, (unsigned)slices), dim3(NN_BLOCK), 0, s, queries, (long long)n, targets,
                       (long long)m, slice_len, (unsigned long long*)best);
    return vfn_check_launch("vfn_nn_sqdist");
}

extern "C" int vfn_tri_areas(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, double* areas, int64_t* info,
                             void* stream) {
    VFN_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_vertices < (1ll << 31) && n_faces < (1ll << 31), "vfn_tri_areas: V %lld / F %lld outside [0, 2^31)",
                (long long)n_vertices, (long long)n_faces);
    if (n_faces == 0) return VFN_OK;
    VFN_REQUIRE(faces && areas && info && (vertices || n_vertices == 0), "vfn_tri_areas: NULL argument");
    hipLaunchKernelGGL(vfn_tri_areas_kernel, dim3(blocks_for(n_faces, 256)), dim3(256), 0, (hipStream_t)stream, vertices, (long long)n_vertices,
                       (const long long*)faces, (long long)n_faces, areas, (unsigned long long*)info);
    return vfn_check_launch("vfn_tri_areas");
}

extern "C" int64_t vfn_cumsum_workspace_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) {
        vfn_set_error("vfn_cumsum_workspace_bytes: n %lld outside [1, 2^31)", (long long)n);
        return -1;
    }
    long long sizes[8];
    const int levels = scan_levels(n, sizes);
    long long total = 0;
    for (int k = 1; k < levels; ++k) total += sizes[k];
    return (int64_t)(total * sizeof(double));
}

extern "C" int vfn_cumsum_f64(const double* x, int64_t n, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t need = vfn_cumsum_workspace_bytes(n);
    if (need < 0) return VFN_ERR_INVALID;
    VFN_REQUIRE(x && out && (need == 0 || workspace) && workspace_bytes >= need, "vfn_cumsum_f64: NULL argument or a workspace of %lld bytes < %lld",
                (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    long long sizes[8];
    const int levels = scan_levels(n, sizes);
    double* level[8];
    level[0] = out;
    double* ws = (double*)workspace;
    for (int k = 1; k < levels; ++k) { level[k] = ws; ws += sizes[k]; }
    // up: level k's block totals are level k + 1's input, scanned in place
    for (int k = 0; k < levels; ++k)
        hipLaunchKernelGGL(vfn_scan_tile_kernel, dim3(blocks_for(sizes[k], SCAN_TILE)), dim3(SCAN_BLOCK), 0, s, k == 0 ? x : (const double*)level[k],
                           sizes[k], level[k], k + 1 < levels ? level[k + 1] : (double*)nullptr);
    // down: every block but the first of a level adds the finished prefix of the blocks before it
    for (int k = levels - 2; k >= 0; --k)
        hipLaunchKernelGGL(vfn_scan_add_kernel, dim3(blocks_for(sizes[k] - SCAN_TILE, 256)), dim3(256), 0, s, level[k], sizes[k],
                           (const double*)level[k + 1]);
    return vfn_check_launch("vfn_cumsum_f64");
}

extern "C" int vfn_sample_surface(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const double* cum,
                                  const double* uniforms, int64_t count, double* points, int64_t* face_index, int64_t* info, void* stream) {
    VFN_REQUIRE(n_vertices >= 1 && n_faces >= 1 && count >= 1 && n_vertices < (1ll << 31) && n_faces < (1ll << 31) && count < (1ll << 31),
                "vfn_sample_surface: V %lld / F %lld / count %lld outside [1, 2^31)", (long long)n_vertices, (long long)n_faces, (long long)count);
    VFN_REQUIRE(vertices && faces && cum && uniforms && points && face_index && info, "vfn_sample_surface: NULL argument");
    hipLaunchKernelGGL(vfn_sample_surface_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, (hipStream_t)stream, vertices, (long long)n_vertices,
                       (const long long*)faces, (long long)n_faces, cum, uniforms, (long long)count, points, (long long*)face_index,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_sample_surface");
}

extern "C" int64_t vfn_reduce_stats_workspace_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) {
        vfn_set_error("vfn_reduce_stats_workspace_bytes: n %lld outside [1, 2^31)", (long long)n);
        return -1;
    }
    return (int64_t)(tree_tiles(n) * sizeof(Stats));
}

extern "C" int vfn_reduce_stats(const double* x, int64_t n, double threshold, double* stats, void* workspace, int64_t workspace_bytes,
                                void* stream) {
    const int64_t need = vfn_reduce_stats_workspace_bytes(n);
    if (need < 0) return VFN_ERR_INVALID;
    VFN_REQUIRE(x && stats && workspace && workspace_bytes >= need, "vfn_reduce_stats: NULL argument or a workspace of %lld bytes < %lld",
                (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const long long p = tree_tiles(n);
    hipLaunchKernelGGL(vfn_reduce_stats_kernel, dim3((unsigned)p), dim3(TREE_LANES), 0, s, x, (long long)n, threshold, (Stats*)workspace);
    hipLaunchKernelGGL(vfn_reduce_stats_top_kernel, dim3(1), dim3(TREE_TOP), 0, s, (const Stats*)workspace, p, stats);
    return vfn_check_launch("vfn_reduce_stats");
}
