// vfn_kmeans.hip — Lloyd's k-means over points in space (vf_nerf_amd/cluster.py): the step of get_dominant_bases (utils/utils.py:216-233)
// that the reference leaves to scikit-learn, after meshops.orient, simplify_vertex_clustering and vertex_normals.
//   kmeans_assign   one lane per point, the k <= 64 centres in LDS: the nearest centre (ties to the LOWEST), its squared distance in the
//                   association of vfn_nn_radius, and how many labels differ from the previous pass (an INTEGER atomic: exact, any order).
//   kmeans_update   every cluster's three coordinate sums and its count along the fixed tree of vfn_tree.h, lane order "near", over the
//                   values label[i] == j ? p[i,c] : +0.0.  A workgroup owns a tile of 4096 points, reads each ONCE into registers and walks
//                   the clusters; a cluster that no point of the tile names gets its partial, +0.0, without a tree (a tree of +0.0 is
//                   +0.0: the same bits).  The count rides along as a double, as vfn_icp_accumulate's: sums of ones below 2^53 are exact.
//   kmeans_seed     one step of farthest-point / D^2 seeding without a host read: mind2 = min(mind2, d2 to the newest seed), whose index
//                   is read from device memory, and the index of the largest mind2 (ties to the LOWEST index).  A maximum under a total
//                   order is associative and commutative: any two-level reduction gives these bits, so this one names no tree.
// All arithmetic fp64 with -ffp-contract=off (build.sh), no floating-point atomics: every output bit is a function of the data alone.
#include "vfn_common.h"
#include "vfn_tree.h"
#include <math.h>

namespace {

constexpr int KM_BLOCK = 256;
constexpr int KM_MAX_K = VFN_KMEANS_MAX_K;
constexpr int KM_C = 4;                                                            // x, y, z sums and the count of one cluster

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

__global__ __launch_bounds__(KM_BLOCK) void vfn_kmeans_assign_kernel(const double* __restrict__ p, long long n, const double* __restrict__ centres, int k,
                                                                     const int* previous, int* label, double* __restrict__ sqdist,
                                                                     unsigned long long* __restrict__ changed, unsigned long long* __restrict__ info) {
    __shared__ double c[3 * KM_MAX_K];
    __shared__ unsigned int differ;
    const int l = threadIdx.x;
    if (l < 3 * k) {
        c[l] = centres[l];
        if (blockIdx.x == 0 && !isfinite(c[l])) atomicOr(info, 1ull);
    }
    if (l == 0) differ = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * KM_BLOCK + l;
    bool moved = false;
    if (i < n) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicOr(info, 1ull);
        double best = vfn_pair_sqdist(x, y, z, c[0], c[1], c[2]);
        int bj = 0;
        for (int j = 1; j < k; ++j) {
            const double d2 = vfn_pair_sqdist(x, y, z, c[3 * j], c[3 * j + 1], c[3 * j + 2]);
            if (d2 < best) { best = d2; bj = j; }                                  // strict: a tie stays with the lower cluster
        }
        moved = previous ? previous[i] != bj : true;                              // (read before label[i] is written: they may be one array)
        label[i] = bj;
        sqdist[i] = best;
    }
    const unsigned long long wave = __ballot(moved);
    if ((l & 63) == 0 && wave) atomicAdd(&differ, (unsigned)__popcll(wave));
    __syncthreads();
    if (l == 0 && differ) atomicAdd(changed, (unsigned long long)differ);
}

using Acc = TreeSum<KM_C>;

// first level: block b owns the points [4096 b, 4096 (b + 1)); lane l holds the points l + 256 s, s < 16, in registers.  For every
// cluster the lane tree ("near") over the lane's slots, then the block tree; partials[(b k + j) 4 + c].
__global__ __launch_bounds__(TREE_LANES) void vfn_kmeans_update_kernel(const double* __restrict__ p, long long n, const int* __restrict__ label, int k,
                                                                       double* __restrict__ partials, unsigned long long* __restrict__ info) {
    __shared__ Acc sh[TREE_LANES];
    __shared__ unsigned long long present;
    const int l = threadIdx.x;
    if (l == 0) present = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * TREE_TILE + l;
    double x[TREE_PER], y[TREE_PER], z[TREE_PER];
    int lab[TREE_PER];
    unsigned long long mine = 0;
    bool bad_label = false, bad_point = false;
#pragma unroll
    for (int s = 0; s < TREE_PER; ++s) {
        const long long i = base + (long long)s * TREE_LANES;
        lab[s] = -1;                                                               // a slot past n, or with a bad label, joins no cluster
        x[s] = y[s] = z[s] = 0.0;
        if (i < n) {
            const int q = label[i];
            if (q < 0 || q >= k) { bad_label = true; continue; }
            lab[s] = q;
            x[s] = p[3 * i]; y[s] = p[3 * i + 1]; z[s] = p[3 * i + 2];
            bad_point = bad_point || !(isfinite(x[s]) && isfinite(y[s]) && isfinite(z[s]));
            mine |= 1ull << q;
        }
    }
    if (bad_label) atomicOr(info, 2ull);
    if (bad_point) atomicOr(info, 1ull);
    if (mine) atomicOr(&present, mine);
    __syncthreads();
    const unsigned long long here = present;
    for (int j = 0; j < k; ++j) {
        double* out = partials + ((long long)blockIdx.x * k + j) * KM_C;
        if (!((here >> j) & 1ull)) {                                               // uniform over the block
            if (l < KM_C) out[l] = 0.0;
            continue;
        }
        const Acc a = tree_lane<TREE_PER, Acc>([&](int s) {
            const bool in = lab[s] == j;
            Acc r;
            r.v[0] = in ? x[s] : 0.0; r.v[1] = in ? y[s] : 0.0; r.v[2] = in ? z[s] : 0.0; r.v[3] = in ? 1.0 : 0.0;
            return r;
        }, TreeAdd());
        tree_block<TREE_LANES>(a, sh, TreeAdd());
        if (l < KM_C) out[l] = sh[0].v[l];
        __syncthreads();                                                           // the next cluster overwrites sh
    }
}

// second level, one block per cluster over its P partials; the block tree one component after the other through the same 1024 doubles.
// Lane 0 finishes: the count as an integer, the centre where the cluster has points.
__global__ __launch_bounds__(TREE_TOP) void vfn_kmeans_update_top_kernel(const double* __restrict__ partials, long long tiles, int k, double* __restrict__ sums,
                                                                         long long* __restrict__ count, double* __restrict__ centres) {
    __shared__ double sh[TREE_TOP];
    const int j = blockIdx.x;
    Acc zero;
#pragma unroll
    for (int c = 0; c < KM_C; ++c) zero.v[c] = 0.0;
    const Acc s = tree_top_lane(tiles, zero, [&](long long b) {
        Acc r;
#pragma unroll
        for (int c = 0; c < KM_C; ++c) r.v[c] = partials[(b * k + j) * KM_C + c];
        return r;
    }, TreeAdd());
    double total[KM_C];
#pragma unroll
    for (int c = 0; c < KM_C; ++c) {
        total[c] = tree_block<TREE_TOP>(s.v[c], sh, TreeAdd());
        __syncthreads();                                                           // the next component overwrites sh
    }
    if (threadIdx.x == 0) {
        const long long m = (long long)total[3];
        count[j] = m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sums[3 * j + c] = total[c];
            if (m > 0) centres[3 * j + c] = total[c] / (double)m;                  // an empty cluster keeps its centre's bits
        }
    }
}

// the maximum of (value, index): the greater value, of equal values the lower index; (-1, -1) where there is nothing (a d2 is >= 0)
struct Far { double v; long long i; };

struct FarJoin {
    __device__ __forceinline__ Far operator()(const Far& a, const Far& b) const { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
};

__device__ __forceinline__ bool seed_index(const long long* newest, long long n, long long* q) {
    *q = newest ? *newest : 0;
    return !newest || (*q >= 0 && *q < n);
}

// a lane takes the 16 points l + 256 s of its tile; the block's maximum goes to part[b]
__global__ __launch_bounds__(TREE_LANES) void vfn_kmeans_seed_kernel(const double* __restrict__ p, long long n, const long long* __restrict__ newest, int first,
                                                                     double* __restrict__ mind2, Far* __restrict__ part, unsigned long long* __restrict__ info) {
    __shared__ Far sh[TREE_LANES];
    const int l = threadIdx.x;
    long long q;
    if (!seed_index(newest, n, &q)) {                                              // nothing is read through a bad index; mind2 stays
        if (blockIdx.x == 0 && l == 0) atomicOr(info, 2ull);
        return;
    }
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (newest) { cx = p[3 * q]; cy = p[3 * q + 1]; cz = p[3 * q + 2]; }
    Far best = {-1.0, -1};
    bool bad = false;
    for (int s = 0; s < TREE_PER; ++s) {
        const long long i = (long long)blockIdx.x * TREE_TILE + l + (long long)s * TREE_LANES;
        if (i >= n) break;
        double d = 0.0;
        if (newest) {
            const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
            bad = bad || !(isfinite(x) && isfinite(y) && isfinite(z));
            d = vfn_pair_sqdist(x, y, z, cx, cy, cz);
            if (!first) { const double old = mind2[i]; d = old < d ? old : d; }
            mind2[i] = d;
        } else {
            d = mind2[i];
        }
        if (part) best = FarJoin()(best, Far{d, i});
    }
    if (bad) atomicOr(info, 1ull);
    if (!part) return;                                                             // uniform: the caller wants no maximum
    tree_block<TREE_LANES>(best, sh, FarJoin());
    if (l == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(TREE_TOP) void vfn_kmeans_seed_top_kernel(const Far* __restrict__ part, long long tiles, const long long* __restrict__ newest,
                                                                       long long n, long long* __restrict__ farthest) {
    __shared__ Far sh[TREE_TOP];
    long long q;
    if (!seed_index(newest, n, &q)) {
        if (threadIdx.x == 0) *farthest = -1;
        return;
    }
    const Far s = tree_top_lane(tiles, Far{-1.0, -1}, [&](long long b) { return part[b]; }, FarJoin());
    tree_block<TREE_TOP>(s, sh, FarJoin());
    if (threadIdx.x == 0) *farthest = sh[0].i;
}

bool sizes_ok(int64_t n, int32_t k) { return n >= 1 && n < (1ll << 31) && k >= 1 && k <= KM_MAX_K; }

}  // namespace

extern "C" int vfn_kmeans_assign(const double* points, int64_t n, const double* centres, int32_t k, const int32_t* previous, int32_t* label,
                                 double* sqdist, int64_t* changed, int64_t* info, void* stream) {
    VFN_REQUIRE(sizes_ok(n, k), "vfn_kmeans_assign: n %lld outside [1, 2^31) or k %d outside [1, %d]", (long long)n, k, KM_MAX_K);
    VFN_REQUIRE(points && centres && label && sqdist && changed && info, "vfn_kmeans_assign: NULL argument");
    hipLaunchKernelGGL(vfn_kmeans_assign_kernel, dim3(blocks_for(n, KM_BLOCK)), dim3(KM_BLOCK), 0, (hipStream_t)stream, points, (long long)n, centres, (int)k,
                       (const int*)previous, (int*)label, sqdist, (unsigned long long*)changed, (unsigned long long*)info);
    return vfn_check_launch("vfn_kmeans_assign");
}

extern "C" int64_t vfn_kmeans_update_workspace_bytes(int64_t n, int32_t k) {
    if (!sizes_ok(n, k)) {
        vfn_set_error("vfn_kmeans_update_workspace_bytes: n %lld outside [1, 2^31) or k %d outside [1, %d]", (long long)n, k, KM_MAX_K);
        return -1;
    }
    return (int64_t)(tree_tiles(n) * k * KM_C * sizeof(double));
}

extern "C" int vfn_kmeans_update(const double* points, int64_t n, const int32_t* label, int32_t k, double* sums, int64_t* count, double* centres,
                                 int64_t* info, void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t need = vfn_kmeans_update_workspace_bytes(n, k);
    if (need < 0) return VFN_ERR_INVALID;
    VFN_REQUIRE(points && label && sums && count && centres && info && workspace && workspace_bytes >= need,
                "vfn_kmeans_update: NULL argument or a workspace of %lld bytes < %lld", (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const long long tiles = tree_tiles(n);
    hipLaunchKernelGGL(vfn_kmeans_update_kernel, dim3((unsigned)tiles), dim3(TREE_LANES), 0, s, points, (long long)n, (const int*)label, (int)k,
                       (double*)workspace, (unsigned long long*)info);
    hipLaunchKernelGGL(vfn_kmeans_update_top_kernel, dim3((unsigned)k), dim3(TREE_TOP), 0, s, (const double*)workspace, tiles, (int)k, sums,
                       (long long*)count, centres);
    return vfn_check_launch("vfn_kmeans_update");
}

extern "C" int64_t vfn_kmeans_seed_workspace_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) {
        vfn_set_error("vfn_kmeans_seed_workspace_bytes: n %lld outside [1, 2^31)", (long long)n);
        return -1;
    }
    return (int64_t)(tree_tiles(n) * sizeof(Far));
}

extern "C" int vfn_kmeans_seed(const double* points, int64_t n, const int64_t* newest, int32_t first, double* mind2, int64_t* farthest,
                               int64_t* info, void* workspace, int64_t workspace_bytes, void* stream) {
    const int64_t need = vfn_kmeans_seed_workspace_bytes(n);
    if (need < 0) return VFN_ERR_INVALID;
    VFN_REQUIRE(points && mind2 && info && (newest || farthest), "vfn_kmeans_seed: NULL argument (newest and farthest may be NULL, not both)");
    VFN_REQUIRE(!farthest || (workspace && workspace_bytes >= need), "vfn_kmeans_seed: no workspace, or one of %lld bytes < %lld",
                (long long)workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const long long tiles = tree_tiles(n);
    hipLaunchKernelGGL(vfn_kmeans_seed_kernel, dim3((unsigned)tiles), dim3(TREE_LANES), 0, s, points, (long long)n, (const long long*)newest, (int)first,
                       mind2, farthest ? (Far*)workspace : (Far*)nullptr, (unsigned long long*)info);
    if (farthest)
        hipLaunchKernelGGL(vfn_kmeans_seed_top_kernel, dim3(1), dim3(TREE_TOP), 0, s, (const Far*)workspace, tiles, (const long long*)newest, (long long)n,
                           (long long*)farthest);
    return vfn_check_launch("vfn_kmeans_seed");
}
