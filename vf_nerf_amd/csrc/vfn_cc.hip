// vfn_cc.hip — connected components of a triangle mesh (vf_nerf_amd/meshops.py: connected_components, filter_components): what a fused
// mesh consists of, so that its floaters can be culled before it is scored.  A specification of ours that follows Open3D's
// cluster_connected_triangles and trimesh's split as remembered (include/vfn.h).
//   cc_union_runs    one lane per item of a sorted key list: equal neighbouring keys unite their two nodes in an int32 forest — a
//                    concurrent union-find (csrc/vfn_forest_core.h has the loops, the invariant, the termination argument and why the
//                    result does not depend on the schedule).  Bound by the latency of dependent loads and compare-and-swaps on the
//                    forest, not by bandwidth: 16 bytes per item are streamed, the forest words are gathered.
//   cc_flatten       one lane per node, after the unions: where its parent chain ends.  Reads the forest, writes another array: no races.
//   cc_segment_sums  one WAVE per segment: lane t adds elements t, t + 64, ... serially from its first one, the 64 partial sums fold as
//                    s[t] += s[t + 32], then 16, 8, 4, 2, 1.  A wave reads 512 contiguous bytes per step.
// The forest is re-read only through DeviceMem's relaxed agent-scope atomic load (csrc/vfn_geom.h has the load and why relaxed is enough).
// All arithmetic of the sums is fp64 with -ffp-contract=off (build.sh).  No floating-point atomics.  No
// node, parent or segment bound indexes memory before it has been compared with its range; no kernel returns before its wave's status
// report, and a wave ORs its status bits into info[0] with at most one atomic (report() of csrc/vfn_geom.h).
#include "vfn_common.h"
#include "vfn_forest_core.h"

namespace {

using namespace vfn_geom;

constexpr int CC_BLOCK = 256;
constexpr int WAVE = 64;
constexpr int SUM_AHEAD = 16;            // loads in flight per lane of cc_segment_sums (speed only: the order of the additions is the header's)

__global__ __launch_bounds__(256) void vfn_cc_union_runs_kernel(const long long* __restrict__ keys, const long long* __restrict__ nodes,
                                                                long long n_items, int* parent, long long n_nodes,
                                                                unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i >= 1 && i < n_items) status = vfn_forest::union_item<DeviceMem>(keys, nodes, i, parent, n_nodes);
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_cc_flatten_kernel(const int* parent, long long n_nodes, long long* __restrict__ root,
                                                             unsigned long long* __restrict__ info) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (v < n_nodes) root[v] = (long long)vfn_forest::chain_end<DeviceMem, 0>(parent, (int)v, &status).root;
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_cc_segment_sums_kernel(const double* __restrict__ x, long long n, const long long* __restrict__ start,
                                                                  long long n_segments, double* __restrict__ sums,
                                                                  unsigned long long* __restrict__ info) {
    const long long seg = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;          // the same for every lane of a wave
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    unsigned status = 0;
    if (seg < n_segments) {
        const long long b = start[seg], e = start[seg + 1];
        double s = 0.0;                                        // a lane without elements holds +0.0
        if (b < 0 || e <= b || e > n) {
            status |= ST_RANGE;
            s = __builtin_nan("");
        } else {
            long long j = b + lane;
            if (j < e) {
                s = x[j];                                      // started from the lane's first element
                j += WAVE;
                // SUM_AHEAD loads are issued before the first of them is added: they do not depend on the running sum, and one wave
                // walking a 2 x 10^6-value segment a load at a time waits a memory latency per step.  The additions keep their order.
                for (; j + (SUM_AHEAD - 1) * WAVE < e; j += SUM_AHEAD * WAVE) {
                    double ahead[SUM_AHEAD];
#pragma unroll
                    for (int q = 0; q < SUM_AHEAD; ++q) ahead[q] = x[j + q * WAVE];
#pragma unroll
                    for (int q = 0; q < SUM_AHEAD; ++q) s = s + ahead[q];
                }
                for (; j < e; j += WAVE) s = s + x[j];
            }
        }
        for (int o = WAVE / 2; o > 0; o >>= 1) s = s + __shfl_down(s, (unsigned)o, WAVE);          // s[t] += s[t + o] for t < o
        if (lane == 0) sums[seg] = s;
    }
    report(status, info);
}

}  // namespace

extern "C" int vfn_cc_union_runs(const int64_t* keys, const int64_t* nodes, int64_t n_items, int32_t* parent, int64_t n_nodes, int64_t* info,
                                 void* stream) {
    VFN_REQUIRE(n_nodes >= 1 && n_nodes < (1ll << 31), "vfn_cc_union_runs: n_nodes %lld outside [1, 2^31)", (long long)n_nodes);
    VFN_REQUIRE(n_items >= 1 && n_items < (3ll << 31), "vfn_cc_union_runs: n_items %lld outside [1, 3 * 2^31)", (long long)n_items);
    VFN_REQUIRE(keys && nodes && parent && info, "vfn_cc_union_runs: NULL argument");
    hipLaunchKernelGGL(vfn_cc_union_runs_kernel, dim3(blocks_for(n_items)), dim3(CC_BLOCK), 0, (hipStream_t)stream, (const long long*)keys,
                       (const long long*)nodes, (long long)n_items, (int*)parent, (long long)n_nodes, (unsigned long long*)info);
    return vfn_check_launch("vfn_cc_union_runs");
}

extern "C" int vfn_cc_flatten(const int32_t* parent, int64_t n_nodes, int64_t* root, int64_t* info, void* stream) {
    VFN_REQUIRE(n_nodes >= 1 && n_nodes < (1ll << 31), "vfn_cc_flatten: n_nodes %lld outside [1, 2^31)", (long long)n_nodes);
    VFN_REQUIRE(parent && root && info, "vfn_cc_flatten: NULL argument");
    hipLaunchKernelGGL(vfn_cc_flatten_kernel, dim3(blocks_for(n_nodes)), dim3(CC_BLOCK), 0, (hipStream_t)stream, (const int*)parent,
                       (long long)n_nodes, (long long*)root, (unsigned long long*)info);
    return vfn_check_launch("vfn_cc_flatten");
}

extern "C" int vfn_cc_segment_sums(const double* sorted_values, int64_t n, const int64_t* start, int64_t n_segments, double* sums, int64_t* info,
                                   void* stream) {
    VFN_REQUIRE(n >= 1 && n < (1ll << 31), "vfn_cc_segment_sums: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(n_segments >= 1 && n_segments <= n, "vfn_cc_segment_sums: n_segments %lld outside [1, n = %lld]", (long long)n_segments,
                (long long)n);
    VFN_REQUIRE(sorted_values && start && sums && info, "vfn_cc_segment_sums: NULL argument");
    hipLaunchKernelGGL(vfn_cc_segment_sums_kernel, dim3(blocks_for(n_segments * WAVE)), dim3(CC_BLOCK), 0, (hipStream_t)stream, sorted_values,
                       (long long)n, (const long long*)start, (long long)n_segments, sums, (unsigned long long*)info);
    return vfn_check_launch("vfn_cc_segment_sums");
}
