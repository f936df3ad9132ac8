// vfn_orient.hip — a consistent winding for a triangle mesh (vf_nerf_amd/meshops.py: orientation, orient): the contrastive marching-cubes
// mesh chooses every cell's sides locally, so neighbouring faces often traverse their shared edge the same way.  A specification of ours
// (include/vfn.h), not verified against trimesh's fix_normals or Open3D's orient_triangles.
//   orient_union_runs  one lane per item of the sorted half-edge list: a run of exactly two equal keys from two faces unites them in an
//                      int32 forest whose words hold (parent << 1) | parity — a concurrent PARITY union-find (csrc/vfn_forest_core.h has
//                      the loops, the invariant, the termination argument and why neither the partition nor an orientable component's
//                      parities depend on the schedule).  Bound by the latency of dependent loads and compare-and-swaps on the forest,
//                      not by bandwidth: 17 bytes per item are streamed (and its two neighbours' keys re-read from cache), the forest
//                      words are gathered.
//   orient_flatten     one lane per node, after the unions: where its chain ends and the XOR of the parities along it.  Reads the forest,
//                      writes two other arrays: no races.
//   orient_votes       one lane per face: its vote for the sign of its component (six times its signed volume against the origin, or
//                      its normal against the direction to the nearest viewpoint).  The sums are vfn_cc_segment_sums'.
// The forest is re-read only through DeviceMem's relaxed agent-scope atomic load (csrc/vfn_geom.h has the load and why relaxed is
// enough: parent and parity travel in one word, and nothing else is published through it).  All arithmetic of
// the votes is fp64 with -ffp-contract=off (build.sh).  No floating-point atomics.  No node, parent or vertex index reaches memory
// before it has been compared with its range; no kernel returns before its wave's status report, and a wave ORs its status bits into
// info[0] with at most one atomic (report() of csrc/vfn_geom.h).
#include "vfn_common.h"
#include "vfn_forest_core.h"

namespace {

using namespace vfn_geom;

constexpr int OR_BLOCK = 256;

__global__ __launch_bounds__(256) void vfn_orient_union_runs_kernel(const long long* __restrict__ keys, const long long* __restrict__ nodes,
                                                                    const unsigned char* __restrict__ dirs, long long n_items, int* forest,
                                                                    long long n_nodes, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i >= 1 && i < n_items) status = vfn_forest::union_item<DeviceMem>(keys, nodes, dirs, i, n_items, forest, n_nodes);
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_orient_flatten_kernel(const int* forest, long long n_nodes, long long* __restrict__ root,
                                                                 unsigned char* __restrict__ parity, unsigned long long* __restrict__ info) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (v < n_nodes) {
        const vfn_forest::Found e = vfn_forest::chain_end<DeviceMem, 1>(forest, (int)v, &status);
        root[v] = (long long)e.root;
        parity[v] = (unsigned char)e.parity;
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_orient_votes_kernel(const double* __restrict__ v, long long n, const long long* __restrict__ f, long long m,
                                                               const unsigned char* __restrict__ parity, int mode,
                                                               const double* __restrict__ views, long long n_views, double* __restrict__ votes,
                                                               unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < m) {
        const long long i0 = f[3 * i];
        long long i1 = f[3 * i + 1], i2 = f[3 * i + 2];
        double t = 0.0;
        if (i0 < 0 || i0 >= n || i1 < 0 || i1 >= n || i2 < 0 || i2 >= n) {
            status |= ST_RANGE;
        } else {
            if (parity && parity[i]) { const long long s = i1; i1 = i2; i2 = s; }
            const double p0[3] = {v[3 * i0], v[3 * i0 + 1], v[3 * i0 + 2]};
            const double p1[3] = {v[3 * i1], v[3 * i1 + 1], v[3 * i1 + 2]};
            const double p2[3] = {v[3 * i2], v[3 * i2 + 1], v[3 * i2 + 2]};
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) fin = fin && isfinite(p0[k]) && isfinite(p1[k]) && isfinite(p2[k]);
            if (mode == VFN_ORIENT_VOLUME) {
                const double c[3] = {p1[1] * p2[2] - p1[2] * p2[1], p1[2] * p2[0] - p1[0] * p2[2], p1[0] * p2[1] - p1[1] * p2[0]};
                t = (p0[0] * c[0] + p0[1] * c[1]) + p0[2] * c[2];
            } else {
                const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
                const double b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
                const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                const double g[3] = {((p0[0] + p1[0]) + p2[0]) / 3.0, ((p0[1] + p1[1]) + p2[1]) / 3.0, ((p0[2] + p1[2]) + p2[2]) / 3.0};
                double best = 0.0, d[3] = {0.0, 0.0, 0.0};
                for (long long j = 0; j < n_views; ++j) {          // every lane reads the same viewpoint: one address per step
                    const double e[3] = {views[3 * j] - g[0], views[3 * j + 1] - g[1], views[3 * j + 2] - g[2]};
                    const double s = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
                    fin = fin && isfinite(views[3 * j]) && isfinite(views[3 * j + 1]) && isfinite(views[3 * j + 2]);
                    if (j == 0 || s < best) { best = s; d[0] = e[0]; d[1] = e[1]; d[2] = e[2]; }
                }
                t = best == 0.0 ? 0.0 : ((c[0] * d[0] + c[1] * d[1]) + c[2] * d[2]) / sqrt(best);
            }
            if (!fin) status |= ST_NONFINITE;
        }
        votes[i] = t;
    }
    report(status, info);
}

}  // namespace

extern "C" int vfn_orient_union_runs(const int64_t* keys, const int64_t* nodes, const uint8_t* dirs, int64_t n_items, int32_t* forest,
                                     int64_t n_nodes, int64_t* info, void* stream) {
    VFN_REQUIRE(n_nodes >= 1 && n_nodes < (1ll << 30), "vfn_orient_union_runs: n_nodes %lld outside [1, 2^30)", (long long)n_nodes);
    VFN_REQUIRE(n_items >= 1 && n_items < (3ll << 30), "vfn_orient_union_runs: n_items %lld outside [1, 3 * 2^30)", (long long)n_items);
    VFN_REQUIRE(keys && nodes && dirs && forest && info, "vfn_orient_union_runs: NULL argument");
    hipLaunchKernelGGL(vfn_orient_union_runs_kernel, dim3(blocks_for(n_items)), dim3(OR_BLOCK), 0, (hipStream_t)stream, (const long long*)keys,
                       (const long long*)nodes, (const unsigned char*)dirs, (long long)n_items, (int*)forest, (long long)n_nodes,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_orient_union_runs");
}

extern "C" int vfn_orient_flatten(const int32_t* forest, int64_t n_nodes, int64_t* root, uint8_t* parity, int64_t* info, void* stream) {
    VFN_REQUIRE(n_nodes >= 1 && n_nodes < (1ll << 30), "vfn_orient_flatten: n_nodes %lld outside [1, 2^30)", (long long)n_nodes);
    VFN_REQUIRE(forest && root && parity && info, "vfn_orient_flatten: NULL argument");
    hipLaunchKernelGGL(vfn_orient_flatten_kernel, dim3(blocks_for(n_nodes)), dim3(OR_BLOCK), 0, (hipStream_t)stream, (const int*)forest,
                       (long long)n_nodes, (long long*)root, (unsigned char*)parity, (unsigned long long*)info);
    return vfn_check_launch("vfn_orient_flatten");
}

extern "C" int vfn_orient_votes(const double* vertices, int64_t n, const int64_t* faces, int64_t m, const uint8_t* parity, int32_t mode,
                                const double* viewpoints, int64_t n_views, double* votes, int64_t* info, void* stream) {
    VFN_REQUIRE(n >= 0 && n < (1ll << 31), "vfn_orient_votes: n %lld outside [0, 2^31)", (long long)n);
    VFN_REQUIRE(m >= 1 && m < (1ll << 31), "vfn_orient_votes: m %lld outside [1, 2^31)", (long long)m);
    VFN_REQUIRE(mode == VFN_ORIENT_VOLUME || mode == VFN_ORIENT_VIEWPOINTS, "vfn_orient_votes: mode %d is not VFN_ORIENT_VOLUME or VFN_ORIENT_VIEWPOINTS",
                (int)mode);
    if (mode == VFN_ORIENT_VIEWPOINTS) {
        VFN_REQUIRE(n_views >= 1 && n_views < (1ll << 31), "vfn_orient_votes: n_views %lld outside [1, 2^31)", (long long)n_views);
        VFN_REQUIRE(viewpoints, "vfn_orient_votes: NULL viewpoints");
    } else {
        VFN_REQUIRE(n_views == 0 && !viewpoints, "vfn_orient_votes: viewpoints given (n_views %lld) to VFN_ORIENT_VOLUME", (long long)n_views);
    }
    VFN_REQUIRE(faces && votes && info && (vertices || n == 0), "vfn_orient_votes: NULL argument");
    hipLaunchKernelGGL(vfn_orient_votes_kernel, dim3(blocks_for(m)), dim3(OR_BLOCK), 0, (hipStream_t)stream, vertices, (long long)n,
                       (const long long*)faces, (long long)m, (const unsigned char*)parity, (int)mode, viewpoints, (long long)n_views, votes,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_orient_votes");
}
