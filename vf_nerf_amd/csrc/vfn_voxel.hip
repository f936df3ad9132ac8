// vfn_voxel.hip — voxel down-sampling of a point set (vf_nerf_amd/voxel.py): the first step of the evaluate_3d_reconstruction protocol
// that the reference's metrics_3d calls.  A specification of ours that imitates Open3D's voxel_down_sample as remembered (include/vfn.h).
//   voxel_keys   one lane per point: c_k = floor((p_k - origin_k) / h), key = (c_0 << 42) | (c_1 << 21) | c_2.  A streaming kernel:
//                a wave reads 64 consecutive rows of 24 bytes (1536 contiguous bytes) and writes 512.  32 bytes per point.
//   voxel_means  one lane per voxel: the serial sum of its segment of the gathered rows in ascending position, started from the first
//                row, divided by the count.  Adjacent lanes read adjacent segments, so a wave's loads fall into one contiguous stretch
//                of about 64 x count rows; a segment is a handful of rows at the voxel sizes of the protocol.  The loads do not depend
//                on the running sum.  A voxel holding every point is walked by one lane: slow, and correct.
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.  No floating-point
// atomics, no LDS, no bit depends on the schedule.  No key indexes memory; a segment is followed only after both its bounds have been
// compared with [0, n].  The status bits of a wave are ORed into info[0] with at most one atomic per wave that saw a bad input
// (report() of csrc/vfn_geom.h).
#include "vfn_common.h"
#include "vfn_geom.h"

namespace {

using namespace vfn_geom;

constexpr int VOX_BLOCK = 256;
constexpr int AXIS_BITS = VFN_VOXEL_AXIS_BITS;
constexpr double AXIS_CELLS = (double)(1ll << AXIS_BITS);

__global__ __launch_bounds__(256) void vfn_voxel_keys_kernel(const double* __restrict__ p, long long n, double ox, double oy, double oz, double h,
                                                             long long* __restrict__ keys, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < n) {
        const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        long long key = -1;
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
            status |= ST_NONFINITE;
        } else {
            const double cx = floor((x - ox) / h), cy = floor((y - oy) / h), cz = floor((z - oz) / h);
            // (a NaN fails every comparison: it is out of range too)
            if (cx >= 0.0 && cx < AXIS_CELLS && cy >= 0.0 && cy < AXIS_CELLS && cz >= 0.0 && cz < AXIS_CELLS)
                key = ((long long)cx << (2 * AXIS_BITS)) | ((long long)cy << AXIS_BITS) | (long long)cz;
            else
                status |= ST_RANGE;
        }
        keys[i] = key;
    }
    report(status, info);
}

template <int C>
__global__ __launch_bounds__(256) void vfn_voxel_means_kernel(const double* __restrict__ x, long long n, const long long* __restrict__ start,
                                                              long long n_voxels, double* __restrict__ means,
                                                              unsigned long long* __restrict__ info) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (v < n_voxels) {
        const long long b = start[v], e = start[v + 1];
        double s[C];
        if (b < 0 || e <= b || e > n) {
            status |= ST_RANGE;
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] = __builtin_nan("");
        } else {
            const double* row = x + b * C;
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] = row[c];
            for (long long j = b + 1; j < e; ++j) {
                row += C;
#pragma unroll
                for (int c = 0; c < C; ++c) s[c] = s[c] + row[c];
            }
            const double count = (double)(e - b);
#pragma unroll
            for (int c = 0; c < C; ++c) s[c] = s[c] / count;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) means[v * C + c] = s[c];
    }
    report(status, info);
}

template <int C>
void launch_means(const double* x, long long n, const long long* start, long long n_voxels, double* means, unsigned long long* info,
                  hipStream_t stream) {
    hipLaunchKernelGGL(vfn_voxel_means_kernel<C>, dim3(blocks_for(n_voxels)), dim3(VOX_BLOCK), 0, stream, x, n, start, n_voxels, means, info);
}

bool count_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }

}  // namespace

extern "C" int vfn_voxel_keys(const double* points, int64_t n, const double* origin, double voxel_size, int64_t* keys, int64_t* info,
                              void* stream) {
    VFN_REQUIRE(count_ok(n), "vfn_voxel_keys: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(points && origin && keys && info, "vfn_voxel_keys: NULL argument");
    VFN_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "vfn_voxel_keys: a non-finite origin");
    VFN_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0 && isfinite(voxel_size * voxel_size) && voxel_size * voxel_size >= 2.2250738585072014e-308,
                "vfn_voxel_keys: voxel_size %g is not finite and > 0 with a normal square", voxel_size);
    hipLaunchKernelGGL(vfn_voxel_keys_kernel, dim3(blocks_for(n)), dim3(VOX_BLOCK), 0, (hipStream_t)stream, points, (long long)n, origin[0],
                       origin[1], origin[2], voxel_size, (long long*)keys, (unsigned long long*)info);
    return vfn_check_launch("vfn_voxel_keys");
}

extern "C" int vfn_voxel_means(const double* sorted_values, int64_t n, int32_t channels, const int64_t* start, int64_t n_voxels, double* means,
                               int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n), "vfn_voxel_means: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(channels >= 1 && channels <= VFN_VOXEL_MAX_CHANNELS, "vfn_voxel_means: channels %d outside [1, %d]", (int)channels,
                VFN_VOXEL_MAX_CHANNELS);
    VFN_REQUIRE(n_voxels >= 1 && n_voxels <= n, "vfn_voxel_means: n_voxels %lld outside [1, n = %lld]", (long long)n_voxels, (long long)n);
    VFN_REQUIRE(sorted_values && start && means && info, "vfn_voxel_means: NULL argument");
    const long long* st = (const long long*)start;
    unsigned long long* inf = (unsigned long long*)info;
    hipStream_t s = (hipStream_t)stream;
    switch (channels) {
        case 1: launch_means<1>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 2: launch_means<2>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 3: launch_means<3>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 4: launch_means<4>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 5: launch_means<5>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 6: launch_means<6>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 7: launch_means<7>(sorted_values, n, st, n_voxels, means, inf, s); break;
        case 8: launch_means<8>(sorted_values, n, st, n_voxels, means, inf, s); break;
        default: launch_means<9>(sorted_values, n, st, n_voxels, means, inf, s); break;
    }
    return vfn_check_launch("vfn_voxel_means");
}
