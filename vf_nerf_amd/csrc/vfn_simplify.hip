// vfn_simplify.hip — vertex-clustering simplification of a triangle mesh (vf_nerf_amd/meshops.py: simplify_vertex_clustering): the part
// that the voxel unit does not already give — every cluster's vertex placed at the minimiser of its faces' plane quadrics, so that
// corners and creases survive the contraction.  A specification of ours that follows Open3D's simplify_vertex_clustering (Quadric) as
// remembered (include/vfn.h).
//   face_planes       one lane per face: the unit normal, the plane's offset from the frame's origin and the area.  A gather kernel
//                     like vfn_face_normals: three rows of 24 bytes read at scattered addresses, 40 contiguous bytes written per face.
//   cluster_quadrics  one WAVE per cluster: lane t turns the items t, t + 64, ... of the cluster's segment into their ten numbers and
//                     adds them serially from its first item; the 64 partial sums of every channel fold as s[t] += s[t + 32], then 16,
//                     8, 4, 2, 1 (vfn_cc_segment_sums' rule); lane 0 solves the 3 x 3 system by the adjugate (csrc/vfn_quadric.h), tests
//                     the minimiser and writes.  Per item 8 bytes of the table and a gathered row of 40 bytes; a cluster of a marching-cubes mesh holds
//                     a few dozen items, so most lanes of a wave idle and the kernel is bound by the latency of the two dependent
//                     loads (the face index, then its plane), not by bandwidth.
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.  No floating-point
// atomics, no LDS, no bit depends on the schedule.  Nothing is read through a segment bound or a face index before it has been compared
// with its range; no kernel returns before its wave's status report, and a wave ORs its status bits into info[0] with at most one
// atomic (report() of csrc/vfn_geom.h).
#include "vfn_common.h"
#include "vfn_geom.h"
#include "vfn_quadric.h"

namespace {

using namespace vfn_geom;
using vfn_quadric::CHANNELS;

constexpr int SIM_BLOCK = 256;
constexpr int WAVE = 64;

__global__ __launch_bounds__(256) void vfn_face_planes_kernel(const double* __restrict__ v, long long n, const long long* __restrict__ f, long long m,
                                                              double ox, double oy, double oz, double* __restrict__ planes,
                                                              unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < m) {
        const long long i0 = f[3 * i], i1 = f[3 * i + 1], i2 = f[3 * i + 2];
        double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (i0 < 0 || i0 >= n || i1 < 0 || i1 >= n || i2 < 0 || i2 >= n) {
            status |= ST_INDEX;
        } else {
            const double p0[3] = {v[3 * i0], v[3 * i0 + 1], v[3 * i0 + 2]};
            const double p1[3] = {v[3 * i1], v[3 * i1 + 1], v[3 * i1 + 2]};
            const double p2[3] = {v[3 * i2], v[3 * i2 + 1], v[3 * i2 + 2]};
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) fin = fin && isfinite(p0[k]) && isfinite(p1[k]) && isfinite(p2[k]);
            if (!fin) status |= ST_NONFINITE;
            const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
            const double b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
            const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
            double r;
            if (unit_vector(c, o, &r, status)) {
                o[3] = plane_offset(o, p0, ox, oy, oz);
                o[4] = 0.5 * r;
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) planes[5 * i + k] = o[k];
    }
    report(status, info);
}

// the ten numbers of one item: the plane (nrm, e, w) seen from the cell centre, u = g - origin
__device__ __forceinline__ void item_numbers(const double* __restrict__ row, const double u[3], double q[CHANNELS]) {
    const double nx = row[0], ny = row[1], nz = row[2], e = row[3], w = row[4];
    double d = nx * u[0];
    d = d + ny * u[1];
    d = d + nz * u[2];
    d = d - e;
    const double wx = w * nx, wy = w * ny, wz = w * nz, wd = w * d;
    q[0] = wx * nx; q[1] = wx * ny; q[2] = wx * nz; q[3] = wy * ny; q[4] = wy * nz; q[5] = wz * nz;
    q[6] = wd * nx; q[7] = wd * ny; q[8] = wd * nz;
    q[9] = wd * d;
}

__global__ __launch_bounds__(256) void vfn_cluster_quadrics_kernel(const double* __restrict__ planes, long long m, const long long* __restrict__ item_face,
                                                                   long long n_items, const long long* __restrict__ start, long long n_clusters,
                                                                   const double* __restrict__ centres, const double* __restrict__ means, double ox,
                                                                   double oy, double oz, double h, double rcond, double* __restrict__ position,
                                                                   unsigned char* __restrict__ placed, double* __restrict__ error,
                                                                   unsigned long long* __restrict__ info) {
    const long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;          // the same for every lane of a wave
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    unsigned status = 0;
    if (q < n_clusters) {
        const long long b = start[q], e = start[q + 1];
        const double g[3] = {centres[3 * q], centres[3 * q + 1], centres[3 * q + 2]};
        const double u[3] = {g[0] - ox, g[1] - oy, g[2] - oz};
        double s[CHANNELS];
#pragma unroll
        for (int c = 0; c < CHANNELS; ++c) s[c] = 0.0;                  // a lane without items holds +0.0
        bool bad = b < 0 || e <= b || e > n_items;
        if (!bad) {
            for (long long j = b + lane; j < e; j += WAVE) {
                const long long face = item_face[j];
                if (face < 0 || face >= m) { bad = true; break; }
                double t[CHANNELS];
                item_numbers(planes + 5 * face, u, t);
                if (j < b + WAVE) {                                    // started from the lane's first item
#pragma unroll
                    for (int c = 0; c < CHANNELS; ++c) s[c] = t[c];
                } else {
#pragma unroll
                    for (int c = 0; c < CHANNELS; ++c) s[c] = s[c] + t[c];
                }
            }
        }
        bad = __ballot(bad) != 0ull;                                    // one bad item spoils its cluster, for every lane alike
#pragma unroll
        for (int c = 0; c < CHANNELS; ++c)
            for (int o = WAVE / 2; o > 0; o >>= 1) s[c] = s[c] + __shfl_down(s[c], (unsigned)o, WAVE);          // s[t] += s[t + o] for t < o
        if (lane == 0) {
            double out[3], err;
            unsigned char ok = 0;
            if (bad) {
                status |= ST_INDEX;
                out[0] = out[1] = out[2] = err = __builtin_nan("");
            } else {
                const vfn_quadric::Minimiser mn = vfn_quadric::minimiser(s);
                const double* x = mn.x;
                const double half = 0.5 * h;
                // (every comparison is false on a NaN)
                const bool accepted = mn.det > rcond * ((mn.t * mn.t) * mn.t) && fabs(x[0]) <= half && fabs(x[1]) <= half && fabs(x[2]) <= half;
                double z[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double mean = means[3 * q + k];
                    out[k] = accepted ? g[k] + x[k] : mean;
                    z[k] = accepted ? x[k] : mean - g[k];
                }
                err = vfn_quadric::value_at(s, z);
                ok = accepted ? 1 : 0;
            }
            position[3 * q] = out[0]; position[3 * q + 1] = out[1]; position[3 * q + 2] = out[2];
            placed[q] = ok;
            error[q] = err;
        }
    }
    report(status, info);
}

bool count_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }

}  // namespace

extern "C" int vfn_face_planes(const double* vertices, int64_t n, const int64_t* faces, int64_t m, const double* origin, double* planes, int64_t* info,
                               void* stream) {
    VFN_REQUIRE(count_ok(n), "vfn_face_planes: n %lld outside [0, 2^31)", (long long)n);
    VFN_REQUIRE(m >= 1 && m < (1ll << 31), "vfn_face_planes: m %lld outside [1, 2^31)", (long long)m);
    VFN_REQUIRE(faces && origin && planes && info && (vertices || n == 0), "vfn_face_planes: NULL argument");
    VFN_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "vfn_face_planes: a non-finite origin");
    hipLaunchKernelGGL(vfn_face_planes_kernel, dim3(blocks_for(m)), dim3(SIM_BLOCK), 0, (hipStream_t)stream, vertices, (long long)n,
                       (const long long*)faces, (long long)m, origin[0], origin[1], origin[2], planes, (unsigned long long*)info);
    return vfn_check_launch("vfn_face_planes");
}

extern "C" int vfn_cluster_quadrics(const double* planes, int64_t m, const int64_t* item_face, int64_t n_items, const int64_t* start,
                                    int64_t n_clusters, const double* centres, const double* means, const double* origin, double voxel_size,
                                    double rcond, double* position, uint8_t* placed, double* error, int64_t* info, void* stream) {
    VFN_REQUIRE(m >= 1 && m < (1ll << 31), "vfn_cluster_quadrics: m %lld outside [1, 2^31)", (long long)m);
    VFN_REQUIRE(n_items >= 1 && n_items < (3ll << 31), "vfn_cluster_quadrics: n_items %lld outside [1, 3 * 2^31)", (long long)n_items);
    VFN_REQUIRE(n_clusters >= 1 && n_clusters <= n_items && n_clusters < (1ll << 31),
                "vfn_cluster_quadrics: n_clusters %lld outside [1, min(n_items = %lld, 2^31 - 1)]", (long long)n_clusters, (long long)n_items);
    VFN_REQUIRE(planes && item_face && start && centres && means && origin && position && placed && error && info,
                "vfn_cluster_quadrics: NULL argument");
    VFN_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "vfn_cluster_quadrics: a non-finite origin");
    VFN_REQUIRE(isfinite(voxel_size) && voxel_size > 0.0 && isfinite(voxel_size * voxel_size) && voxel_size * voxel_size >= 2.2250738585072014e-308,
                "vfn_cluster_quadrics: voxel_size %g is not finite and > 0 with a normal square", voxel_size);
    VFN_REQUIRE(isfinite(rcond) && rcond >= 0.0 && rcond <= 1.0, "vfn_cluster_quadrics: rcond %g outside [0, 1]", rcond);
    hipLaunchKernelGGL(vfn_cluster_quadrics_kernel, dim3(blocks_for(n_clusters * WAVE)), dim3(SIM_BLOCK), 0, (hipStream_t)stream, planes,
                       (long long)m, (const long long*)item_face, (long long)n_items, (const long long*)start, (long long)n_clusters, centres,
                       means, origin[0], origin[1], origin[2], voxel_size, rcond, position, (unsigned char*)placed, error,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_cluster_quadrics");
}
