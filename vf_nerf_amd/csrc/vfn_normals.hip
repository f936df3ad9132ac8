// vfn_normals.hip — normals of a triangle mesh (vf_nerf_amd/meshops.py) and the dots of normal consistency (vf_nerf_amd/metrics3d.py):
// what the reference leaves to Open3D's compute_vertex_normals() before it writes tsdf.ply (evaluation/methods.py:664-665).
//   face_normals    one lane per face: the cross product of two edges (its length is twice the area), optionally made a unit vector.
//   vertex_normals  one lane per vertex: the unnormalised normals of its faces added in the order of its CSR row (ascending face, so the
//                   bits are a function of the mesh alone), then made a unit vector — area weighting.  A row averages six faces; a long
//                   row is slow (one lane walks it) and stays correct.
//   normal_dots     one lane per sample: |qn . tn[index]|.
// All arithmetic fp64 with -ffp-contract=off (build.sh): the expressions of include/vfn.h, operation for operation.  No floating-point
// atomics, no LDS, no bit depends on the schedule.  These are gather kernels: every lane reads rows of 24 bytes (three doubles or three
// int64) at scattered addresses, as three 8-byte loads — a row is 8-byte aligned, not 16.  Nothing is read through an index before the
// index has been compared with its range.  The status bits of a wave are ORed into info[0] with at most one atomic per wave that saw
// a bad input (report() of csrc/vfn_geom.h).
#include "vfn_common.h"
#include "vfn_geom.h"

namespace {

using namespace vfn_geom;

constexpr int NRM_BLOCK = 256;

// unit(c, fallback) of include/vfn.h
__device__ __forceinline__ void unit(const double c[3], double fx, double fy, double fz, double out[3], unsigned& status) {
    double r;
    if (!unit_vector(c, out, &r, status)) { out[0] = fx; out[1] = fy; out[2] = fz; }
}

__global__ __launch_bounds__(256) void vfn_face_normals_kernel(const double* __restrict__ v, long long n, const long long* __restrict__ f, long long m,
                                                               int normalise, double* __restrict__ out, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < m) {
        const long long i0 = f[3 * i], i1 = f[3 * i + 1], i2 = f[3 * i + 2];
        double o[3] = {0.0, 0.0, 0.0};
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
            if (normalise) {
                unit(c, 0.0, 0.0, 0.0, o, status);
            } else {
                o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
                if (fin && !(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) status |= ST_OVERFLOW;
            }
        }
        out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
    }
    report(status, info);
}

// nnz = row_start[n] is read on the device (one address for every lane); a row is followed only inside [0, nnz]
__global__ __launch_bounds__(256) void vfn_vertex_normals_kernel(const double* __restrict__ fn, long long m, const long long* __restrict__ row_start,
                                                                 const long long* __restrict__ incident, long long n, double* __restrict__ out,
                                                                 unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < n) {
        const long long nnz = row_start[n];
        const long long b = row_start[i], e = row_start[i + 1];
        double o[3] = {0.0, 0.0, 1.0};
        if (b < 0 || e < b || e > nnz || (e > b && m == 0)) {           // (without faces no row is followed: incident may be NULL)
            status |= ST_INDEX;
        } else if (e > b) {
            double s[3] = {0.0, 0.0, 0.0};
            bool ok = true, fin = true;
            for (long long j = b; j < e; ++j) {
                const long long q = incident[j];
                if (q < 0 || q >= m) { ok = false; break; }
                const double x = fn[3 * q], y = fn[3 * q + 1], z = fn[3 * q + 2];
                fin = fin && isfinite(x) && isfinite(y) && isfinite(z);
                if (j == b) { s[0] = x; s[1] = y; s[2] = z; }
                else { s[0] = s[0] + x; s[1] = s[1] + y; s[2] = s[2] + z; }
            }
            if (!ok) {
                status |= ST_INDEX;
            } else {
                if (!fin) status |= ST_NONFINITE;
                unit(s, 0.0, 0.0, 1.0, o, status);
            }
        }
        out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_normal_dots_kernel(const double* __restrict__ qn, long long n, const double* __restrict__ tn, long long m,
                                                              const long long* __restrict__ index, double* __restrict__ out,
                                                              unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < n) {
        const long long j = index[i];
        double r = 0.0;
        if (j < 0 || j >= m) {
            status |= ST_INDEX;
        } else {
            const double qx = qn[3 * i], qy = qn[3 * i + 1], qz = qn[3 * i + 2];
            const double tx = tn[3 * j], ty = tn[3 * j + 1], tz = tn[3 * j + 2];
            if (!(isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(tx) && isfinite(ty) && isfinite(tz))) status |= ST_NONFINITE;
            double d = qx * tx;
            d = d + qy * ty;
            d = d + qz * tz;
            r = fabs(d);
        }
        out[i] = r;
    }
    report(status, info);
}

bool count_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }

}  // namespace

extern "C" int vfn_face_normals(const double* vertices, int64_t n, const int64_t* faces, int64_t m, int32_t normalise, double* out, int64_t* info,
                                void* stream) {
    VFN_REQUIRE(count_ok(n) && count_ok(m), "vfn_face_normals: n %lld / m %lld outside [0, 2^31)", (long long)n, (long long)m);
    VFN_REQUIRE(normalise == 0 || normalise == 1, "vfn_face_normals: normalise %d is not 0 or 1", (int)normalise);
    VFN_REQUIRE(info, "vfn_face_normals: NULL info");
    if (m == 0) return VFN_OK;
    VFN_REQUIRE(faces && out && (vertices || n == 0), "vfn_face_normals: NULL argument");
    hipLaunchKernelGGL(vfn_face_normals_kernel, dim3(blocks_for(m)), dim3(NRM_BLOCK), 0, (hipStream_t)stream, vertices, (long long)n,
                       (const long long*)faces, (long long)m, (int)normalise, out, (unsigned long long*)info);
    return vfn_check_launch("vfn_face_normals");
}

extern "C" int vfn_vertex_normals(const double* face_normals, int64_t m, const int64_t* row_start, const int64_t* incident, int64_t n, double* out,
                                  int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n) && count_ok(m), "vfn_vertex_normals: n %lld / m %lld outside [0, 2^31)", (long long)n, (long long)m);
    VFN_REQUIRE(info, "vfn_vertex_normals: NULL info");
    if (n == 0) return VFN_OK;
    // (incident may be NULL only for a mesh without faces: the kernel then follows no row, whatever row_start says — m = 0 refuses every face)
    VFN_REQUIRE(row_start && out && (m == 0 || (face_normals && incident)), "vfn_vertex_normals: NULL argument");
    hipLaunchKernelGGL(vfn_vertex_normals_kernel, dim3(blocks_for(n)), dim3(NRM_BLOCK), 0, (hipStream_t)stream, face_normals, (long long)m,
                       (const long long*)row_start, (const long long*)incident, (long long)n, out, (unsigned long long*)info);
    return vfn_check_launch("vfn_vertex_normals");
}

extern "C" int vfn_normal_dots(const double* qn, int64_t n, const double* tn, int64_t m, const int64_t* index, double* out, int64_t* info,
                               void* stream) {
    VFN_REQUIRE(count_ok(n) && count_ok(m), "vfn_normal_dots: n %lld / m %lld outside [0, 2^31)", (long long)n, (long long)m);
    VFN_REQUIRE(info, "vfn_normal_dots: NULL info");
    if (n == 0) return VFN_OK;
    VFN_REQUIRE(qn && index && out && (tn || m == 0), "vfn_normal_dots: NULL argument");
    hipLaunchKernelGGL(vfn_normal_dots_kernel, dim3(blocks_for(n)), dim3(NRM_BLOCK), 0, (hipStream_t)stream, qn, (long long)n, tn, (long long)m,
                       (const long long*)index, out, (unsigned long long*)info);
    return vfn_check_launch("vfn_normal_dots");
}
