// vfn_raster.hip — the depth of a triangle mesh as pinhole cameras see it, and Laplacian smoothing of its vertices: what
// evaluation/methods.py:33-72 (refuse) and :686-691 (tsdf-smoothed) need on top of the TSDF volume.  include/vfn.h states the arithmetic
// ("Rasterising a mesh's depth"); here:
//   raster   ONE launch for all views of a call.  A lane owns one face: it reads its three indices and world vertices once, keeps them
//            in registers and walks the views of its chunk (grid.y splits the views so that a small mesh still fills the device; the
//            minimum does not care who arrives first).  The view index is wave-uniform, so a view's 16 parameters are scalar loads.
//            Per view: camera-space vertices, the z cull, the three edge normals and D, the candidate rectangle.  A rectangle of at
//            most SMALL x SMALL pixels is walked by the lane itself.  Larger ones, and every face that straddles the near plane (its
//            rectangle is the whole image), are taken by the WAVE: the lanes that hold one are balloted, the wave takes them one at a
//            time in lane order, the coefficients go to scalar registers and the 64 lanes stride over the rectangle, neighbouring
//            lanes on neighbouring pixels of a row.  No list, no second launch, nothing that can overflow.
//   depth    the float's bit pattern as uint32 (positive floats order as unsigned integers), filled with +inf by the call, updated
//            with a 32-bit atomicMin behind a plain load (a fragment that is already behind sends no atomic; a stale load can only
//            let through an atomic that loses), +inf turned into 0 by a last pass.  The minimum commutes: no bit depends on the
//            order of faces, lanes or launches.
//   smooth   one lane per vertex, one Jacobi step from src to dst over a CSR of ascending neighbours.  No atomics.
// Both forms of the pixel walk call the same fragment(): the bits cannot differ.  fp64 without contraction: -ffp-contract=off (build.sh).
#include "vfn_common.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;
constexpr int SMALL = 8;                 // a candidate rectangle of at most SMALL x SMALL pixels stays with its lane
constexpr unsigned INF_BITS = 0x7f800000u;
constexpr unsigned long long ST_NONFINITE = 1ull, ST_INDEX = 2ull;

struct Mesh {
    const double* v;
    long long nv;
    const long long* f;
    long long nf;
};

struct Cams {
    const float* intr;       // [V, 4]: fx fy cx cy
    const float* extr;       // [V, 12]: world -> camera rows
    int n, h, w;
    double near, far, c;
};

struct Counters {
    unsigned long long frags = 0, atomics = 0, coop = 0;
};

__device__ __forceinline__ bool finite3(const double p[3]) { return p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0; }

__device__ __forceinline__ double cam_row(const float* __restrict__ e, const double p[3]) {
    return (((double)e[0] * p[0] + (double)e[1] * p[1]) + (double)e[2] * p[2]) + (double)e[3];
}

__device__ __forceinline__ void cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// one (face, pixel) pair: n = the three edge normals n0 n1 n2, D the face's determinant, (dx, dy, 1) the pixel's ray
__device__ __forceinline__ void fragment(const double n[9], double D, double dx, double dy, double near, double far, unsigned* __restrict__ px,
                                         Counters& cnt) {
    const double e0 = (n[0] * dx + n[1] * dy) + n[2];
    const double e1 = (n[3] * dx + n[4] * dy) + n[5];
    const double e2 = (n[6] * dx + n[7] * dy) + n[8];
    const double s = (e0 + e1) + e2;
    const bool inside = D > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    if (!inside || !(s != 0.0)) return;
    const double z = D / s;
    if (!(z >= near && z <= far)) return;
    const unsigned bits = __float_as_uint((float)z);          // near > 0: a positive float, ordered as its bits
    ++cnt.frags;
    if (bits < *px) {
        atomicMin(px, bits);
        ++cnt.atomics;
    }
}

__device__ __forceinline__ double bcast(double x, int src) {   // src wave-uniform: the value lands in scalar registers
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, src), hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

__global__ __launch_bounds__(THREADS) void vfn_raster_fill_kernel(unsigned* __restrict__ depth, long long pixels, const double* __restrict__ v,
                                                                  long long n3, unsigned long long* __restrict__ info) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long i = t; i < pixels; i += stride) depth[i] = INF_BITS;
    bool bad = false;
    for (long long i = t; i < n3; i += stride) bad |= !(v[i] - v[i] == 0.0);
    if (bad) atomicOr(info, ST_NONFINITE);
}

__global__ __launch_bounds__(THREADS) void vfn_raster_finish_kernel(unsigned* __restrict__ depth, long long pixels) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pixels && depth[i] == INF_BITS) depth[i] = 0u;
}

__global__ __launch_bounds__(THREADS) void vfn_raster_kernel(Mesh mesh, Cams cams, unsigned* __restrict__ depth, int views_per_chunk,
                                                             unsigned long long* __restrict__ info) {
    const long long face = (long long)blockIdx.x * THREADS + threadIdx.x;
    bool have = face < mesh.nf;
    double X[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (have) {
        const long long a = mesh.f[3 * face], b = mesh.f[3 * face + 1], c = mesh.f[3 * face + 2];
        if (a < 0 || a >= mesh.nv || b < 0 || b >= mesh.nv || c < 0 || c >= mesh.nv) {
            atomicOr(info, ST_INDEX);                          // nothing is read through a bad index
            have = false;
        } else {
            const long long q[3] = {a, b, c};
#pragma unroll
            for (int k = 0; k < 3; ++k) { X[k][0] = mesh.v[3 * q[k]]; X[k][1] = mesh.v[3 * q[k] + 1]; X[k][2] = mesh.v[3 * q[k] + 2]; }
            if (!(finite3(X[0]) && finite3(X[1]) && finite3(X[2]))) have = false;      // (the fill pass has reported it)
        }
    }
    const int view0 = blockIdx.y * views_per_chunk, view1 = min(cams.n, view0 + views_per_chunk);
    const double near = cams.near, far = cams.far, pc = cams.c;
    const int W = cams.w, H = cams.h;
    Counters cnt;

    for (int view = view0; view < view1; ++view) {
        const float* __restrict__ e = cams.extr + (long long)view * 12;
        const float* __restrict__ k = cams.intr + (long long)view * 4;
        const double fx = (double)k[0], fy = (double)k[1], cx = (double)k[2], cy = (double)k[3];
        unsigned* __restrict__ img = depth + (long long)view * H * W;

        double n[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, D = 0.0;
        int u0 = 0, u1 = -1, v0 = 0, v1 = -1;
        bool live = false;
        if (have) {
            double P[3][3];
#pragma unroll
            for (int q = 0; q < 3; ++q) { P[q][0] = cam_row(e, X[q]); P[q][1] = cam_row(e + 4, X[q]); P[q][2] = cam_row(e + 8, X[q]); }
            const bool behind = P[0][2] < near && P[1][2] < near && P[2][2] < near;
            const bool beyond = P[0][2] > far && P[1][2] > far && P[2][2] > far;
            if (!behind && !beyond) {
                cross(P[1], P[2], n);
                cross(P[2], P[0], n + 3);
                cross(P[0], P[1], n + 6);
                D = (P[0][0] * n[0] + P[0][1] * n[1]) + P[0][2] * n[2];
                if (D != 0.0 && D - D == 0.0) {
                    if (P[0][2] >= near && P[1][2] >= near && P[2][2] >= near) {
                        double px[3], py[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) { px[q] = (P[q][0] * fx) / P[q][2] + cx; py[q] = (P[q][1] * fy) / P[q][2] + cy; }
                        const double ulo = fmax(0.0, ceil(fmin(fmin(px[0], px[1]), px[2]) - pc) - 1.0);
                        const double uhi = fmin((double)(W - 1), floor(fmax(fmax(px[0], px[1]), px[2]) - pc) + 1.0);
                        const double vlo = fmax(0.0, ceil(fmin(fmin(py[0], py[1]), py[2]) - pc) - 1.0);
                        const double vhi = fmin((double)(H - 1), floor(fmax(fmax(py[0], py[1]), py[2]) - pc) + 1.0);
                        if (ulo <= uhi && vlo <= vhi) {        // (both ends lie in [0, W - 1] x [0, H - 1] here: the casts are exact)
                            u0 = (int)ulo; u1 = (int)uhi; v0 = (int)vlo; v1 = (int)vhi;
                            live = true;
                        }
                    } else {                                   // the face straddles the near plane: every pixel of the view
                        u0 = 0; u1 = W - 1; v0 = 0; v1 = H - 1;
                        live = true;
                    }
                }
            }
        }
        const bool big = live && (u1 - u0 >= SMALL || v1 - v0 >= SMALL);
        if (live && !big) {
            for (int u = u0; u <= u1; ++u) {
                const double dx = (((double)u + pc) - cx) / fx;
                for (int v = v0; v <= v1; ++v) {
                    const double dy = (((double)v + pc) - cy) / fy;
                    fragment(n, D, dx, dy, near, far, img + (long long)v * W + u, cnt);
                }
            }
        }
        unsigned long long mask = __ballot(big);
        if (mask) {
            const int lane = threadIdx.x & 63;
            while (mask) {
                const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
                mask &= mask - 1;
                double sn[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) sn[i] = bcast(n[i], src);
                const double sD = bcast(D, src);
                const int su0 = __builtin_amdgcn_readlane(u0, src), su1 = __builtin_amdgcn_readlane(u1, src);
                const int sv0 = __builtin_amdgcn_readlane(v0, src), sv1 = __builtin_amdgcn_readlane(v1, src);
                const int nu = su1 - su0 + 1;
                const long long count = (long long)nu * (sv1 - sv0 + 1);
                if (lane == src) ++cnt.coop;
                for (long long p = lane; p < count; p += 64) {
                    const int u = su0 + (int)(p % nu), v = sv0 + (int)(p / nu);
                    const double dx = (((double)u + pc) - cx) / fx, dy = (((double)v + pc) - cy) / fy;
                    fragment(sn, sD, dx, dy, near, far, img + (long long)v * W + u, cnt);
                }
            }
        }
    }
    // the counters of the write-up: one atomic per wave and word
    const unsigned long long fr = wave_sum(cnt.frags), at = wave_sum(cnt.atomics), co = wave_sum(cnt.coop);
    if ((threadIdx.x & 63) == 0) {
        if (fr) atomicAdd(info + 1, fr);
        if (at) atomicAdd(info + 2, at);
        if (co) atomicAdd(info + 3, co);
    }
}

__global__ __launch_bounds__(THREADS) void vfn_smooth_kernel(const double* __restrict__ src, double* __restrict__ dst, long long n,
                                                             const long long* __restrict__ row_start, const long long* __restrict__ nb,
                                                             long long nnz, double lam, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
    double out[3] = {v[0], v[1], v[2]};
    const long long b = row_start[i], e = row_start[i + 1];
    if (b < 0 || e < b || e > nnz) {
        atomicOr(info, ST_INDEX);
    } else if (e > b) {
        double s[3] = {0.0, 0.0, 0.0};
        bool ok = true;
        for (long long j = b; j < e; ++j) {
            const long long q = nb[j];
            if (q < 0 || q >= n) { ok = false; break; }
            if (j == b) { s[0] = src[3 * q]; s[1] = src[3 * q + 1]; s[2] = src[3 * q + 2]; }
            else { s[0] = s[0] + src[3 * q]; s[1] = s[1] + src[3 * q + 1]; s[2] = s[2] + src[3 * q + 2]; }
        }
        if (!ok) {
            atomicOr(info, ST_INDEX);
        } else {
            const double count = (double)(e - b);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = v[c] + lam * (s[c] / count - v[c]);
        }
    }
    dst[3 * i] = out[0]; dst[3 * i + 1] = out[1]; dst[3 * i + 2] = out[2];
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int vfn_raster_depth(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const float* intrinsics,
                                const float* extrinsics, int32_t n_views, int32_t height, int32_t width, float near, float far,
                                float pixel_centre, float* depth, int64_t* info, void* stream) {
    VFN_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_vertices < (1ll << 31) && n_faces < (1ll << 31),
                "vfn_raster_depth: %lld vertices / %lld faces outside [0, 2^31)", (long long)n_vertices, (long long)n_faces);
    VFN_REQUIRE(n_views >= 0 && height >= 1 && width >= 1, "vfn_raster_depth: bad views (%d of %d x %d)", n_views, height, width);
    VFN_REQUIRE((long long)height * width < (1ll << 31) && (long long)n_views * height * width < (1ll << 31),
                "vfn_raster_depth: %d views of %d x %d pixels reach the 2^31 limit of one call", n_views, height, width);
    VFN_REQUIRE(near > 0.f && far - far == 0.f && far > near, "vfn_raster_depth: need 0 < near < far, both finite (near %g, far %g)", (double)near,
                (double)far);
    VFN_REQUIRE(pixel_centre - pixel_centre == 0.f, "vfn_raster_depth: pixel_centre must be finite");
    if (n_views == 0) return VFN_OK;
    VFN_REQUIRE(depth && info && intrinsics && extrinsics, "vfn_raster_depth: NULL argument");
    VFN_REQUIRE(n_faces == 0 || faces, "vfn_raster_depth: NULL faces");
    VFN_REQUIRE(n_vertices == 0 || vertices, "vfn_raster_depth: NULL vertices");
    hipStream_t s = (hipStream_t)stream;
    const long long pixels = (long long)n_views * height * width;
    unsigned* bits = (unsigned*)depth;
    long long fill_blocks = (pixels + THREADS - 1) / THREADS;
    if (fill_blocks > 65536) fill_blocks = 65536;
    hipLaunchKernelGGL(vfn_raster_fill_kernel, dim3((unsigned)fill_blocks), dim3(THREADS), 0, s, bits, pixels, vertices, (long long)n_vertices * 3,
                       (unsigned long long*)info);
    if (n_faces > 0) {
        const long long face_blocks = (n_faces + THREADS - 1) / THREADS;
        // enough workgroups for the device whatever the mesh's size: the views split over grid.y once the faces alone are too few
        long long chunks = (4096 + face_blocks - 1) / face_blocks;
        if (chunks > n_views) chunks = n_views;
        if (chunks < 1) chunks = 1;
        const int per = (int)((n_views + chunks - 1) / chunks);
        chunks = (n_views + per - 1) / per;
        Mesh mesh{vertices, (long long)n_vertices, (const long long*)faces, (long long)n_faces};
        Cams cams{intrinsics, extrinsics, n_views, height, width, (double)near, (double)far, (double)pixel_centre};
        hipLaunchKernelGGL(vfn_raster_kernel, dim3((unsigned)face_blocks, (unsigned)chunks), dim3(THREADS), 0, s, mesh, cams, bits, per,
                           (unsigned long long*)info);
    }
    hipLaunchKernelGGL(vfn_raster_finish_kernel, dim3(blocks_for(pixels)), dim3(THREADS), 0, s, bits, pixels);
    return vfn_check_launch("vfn_raster_depth");
}

extern "C" int vfn_smooth_laplacian_step(const double* src, double* dst, int64_t n_vertices, const int64_t* row_start, const int64_t* neighbours,
                                         int64_t n_neighbours, double lam, int64_t* info, void* stream) {
    VFN_REQUIRE(n_vertices >= 0 && n_vertices < (1ll << 31) && n_neighbours >= 0, "vfn_smooth_laplacian_step: %lld vertices / %lld neighbours out of range",
                (long long)n_vertices, (long long)n_neighbours);
    VFN_REQUIRE(lam - lam == 0.0, "vfn_smooth_laplacian_step: lam must be finite");
    if (n_vertices == 0) return VFN_OK;
    VFN_REQUIRE(src && dst && src != dst && row_start && info && (neighbours || n_neighbours == 0),
                "vfn_smooth_laplacian_step: NULL argument, or src and dst are one array (the step is a Jacobi update)");
    hipLaunchKernelGGL(vfn_smooth_kernel, dim3(blocks_for(n_vertices)), dim3(THREADS), 0, (hipStream_t)stream, src, dst, (long long)n_vertices,
                       (const long long*)row_start, (const long long*)neighbours, (long long)n_neighbours, lam, (unsigned long long*)info);
    return vfn_check_launch("vfn_smooth_laplacian_step");
}
