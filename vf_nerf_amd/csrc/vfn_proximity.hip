// vfn_proximity.hip — every query's closest point ON a triangle mesh, with the face (include/vfn.h: vfn_tri_cell_ranges,
// vfn_tri_cell_pairs, vfn_tri_nearest, vfn_tri_nearest_list): the point-to-surface search beside the point-to-point searches of
// csrc/vfn_nn.hip, on the same uniform grid and with the same stop rule.
//   tri_cell_ranges   one lane per face: its nine coordinates packed into a row of tri[F, 9], its box, through vfn_cell_of the low and
//                     the high cell per axis and the number of cells covered (0: a face with an index outside [0, V), which nothing is
//                     read through and which no later kernel evaluates).
//   tri_cell_pairs    one lane per face that is not large: (key, face) for every covered cell, from the face's exclusive prefix sum.
//   tri_nearest       one lane per query: the large faces first, then the cells around the query's own, ring by ring, every pair
//                     of a cell through vfn_closest_on_triangle (csrc/vfn_proximity_core.h); the stop rule, the leftover list and
//                     the ring walk are vfn_nn_nearest's.  Lanes diverge: vector loads, no LDS, no lane waits on another.
//   tri_nearest_list  one wave per listed query: 64 lanes stride over all faces in their ORIGINAL order, then a lexicographic
//                     (d2, face) minimum across the wave by shuffles, the closest point following the winner.
// All arithmetic fp64 with -ffp-contract=off (build.sh).  The only atomics are integer ones: atomicOr on the status word, atomicAdd on
// leftover_count.
//
// WHY THE GRID CANNOT CHANGE A BIT.  The result is defined without the grid: the minimum of (d2(q, face j), j) in lexicographic order
// over all faces with ncells > 0, and the closest point c of the winner.  (d2, c) of a pair is a pure function of the query and the
// face's nine coordinates, so a face met twice (it is registered in every cell its box touches) gives the same pair twice and the
// minimum is idempotent; the order of the visit does not matter either.  The list kernel and the large list visit their faces
// unconditionally.  It remains that a query which STOPS after ring r has missed no face that could win or tie.  The argument of
// csrc/vfn_nn.hip, steps (a)-(e), is about ONE target point t with three properties: t lies in [o, e]; t lies in a cell that rings
// 0..r do not hold; d2 is vfn_pair_sqdist(q, t).  For a face j that is not large and has no registered cell in rings 0..r take
// t = c(q, j), the point the pair routine returns:
//   * P2 (include/vfn.h): c lies in the face's box [lo_j, hi_j] exactly, and [o, e] is the box of all vertices that some face names,
//     so c lies in [o, e];
//   * per axis cell() is monotone (x -> min(max(x, o), e), the rounded subtraction of o, the rounded division by h > 0, floor and the
//     clamps are each non-decreasing), so cell(lo_j) <= cell(c) <= cell(hi_j): cell(c) is one of the cells face j is registered in
//     — the product of its per-axis ranges, which is exactly what tri_cell_ranges / tri_cell_pairs write — and none of those is in
//     rings 0..r;
//   * P3: d2(q, j) is vfn_pair_sqdist(q, c), operation for operation.
// Steps (a)-(e) then give d2(q, j) > lb > best, strictly: the face can neither win nor tie.  No new error analysis is needed: the
// triangle never enters the bound, only the point the routine returned.  A NaN or infinite query cannot reach memory it should not:
// as there, the cell is clamped in double before the conversion and every range is clipped to [0, n_pairs].
#include "vfn_common.h"
#include "vfn_proximity_core.h"
#include <math.h>

namespace {

constexpr int PX_BLOCK = 256;
constexpr int WAVE = 64;                                                            // gfx950: one query per wave in the list kernel
constexpr int GRID_CAP = VFN_ICP_GRID_CAP;
constexpr double RING_GUARD = 1.0 / (double)(1ll << VFN_ICP_GRID_MARGIN_LOG2);      // 2^-20
constexpr double RING_SHAVE = 1.0 - 1.0 / (double)(1ll << VFN_ICP_GRID_MARGIN_LOG2);    // 1 - 2^-20
constexpr double MIN_NORMAL = 2.2250738585072014e-308;                              // 2^-1022
constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

struct Grid { double o[3], e[3], h; int dim[3]; };

__device__ __forceinline__ double plus_inf() { return __longlong_as_double((long long)INF_BITS); }

__global__ __launch_bounds__(PX_BLOCK) void vfn_tri_cell_ranges_kernel(const double* __restrict__ v, long long nv, const long long* __restrict__ f,
                                                                       long long nf, Grid g, double* __restrict__ tri, int* __restrict__ cell_lo,
                                                                       int* __restrict__ cell_hi, int* __restrict__ ncells,
                                                                       unsigned long long* __restrict__ info) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nf) return;
    const long long i[3] = {f[3 * j], f[3 * j + 1], f[3 * j + 2]};
    if (i[0] < 0 || i[0] >= nv || i[1] < 0 || i[1] >= nv || i[2] < 0 || i[2] >= nv) {           // nothing is read through it
        for (int k = 0; k < 9; ++k) tri[9 * j + k] = 0.0;
        for (int k = 0; k < 3; ++k) { cell_lo[3 * j + k] = 0; cell_hi[3 * j + k] = -1; }
        ncells[j] = 0;
        atomicOr(info, 2ull);
        return;
    }
    double p[9];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[3 * a + k] = v[3 * i[a] + k];
            finite = finite && isfinite(p[3 * a + k]);
            tri[9 * j + 3 * a + k] = p[3 * a + k];
        }
    if (!finite) atomicOr(info, 1ull);
    int count = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double lo = p[k], hi = p[k];
        if (p[3 + k] < lo) lo = p[3 + k];
        if (p[6 + k] < lo) lo = p[6 + k];
        if (p[3 + k] > hi) hi = p[3 + k];
        if (p[6 + k] > hi) hi = p[6 + k];
        const int c0 = vfn_cell_of(lo, g.o[k], g.e[k], g.h, g.dim[k]);
        int c1 = vfn_cell_of(hi, g.o[k], g.e[k], g.h, g.dim[k]);
        c1 = c1 < c0 ? c0 : c1;                                      // (a NaN coordinate: keep the range ordered)
        cell_lo[3 * j + k] = c0;
        cell_hi[3 * j + k] = c1;
        count *= c1 - c0 + 1;                                        // at most 128^3 = 2^21
    }
    ncells[j] = count;
}

// a face with 1 <= ncells <= big_face_cells writes its pairs at offset[j] .. offset[j] + ncells[j]; any other face writes nothing
__global__ __launch_bounds__(PX_BLOCK) void vfn_tri_cell_pairs_kernel(const int* __restrict__ cell_lo, const int* __restrict__ cell_hi,
                                                                      const int* __restrict__ ncells, const long long* __restrict__ offset,
                                                                      long long nf, long long big, Grid g, long long n_pairs,
                                                                      int* __restrict__ key, int* __restrict__ face,
                                                                      unsigned long long* __restrict__ info) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nf) return;
    const long long count = ncells[j];
    if (count < 1 || count > big) return;
    int lo[3], hi[3];
    long long check = 1;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        lo[k] = cell_lo[3 * j + k]; hi[k] = cell_hi[3 * j + k];
        ok = ok && lo[k] >= 0 && hi[k] >= lo[k] && hi[k] < g.dim[k];
        check *= (long long)hi[k] - lo[k] + 1;
    }
    long long at = offset[j];
    if (!ok || check != count || at < 0 || at > n_pairs - count) {   // tables that do not belong together: write nothing
        atomicOr(info, 2ull);
        return;
    }
    for (int ix = lo[0]; ix <= hi[0]; ++ix)
        for (int iy = lo[1]; iy <= hi[1]; ++iy)
            for (int iz = lo[2]; iz <= hi[2]; ++iz, ++at) {
                key[at] = (ix * g.dim[1] + iy) * g.dim[2] + iz;
                face[at] = (int)j;
            }
}

struct Found {
    double d2, c[3];
    long long face;
};

// face j against the query: the lexicographic minimum of (d2, face); a face evaluated again changes nothing
__device__ __forceinline__ void try_face(long long j, const double* __restrict__ tri, const double* p, Found& best) {
    double t[9], c[3], d2;
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = tri[9 * j + k];
    vfn_proximity::closest_on_triangle(p, t, t + 3, t + 6, c, &d2);
    if (d2 < best.d2 || (d2 == best.d2 && j < best.face)) {
        best.d2 = d2; best.face = j;
        best.c[0] = c[0]; best.c[1] = c[1]; best.c[2] = c[2];
    }
}

// the sorted pairs [j, j1) against one query
__device__ __forceinline__ void scan_pairs(long long j, long long j1, long long n_pairs, long long nf, const int* __restrict__ pair_face,
                                           const double* __restrict__ tri, const double* p, Found& best) {
    j = j < 0 ? 0 : j;
    j1 = j1 > n_pairs ? n_pairs : j1;
    for (; j < j1; ++j) {
        const long long k = pair_face[j];
        if (k >= 0 && k < nf && k != best.face) try_face(k, tri, p, best);      // (the winner met again: the same pair, skipped)
    }
}

__global__ __launch_bounds__(PX_BLOCK) void vfn_tri_nearest_kernel(const double* __restrict__ q, long long n, const double* __restrict__ tri, long long nf,
                                                                   const int* __restrict__ pair_face, long long n_pairs,
                                                                   const int* __restrict__ cell_start, const long long* __restrict__ large,
                                                                   long long n_large, Grid g, int max_rings, const long long* __restrict__ order,
                                                                   long long* __restrict__ face, double* __restrict__ closest,
                                                                   double* __restrict__ sqdist, long long* __restrict__ leftover,
                                                                   unsigned long long* __restrict__ leftover_count,
                                                                   unsigned long long* __restrict__ info) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= n) return;
    const long long i = order ? order[lane] : lane;
    if (i < 0 || i >= n) return;
    const double p[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) atomicOr(info, 1ull);
    int c[3];
    double s = 1.0;
    int cover = 0;
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
    Found best;
    best.d2 = plus_inf(); best.face = -1;
    best.c[0] = best.c[1] = best.c[2] = plus_inf();
    for (long long k = 0; k < n_large; ++k) {                        // the large faces: every query, before ring 0
        const long long j = large[k];
        if (j >= 0 && j < nf) try_face(j, tri, p, best);
    }
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
                if (x_face || iy - c[1] == r || c[1] - iy == r) {
                    scan_pairs(cell_start[row + z0], cell_start[row + z1 + 1], n_pairs, nf, pair_face, tri, p, best);
                } else {
                    if (zl >= 0) scan_pairs(cell_start[row + zl], cell_start[row + zl + 1], n_pairs, nf, pair_face, tri, p, best);
                    if (zh < g.dim[2]) scan_pairs(cell_start[row + zh], cell_start[row + zh + 1], n_pairs, nf, pair_face, tri, p, best);
                }
            }
        }
        if (r >= cover) {
            stopped = true;
        } else {
            const double rs = (double)r + s;
            const double w = rs * g.h;
            const double lb = (w * w) * RING_SHAVE;
            stopped = rs >= RING_GUARD && lb >= MIN_NORMAL && best.d2 < lb;
        }
    }
    if (stopped) {
        face[i] = best.face;
        sqdist[i] = best.d2;
        closest[3 * i] = best.c[0]; closest[3 * i + 1] = best.c[1]; closest[3 * i + 2] = best.c[2];
    } else {
        const unsigned long long slot = atomicAdd(leftover_count, 1ull);
        if (slot < (unsigned long long)n) leftover[slot] = i;
    }
}

// wave w serves the query leftover[w]; lane l takes the faces l, l + 64, ... in ascending order and keeps its first strict minimum, so
// a lane's (d2, j) is its lexicographic minimum; the butterfly joins the 64 of them and the closest point travels with its pair.  A
// lane without a face below +inf holds (+inf, -1).  The loop bounds are wave-uniform; a face with ncells = 0 is skipped by its lane.
__global__ __launch_bounds__(PX_BLOCK) void vfn_tri_nearest_list_kernel(const double* __restrict__ q, long long n, const double* __restrict__ tri,
                                                                        const int* __restrict__ ncells, long long nf,
                                                                        const long long* __restrict__ list, long long count,
                                                                        long long* __restrict__ face, double* __restrict__ closest,
                                                                        double* __restrict__ sqdist, unsigned long long* __restrict__ info) {
    const long long wave = ((long long)blockIdx.x * PX_BLOCK + threadIdx.x) / WAVE;
    const int l = threadIdx.x % WAVE;
    if (wave >= count) return;                                       // (the whole wave)
    const long long i = list[wave];
    if (i < 0 || i >= n) return;                                     // (the whole wave)
    const double p[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    if (l == 0 && !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) atomicOr(info, 1ull);
    Found best;
    best.d2 = plus_inf(); best.face = -1;
    best.c[0] = best.c[1] = best.c[2] = plus_inf();
    for (long long base = 0; base < nf; base += WAVE) {
        const long long j = base + l;
        if (j < nf && ncells[j] > 0) try_face(j, tri, p, best);      // ascending j per lane: `j < best.face` never holds here
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const double ob = __shfl_xor(best.d2, d, WAVE);
        const long long oj = __shfl_xor(best.face, d, WAVE);
        const double o0 = __shfl_xor(best.c[0], d, WAVE), o1 = __shfl_xor(best.c[1], d, WAVE), o2 = __shfl_xor(best.c[2], d, WAVE);
        if (ob < best.d2 || (ob == best.d2 && oj < best.face)) {
            best.d2 = ob; best.face = oj;
            best.c[0] = o0; best.c[1] = o1; best.c[2] = o2;
        }
    }
    if (l == 0) {
        face[i] = best.face;
        sqdist[i] = best.d2;
        closest[3 * i] = best.c[0]; closest[3 * i + 1] = best.c[1]; closest[3 * i + 2] = best.c[2];
    }
}

bool count_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }

// box[7] and the dimensions under the limits of vfn_nn_nearest
int read_grid(const char* who, const double* box, int32_t nx, int32_t ny, int32_t nz, Grid* g) {
    VFN_REQUIRE(box, "%s: NULL argument", who);
    VFN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= GRID_CAP && ny <= GRID_CAP && nz <= GRID_CAP, "%s: grid %d x %d x %d outside [1, %d]^3", who,
                nx, ny, nz, GRID_CAP);
    for (int k = 0; k < 3; ++k) { g->o[k] = box[k]; g->e[k] = box[3 + k]; }
    g->h = box[6];
    g->dim[0] = nx; g->dim[1] = ny; g->dim[2] = nz;
    const double reach = (GRID_CAP + 2) * g->h;
    bool box_ok = isfinite(g->h) && g->h >= MIN_NORMAL && isfinite(reach * reach);
    for (int k = 0; k < 3; ++k)
        box_ok = box_ok && isfinite(g->o[k]) && isfinite(g->e[k]) && g->o[k] <= g->e[k] && (g->e[k] - g->o[k]) / g->h <= GRID_CAP + 1;
    VFN_REQUIRE(box_ok, "%s: the box is not finite and ordered, or its cell edge %g is not normal, below (max - min) / %d, or (%d h)^2 overflows", who,
                g->h, GRID_CAP, GRID_CAP + 2);
    return VFN_OK;
}

}  // namespace

extern "C" int vfn_tri_cell_ranges(const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, const double* box,
                                   int32_t nx, int32_t ny, int32_t nz, double* tri, int32_t* cell_lo, int32_t* cell_hi, int32_t* ncells,
                                   int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n_vertices) && count_ok(n_faces), "vfn_tri_cell_ranges: n_vertices %lld / n_faces %lld outside [1, 2^31)",
                (long long)n_vertices, (long long)n_faces);
    Grid g;
    if (int rc = read_grid("vfn_tri_cell_ranges", box, nx, ny, nz, &g)) return rc;
    VFN_REQUIRE(vertices && faces && tri && cell_lo && cell_hi && ncells && info, "vfn_tri_cell_ranges: NULL argument");
    hipLaunchKernelGGL(vfn_tri_cell_ranges_kernel, dim3(blocks_for(n_faces, PX_BLOCK)), dim3(PX_BLOCK), 0, (hipStream_t)stream, vertices,
                       (long long)n_vertices, (const long long*)faces, (long long)n_faces, g, tri, (int*)cell_lo, (int*)cell_hi, (int*)ncells,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_tri_cell_ranges");
}

extern "C" int vfn_tri_cell_pairs(const int32_t* cell_lo, const int32_t* cell_hi, const int32_t* ncells, const int64_t* offset, int64_t n_faces,
                                  int64_t big_face_cells, int32_t nx, int32_t ny, int32_t nz, int64_t n_pairs, int32_t* key, int32_t* face,
                                  int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n_faces), "vfn_tri_cell_pairs: n_faces %lld outside [1, 2^31)", (long long)n_faces);
    VFN_REQUIRE(n_pairs >= 1 && n_pairs < (1ll << 31), "vfn_tri_cell_pairs: n_pairs %lld outside [1, 2^31)", (long long)n_pairs);
    VFN_REQUIRE(big_face_cells >= 0, "vfn_tri_cell_pairs: big_face_cells %lld is negative", (long long)big_face_cells);
    VFN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= GRID_CAP && ny <= GRID_CAP && nz <= GRID_CAP, "vfn_tri_cell_pairs: grid %d x %d x %d outside [1, %d]^3",
                nx, ny, nz, GRID_CAP);
    VFN_REQUIRE(cell_lo && cell_hi && ncells && offset && key && face && info, "vfn_tri_cell_pairs: NULL argument");
    Grid g = {};
    g.dim[0] = nx; g.dim[1] = ny; g.dim[2] = nz;
    hipLaunchKernelGGL(vfn_tri_cell_pairs_kernel, dim3(blocks_for(n_faces, PX_BLOCK)), dim3(PX_BLOCK), 0, (hipStream_t)stream, (const int*)cell_lo,
                       (const int*)cell_hi, (const int*)ncells, (const long long*)offset, (long long)n_faces, (long long)big_face_cells, g,
                       (long long)n_pairs, (int*)key, (int*)face, (unsigned long long*)info);
    return vfn_check_launch("vfn_tri_cell_pairs");
}

extern "C" int vfn_tri_nearest(const double* queries, int64_t n, const double* tri, int64_t n_faces, const int32_t* pair_face, int64_t n_pairs,
                               const int32_t* cell_start, const int64_t* large, int64_t n_large, const double* box, int32_t nx, int32_t ny,
                               int32_t nz, int32_t max_rings, const int64_t* order, int64_t* face, double* closest, double* sqdist,
                               int64_t* leftover, int64_t* leftover_count, int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n) && count_ok(n_faces), "vfn_tri_nearest: n %lld / n_faces %lld outside [1, 2^31)", (long long)n, (long long)n_faces);
    VFN_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31), "vfn_tri_nearest: n_pairs %lld outside [0, 2^31)", (long long)n_pairs);
    VFN_REQUIRE(n_large >= 0 && n_large <= n_faces, "vfn_tri_nearest: n_large %lld outside [0, n_faces = %lld]", (long long)n_large, (long long)n_faces);
    VFN_REQUIRE(max_rings >= 0, "vfn_tri_nearest: max_rings %d is negative", max_rings);
    Grid g;
    if (int rc = read_grid("vfn_tri_nearest", box, nx, ny, nz, &g)) return rc;
    VFN_REQUIRE(queries && tri && cell_start && face && closest && sqdist && leftover && leftover_count && info && (pair_face || n_pairs == 0) &&
                    (large || n_large == 0),
                "vfn_tri_nearest: NULL argument");
    hipLaunchKernelGGL(vfn_tri_nearest_kernel, dim3(blocks_for(n, PX_BLOCK)), dim3(PX_BLOCK), 0, (hipStream_t)stream, queries, (long long)n, tri,
                       (long long)n_faces, (const int*)pair_face, (long long)n_pairs, (const int*)cell_start, (const long long*)large,
                       (long long)n_large, g, (int)max_rings, (const long long*)order, (long long*)face, closest, sqdist, (long long*)leftover,
                       (unsigned long long*)leftover_count, (unsigned long long*)info);
    return vfn_check_launch("vfn_tri_nearest");
}

extern "C" int vfn_tri_nearest_list(const double* queries, int64_t n, const double* tri, const int32_t* ncells, int64_t n_faces,
                                    const int64_t* list, int64_t count, int64_t* face, double* closest, double* sqdist, int64_t* info,
                                    void* stream) {
    VFN_REQUIRE(count_ok(n) && count_ok(n_faces), "vfn_tri_nearest_list: n %lld / n_faces %lld outside [1, 2^31)", (long long)n, (long long)n_faces);
    VFN_REQUIRE(count >= 1 && count <= n, "vfn_tri_nearest_list: count %lld outside [1, n = %lld]", (long long)count, (long long)n);
    VFN_REQUIRE(queries && tri && ncells && list && face && closest && sqdist && info, "vfn_tri_nearest_list: NULL argument");
    hipLaunchKernelGGL(vfn_tri_nearest_list_kernel, dim3(blocks_for(count, PX_BLOCK / WAVE)), dim3(PX_BLOCK), 0, (hipStream_t)stream, queries,
                       (long long)n, tri, (const int*)ncells, (long long)n_faces, (const long long*)list, (long long)count, (long long*)face, closest,
                       sqdist, (unsigned long long*)info);
    return vfn_check_launch("vfn_tri_nearest_list");
}
