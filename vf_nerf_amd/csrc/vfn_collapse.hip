// vfn_collapse.hip — one round of the quadric edge-collapse decimation (vf_nerf_amd/decimate.py: collapse_round, simplify_edge_collapse):
// a round-based, memoryless decimation AS SPECIFIED BY US (include/vfn.h), not the serial priority-queue order of trimesh / Open3D.
//   boundary_planes   one lane per boundary edge: the plane through the edge, perpendicular to its face.  Three gathered rows (two
//                     vertices of 24 bytes, a face plane of 40), 40 contiguous bytes written.
//   vertex_quadrics   one LANE per vertex: its ten sums over its plane rows, serially from the first (vfn_voxel_means' rule).  A vertex
//                     of a marching-cubes mesh has about six rows, so a wave per vertex would idle 58 lanes; per row 8 bytes of the
//                     table and a gathered 40-byte plane, two dependent loads: bound by their latency, not by bandwidth.
//   edge_candidates   one lane per unique edge: csrc/vfn_collapse_core.h — two quadrics of 80 bytes and two positions gathered, the solve,
//                     then the walk over both 1-rings (table entry -> face -> three vertices: three dependent loads per face, about
//                     ten faces an edge).  The walk dominates; it is latency-bound and divergent by the rings' lengths.
//   select            four small launches on one stream: every vertex's lowest (cost, edge) among its candidates by two integer
//                     atomicMin passes (the cost's bit pattern, then the edge index among the edges that hold that cost: a minimum is
//                     associative and commutative, so the result is the data's alone); the edges both of whose ends chose them are
//                     proposed; every face withdraws all but the lowest of the proposed edges its corners see, by plain byte stores of
//                     1 (idempotent: no atomic).
// All arithmetic fp64 with -ffp-contract=off (build.sh).  No floating-point atomics, no LDS, no bit depends on the schedule.  Nothing is
// read through a segment bound, a row or an index before it has been compared with its range; no kernel returns before its wave's status
// report, and a wave ORs its status bits into info[0] with at most one atomic (report() of csrc/vfn_geom.h).
#include "vfn_common.h"
#include "vfn_collapse_core.h"

namespace {

using namespace vfn_geom;
using namespace vfn_collapse;

constexpr int COL_BLOCK = 256;
constexpr unsigned long long NO_COST = ~0ull;
constexpr long long NO_EDGE = 0x7fffffffffffffffll;

__global__ __launch_bounds__(256) void vfn_boundary_planes_kernel(const double* __restrict__ v, long long n, const double* __restrict__ planes, long long m,
                                                                  const long long* __restrict__ face, const long long* __restrict__ from,
                                                                  const long long* __restrict__ to, long long count, double ox, double oy, double oz,
                                                                  double weight, double* __restrict__ out, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < count) {
        const long long f = face[i], a = from[i], b = to[i];
        double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (f < 0 || f >= m || a < 0 || a >= n || b < 0 || b >= n) {
            status |= ST_INDEX;
        } else {
            const double pa[3] = {v[3 * a], v[3 * a + 1], v[3 * a + 2]};
            const double pb[3] = {v[3 * b], v[3 * b + 1], v[3 * b + 2]};
            const double nf[3] = {planes[5 * f], planes[5 * f + 1], planes[5 * f + 2]};
            const double area = planes[5 * f + 4];
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) fin = fin && isfinite(pa[k]) && isfinite(pb[k]) && isfinite(nf[k]);
            if (!fin || !isfinite(area)) status |= ST_NONFINITE;
            const double d[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
            const double c[3] = {d[1] * nf[2] - d[2] * nf[1], d[2] * nf[0] - d[0] * nf[2], d[0] * nf[1] - d[1] * nf[0]};
            double r;
            if (unit_vector(c, o, &r, status)) {
                o[3] = plane_offset(o, pa, ox, oy, oz);
                o[4] = weight * area;
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) out[5 * i + k] = o[k];
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_vertex_quadrics_kernel(const double* __restrict__ planes, long long rows, const long long* __restrict__ item_row,
                                                                  long long n_items, const long long* __restrict__ start, long long n,
                                                                  double* __restrict__ quadrics, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < n) {
        const long long b = start[i], e = start[i + 1];
        double s[CHANNELS];
#pragma unroll
        for (int c = 0; c < CHANNELS; ++c) s[c] = 0.0;                  // a vertex without rows holds ten +0.0
        bool bad = b < 0 || e < b || e > n_items;
        if (!bad) {
            for (long long j = b; j < e; ++j) {
                const long long row = item_row[j];
                if (row < 0 || row >= rows) { bad = true; break; }
                const double nx = planes[5 * row], ny = planes[5 * row + 1], nz = planes[5 * row + 2], off = planes[5 * row + 3], w = planes[5 * row + 4];
                const double wx = w * nx, wy = w * ny, wz = w * nz, we = w * off;
                const double t[CHANNELS] = {wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, -(we * nx), -(we * ny), -(we * nz), we * off};
                if (j == b) {                                          // started from the first row
#pragma unroll
                    for (int c = 0; c < CHANNELS; ++c) s[c] = t[c];
                } else {
#pragma unroll
                    for (int c = 0; c < CHANNELS; ++c) s[c] = s[c] + t[c];
                }
            }
        }
        if (bad) {
            status |= ST_INDEX;
#pragma unroll
            for (int c = 0; c < CHANNELS; ++c) s[c] = __builtin_nan("");
        }
#pragma unroll
        for (int c = 0; c < CHANNELS; ++c) quadrics[CHANNELS * i + c] = s[c];
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_edge_candidates_kernel(Mesh g, const long long* __restrict__ edge_a, const long long* __restrict__ edge_b,
                                                                  const long long* __restrict__ run, long long n_edges, double* __restrict__ point,
                                                                  double* __restrict__ cost, double* __restrict__ par, unsigned char* __restrict__ flags,
                                                                  unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < n_edges) {
        Edge out;
        status = edge(g, edge_a[i], edge_b[i], run[i], &out);
        point[3 * i] = out.point[0]; point[3 * i + 1] = out.point[1]; point[3 * i + 2] = out.point[2];
        cost[i] = out.cost;
        par[i] = out.s;
        flags[i] = out.flags;
    }
    report(status, info);
}

// ---- the selection -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vfn_select_fill_kernel(unsigned long long* __restrict__ best_cost, long long* __restrict__ best_edge, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        best_cost[i] = NO_COST;
        best_edge[i] = NO_EDGE;
    }
}

// is edge i a candidate whose ends may be read through?
__device__ __forceinline__ bool live(const unsigned char* __restrict__ flags, const long long* __restrict__ edge_a, const long long* __restrict__ edge_b,
                                     long long i, long long n, long long* a, long long* b, unsigned* status) {
    if (!(flags[i] & F_CANDIDATE)) return false;
    *a = edge_a[i];
    *b = edge_b[i];
    if (*a < 0 || *a >= n || *b < 0 || *b >= n) { *status |= ST_INDEX; return false; }
    return true;
}

__global__ __launch_bounds__(256) void vfn_select_cost_kernel(const double* __restrict__ cost, const unsigned char* __restrict__ flags,
                                                              const long long* __restrict__ edge_a, const long long* __restrict__ edge_b, long long n_edges,
                                                              long long n, unsigned long long* __restrict__ best_cost, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    long long a, b;
    if (i < n_edges && live(flags, edge_a, edge_b, i, n, &a, &b, &status)) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(cost[i]);          // a cost is >= +0.0: its bits order like its value
        atomicMin(best_cost + a, bits);
        atomicMin(best_cost + b, bits);
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_select_edge_kernel(const double* __restrict__ cost, const unsigned char* __restrict__ flags,
                                                              const long long* __restrict__ edge_a, const long long* __restrict__ edge_b, long long n_edges,
                                                              long long n, const unsigned long long* __restrict__ best_cost,
                                                              long long* __restrict__ best_edge, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    long long a, b;
    if (i < n_edges && live(flags, edge_a, edge_b, i, n, &a, &b, &status)) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(cost[i]);
        if (best_cost[a] == bits) atomicMin(best_edge + a, i);
        if (best_cost[b] == bits) atomicMin(best_edge + b, i);
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_select_propose_kernel(const unsigned char* __restrict__ flags, const long long* __restrict__ edge_a,
                                                                 const long long* __restrict__ edge_b, long long n_edges, long long n,
                                                                 const long long* __restrict__ best_edge, unsigned char* __restrict__ proposed,
                                                                 unsigned char* __restrict__ withdrawn, unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < n_edges) {
        long long a, b;
        const bool both = live(flags, edge_a, edge_b, i, n, &a, &b, &status) && best_edge[a] == i && best_edge[b] == i;
        proposed[i] = both ? 1 : 0;
        withdrawn[i] = 0;
    }
    report(status, info);
}

__global__ __launch_bounds__(256) void vfn_select_withdraw_kernel(const long long* __restrict__ faces, long long m, long long n, const double* __restrict__ cost,
                                                                  long long n_edges, const long long* __restrict__ best_edge,
                                                                  const unsigned char* __restrict__ proposed, unsigned char* __restrict__ withdrawn,
                                                                  unsigned long long* __restrict__ info) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (i < m) {
        long long seen[3];
        int count = 0;
        long long low = NO_EDGE;
        unsigned long long low_bits = NO_COST;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long vertex = faces[3 * i + c];
            seen[c] = NO_EDGE;
            if (vertex < 0 || vertex >= n) { status |= ST_INDEX; continue; }
            const long long e = best_edge[vertex];
            if (e == NO_EDGE) continue;
            if (e < 0 || e >= n_edges) { status |= ST_INDEX; continue; }
            if (!proposed[e]) continue;
            seen[c] = e;
            ++count;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(cost[e]);
            if (bits < low_bits || (bits == low_bits && e < low)) { low_bits = bits; low = e; }
        }
        if (count > 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (seen[c] != NO_EDGE && seen[c] != low) withdrawn[seen[c]] = 1;          // plain, idempotent
        }
    }
    report(status, info);
}

bool count_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }

}  // namespace

extern "C" int vfn_boundary_planes(const double* vertices, int64_t n, const double* planes, int64_t m, const int64_t* face, const int64_t* from,
                                   const int64_t* to, int64_t count, const double* origin, double boundary_weight, double* out, int64_t* info,
                                   void* stream) {
    VFN_REQUIRE(count_ok(n), "vfn_boundary_planes: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(count_ok(m), "vfn_boundary_planes: m %lld outside [1, 2^31)", (long long)m);
    VFN_REQUIRE(count >= 1 && count <= 3 * m, "vfn_boundary_planes: count %lld outside [1, 3 m = %lld]", (long long)count, (long long)(3 * m));
    VFN_REQUIRE(vertices && planes && face && from && to && origin && out && info, "vfn_boundary_planes: NULL argument");
    VFN_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "vfn_boundary_planes: a non-finite origin");
    VFN_REQUIRE(isfinite(boundary_weight) && boundary_weight >= 0.0, "vfn_boundary_planes: boundary_weight %g is not finite and >= 0", boundary_weight);
    hipLaunchKernelGGL(vfn_boundary_planes_kernel, dim3(blocks_for(count)), dim3(COL_BLOCK), 0, (hipStream_t)stream, vertices, (long long)n, planes,
                       (long long)m, (const long long*)face, (const long long*)from, (const long long*)to, (long long)count, origin[0], origin[1],
                       origin[2], boundary_weight, out, (unsigned long long*)info);
    return vfn_check_launch("vfn_boundary_planes");
}

extern "C" int vfn_vertex_quadrics(const double* planes, int64_t rows, const int64_t* item_row, int64_t n_items, const int64_t* start, int64_t n,
                                   double* quadrics, int64_t* info, void* stream) {
    VFN_REQUIRE(rows >= 1 && rows < (1ll << 33), "vfn_vertex_quadrics: rows %lld outside [1, 2^33)", (long long)rows);
    VFN_REQUIRE(n_items >= 1 && n_items < (1ll << 35), "vfn_vertex_quadrics: n_items %lld outside [1, 2^35)", (long long)n_items);
    VFN_REQUIRE(count_ok(n), "vfn_vertex_quadrics: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(planes && item_row && start && quadrics && info, "vfn_vertex_quadrics: NULL argument");
    hipLaunchKernelGGL(vfn_vertex_quadrics_kernel, dim3(blocks_for(n)), dim3(COL_BLOCK), 0, (hipStream_t)stream, planes, (long long)rows,
                       (const long long*)item_row, (long long)n_items, (const long long*)start, (long long)n, quadrics, (unsigned long long*)info);
    return vfn_check_launch("vfn_vertex_quadrics");
}

extern "C" int vfn_edge_collapse_candidates(const double* vertices, int64_t n, const int64_t* faces, int64_t m, const double* quadrics,
                                            const int64_t* item_row, int64_t n_items, const int64_t* start, int64_t rows, const int64_t* edge_a,
                                            const int64_t* edge_b, const int64_t* run, int64_t n_edges, const double* origin, double rcond, double reach,
                                            double max_error, double* point, double* cost, double* s, uint8_t* flags, int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n), "vfn_edge_collapse_candidates: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(count_ok(m), "vfn_edge_collapse_candidates: m %lld outside [1, 2^31)", (long long)m);
    VFN_REQUIRE(n_items >= 1 && n_items < (1ll << 35), "vfn_edge_collapse_candidates: n_items %lld outside [1, 2^35)", (long long)n_items);
    VFN_REQUIRE(rows >= m && rows <= 4 * m, "vfn_edge_collapse_candidates: rows %lld outside [m = %lld, 4 m]", (long long)rows, (long long)m);
    VFN_REQUIRE(n_edges >= 1 && n_edges <= 3 * m, "vfn_edge_collapse_candidates: n_edges %lld outside [1, 3 m = %lld]", (long long)n_edges,
                (long long)(3 * m));
    VFN_REQUIRE(vertices && faces && quadrics && item_row && start && edge_a && edge_b && run && origin && point && cost && s && flags && info,
                "vfn_edge_collapse_candidates: NULL argument");
    VFN_REQUIRE(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]), "vfn_edge_collapse_candidates: a non-finite origin");
    VFN_REQUIRE(isfinite(rcond) && rcond >= 0.0 && rcond <= 1.0, "vfn_edge_collapse_candidates: rcond %g outside [0, 1]", rcond);
    VFN_REQUIRE(isfinite(reach) && reach >= 0.0 && isfinite(reach * reach), "vfn_edge_collapse_candidates: reach %g is not finite and >= 0 with a finite square",
                reach);
    VFN_REQUIRE(max_error >= 0.0, "vfn_edge_collapse_candidates: max_error %g is not >= 0 (+inf: no bound)", max_error);
    Mesh g;
    g.v = vertices; g.n = n; g.f = (const long long*)faces; g.m = m; g.q = quadrics; g.item_row = (const long long*)item_row; g.n_items = n_items;
    g.start = (const long long*)start; g.rows = rows; g.o[0] = origin[0]; g.o[1] = origin[1]; g.o[2] = origin[2];
    g.rcond = rcond; g.reach = reach; g.max_error = max_error;
    hipLaunchKernelGGL(vfn_edge_candidates_kernel, dim3(blocks_for(n_edges)), dim3(COL_BLOCK), 0, (hipStream_t)stream, g, (const long long*)edge_a,
                       (const long long*)edge_b, (const long long*)run, (long long)n_edges, point, cost, s, (unsigned char*)flags,
                       (unsigned long long*)info);
    return vfn_check_launch("vfn_edge_collapse_candidates");
}

extern "C" int vfn_collapse_select(const double* cost, const uint8_t* flags, const int64_t* edge_a, const int64_t* edge_b, int64_t n_edges,
                                   const int64_t* faces, int64_t m, int64_t n, int64_t* best_cost, int64_t* best_edge, uint8_t* proposed,
                                   uint8_t* withdrawn, int64_t* info, void* stream) {
    VFN_REQUIRE(count_ok(n), "vfn_collapse_select: n %lld outside [1, 2^31)", (long long)n);
    VFN_REQUIRE(count_ok(m), "vfn_collapse_select: m %lld outside [1, 2^31)", (long long)m);
    VFN_REQUIRE(n_edges >= 1 && n_edges <= 3 * m, "vfn_collapse_select: n_edges %lld outside [1, 3 m = %lld]", (long long)n_edges, (long long)(3 * m));
    VFN_REQUIRE(cost && flags && edge_a && edge_b && faces && best_cost && best_edge && proposed && withdrawn && info, "vfn_collapse_select: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const long long* ea = (const long long*)edge_a;
    const long long* eb = (const long long*)edge_b;
    unsigned long long* bc = (unsigned long long*)best_cost;
    long long* be = (long long*)best_edge;
    unsigned long long* word = (unsigned long long*)info;
    hipLaunchKernelGGL(vfn_select_fill_kernel, dim3(blocks_for(n)), dim3(COL_BLOCK), 0, st, bc, be, (long long)n);
    hipLaunchKernelGGL(vfn_select_cost_kernel, dim3(blocks_for(n_edges)), dim3(COL_BLOCK), 0, st, cost, (const unsigned char*)flags, ea, eb,
                       (long long)n_edges, (long long)n, bc, word);
    hipLaunchKernelGGL(vfn_select_edge_kernel, dim3(blocks_for(n_edges)), dim3(COL_BLOCK), 0, st, cost, (const unsigned char*)flags, ea, eb,
                       (long long)n_edges, (long long)n, (const unsigned long long*)bc, be, word);
    hipLaunchKernelGGL(vfn_select_propose_kernel, dim3(blocks_for(n_edges)), dim3(COL_BLOCK), 0, st, (const unsigned char*)flags, ea, eb,
                       (long long)n_edges, (long long)n, (const long long*)be, (unsigned char*)proposed, (unsigned char*)withdrawn, word);
    hipLaunchKernelGGL(vfn_select_withdraw_kernel, dim3(blocks_for(m)), dim3(COL_BLOCK), 0, st, (const long long*)faces, (long long)m, (long long)n, cost,
                       (long long)n_edges, (const long long*)be, (const unsigned char*)proposed, (unsigned char*)withdrawn, word);
    return vfn_check_launch("vfn_collapse_select");
}
