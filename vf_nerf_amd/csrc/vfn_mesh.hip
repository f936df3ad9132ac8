// vfn_mesh.hip — contrastive marching cubes on the device: evaluation/utils/marching_cubes_vt.py:186-315
// (contrastive_marching_cubes, combs_to_verts :62-101, vertex_interpolate :9-16), the last host stage of the evaluator's mesh
// pipeline (evaluation/methods.py:140-322).  The reference visits every surface cell in a Python loop and deduplicates vertices
// in a dict; here (count and emit are the extraction skeleton of vfn_mc_extract.h over the mesh source below):
//   count     one lane per cell POSITION in the reference's order: it evaluates the cell's eight corner values and case and writes
//             its triangle count; an ordered device scan (rocPRIM through hipCUB) gives every triangle its output slot.
//   emit      the same lanes again: the float64 corner positions of the cell's triangles at their slots (3 vertices per triangle,
//             slot = 3 x triangle + corner: the reference's order of first appearance).
//   dedup     one lane per vertex slot: an open-addressing table keyed on the canonical 24-byte position (-0.0 folded onto +0.0,
//             as a Python dict's float equality does).  The bucket is claimed with a 32-bit CAS, full keys are compared (never
//             hashes alone), and the bucket's owner is the MINIMUM slot (atomicMin), so the result does not depend on the order in
//             which the atomics arrive.
//   number    a flag (slot == owner) and a scan give every owner its vertex id (ids in order of first appearance); the owner's raw
//             bits (the first occurrence's) become vertices[V,3] and every slot's owner id becomes faces[F,3].
// Two input forms feed the same code: GENERAL (comb [M,28] + udf [M,28,2] + cell indices [M,3] or the dense raster, fp32 or fp64:
// what the reference's call site hands over, any comb table) and FUSED (the side byte per cell of vfn_grid_unify_direction_sides
// + the field norms [res^3]: the 28 + 56 values per cell of make_comb_format are never written).  Integer atomics at device
// scope only; no float atomics.  All arithmetic in fp64 with -ffp-contract=off (build.sh): the reference's numpy expressions,
// operation for operation.
#include "vfn_common.h"
#include "vfn_mc_extract.h"    // TRI / EDGE_A / EDGE_B / INC, the ordered scan, count -> scan -> total -> emit over a source

namespace {

// the host copies vfn_mesh_tables hands out (it pads the entries after a row's -1 with -1)
const signed char TRI_HOST[256][16] = {VFN_MC_TRI_ROWS};
const int EDGE_A_HOST[12] = VFN_MC_EDGE_A;
const int EDGE_B_HOST[12] = VFN_MC_EDGE_B;
// the 28 corner pairs (a < b) in the order of marching_cubes_vt.combs, and pair index of (a, b) for a < b
__device__ __constant__ unsigned char PA[28] = VFN_MC_PAIR_A;
__device__ __constant__ unsigned char PB[28] = VFN_MC_PAIR_B;

__device__ __forceinline__ int pair_index(int a, int b) {     // a < b
    return a * 7 - a * (a - 1) / 2 + (b - a - 1);
}

constexpr unsigned STATUS_NONFINITE = 1u, STATUS_INDEX = 2u;

// the mesh source of vfn_mc_extract.h, in its general and fused forms
struct MeshArgs {
    using Value = double;
    struct Emit { double P[8][3]; };     // the cell's corner positions
    int form;                     // VFN_MESH_GENERAL | VFN_MESH_FUSED
    const void* comb;             // general: [m, 28]
    const void* udf;              // general: [m, 28, 2] or NULL
    int f64;                      // general: comb / udf are double (else float)
    const long long* cells;       // general: [m, 3] or NULL (the dense raster: m == res^3)
    const unsigned char* sides;   // fused: [res^3]
    const float* norms;           // fused: [res^3]
    long long m;                  // cell positions
    int res;
    double size, iso;

    __host__ __device__ long long positions() const { return m; }
    __device__ bool eval(long long p, int c[3], double v[8], int& top, unsigned& status) const;
    __device__ void emit_setup(const int c[3], Emit& em) const;
    __device__ void vertex(const int c[3], const double v[8], const Emit& em, int e, double out[3]) const;
};

__device__ __forceinline__ double grid_pos(int i, int res, double size) {
    return (double)i / (double)res * size - size / 2.0;     // mgrid / res * size - size / 2 (no contraction: -ffp-contract=off)
}

__device__ __forceinline__ bool finite(double x) { return x - x == 0.0; }

// combs_to_verts (:62-101) on one row of the general form: the corner values, and whether they came from udf (max comb > 0.5)
template <typename T>
__device__ bool general_values(const T* __restrict__ comb, const T* __restrict__ udf, double v[8]) {
    T mx = comb[0];
    int am = 0;
    bool nan = comb[0] != comb[0];
    for (int q = 1; q < 28; ++q) {
        const T x = comb[q];
        nan |= x != x;
        if (x > mx) { mx = x; am = q; }                           // first maximum (np.argmax)
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = 0.0;
    if (nan || !(mx > (T)0.5)) return false;                     // (np.max of a row holding a NaN is NaN: not > 0.5)
    const int a0 = PA[am], a1 = PB[am];
    unsigned cls1 = 1u << a1;
    for (int q = 0; q < 8; ++q) {
        if (q == a0 || q == a1) continue;
        const T c0 = comb[pair_index(min(q, a0), max(q, a0))], c1 = comb[pair_index(min(q, a1), max(q, a1))];
        if (c0 > c1) cls1 |= 1u << q;
    }
    for (int q = 0; q < 8; ++q) {
        const bool one = (cls1 >> q) & 1u;
        if (!udf) v[q] = one ? 1.0 : 0.0;
        else v[q] = (one ? 1.0 : -1.0) * (double)udf[q == 0 ? 0 : 2 * (q - 1) + 1];   // idx_in_combs: [0,0] [0,1] [1,1] .. [6,1]
    }
    return true;
}

// one cell position: its grid coordinates, corner values and case.  Returns false for a position that yields nothing.
__device__ bool MeshArgs::eval(long long p, int c[3], double v[8], int& top, unsigned& status) const {
    const long long r = res;
    bool from_norms;
    if (form == VFN_MESH_FUSED) {
        // evaluation/methods.py:184-188: (res/2)^3 blocks of 2x2x2 cells in raster order, corner order inside a block
        const long long blk = p >> 3, h = r >> 1;
        const int q = (int)(p & 7);
        c[0] = (int)(blk / (h * h)) * 2 + INC[q][0];
        c[1] = (int)((blk / h) % h) * 2 + INC[q][1];
        c[2] = (int)(blk % h) * 2 + INC[q][2];
        const long long cell = ((long long)c[0] * r + c[1]) * r + c[2];
        if (!finite((double)norms[cell])) status |= STATUS_NONFINITE;      // every grid point is corner 0 of one position
        const unsigned bits = sides[cell];
        if (bits == 0u || bits == 0xffu) return false;           // comb all zero: max 0 <= 0.5, no triangles
        // comb(a, b) = bit_a ^ bit_b: the anchor pair is (0, first corner unlike 0), and corner v sides with the second anchor iff
        // its bit differs from corner 0's: value = (bit_v != bit_0 ? +1 : -1) x norm(corner v), norm 0 outside the grid
        const unsigned b0 = bits & 1u;
#pragma unroll
        for (int q2 = 0; q2 < 8; ++q2) {
            const int ii = c[0] + INC[q2][0], jj = c[1] + INC[q2][1], kk = c[2] + INC[q2][2];
            const float nv = (ii < r && jj < r && kk < r) ? norms[((long long)ii * r + jj) * r + kk] : 0.f;
            v[q2] = (((bits >> q2) & 1u) != b0 ? 1.0 : -1.0) * (double)nv;
        }
        from_norms = true;
    } else {
        if (cells) {
            for (int d = 0; d < 3; ++d) {
                const long long x = cells[p * 3 + d];
                if (x < 0 || x >= r) { status |= STATUS_INDEX; return false; }
                c[d] = (int)x;
            }
        } else {
            c[0] = (int)(p / (r * r)); c[1] = (int)((p / r) % r); c[2] = (int)(p % r);
        }
        if (f64) from_norms = general_values<double>((const double*)comb + p * 28, udf ? (const double*)udf + p * 56 : nullptr, v);
        else from_norms = general_values<float>((const float*)comb + p * 28, udf ? (const float*)udf + p * 56 : nullptr, v);
    }
    int t = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) t |= (v[q] < iso ? 1 : 0) << q;
    top = t;
    if (t == 0 || t == 255) return false;                      // EDGE_TABLE[0] = EDGE_TABLE[255] = 0: no edge is cut
    if (from_norms && form != VFN_MESH_FUSED)
        for (int q = 0; q < 8; ++q)
            if (!finite(v[q])) status |= STATUS_NONFINITE;
    return true;
}

// vertex_interpolate (:9-16): swap when p1 > p2 in any component, interpolate only when |v1 - v2| > 1e-5
__device__ __forceinline__ void MeshArgs::vertex(const int[3], const double v[8], const Emit& em, int e, double out[3]) const {
    const double (*P)[3] = em.P;
    int e1 = EDGE_A[e], e2 = EDGE_B[e];
    if (P[e1][0] > P[e2][0] || P[e1][1] > P[e2][1] || P[e1][2] > P[e2][2]) { const int t = e1; e1 = e2; e2 = t; }
    const double v1 = v[e1], v2 = v[e2];
    if (fabs(v1 - v2) > 1e-5) {
        for (int d = 0; d < 3; ++d) out[d] = P[e1][d] + (P[e2][d] - P[e1][d]) * (iso - v1) / (v2 - v1);
    } else {
        for (int d = 0; d < 3; ++d) out[d] = P[e1][d];
    }
}

__device__ __forceinline__ void MeshArgs::emit_setup(const int c[3], Emit& em) const {
#pragma unroll
    for (int q = 0; q < 8; ++q)
        for (int d = 0; d < 3; ++d) em.P[q][d] = grid_pos(c[d] + INC[q][d], res, size);
}

// ---- deduplication ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long canon(double x) {
    return x == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(x);     // 0.0 == -0.0 in a dict: one key
}

__device__ __forceinline__ unsigned long long mix(unsigned long long h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}

__global__ void vfn_mesh_table_init_kernel(int* __restrict__ table, int* __restrict__ owner, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { table[i] = -1; owner[i] = 0x7fffffff; }
}

__global__ __launch_bounds__(256) void vfn_mesh_dedup_kernel(const double* __restrict__ tv, long long n_slots, int* __restrict__ table,
                                                             int* __restrict__ owner, long long mask, int* __restrict__ bucket) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const unsigned long long k0 = canon(tv[s * 3]), k1 = canon(tv[s * 3 + 1]), k2 = canon(tv[s * 3 + 2]);
    long long h = (long long)(mix(k0 ^ mix(k1 ^ mix(k2))) & (unsigned long long)mask);
    for (;;) {
        int cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur < 0) {
            const int prev = atomicCAS(&table[h], -1, (int)s);
            if (prev < 0) break;                                  // claimed: this slot's key lives in bucket h
            cur = prev;
        }
        // the bucket holds some slot's key (written by the emit launch, complete before this one started): compare all 24 bytes
        if (canon(tv[(long long)cur * 3]) == k0 && canon(tv[(long long)cur * 3 + 1]) == k1 && canon(tv[(long long)cur * 3 + 2]) == k2) break;
        h = (h + 1) & mask;
    }
    bucket[s] = (int)h;
    atomicMin(&owner[h], (int)s);                                  // the first appearance owns the key, whoever claimed the bucket
}

__global__ __launch_bounds__(256) void vfn_mesh_flag_kernel(const int* __restrict__ owner, const int* __restrict__ bucket, long long n_slots,
                                                            int* __restrict__ flag) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_slots) flag[s] = owner[bucket[s]] == (int)s ? 1 : 0;
}

__global__ __launch_bounds__(256) void vfn_mesh_number_kernel(const double* __restrict__ tv, long long n_slots, const int* __restrict__ owner,
                                                              const int* __restrict__ bucket, const int* __restrict__ vid_incl,
                                                              double* __restrict__ vertices, long long* __restrict__ faces) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int o = owner[bucket[s]];
    const int id = vid_incl[o] - 1;                                // the owner is flagged: its inclusive count includes itself
    faces[s] = id;
    if (o == (int)s) {
        vertices[(long long)id * 3] = tv[s * 3];
        vertices[(long long)id * 3 + 1] = tv[s * 3 + 1];
        vertices[(long long)id * 3 + 2] = tv[s * 3 + 2];
    }
}

// evaluation/methods.py:223-226 on the device: norms = torch.norm(x, dim=1) as torch's CPU kernel evaluates it (the FMA chain
// fma(z, z, fma(y, y, x x)), then a correctly rounded sqrt) and unit = F.normalize(x, dim=1) = x / max(norm, 1e-12)
__global__ __launch_bounds__(256) void vfn_mesh_field_norms_kernel(const float* __restrict__ x, long long n, float* __restrict__ norms,
                                                                   float* __restrict__ unit) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = x[i * 3], b = x[i * 3 + 1], c = x[i * 3 + 2];
    const float nr = sqrtf(fmaf(c, c, fmaf(b, b, a * a)));
    norms[i] = nr;
    if (unit) {
        const float d = fmaxf(nr, 1e-12f);
        unit[i * 3] = a / d; unit[i * 3 + 1] = b / d; unit[i * 3 + 2] = c / d;
    }
}

int make_args(MeshArgs& a, int32_t form, const void* comb, const void* udf, int32_t f64, const int64_t* cells, const uint8_t* sides,
              const float* norms, int64_t m, int32_t res, double size, double isovalue, const char* what) {
    a = MeshArgs{};
    a.form = form; a.comb = comb; a.udf = udf; a.f64 = f64; a.cells = (const long long*)cells; a.sides = sides; a.norms = norms;
    a.m = m; a.res = res; a.size = size; a.iso = isovalue;
    VFN_REQUIRE(res >= 1 && res <= 2048 && m >= 0 && m < (1ll << 31), "%s: bad res %d / m %lld", what, res, (long long)m);
    if (form == VFN_MESH_FUSED) {
        VFN_REQUIRE(sides && norms, "%s: fused form needs sides and norms", what);
        VFN_REQUIRE(res % 2 == 0 && res <= 1024 && m == (int64_t)res * res * res, "%s: fused form needs an even res <= 1024 and m = res^3", what);
    } else {
        VFN_REQUIRE(form == VFN_MESH_GENERAL, "%s: unknown form %d", what, form);
        VFN_REQUIRE(m == 0 || comb, "%s: NULL comb", what);
        VFN_REQUIRE(cells || m == (int64_t)res * res * res, "%s: dense form needs m = res^3", what);
    }
    return VFN_OK;
}

}  // namespace

extern "C" int vfn_mesh_tables(int32_t* edge_table, int32_t* edge_vertex, int8_t* tri_table) {
    VFN_REQUIRE(edge_table && edge_vertex && tri_table, "vfn_mesh_tables: NULL argument");
    for (int c = 0; c < 256; ++c) {
        int m = 0;
        for (int e = 0; e < 12; ++e)
            if (((c >> EDGE_A_HOST[e]) ^ (c >> EDGE_B_HOST[e])) & 1) m |= 1 << e;
        edge_table[c] = m;
        bool ended = false;
        for (int t = 0; t < 16; ++t) {
            ended = ended || TRI_HOST[c][t] < 0;
            tri_table[c * 16 + t] = ended ? (int8_t)-1 : (int8_t)TRI_HOST[c][t];
        }
    }
    for (int e = 0; e < 12; ++e) { edge_vertex[2 * e] = EDGE_A_HOST[e]; edge_vertex[2 * e + 1] = EDGE_B_HOST[e]; }
    return VFN_OK;
}

extern "C" int64_t vfn_mesh_scan_workspace_bytes(int64_t n) {
    size_t b = 0;
    if (n < 1) n = 1;
    if (vfn_mc_scan_bytes(n, &b) != VFN_OK) return -1;
    return (int64_t)b;
}

extern "C" int vfn_mesh_count(int32_t form, const void* comb, const void* udf, int32_t f64, const int64_t* cells, const uint8_t* sides,
                              const float* norms, int64_t m, int32_t res, double size, double isovalue, int32_t* counts, int32_t* offsets,
                              int64_t* info, void* scan_ws, int64_t scan_ws_bytes, void* stream) {
    MeshArgs a;
    const int rc = make_args(a, form, comb, udf, f64, cells, sides, norms, m, res, size, isovalue, "vfn_mesh_count");
    if (rc != VFN_OK) return rc;
    return vfn_mc_count(a, counts, offsets, info, scan_ws, scan_ws_bytes, (hipStream_t)stream, "vfn_mesh_count");
}

extern "C" int vfn_mesh_emit(int32_t form, const void* comb, const void* udf, int32_t f64, const int64_t* cells, const uint8_t* sides,
                             const float* norms, int64_t m, int32_t res, double size, double isovalue, const int32_t* counts,
                             const int32_t* offsets, double* tri_verts, void* stream) {
    MeshArgs a;
    const int rc = make_args(a, form, comb, udf, f64, cells, sides, norms, m, res, size, isovalue, "vfn_mesh_emit");
    if (rc != VFN_OK) return rc;
    return vfn_mc_emit(a, counts, offsets, tri_verts, (hipStream_t)stream, "vfn_mesh_emit");
}

extern "C" int vfn_mesh_dedup(const double* tri_verts, int64_t n_slots, int32_t* table, int32_t* owner, int64_t table_size, int32_t* bucket,
                              int32_t* flags, int32_t* vid, int64_t* info, void* scan_ws, int64_t scan_ws_bytes, void* stream) {
    VFN_REQUIRE(info && n_slots >= 0 && n_slots < (1ll << 31), "vfn_mesh_dedup: bad argument (n_slots %lld)", (long long)n_slots);
    hipStream_t s = (hipStream_t)stream;
    if (n_slots > 0) {
        VFN_REQUIRE(tri_verts && table && owner && bucket && flags && vid, "vfn_mesh_dedup: NULL argument");
        VFN_REQUIRE(table_size >= 2 * n_slots && (table_size & (table_size - 1)) == 0, "vfn_mesh_dedup: table size %lld is not a power of two "
                    ">= 2 x %lld slots", (long long)table_size, (long long)n_slots);
        hipLaunchKernelGGL(vfn_mesh_table_init_kernel, dim3(blocks_for(table_size)), dim3(256), 0, s, (int*)table, (int*)owner, (long long)table_size);
        hipLaunchKernelGGL(vfn_mesh_dedup_kernel, dim3(blocks_for(n_slots)), dim3(256), 0, s, tri_verts, (long long)n_slots, (int*)table,
                           (int*)owner, (long long)(table_size - 1), (int*)bucket);
        hipLaunchKernelGGL(vfn_mesh_flag_kernel, dim3(blocks_for(n_slots)), dim3(256), 0, s, (const int*)owner, (const int*)bucket,
                           (long long)n_slots, (int*)flags);
        const int rc = vfn_mc_inclusive_scan(flags, vid, n_slots, scan_ws, scan_ws_bytes, s, "vfn_mesh_dedup");
        if (rc != VFN_OK) return rc;
    }
    hipLaunchKernelGGL(vfn_mc_total_kernel, dim3(1), dim3(64), 0, s, (const int*)vid, (long long)(n_slots - 1), (long long*)info, 2);
    return vfn_check_launch("vfn_mesh_dedup");
}

extern "C" int vfn_mesh_number(const double* tri_verts, int64_t n_slots, const int32_t* owner, const int32_t* bucket, const int32_t* vid,
                               double* vertices, int64_t* faces, void* stream) {
    if (n_slots <= 0) return VFN_OK;
    VFN_REQUIRE(tri_verts && owner && bucket && vid && vertices && faces && n_slots < (1ll << 31), "vfn_mesh_number: bad argument");
    hipLaunchKernelGGL(vfn_mesh_number_kernel, dim3(blocks_for(n_slots)), dim3(256), 0, (hipStream_t)stream, tri_verts, (long long)n_slots,
                       (const int*)owner, (const int*)bucket, (const int*)vid, vertices, (long long*)faces);
    return vfn_check_launch("vfn_mesh_number");
}

extern "C" int vfn_mesh_field_norms(const float* field, int64_t n, float* norms, float* unit, void* stream) {
    if (n <= 0) return VFN_OK;
    VFN_REQUIRE(field && norms, "vfn_mesh_field_norms: NULL argument");
    hipLaunchKernelGGL(vfn_mesh_field_norms_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, field, (long long)n, norms, unit);
    return vfn_check_launch("vfn_mesh_field_norms");
}
