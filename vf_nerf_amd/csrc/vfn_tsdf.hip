// vfn_tsdf.hip — a dense truncated-signed-distance volume on the device: the stage between the rendered depth maps and the mesh that
// evaluation/methods.py:613-665 (tsdf_mesh) reports, with the semantics of a uniform TSDF volume (projective integration with a
// running mean, extraction of the zero level set with classic marching cubes).  include/vfn.h states the arithmetic; here:
//   integrate  ONE pass over the volume for ALL views of a call.  A lane owns RUN = 4 consecutive k voxels (16-B loads and stores of
//              tsdf and weight), keeps them in registers and applies the views in index order, rounding after each: the bits of V
//              single-view calls.  A workgroup covers a brick of 4 x 8 x 32 voxels; its 256 lanes first test one view each against the
//              brick (below), the ballots go to LDS, and every wave then walks the set bits in ascending order — the view index is
//              wave-uniform, so the 16 per-view parameters are scalar loads, not per-lane ones.  The depth reads are gathers:
//              neighbouring lanes project to neighbouring pixels and the caches serve them.  The dense and the block-sparse kernel are
//              ONE code path around their own index derivation: load_vec / store_vec (a run and its 12 colour floats, 16 B at a time),
//              apply_views<lanes> (brick test, ballots, the walk) and integrate_view (the arithmetic).  Only the dense kernel has a
//              scalar form, for rows that are no multiple of four voxels or arrays off the 16-B boundary; it is written there.
//   brick test A view is skipped for a brick only when NO voxel centre of the brick can pass the per-voxel tests.  The test uses the
//              voxel's own fp32 expressions at the brick's extreme centres: every operation of x -> xc -> (xc fx) / zc + cx + 0.5 is
//              monotone in each operand once the signs of the coefficients are fixed, and rounding keeps order (a <= b gives
//              fl(a) <= fl(b)), so the extreme of the ROUNDED value over the brick is the rounded value at a corner — no margin, no
//              second arithmetic.  A NaN anywhere makes every comparison false and the view is kept.
//   count/emit the extraction skeleton of vfn_mc_extract.h over the TSDF source below, one lane per cell in C order: the case from the
//              signs of the eight corner values (a corner with weight 0 voids the cell), the triangle count, the ordered scan, then
//              every triangle's three float64 vertices at their slots in the layout vfn_mesh_dedup / vfn_mesh_number consume.  A vertex is a function of its edge alone, so the (up to) four
//              cells around an edge emit identical bits and the positional merge joins them.
//   colour     the COLOUR instantiation of the integration kernel carries a lane's 4 x 3 colour floats next to tsdf and weight (three
//              16-B accesses in the vector form) and reads the pixel's three bytes with byte loads, issued with the depth load; the
//              colourless instantiation is the code it was (the colour arguments are an empty record at the END of its arguments).
//              emit_colours is a second source over the same skeleton whose vertex() is a colour (colour_at, for both volumes, from the
//              two voxel indices a source computes); vertex_colours picks, per vertex,
//              the colour of the lowest slot that carries its id (an integer atomicMin per slot, then a gather).
// No floating-point atomics.  fp32 (integration) and fp64 (vertices, colours) without contraction: -ffp-contract=off (build.sh),
// correctly rounded / and sqrtf.
#include "vfn_common.h"
#include "vfn_mc_extract.h"    // EDGE_A / EDGE_B / INC, count -> scan -> total -> emit over a source

namespace {

constexpr int RUN = 4;                     // consecutive k voxels of a lane: one 16-B access per array
constexpr int BK_RUNS = 8, BJ = 8, BI = 4; // lanes of a workgroup along k (runs), j, i: a brick of 4 x 8 x 32 voxels, one i-slab per wave
constexpr int BK = BK_RUNS * RUN;
constexpr int THREADS = BK_RUNS * BJ * BI;
static_assert(THREADS == 256, "one view per lane in the brick test, four ballots per round");

struct Volume {
    float* tsdf;
    float* weight;
    int nx, ny, nz;
    float ox, oy, oz, vl, trunc;
};

struct Views {
    const float* depth;        // [V, H, W]
    const float* intr;         // [V, 4]: fx fy cx cy
    const float* extr;         // [V, 12]: world -> camera rows
    int n, h, w;
};

// what the COLOUR instantiation adds to the kernel's arguments; empty without colour
template <bool COLOUR> struct Colour {};
template <> struct Colour<true> {
    float* colour;             // [nx, ny, nz, 3], byte units
    const unsigned char* rgb;  // [V, H, W, 3]
};

__device__ __forceinline__ float centre(float o, int i, float vl) { return o + ((float)i + 0.5f) * vl; }

__device__ __forceinline__ float cam_row(const float* __restrict__ e, float x, float y, float z) {
    return ((e[0] * x + e[1] * y) + e[2] * z) + e[3];
}

// the largest / smallest ROUNDED value of cam_row over the box [lo, hi]^3 of voxel centres: at the corner the coefficient signs select
__device__ __forceinline__ float row_max(const float* __restrict__ e, const float lo[3], const float hi[3]) {
    return cam_row(e, e[0] >= 0.f ? hi[0] : lo[0], e[1] >= 0.f ? hi[1] : lo[1], e[2] >= 0.f ? hi[2] : lo[2]);
}
__device__ __forceinline__ float row_min(const float* __restrict__ e, const float lo[3], const float hi[3]) {
    return cam_row(e, e[0] >= 0.f ? lo[0] : hi[0], e[1] >= 0.f ? lo[1] : hi[1], e[2] >= 0.f ? lo[2] : hi[2]);
}

// One image axis: can floorf(((c f) / zc + p) + 0.5f) lie in [0, size) for some c in [c_lo, c_hi], zc in [z_lo, z_hi], zc > 0?
// (f > 0.)  n / zc with zc > 0 falls with zc where n >= 0 and rises where n < 0; without a positive lower bound of zc a positive
// quotient is unbounded.  false only when every candidate is provably outside.
__device__ __forceinline__ bool axis_may_hit(float c_lo, float c_hi, float z_lo, float z_hi, float f, float p, float size) {
    const float n_hi = c_hi * f, n_lo = c_lo * f;
    if (n_hi < 0.f) {                                         // largest quotient at the largest zc
        if (((n_hi / z_hi + p) + 0.5f) < 0.f) return false;
    } else if (n_hi >= 0.f && z_lo > 0.f) {                   // largest quotient at the smallest zc
        if (((n_hi / z_lo + p) + 0.5f) < 0.f) return false;
    }
    if (n_lo >= 0.f) {                                        // smallest quotient at the largest zc
        if (((n_lo / z_hi + p) + 0.5f) >= size) return false;
    } else if (n_lo < 0.f && z_lo > 0.f) {                    // smallest quotient at the smallest zc
        if (((n_lo / z_lo + p) + 0.5f) >= size) return false;
    }
    return true;
}

__device__ bool brick_may_see(const float* __restrict__ e, const float* __restrict__ k, const float lo[3], const float hi[3], float wf, float hf) {
    const float z_hi = row_max(e + 8, lo, hi);
    if (z_hi <= 0.f) return false;                            // zc <= 0 for every voxel of the brick
    const float fx = k[0], fy = k[1];
    if (!(fx > 0.f) || !(fy > 0.f)) return true;              // (the monotonicity argument needs positive focal lengths)
    const float z_lo = row_min(e + 8, lo, hi);
    if (!axis_may_hit(row_min(e, lo, hi), row_max(e, lo, hi), z_lo, z_hi, fx, k[2], wf)) return false;
    if (!axis_may_hit(row_min(e + 4, lo, hi), row_max(e + 4, lo, hi), z_lo, z_hi, fy, k[3], hf)) return false;
    return true;
}

// A lane's run of RUN consecutive k voxels lives in registers as ts / wt / col, arrays of the KERNEL: both integrating kernels load them
// here, update them view by view and store them here.  `off` is the run's first voxel in the arrays; a lane's 12 colour floats are
// contiguous there, three 16-B accesses.  (The arrays are not members of one record: hipcc then allocates all six kernels differently
// and gives the scalar colour form 100 B of scratch per lane, see profiles/r24.)
template <bool COLOUR>
__device__ __forceinline__ void load_vec(float ts[RUN], float wt[RUN], float (*col)[3], const float* tsdf, const float* weight,
                                         const Colour<COLOUR>& cl, long long off) {
    const float4 a = *reinterpret_cast<const float4*>(tsdf + off), c = *reinterpret_cast<const float4*>(weight + off);
    ts[0] = a.x; ts[1] = a.y; ts[2] = a.z; ts[3] = a.w;
    wt[0] = c.x; wt[1] = c.y; wt[2] = c.z; wt[3] = c.w;
    if constexpr (COLOUR) {
        const float4* __restrict__ q = reinterpret_cast<const float4*>(cl.colour + off * 3);
        const float4 p = q[0], b4 = q[1], d = q[2];
        col[0][0] = p.x; col[0][1] = p.y; col[0][2] = p.z; col[1][0] = p.w;
        col[1][1] = b4.x; col[1][2] = b4.y; col[2][0] = b4.z; col[2][1] = b4.w;
        col[2][2] = d.x; col[3][0] = d.y; col[3][1] = d.z; col[3][2] = d.w;
    }
}

template <bool COLOUR>
__device__ __forceinline__ void store_vec(const float ts[RUN], const float wt[RUN], const float (*col)[3], float* tsdf, float* weight,
                                          const Colour<COLOUR>& cl, long long off) {
    *reinterpret_cast<float4*>(tsdf + off) = make_float4(ts[0], ts[1], ts[2], ts[3]);
    *reinterpret_cast<float4*>(weight + off) = make_float4(wt[0], wt[1], wt[2], wt[3]);
    if constexpr (COLOUR) {
        float4* __restrict__ q = reinterpret_cast<float4*>(cl.colour + off * 3);
        q[0] = make_float4(col[0][0], col[0][1], col[0][2], col[1][0]);
        q[1] = make_float4(col[1][1], col[1][2], col[2][0], col[2][1]);
        q[2] = make_float4(col[2][2], col[3][0], col[3][1], col[3][2]);
    }
}

// one view into the RUN voxels of a lane (include/vfn.h: the association is the contract)
template <bool COLOUR>
__device__ __forceinline__ void integrate_view(const Views& vs, const Colour<COLOUR>& cl, int view, float x, float y, const float z[RUN], int cnt,
                                               float trunc, float ts[RUN], float wt[RUN], float (*col)[3]) {
    const float* __restrict__ e = vs.extr + (long long)view * 12;
    const float* __restrict__ k = vs.intr + (long long)view * 4;
    const float* __restrict__ dv = vs.depth + (long long)view * vs.h * vs.w;
    const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
    const float wf = (float)vs.w, hf = (float)vs.h;
    const float px = e[0] * x + e[1] * y, py = e[4] * x + e[5] * y, pz = e[8] * x + e[9] * y;      // (the z-independent sums)
#pragma unroll
    for (int r = 0; r < RUN; ++r) {
        if (r >= cnt) continue;
        const float zc = (pz + e[10] * z[r]) + e[11];
        if (!(zc > 0.f)) continue;
        const float xc = (px + e[2] * z[r]) + e[3], yc = (py + e[6] * z[r]) + e[7];
        const float u = floorf(((xc * fx) / zc + cx) + 0.5f), v = floorf(((yc * fy) / zc + cy) + 0.5f);
        if (!(u >= 0.f && u < wf && v >= 0.f && v < hf)) continue;
        const long long pix = (long long)(int)v * vs.w + (int)u;
        const float d = dv[pix];
        float p[3] = {0.f, 0.f, 0.f};
        if constexpr (COLOUR) {                               // the pixel the depth is read from; issued with it, used only below
            const unsigned char* __restrict__ px = cl.rgb + ((long long)view * vs.h * vs.w + pix) * 3;
            p[0] = (float)px[0]; p[1] = (float)px[1]; p[2] = (float)px[2];
        }
        if (!(d > 0.f)) continue;
        const float a = (u - cx) / fx, b = (v - cy) / fy;
        const float m = sqrtf((1.0f + a * a) + b * b);
        const float sdf = (d - zc) * m;
        if (!(sdf > -trunc)) continue;
        const float t = fminf(1.0f, sdf / trunc);
        if constexpr (COLOUR) {                               // with the weight BEFORE its increment
#pragma unroll
            for (int c = 0; c < 3; ++c) col[r][c] = (col[r][c] * wt[r] + p[c]) / (wt[r] + 1.0f);
        }
        ts[r] = (ts[r] * wt[r] + t) / (wt[r] + 1.0f);
        wt[r] = wt[r] + 1.0f;
    }
}

// All views of a call into a lane's run, by a workgroup of N lanes whose voxel centres lie in the box [lo, hi]: every lane tests one view
// per round against the box, the ballots go to the N / 64 words of `seen` in LDS, and each wave walks the set bits in ascending order
// (the view index is wave-uniform).  Every lane of the workgroup arrives here, one without voxels with cnt == 0.  (`seen` is the
// kernel's own __shared__ array: with a function-scope one hipcc generates other code for the dense kernels, see profiles/r24.)
template <int N, bool COLOUR>
__device__ __forceinline__ void apply_views(const Views& vs, const Colour<COLOUR>& cl, const float lo[3], const float hi[3], float x, float y,
                                            const float z[RUN], int cnt, float trunc, float ts[RUN], float wt[RUN], float (*col)[3],
                                            unsigned long long* seen) {
    static_assert(N % 64 == 0, "whole waves: one ballot word each");
    const int t = threadIdx.x;
    const float wf = (float)vs.w, hf = (float)vs.h;
    for (int base = 0; base < vs.n; base += N) {
        const int mine = base + t;
        const bool may = mine < vs.n && brick_may_see(vs.extr + (long long)mine * 12, vs.intr + (long long)mine * 4, lo, hi, wf, hf);
        const unsigned long long ballot = __ballot(may);
        if ((t & 63) == 0) seen[t >> 6] = ballot;
        __syncthreads();
        for (int g = 0; g < N / 64; ++g) {
            const unsigned long long m64 = seen[g];
            unsigned m_lo = __builtin_amdgcn_readfirstlane((unsigned)m64), m_hi = __builtin_amdgcn_readfirstlane((unsigned)(m64 >> 32));
            while (m_lo) {                                    // ascending view order
                const int bit = __builtin_ctz(m_lo);
                m_lo &= m_lo - 1;
                integrate_view<COLOUR>(vs, cl, base + g * 64 + bit, x, y, z, cnt, trunc, ts, wt, col);
            }
            while (m_hi) {
                const int bit = __builtin_ctz(m_hi);
                m_hi &= m_hi - 1;
                integrate_view<COLOUR>(vs, cl, base + g * 64 + 32 + bit, x, y, z, cnt, trunc, ts, wt, col);
            }
        }
        __syncthreads();
    }
}

template <bool VEC, bool COLOUR>
__global__ __launch_bounds__(THREADS) void vfn_tsdf_integrate_kernel(Volume vol, Views vs, int nbj, int nbk, Colour<COLOUR> cl) {
    __shared__ unsigned long long seen[THREADS / 64];
    const long long b = blockIdx.x;
    const int bk = (int)(b % nbk), bj = (int)((b / nbk) % nbj), bi = (int)(b / ((long long)nbk * nbj));
    const int t = threadIdx.x;
    const int i = bi * BI + (t >> 6), j = bj * BJ + ((t >> 3) & 7), k0 = bk * BK + (t & 7) * RUN;
    const bool live = i < vol.nx && j < vol.ny && k0 < vol.nz;
    const int cnt = live ? min(RUN, vol.nz - k0) : 0;
    const long long off = ((long long)i * vol.ny + j) * vol.nz + k0;

    float ts[RUN] = {0.f, 0.f, 0.f, 0.f}, wt[RUN] = {0.f, 0.f, 0.f, 0.f}, z[RUN];
    float col[COLOUR ? RUN : 1][3] = {};                     // a lane's 12 contiguous colour floats
    if (live) {
        if (VEC) {
            load_vec<COLOUR>(ts, wt, col, vol.tsdf, vol.weight, cl, off);
        } else {                                              // rows that are no multiple of four voxels, arrays off the 16-B boundary
            for (int r = 0; r < cnt; ++r) { ts[r] = vol.tsdf[off + r]; wt[r] = vol.weight[off + r]; }
            if constexpr (COLOUR) {
                for (int r = 0; r < cnt; ++r)
                    for (int c = 0; c < 3; ++c) col[r][c] = cl.colour[(off + r) * 3 + c];
            }
        }
    }
    const float x = centre(vol.ox, i, vol.vl), y = centre(vol.oy, j, vol.vl);
#pragma unroll
    for (int r = 0; r < RUN; ++r) z[r] = centre(vol.oz, k0 + r, vol.vl);

    // the brick's extreme voxel centres (the same fp32 expression the lanes evaluate: monotone in the index)
    const float lo[3] = {centre(vol.ox, bi * BI, vol.vl), centre(vol.oy, bj * BJ, vol.vl), centre(vol.oz, bk * BK, vol.vl)};
    const float hi[3] = {centre(vol.ox, min(bi * BI + BI, vol.nx) - 1, vol.vl), centre(vol.oy, min(bj * BJ + BJ, vol.ny) - 1, vol.vl),
                         centre(vol.oz, min(bk * BK + BK, vol.nz) - 1, vol.vl)};
    apply_views<THREADS>(vs, cl, lo, hi, x, y, z, cnt, vol.trunc, ts, wt, col, seen);

    if (live) {
        if (VEC) {
            store_vec<COLOUR>(ts, wt, col, vol.tsdf, vol.weight, cl, off);
        } else {
            for (int r = 0; r < cnt; ++r) { vol.tsdf[off + r] = ts[r]; vol.weight[off + r] = wt[r]; }
            if constexpr (COLOUR) {
                for (int r = 0; r < cnt; ++r)
                    for (int c = 0; c < 3; ++c) cl.colour[(off + r) * 3 + c] = col[r][c];
            }
        }
    }
}

// ---- extraction -------------------------------------------------------------------------------------------------------
// cut edge e of a cell: its axis, and its endpoints as corner numbers — L the one with the lower lattice index, U the other
__device__ __forceinline__ void edge_ends(int e, int& ql, int& qu, int& axis) {
    const int qa = EDGE_A[e], qb = EDGE_B[e];
    axis = 0;
    if (INC[qa][1] != INC[qb][1]) axis = 1;
    if (INC[qa][2] != INC[qb][2]) axis = 2;
    const bool a_low = INC[qa][axis] < INC[qb][axis];
    ql = a_low ? qa : qb;
    qu = a_low ? qb : qa;
}

// the colour on a cut edge with endpoints ql / qu: the colours of their voxels il / iu of `colour`, mixed as the position is, in [0, 1]
__device__ __forceinline__ void colour_at(const float v[8], int ql, int qu, long long il, long long iu, const float* colour, double out[3]) {
    const double fl = fabs((double)v[ql]), fu = fabs((double)v[qu]);
    const double r = fl / (fl + fu);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        out[ch] = ((1.0 - r) * (double)colour[il * 3 + ch] + r * (double)colour[iu * 3 + ch]) / 255.0;
}

// the TSDF source of vfn_mc_extract.h: it never sets a status
struct Lattice {
    using Value = float;
    struct Emit {};
    const float* tsdf;
    const float* weight;
    int nx, ny, nz;
    long long cells;          // (nx - 1)(ny - 1)(nz - 1)
    float ox, oy, oz, vl;

    __host__ __device__ long long positions() const { return cells; }

    // cell p in C order: its lattice index, corner values and case; false for a cell that emits nothing
    __device__ __forceinline__ bool eval(long long p, int c[3], float v[8], int& top, unsigned&) const {
        const long long cz = nz - 1, cy = ny - 1;
        c[2] = (int)(p % cz);
        c[1] = (int)((p / cz) % cy);
        c[0] = (int)(p / (cz * cy));
        int t = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const long long idx = ((long long)(c[0] + INC[q][0]) * ny + (c[1] + INC[q][1])) * nz + (c[2] + INC[q][2]);
            if (weight[idx] == 0.f) return false;                 // an unobserved corner voids the cell
            v[q] = tsdf[idx];
            t |= (v[q] < 0.f ? 1 : 0) << q;                       // exactly 0 counts as outside
        }
        top = t;
        return t != 0 && t != 255;
    }

    __device__ __forceinline__ void emit_setup(const int[3], Emit&) const {}

    // the vertex of cut edge e of the cell: a function of the edge alone (its lower endpoint L, its axis, the two values)
    __device__ __forceinline__ void vertex(const int c[3], const float v[8], const Emit&, int e, double out[3]) const {
        int ql, qu, axis;
        edge_ends(e, ql, qu, axis);
        const double vld = (double)vl;
        const double o[3] = {(double)ox, (double)oy, (double)oz};
#pragma unroll
        for (int d = 0; d < 3; ++d) out[d] = o[d] + ((double)(c[d] + INC[ql][d]) + 0.5) * vld;
        const double fl = fabs((double)v[ql]), fu = fabs((double)v[qu]);
        out[axis] = out[axis] + (fl / (fl + fu)) * vld;
    }
};

// the same cells through the same skeleton, with a colour where the lattice source has a position (include/vfn.h: vfn_tsdf_emit_colours)
struct LatticeColours {
    using Value = float;
    using Emit = Lattice::Emit;
    Lattice at;
    const float* colour;      // [nx, ny, nz, 3]

    __host__ __device__ long long positions() const { return at.positions(); }
    __device__ __forceinline__ bool eval(long long p, int c[3], float v[8], int& top, unsigned& status) const { return at.eval(p, c, v, top, status); }
    __device__ __forceinline__ void emit_setup(const int[3], Emit&) const {}

    __device__ __forceinline__ void vertex(const int c[3], const float v[8], const Emit&, int e, double out[3]) const {
        int ql, qu, axis;
        edge_ends(e, ql, qu, axis);
        const long long il = ((long long)(c[0] + INC[ql][0]) * at.ny + (c[1] + INC[ql][1])) * at.nz + (c[2] + INC[ql][2]);
        const long long iu = ((long long)(c[0] + INC[qu][0]) * at.ny + (c[1] + INC[qu][1])) * at.nz + (c[2] + INC[qu][2]);
        colour_at(v, ql, qu, il, iu, colour, out);
    }
};

// first[v] = the lowest slot whose id is v (first is filled with a value above every slot before)
__global__ __launch_bounds__(256) void vfn_tsdf_first_slot_kernel(const long long* __restrict__ ids, long long n_slots, int* __restrict__ first,
                                                                  long long n_vert) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const long long v = ids[s];
    if (v >= 0 && v < n_vert) atomicMin(first + v, (int)s);
}

__global__ __launch_bounds__(256) void vfn_tsdf_gather_colours_kernel(const double* __restrict__ tri_cols, long long n_slots,
                                                                      const int* __restrict__ first, long long n_vert, double* __restrict__ colours) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vert) return;
    const long long s = first[v];
    const bool ok = s >= 0 && s < n_slots;                    // (a vertex no slot names: cannot come from vfn_mesh_number; zeros, not a fault)
#pragma unroll
    for (int c = 0; c < 3; ++c) colours[v * 3 + c] = ok ? tri_cols[s * 3 + c] : 0.0;
}

int check_dims(int32_t nx, int32_t ny, int32_t nz, float vl, const char* what) {
    VFN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny < (1ll << 31) && (long long)nx * ny * nz < (1ll << 31),
                "%s: dims (%d, %d, %d) must be positive with fewer than 2^31 voxels", what, nx, ny, nz);
    VFN_REQUIRE(vl > 0.f && vl - vl == 0.f, "%s: voxel_length must be positive and finite", what);
    return VFN_OK;
}

int make_lattice(Lattice& a, const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float vl,
                 const char* what) {
    const int rc = check_dims(nx, ny, nz, vl, what);
    if (rc != VFN_OK) return rc;
    VFN_REQUIRE(tsdf && weight, "%s: NULL volume", what);
    a = Lattice{tsdf, weight, nx, ny, nz, (long long)(nx - 1) * (ny - 1) * (nz - 1), ox, oy, oz, vl};
    return VFN_OK;
}

// what every entry point that takes views checks before it looks at a pointer
int check_views(const char* what, float sdf_trunc, int32_t n_views, int32_t height, int32_t width) {
    VFN_REQUIRE(sdf_trunc > 0.f && sdf_trunc - sdf_trunc == 0.f, "%s: sdf_trunc must be positive and finite", what);
    VFN_REQUIRE(n_views >= 0 && height >= 1 && width >= 1 && (long long)height * width < (1ll << 31),
                "%s: bad views (%d of %d x %d)", what, n_views, height, width);
    return VFN_OK;
}

// `colour` / `rgb` are read only by the COLOUR instantiation
template <bool COLOUR>
Colour<COLOUR> make_colour(float* colour, const unsigned char* rgb) {
    Colour<COLOUR> cl;
    if constexpr (COLOUR) {
        cl.colour = colour;
        cl.rgb = rgb;
    }
    return cl;
}

// the checks and the launch of both dense integrating entry points
template <bool COLOUR>
int integrate(const char* what, float* tsdf, float* weight, float* colour, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
              float voxel_length, float sdf_trunc, const float* depth, const unsigned char* rgb, int32_t height, int32_t width,
              const float* intrinsics, const float* extrinsics, int32_t n_views, void* stream) {
    int rc = check_dims(nx, ny, nz, voxel_length, what);
    if (rc != VFN_OK) return rc;
    VFN_REQUIRE(tsdf && weight && (!COLOUR || colour), "%s: NULL volume", what);
    rc = check_views(what, sdf_trunc, n_views, height, width);
    if (rc != VFN_OK) return rc;
    if (n_views == 0) return VFN_OK;
    VFN_REQUIRE(depth && intrinsics && extrinsics && (!COLOUR || rgb), "%s: NULL view argument", what);
    const long long nbi = (nx + BI - 1) / BI, nbj = (ny + BJ - 1) / BJ, nbk = (nz + BK - 1) / BK;
    const long long bricks = nbi * nbj * nbk;
    VFN_REQUIRE(bricks < (1ll << 31), "%s: %lld bricks exceed one launch", what, bricks);
    Volume vol{tsdf, weight, nx, ny, nz, ox, oy, oz, voxel_length, sdf_trunc};
    Views vs{depth, intrinsics, extrinsics, n_views, height, width};
    const Colour<COLOUR> cl = make_colour<COLOUR>(colour, rgb);
    // 16-B accesses need rows of a multiple of four voxels and 16-B aligned arrays (a lane's 12 colour floats then start on a multiple
    // of 48 B); anything else takes the scalar form.  (`colour` is NULL without COLOUR.)
    const bool vec = nz % RUN == 0 && ((uintptr_t)tsdf & 15) == 0 && ((uintptr_t)weight & 15) == 0 && ((uintptr_t)colour & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((vfn_tsdf_integrate_kernel<true, COLOUR>), dim3((unsigned)bricks), dim3(THREADS), 0, s, vol, vs, (int)nbj, (int)nbk, cl);
    else hipLaunchKernelGGL((vfn_tsdf_integrate_kernel<false, COLOUR>), dim3((unsigned)bricks), dim3(THREADS), 0, s, vol, vs, (int)nbj, (int)nbk, cl);
    return vfn_check_launch(what);
}

}  // namespace

extern "C" int vfn_tsdf_integrate(float* tsdf, float* weight, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
                                  float voxel_length, float sdf_trunc, const float* depth, int32_t height, int32_t width,
                                  const float* intrinsics, const float* extrinsics, int32_t n_views, void* stream) {
    return integrate<false>("vfn_tsdf_integrate", tsdf, weight, nullptr, nx, ny, nz, ox, oy, oz, voxel_length, sdf_trunc, depth, nullptr, height,
                            width, intrinsics, extrinsics, n_views, stream);
}

extern "C" int vfn_tsdf_integrate_rgb(float* tsdf, float* weight, float* colour, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
                                      float voxel_length, float sdf_trunc, const float* depth, const uint8_t* rgb, int32_t height, int32_t width,
                                      const float* intrinsics, const float* extrinsics, int32_t n_views, void* stream) {
    return integrate<true>("vfn_tsdf_integrate_rgb", tsdf, weight, colour, nx, ny, nz, ox, oy, oz, voxel_length, sdf_trunc, depth, rgb, height,
                           width, intrinsics, extrinsics, n_views, stream);
}

extern "C" int vfn_tsdf_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, int32_t* counts, int32_t* offsets,
                              int64_t* info, void* scan_ws, int64_t scan_ws_bytes, void* stream) {
    Lattice a;
    const int rc = make_lattice(a, tsdf, weight, nx, ny, nz, 0.f, 0.f, 0.f, 1.f, "vfn_tsdf_count");
    if (rc != VFN_OK) return rc;
    return vfn_mc_count(a, counts, offsets, info, scan_ws, scan_ws_bytes, (hipStream_t)stream, "vfn_tsdf_count");
}

extern "C" int vfn_tsdf_emit(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz,
                             float voxel_length, const int32_t* counts, const int32_t* offsets, double* tri_verts, void* stream) {
    Lattice a;
    const int rc = make_lattice(a, tsdf, weight, nx, ny, nz, ox, oy, oz, voxel_length, "vfn_tsdf_emit");
    if (rc != VFN_OK) return rc;
    return vfn_mc_emit(a, counts, offsets, tri_verts, (hipStream_t)stream, "vfn_tsdf_emit");
}

extern "C" int vfn_tsdf_emit_colours(const float* tsdf, const float* weight, const float* colour, int32_t nx, int32_t ny, int32_t nz,
                                     const int32_t* counts, const int32_t* offsets, double* tri_cols, void* stream) {
    LatticeColours a;
    const int rc = make_lattice(a.at, tsdf, weight, nx, ny, nz, 0.f, 0.f, 0.f, 1.f, "vfn_tsdf_emit_colours");
    if (rc != VFN_OK) return rc;
    VFN_REQUIRE(colour, "vfn_tsdf_emit_colours: NULL colour volume");
    a.colour = colour;
    return vfn_mc_emit(a, counts, offsets, tri_cols, (hipStream_t)stream, "vfn_tsdf_emit_colours");
}

extern "C" int vfn_tsdf_vertex_colours(const int64_t* ids, int64_t n_slots, const double* tri_cols, int32_t* first, int64_t n_vertices,
                                       double* colours, void* stream) {
    VFN_REQUIRE(n_slots >= 0 && n_slots < (1ll << 31) && n_vertices >= 0 && n_vertices <= n_slots,
                "vfn_tsdf_vertex_colours: %lld vertices of %lld slots are outside the limits", (long long)n_vertices, (long long)n_slots);
    if (n_vertices == 0) return VFN_OK;
    VFN_REQUIRE(ids && tri_cols && first && colours, "vfn_tsdf_vertex_colours: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(first, 0x7f, (size_t)n_vertices * sizeof(int32_t), s);      // 0x7f7f7f7f: above every slot
    if (e != hipSuccess) {
        vfn_set_error("vfn_tsdf_vertex_colours: memset failed: %s", hipGetErrorString(e));
        return VFN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(vfn_tsdf_first_slot_kernel, dim3(blocks_for(n_slots)), dim3(256), 0, s, (const long long*)ids, (long long)n_slots,
                       (int*)first, (long long)n_vertices);
    hipLaunchKernelGGL(vfn_tsdf_gather_colours_kernel, dim3(blocks_for(n_vertices)), dim3(256), 0, s, tri_cols, (long long)n_slots,
                       (const int*)first, (long long)n_vertices, colours);
    return vfn_check_launch("vfn_tsdf_vertex_colours");
}

// ---- the block-sparse volume (include/vfn.h: "A block-sparse TSDF volume") ------------------------------------------------
// Blocks of BLOCK^3 voxels of the SAME lattice, opened near the back-projected depth points and stored one after another:
//   mark       one lane per pixel of every view, float64: the blocks its point's ball touches get a byte 1 (a plain store of a constant;
//              lanes that race store the same value).  Numbering the new blocks is torch plumbing on the marks.
//   integrate  one workgroup of 128 lanes per block, a lane owns RUN consecutive k voxels (always 16-B aligned inside a block: only the
//              vector form).  x, y, z come from the GLOBAL index through centre(); the kernel derives the indices, the offset and the
//              block's extreme in-lattice centres, everything else is the dense kernel's own code — load_vec, apply_views<128>, store_vec
//              — so a voxel holds the dense volume's bits.  Voxels of an edge block beyond dims are never updated.
//   count/emit a third source of vfn_mc_extract.h: position p is block p >> 9, local cell (p >> 6) & 7, (p >> 3) & 7, p & 7; corners
//              come from this block or from the neighbour block_of names; an absent neighbour voids the cell.  vertex() is Lattice's with
//              the global index: the dense mesh's position bits.
namespace {

constexpr int BLOCK = 8, BLOCK_VOXELS = BLOCK * BLOCK * BLOCK;
constexpr int SP_THREADS = BLOCK_VOXELS / RUN;            // 128 lanes: two waves
static_assert(SP_THREADS == 128 && BLOCK % RUN == 0, "a lane's run stays inside one row of a block");

struct MarkArgs {
    const float* depth;        // [V, H, W]
    const double* cam;         // [V, 17]: C[12] (camera -> world rows), fx fy cx cy, q
    unsigned char* marks;      // [nbx, nby, nbz]
    int n, h, w;
    int nb[3];
    double o[3], vl, tr;
};

__global__ __launch_bounds__(256) void vfn_tsdf_sparse_mark_kernel(MarkArgs a) {
    const long long pixels = (long long)a.h * a.w;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels * a.n) return;
    const int view = (int)(p / pixels);
    const long long pix = p - (long long)view * pixels;
    const int v = (int)(pix / a.w), u = (int)(pix - (long long)v * a.w);
    const double d = (double)a.depth[p];
    if (!(d > 0.0)) return;
    const double* __restrict__ c = a.cam + (long long)view * 17;
    const double fx = c[12], fy = c[13], cx = c[14], cy = c[15], q = c[16];
    const double ca = ((double)u - cx) / fx, cb = ((double)v - cy) / fy;
    const double ad = ca * d, bd = cb * d;
    const double r = (a.tr + (0.5 * (d + a.tr)) * q) + 2.0 * a.vl;
    const double edge = 8.0 * a.vl;
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double P = ((c[4 * k] * ad + c[4 * k + 1] * bd) + c[4 * k + 2] * d) + c[4 * k + 3];
        double l = floor(((P - r) - a.o[k]) / edge), h = floor(((P + r) - a.o[k]) / edge);
        const double last = (double)(a.nb[k] - 1);
        if (!(h >= 0.0) || !(l <= last)) return;              // outside the block lattice, or NaN
        l = l < 0.0 ? 0.0 : l;
        h = h > last ? last : h;
        lo[k] = (int)l;
        hi[k] = (int)h;
    }
    for (int bi = lo[0]; bi <= hi[0]; ++bi)
        for (int bj = lo[1]; bj <= hi[1]; ++bj) {
            unsigned char* __restrict__ row = a.marks + ((long long)bi * a.nb[1] + bj) * a.nb[2];
            for (int bk = lo[2]; bk <= hi[2]; ++bk)
                if (row[bk] == 0) row[bk] = 1;
        }
}

struct SparseVolume {
    float* tsdf;               // [n_blocks, 8, 8, 8]
    float* weight;
    const int* coords;         // [n_blocks, 3]
    int nx, ny, nz;
    float ox, oy, oz, vl, trunc;
};

template <bool COLOUR>
__global__ __launch_bounds__(SP_THREADS) void vfn_tsdf_sparse_integrate_kernel(SparseVolume vol, Views vs, Colour<COLOUR> cl) {
    __shared__ unsigned long long seen[SP_THREADS / 64];
    const long long blk = blockIdx.x;
    const int t = threadIdx.x;
    const int b0 = vol.coords[blk * 3] * BLOCK, b1 = vol.coords[blk * 3 + 1] * BLOCK, b2 = vol.coords[blk * 3 + 2] * BLOCK;
    const int i = b0 + (t >> 4), j = b1 + ((t >> 1) & 7), k0 = b2 + (t & 1) * RUN;
    const int cnt = (i < vol.nx && j < vol.ny) ? max(0, min(RUN, vol.nz - k0)) : 0;      // voxels beyond dims are never updated
    const long long off = blk * BLOCK_VOXELS + (long long)t * RUN;

    float ts[RUN], wt[RUN], z[RUN];
    float col[COLOUR ? RUN : 1][3] = {};
    load_vec<COLOUR>(ts, wt, col, vol.tsdf, vol.weight, cl, off);
    const float x = centre(vol.ox, i, vol.vl), y = centre(vol.oy, j, vol.vl);
#pragma unroll
    for (int r = 0; r < RUN; ++r) z[r] = centre(vol.oz, k0 + r, vol.vl);

    // the block's extreme in-lattice voxel centres (a block of the block lattice holds at least one voxel of the lattice)
    const float lo[3] = {centre(vol.ox, b0, vol.vl), centre(vol.oy, b1, vol.vl), centre(vol.oz, b2, vol.vl)};
    const float hi[3] = {centre(vol.ox, min(b0 + BLOCK, vol.nx) - 1, vol.vl), centre(vol.oy, min(b1 + BLOCK, vol.ny) - 1, vol.vl),
                         centre(vol.oz, min(b2 + BLOCK, vol.nz) - 1, vol.vl)};
    apply_views<SP_THREADS>(vs, cl, lo, hi, x, y, z, cnt, vol.trunc, ts, wt, col, seen);

    store_vec<COLOUR>(ts, wt, col, vol.tsdf, vol.weight, cl, off);
}

// the sparse source of vfn_mc_extract.h; c[] is the GLOBAL cell index, so Lattice::vertex gives the dense mesh's bits
struct SparseLattice {
    using Value = float;
    using Emit = Lattice::Emit;
    Lattice at;               // origin / voxel length / dims of the lattice (its tsdf / weight are the block storage)
    const int* block_of;      // [nbx, nby, nbz], -1 for absent
    const int* coords;        // [n_blocks, 3]
    int nby, nbz;
    long long n_positions;    // n_blocks * 512

    __host__ __device__ long long positions() const { return n_positions; }

    // the storage index of lattice voxel g (inside dims), -1 when its block is absent; `home` / b: the block the cell belongs to
    __device__ __forceinline__ long long voxel(const int g[3], const int home[3], long long b) const {
        const int bb[3] = {g[0] >> 3, g[1] >> 3, g[2] >> 3};
        long long id = b;
        if (bb[0] != home[0] || bb[1] != home[1] || bb[2] != home[2]) id = block_of[((long long)bb[0] * nby + bb[1]) * nbz + bb[2]];
        if (id < 0) return -1;
        return id * BLOCK_VOXELS + (((g[0] & 7) * BLOCK + (g[1] & 7)) * BLOCK + (g[2] & 7));
    }

    __device__ __forceinline__ bool eval(long long p, int c[3], float v[8], int& top, unsigned&) const {
        const long long b = p >> 9;
        const int home[3] = {coords[b * 3], coords[b * 3 + 1], coords[b * 3 + 2]};
        c[0] = home[0] * BLOCK + (int)((p >> 6) & 7);
        c[1] = home[1] * BLOCK + (int)((p >> 3) & 7);
        c[2] = home[2] * BLOCK + (int)(p & 7);
        if (c[0] + 1 >= at.nx || c[1] + 1 >= at.ny || c[2] + 1 >= at.nz) return false;
        int t = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int g[3] = {c[0] + INC[q][0], c[1] + INC[q][1], c[2] + INC[q][2]};
            const long long idx = voxel(g, home, b);
            if (idx < 0 || at.weight[idx] == 0.f) return false;   // an absent block voids the cell like an unobserved corner
            v[q] = at.tsdf[idx];
            t |= (v[q] < 0.f ? 1 : 0) << q;
        }
        top = t;
        return t != 0 && t != 255;
    }

    __device__ __forceinline__ void emit_setup(const int[3], Emit&) const {}
    __device__ __forceinline__ void vertex(const int c[3], const float v[8], const Emit& em, int e, double out[3]) const { at.vertex(c, v, em, e, out); }
};

struct SparseLatticeColours {
    using Value = float;
    using Emit = Lattice::Emit;
    SparseLattice sp;
    const float* colour;      // [n_blocks, 8, 8, 8, 3]

    __host__ __device__ long long positions() const { return sp.positions(); }
    __device__ __forceinline__ bool eval(long long p, int c[3], float v[8], int& top, unsigned& status) const { return sp.eval(p, c, v, top, status); }
    __device__ __forceinline__ void emit_setup(const int[3], Emit&) const {}

    __device__ __forceinline__ void vertex(const int c[3], const float v[8], const Emit&, int e, double out[3]) const {
        int ql, qu, axis;
        edge_ends(e, ql, qu, axis);
        const int home[3] = {c[0] >> 3, c[1] >> 3, c[2] >> 3};
        const long long b = sp.block_of[((long long)home[0] * sp.nby + home[1]) * sp.nbz + home[2]];
        const int gl[3] = {c[0] + INC[ql][0], c[1] + INC[ql][1], c[2] + INC[ql][2]};
        const int gu[3] = {c[0] + INC[qu][0], c[1] + INC[qu][1], c[2] + INC[qu][2]};
        colour_at(v, ql, qu, sp.voxel(gl, home, b), sp.voxel(gu, home, b), colour, out);      // (both present: eval passed)
    }
};

int check_sparse_dims(int32_t nx, int32_t ny, int32_t nz, int32_t n_blocks, float vl, const char* what) {
    VFN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= (1 << 24) && ny <= (1 << 24) && nz <= (1 << 24),
                "%s: dims (%d, %d, %d) must lie in [1, 2^24]", what, nx, ny, nz);
    const long long nbx = (nx + BLOCK - 1) / BLOCK, nby = (ny + BLOCK - 1) / BLOCK, nbz = (nz + BLOCK - 1) / BLOCK;
    VFN_REQUIRE(nbx * nby < (1ll << 31) && nbx * nby * nbz < (1ll << 31), "%s: the block lattice of dims (%d, %d, %d) exceeds 2^31 blocks", what,
                nx, ny, nz);
    VFN_REQUIRE(n_blocks >= 0 && (long long)n_blocks * BLOCK_VOXELS < (1ll << 31) && n_blocks <= nbx * nby * nbz,
                "%s: %d blocks are outside the limits", what, n_blocks);
    VFN_REQUIRE(vl > 0.f && vl - vl == 0.f, "%s: voxel_length must be positive and finite", what);
    return VFN_OK;
}

int make_sparse_lattice(SparseLattice& a, const float* tsdf, const float* weight, const int32_t* block_of, const int32_t* coords, int32_t n_blocks,
                        int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float vl, const char* what) {
    const int rc = check_sparse_dims(nx, ny, nz, n_blocks, vl, what);
    if (rc != VFN_OK) return rc;
    VFN_REQUIRE(n_blocks == 0 || (tsdf && weight && block_of && coords), "%s: NULL volume", what);
    a.at = Lattice{tsdf, weight, nx, ny, nz, 0ll, ox, oy, oz, vl};
    a.block_of = (const int*)block_of;
    a.coords = (const int*)coords;
    a.nby = (ny + BLOCK - 1) / BLOCK;
    a.nbz = (nz + BLOCK - 1) / BLOCK;
    a.n_positions = (long long)n_blocks * BLOCK_VOXELS;
    return VFN_OK;
}

template <bool COLOUR>
int sparse_integrate(const char* what, float* tsdf, float* weight, float* colour, const int32_t* coords, int32_t n_blocks, int32_t nx, int32_t ny,
                     int32_t nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc, const float* depth, const unsigned char* rgb,
                     int32_t height, int32_t width, const float* intrinsics, const float* extrinsics, int32_t n_views, void* stream) {
    int rc = check_sparse_dims(nx, ny, nz, n_blocks, voxel_length, what);
    if (rc != VFN_OK) return rc;
    rc = check_views(what, sdf_trunc, n_views, height, width);
    if (rc != VFN_OK) return rc;
    if (n_views == 0 || n_blocks == 0) return VFN_OK;
    VFN_REQUIRE(tsdf && weight && coords && (!COLOUR || colour), "%s: NULL volume", what);
    VFN_REQUIRE(depth && intrinsics && extrinsics && (!COLOUR || rgb), "%s: NULL view argument", what);
    VFN_REQUIRE(((uintptr_t)tsdf & 15) == 0 && ((uintptr_t)weight & 15) == 0 && ((uintptr_t)colour & 15) == 0, "%s: the block storage must be 16-B aligned",
                what);
    SparseVolume vol{tsdf, weight, (const int*)coords, nx, ny, nz, ox, oy, oz, voxel_length, sdf_trunc};
    Views vs{depth, intrinsics, extrinsics, n_views, height, width};
    hipLaunchKernelGGL((vfn_tsdf_sparse_integrate_kernel<COLOUR>), dim3((unsigned)n_blocks), dim3(SP_THREADS), 0, (hipStream_t)stream, vol, vs,
                       make_colour<COLOUR>(colour, rgb));
    return vfn_check_launch(what);
}

}  // namespace

extern "C" int vfn_tsdf_sparse_mark(uint8_t* marks, int32_t nbx, int32_t nby, int32_t nbz, float ox, float oy, float oz, float voxel_length,
                                    float sdf_trunc, const float* depth, int32_t height, int32_t width, const double* cameras, int32_t n_views,
                                    void* stream) {
    const char* what = "vfn_tsdf_sparse_mark";
    VFN_REQUIRE(nbx >= 1 && nby >= 1 && nbz >= 1 && (long long)nbx * nby < (1ll << 31) && (long long)nbx * nby * nbz < (1ll << 31),
                "%s: the block lattice (%d, %d, %d) must be positive with fewer than 2^31 blocks", what, nbx, nby, nbz);
    VFN_REQUIRE(voxel_length > 0.f && voxel_length - voxel_length == 0.f && sdf_trunc > 0.f && sdf_trunc - sdf_trunc == 0.f,
                "%s: voxel_length and sdf_trunc must be positive and finite", what);
    const int rc = check_views(what, sdf_trunc, n_views, height, width);      // (sdf_trunc has passed: this is the view part)
    if (rc != VFN_OK) return rc;
    if (n_views == 0) return VFN_OK;
    VFN_REQUIRE(marks && depth && cameras, "%s: NULL argument", what);
    const long long lanes = (long long)height * width * n_views;
    VFN_REQUIRE((lanes + 255) / 256 < (1ll << 31), "%s: %lld pixels exceed one launch", what, lanes);
    MarkArgs a{depth, cameras, marks, n_views, height, width, {nbx, nby, nbz}, {(double)ox, (double)oy, (double)oz}, (double)voxel_length,
               (double)sdf_trunc};
    hipLaunchKernelGGL(vfn_tsdf_sparse_mark_kernel, dim3(blocks_for(lanes)), dim3(256), 0, (hipStream_t)stream, a);
    return vfn_check_launch(what);
}

extern "C" int vfn_tsdf_sparse_integrate(float* tsdf, float* weight, const int32_t* block_coords, int32_t n_blocks, int32_t nx, int32_t ny,
                                         int32_t nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc, const float* depth,
                                         int32_t height, int32_t width, const float* intrinsics, const float* extrinsics, int32_t n_views,
                                         void* stream) {
    return sparse_integrate<false>("vfn_tsdf_sparse_integrate", tsdf, weight, nullptr, block_coords, n_blocks, nx, ny, nz, ox, oy, oz, voxel_length,
                                   sdf_trunc, depth, nullptr, height, width, intrinsics, extrinsics, n_views, stream);
}

extern "C" int vfn_tsdf_sparse_integrate_rgb(float* tsdf, float* weight, float* colour, const int32_t* block_coords, int32_t n_blocks, int32_t nx,
                                             int32_t ny, int32_t nz, float ox, float oy, float oz, float voxel_length, float sdf_trunc,
                                             const float* depth, const uint8_t* rgb, int32_t height, int32_t width, const float* intrinsics,
                                             const float* extrinsics, int32_t n_views, void* stream) {
    return sparse_integrate<true>("vfn_tsdf_sparse_integrate_rgb", tsdf, weight, colour, block_coords, n_blocks, nx, ny, nz, ox, oy, oz,
                                  voxel_length, sdf_trunc, depth, rgb, height, width, intrinsics, extrinsics, n_views, stream);
}

extern "C" int vfn_tsdf_sparse_count(const float* tsdf, const float* weight, const int32_t* block_of, const int32_t* block_coords, int32_t n_blocks,
                                     int32_t nx, int32_t ny, int32_t nz, int32_t* counts, int32_t* offsets, int64_t* info, void* scan_ws,
                                     int64_t scan_ws_bytes, void* stream) {
    SparseLattice a;
    const int rc = make_sparse_lattice(a, tsdf, weight, block_of, block_coords, n_blocks, nx, ny, nz, 0.f, 0.f, 0.f, 1.f, "vfn_tsdf_sparse_count");
    if (rc != VFN_OK) return rc;
    return vfn_mc_count(a, counts, offsets, info, scan_ws, scan_ws_bytes, (hipStream_t)stream, "vfn_tsdf_sparse_count");
}

extern "C" int vfn_tsdf_sparse_emit(const float* tsdf, const float* weight, const int32_t* block_of, const int32_t* block_coords, int32_t n_blocks,
                                    int32_t nx, int32_t ny, int32_t nz, float ox, float oy, float oz, float voxel_length, const int32_t* counts,
                                    const int32_t* offsets, double* tri_verts, void* stream) {
    SparseLattice a;
    const int rc = make_sparse_lattice(a, tsdf, weight, block_of, block_coords, n_blocks, nx, ny, nz, ox, oy, oz, voxel_length, "vfn_tsdf_sparse_emit");
    if (rc != VFN_OK) return rc;
    return vfn_mc_emit(a, counts, offsets, tri_verts, (hipStream_t)stream, "vfn_tsdf_sparse_emit");
}

extern "C" int vfn_tsdf_sparse_emit_colours(const float* tsdf, const float* weight, const float* colour, const int32_t* block_of,
                                            const int32_t* block_coords, int32_t n_blocks, int32_t nx, int32_t ny, int32_t nz,
                                            const int32_t* counts, const int32_t* offsets, double* tri_cols, void* stream) {
    SparseLatticeColours a;
    const int rc = make_sparse_lattice(a.sp, tsdf, weight, block_of, block_coords, n_blocks, nx, ny, nz, 0.f, 0.f, 0.f, 1.f,
                                       "vfn_tsdf_sparse_emit_colours");
    if (rc != VFN_OK) return rc;
    VFN_REQUIRE(n_blocks == 0 || colour, "vfn_tsdf_sparse_emit_colours: NULL colour volume");
    a.colour = colour;
    return vfn_mc_emit(a, counts, offsets, tri_cols, (hipStream_t)stream, "vfn_tsdf_sparse_emit_colours");
}
