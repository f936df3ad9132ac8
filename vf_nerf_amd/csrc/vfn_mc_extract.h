// vfn_mc_extract.h — the extraction skeleton shared by the translation units that triangulate a lattice (csrc/vfn_mesh.hip: contrastive
// marching cubes; csrc/vfn_tsdf.hip: the zero level set of a TSDF volume): the case tables in constant memory, the ordered device scan,
// and count -> scan -> total -> emit over the cell positions of a SOURCE.  A source is a POD passed to the kernels by value:
//   Value, Emit                        the type of a corner value; what an emitting lane keeps besides the cell (a POD, may be empty)
//   positions()                        the number of cell positions (host and device)
//   eval(p, c, v, top, status)         position p into the cell: lattice index c[3], corner values v[8], the case; false for a position
//                                      that yields nothing.  Bad input sets bits of status
//   emit_setup(c, em)                  once per emitting lane, after eval
//   vertex(c, v, em, e, out)           the float64 vertex of cut edge e
// The cell is handed over as separate arrays, not as one record: v (and the mesh source's corner positions) are indexed by a run-time
// corner number, and the compiler does not split a local record that is indexed so — the whole record then lives in scratch or LDS.
// Everything here has internal linkage: each including unit gets its own tables and its own instantiations.
#pragma once
#include "vfn_common.h"
#include "vfn_geom.h"         // the launch size, a wave's status report
#include "vfn_mc_tables.h"
#include <hipcub/hipcub.hpp>

namespace {

// (entries after a row's -1 are never read)
__device__ __constant__ signed char TRI[256][16] = {VFN_MC_TRI_ROWS};
__device__ __constant__ int EDGE_A[12] = VFN_MC_EDGE_A;
__device__ __constant__ int EDGE_B[12] = VFN_MC_EDGE_B;
__device__ __constant__ int INC[8][3] = VFN_MC_INC;

__device__ __forceinline__ int tri_count(int top) {
    int n = 0;
    while (n < 5 && TRI[top][3 * n] >= 0) ++n;
    return n;
}

using vfn_geom::blocks_for;

// The ordered inclusive scan over n int32 values (rocPRIM through hipCUB) that gives every triangle / vertex its output slot.
inline int vfn_mc_scan_bytes(long long n, size_t* bytes) {
    *bytes = 0;
    const hipError_t e = hipcub::DeviceScan::InclusiveSum(nullptr, *bytes, (const int*)nullptr, (int*)nullptr, (int)n);
    return e == hipSuccess ? VFN_OK : VFN_ERR_LAUNCH;
}

inline int vfn_mc_inclusive_scan(const int* in, int* out, long long n, void* ws, long long ws_bytes, hipStream_t s, const char* what) {
    size_t need = 0;
    VFN_REQUIRE(vfn_mc_scan_bytes(n, &need) == VFN_OK, "%s: scan size query failed", what);
    VFN_REQUIRE(ws && (long long)need <= ws_bytes, "%s: scan workspace of %lld bytes < %lld needed", what, ws_bytes, (long long)need);
    const hipError_t e = hipcub::DeviceScan::InclusiveSum(ws, need, in, out, (int)n, s);
    if (e != hipSuccess) {
        vfn_set_error("%s: scan failed: %s", what, hipGetErrorString(e));
        return VFN_ERR_LAUNCH;
    }
    return VFN_OK;
}

// info[slot] = the last inclusive count (0 for an empty scan)
__global__ void vfn_mc_total_kernel(const int* __restrict__ incl, long long last, long long* __restrict__ info, int slot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) info[slot] = last >= 0 ? (long long)incl[last] : 0ll;
}

// one lane per cell POSITION: its triangle count; the status bits of a wave are ORed into info[1] (a source that never sets one
// leaves info[1] untouched)
template <class Source>
__global__ __launch_bounds__(256) void vfn_mc_count_kernel(Source a, int* __restrict__ counts, long long* __restrict__ info) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned status = 0;
    if (p < a.positions()) {
        int c[3], top = 0;
        typename Source::Value v[8];
        counts[p] = a.eval(p, c, v, top, status) ? tri_count(top) : 0;
    }
    vfn_geom::report(status, (unsigned long long*)&info[1]);
}

// the same lanes again: every triangle's three float64 vertices at their slots (slot = 3 x triangle + corner)
template <class Source>
__global__ __launch_bounds__(256) void vfn_mc_emit_kernel(Source a, const int* __restrict__ counts, const int* __restrict__ incl,
                                                          double* __restrict__ tri_verts) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.positions()) return;
    const int n = counts[p];
    if (n == 0) return;
    int c[3], top = 0;
    typename Source::Value v[8];
    unsigned status = 0;
    if (!a.eval(p, c, v, top, status)) return;
    typename Source::Emit em;
    a.emit_setup(c, em);
    const long long slot0 = (long long)(incl[p] - n) * 3;
    for (int t = 0; t < n; ++t)
        for (int k = 0; k < 3; ++k) {
            double x[3];
            a.vertex(c, v, em, TRI[top][3 * t + k], x);
            double* o = tri_verts + (slot0 + 3 * t + k) * 3;
            o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
        }
}

// count -> ordered scan -> total: counts[p], offsets[p] (inclusive) and info[0] = the number of triangles
template <class Source>
int vfn_mc_count(const Source& a, int32_t* counts, int32_t* offsets, int64_t* info, void* scan_ws, int64_t scan_ws_bytes, hipStream_t s,
                 const char* what) {
    const long long m = a.positions();
    VFN_REQUIRE(info && (m == 0 || (counts && offsets)), "%s: NULL output", what);
    if (m > 0) {
        hipLaunchKernelGGL(vfn_mc_count_kernel<Source>, dim3(blocks_for(m)), dim3(256), 0, s, a, (int*)counts, (long long*)info);
        const int rc = vfn_mc_inclusive_scan(counts, offsets, m, scan_ws, scan_ws_bytes, s, what);
        if (rc != VFN_OK) return rc;
    }
    hipLaunchKernelGGL(vfn_mc_total_kernel, dim3(1), dim3(64), 0, s, (const int*)offsets, m - 1, (long long*)info, 0);
    return vfn_check_launch(what);
}

template <class Source>
int vfn_mc_emit(const Source& a, const int32_t* counts, const int32_t* offsets, double* tri_verts, hipStream_t s, const char* what) {
    if (a.positions() == 0) return VFN_OK;
    VFN_REQUIRE(counts && offsets && tri_verts, "%s: NULL argument", what);
    hipLaunchKernelGGL(vfn_mc_emit_kernel<Source>, dim3(blocks_for(a.positions())), dim3(256), 0, s, a, (const int*)counts, (const int*)offsets,
                       tri_verts);
    return vfn_check_launch(what);
}

}  // namespace
