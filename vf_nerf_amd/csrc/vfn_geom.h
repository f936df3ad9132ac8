// vfn_geom.h — what the fp64 mesh units (vfn_normals, vfn_voxel, vfn_cc, vfn_orient, vfn_simplify, vfn_collapse) and, through
// csrc/vfn_mc_extract.h, the lattice units (vfn_mesh, vfn_tsdf) share: the status bits of include/vfn.h, the launch size and a wave's
// status report — those for every unit —, the forest's memory accesses, and the unit vector of a cross product with a plane's offset.
// The status bits also compile for the host (csrc/vfn_forest_core.h, csrc/vfn_collapse_core.h); the rest is device code, for units built
// with -ffp-contract=off (build.sh).
#pragma once
#include <math.h>

namespace vfn_geom {

// a non-finite input; an index, node, parent or segment outside its range (either name, as include/vfn.h words it); a finite input
// whose cross product or length is not
constexpr unsigned ST_NONFINITE = 1u, ST_INDEX = 2u, ST_RANGE = ST_INDEX, ST_OVERFLOW = 4u;

}  // namespace vfn_geom

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace vfn_geom {

inline unsigned blocks_for(long long n, int block = 256) { return (unsigned)((n + block - 1) / block); }

// The status bits of a wave are ORed into info[0] with at most one atomic, and none from a wave that saw no bad input.
// every lane of the wave arrives here (no early return in the kernels)
__device__ __forceinline__ void report(unsigned status, unsigned long long* __restrict__ info) {
    const unsigned long long any = __ballot(status != 0u);
    if (any) {
        unsigned all = status;
        for (int o = 32; o > 0; o >>= 1) all |= (unsigned)__shfl_xor((int)all, o, 64);
        if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(any)) atomicOr(info, (unsigned long long)all);
    }
}

// The `Mem` of csrc/vfn_forest_core.h on the device.  A forest is re-read only through this load: never through a plain load that the
// compiler may keep in a register across a loop.  The orders are relaxed because the forest words are the only data: nothing else is
// published through them.
struct DeviceMem {
    using word = int;
    static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    // -> the value found: `expected` exactly when the swap happened
    static __device__ __forceinline__ int cas(int* p, int expected, int desired) {
        __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
};

// c / |c| of include/vfn.h: *r = sqrt((c0 c0 + c1 c1) + c2 c2).  Where r > 0 and finite, out = c / r and true; otherwise out is left
// as it was, false, and ST_OVERFLOW where r is not finite.
__device__ __forceinline__ bool unit_vector(const double c[3], double out[3], double* r, unsigned& status) {
    double s = c[0] * c[0];
    s = s + c[1] * c[1];
    s = s + c[2] * c[2];
    *r = sqrt(s);
    const bool ok = *r > 0.0 && isfinite(*r);
    if (ok) {
        out[0] = c[0] / *r; out[1] = c[1] / *r; out[2] = c[2] / *r;
    } else if (!isfinite(*r)) {
        status |= ST_OVERFLOW;
    }
    return ok;
}

// e = n . (p - origin) of a plane row: the offset from the frame's origin of the plane through p with unit normal n
__device__ __forceinline__ double plane_offset(const double n[3], const double p[3], double ox, double oy, double oz) {
    double e = n[0] * (p[0] - ox);
    e = e + n[1] * (p[1] - oy);
    e = e + n[2] * (p[2] - oz);
    return e;
}

}  // namespace vfn_geom
#endif
