// vfn_quadric.h — what vfn_cluster_quadrics (csrc/vfn_simplify.hip) and vfn_edge_collapse_candidates (csrc/vfn_collapse_core.h) do with
// the ten sums of a quadric, as ONE text that compiles for the device and for the host: the 3 x 3 solve by the adjugate and the
// quadric's value at a point.  fp64, built without contraction on both sides (-ffp-contract=off): the expressions of include/vfn.h,
// operation for operation.  How the ten sums are made (about the cell centre, about the origin) and when a minimiser is accepted
// (inside its cell, within reach of its edge) differ between the two users and stay with them.
#pragma once

#if defined(__HIPCC__)
#define VFN_QUADRIC_FN __host__ __device__ __forceinline__
#else
#define VFN_QUADRIC_FN inline
#endif

namespace vfn_quadric {

constexpr int CHANNELS = 10;             // a00 a01 a02 a11 a12 a22, b0 b1 b2, c: the value at z is z'Az + 2 b'z + c

struct Minimiser {
    double det;        // of A, by the first row of its adjugate
    double x[3];       // -adj(A) b / det: NaN or infinite where det is 0
    double t;          // the mean of A's diagonal: det is judged against rcond * t^3
};

VFN_QUADRIC_FN Minimiser minimiser(const double* s) {
    const double a00 = s[0], a01 = s[1], a02 = s[2], a11 = s[3], a12 = s[4], a22 = s[5], b0 = s[6], b1 = s[7], b2 = s[8];
    const double m00 = a11 * a22 - a12 * a12, m01 = a02 * a12 - a01 * a22, m02 = a01 * a12 - a02 * a11;
    const double m11 = a00 * a22 - a02 * a02, m12 = a01 * a02 - a00 * a12, m22 = a00 * a11 - a01 * a01;
    const double det = (a00 * m00 + a01 * m01) + a02 * m02;
    const double y0 = (m00 * b0 + m01 * b1) + m02 * b2, y1 = (m01 * b0 + m11 * b1) + m12 * b2, y2 = (m02 * b0 + m12 * b1) + m22 * b2;
    return Minimiser{det, {-(y0 / det), -(y1 / det), -(y2 / det)}, ((a00 + a11) + a22) / 3.0};
}

// the quadric at the offset z from the point its sums were taken about
VFN_QUADRIC_FN double value_at(const double* s, const double* z) {
    const double p0 = (s[0] * z[0] + s[1] * z[1]) + s[2] * z[2], p1 = (s[1] * z[0] + s[3] * z[1]) + s[4] * z[2],
                 p2 = (s[2] * z[0] + s[4] * z[1]) + s[5] * z[2];
    return (((z[0] * p0 + z[1] * p1) + z[2] * p2) + 2.0 * ((s[6] * z[0] + s[7] * z[1]) + s[8] * z[2])) + s[9];
}

}  // namespace vfn_quadric
