// vfn_proximity_core.h — the closest point of ONE triangle to ONE query (include/vfn.h: vfn_closest_on_triangle), as ONE text that
// compiles for the device (csrc/vfn_proximity.hip) and for the host (tests/c_abi/proximity_core_host.cpp runs it under a sanitizer).
// fp64 throughout, built without contraction on both sides (-ffp-contract=off): the expressions of include/vfn.h, operation for
// operation.  A pure function of its twelve inputs: no memory is read, nothing depends on a neighbour.
//
// Seven candidates in a fixed order — the closest points of the segments AB, BC, CA (1-3), the foot of the perpendicular on the plane
// where it falls inside the triangle (4), and the vertices A, B, C in their own bits (5-7) —, each clamped into the triangle's box, each
// with d2 = the point-to-point expression (dx dx + dy dy) + dz dz; the result is the minimum of (d2, candidate number).
// Every comparison is written so that a NaN intermediate (possible only where a product of finite inputs overflows) takes a defined
// branch and is replaced by a number: min / max / clamp are comparisons, never fmin / fmax, whose answer for -0 against +0 is the
// library's choice.
#pragma once

#if defined(__HIPCC__)
#define VFN_PROXIMITY_FN __host__ __device__ __forceinline__
#else
#define VFN_PROXIMITY_FN inline
#endif

namespace vfn_proximity {

constexpr int CANDIDATES = 7;

// the squared distance of include/vfn.h (vfn_nn_sqdist): the same expression as vfn_pair_sqdist of csrc/vfn_common.h
VFN_PROXIMITY_FN double pair_sqdist(const double* q, const double* t) {
    const double dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
    return (dx * dx + dy * dy) + dz * dz;
}

VFN_PROXIMITY_FN double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

VFN_PROXIMITY_FN void cross3(const double* a, const double* b, double* out) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// x into [lo, hi] by comparisons: a NaN becomes lo, a value equal to a bound keeps its own bits
VFN_PROXIMITY_FN double clamp_into(double x, double lo, double hi) {
    if (!(x >= lo)) x = lo;
    if (!(x <= hi)) x = hi;
    return x;
}

struct Best {
    double c[3], d2;
};

// the candidate `p`, clamped into the box, against the best so far: strictly smaller d2 only, so an earlier candidate keeps a tie
VFN_PROXIMITY_FN void offer(const double* q, const double* p, const double* lo, const double* hi, bool first, Best& best) {
    const double c[3] = {clamp_into(p[0], lo[0], hi[0]), clamp_into(p[1], lo[1], hi[1]), clamp_into(p[2], lo[2], hi[2])};
    const double d2 = pair_sqdist(q, c);
    if (first || d2 < best.d2) {
        best.c[0] = c[0]; best.c[1] = c[1]; best.c[2] = c[2];
        best.d2 = d2;
    }
}

// the closest point of the segment P -> Q: t = dot(q - P, d) / dot(d, d) with d = Q - P; t <= 0 or dot(d, d) == 0: P itself,
// t >= 1: Q itself, otherwise P + t d
VFN_PROXIMITY_FN void on_segment(const double* q, const double* P, const double* Q, double* out) {
    const double d[3] = {Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]};
    const double w[3] = {q[0] - P[0], q[1] - P[1], q[2] - P[2]};
    const double dd = dot3(d, d);
    const double t = dot3(w, d) / dd;
    if (dd == 0.0 || t <= 0.0) {
        out[0] = P[0]; out[1] = P[1]; out[2] = P[2];
    } else if (t >= 1.0) {
        out[0] = Q[0]; out[1] = Q[1]; out[2] = Q[2];
    } else {
        out[0] = P[0] + t * d[0]; out[1] = P[1] + t * d[1]; out[2] = P[2] + t * d[2];
    }
}

// the edge function of P1 -> P2 at p: dot((P2 - P1) x (p - P1), n); >= 0 on the inner side and on the edge's line
VFN_PROXIMITY_FN double edge_side(const double* P1, const double* P2, const double* p, const double* n) {
    const double u[3] = {P2[0] - P1[0], P2[1] - P1[1], P2[2] - P1[2]};
    const double v[3] = {p[0] - P1[0], p[1] - P1[1], p[2] - P1[2]};
    double c[3];
    cross3(u, v, c);
    return dot3(c, n);
}

// -> c[3], *d2 of include/vfn.h: vfn_closest_on_triangle
VFN_PROXIMITY_FN void closest_on_triangle(const double* q, const double* A, const double* B, const double* C, double* c, double* d2) {
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = A[k]; hi[k] = A[k];
        if (B[k] < lo[k]) lo[k] = B[k];
        if (C[k] < lo[k]) lo[k] = C[k];
        if (B[k] > hi[k]) hi[k] = B[k];
        if (C[k] > hi[k]) hi[k] = C[k];
    }
    Best best;
    double p[3];
    on_segment(q, A, B, p);
    offer(q, p, lo, hi, true, best);
    on_segment(q, B, C, p);
    offer(q, p, lo, hi, false, best);
    on_segment(q, C, A, p);
    offer(q, p, lo, hi, false, best);
    const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const double e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    double n[3];
    cross3(e1, e2, n);
    const double nn = dot3(n, n);
    if (nn > 0.0) {
        const double w[3] = {q[0] - A[0], q[1] - A[1], q[2] - A[2]};
        const double s = dot3(w, n) / nn;
        p[0] = q[0] - s * n[0]; p[1] = q[1] - s * n[1]; p[2] = q[2] - s * n[2];
        if (edge_side(A, B, p, n) >= 0.0 && edge_side(B, C, p, n) >= 0.0 && edge_side(C, A, p, n) >= 0.0) offer(q, p, lo, hi, false, best);
    }
    offer(q, A, lo, hi, false, best);
    offer(q, B, lo, hi, false, best);
    offer(q, C, lo, hi, false, best);
    c[0] = best.c[0]; c[1] = best.c[1]; c[2] = best.c[2];
    *d2 = best.d2;
}

}  // namespace vfn_proximity
