// vfn_collapse_core.h — what one edge of csrc/vfn_collapse.hip (include/vfn.h: vfn_edge_collapse_candidates) computes, as ONE text that
// compiles for the device and for the host: the sum of the two end quadrics, the solve of csrc/vfn_quadric.h, the fallback to
// the midpoint or an end, the attribute parameter and the flip test over both 1-rings through the vertices' item table.
// tests/c_abi/collapse_core_host.cpp runs it over small meshes under a sanitizer before it ever runs on a card.  fp64 throughout, built
// without contraction on both sides (-ffp-contract=off): the expressions of include/vfn.h, operation for operation.  Nothing is read
// through a segment bound, a row or a vertex index before it has been compared with its range.
#pragma once
#include <math.h>
#include <stdint.h>
#include "vfn_geom.h"
#include "vfn_quadric.h"

#if defined(__HIPCC__)
#define VFN_COLLAPSE_FN __host__ __device__ __forceinline__
#else
#define VFN_COLLAPSE_FN inline
#endif

namespace vfn_collapse {

using vfn_geom::ST_INDEX;
using vfn_geom::ST_NONFINITE;
using vfn_quadric::CHANNELS;
using vfn_quadric::value_at;
// the flag byte of an edge
constexpr unsigned char F_CANDIDATE = 1, F_ACCEPTED = 2, F_NONMANIFOLD = 4, F_NONFINITE = 8, F_OVER = 16, F_FLIP = 32;

struct Mesh {
    const double* v;             // [n, 3]
    long long n;
    const long long* f;          // [m, 3]
    long long m;
    const double* q;             // [n, 10]: the vertices' quadrics about the origin
    const long long* item_row;   // [n_items]: every vertex's plane rows, ascending; rows >= m are boundary rows, not faces
    long long n_items;
    const long long* start;      // [n + 1]
    long long rows;              // m + the boundary rows
    double o[3];                 // the frame's origin
    double rcond, reach, max_error;
};

struct Edge {
    double point[3], cost, s;
    unsigned char flags;
};

// the faces of vertex `moving` that do not name `other`, with `moving` at `point`: false as soon as one of them turns over.
// -> status bits; *ok is cleared on a flip
VFN_COLLAPSE_FN unsigned ring_keeps_its_side(const Mesh& g, long long moving, long long other, const double* point, bool* ok) {
    const long long b = g.start[moving], e = g.start[moving + 1];
    if (b < 0 || e < b || e > g.n_items) return ST_INDEX;
    for (long long j = b; j < e; ++j) {
        const long long row = g.item_row[j];
        if (row < 0 || row >= g.rows) return ST_INDEX;
        if (row >= g.m) continue;                                                   // a boundary row: no face
        const long long i[3] = {g.f[3 * row], g.f[3 * row + 1], g.f[3 * row + 2]};
        if (i[0] < 0 || i[0] >= g.n || i[1] < 0 || i[1] >= g.n || i[2] < 0 || i[2] >= g.n) return ST_INDEX;
        if (i[0] == other || i[1] == other || i[2] == other) continue;              // it names both ends: the collapse removes it
        if (i[0] != moving && i[1] != moving && i[2] != moving) return ST_INDEX;     // the table names a face that is not the vertex's
        double p[3][3], w[3][3];
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) {
                p[c][k] = g.v[3 * i[c] + k];
                w[c][k] = i[c] == moving ? point[k] : p[c][k];
            }
        const double a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double d[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double c_old[3] = {a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]};
        if (c_old[0] == 0.0 && c_old[1] == 0.0 && c_old[2] == 0.0) continue;         // a face without area imposes nothing
        const double an[3] = {w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2]};
        const double dn[3] = {w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2]};
        const double c_new[3] = {an[1] * dn[2] - an[2] * dn[1], an[2] * dn[0] - an[0] * dn[2], an[0] * dn[1] - an[1] * dn[0]};
        const double dot = (c_old[0] * c_new[0] + c_old[1] * c_new[1]) + c_old[2] * c_new[2];
        if (!(dot > 0.0)) { *ok = false; return 0u; }                                // (false on a NaN too)
    }
    return 0u;
}

// the edge (a, b) held by `run` corner pairs -> what a collapse of it would do; the status bits are returned
VFN_COLLAPSE_FN unsigned edge(const Mesh& g, long long a, long long b, long long run, Edge* out) {
    const double nan = __builtin_nan("");
    out->point[0] = out->point[1] = out->point[2] = out->cost = out->s = nan;
    out->flags = 0;
    if (a < 0 || a >= g.n || b < 0 || b >= g.n || a == b) return ST_INDEX;
    double s[CHANNELS], pa[3], pb[3], d[3], mid[3];
    for (int c = 0; c < CHANNELS; ++c) s[c] = g.q[CHANNELS * a + c] + g.q[CHANNELS * b + c];
    for (int k = 0; k < 3; ++k) {
        pa[k] = g.v[3 * a + k];
        pb[k] = g.v[3 * b + k];
        d[k] = pb[k] - pa[k];
        mid[k] = 0.5 * (pa[k] + pb[k]);
    }
    const double l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const vfn_quadric::Minimiser mn = vfn_quadric::minimiser(s);
    const double* x = mn.x;
    const double r[3] = {x[0] - (mid[0] - g.o[0]), x[1] - (mid[1] - g.o[1]), x[2] - (mid[2] - g.o[2])};
    const double r2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    // (every comparison is false on a NaN)
    const bool accepted = mn.det > g.rcond * ((mn.t * mn.t) * mn.t) && r2 <= (g.reach * g.reach) * l2;
    double point[3], value;
    if (accepted) {
        for (int k = 0; k < 3; ++k) point[k] = g.o[k] + x[k];
        value = value_at(s, x);
    } else {                                                                         // the lowest of (midpoint, Pa, Pb), a tie to the earlier
        const double* tried[3] = {mid, pa, pb};
        value = nan;
        for (int c = 0; c < 3; ++c) {
            const double z[3] = {tried[c][0] - g.o[0], tried[c][1] - g.o[1], tried[c][2] - g.o[2]};
            const double val = value_at(s, z);
            if (c == 0 || val < value) {
                value = val;
                for (int k = 0; k < 3; ++k) point[k] = tried[c][k];
            }
        }
    }
    const double cost = value > 0.0 ? value : 0.0;                                   // +0.0 for a value of -0.0, below zero or NaN
    const double gap[3] = {point[0] - pa[0], point[1] - pa[1], point[2] - pa[2]};
    double par = ((gap[0] * d[0] + gap[1] * d[1]) + gap[2] * d[2]) / l2;
    if (!(par >= 0.0)) par = 0.0;                                                    // below 0, -0.0 and NaN (an edge without length)
    if (par > 1.0) par = 1.0;
    for (int k = 0; k < 3; ++k) out->point[k] = point[k];
    out->cost = cost;
    out->s = par;
    unsigned status = 0;
    unsigned char flags = accepted ? F_ACCEPTED : 0;
    if (run > 2) flags |= F_NONMANIFOLD;
    if (!isfinite(value) || !isfinite(point[0]) || !isfinite(point[1]) || !isfinite(point[2])) {
        flags |= F_NONFINITE;
        status |= ST_NONFINITE;
    }
    if (cost > g.max_error) flags |= F_OVER;
    if (!(flags & (F_NONMANIFOLD | F_NONFINITE | F_OVER))) {                         // the flip test, of those that are still candidates only
        bool ok = true;
        status |= ring_keeps_its_side(g, a, b, point, &ok);
        if (ok && !(status & ST_INDEX)) status |= ring_keeps_its_side(g, b, a, point, &ok);
        if (!ok) flags |= F_FLIP;
        else if (!(status & ST_INDEX)) flags |= F_CANDIDATE;
    }
    out->flags = flags;
    return status;
}

}  // namespace vfn_collapse
