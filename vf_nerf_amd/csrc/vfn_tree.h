// vfn_tree.h — THE FIXED TREE of include/vfn.h, once: the two-level reduction of vfn_metrics.hip (statistics), vfn_icp.hip (the 17 sums)
// and vfn_image.hip (the per-view sums).  No floating-point atomics; the bits are a function of the sizes and the data alone.  A join
// always has the lower slot, lane or partial on the left.  The callers differ in the element (Stats, TreeSum<17>, TreeSum<2>, a
// double), in the join, and in the order of a lane's 16 slots — nothing else.
#pragma once
#include "vfn_common.h"

namespace {

constexpr int TREE_LANES = VFN_TREE_LANES, TREE_PER = VFN_TREE_PER, TREE_TILE = TREE_LANES * TREE_PER;   // 256 x 16 = 4096 values a block
constexpr int TREE_TOP = VFN_TREE_TOP;                                                                   // lanes of the second level

inline long long tree_tiles(long long n) { return (n + TREE_TILE - 1) / TREE_TILE; }

// C sums that travel together; the identity is +0.0
template <int C>
struct TreeSum { double v[C]; };

struct TreeAdd {
    __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
    template <int C>
    __device__ __forceinline__ TreeSum<C> operator()(const TreeSum<C>& a, const TreeSum<C>& b) const {
        TreeSum<C> r;
#pragma unroll
        for (int c = 0; c < C; ++c) r.v[c] = a.v[c] + b.v[c];
        return r;
    }
};

// Block tree over the LANES values of a block (LANES = blockDim.x, a power of two), the same pairs for every launch: lane l takes lane
// l + d for d = LANES / 2 ... 1.  Every lane returns the root.  sh[LANES] may be used again after a barrier of the caller's.
template <int LANES, typename T, typename Join>
__device__ __forceinline__ T tree_block(const T& mine, T* sh, Join join) {
    const int l = threadIdx.x;
    sh[l] = mine;
    __syncthreads();
    for (int d = LANES / 2; d >= 1; d >>= 1) {
        if (l < d) sh[l] = join(sh[l], sh[l + d]);
        __syncthreads();
    }
    return sh[0];
}

// Second level, a lane's share before the block tree over TREE_TOP lanes: lane l starts from partial l (the identity if l >= p) and
// joins the partials l + 1024, l + 2048, ... serially.
template <typename T, typename Load, typename Join>
__device__ __forceinline__ T tree_top_lane(long long p, const T& identity, Load load, Join join) {
    T s = identity;
    bool first = true;
    for (long long i = threadIdx.x; i < p; i += TREE_TOP) {
        s = first ? load(i) : join(s, load(i));
        first = false;
    }
    return s;
}

// Lane tree: the balanced tree (4 levels) over a lane's 16 slots as a binary counter.  leaf(k) is position k of the tree, called in
// ascending k; position k joins the finished subtree of its size on its left for every trailing 1 bit of k, so
// ((p0 + p1) + (p2 + p3)) + ... with at most four finished subtrees alive.  Which slot stands at position k is the caller's lane order:
// "near" = k itself, "far" = tree_far_slot(k).  UNROLL is the caller's too: 1 keeps one leaf in flight, TREE_PER resolves the counter
// at compile time.
template <int UNROLL, typename T, typename Leaf, typename Join>
__device__ __forceinline__ T tree_lane(Leaf leaf, Join join) {
    static_assert(TREE_PER == 16, "the counter below has four levels");
    T s0, s1, s2, s3, a;
#pragma unroll UNROLL
    for (int k = 0; k < TREE_PER; ++k) {
        a = leaf(k);
        if (!(k & 1)) { s0 = a; continue; }
        a = join(s0, a);
        if (!(k & 2)) { s1 = a; continue; }
        a = join(s1, a);
        if (!(k & 4)) { s2 = a; continue; }
        a = join(s2, a);
        if (!(k & 8)) { s3 = a; continue; }
        a = join(s3, a);
    }
    return a;
}

// position -> slot of the "far" order: the 4-bit reversal 0, 8, 4, 12, 2, 10, 6, 14, 1, 9, ... (slot k meets slot k + 8 first)
__device__ __forceinline__ constexpr int tree_far_slot(int k) { return ((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | ((k & 8) >> 3); }

}  // namespace
