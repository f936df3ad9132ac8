// vfn_cc_core.h — the concurrent union-find of csrc/vfn_cc.hip (include/vfn.h: vfn_cc_union_runs, vfn_cc_flatten), as ONE text that
// compiles for the device and for the host.  `Mem` says how a word of the forest is loaded and compare-and-swapped: the device gives
// relaxed agent-scope atomics on int, tests/c_abi/cc_core_host.cpp gives std::atomic<int32_t>, so that the loops below run on 16 host
// threads (under a sanitizer) before they ever run on a card.
//
// THE FOREST.  parent[x] is a node index; the caller fills it with the identity.  Two things only ever write it:
//   a hook      compare-and-swap parent[a]: a -> b with b < a, where a and b were both found as roots;
//   a halving   compare-and-swap parent[x]: p -> g with g = parent[p] < p < x (path halving; a failure is ignored).
// INVARIANT  parent[x] <= x at all times, with equality exactly while x is a root.  A hook writes b < a.  A halving writes g < p <= the
//   word it replaces.  A node that stopped being a root never becomes one again: only a hook's swap expects parent[a] == a, and
//   no write ever stores x into parent[x].  So a halving (whose x is no root) and a hook (whose a is a root) never meet on one word,
//   and a halving replaces an ancestor of x by another ancestor of x: it changes no tree's node set.
// TERMINATION  Every find walks strictly downwards (x -> g < x), so it ends after at most x steps — also on a forest that the caller
//   filled with something else, because a word outside [0, x] ends the walk (BAD) before it is used as an index.  A unite repeats only
//   after a failed hook; the hook failed because parent[a] was no longer a, that is because some other hook succeeded on a in the
//   meantime.  Every successful hook removes one root for good, so over the whole launch hooks succeed at most n - 1 times; and one
//   successful hook fails a given unite at most once (that unite's next find no longer ends at a).  So a unite repeats at most n - 1
//   times.  Nothing waits for another lane: a lane that lost a swap goes on with its own work, so lanes of one wave that diverge in
//   these loops cannot block each other.
// THE RESULT DOES NOT DEPEND ON THE SCHEDULE  Trees only ever merge by hooks, and a hook joins the trees of the two ends of a requested
//   pair: two nodes end in one tree only if a chain of requested pairs joins them.  A unite returns only when both ends ARE in one
//   tree (a == b after the finds, or its own hook made them so): every requested pair ends in one tree.  So the final trees are the
//   connected components of the requested pairs, whatever the order.  Inside a tree every non-root has parent[x] < x, so the root is
//   smaller than every other node of its tree: the root is the component's lowest index, again whatever the order.  The shape of
//   the trees in between does depend on the schedule; vfn_cc_flatten runs after the launch and reads only where chains end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VFN_CC_FN __device__ __forceinline__
#else
#define VFN_CC_FN inline
#endif

namespace vfn_cc {

constexpr int BAD = -1;                  // a word outside [0, x] was met: the forest is not one of ours
constexpr unsigned ST_RANGE = 2u;        // the status bit of include/vfn.h: a node, a parent or a segment outside its range

// Mem: struct { using word = ...; static int load(const word*); static int cas(word*, int expected, int desired) -> the value found; }

// -> the root of x's tree at some moment of the call, or BAD.  x in [0, n) is the caller's to check.
template <class Mem>
VFN_CC_FN int find(typename Mem::word* parent, int x) {
    for (;;) {
        const int p = Mem::load(parent + x);
        if (p == x) return x;
        if (p < 0 || p > x) return BAD;
        const int g = Mem::load(parent + p);
        if (g == p) return p;
        if (g < 0 || g > p) return BAD;
        Mem::cas(parent + x, p, g);          // halving: x skips p.  Lost to another halving of x: that one wrote an ancestor too.
        x = g;
    }
}

// a and b in [0, n) -> 0 once they are in one tree, ST_RANGE on a forest that is not ours
template <class Mem>
VFN_CC_FN unsigned unite(typename Mem::word* parent, int a, int b) {
    for (;;) {
        a = find<Mem>(parent, a);
        b = find<Mem>(parent, b);
        if (a == BAD || b == BAD) return ST_RANGE;
        if (a == b) return 0u;
        if (a < b) { const int t = a; a = b; b = t; }          // the larger root goes under the smaller
        if (Mem::cas(parent + a, a, b) == a) return 0u;
        // a was hooked by someone else since the find: find again from where we stand
    }
}

// item i >= 1 of vfn_cc_union_runs: where keys[i] == keys[i-1] >= 0, unite nodes[i-1] and nodes[i].  No node indexes memory before it
// has been compared with [0, n_nodes).
template <class Mem>
VFN_CC_FN unsigned union_item(const long long* keys, const long long* nodes, long long i, typename Mem::word* parent, long long n_nodes) {
    const long long k = keys[i];
    if (k < 0 || k != keys[i - 1]) return 0u;
    const long long a = nodes[i - 1], b = nodes[i];
    if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) return ST_RANGE;
    return unite<Mem>(parent, (int)a, (int)b);
}

// node v of vfn_cc_flatten: where v's chain ends, or BAD (with *status |= ST_RANGE) when a parent leaves [0, its node].  No halving:
// the forest is only read.
template <class Mem>
VFN_CC_FN int chain_end(const typename Mem::word* parent, int v, unsigned* status) {
    int x = v;
    for (;;) {
        const int p = Mem::load(parent + x);
        if (p == x) return x;
        if (p < 0 || p > x) { *status |= ST_RANGE; return BAD; }
        x = p;
    }
}

}  // namespace vfn_cc
