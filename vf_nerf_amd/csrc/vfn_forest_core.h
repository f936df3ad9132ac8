// vfn_forest_core.h — the concurrent union-find of csrc/vfn_cc.hip and csrc/vfn_orient.hip (include/vfn.h: vfn_cc_union_runs,
// vfn_cc_flatten, vfn_orient_union_runs, vfn_orient_flatten), as ONE text that compiles for the device and for the host, and ONE text
// for the plain forest and the parity forest: PARITY_BITS is a template argument, 0 for vfn_cc and 1 for vfn_orient, so every shift and
// mask below is a constant and the plain forest pays nothing for the bit it does not have.  `Mem` says how a word of the forest is
// loaded and compare-and-swapped: the device gives relaxed agent-scope atomics on int (csrc/vfn_geom.h: DeviceMem),
// tests/c_abi/forest_core_host.cpp gives std::atomic<int32_t>, so that the loops below run on 16 host threads (under a sanitizer) before
// they ever run on a card.
//
// THE WORD.  forest[x] = (parent << PARITY_BITS) | parity: the parent of x and the parity of x RELATIVE TO THAT PARENT (1: x is wound
//   against it), in ONE int32 — every load and every compare-and-swap sees a parent with ITS parity, never a parent from one write and a
//   parity from another.  The caller fills forest[x] with x << PARITY_BITS: every node a root, parity 0.  So a forest holds fewer than
//   2^(31 - PARITY_BITS) nodes.  Two things only ever write a word:
//   a hook      compare-and-swap forest[a]: (a, 0) -> (b, q) with b < a, where a and b were both found as roots and
//               q = pa ^ pb ^ want: pa, pb the parities the two finds returned for the ends of the requested pair, want the parity the
//               pair asks for between its ends;
//   a halving   compare-and-swap forest[x]: (p, s) -> (g, s ^ u) where (g, u) was loaded from forest[p], g < p < x.  A failure is ignored.
// WITH PARITY_BITS = 0 the word is the parent, the fill is the identity, every parity below is the constant 0 and `want` must be 0: what
//   remains of this text is the plain forest — a hook writes a -> b, a halving p -> g, "a root word with its parity bit set" cannot
//   occur, and of the four arguments only the invariant, the termination and the partition say anything.  They hold as written.
// INVARIANT  parent[x] <= x at all times, with equality exactly while x is a root, and a root's parity bit is 0.  A hook writes b < a.
//   A halving writes g < p.  So a word only ever DECREASES: a node that stopped being a root never becomes one again (no write stores
//   x << PARITY_BITS into forest[x], and a compare-and-swap that expects it cannot be fooled by a word that left and came back).  A
//   halving (whose x is no root) and a hook (whose a is a root) never meet on one word, and a halving replaces an ancestor of x by
//   another ancestor of x: it changes no tree's node set.
// TERMINATION  Every find walks strictly downwards (x -> g < x), so it ends after at most x steps — also on a forest that the caller
//   filled with something else, because a word whose parent lies outside [0, x], or a root word with its parity bit set (on which a
//   hook's swap could never succeed), ends the walk (BAD) before it is used as an index.  A unite repeats only after a failed hook;
//   the hook failed because forest[a] was no longer (a, 0), that is because some other hook succeeded on a in the meantime.  Every
//   successful hook removes one root for good, so over the whole launch hooks succeed at most n - 1 times; and one successful hook
//   fails a given unite at most once (that unite's next find no longer ends at a).  So a unite repeats at most n - 1 times.  Nothing
//   waits for another lane: a lane that lost a swap goes on with its own work, so lanes of one wave that diverge in these loops
//   cannot block each other.
// RELATIVE PARITIES NEVER CHANGE  Define par(x, y), for x and y in one tree, as the XOR of the parity bits along the two chains up to
//   where they meet.  Once x and y are in one tree, par(x, y) never changes.  A halving replaces the chain x -> p -> g by x -> g with
//   the bit s ^ u, the XOR of the two bits it skips: every chain through x keeps its XOR.  A hook hangs a whole tree under a node of
//   another: chains inside either tree are untouched, only chains between the two become defined.  That is why s ^ u is right although
//   forest[p] was read LATER than forest[x]: par(x, p) = s was true when forest[x] was read and is therefore still true, par(p, g) = u
//   was true when forest[p] was read, so par(x, g) = s ^ u holds from then on — and if forest[x] is no longer (p, s) the swap fails and
//   nothing is written.  For the same reason what a find returns stays true: the node it ends at was a root when its word was read,
//   and the parity it accumulated is par(start, that node) for good, root or not.  A hook then hangs the root a under b with
//   q = par(a-end, a) ^ want ^ par(b-end, b): the requested pair gets exactly the parity it asked for, whether or not b is still a root.
// THE PARTITION AND THE ROOTS DO NOT DEPEND ON THE SCHEDULE  Trees only ever merge by hooks, and a hook joins the trees of the two ends of
//   a requested pair: two nodes end in one tree only if a chain of requested pairs joins them.  A unite returns only when both ends ARE
//   in one tree (one root after the finds, or its own hook made them so): every requested pair ends in one tree.  So the final trees
//   are the connected components of the requested pairs, whatever the order.  Inside a tree every non-root has parent < itself, so
//   the root is the component's lowest index, again whatever the order.  The shape of the trees in between does depend on the
//   schedule; the flatten kernels run after the launch and read only where chains end.
// THE PARITIES OF AN ORIENTABLE COMPONENT DO NOT DEPEND ON THE SCHEDULE  Every hook realises the parity of one requested pair, and every
//   final tree is spanned by the pairs whose hooks succeeded: par(x, root) is the XOR of `want` along a chain of requested pairs from x
//   to the root.  In an orientable component all constraints can hold together, so that XOR is the same along EVERY chain of requested
//   pairs — it is the one assignment with parity 0 at the root.  Which pairs became hooks depends on the schedule; the value does not.
//   In a component that is not orientable the pairs whose unite found one root were never compared (conflicts are not judged here) and
//   the parities do depend on the schedule: the caller tests every requested pair against the flattened parities afterwards — some
//   pair must fail, whatever spanning tree the schedule chose — and zeroes the parities of such a component.
#pragma once
#include <stdint.h>
#include "vfn_geom.h"

#if defined(__HIPCC__)
#define VFN_FOREST_FN __device__ __forceinline__
#else
#define VFN_FOREST_FN inline
#endif

namespace vfn_forest {

using vfn_geom::ST_RANGE;                // the status bit of include/vfn.h: a node, a parent or a segment outside its range
constexpr int BAD = -1;                  // a word that is not ours was met

// Mem: struct { using word = ...; static int load(const word*); static int cas(word*, int expected, int desired) -> the value found; }

struct Found {
    int root;          // BAD, or the node the walk ended at (a root when its word was read)
    int parity;        // par(start, root)
};

// -> the root of x's tree at some moment of the call with x's parity relative to it, or BAD.  x in [0, n) is the caller's to check.
template <class Mem, int PARITY_BITS>
VFN_FOREST_FN Found find(typename Mem::word* forest, int x) {
    static_assert(PARITY_BITS == 0 || PARITY_BITS == 1, "a word holds a parent and at most one parity bit");
    constexpr int MASK = (1 << PARITY_BITS) - 1;
    int acc = 0;                                          // par(start, x)
    for (;;) {
        const int w = Mem::load(forest + x);
        const int p = w >> PARITY_BITS, s = w & MASK;
        if (w < 0 || p > x || (p == x && s)) return Found{BAD, 0};
        if (p == x) return Found{x, acc};
        const int w2 = Mem::load(forest + p);
        const int g = w2 >> PARITY_BITS, u = w2 & MASK;
        if (w2 < 0 || g > p || (g == p && u)) return Found{BAD, 0};
        if (g == p) return Found{p, acc ^ s};
        Mem::cas(forest + x, w, (g << PARITY_BITS) | (s ^ u));      // halving: x skips p.  Lost to another halving of x: that one wrote an ancestor too.
        acc ^= s ^ u;
        x = g;
    }
}

// a and b in [0, n), want in [0, 2^PARITY_BITS) -> 0 once they are in one tree (with par(a, b) == want if this call's hook joined them),
// ST_RANGE on a forest that is not ours
template <class Mem, int PARITY_BITS>
VFN_FOREST_FN unsigned unite(typename Mem::word* forest, int a, int b, int want) {
    for (;;) {
        const Found fa = find<Mem, PARITY_BITS>(forest, a);
        const Found fb = find<Mem, PARITY_BITS>(forest, b);
        if (fa.root == BAD || fb.root == BAD) return ST_RANGE;
        want ^= fa.parity ^ fb.parity;                    // now the parity asked for between the two nodes the finds ended at
        a = fa.root;
        b = fb.root;
        if (a == b) return 0u;                            // one tree already: nothing is written, a conflict is the caller's to find
        if (a < b) { const int t = a; a = b; b = t; }     // the larger root goes under the smaller
        if (Mem::cas(forest + a, a << PARITY_BITS, (b << PARITY_BITS) | want) == (a << PARITY_BITS)) return 0u;
        // a was hooked by someone else since the find: find again from where we stand (par(a, b) asked for is still `want`)
    }
}

// node v of the flatten kernels: where v's chain ends and the XOR of the parity bits along it, or BAD (with *status |= ST_RANGE).  No
// halving: the forest is only read.
template <class Mem, int PARITY_BITS>
VFN_FOREST_FN Found chain_end(const typename Mem::word* forest, int v, unsigned* status) {
    constexpr int MASK = (1 << PARITY_BITS) - 1;
    int x = v, acc = 0;
    for (;;) {
        const int w = Mem::load(forest + x);
        const int p = w >> PARITY_BITS, s = w & MASK;
        // (the plain forest asks for a root before the range, the order vfn_cc_flatten was measured with: profiles/r23)
        if constexpr (PARITY_BITS == 0) { if (w == x) return Found{x, 0}; }
        if (w < 0 || p > x || (p == x && s)) { *status |= ST_RANGE; return Found{BAD, 0}; }
        if (p == x) return Found{x, acc};
        acc ^= s;
        x = p;
    }
}

// ---- the two item rules: which pairs of a sorted key list are requested.  No node indexes memory before it has been compared with
// [0, n_nodes).

// item i >= 1 of vfn_cc_union_runs (the plain forest): where keys[i] == keys[i-1] >= 0, unite nodes[i-1] and nodes[i]
template <class Mem>
VFN_FOREST_FN unsigned union_item(const long long* keys, const long long* nodes, long long i, typename Mem::word* parent, long long n_nodes) {
    const long long k = keys[i];
    if (k < 0 || k != keys[i - 1]) return 0u;
    const long long a = nodes[i - 1], b = nodes[i];
    if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) return ST_RANGE;
    return unite<Mem, 0>(parent, (int)a, (int)b, 0);
}

// is (i - 1, i) a run of exactly two equal keys >= 0?
VFN_FOREST_FN bool run_of_two(const long long* keys, long long i, long long n_items) {
    const long long k = keys[i];
    if (k < 0 || k != keys[i - 1]) return false;
    if (i >= 2 && keys[i - 2] == k) return false;
    if (i + 1 < n_items && keys[i + 1] == k) return false;
    return true;
}

// item i >= 1 of vfn_orient_union_runs (the parity forest): a run of two from two faces asks for parity 1 where both traverse the edge
// the same way
template <class Mem>
VFN_FOREST_FN unsigned union_item(const long long* keys, const long long* nodes, const unsigned char* dirs, long long i, long long n_items,
                                  typename Mem::word* forest, long long n_nodes) {
    if (!run_of_two(keys, i, n_items)) return 0u;
    const long long a = nodes[i - 1], b = nodes[i];
    if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes) return ST_RANGE;
    if (a == b) return 0u;                                // both items of one face: no edge between two faces
    const int want = (dirs[i - 1] != 0) == (dirs[i] != 0) ? 1 : 0;
    return unite<Mem, 1>(forest, (int)a, (int)b, want);
}

}  // namespace vfn_forest
