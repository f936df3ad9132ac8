// forest_core_host.cpp — the union-find of csrc/vfn_forest_core.h on host threads: the SAME find / unite / union_item / chain_end text that
// csrc/vfn_cc.hip (the plain forest) and csrc/vfn_orient.hip (the parity forest) compile for the device, with std::atomic<int32_t>
// (relaxed, as on the device) in place of the device's atomics.  A stand-alone program: build it with the host compiler, with
// -fsanitize=address,undefined or -fsanitize=thread, and run it before the kernels ever see a card — a union-find that spins would hang one.
//
//   forest_core_host MODE THREADS < cases          MODE: plain | parity
// reads cases of the form
//   n_nodes n_items            (n_nodes = 0 ends the input)
//   key node                   plain: n_items lines, the sorted keys with their nodes, as vfn_cc_union_runs takes them
//   key node dir               parity: with their direction bytes, as vfn_orient_union_runs takes them
// runs every case once on ONE thread in item order, then on THREADS threads with the items dealt in four ways — strided (thread t takes
// t, t + THREADS, ...: neighbouring items, the ones that meet on the same words, always on different threads), strided from the last
// item down, in contiguous blocks, and strided through a fixed shuffle — and holds every threaded run to the serial one: the status, every
// root, and every parity of a component in which the serial parities break no constraint (the others depend on the schedule by
// contract).  Prints of the serial run, per case,
//   plain:  one line, the status word, then root[0 .. n_nodes)
//   parity: three lines, "status mismatches broken_constraints", root[0 .. n_nodes), parity[0 .. n_nodes)
// and exits with 4 if any threaded run of any case differed from its serial one.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>
#include <vector>

#include "../../vf_nerf_amd/csrc/vfn_forest_core.h"

struct HostMem {
    using word = std::atomic<int32_t>;
    static int load(const word* p) { return p->load(std::memory_order_relaxed); }
    static int cas(word* p, int expected, int desired) {
        int32_t e = expected;
        p->compare_exchange_strong(e, desired, std::memory_order_relaxed, std::memory_order_relaxed);
        return e;
    }
};

struct Case {
    long long n_nodes = 0;
    std::vector<long long> keys, nodes;
    std::vector<unsigned char> dirs;          // parity only
};

struct Result {
    unsigned status = 0u;
    std::vector<int> root;
    std::vector<unsigned char> parity;
};

// work[t]: the items thread t takes, in its order
template <int PARITY_BITS>
static Result run(const Case& c, const std::vector<std::vector<long long>>& work) {
    const long long n_items = (long long)c.keys.size();
    std::vector<std::atomic<int32_t>> forest((size_t)c.n_nodes);
    for (long long v = 0; v < c.n_nodes; ++v) forest[(size_t)v].store((int32_t)(v << PARITY_BITS), std::memory_order_relaxed);
    std::atomic<unsigned> status{0u};
    std::vector<std::thread> pool;
    for (size_t t = 0; t < work.size(); ++t)
        pool.emplace_back([&, t] {
            unsigned mine = 0u;
            for (long long i : work[t]) {
                if constexpr (PARITY_BITS != 0)
                    mine |= vfn_forest::union_item<HostMem>(c.keys.data(), c.nodes.data(), c.dirs.data(), i, n_items, forest.data(), c.n_nodes);
                else
                    mine |= vfn_forest::union_item<HostMem>(c.keys.data(), c.nodes.data(), i, forest.data(), c.n_nodes);
            }
            status.fetch_or(mine, std::memory_order_relaxed);
        });
    for (auto& th : pool) th.join();
    Result r;
    r.status = status.load();
    r.root.resize((size_t)c.n_nodes);
    r.parity.resize((size_t)c.n_nodes);
    for (long long v = 0; v < c.n_nodes; ++v) {
        const vfn_forest::Found e = vfn_forest::chain_end<HostMem, PARITY_BITS>(forest.data(), (int)v, &r.status);
        r.root[(size_t)v] = e.root;
        r.parity[(size_t)v] = (unsigned char)e.parity;
    }
    return r;
}

// the items 1 .. n_items - 1 dealt to the threads: 0 strided, 1 strided from the last item down, 2 contiguous blocks, 3 strided through a shuffle
static std::vector<std::vector<long long>> deal(long long n_items, int threads, int how) {
    std::vector<long long> order((size_t)(n_items > 0 ? n_items - 1 : 0));
    std::iota(order.begin(), order.end(), 1ll);
    if (how == 1) std::reverse(order.begin(), order.end());
    if (how == 3) {
        unsigned long long s = 0x9e3779b97f4a7c15ull;
        for (size_t q = order.size(); q > 1; --q) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(order[q - 1], order[(size_t)((s >> 33) % q)]);
        }
    }
    std::vector<std::vector<long long>> work((size_t)threads);
    const size_t per = (order.size() + (size_t)threads - 1) / (size_t)threads;
    for (size_t q = 0; q < order.size(); ++q) work[how == 2 ? q / per : q % (size_t)threads].push_back(order[q]);
    return work;
}

// words that are not ours end a walk before they index anything, and nothing is written.  The forests are written as (parent, parity)
// pairs; the plain forest takes those of them that need no parity bit.
template <int PARITY_BITS>
static bool refuses_foreign_words() {
    struct Foreign { int parent[3], parity[3], at; };
    const Foreign cases[4] = {{{0, 1, 2}, {1, 0, 0}, 0},            // a root with its parity bit set
                              {{0, 5, 2}, {0, 0, 0}, 1},            // a parent above its node
                              {{0, -1, 2}, {0, 0, 0}, 1},           // a negative word
                              {{0, 1, 2}, {0, 0, 1}, 2}};           // a root with its parity bit set, further up
    for (const Foreign& c : cases) {
        if (!PARITY_BITS && (c.parity[0] || c.parity[1] || c.parity[2])) continue;
        std::atomic<int32_t> forest[3];
        int32_t words[3];
        for (int v = 0; v < 3; ++v) {
            words[v] = (int32_t)(c.parent[v] * (1 << PARITY_BITS)) | c.parity[v];
            forest[v].store(words[v], std::memory_order_relaxed);
        }
        unsigned st = 0u;
        if (vfn_forest::find<HostMem, PARITY_BITS>(forest, c.at).root != vfn_forest::BAD) return false;
        if (vfn_forest::chain_end<HostMem, PARITY_BITS>(forest, c.at, &st).root != vfn_forest::BAD || st != vfn_forest::ST_RANGE) return false;
        if (vfn_forest::unite<HostMem, PARITY_BITS>(forest, c.at, c.at == 0 ? 1 : 0, PARITY_BITS) != vfn_forest::ST_RANGE) return false;
        for (int v = 0; v < 3; ++v)
            if (forest[v].load() != words[v]) return false;
    }
    return true;
}

// -> 0, 2 on bad input, 3 on a foreign word followed, 4 on a threaded run that differed from the serial one
template <int PARITY_BITS>
static int run_cases(int threads) {
    if (!refuses_foreign_words<PARITY_BITS>()) { fprintf(stderr, "forest_core_host: a foreign word was followed\n"); return 3; }
    long long n_items, differed = 0;
    Case c;
    while (scanf("%lld %lld", &c.n_nodes, &n_items) == 2 && c.n_nodes > 0) {
        if (c.n_nodes >= (1ll << (31 - PARITY_BITS)) || n_items < 0) { fprintf(stderr, "forest_core_host: bad counts\n"); return 2; }
        c.keys.assign((size_t)n_items, 0);
        c.nodes.assign((size_t)n_items, 0);
        c.dirs.assign((size_t)n_items, 0);
        for (long long i = 0; i < n_items; ++i) {
            int d = 0;
            bool ok = scanf("%lld %lld", &c.keys[(size_t)i], &c.nodes[(size_t)i]) == 2;
            if (PARITY_BITS) ok = ok && scanf("%d", &d) == 1;
            if (!ok) { fprintf(stderr, "forest_core_host: short case\n"); return 2; }
            c.dirs[(size_t)i] = (unsigned char)d;
        }
        const Result serial = run<PARITY_BITS>(c, deal(n_items, 1, 0));
        // the constraints the serial parities break, and the components (by root) they make non-orientable
        std::vector<char> broken((size_t)c.n_nodes, 0);
        long long n_broken = 0;
        for (long long i = 1; PARITY_BITS && i < n_items; ++i) {
            if (!vfn_forest::run_of_two(c.keys.data(), i, n_items)) continue;
            const long long a = c.nodes[(size_t)i - 1], b = c.nodes[(size_t)i];
            if (a < 0 || a >= c.n_nodes || b < 0 || b >= c.n_nodes || a == b || serial.root[(size_t)a] < 0) continue;
            const int want = (c.dirs[(size_t)i - 1] != 0) == (c.dirs[(size_t)i] != 0);
            if ((serial.parity[(size_t)a] ^ serial.parity[(size_t)b]) != want) { broken[(size_t)serial.root[(size_t)a]] = 1; ++n_broken; }
        }
        long long mismatches = 0;
        for (int how = 0; how < 4; ++how) {
            const Result got = run<PARITY_BITS>(c, deal(n_items, threads, how));
            if (got.status != serial.status) ++mismatches;
            for (long long v = 0; v < c.n_nodes; ++v) {
                if (got.root[(size_t)v] != serial.root[(size_t)v]) { ++mismatches; continue; }
                const int r = serial.root[(size_t)v];
                if (r >= 0 && !broken[(size_t)r] && got.parity[(size_t)v] != serial.parity[(size_t)v]) ++mismatches;
            }
        }
        differed += mismatches;
        if (PARITY_BITS) {
            printf("%u %lld %lld\n", serial.status, mismatches, n_broken);
            for (long long v = 0; v < c.n_nodes; ++v) printf(v ? " %d" : "%d", serial.root[(size_t)v]);
            printf("\n");
            for (long long v = 0; v < c.n_nodes; ++v) printf(v ? " %d" : "%d", (int)serial.parity[(size_t)v]);
            printf("\n");
        } else {
            printf("%u", serial.status);
            for (long long v = 0; v < c.n_nodes; ++v) printf(" %d", serial.root[(size_t)v]);
            printf("\n");
        }
    }
    if (differed) { fprintf(stderr, "forest_core_host: %lld values of threaded runs differ from the serial run\n", differed); return 4; }
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    const int threads = argc > 2 ? atoi(argv[2]) : 16;
    if (threads < 1 || threads > 256) { fprintf(stderr, "forest_core_host: THREADS outside [1, 256]\n"); return 2; }
    if (!strcmp(mode, "plain")) return run_cases<0>(threads);
    if (!strcmp(mode, "parity")) return run_cases<1>(threads);
    fprintf(stderr, "forest_core_host: MODE is plain or parity\n");
    return 2;
}
