// orient_core_host.cpp — the parity union-find of csrc/vfn_orient_core.h on host threads: the SAME find / unite / union_item / chain_end
// text that csrc/vfn_orient.hip compiles for the device, with std::atomic<int32_t> (relaxed, as on the device) in place of the device's
// atomics.  A stand-alone program: build it with the host compiler, with -fsanitize=address,undefined or -fsanitize=thread, and run it
// before the kernels ever see a card — a union-find that spins would hang one.
//
//   orient_core_host THREADS < cases
// reads cases of the form
//   n_nodes n_items            (n_nodes = 0 ends the input)
//   key node dir               n_items lines: the sorted keys with their nodes and direction bytes, as vfn_orient_union_runs takes them
// runs every case once on ONE thread in item order, then on THREADS threads with the items dealt in four ways — strided (thread t takes
// t, t + THREADS, ...: neighbouring items, the ones that meet on the same words, always on different threads), strided from the last
// item down, in contiguous blocks, and strided through a fixed shuffle — and holds every threaded run to the serial one: the status, every
// root, and every parity of a component in which the serial parities break no constraint (the others depend on the schedule by
// contract).  Prints per case three lines: "status mismatches broken_constraints", root[0 .. n_nodes), parity[0 .. n_nodes) of the serial run.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <thread>
#include <vector>

#include "../../vf_nerf_amd/csrc/vfn_orient_core.h"

struct HostMem {
    using word = std::atomic<int32_t>;
    static int load(const word* p) { return p->load(std::memory_order_relaxed); }
    static int cas(word* p, int expected, int desired) {
        int32_t e = expected;
        p->compare_exchange_strong(e, desired, std::memory_order_relaxed, std::memory_order_relaxed);
        return e;
    }
};

struct Result {
    unsigned status = 0u;
    std::vector<int> root;
    std::vector<unsigned char> parity;
};

// work[t]: the items thread t takes, in its order
static Result run(const std::vector<long long>& keys, const std::vector<long long>& nodes, const std::vector<unsigned char>& dirs,
                  long long n_nodes, const std::vector<std::vector<long long>>& work) {
    const long long n_items = (long long)keys.size();
    std::vector<std::atomic<int32_t>> forest((size_t)n_nodes);
    for (long long v = 0; v < n_nodes; ++v) forest[(size_t)v].store((int32_t)(v << 1), std::memory_order_relaxed);
    std::atomic<unsigned> status{0u};
    std::vector<std::thread> pool;
    for (size_t t = 0; t < work.size(); ++t)
        pool.emplace_back([&, t] {
            unsigned mine = 0u;
            for (long long i : work[t])
                mine |= vfn_orient::union_item<HostMem>(keys.data(), nodes.data(), dirs.data(), i, n_items, forest.data(), n_nodes);
            status.fetch_or(mine, std::memory_order_relaxed);
        });
    for (auto& th : pool) th.join();
    Result r;
    r.status = status.load();
    r.root.resize((size_t)n_nodes);
    r.parity.resize((size_t)n_nodes);
    for (long long v = 0; v < n_nodes; ++v) {
        const vfn_orient::Found e = vfn_orient::chain_end<HostMem>(forest.data(), (int)v, &r.status);
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

// words that are not ours end a walk before they index anything, and nothing is written
static bool refuses_foreign_words() {
    struct Case { int32_t words[3]; int at; };
    const Case cases[4] = {{{1, 2, 4}, 0},            // a root with its parity bit set
                           {{0, 10, 4}, 1},           // a parent above its node
                           {{0, -2, 4}, 1},           // a negative word
                           {{0, 2, 5}, 2}};           // a root with its parity bit set, further up
    for (const Case& c : cases) {
        std::atomic<int32_t> forest[3];
        for (int v = 0; v < 3; ++v) forest[v].store(c.words[v], std::memory_order_relaxed);
        unsigned st = 0u;
        if (vfn_orient::find<HostMem>(forest, c.at).root != vfn_orient::BAD) return false;
        if (vfn_orient::chain_end<HostMem>(forest, c.at, &st).root != vfn_orient::BAD || st != vfn_orient::ST_RANGE) return false;
        if (vfn_orient::unite<HostMem>(forest, c.at, c.at == 0 ? 1 : 0, 1) != vfn_orient::ST_RANGE) return false;
        for (int v = 0; v < 3; ++v)
            if (forest[v].load() != c.words[v]) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 16;
    if (threads < 1 || threads > 256) { fprintf(stderr, "orient_core_host: THREADS outside [1, 256]\n"); return 2; }
    if (!refuses_foreign_words()) { fprintf(stderr, "orient_core_host: a foreign word was followed\n"); return 3; }
    long long n_nodes, n_items;
    while (scanf("%lld %lld", &n_nodes, &n_items) == 2 && n_nodes > 0) {
        if (n_nodes >= (1ll << 30) || n_items < 0) { fprintf(stderr, "orient_core_host: bad counts\n"); return 2; }
        std::vector<long long> keys((size_t)n_items), nodes((size_t)n_items);
        std::vector<unsigned char> dirs((size_t)n_items);
        for (long long i = 0; i < n_items; ++i) {
            int d;
            if (scanf("%lld %lld %d", &keys[(size_t)i], &nodes[(size_t)i], &d) != 3) { fprintf(stderr, "orient_core_host: short case\n"); return 2; }
            dirs[(size_t)i] = (unsigned char)d;
        }
        const Result serial = run(keys, nodes, dirs, n_nodes, deal(n_items, 1, 0));
        // the constraints the serial parities break, and the components (by root) they make non-orientable
        std::vector<char> broken((size_t)n_nodes, 0);
        long long n_broken = 0;
        for (long long i = 1; i < n_items; ++i) {
            if (!vfn_orient::run_of_two(keys.data(), i, n_items)) continue;
            const long long a = nodes[(size_t)i - 1], b = nodes[(size_t)i];
            if (a < 0 || a >= n_nodes || b < 0 || b >= n_nodes || a == b || serial.root[(size_t)a] < 0) continue;
            const int want = (dirs[(size_t)i - 1] != 0) == (dirs[(size_t)i] != 0);
            if ((serial.parity[(size_t)a] ^ serial.parity[(size_t)b]) != want) { broken[(size_t)serial.root[(size_t)a]] = 1; ++n_broken; }
        }
        long long mismatches = 0;
        for (int how = 0; how < 4; ++how) {
            const Result got = run(keys, nodes, dirs, n_nodes, deal(n_items, threads, how));
            if (got.status != serial.status) ++mismatches;
            for (long long v = 0; v < n_nodes; ++v) {
                if (got.root[(size_t)v] != serial.root[(size_t)v]) { ++mismatches; continue; }
                const int r = serial.root[(size_t)v];
                if (r >= 0 && !broken[(size_t)r] && got.parity[(size_t)v] != serial.parity[(size_t)v]) ++mismatches;
            }
        }
        printf("%u %lld %lld\n", serial.status, mismatches, n_broken);
        for (long long v = 0; v < n_nodes; ++v) printf(v ? " %d" : "%d", serial.root[(size_t)v]);
        printf("\n");
        for (long long v = 0; v < n_nodes; ++v) printf(v ? " %d" : "%d", (int)serial.parity[(size_t)v]);
        printf("\n");
    }
    return 0;
}
