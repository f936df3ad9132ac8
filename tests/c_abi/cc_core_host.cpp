// cc_core_host.cpp — the union-find of csrc/vfn_cc_core.h on host threads: the SAME find / unite / union_item / chain_end text that
// csrc/vfn_cc.hip compiles for the device, with std::atomic<int32_t> (relaxed, as on the device) in place of the device's atomics.
// A stand-alone program: build it with the host compiler, with -fsanitize=address,undefined or -fsanitize=thread, and run it before the
// kernels ever see a card — a union-find that spins would hang one.
//
//   cc_core_host THREADS < cases
// reads cases of the form
//   n_nodes n_items            (n_nodes = 0 ends the input)
//   key node                   n_items lines: the sorted keys with their nodes, as vfn_cc_union_runs takes them
// and prints per case one line: the status word, then root[0 .. n_nodes).  Thread t takes the items t, t + THREADS, ...: neighbouring
// items — the ones that meet on the same words of the forest — always run on different threads.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../vf_nerf_amd/csrc/vfn_cc_core.h"

struct HostMem {
    using word = std::atomic<int32_t>;
    static int load(const word* p) { return p->load(std::memory_order_relaxed); }
    static int cas(word* p, int expected, int desired) {
        int32_t e = expected;
        p->compare_exchange_strong(e, desired, std::memory_order_relaxed, std::memory_order_relaxed);
        return e;
    }
};

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 16;
    if (threads < 1 || threads > 256) { fprintf(stderr, "cc_core_host: THREADS outside [1, 256]\n"); return 2; }
    long long n_nodes, n_items;
    while (scanf("%lld %lld", &n_nodes, &n_items) == 2 && n_nodes > 0) {
        if (n_nodes >= (1ll << 31) || n_items < 0) { fprintf(stderr, "cc_core_host: bad counts\n"); return 2; }
        std::vector<long long> keys((size_t)n_items), nodes((size_t)n_items);
        for (long long i = 0; i < n_items; ++i)
            if (scanf("%lld %lld", &keys[(size_t)i], &nodes[(size_t)i]) != 2) { fprintf(stderr, "cc_core_host: short case\n"); return 2; }
        std::vector<std::atomic<int32_t>> parent((size_t)n_nodes);
        for (long long v = 0; v < n_nodes; ++v) parent[(size_t)v].store((int32_t)v, std::memory_order_relaxed);
        std::atomic<unsigned> status{0u};
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                unsigned mine = 0u;
                for (long long i = 1 + t; i < n_items; i += threads)
                    mine |= vfn_cc::union_item<HostMem>(keys.data(), nodes.data(), i, parent.data(), n_nodes);
                status.fetch_or(mine, std::memory_order_relaxed);
            });
        for (auto& th : pool) th.join();
        unsigned st = status.load();
        std::vector<int> root((size_t)n_nodes);
        for (long long v = 0; v < n_nodes; ++v) root[(size_t)v] = vfn_cc::chain_end<HostMem>(parent.data(), (int)v, &st);
        printf("%u", st);
        for (long long v = 0; v < n_nodes; ++v) printf(" %d", root[(size_t)v]);
        printf("\n");
    }
    return 0;
}
