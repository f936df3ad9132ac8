// collapse_core_host.cpp — the per-edge routine of csrc/vfn_collapse_core.h on the host: the SAME text that csrc/vfn_collapse.hip compiles
// for the device (the sum of the two end quadrics, the adjugate solve, the fallback, the attribute parameter, the flip walk over both
// 1-rings through the item table).  A stand-alone program: build it with the host compiler, -ffp-contract=off and
// -fsanitize=address,undefined, and run it before the kernel ever sees a card — a walk that leaves its table would be caught here.
//
//   collapse_core_host < cases
// reads cases of the form
//   n m n_items rows n_edges                    (n = 0 ends the input)
//   ox oy oz rcond reach max_error              (numbers as strtod reads them: hexadecimal floats, "inf")
//   3 n coordinates, 3 m face indices, 10 n quadric numbers, n_items rows, n + 1 segment bounds
//   a b run                                     n_edges lines
// and prints per case the line "status n_edges", then per edge "flags cost s x y z": the flags in decimal, the doubles as the 16
// hexadecimal digits of their bits.  Every array is allocated at its exact size, so that a read past an end is the sanitizer's.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vf_nerf_amd/csrc/vfn_collapse_core.h"

static bool read_doubles(std::vector<double>& out) {
    for (double& x : out)
        if (scanf("%lf", &x) != 1) return false;
    return true;
}

static bool read_ints(std::vector<long long>& out) {
    for (long long& x : out)
        if (scanf("%lld", &x) != 1) return false;
    return true;
}

static unsigned long long bits(double x) {
    unsigned long long u;
    memcpy(&u, &x, sizeof u);
    return u;
}

int main() {
    long long n, m, n_items, rows, n_edges;
    while (scanf("%lld %lld %lld %lld %lld", &n, &m, &n_items, &rows, &n_edges) == 5 && n > 0) {
        if (m < 1 || n_items < 0 || rows < m || n_edges < 0 || n > (1 << 24) || m > (1 << 24) || n_items > (1 << 26) || n_edges > (1 << 26)) {
            fprintf(stderr, "collapse_core_host: bad counts\n");
            return 2;
        }
        std::vector<double> head(6), v((size_t)(3 * n)), q((size_t)(10 * n));
        std::vector<long long> f((size_t)(3 * m)), item_row((size_t)n_items), start((size_t)(n + 1)), edges((size_t)(3 * n_edges));
        if (!read_doubles(head) || !read_doubles(v) || !read_ints(f) || !read_doubles(q) || !read_ints(item_row) || !read_ints(start) ||
            !read_ints(edges)) {
            fprintf(stderr, "collapse_core_host: short case\n");
            return 2;
        }
        vfn_collapse::Mesh g;
        g.v = v.data(); g.n = n; g.f = f.data(); g.m = m; g.q = q.data(); g.item_row = item_row.data(); g.n_items = n_items;
        g.start = start.data(); g.rows = rows;
        g.o[0] = head[0]; g.o[1] = head[1]; g.o[2] = head[2];
        g.rcond = head[3]; g.reach = head[4]; g.max_error = head[5];
        unsigned status = 0;
        std::vector<vfn_collapse::Edge> out((size_t)n_edges);
        for (long long e = 0; e < n_edges; ++e)
            status |= vfn_collapse::edge(g, edges[(size_t)(3 * e)], edges[(size_t)(3 * e + 1)], edges[(size_t)(3 * e + 2)], &out[(size_t)e]);
        printf("%u %lld\n", status, n_edges);
        for (const vfn_collapse::Edge& r : out)
            printf("%u %016llx %016llx %016llx %016llx %016llx\n", (unsigned)r.flags, bits(r.cost), bits(r.s), bits(r.point[0]), bits(r.point[1]),
                   bits(r.point[2]));
    }
    return 0;
}
