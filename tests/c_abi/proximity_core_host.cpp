// proximity_core_host.cpp — the pair routine of csrc/vfn_proximity_core.h on the host: the SAME text that csrc/vfn_proximity.hip compiles
// for the device (seven candidates, the clamp into the triangle's box, the minimum of (d2, candidate)).  A stand-alone program: build
// it with the host compiler, -ffp-contract=off and -fsanitize=address,undefined, and run it before the kernel ever sees a card.
//
//   proximity_core_host < pairs
// reads the number of pairs, then per pair twelve numbers q A B C (as strtod reads them: hexadecimal floats, "inf", "nan"), and
// prints per pair "x y z d2": the closest point and the squared distance as the 16 hexadecimal digits of their bits.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../vf_nerf_amd/csrc/vfn_proximity_core.h"

static unsigned long long bits(double x) {
    unsigned long long u;
    memcpy(&u, &x, sizeof u);
    return u;
}

int main() {
    long long n;
    if (scanf("%lld", &n) != 1 || n < 0 || n > (1 << 24)) {
        fprintf(stderr, "proximity_core_host: bad count\n");
        return 2;
    }
    for (long long i = 0; i < n; ++i) {
        std::vector<double> in(12);                      // at its exact size: a read past an end is the sanitizer's
        for (double& x : in)
            if (scanf("%lf", &x) != 1) {
                fprintf(stderr, "proximity_core_host: pair %lld is short\n", i);
                return 2;
            }
        std::vector<double> c(3);
        double d2;
        vfn_proximity::closest_on_triangle(in.data(), in.data() + 3, in.data() + 6, in.data() + 9, c.data(), &d2);
        printf("%016llx %016llx %016llx %016llx\n", bits(c[0]), bits(c[1]), bits(c[2]), bits(d2));
    }
    return 0;
}
