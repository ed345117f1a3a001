// Stand-alone host program around bl1c::lds_doubles / bl1c::lds_doubles_long (bayesloop_amd/csrc/blhip_chain1d.hpp), the LDS footprints the
// selector (plan_geometry) and the launchers of the chain-resident 1-D kernels size a block by:
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/chain1d_lds_main.cpp -o chain1d_lds && ./chain1d_lds 8192 540 0  6163 46 1
// Arguments: triples (cells, radius, 0 / 1 = with the shift flavour's coefficient row).  Prints one line per triple:
//     n LW shift  doubles of the standard layout  doubles of the long-row layout
// and, first, the constants the envelope is made of.
#include <cstdio>
#include <cstdlib>

#include "../../bayesloop_amd/csrc/blhip_chain1d.hpp"

int main(int argc, char **argv) {
    std::printf("NT %d NMAX %d NMAX_LONG %d CPT_LONG %d\n", bl1c::NT, bl1c::NMAX, bl1c::NMAX_LONG, bl1c::CPT_LONG);
    for (int k = 1; k + 2 < argc; k += 3) {
        const int n = std::atoi(argv[k]), lw = std::atoi(argv[k + 1]);
        const bool shift = std::atoi(argv[k + 2]) != 0;
        std::printf("%d %d %d %zu %zu\n", n, lw, shift ? 1 : 0, bl1c::lds_doubles(n, lw, shift), bl1c::lds_doubles_long(n, lw, shift));
    }
    return 0;
}
