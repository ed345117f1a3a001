// Stand-alone host program around the host functions of bayesloop_amd/csrc/blhip_chain_nd.hpp: the LDS need of the chain-resident N-D
// kernel (bln::chain_nd_lds_doubles), the envelope it gives under the 150 KB the host allows a block (chain_nd_fits, chain_nd_max_cells),
// the block size (chain_nd_threads) and the routing predicate (chain_nd_route):
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/chain_nd_lds_main.cpp -o chain_nd_lds && ./chain_nd_lds 9408 47 2 167  9472 3 2 168
// Arguments: quadruples (cells, widest radius of the batch, walks of the program, sum of the axis lengths).  Prints the constants, one
// line per quadruple
//     G LW walks n_sum  doubles  fits (0 / 1)  threads  cells per thread held in registers  largest G admitted beside these taps and grid values
// then the routing table "route option envelope G chains walks W -> 0 / 1  kernel_us plain_us threads" (256 CUs; lw > 30: a radius beyond its axis) over the shapes the cost model was
// fitted to and their neighbours, and checks monotonicity in G and in the radius over a sweep: exit
// status 1 and a message if the need ever shrinks as either grows, or if the envelope re-admits a larger problem.
#include <cstdio>
#include <cstdlib>

#include "../../bayesloop_amd/csrc/blhip_chain_nd.hpp"

int main(int argc, char **argv) {
    std::printf("NT_SMALL %d NT_LARGE %d RED %d MAXPASS %d MIN_CHAINS %d LIMIT %zu SMALL_BYTES %zu\n", bln::CHAIN_ND_NT_SMALL, bln::CHAIN_ND_NT_LARGE,
                bln::CHAIN_ND_RED, bln::CHAIN_ND_MAXPASS, bln::CHAIN_ND_MIN_CHAINS, bln::CHAIN_ND_LDS_LIMIT, bln::CHAIN_ND_SMALL_BYTES);
    for (int k = 1; k + 3 < argc; k += 4) {
        const long long G = std::atoll(argv[k]), ns = std::atoll(argv[k + 3]);
        const int lw = std::atoi(argv[k + 1]), np = std::atoi(argv[k + 2]);
        const int nt = bln::chain_nd_threads(G, lw, np, ns);
        std::printf("%lld %d %d %lld %zu %d %d %d %lld\n", G, lw, np, ns, bln::chain_nd_lds_doubles(G, lw, np, ns), bln::chain_nd_fits(G, lw, np, ns) ? 1 : 0, nt,
                    bln::chain_nd_cpt(nt), bln::chain_nd_max_cells(lw, np, ns));
    }
    const int opts[] = {0, 1, 2};
    struct Shape { long long G, B; int walks, W, lw, ns; };
    const Shape shapes[] = {{1260, 1, 2, 14, 3, 37},   {1260, 8, 2, 14, 3, 37},    {1260, 15, 2, 14, 3, 37},  {1260, 16, 2, 14, 3, 37},  {1260, 64, 2, 14, 3, 37},
                            {1260, 512, 2, 14, 3, 37}, {1260, 5000, 2, 14, 3, 37}, {8000, 16, 2, 14, 3, 73},  {8000, 32, 2, 14, 3, 73},  {8000, 64, 2, 14, 3, 73},
                            {8000, 400, 2, 14, 3, 73}, {9408, 16, 2, 14, 3, 167},  {9408, 256, 2, 14, 3, 167}, {1260, 64, 2, 42, 17, 37}, {1260, 16, 1, 81, 40, 37},
                            {1260, 16, 0, 0, 0, 37},   {105, 16, 2, 28, 9, 15},    {4000, 16, 2, 14, 3, 53},  {5600, 16, 2, 14, 3, 61},  {9408, 16, 2, 102, 47, 167}};
    for (int o : opts)
        for (int env = 0; env < 2; ++env)
            for (const Shape &h : shapes) {
                const int nt = bln::chain_nd_threads(h.G, h.lw, 2, h.ns);
                std::printf("route %d %d %lld %lld %d %d %d %.3f %.3f %d\n", o, env, h.G, h.B, h.walks, h.W,
                            bln::chain_nd_route(o, env != 0, h.G, h.B, h.walks, h.W, h.lw > 30, nt, 256) ? 1 : 0, bln::chain_nd_kernel_us(h.G, h.B, h.W, nt, 256),
                            bln::chain_nd_plain_us(h.G, h.B, h.walks, h.W), nt);
            }
    // monotonicity: the need grows strictly with G, with the radius (one walk or more) and with the number of walks; once refused, every
    // larger problem is refused; every admitted grid has at most CPT cells per thread
    const int radii[] = {0, 1, 3, 17, 64, 540, 4000, 9600, 20000};
    const int walks[] = {0, 1, 2, 3, 8};
    for (int lw : radii)
        for (int np : walks) {
            bool refused = false;
            size_t prev = 0;
            for (long long G = 1; G <= 12000; ++G) {
                const long long ns = 3 + G / 64;
                const size_t need = bln::chain_nd_lds_doubles(G, lw, np, ns);
                if (need <= prev) { std::printf("not monotonic in G at G = %lld, radius %d\n", G, lw); return 1; }
                prev = need;
                const bool fits = bln::chain_nd_fits(G, lw, np, ns);
                if (fits && refused) { std::printf("re-admitted G = %lld, radius %d\n", G, lw); return 1; }
                if (fits != (G <= bln::chain_nd_max_cells(lw, np, ns))) { std::printf("max_cells disagrees at G = %lld, radius %d\n", G, lw); return 1; }
                const int nt = bln::chain_nd_threads(G, lw, np, ns);
                if (fits && G > (long long)nt * bln::chain_nd_cpt(nt)) { std::printf("G = %lld: more than CPT cells per thread\n", G); return 1; }
                if (np + 1 <= bln::CHAIN_ND_MAXPASS && bln::chain_nd_lds_doubles(G, lw, np + 1, ns) <= need) { std::printf("not monotonic in the walks\n"); return 1; }
                refused = refused || !fits;
            }
        }
    const long long cells[] = {1, 105, 378, 1260, 8000, 9408, 9472};
    for (long long G : cells) {
        size_t prev = 0;
        bool refused = false;
        for (int lw = 0; lw <= 12000; ++lw) {
            const size_t need = bln::chain_nd_lds_doubles(G, lw, 2, 40);
            if (need <= prev) { std::printf("not monotonic in the radius at G = %lld, radius %d\n", G, lw); return 1; }
            prev = need;
            const bool fits = bln::chain_nd_fits(G, lw, 2, 40);
            if (fits && refused) { std::printf("re-admitted G = %lld, radius %d\n", G, lw); return 1; }
            refused = refused || !fits;
        }
    }
    if (bln::chain_nd_fits(100, 1, bln::CHAIN_ND_MAXPASS + 1, 20)) { std::printf("more walks than the parameter block holds\n"); return 1; }
    std::printf("monotonic\n");
    return 0;
}
