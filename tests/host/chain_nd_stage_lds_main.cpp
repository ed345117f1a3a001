// Stand-alone host program around the host functions of the stage flavour of the chain-resident N-D kernel
// (bayesloop_amd/csrc/blhip_chain_nd.hpp): the doubles of a tap slot (bln::chain_nd_stage_slot), the LDS need
// (chain_nd_stage_lds_doubles), the envelope under the 150 KB the host allows a block (chain_nd_stage_fits, chain_nd_stage_max_cells), the
// block size (chain_nd_stage_threads) and the routing predicate (chain_nd_stage_route):
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/chain_nd_stage_lds_main.cpp -o chain_nd_stage_lds && ./chain_nd_stage_lds 1260 3 37 2 37
// Arguments: quintuples (cells, widest walk radius, widest shift radius, passes of the program, sum of the axis lengths).  Prints the
// constants, one line per quintuple
//     G lw_walk lw_shift passes n_sum  slot doubles  fits (0 / 1)  threads  cells per thread held in registers  largest G admitted
// then the routing table "route chain_nd chain_nd_stages envelope G chains filters W sweeps shifts -> 0 / 1  kernel_us plain_us threads"
// (256 CUs), and checks over a sweep that the need grows with the cells, the radii and the passes, that the envelope never re-admits a
// larger problem, and that an admitted grid has at most CPT cells per thread: exit status 1 and a message otherwise.
#include <cstdio>
#include <cstdlib>

#include "../../bayesloop_amd/csrc/blhip_chain_nd.hpp"

int main(int argc, char **argv) {
    std::printf("NT_SMALL %d NT_LARGE %d RED %d MAXPASS %d MIN_CHAINS %d LIMIT %zu SMALL_BYTES %zu MEASURED %d WALK %d NOTEQUAL %d SHIFT %d\n",
                bln::CHAIN_ND_NT_SMALL, bln::CHAIN_ND_NT_LARGE, bln::CHAIN_ND_RED, bln::CHAIN_ND_MAXPASS, bln::CHAIN_ND_MIN_CHAINS, bln::CHAIN_ND_LDS_LIMIT,
                bln::CHAIN_ND_SMALL_BYTES, bln::CHAIN_ND_STAGE_MEASURED ? 1 : 0, (int)bln::CHAIN_ND_WALK, (int)bln::CHAIN_ND_NOTEQUAL, (int)bln::CHAIN_ND_SHIFT);
    for (int k = 1; k + 4 < argc; k += 5) {
        const long long G = std::atoll(argv[k]), ns = std::atoll(argv[k + 4]);
        const int lww = std::atoi(argv[k + 1]), lws = std::atoi(argv[k + 2]), np = std::atoi(argv[k + 3]);
        const int slot = bln::chain_nd_stage_slot(lww, lws);
        const int nt = bln::chain_nd_stage_threads(G, slot, np, ns);
        std::printf("%lld %d %d %d %lld %d %zu %d %d %d %lld\n", G, lww, lws, np, ns, slot, bln::chain_nd_stage_lds_doubles(G, slot, np, ns),
                    bln::chain_nd_stage_fits(G, slot, np, ns) ? 1 : 0, nt, bln::chain_nd_cpt(nt), bln::chain_nd_stage_max_cells(slot, np, ns));
    }
    struct Shape { long long G, B; int filters, W, sweeps, shifts, slot, np, ns; };
    // NotEqual alone; walk (radius 3) + NotEqual; a shift of ~3 cells (radius 38); a resumed batch of two walks; no pass at all
    const Shape shapes[] = {{1260, 1, 0, 0, 3, 0, 1, 1, 37},    {1260, 15, 0, 0, 3, 0, 1, 1, 37},   {1260, 16, 0, 0, 3, 0, 1, 1, 37},  {1260, 256, 0, 0, 3, 0, 1, 1, 37},
                            {2160, 16, 0, 0, 3, 0, 1, 1, 47},   {8000, 16, 0, 0, 3, 0, 1, 1, 67},   {8000, 64, 0, 0, 3, 0, 1, 1, 67},  {1260, 16, 1, 7, 3, 0, 4, 2, 37},
                            {2160, 64, 1, 7, 3, 0, 4, 2, 47},   {8000, 16, 1, 7, 3, 0, 4, 2, 67},   {8000, 64, 1, 7, 3, 0, 4, 2, 67},  {8000, 256, 1, 7, 3, 0, 4, 2, 67},
                            {1260, 16, 1, 77, 1, 1, 77, 1, 37}, {1260, 256, 1, 77, 1, 1, 77, 1, 37}, {2160, 64, 1, 77, 1, 1, 77, 1, 47}, {8000, 256, 1, 77, 1, 1, 77, 1, 67},
                            {1260, 16, 2, 14, 0, 0, 4, 2, 37},  {1260, 16, 0, 0, 0, 0, 1, 0, 37},   {105, 16, 1, 75, 4, 1, 75, 2, 15},  {1260, 5000, 1, 7, 3, 0, 4, 2, 37}};
    for (int o = 0; o < 3; ++o)
        for (int so = 0; so < 2; ++so)
            for (int env = 0; env < 2; ++env)
                for (const Shape &h : shapes) {
                    const int nt = bln::chain_nd_stage_threads(h.G, h.slot, h.np, h.ns);
                    std::printf("route %d %d %d %lld %lld %d %d %d %d %d %.3f %.3f %d\n", o, so, env, h.G, h.B, h.filters, h.W, h.sweeps, h.shifts,
                                bln::chain_nd_stage_route(o, so, env != 0, h.G, h.B, h.filters, h.W, h.sweeps, h.shifts, false, nt, 256) ? 1 : 0,
                                bln::chain_nd_stage_kernel_us(h.G, h.B, h.W, h.sweeps, nt, 256), bln::chain_nd_stage_plain_us(h.G, h.B, h.filters, h.W, h.sweeps, h.shifts), nt);
                }
    // the slot: a walk's half kernel or a shift's whole stencil, whichever is wider; never below one double
    const int radii[] = {0, 1, 3, 17, 46, 64, 540, 4000};
    for (int lww : radii)
        for (int lws : radii) {
            const int slot = bln::chain_nd_stage_slot(lww, lws);
            if (slot < lww + 1 || (lws > 0 && slot < 2 * lws + 1) || slot < 1 || (slot != lww + 1 && slot != 2 * lws + 1)) {
                std::printf("slot %d for radii %d, %d\n", slot, lww, lws);
                return 1;
            }
        }
    const int slots[] = {1, 4, 18, 69, 93, 541, 4001, 9600, 20000};
    const int passes[] = {0, 1, 2, 3, 8};
    for (int slot : slots)
        for (int np : passes) {
            bool refused = false;
            size_t prev = 0;
            for (long long G = 1; G <= 12000; ++G) {
                const long long ns = 3 + G / 64;
                const size_t need = bln::chain_nd_stage_lds_doubles(G, slot, np, ns);
                if (need <= prev) { std::printf("not monotonic in G at G = %lld, slot %d\n", G, slot); return 1; }
                prev = need;
                const bool fits = bln::chain_nd_stage_fits(G, slot, np, ns);
                if (fits && refused) { std::printf("re-admitted G = %lld, slot %d\n", G, slot); return 1; }
                if (fits != (G <= bln::chain_nd_stage_max_cells(slot, np, ns))) { std::printf("max_cells disagrees at G = %lld, slot %d\n", G, slot); return 1; }
                const int nt = bln::chain_nd_stage_threads(G, slot, np, ns);
                if (fits && G > (long long)nt * bln::chain_nd_cpt(nt)) { std::printf("G = %lld: more than CPT cells per thread\n", G); return 1; }
                if (np + 1 <= bln::CHAIN_ND_MAXPASS && bln::chain_nd_stage_lds_doubles(G, slot, np + 1, ns) <= need) { std::printf("not monotonic in the passes\n"); return 1; }
                if (bln::chain_nd_stage_lds_doubles(G, slot + 1, np, ns) < need || (np > 0 && bln::chain_nd_stage_lds_doubles(G, slot + 1, np, ns) == need)) {
                    std::printf("not monotonic in the slot\n");
                    return 1;
                }
                refused = refused || !fits;
            }
        }
    if (bln::chain_nd_stage_fits(100, 4, bln::CHAIN_ND_MAXPASS + 1, 20)) { std::printf("more passes than the parameter block holds\n"); return 1; }
    // a program of walks alone needs what chain_nd_lds_doubles says: a resumed batch of walks fits wherever the same batch fits unresumed
    for (int lw = 0; lw <= 60; ++lw)
        for (int np = 0; np <= bln::CHAIN_ND_MAXPASS; ++np)
            if (bln::chain_nd_stage_lds_doubles(1260, bln::chain_nd_stage_slot(lw, 0), np, 37) != bln::chain_nd_lds_doubles(1260, lw, np, 37)) {
                std::printf("walks alone: the two needs differ at radius %d\n", lw);
                return 1;
            }
    std::printf("monotonic\n");
    return 0;
}
