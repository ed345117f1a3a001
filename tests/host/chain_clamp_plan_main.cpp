// Stand-alone host program around bayesloop_amd/csrc/blhip_chainclamp_plan.hpp: which batches take blc::chain_clamp_kernel (RegimeSwitch inside
// the chain-resident kernel on two-parameter grids) -- the envelope (blcp::chain_clamp_envelope) and the routing rule (blcp::chain_clamp_route):
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/chain_clamp_plan_main.cpp -o chain_clamp_plan && ./chain_clamp_plan
// Arguments: groups of 14 integers, the fields of blcp::ClampFacts
//     ndim gaussian_recurrence n0 n1 radius0 radius1 regime_switch_only composed restarts same_taps resumed carried backward_init cus
// Prints the constants, one line "facts <the 14 values> -> envelope (0 / 1) rows strips ring" per group, then the routing table
// "route option envelope chains strips steps passes cus -> 0 / 1" over a fixed list of batch shapes.
#include <cstdio>
#include <cstdlib>

#include "../../bayesloop_amd/csrc/blhip_chainclamp_plan.hpp"

int main(int argc, char **argv) {
    std::printf("ROWS_MIN %d ROWS_MAX %d COLS_MAX %d RADIUS_MAX %d STRIP_COLS %d VARIANT %d MIN_PASS_STEPS %lld\n", blcp::ROWS_MIN, blcp::ROWS_MAX, blcp::COLS_MAX,
                blcp::RADIUS_MAX, blcp::STRIP_COLS, blcp::VARIANT, blcp::MIN_PASS_STEPS);
    for (int k = 1; k + 13 < argc; k += 14) {
        int v[14];
        for (int q = 0; q < 14; ++q) v[q] = std::atoi(argv[k + q]);
        blcp::ClampFacts f;
        f.ndim = v[0]; f.gaussian_recurrence = v[1] != 0; f.n0 = v[2]; f.n1 = v[3]; f.radius0 = v[4]; f.radius1 = v[5];
        f.regime_switch_only = v[6] != 0; f.composed = v[7] != 0; f.restarts = v[8] != 0; f.same_taps = v[9] != 0;
        f.resumed = v[10] != 0; f.carried = v[11] != 0; f.backward_init = v[12] != 0; f.cus = v[13];
        std::printf("facts");
        for (int q = 0; q < 14; ++q) std::printf(" %d", v[q]);
        std::printf(" -> %d %d %d %d\n", blcp::chain_clamp_envelope(f) ? 1 : 0, blcp::clamp_rows(f.n0), blcp::clamp_strips(f.n1), blcp::clamp_ring(f.radius0));
    }
    struct Shape { long long chains; int strips; long long steps; int passes, cus; };
    const Shape shapes[] = {{1, 2, 6, 2, 256},     {1, 2, 6, 1, 256},    {1, 13, 1000, 2, 256}, {1, 13, 1000, 1, 256}, {1, 13, 2, 2, 256},  {1, 13, 3, 2, 256},   {1, 13, 4, 2, 256},
                            {1, 13, 4, 1, 256},    {1, 13, 7, 1, 256},   {1, 13, 8, 1, 256},    {64, 16, 256, 2, 256}, {17, 16, 256, 1, 256}, {64, 32, 256, 1, 256}, {9, 32, 4, 2, 256},
                            {3, 2, 3, 1, 256},     {200, 2, 16, 2, 256}, {1, 64, 100, 2, 256},  {1, 64, 100, 2, 32},   {0, 2, 100, 2, 256}};
    for (int o = 0; o < 3; ++o)
        for (int env = 0; env < 2; ++env)
            for (const Shape &h : shapes)
                std::printf("route %d %d %lld %d %lld %d %d %d\n", o, env, h.chains, h.strips, h.steps, h.passes, h.cus,
                            blcp::chain_clamp_route(o, env != 0, h.chains, h.strips, h.steps, h.passes, h.cus) ? 1 : 0);
    // ring lengths: radius 0 -> 4, 1 .. 8 -> 8, 9 .. 16 -> 12, .. 33 .. 40 -> 24, monotone
    int prev = 4;
    for (int r = 0; r <= blcp::RADIUS_MAX; ++r) {
        const int nk = blcp::clamp_ring(r);
        if (nk < prev || (nk != 4 && (nk % 4 != 0 || nk < 8 || nk > 24 || (4 * nk - 16) / 2 < r))) { std::printf("ring length %d for radius %d\n", nk, r); return 1; }
        prev = nk;
    }
    std::printf("rings ok\n");
    return 0;
}
