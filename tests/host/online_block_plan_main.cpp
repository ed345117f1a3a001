// Stand-alone host program around the time-chunk planner of an online block (bayesloop_amd/csrc/blhip_online.hpp: blo::online_block_plan):
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/online_block_plan_main.cpp -o online_block_plan && ./online_block_plan
// Over a few grids, chain counts and numbers of history planes it sweeps the budget from one step's bytes to the whole block's and checks
// that the steps per chunk never fall as the budget grows, that the chunk fits, that one more step would not, that the chunks cover the
// block, that a budget below one step is refused with the floor reported, and that bad arguments are refused.  Last line
// "online block plan: ok" (exit 0) or the first violation (exit 1).
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../bayesloop_amd/csrc/blhip_online.hpp"

struct Shape { int ndim; int64_t n[4]; int64_t chains, planes, N; };

static int sweep(const Shape &s) {
    blo::BlockPlan whole;
    if (!blo::online_block_plan(s.ndim, s.n, s.chains, s.planes, s.N, 1e30, whole)) return 1;
    if (whole.steps != s.N || whole.n_chunks != 1) return 2;
    const double lo = (double)whole.min_budget_bytes, hi = (double)whole.chunk_bytes * 1.01;
    blo::BlockPlan P;
    if (blo::online_block_plan(s.ndim, s.n, s.chains, s.planes, s.N, lo - 1.0, P)) return 3;          // below one step: an error ...
    if (P.min_budget_bytes != whole.min_budget_bytes || P.steps != 0) return 4;                        // ... that names the floor
    int64_t last = 0;
    for (int k = 0; k <= 200; ++k) {
        const double budget = lo + (hi - lo) * k / 200.0;
        if (!blo::online_block_plan(s.ndim, s.n, s.chains, s.planes, s.N, budget, P)) return 5;
        if (P.steps < 1 || P.steps > s.N || P.steps < last) return 6;
        if ((double)P.chunk_bytes > budget) return 7;
        if (P.steps < s.N) {
            blo::BlockPlan more;
            if (!blo::online_block_plan(s.ndim, s.n, s.chains, s.planes, P.steps + 1, 1e30, more)) return 8;
            if (!((double)more.chunk_bytes > budget)) return 9;
        }
        if (P.n_chunks != (s.N + P.steps - 1) / P.steps) return 10;
        last = P.steps;
    }
    return last == s.N ? 0 : 11;
}

int main() {
    const Shape shapes[] = {
        {1, {1000, 0, 0, 0}, 64, 3, 1000}, {1, {200, 0, 0, 0}, 4, 0, 5}, {1, {4608, 0, 0, 0}, 33, 1, 7}, {2, {256, 256, 0, 0}, 32, 1, 256},
        {2, {64, 48, 0, 0}, 5, 4, 7}, {2, {20, 20, 0, 0}, 1, 1, 1}, {3, {5, 18, 14, 0}, 16, 4, 256}, {4, {3, 7, 5, 2}, 2, 3, 100000},
    };
    for (const Shape &s : shapes) {
        const int bad = sweep(s);
        std::printf("shape ndim %d n0 %lld chains %lld planes %lld N %lld -> %d\n", s.ndim, (long long)s.n[0], (long long)s.chains, (long long)s.planes,
                    (long long)s.N, bad);
        if (bad) { std::printf("violation %d\n", bad); return 1; }
    }
    blo::BlockPlan P;
    const int64_t n1[4] = {100, 0, 0, 0}, nbad[4] = {0, 0, 0, 0};
    if (blo::online_block_plan(0, n1, 1, 1, 1, 1e9, P) || blo::online_block_plan(5, n1, 1, 1, 1, 1e9, P) || blo::online_block_plan(1, nullptr, 1, 1, 1, 1e9, P) ||
        blo::online_block_plan(1, nbad, 1, 1, 1, 1e9, P) || blo::online_block_plan(1, n1, 0, 1, 1, 1e9, P) || blo::online_block_plan(1, n1, 1, -1, 1, 1e9, P) ||
        blo::online_block_plan(1, n1, 1, 1, 0, 1e9, P) || blo::online_block_plan(1, n1, 1, 1, 1, std::nan(""), P) || P.min_budget_bytes != 0) {
        std::printf("bad arguments accepted\n");
        return 1;
    }
    std::printf("online block plan: ok\n");
    return 0;
}
