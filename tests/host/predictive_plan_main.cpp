// Stand-alone host program around the plan of the posterior predictive (bayesloop_amd/csrc/blhip_predictive.hpp: blpp::predictive_plan):
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/predictive_plan_main.cpp -o predictive_plan && ./predictive_plan
// Arguments: groups of 5 numbers  G T X average budget  (budget 0: the smallest one the plan accepts, -k: that minus k bytes).
// Prints the constants, then one line per group
//     plan G T X average budget -> ok slab n_slabs rows_per_chunk n_chunks workspace_bytes min_budget_bytes off_out off_avg off_rows off_part
// and walks the slabs and chunks of every accepted plan the way the library's launches do: every cell in exactly one slab, every value in
// exactly one chunk, the places inside the workspace disjoint, in order and inside it.  Last line "covered" (exit 0) or the first violation
// (exit 1).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bayesloop_amd/csrc/blhip_predictive.hpp"

static int check(long long G, long long T, long long X, bool average, const blpp::PredPlan &P) {
    if (P.slab < blpp::SLAB_MIN || P.slab % blpp::KSTEP != 0 || P.n_slabs < 1 || P.n_slabs > blpp::SLABS_MAX) return 1;
    if (P.rows_per_chunk < 1 || P.rows_per_chunk > blpp::NXT * blpp::XT || P.rows_per_chunk > X) return 2;
    // cells: the slabs as contract_kernel walks them
    if (G <= (1ll << 22)) {
        std::vector<unsigned char> hit((size_t)G, 0);
        for (long long s = 0; s < P.n_slabs; ++s) {
            const long long lo = s * P.slab, hi = lo + P.slab < G ? lo + P.slab : G;
            if (lo >= hi) return 3;                          // an empty slab
            for (long long c = lo; c < hi; ++c) ++hit[(size_t)c];
        }
        for (long long c = 0; c < G; ++c)
            if (hit[(size_t)c] != 1) return 4;
    } else if ((P.n_slabs - 1) * P.slab >= G || P.n_slabs * P.slab < G) return 5;
    // values: the chunks as the entry point walks them
    std::vector<unsigned char> seen((size_t)X, 0);
    long long chunks = 0;
    for (long long c0 = 0; c0 < X; c0 += P.rows_per_chunk, ++chunks) {
        const long long xc = P.rows_per_chunk < X - c0 ? P.rows_per_chunk : X - c0;
        for (long long j = 0; j < xc; ++j) ++seen[(size_t)(c0 + j)];
    }
    if (chunks != P.n_chunks) return 6;
    for (long long j = 0; j < X; ++j)
        if (seen[(size_t)j] != 1) return 7;
    // the places inside the workspace
    const long long out_b = T * X * 8, avg_b = average ? G * 8 : 0, rows_b = P.rows_per_chunk * G * 8, part_b = P.n_slabs * T * P.rows_per_chunk * 8;
    if (P.off_out != 0 || P.off_avg < P.off_out + out_b || P.off_rows < P.off_avg + avg_b || P.off_part < P.off_rows + rows_b ||
        P.workspace_bytes < P.off_part + part_b)
        return 8;
    if (P.off_avg % 256 || P.off_rows % 256 || P.off_part % 256) return 9;
    return 0;
}

int main(int argc, char **argv) {
    std::printf("TM %d XT %d NXT %d RUN %d KSTEP %d SLAB_MIN %lld SLABS_MAX %lld\n", blpp::TM, blpp::XT, blpp::NXT, blpp::RUN, blpp::KSTEP, blpp::SLAB_MIN,
                blpp::SLABS_MAX);
    for (int k = 1; k + 4 < argc; k += 5) {
        const long long G = std::atoll(argv[k]), T = std::atoll(argv[k + 1]), X = std::atoll(argv[k + 2]);
        const bool average = std::atoi(argv[k + 3]) != 0;
        double budget = std::atof(argv[k + 4]);
        blpp::PredPlan P;
        if (budget <= 0.0) {
            blpp::predictive_plan(G, T, X, average, 0.0, P);
            budget = (double)P.min_budget_bytes + budget;
        }
        const bool ok = blpp::predictive_plan(G, T, X, average, budget, P);
        std::printf("plan %lld %lld %lld %d %.0f -> %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", G, T, X, average ? 1 : 0, budget, ok ? 1 : 0, P.slab, P.n_slabs,
                    P.rows_per_chunk, P.n_chunks, P.workspace_bytes, P.min_budget_bytes, P.off_out, P.off_avg, P.off_rows, P.off_part);
        if (ok) {
            if ((double)P.workspace_bytes > budget) { std::printf("workspace above the budget\n"); return 1; }
            const int bad = check(G, T, X, average, P);
            if (bad) { std::printf("violation %d\n", bad); return 1; }
        }
    }
    std::printf("covered\n");
    return 0;
}
