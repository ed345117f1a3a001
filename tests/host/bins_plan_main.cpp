// Stand-alone host program around bayesloop_amd/csrc/blhip_bins.hpp: the host-only part of the distribution queries at many time steps -- the
// check of a map, its per-slab order (the permutation, the groups, the runs) and the chunk plan.  It launches nothing and runs on a CPU.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/bins_plan_main.cpp -o bins_plan && ./bins_plan order MAP.i32 N_BINS SLAB GW
// Commands (one per run):
//   check MAP.i32 N_BINS                   MAP.i32: the map as raw int32, one per cell  -> "check 0" or "check -1 MESSAGE"
//   order MAP.i32 N_BINS SLAB GW_MAX [ROWS.f64]
//                                          -> "order G n_bins slab n_slabs gw n_runs n_groups n_multi max_slots cells_in table_bytes"
//                                             per slab   "slab K GROUPS MULTI"
//                                             per group  "group K G DST C0 C1 .. C(gw-1)"   DST: r<run> (its only group) or s<slot>; C: the
//                                                        cell (global index) of every place, -1 = padding
//                                             per run of several groups  "multi RUN SLOT0 GROUPS"
//                                             per bin    "bin B RUN RUN .."   its runs, in the order they are added
//                                             with ROWS.f64 (raw float64, whole rows of G): per row "sums S HEX HEX .." -- the row added per
//                                             bin in the order the kernels add (ordered_sums), as hexadecimal floats
//   shape SLAB SB GW                       -> "shape slab sb gw_max"   what a call runs with when these are asked for
//   plan N_BINS N_RUNS TABLE_BYTES N_STEPS SB BUDGET
//                                          -> "plan OK steps_per_chunk n_chunks workspace_bytes min_budget_bytes off_steps off_part off_out"
//                                             OK: 1, or 0 for a refusal (bad arguments: min_budget_bytes 0)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bayesloop_amd/csrc/blhip_bins.hpp"

namespace {

template <class T> std::vector<T> read_file(const char *path) {
    std::vector<T> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    T buf[4096];
    size_t n;
    while ((n = std::fread(buf, sizeof(T), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

int usage() {
    std::fprintf(stderr, "usage: bins_plan check|order|shape|plan ... (see the head of tests/host/bins_plan_main.cpp)\n");
    return 2;
}

}   // namespace

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    if (cmd == "check" && argc == 4) {
        const std::vector<int32_t> map = read_file<int32_t>(argv[2]);
        char err[256] = "";
        const int rc = blb::check_bins(map.empty() ? nullptr : map.data(), (int64_t)map.size(), std::atoll(argv[3]), err, (int)sizeof err);
        std::printf("check %d %s\n", rc, err);
        return 0;
    }
    if (cmd == "shape" && argc == 5) {
        const blb::Shape s = blb::shape(std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]));
        std::printf("shape %lld %d %d\n", s.slab, s.sb, s.gw_max);
        return 0;
    }
    if (cmd == "plan" && argc == 8) {
        blb::BinsPlan P;
        const bool ok = blb::bins_plan(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), std::atoi(argv[6]), std::atof(argv[7]), P);
        std::printf("plan %d %lld %lld %lld %lld %lld %lld %lld\n", ok ? 1 : 0, P.steps_per_chunk, P.n_chunks, P.workspace_bytes, P.min_budget_bytes, P.off_steps,
                    P.off_part, P.off_out);
        return 0;
    }
    if (cmd == "order" && (argc == 6 || argc == 7)) {
        const std::vector<int32_t> map = read_file<int32_t>(argv[2]);
        const long long G = (long long)map.size(), n_bins = std::atoll(argv[3]), slab = std::atoll(argv[4]);
        char err[256] = "";
        if (blb::check_bins(map.empty() ? nullptr : map.data(), G, n_bins, err, (int)sizeof err) != 0) { std::printf("check -1 %s\n", err); return 1; }
        blb::Order O;
        if (!blb::order(map.data(), G, n_bins, slab, std::atoi(argv[5]), O)) { std::printf("order refused\n"); return 1; }
        std::printf("order %lld %lld %lld %lld %d %lld %lld %lld %lld %lld %lld\n", O.G, O.n_bins, O.slab, O.n_slabs, O.gw, O.n_runs, O.n_groups, O.n_multi, O.max_slots,
                    O.cells_in, O.table_bytes());
        const long long *goff = O.slabs.data(), *moff = O.slabs.data() + O.n_slabs + 1;
        const int32_t *perm = O.tab.data() + O.off_perm, *gdst = O.tab.data() + O.off_gdst, *multi = O.tab.data() + O.off_multi;
        const int32_t *bin_ptr = O.tab.data() + O.off_binptr, *bin_runs = O.tab.data() + O.off_binruns;
        for (long long k = 0; k < O.n_slabs; ++k) {
            const long long ng = goff[k + 1] - goff[k];
            std::printf("slab %lld %lld %lld\n", k, ng, moff[k + 1] - moff[k]);
            for (long long g = 0; g < ng; ++g) {
                const int32_t d = gdst[goff[k] + g];
                std::printf("group %lld %lld %c%d", k, g, d >= 0 ? 'r' : 's', d >= 0 ? d : -1 - d);
                for (int j = 0; j < O.gw; ++j) {
                    const int32_t c = perm[goff[k] * O.gw + j * ng + g];
                    std::printf(" %lld", c == O.slab ? -1ll : k * O.slab + c);
                }
                std::printf("\n");
            }
            for (long long q = moff[k]; q < moff[k + 1]; ++q) std::printf("multi %d %d %d\n", multi[3 * q], multi[3 * q + 1], multi[3 * q + 2]);
        }
        for (long long b = 0; b < n_bins; ++b) {
            std::printf("bin %lld", b);
            for (int32_t i = bin_ptr[b]; i < bin_ptr[b + 1]; ++i) std::printf(" %d", bin_runs[i]);
            std::printf("\n");
        }
        if (argc == 7) {
            const std::vector<double> rows = read_file<double>(argv[6]);
            const long long n_rows = (long long)rows.size() / G;
            std::vector<double> out((size_t)(n_rows * n_bins));
            blb::ordered_sums(O, rows.data(), n_rows, out.data());
            for (long long s = 0; s < n_rows; ++s) {
                std::printf("sums %lld", s);
                for (long long b = 0; b < n_bins; ++b) std::printf(" %a", out[(size_t)(s * n_bins + b)]);
                std::printf("\n");
            }
        }
        return 0;
    }
    return usage();
}
