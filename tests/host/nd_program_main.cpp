// Stand-alone host program around bayesloop_amd/csrc/blhip_nd_program.hpp: the transition program of a batch on grids with 3 and 4
// parameters -- which source every (step, chain) consumes and which tap set every pass of every chain filters with -- printed for one
// problem on a fixed grid: 3 x 4 x 5 cells, lattice constants (1, 0.5, 0.25), T = 5 steps with time stamps 0 .. 4.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/nd_program_main.cpp -o nd_program && ./nd_program 0 -1 2 1  1 1 -1 0  0.5 0
// Arguments: resume (0 / 1), resume_time, chains B, number of ops, then (kind axis segment flags) per op, then the B x n_ops op values,
// then, optionally, five time stamps in place of 0 .. 4.
// Prints the per-call facts, then "refused <message>" if the shifts or the builder refuse the problem, else the arrays of NdBatchProgram:
// kindF / kindB / stepKF / stepKB as [t][b], "tapF q" / "tapB q" per pass (one row also without passes) as [t][b], "limit q" per pass as [b], the radius of every tap
// set, lw_max, the cost-model inputs and the number of zero doubles the tap weights end in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/blhip.h"
#include "../../bayesloop_amd/csrc/blhip_kernels.hpp"
#include "../../bayesloop_amd/csrc/blhip_err.hpp"

using namespace blk;
using blerr::fail;

namespace {
#include "../../bayesloop_amd/csrc/blhip_taps.hpp"
#include "../../bayesloop_amd/csrc/blhip_nd_program.hpp"

template <class V> void row(const char *name, int q, const V *v, size_t n, const char *fmt) {
    std::printf(q < 0 ? "%s" : "%s %d", name, q);
    for (size_t k = 0; k < n; ++k) { std::printf(" "); std::printf(fmt, v[k]); }
    std::printf("\n");
}
}   // namespace

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: resume resume_time B n_ops (kind axis segment flags) x n_ops, values x B n_ops\n"); return 2; }
    const bool resume = std::atoi(argv[1]) != 0;
    const int64_t B = std::atoll(argv[3]);
    const int n_ops = std::atoi(argv[4]);
    const int n_args = 5 + 4 * n_ops + (int)B * n_ops;
    if (B < 1 || n_ops < 0 || (argc != n_args && argc != n_args + 5)) { std::fprintf(stderr, "bad argument count\n"); return 2; }
    std::vector<blhip_op> ops(n_ops);
    for (int k = 0; k < n_ops; ++k) {
        ops[k] = blhip_op{};
        ops[k].kind = std::atoi(argv[5 + 4 * k]); ops[k].axis = std::atoi(argv[6 + 4 * k]);
        ops[k].segment = std::atoi(argv[7 + 4 * k]); ops[k].flags = std::atoi(argv[8 + 4 * k]);
    }
    std::vector<double> val((size_t)B * n_ops);
    for (size_t k = 0; k < val.size(); ++k) val[k] = std::strtod(argv[5 + 4 * n_ops + k], nullptr);      // ("nan" parses as NaN)
    double stamps[5] = {0.0, 1.0, 2.0, 3.0, 4.0};
    for (int t = 0; t < 5 && argc == n_args + 5; ++t) stamps[t] = std::strtod(argv[n_args + t], nullptr);
    blhip_problem p{};
    p.ndim = 3; p.n[0] = 3; p.n[1] = 4; p.n[2] = 5;
    p.lattice[0] = 1.0; p.lattice[1] = 0.5; p.lattice[2] = 0.25;
    p.T = 5; p.timestamps = stamps; p.resume_time = std::strtod(argv[2], nullptr);
    p.n_ops = n_ops; p.ops = ops.data();
    const double dV = p.lattice[0] * p.lattice[1] * p.lattice[2];

    const NdFacts F = nd_facts(&p);
    std::printf("facts npass %d time_dependent %d has_stage %d has_shift %d n_sum %lld\n", F.npass, F.time_dependent ? 1 : 0, F.has_stage ? 1 : 0,
                F.has_shift ? 1 : 0, F.n_sum);
    row("pass_ops", -1, F.pass_ops.data(), F.pass_ops.size(), "%d");
    NdBatchProgram P;
    try {
        nd_refuse_shifts(&p, F, B, val.data(), resume);
        build_nd_program(&p, F, 0, B, val.data(), resume, dV, P);
    } catch (const blerr::Fail &e) {
        std::printf("refused %s\n", e.msg.c_str());
        return 0;
    }
    const size_t nT = (size_t)p.T * B;
    std::vector<int> kinds(nT);
    auto kind_row = [&](const char *name, const std::vector<unsigned char> &v) {
        if (v.empty()) return;
        for (size_t k = 0; k < nT; ++k) kinds[k] = v[k];
        row(name, -1, kinds.data(), nT, "%d");
    };
    kind_row("kindF", P.kindF); kind_row("kindB", P.kindB); kind_row("stepKF", P.stepKF); kind_row("stepKB", P.stepKB);
    std::printf("tap_entries %zu %zu\n", P.tapF.size(), P.tapB.size());
    for (int q = 0; q < std::max(1, F.npass); ++q) { row("tapF", q, &P.tapF[(size_t)q * nT], nT, "%d"); row("tapB", q, &P.tapB[(size_t)q * nT], nT, "%d"); }
    for (int q = 0; q < F.npass && !P.limit.empty(); ++q) row("limit", q, &P.limit[(size_t)q * B], (size_t)B, "%.17g");
    row("tap_lw", -1, P.taps.lw.data(), P.taps.lw.size(), "%d");
    row("tap_lw2", -1, P.taps.lw2.data(), P.taps.lw2.size(), "%d");
    row("tap_off", -1, P.taps.off.data(), P.taps.off.size(), "%d");
    int zeros = 0;
    while (zeros < (int)P.taps.w.size() && P.taps.w[P.taps.w.size() - 1 - zeros] == 0.0) ++zeros;
    std::printf("weights %zu trailing_zeros %d\n", P.taps.w.size(), zeros);
    std::printf("lw_max %d\n", P.lw_max);
    std::printf("cost walks_on %d W_taps %d beyond_axis %d\n", P.walks_on, P.W_taps, P.beyond_axis ? 1 : 0);
    return 0;
}
