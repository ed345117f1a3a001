// Stand-alone host program around bayesloop_amd/csrc/blhip_nd_program.hpp: what the program builder hands the stage flavour of the
// chain-resident N-D kernel (bln::chain_nd_stage_kernel) -- the kind of every pass, the per-chain limits, the widest walk and shift
// radius, the inputs of its cost model -- printed for one problem on a fixed grid: 3 x 4 x 5 cells, lattice constants (1, 0.5, 0.25),
// T = 5 steps with time stamps 0 .. 4 (tests/host/nd_program_main.cpp prints the fields that were there before, on the same grid).
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/nd_stage_program_main.cpp -o nd_stage_program && ./nd_stage_program 0 -1 2 1  6 0 -1 0  -3 -2
// Arguments: resume (0 / 1), resume_time, chains B, number of ops, then (kind axis segment flags) per op, then the B x n_ops op values.
// Prints "pass_kind" per pass, "kindF" / "kindB" as [t][b] (the source kinds: what the kernel loads by), "tapF q" / "tapB q" per pass as
// [t][b], "limit q" per pass as [b], the radius of every tap set, then "stage lw_walk_max .. lw_shift_max .. launches .. W .. filters ..
// sweeps .. shifts .. beyond_axis ..", or "refused <message>".
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
    if (B < 1 || n_ops < 0 || argc != 5 + 4 * n_ops + (int)B * n_ops) { std::fprintf(stderr, "bad argument count\n"); return 2; }
    std::vector<blhip_op> ops(n_ops);
    for (int k = 0; k < n_ops; ++k) {
        ops[k] = blhip_op{};
        ops[k].kind = std::atoi(argv[5 + 4 * k]); ops[k].axis = std::atoi(argv[6 + 4 * k]);
        ops[k].segment = std::atoi(argv[7 + 4 * k]); ops[k].flags = std::atoi(argv[8 + 4 * k]);
    }
    std::vector<double> val((size_t)B * n_ops);
    for (size_t k = 0; k < val.size(); ++k) val[k] = std::strtod(argv[5 + 4 * n_ops + k], nullptr);
    double stamps[5] = {0.0, 1.0, 2.0, 3.0, 4.0};
    blhip_problem p{};
    p.ndim = 3; p.n[0] = 3; p.n[1] = 4; p.n[2] = 5;
    p.lattice[0] = 1.0; p.lattice[1] = 0.5; p.lattice[2] = 0.25;
    p.T = 5; p.timestamps = stamps; p.resume_time = std::strtod(argv[2], nullptr);
    p.n_ops = n_ops; p.ops = ops.data();
    const double dV = p.lattice[0] * p.lattice[1] * p.lattice[2];

    const NdFacts F = nd_facts(&p);
    row("pass_kind", -1, F.pass_kind.data(), F.pass_kind.size(), "%d");
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
    for (size_t k = 0; k < nT; ++k) kinds[k] = P.kindF[k];
    row("kindF", -1, kinds.data(), nT, "%d");
    for (size_t k = 0; k < nT; ++k) kinds[k] = P.kindB[k];
    row("kindB", -1, kinds.data(), nT, "%d");
    for (int q = 0; q < F.npass; ++q) { row("tapF", q, &P.tapF[(size_t)q * nT], nT, "%d"); row("tapB", q, &P.tapB[(size_t)q * nT], nT, "%d"); }
    for (int q = 0; q < F.npass && !P.limit.empty(); ++q) row("limit", q, &P.limit[(size_t)q * B], (size_t)B, "%.17g");
    row("tap_lw", -1, P.taps.lw.data(), P.taps.lw.size(), "%d");
    std::printf("stage lw_walk_max %d lw_shift_max %d launches %d W %d filters %d sweeps %d shifts %d beyond_axis %d\n", P.lw_walk_max, P.lw_shift_max,
                P.stage_launches, P.stage_W, P.stage_filters, P.stage_sweeps, P.stage_shifts, P.stage_beyond_axis ? 1 : 0);
    return 0;
}
