// Stand-alone host program around bayesloop_amd/csrc/blhip_series.hpp for the admission rule and the memory plan of series fits in groups
// (blhip_set_series_groups; HyperStudy.fitMany): S series x H chains on a one-parameter grid.  It launches nothing and runs on a CPU.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/series_group_main.cpp -o series_group
//     ./series_group T n H S evidence_only budget cap [ndim]
// prints ONE line:
//     check <rc> | plan <rc> groups <g> batches <b> bytes <bytes> least <least> chain <series_chain_bytes> | <reason of a refusal>
// and, for H = 1, a second one with blhip_host_series_plan's figures:
//     series_plan <rc> <per> <batches> <bytes> <least>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/blhip.h"
#include "../../bayesloop_amd/csrc/blhip_kernels.hpp"
#include "../../bayesloop_amd/csrc/blhip_err.hpp"
#include "../../bayesloop_amd/csrc/blhip_bigshift.hpp"
#include "../../bayesloop_amd/csrc/blhip_chainres.hpp"
#include "../../bayesloop_amd/csrc/blhip_chainclamp_plan.hpp"
#include "../../bayesloop_amd/csrc/blhip_fused1d.hpp"
#include "../../bayesloop_amd/csrc/blhip_chain1d.hpp"

using namespace blk;
using blerr::fail;

namespace {
#include "../../bayesloop_amd/csrc/blhip_program.hpp"
// (what the library's launch tables define in front of the header: tests/test_chain_plan_host.py holds these two to blhip_launch.hpp's text)
constexpr int FAST_R0_MAX = 40;
bool fold2_shape(int ntw) { return ntw >= 1 && ntw <= 4; }
#include "../../bayesloop_amd/csrc/blhip_chain_plan.hpp"
#include "../../bayesloop_amd/csrc/blhip_series.hpp"
}   // namespace

int main(int argc, char **argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: series_group T n H S evidence_only budget cap [ndim]\n"); return 2; }
    const long long T = std::atoll(argv[1]), n = std::atoll(argv[2]), H = std::atoll(argv[3]), S = std::atoll(argv[4]);
    // (a fit that keeps posteriors folds its groups: BLHIP_ACCUMULATE, which a fit of single chains -- H = 1 -- does not take)
    const int flags = std::atoi(argv[5]) ? BLHIP_EVIDENCE_ONLY : (BLHIP_KEEP_POSTERIOR | (H > 1 ? BLHIP_ACCUMULATE : 0));
    const double budget = std::atof(argv[6]);
    const long long cap = std::atoll(argv[7]);
    const int ndim = argc > 8 ? std::atoi(argv[8]) : 1;
    std::vector<double> m((size_t)n), data((size_t)T, 1.0), ts((size_t)T, 0.0), prior((size_t)n, 1.0 / (double)n);
    for (long long j = 0; j < n; ++j) m[(size_t)j] = 0.1 + 0.01 * (double)j;
    blhip_op op{};
    op.kind = BLHIP_OP_GRW; op.axis = 0; op.segment = -1;
    blhip_problem p{};
    p.ndim = ndim; p.obs_model = ndim == 1 ? BLHIP_OM_POISSON : BLHIP_OM_GAUSSIAN; p.T = T; p.seg_len = 1; p.data_dim = 1;
    for (int k = 0; k < ndim; ++k) { p.n[k] = n; p.marginal[k] = m.data(); p.lattice[k] = 0.01; }
    p.data = data.data(); p.timestamps = ts.data(); p.prior = prior.data();
    p.n_ops = 1; p.ops = &op;
    char why[256] = "", why2[256] = "";
    const int rc_check = series_group_check(&p, S, H, flags, why, (int)sizeof why);
    int64_t out[4] = {0, 0, 0, 0};
    const int rc_plan = series_group_plan(&p, S, H, flags, budget, cap, out, why2, (int)sizeof why2);
    std::printf("check %d | plan %d groups %lld batches %lld bytes %lld least %lld chain %.0f | %s\n", rc_check, rc_plan, (long long)out[0],
                (long long)out[1], (long long)out[2], (long long)out[3], ndim == 1 ? series_chain_bytes(&p, p.obs_model, (flags & BLHIP_EVIDENCE_ONLY) != 0) : 0.0,
                rc_check ? why : why2);
    if (H == 1) {
        int64_t o1[4] = {0, 0, 0, 0};
        const int rc1 = series_plan(&p, S, flags & ~BLHIP_ACCUMULATE, budget, o1);
        std::printf("series_plan %d %lld %lld %lld %lld\n", rc1, (long long)o1[0], (long long)o1[1], (long long)o1[2], (long long)o1[3]);
    }
    return 0;
}
