// Stand-alone host program around bayesloop_amd/csrc/blhip_chain_plan.hpp for the two planning rules a series fit on a two-parameter grid
// (blhip_set_series; Study.fitMany) depends on.  It launches nothing and runs on a CPU.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/series_route_main.cpp -o series_route && ./series_route
//   1. chain_prefix_plan: the chains of a change-point batch of a hyper-study are identical up to their first restart, and all but one leave
//      that prefix to the providing chain.  The chains of a series batch observe their OWN data: ChainFacts::series keeps every prefix.
//      Printed for three no-stencil chains that restart at step 3 of 6, as "prefix <hyper|series> <evidence_only|fused>: share S skip K saved N".
//   2. series_route_refusal: only blc::chain_kernel / blc::chainax_kernel read per-chain data; a series batch on any other route has to
//      fail.  Printed as "route <what>: runs" or "route <what>: fails: <reason>".
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

using namespace blk;
using blerr::fail;

namespace {
#include "../../bayesloop_amd/csrc/blhip_program.hpp"
// (what the library's launch tables define in front of the header: tests/test_chain_plan_host.py holds these two to blhip_launch.hpp's text)
constexpr int FAST_R0_MAX = 40;
bool fold2_shape(int ntw) { return ntw >= 1 && ntw <= 4; }
#include "../../bayesloop_amd/csrc/blhip_chain_plan.hpp"

void prefix(const char *who, const char *fit, bool series, bool evidence_only, bool fused) {
    const int64_t T = 6, B = 3;
    const size_t nT = (size_t)T * B;
    ChainProgram prog;
    TapTable taps;
    prog.kindF.assign(nT, SRC_PREV); prog.kindB.assign(nT, SRC_PREV);
    prog.cmodeF.assign(nT, 0); prog.cmodeB.assign(nT, 0);
    prog.limitF.assign(nT, 0.0); prog.limitB.assign(nT, 0.0);
    prog.tapF0.assign(nT, -1); prog.tapF1.assign(nT, -1); prog.tapB0.assign(nT, -1); prog.tapB1.assign(nT, -1);
    for (int64_t b = 0; b < B; ++b) {
        prog.kindF[b] = SRC_PRIOR;
        prog.kindF[(size_t)3 * B + b] = SRC_RESET;
        prog.kindB[(size_t)2 * B + b] = SRC_RESET;
        prog.kindB[(size_t)(T - 1) * B + b] = SRC_UNIFORM;
    }
    Geometry g{};
    g.n0 = 128; g.n1 = 16; g.G = (long long)g.n0 * g.n1;
    ChainOptions O;
    ChainFacts F;
    F.ndim = 2; F.obs_model = BLHIP_OM_GAUSSIAN; F.use_rec = true; F.d = 1; F.fast = true;
    F.full = !evidence_only; F.evidence_only = evidence_only; F.accumulate = fused;
    F.n0 = g.n0; F.n1 = g.n1; F.G = g.G; F.T = T; F.B = B;
    F.series = series;
    ChainAdmit A = chain_admit(F, O, prog);
    ChainResPlan cp;
    cp.r0_max = A.r0_max; cp.allow_ax1 = A.allow_ax1;
    bool clamp = false;
    const bool planned = A.plan && plan_chainres(g, prog, taps, B, T, F.full, F.cus(), cp);
    if (!chain_settle(F, O, A, planned, cp, clamp) || !cp.has_reset) { std::printf("prefix %s %s: no route\n", who, fit); return; }
    const ChainPrefix P = chain_prefix_plan(F, O, prog, cp, cp.ax1, fused);
    std::printf("prefix %s %s: share %d skip %d saved %lld\n", who, fit, P.share ? 1 : 0, P.skip ? 1 : 0, P.saved);
}

void route(const char *what, bool series, int ndim, bool chain_on, bool clamp, bool repeat) {
    const char *why = series_route_refusal(series, ndim, chain_on, clamp, repeat);
    if (why) std::printf("route %s: fails: %s\n", what, why);
    else std::printf("route %s: runs\n", what);
}
}   // namespace

int main() {
    prefix("hyper", "evidence_only", false, true, false);
    prefix("series", "evidence_only", true, true, false);
    prefix("hyper", "fused", false, false, true);
    prefix("series", "fused", true, false, true);
    route("series 2d chain", true, 2, true, false, false);
    route("series 2d declined", true, 2, false, false, false);
    route("series 2d clamp", true, 2, true, true, false);
    route("series 2d repeat", true, 2, true, false, true);
    route("series 1d declined", true, 1, false, false, false);
    route("fit 2d declined", false, 2, false, false, false);
    route("fit 2d repeat", false, 2, true, false, true);
    return 0;
}
