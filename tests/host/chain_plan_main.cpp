// Stand-alone host program around bayesloop_amd/csrc/blhip_chain_plan.hpp: the route of a batch through the chain-resident kernels of
// two-parameter grids -- plan_chainres and the stages ChainRun::setup (blhip_fit_paths.hpp) runs around it, in its order, without the device
// steps between them -- printed for one batch built from the command line.  It launches nothing and runs on a CPU.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/chain_plan_main.cpp -o chain_plan && ./chain_plan n0=100 n1=20 T=8 chain=3 chain=2 chain=1
// Arguments, key=value in any order:
//   n0 n1 T cus            the grid (rows, columns), the steps, the compute units (256)
//   chain=R0[:R1[:F[:B[:t/R]]]]   one chain: walk radii on the two axes; F the forward steps that restart, joined by '+' ('-': none); B the
//                          backward steps that restart ('=': step t where forward step t + 1 does, the default); t/R: from forward step t on
//                          (backward: t - 1 on) the axis-0 walk has radius R -- a second tap set
//   om=gauss|table clamp=1 the observation model (gauss: the recurrence, one data dimension; table: a likelihood table exists); RegimeSwitch steps
//   full accumulate keep carry resume evidence_only forward_only backward_init chain_means allow_chainres resident_ok acc_aligned   facts, 0 / 1
//   chain_resident chain_table chain_ax1 chain_wide chain_clamp fuse_accumulate fold2 fold2_cp chain_depad share_prefix skip_prefix   options
//   admitted=0|1           what the memory admission of a padded batch's second sequence answers (1)
//   admits=need,fraction,free,own              -> "admits 0 / 1" (chain_admits alone)
//   launch=nslots,Gk,T,bwd,fold,two,ax1,tab,evidence_only,nk,share,skip[,tshare of every chain of the launch]   -> "cost bytes flops cells"
//                          (chain_launch_cost alone, with epilogue and band flop of 1 and 0)
//   source=on,resident_failed,post_private,pad,ax1,depad,n0   -> "source layout sm_n0 through_depad" (chain_fold_source alone; layout 0 row-major,
//                          1 strip-major, 2 padded)
// Prints "constants", "admit", then "plan refused" or the plan, "route", and where the path is on "fold", "fold_source" (the layout the
// separate fold reads after each of the three outcomes of the planned batch) and "prefix" (see the code).
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
// what the library's launch tables (blhip_launch.hpp: every kernel family) define in front of the header; tests/test_chain_plan_host.py
// holds these two to that file's text
constexpr int FAST_R0_MAX = 40;
bool fold2_shape(int ntw) { return ntw >= 1 && ntw <= 4; }
#include "../../bayesloop_amd/csrc/blhip_chain_plan.hpp"

void row(const char *name, const std::vector<int> &v) {
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out(1);
    for (char c : s) { if (c == sep) out.emplace_back(); else out.back() += c; }
    return out;
}

struct Chain { int r0 = 0, r1 = 0; std::vector<int> rF, rB; bool mirror = true; int alt_t = -1, alt_r = 0; };

Chain parse_chain(const std::string &spec) {
    Chain c;
    const std::vector<std::string> f = split(spec, ':');
    c.r0 = std::atoi(f[0].c_str());
    if (f.size() > 1) c.r1 = std::atoi(f[1].c_str());
    auto steps = [](const std::string &s) { std::vector<int> v; if (s != "-" && !s.empty()) for (const std::string &x : split(s, '+')) v.push_back(std::atoi(x.c_str())); return v; };
    if (f.size() > 2) c.rF = steps(f[2]);
    if (f.size() > 3 && f[3] != "=") { c.mirror = false; c.rB = steps(f[3]); }
    if (f.size() > 4) { const std::vector<std::string> a = split(f[4], '/'); c.alt_t = std::atoi(a[0].c_str()); c.alt_r = std::atoi(a[1].c_str()); }
    if (c.mirror) for (int t : c.rF) c.rB.push_back(t - 1);
    return c;
}

// a tap set per (axis, radius): the planner reads the radii only
int tap_of(TapTable &taps, std::map<std::pair<int, int>, int> &ids, int axis, int r) {
    if (r <= 0) return -1;
    auto it = ids.find({axis, r});
    if (it != ids.end()) return it->second;
    const int id = (int)taps.lw.size();
    taps.off.push_back((int)taps.w.size()); taps.lw.push_back(r); taps.lw2.push_back(0);
    taps.w.resize(taps.w.size() + r + 1, 0.0);
    return ids[{axis, r}] = id;
}

void build(const std::vector<Chain> &chains, int64_t T, bool clamp, TapTable &taps, ChainProgram &prog) {
    const int64_t B = (int64_t)chains.size();
    const size_t nT = (size_t)T * B;
    std::map<std::pair<int, int>, int> ids;
    prog.kindF.assign(nT, SRC_PREV); prog.kindB.assign(nT, SRC_PREV);
    prog.cmodeF.assign(nT, clamp ? 1 : 0); prog.cmodeB.assign(nT, clamp ? 1 : 0);
    prog.limitF.assign(nT, 0.0); prog.limitB.assign(nT, 0.0);
    prog.tapF0.assign(nT, -1); prog.tapF1.assign(nT, -1); prog.tapB0.assign(nT, -1); prog.tapB1.assign(nT, -1);
    prog.has_clamp = prog.other_clamp = clamp;
    for (int64_t b = 0; b < B; ++b) {
        const Chain &c = chains[b];
        auto has = [](const std::vector<int> &v, int64_t t) { return std::find(v.begin(), v.end(), (int)t) != v.end(); };
        for (int64_t t = 0; t < T; ++t) {
            const size_t k = (size_t)t * B + b;
            // forward step t and backward step t - 1 apply the same transition
            const int r0 = (c.alt_t >= 0 && t >= c.alt_t) ? c.alt_r : c.r0;
            if (t == 0) prog.kindF[k] = SRC_PRIOR;
            else {
                if (has(c.rF, t)) prog.kindF[k] = SRC_RESET;
                prog.tapF0[k] = tap_of(taps, ids, 0, r0); prog.tapF1[k] = tap_of(taps, ids, 1, c.r1);
                const size_t kb = (size_t)(t - 1) * B + b;
                prog.tapB0[kb] = prog.tapF0[k]; prog.tapB1[kb] = prog.tapF1[k];
            }
            if (t == T - 1) prog.kindB[k] = SRC_UNIFORM;
            else if (has(c.rB, t)) prog.kindB[k] = SRC_RESET;
            prog.LW0 = std::max(prog.LW0, r0); prog.LW1 = std::max(prog.LW1, c.r1);
        }
    }
}

int run_admits(const std::string &v) {
    const std::vector<std::string> a = split(v, ',');
    if (a.size() != 4) return 2;
    std::printf("admits %d\n", chain_admits(std::strtod(a[0].c_str(), nullptr), std::strtod(a[1].c_str(), nullptr), std::strtod(a[2].c_str(), nullptr), std::strtod(a[3].c_str(), nullptr)) ? 1 : 0);
    return 0;
}

int run_launch(const std::string &v) {
    const std::vector<std::string> a = split(v, ',');
    if (a.size() < 12) return 2;
    auto I = [&](size_t k) { return std::atoll(a[k].c_str()); };
    ChainLaunch L;
    L.nslots = (int)I(0); L.Gk = I(1); L.T = I(2); L.bwd = I(3) != 0; L.fold_now = I(4) != 0; L.two = I(5) != 0; L.ax1 = I(6) != 0; L.tab = I(7) != 0;
    L.evidence_only = I(8) != 0; L.nk = (int)I(9); L.share_prefix = I(10) != 0; L.skip_prefix = I(11) != 0;
    std::vector<int> tsh, ids;
    for (size_t k = 12; k < a.size(); ++k) { tsh.push_back((int)I(k)); ids.push_back((int)ids.size()); }
    if (!tsh.empty() && (int)tsh.size() != L.nslots) return 2;
    if (tsh.empty() && (L.share_prefix || L.skip_prefix)) return 2;
    L.tshare = tsh.data(); L.chains = ids.data();
    const ChainLaunchCost c = chain_launch_cost(L, 1.0, 0.0);          // (flops = the cells the launch computes)
    std::printf("cost %.17g %.17g\n", c.bytes, c.flops);
    return 0;
}

int run_source(const std::string &v) {
    const std::vector<std::string> a = split(v, ',');
    if (a.size() != 7) return 2;
    auto I = [&](size_t k) { return std::atoi(a[k].c_str()); };
    const ChainFoldSource s = chain_fold_source(I(0) != 0, I(1) != 0, I(2) != 0, I(3) != 0, I(4) != 0, I(5) != 0, I(6));
    std::printf("source %d %d %d\n", s.layout, s.sm_n0, s.through_depad ? 1 : 0);
    return 0;
}
}   // namespace

int main(int argc, char **argv) {
    std::map<std::string, double> kv = {{"n0", 128}, {"n1", 16}, {"T", 8}, {"cus", 256}, {"clamp", 0}, {"full", 1}, {"accumulate", 0}, {"keep", 0}, {"carry", 0},
        {"resume", 0}, {"evidence_only", 0}, {"forward_only", 0}, {"backward_init", 0}, {"chain_means", 0}, {"allow_chainres", 1}, {"resident_ok", 1}, {"acc_aligned", 1},
        {"chain_resident", 1}, {"chain_table", 1}, {"chain_ax1", 1}, {"chain_wide", 1}, {"chain_clamp", 1}, {"fuse_accumulate", 1}, {"fold2", 1}, {"fold2_cp", 1},
        {"chain_depad", 1}, {"share_prefix", 1}, {"skip_prefix", 1}, {"admitted", 1}};
    std::string om = "gauss";
    std::vector<Chain> chains;
    std::printf("constants FAST_R0_MAX %d fold2_shape", FAST_R0_MAX);
    for (int ntw = 0; ntw <= 8; ++ntw) std::printf(" %d", fold2_shape(ntw) ? 1 : 0);
    std::printf(" CHAIN_R0_MAX %d MAXLAG %d\n", CHAIN_R0_MAX, blc::MAXLAG);
    for (int k = 1; k < argc; ++k) {
        const std::string a = argv[k];
        const size_t eq = a.find('=');
        if (eq == std::string::npos) { std::fprintf(stderr, "not key=value: %s\n", argv[k]); return 2; }
        const std::string key = a.substr(0, eq), val = a.substr(eq + 1);
        if (key == "chain") chains.push_back(parse_chain(val));
        else if (key == "om") om = val;
        else if (key == "admits") { if (int e = run_admits(val)) return e; }
        else if (key == "launch") { if (int e = run_launch(val)) return e; }
        else if (key == "source") { if (int e = run_source(val)) return e; }
        else if (kv.count(key)) kv[key] = std::strtod(val.c_str(), nullptr);
        else { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    if (chains.empty()) return 0;
    auto on = [&](const char *k) { return kv[k] != 0.0; };
    const int64_t T = (int64_t)kv["T"], B = (int64_t)chains.size();
    TapTable taps;
    ChainProgram prog;
    build(chains, T, on("clamp"), taps, prog);
    Geometry g{};
    g.n0 = (int)kv["n0"]; g.n1 = (int)kv["n1"]; g.G = (long long)g.n0 * g.n1;

    ChainOptions O;
    O.chain_resident = on("chain_resident"); O.chain_table = on("chain_table"); O.chain_ax1 = on("chain_ax1"); O.chain_wide = on("chain_wide");
    O.chain_clamp = (int)kv["chain_clamp"]; O.fuse_accumulate = on("fuse_accumulate"); O.fold2 = on("fold2"); O.fold2_cp = on("fold2_cp");
    O.chain_depad = on("chain_depad"); O.share_prefix = on("share_prefix"); O.skip_prefix = on("skip_prefix");
    ChainFacts F;
    F.ndim = 2; F.obs_model = om == "table" ? BLHIP_OM_TABLE : BLHIP_OM_GAUSSIAN; F.use_rec = om == "gauss"; F.d = 1; F.has_lik_table = om == "table";
    F.fast = !on("clamp"); F.fast_but_clamp = on("clamp");
    F.has_clamp = prog.has_clamp; F.LW0 = prog.LW0; F.LW1 = prog.LW1;
    F.resume = on("resume"); F.carry = on("carry"); F.full = on("full"); F.keep = on("keep"); F.accumulate = on("accumulate");
    F.evidence_only = on("evidence_only"); F.forward_only = on("forward_only"); F.backward_init = on("backward_init");
    F.n0 = g.n0; F.n1 = g.n1; F.G = g.G; F.T = T; F.B = B;
    F.chain_means = on("chain_means"); F.allow_chainres = on("allow_chainres"); F.resident_ok = on("resident_ok"); F.num_cus = (int)kv["cus"];
    F.acc_aligned = on("acc_aligned");

    // the stages, in ChainRun::setup's order
    ChainAdmit A = chain_admit(F, O, prog);
    std::printf("admit gauss %d tab %d may_ax1 %d clamp_try %d plan %d r0_max %d allow_ax1 %d\n", A.gauss, A.tab, A.may_ax1, A.clamp_try, A.plan, A.r0_max, A.allow_ax1);
    if (!A.plan) return 0;
    ChainResPlan cp;
    cp.r0_max = A.r0_max; cp.allow_ax1 = A.allow_ax1;
    const bool planned = plan_chainres(g, prog, taps, B, T, F.full, F.cus(), cp);
    if (!planned) std::printf("plan refused\n");
    else {
        std::printf("plan n0p %d n1p %d pad %d strips %d ntw %d cpr %d ax1 %d has_reset %d mixed %d\n", cp.n0p, cp.n1p, cp.pad, cp.strips, cp.ntw, cp.cpr, cp.ax1, cp.has_reset, cp.mixed);
        row("order", cp.order); row("round_start", cp.round_start); row("round_nk", cp.round_nk); row("tap_id", cp.tap_id); row("tap_id1", cp.tap_id1);
        row("tap_lw", taps.lw);
    }
    bool clamp = false;
    const bool path = chain_settle(F, O, A, planned, cp, clamp);
    std::printf("route on %d clamp %d n0p %d ntw %d pad %d\n", path, clamp, cp.n0p, cp.ntw, cp.pad);
    if (!path) return 0;
    row("route_nk", cp.round_nk);
    const bool tab = A.tab, ax1 = cp.ax1;
    ChainFold f = chain_fold_plan(F, O, prog, taps, cp, tab, ax1, clamp);
    std::printf("fold_plan post_private %d fused %d fold2 %d slots_used %d\n", f.post_private, f.fused, f.fold2, f.slots_used);
    bool keep = true, depad = false;
    const bool needs = chain_needs_depad(F, cp, ax1, f.post_private);
    if (needs) keep = depad = chain_padding_rule(F, O, cp, on("admitted"), f);
    keep = keep && chain_fold_settle(F, cp, tab, ax1, f);
    std::printf("fold keep %d needs_depad %d depad %d post_private %d fused %d fold2 %d slots_used %d\n", keep, needs, depad, f.post_private, f.fused, f.fold2, f.slots_used);
    // what finish_batch folds from, with the members as ChainRun holds them behind setup (on = keep; a decline clears none of the others):
    // the chain kernels ran | the batch was declined | they failed a check and the launch-per-step kernels repeated the batch
    std::printf("fold_source");
    const char *outcome[3] = {"ran", "declined", "failed"};
    for (int k = 0; k < 3; ++k) {
        const ChainFoldSource s = chain_fold_source(k == 1 ? false : keep, k == 2, f.post_private, cp.pad, ax1, depad, g.n0);
        std::printf(" %s_layout %d %s_n0 %d %s_depad %d", outcome[k], s.layout, outcome[k], s.sm_n0, outcome[k], s.through_depad ? 1 : 0);
    }
    std::printf("\n");
    row("round_start_b", f.round_start_b); row("round_nk_b", f.round_nk_b);
    if (!keep) return 0;
    const ChainPrefix P = chain_prefix_plan(F, O, prog, cp, ax1, f.fused);
    std::printf("prefix share %d skip %d prov %d saved %lld\n", P.share, P.skip, P.prov, P.saved);
    row("tfirst", P.tfirst); row("tsh", P.tsh);
    return 0;
}
