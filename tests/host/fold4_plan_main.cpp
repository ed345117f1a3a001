// Stand-alone host program around chain_fold_plan (bayesloop_amd/csrc/blhip_chain_plan.hpp) for the FOUR-chain flavour of the two-chain fold
// kernel: the rounds, ring lengths and partial accumulators of the folding backward pass of a hyper-study's full fit, with the options
// fold4 / fold4_min_chains as given.  It launches nothing and runs on a CPU.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/fold4_plan_main.cpp -o fold4_plan && ./fold4_plan n0=128 n1=16 cus=8 fold4_min_chains=1 chain=3 chain=3
// Arguments, key=value in any order: n0 n1 T cus, chain=R0[...] (chain_plan_main.cpp's chain syntax), om=gauss|table, fold4, fold4_min_chains, fold2.
// Prints "plan strips .. ntw .. cpr .. pad ..", "fold fused .. fold2 .. fold4 .. slots_used ..", "round_start_b ..", "round_nk_b ..",
// "cost <bytes per cell and chain-step of a full round's launch>".
// (the batch builder -- chains -> transition program and tap table -- is chain_plan_main.cpp's: that file is compiled in with its main renamed)
#define main chain_plan_cli_main
#include "chain_plan_main.cpp"
#undef main

int main(int argc, char **argv) {
    std::map<std::string, double> kv = {{"n0", 128}, {"n1", 16}, {"T", 8}, {"cus", 256}, {"fold4", 1}, {"fold4_min_chains", 32}, {"fold2", 1}};
    std::string om = "gauss";
    std::vector<Chain> chains;
    for (int k = 1; k < argc; ++k) {
        const std::string a = argv[k];
        const size_t eq = a.find('=');
        if (eq == std::string::npos) { std::fprintf(stderr, "not key=value: %s\n", argv[k]); return 2; }
        const std::string key = a.substr(0, eq), val = a.substr(eq + 1);
        if (key == "chain") chains.push_back(parse_chain(val));
        else if (key == "om") om = val;
        else if (kv.count(key)) kv[key] = std::strtod(val.c_str(), nullptr);
        else { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    if (chains.empty()) return 2;
    const int64_t T = (int64_t)kv["T"], B = (int64_t)chains.size();
    TapTable taps;
    ChainProgram prog;
    build(chains, T, false, taps, prog);
    Geometry g{};
    g.n0 = (int)kv["n0"]; g.n1 = (int)kv["n1"]; g.G = (long long)g.n0 * g.n1;
    ChainOptions O;
    O.fold2 = kv["fold2"] != 0.0; O.fold4 = kv["fold4"] != 0.0; O.fold4_min_chains = (int)kv["fold4_min_chains"];
    ChainFacts F;
    F.ndim = 2; F.obs_model = om == "table" ? BLHIP_OM_TABLE : BLHIP_OM_GAUSSIAN; F.use_rec = om == "gauss"; F.d = 1; F.has_lik_table = om == "table";
    F.fast = true; F.LW0 = prog.LW0; F.LW1 = prog.LW1;
    F.full = true; F.accumulate = true;                    // a hyper-study's full fit: the posteriors go into the average only
    F.n0 = g.n0; F.n1 = g.n1; F.G = g.G; F.T = T; F.B = B; F.num_cus = (int)kv["cus"];
    ChainAdmit A = chain_admit(F, O, prog);
    ChainResPlan cp;
    cp.r0_max = A.r0_max; cp.allow_ax1 = A.allow_ax1;
    bool clamp = false;
    const bool planned = A.plan && plan_chainres(g, prog, taps, B, T, F.full, F.cus(), cp);
    if (!planned || !chain_settle(F, O, A, planned, cp, clamp)) { std::printf("off\n"); return 0; }
    std::printf("plan strips %d ntw %d cpr %d pad %d\n", cp.strips, cp.ntw, cp.cpr, cp.pad);
    ChainFold f = chain_fold_plan(F, O, prog, taps, cp, A.tab, cp.ax1, clamp);
    bool keep = true;
    if (chain_needs_depad(F, cp, cp.ax1, f.post_private)) keep = chain_padding_rule(F, O, cp, true, f);
    keep = keep && chain_fold_settle(F, cp, A.tab, cp.ax1, f);
    std::printf("fold keep %d fused %d fold2 %d fold4 %d slots_used %d\n", keep, f.fused, f.fold2, f.fold4, f.slots_used);
    row("round_start_b", f.round_start_b); row("round_nk_b", f.round_nk_b);
    if (f.fold2 && f.round_start_b.size() > 1) {
        ChainLaunch L;
        L.nslots = f.round_start_b[1] - f.round_start_b[0]; L.Gk = (long long)cp.n0p * cp.n1p; L.T = T; L.bwd = true; L.fold_now = true; L.two = true; L.quad = f.fold4;
        L.nk = f.round_nk_b[0];
        const ChainLaunchCost c = chain_launch_cost(L, 1.0, 0.0);          // (flops = the cells the launch computes)
        std::printf("cost %.17g\n", c.bytes / c.flops);
    }
    return 0;
}
