// Which batches take blc::chain_clamp_kernel (blhip_chainclamp.hpp): the envelope and the routing rule, as pure host functions of plain
// facts about the batch -- no HIP, no library state (tests/host/chain_clamp_plan_main.cpp builds a stand-alone program around this header).
#pragma once

namespace blcp {

constexpr int ROWS_MIN = 32, ROWS_MAX = 512, COLS_MAX = 1024, RADIUS_MAX = 40, STRIP_COLS = 16;
constexpr int VARIANT = 11;        // blhip_timing::fwd_kernel_variant / bwd_kernel_variant of a pass on these kernels

// what the decision reads: everything chain_admit (blhip_chain_plan.hpp: clamp_facts) knows about the batch before plan_chainres plans the launches
struct ClampFacts {
    int ndim = 2;
    bool gaussian_recurrence = true;   // the Gaussian model, evaluated by the likelihood recurrence (no table, no per-cell exponential)
    int n0 = 0, n1 = 0;                // rows (first parameter) and columns of the grid
    int radius0 = 0, radius1 = 0;      // widest walk on the first / second parameter over the batch
    bool regime_switch_only = true;    // every clamp mode of the program is 1 or 2 (RegimeSwitch): no NotEqual, Deterministic, dense kernel
    bool composed = false;             // a `multi` stage list (ChainProgram::multi)
    bool restarts = false;             // a change point / break point: some step consumes the reset distribution
    bool same_taps = true;             // every chain applies ONE tap set at every step that filters
    bool resumed = false, carried = false, backward_init = false;
    int cus = 256;                     // compute units the launch may count on (co-residency: one block per CU)
};

// rows the kernels work on: 128, 256 or 512 (a 384-row grid runs padded inside 512); 0: outside the envelope
inline int clamp_rows(int n0) { return n0 < ROWS_MIN || n0 > ROWS_MAX ? 0 : (n0 <= 128 ? 128 : (n0 <= 256 ? 256 : 512)); }
inline int clamp_strips(int n1) { return (n1 + STRIP_COLS - 1) / STRIP_COLS; }
// ring length of a launch whose widest chain has radius r (0: no stencil): 4, 8, 12 .. 24; 0: a radius beyond the envelope
inline int clamp_ring(int r) { return r <= 0 ? 4 : (r > RADIUS_MAX ? 0 : (16 + 2 * ((r + 7) / 8 * 8)) / 4); }

inline bool chain_clamp_envelope(const ClampFacts &f) {
    if (f.ndim != 2 || !f.gaussian_recurrence) return false;
    if (!f.regime_switch_only || f.composed || f.restarts || !f.same_taps) return false;
    if (f.resumed || f.carried || f.backward_init) return false;
    if (clamp_rows(f.n0) == 0 || f.n1 < STRIP_COLS || f.n1 > COLS_MAX) return false;
    if (f.radius1 != 0 || f.radius0 > RADIUS_MAX || f.radius0 >= f.n0) return false;
    return clamp_strips(f.n1) <= f.cus;          // (block budget: at least one chain's strips co-resident; nslots = cus / strips per launch)
}

// option chain_clamp: 0 off, 2 wherever the envelope admits, 1 (default) where the kernels were measured faster than a launch per step by
// more than the pool's box-to-box spread (profiles/chain_clamp_notes.md).  Measured, from 1 chain x 2 strips to 64 chains x 32 strips:
//   * a launch per step costs the old path >= 17 us per step and pass (step kernel + reduction), more with chains x strips (10 - 28 ps per
//     cell of the batch); a step of a round of resident chains costs 2.9 us (13 strips) .. 6 us (64 strips, 512 rows), and a round holds
//     cus / strips chains -- per chain and step the resident kernels are 4 - 10 x cheaper whatever chains x strips is, partial last rounds
//     included (17 chains in rounds of 16, 9 in rounds of 8: 3.1 x and 4.6 x faster);
//   * the resident pass costs ~60 us once per fit (its metadata, the anchor table, the scale bookkeeping): what decides is how many
//     launches it saves, steps x passes (2 passes: a full fit; 1: evidence-only and forward-only).  At 2 - 3 pass-steps the fits were
//     equal or 10 - 30 % slower, at 8 and more 8 - 36 % faster and growing with the pass (5 - 10 x at hundreds of steps).
// So: pass-steps = steps x passes >= MIN_PASS_STEPS, for any chains x strips the envelope admits.  (Evidence-only fits of 4 .. 7 steps and
// full fits of 3 were not measured: they stay on the old path.)
constexpr long long MIN_PASS_STEPS = 8;
inline bool chain_clamp_route(int option, bool envelope, long long chains, int strips, long long steps, int passes, int cus) {
    if (!envelope || option == 0 || chains < 1 || strips < 1 || strips > cus) return false;
    if (option == 2) return true;
    return steps * passes >= MIN_PASS_STEPS;
}

}   // namespace blcp
