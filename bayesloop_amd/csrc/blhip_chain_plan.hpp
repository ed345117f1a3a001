// The route of a batch through the chain-resident kernels of two-parameter grids (blhip_chainres.hpp, blhip_chainax.hpp, blhip_chainclamp.hpp):
// everything ChainRun (blhip_fit_paths.hpp) decides that needs no HIP call -- which kernels run, on which geometry, in which rounds, whether
// the backward pass folds, what a padded batch does, which steps change-point chains share, which layout the separate fold reads afterwards,
// and what a launch moves and computes.  Pure
// functions of plain facts (ChainFacts), the options (ChainOptions) and the batch's transition program, one per stage, because
// plan_chainres and the memory admissions of the device side sit between them; tests/host/chain_plan_main.cpp builds a stand-alone program
// around this header (tests/test_chain_plan_host.py).
// Included by blhip.hip INSIDE its anonymous namespace, after Geometry, ChainProgram, TapTable (blhip_program.hpp), FAST_R0_MAX and
// fold2_shape (blhip_launch.hpp), the blc:: constants (blhip_chainres.hpp) and blcp:: (blhip_chainclamp_plan.hpp).
#pragma once

constexpr int CHAIN_MIN_ROWS = 32;            // smallest grid (rows) the chain-resident kernels take (on the 128-row geometry)
constexpr int CHAIN_R0_MAX = 80;               // widest band of the chain-resident kernels (ring of 44 entries); option chain_wide = 0: FAST_R0_MAX
constexpr int CHAIN_TALL_ROWS = 1024;         // ... and the one geometry beyond 512 rows: grids of 513 .. 1024 rows (option chain_tall = 0: off)
inline bool chain_rows_ok(int n0) { return n0 >= CHAIN_MIN_ROWS && n0 <= CHAIN_TALL_ROWS; }
inline bool chain_tall(int n0) { return n0 > 512 && n0 <= CHAIN_TALL_ROWS; }

// The geometry the kernels lay a chain of an n0 x n1 grid out on -- the ONE copy of the rule: plan_chainres plans with it, and the series
// plan (blhip_series.hpp: blhip_host_series_plan, and chains_per_batch for a series fit) counts a chain's bytes with it.  Strips: rows 128 / 256 / 384 / 512, or 1024 beyond 512, columns a
// multiple of 16.  Square (walks on both parameters, blc::chainax_kernel; grids of up to 512 rows and columns): the next of 128 / 256 / 512.
struct ChainGeometry { int n0p = 0, n1p = 0; };
inline int chain_square_side(int n0, int n1) { return std::max(n0, n1) <= 128 ? 128 : (std::max(n0, n1) <= 256 ? 256 : 512); }
inline ChainGeometry chain_geometry(int n0, int n1, bool square) {
    ChainGeometry c;
    if (square) { c.n0p = c.n1p = chain_square_side(n0, n1); return c; }
    c.n0p = chain_tall(n0) ? CHAIN_TALL_ROWS : (n0 + 127) / 128 * 128;
    c.n1p = (n1 + blc::WCOL - 1) / blc::WCOL * blc::WCOL;
    return c;
}
// tabulated likelihoods (blc::chain_kernel TAB): geometries of at most 512 rows, and no padded one of 384 / 512 rows (chain_settle)
inline bool chain_table_geometry_ok(int n0p, bool pad) { return n0p <= 512 && !(pad && n0p >= 384); }

// The chain-resident path (blhip_chainres.hpp): which chains of the batch run together, in which order, with which band width.
struct ChainResPlan {
    int ntw = 0, strips = 0, cpr = 0;            // product tiles per wave, strips per chain, chains per launch
    int n0p = 0, n1p = 0;                        // the geometry the kernels work on: rows 128 / 256 / 512, columns a multiple of 16
    bool pad = false;                            // the grid is smaller than that (padded cells hold zeros; sequences private to the fit only)
    int r0_max = 40;                             // widest axis-0 radius the launch may carry (set by the caller: 80 for 1024 rows)
    bool has_reset = false;                      // change points: some steps consume the reset distribution
    bool mixed = false;                          // ... in chains that also filter (random walk + change point in one model)
    std::vector<unsigned char> ckF, ckB;         // [T][B] what a step of the chain kernels consumes: SRC_PREV / SRC_RESET (| 0x80: unfiltered)
    std::vector<int> order, tap_id;              // chains sorted by stencil radius; the chain's axis-0 kernel (-1: none)
    bool allow_ax1 = false;                      // (set by the caller) walks on the second parameter too may be planned: blc::chainax_kernel
    bool ax1 = false;                            // ... and some chain has one: the batch runs the transposing kernels (square exact geometry)
    std::vector<int> tap_id1;                    // the chain's axis-1 kernel (-1: none)
    std::vector<int> round_start, round_nk;      // launches: order[round_start[r] .. round_start[r + 1]), band blocks NK
};

// every chain: prior, then the SAME axis-0 kernel at every step, nothing on axis 1 (forward; mirrored backward)
bool plan_chainres(const Geometry &g, const ChainProgram &prog, const TapTable &taps, int64_t B, int64_t T, bool full, int cus, ChainResPlan &cp) {
    // any grid of 32 .. 512 rows: the kernels work on the next geometry of 128 / 256 / 384 / 512 rows x a multiple of 16 columns;
    // 513 .. 1024 rows: 1024 rows x a multiple of 16 columns (one copy of the strip in LDS: blc::chain_kernel TALL; change-point batches keep their state in registers there too)
    if (!chain_rows_ok(g.n0)) return false;
    const ChainGeometry cg = chain_geometry(g.n0, g.n1, false);
    cp.n0p = cg.n0p; cp.n1p = cg.n1p;
    cp.pad = cp.n0p != g.n0 || cp.n1p != g.n1;
    cp.strips = cp.n1p / blc::WCOL;
    cp.ntw = cp.n0p / (blc::NW * blc::TM);
    if (cp.strips > blc::MAX_STRIPS || cp.strips > cus) return false;
    cp.cpr = cus / cp.strips;
    cp.tap_id.assign(B, -1);
    cp.tap_id1.assign(B, -1);
    cp.ax1 = false;
    // walks on both parameters (blhip_chainax.hpp): an exact square geometry (the blocks of a chain change between column strips and row strips)
    // -- the next square geometry of 128 / 256 / 512 rows = columns that holds the grid (PAD kernels where it is larger)
    const int ax_n = chain_square_side(g.n0, g.n1);
    const bool ax1_geom = cp.allow_ax1 && std::max(g.n0, g.n1) <= 512 && g.n0 >= 32 && g.n1 >= 32 && ax_n / blc::WCOL <= cus;
    std::vector<int> lw(B, 0);
    cp.ckF.assign((size_t)T * B, (unsigned char)SRC_PREV);
    cp.ckB.assign((size_t)T * B, (unsigned char)SRC_PREV);
    for (int64_t b = 0; b < B; ++b) {
        if (prog.kindF[b] != SRC_PRIOR || prog.tapF0[b] >= 0 || prog.tapF1[b] >= 0) return false;
        // the chain's band: the kernel of the first step that filters (every filtering step must use the same one)
        int k0 = -1, k1 = -1;
        for (int64_t t = 1; t < T && k0 < 0; ++t) k0 = prog.tapF0[(size_t)t * B + b];
        for (int64_t t = 0; t + 1 < T && k0 < 0 && full; ++t) k0 = prog.tapB0[(size_t)t * B + b];
        if (ax1_geom) {
            for (int64_t t = 1; t < T && k1 < 0; ++t) k1 = prog.tapF1[(size_t)t * B + b];
            for (int64_t t = 0; t + 1 < T && k1 < 0 && full; ++t) k1 = prog.tapB1[(size_t)t * B + b];
        }
        // a step either continues from the previous state through the chain's band, or RESTARTS from the reset distribution (a
        // change point, transitionModels.py:300-312) -- through the band (the change point comes before the random walk in the
        // combined model's list) or unfiltered (it comes after: the walk's output is discarded)
        auto classify = [&](unsigned char kind, int t0, int t1, unsigned char &out) {
            // (k1 = -1 unless the both-axes kernels may be planned; a restart passes through BOTH of the chain's bands or through none)
            if (kind == SRC_PREV && t0 == k0 && t1 == k1) { out = (unsigned char)SRC_PREV; return true; }
            if (kind == SRC_RESET && ((t0 == k0 && t1 == k1) || (t0 < 0 && t1 < 0))) {
                const bool filters = k0 >= 0 || k1 >= 0;
                out = (unsigned char)(SRC_RESET | ((filters && t0 < 0 && t1 < 0) ? 0x80 : 0));          // bit 7: no filter at this step
                cp.has_reset = true;
                if (filters) cp.mixed = true;
                return true;
            }
            return false;
        };
        for (int64_t t = 1; t < T; ++t) {
            const size_t k = (size_t)t * B + b;
            if (!classify(prog.kindF[k], prog.tapF0[k], prog.tapF1[k], cp.ckF[k])) return false;
        }
        if (full) {
            const size_t kl = (size_t)(T - 1) * B + b;
            if (prog.kindB[kl] != SRC_UNIFORM || prog.tapB0[kl] >= 0 || prog.tapB1[kl] >= 0) return false;
            for (int64_t t = 0; t < T - 1; ++t) {
                const size_t k = (size_t)t * B + b;
                if (!classify(prog.kindB[k], prog.tapB0[k], prog.tapB1[k], cp.ckB[k])) return false;
            }
        }
        cp.tap_id[b] = k0;
        cp.tap_id1[b] = k1;
        lw[b] = k0 >= 0 ? taps.lw[k0] : 0;
        if (lw[b] > cp.r0_max || lw[b] >= g.n0) return false;          // (single-period reflection)
        if (k1 >= 0) {
            cp.ax1 = true;
            if (taps.lw[k1] >= g.n1) return false;
            lw[b] = std::max(lw[b], taps.lw[k1]);                       // (one ring length for both filters: the wider walk's)
        }
    }
    if (cp.ax1) {
        // the transposing kernels: bands of radius <= 40 on either axis (ring lengths 8 .. 24 in steps of 4; the band's rounded radius inside
        // the grid: single-period reflection); the square geometry replaces the strip geometry planned above
        for (int64_t b = 0; b < B; ++b) if (lw[b] > FAST_R0_MAX || (std::max(8, (lw[b] + 7) / 8 * 8)) >= std::min(g.n0, g.n1)) return false;
        cp.n0p = cp.n1p = ax_n;
        cp.strips = ax_n / blc::WCOL;
        cp.ntw = ax_n / (blc::NW * blc::TM);
        cp.pad = ax_n != g.n0 || ax_n != g.n1;
        cp.cpr = cus / cp.strips;
    }
    cp.order.resize(B);
    for (int64_t b = 0; b < B; ++b) cp.order[b] = (int)b;
    std::stable_sort(cp.order.begin(), cp.order.end(), [&](int a, int c) { return lw[a] < lw[c]; });
    cp.round_start.clear(); cp.round_nk.clear();
    for (int64_t s0 = 0; s0 < B; s0 += cp.cpr) {
        const int64_t s1 = std::min<int64_t>(B, s0 + cp.cpr);
        int r0 = std::max(4, (lw[cp.order[s1 - 1]] + 3) / 4 * 4);             // (a product costs 64 cycles: bands as narrow as the widest chain of the launch allows)
        if (cp.ax1) r0 = std::max(8, (r0 + 7) / 8 * 8);                        // (ring lengths 8, 12, .. 24)
        cp.round_start.push_back((int)s0);
        cp.round_nk.push_back((prog.LW0 == 0 && !cp.ax1) ? 4 : (blc::TM + 2 * r0) / 4);          // (4: the no-stencil kernel)
    }
    cp.round_start.push_back((int)B);
    return true;
}

// ---- what the stages read ----------------------------------------------------------------------------------------------------------------
// the engine options of the path, read once per batch (ChainRun: chain_options); names and defaults are the options'
struct ChainOptions {
    bool chain_resident = true, chain_table = true, chain_ax1 = true, chain_wide = true;
    int chain_clamp = 1;                           // 0 off, 1 where measured faster, 2 wherever the envelope admits (blcp::chain_clamp_route)
    bool fuse_accumulate = true, fold2 = true, fold2_cp = true, chain_depad = true, share_prefix = true, skip_prefix = true;
    int chain_resident_lag = 4;                    // clamped to 2 .. blc::MAXLAG (lag 1 would need the sum of the step in flight)
    bool carry_partials = true;
    bool fold4 = true;                             // four chains per accumulator cell (blc::chain_fold2_kernel QUAD) where chain_fold_plan admits it; 0: the two-chain kernel
    int fold4_min_chains = 32;                     // ... for batches of at least so many chains
};

// plain facts about the batch: no pointer into device memory, no library state
struct ChainFacts {
    int ndim = 2, obs_model = 0;                   // BLHIP_OM_*
    bool use_rec = false;                          // the Gaussian model runs the likelihood recurrence
    int d = 0;                                     // data dimensions of the recurrence
    bool has_lik_table = false;                    // DeviceTables::lik exists
    bool fast = false, fast_but_clamp = false;     // GeometryPlan: the batch would take the fast kernels (... but for its clamps)
    bool has_clamp = false; int LW0 = 0, LW1 = 0;  // ChainProgram: clamps; the widest radius on either axis
    bool resume = false, carry = false, full = false, keep = false, accumulate = false, evidence_only = false, forward_only = false;      // FitFlags
    bool backward_init = false;                    // a caller-supplied backward message
    int n0 = 0, n1 = 0; long long G = 0;           // the grid
    int64_t T = 0, B = 0;
    bool chain_means = false, allow_chainres = true, resident_ok = true;
    int num_cus = 256;
    bool acc_aligned = true;                       // the average posterior's buffer is 16-byte aligned
    bool series = false;                           // a series fit (blhip_set_series): every chain of the batch observes its OWN data
    int cus() const { return std::min(num_cus, 256); }      // compute units a launch counts on: one block per CU
};

// what blcp::chain_clamp_envelope reads, from the batch (restarts / same_taps: filled in behind plan_chainres); false: a clamp mode the
// kernels do not carry
inline bool clamp_facts(const ChainFacts &F, const ChainProgram &prog, bool gauss, blcp::ClampFacts &f) {
    f.ndim = F.ndim; f.gaussian_recurrence = gauss;
    f.n0 = F.n0; f.n1 = F.n1; f.radius0 = prog.LW0; f.radius1 = prog.LW1;
    f.composed = prog.multi;
    f.resumed = F.resume; f.carried = F.carry; f.backward_init = F.backward_init;
    f.cus = F.cus();
    f.regime_switch_only = prog.other_clamp && !prog.dense_clamp && !prog.has_shift;
    for (size_t e = 0; e < prog.cmodeF.size() && f.regime_switch_only; ++e) f.regime_switch_only = prog.cmodeF[e] <= 2 && prog.cmodeB[e] <= 2;
    return f.regime_switch_only;
}

// ---- stage 1, before plan_chainres: which likelihood flavour, which kernel families may be planned -----------------------------------------
struct ChainAdmit {
    // the likelihood: the Gaussian recurrence, or a table (every other model on a 2-D grid -- built on the device for the closed-form
    // ones, evaluated by the caller otherwise: blc::chain_kernel TAB, geometries of <= 512 rows -- padded grids too --, radius <= 40, one chain per block)
    bool gauss = false, tab = false;
    bool may_ax1 = false;                          // walks on the second parameter too: the transposing kernels (blc::chainax_kernel)
    bool clamp_try = false;                        // RegimeSwitch batches (blhip_chainclamp.hpp) inside blcp::chain_clamp_envelope
    bool plan = false;                             // the batch may take the path: plan_chainres is called, with ...
    int r0_max = FAST_R0_MAX; bool allow_ax1 = false;      // ... these (ChainResPlan::r0_max / allow_ax1)
    blcp::ClampFacts cf;
};

inline ChainAdmit chain_admit(const ChainFacts &F, const ChainOptions &O, const ChainProgram &prog) {
    ChainAdmit A;
    A.gauss = F.obs_model == BLHIP_OM_GAUSSIAN && F.use_rec && F.d <= blc::DMAX;
    A.tab = F.obs_model == BLHIP_OM_TABLE && F.has_lik_table && O.chain_table;
    A.may_ax1 = (A.gauss || A.tab) && F.LW1 > 0 && O.chain_ax1;
    A.clamp_try = F.has_clamp && F.fast_but_clamp && O.chain_clamp != 0 && clamp_facts(F, prog, A.gauss, A.cf) && blcp::chain_clamp_envelope(A.cf);
    A.plan = (F.fast || A.clamp_try) && (A.gauss || A.tab) && !F.resume && !F.carry && !F.backward_init && (!F.has_clamp || A.clamp_try) &&
             (F.LW1 == 0 || A.may_ax1) && (double)F.G * 8.0 < 4.0e9 && O.chain_resident && F.resident_ok && F.allow_chainres;
    A.r0_max = (!A.tab && !A.clamp_try && O.chain_wide) ? CHAIN_R0_MAX : FAST_R0_MAX;
    A.allow_ax1 = A.may_ax1;
    return A;
}

// ---- stage 2, behind plan_chainres: the clamp kernels' envelope and route, their geometry, what has no kernel -> the path is on ------------
inline bool chain_settle(const ChainFacts &F, const ChainOptions &O, ChainAdmit &A, bool planned, ChainResPlan &cp, bool &clamp) {
    bool on = planned;
    clamp = false;
    if (A.clamp_try) {
        // (plan_chainres has checked: the prior first, ONE tap set per chain at every step, restarts noted)
        A.cf.same_taps = on; A.cf.restarts = on && cp.has_reset;
        on = on && blcp::chain_clamp_envelope(A.cf) && !cp.ax1 && cp.ntw <= 4 &&
             blcp::chain_clamp_route(O.chain_clamp, true, F.B, cp.strips, F.T, F.full ? 2 : 1, F.cus());
        if (on) {
            clamp = true;
            if (cp.ntw == 3) { cp.ntw = 4; cp.n0p = 512; cp.pad = true; }          // (a 384-row grid runs padded inside 512 rows)
            for (int &nk : cp.round_nk) nk = nk <= 4 ? 4 : (nk + 3) / 4 * 4;       // (ring lengths 4, 8, 12 .. 24)
        }
    }
    if (on && A.tab && cp.ntw > 4) on = false;
    if (on && A.tab && !cp.ax1 && !chain_table_geometry_ok(cp.n0p, cp.pad)) on = false;      // (padded 384 / 512-row geometries with a likelihood table: no kernel -- never selected by a test or workload, pruned in round 5)
    if (on && F.LW1 > 0 && !cp.ax1) on = false;
    return on;
}

// ---- the memory admissions of the device side: need < fraction x (free memory + what the context already holds for the purpose) -----------
inline bool chain_admits(double need, double fraction, double free_bytes, double own_cap) { return need < fraction * (free_bytes + own_cap); }
constexpr double CHAIN_AXLIK_MAX_BYTES = 8.0e9;        // largest likelihood table of the even steps the both-axes kernels are given

// ---- stage 3: does the backward pass fold, and how ------------------------------------------------------------------------------------------
struct ChainFold {
    bool post_private = false;                     // ChainRun::post_private / fused / fold2 / round_start_b / round_nk_b / slots_used
    bool fused = false, fold2 = false;
    bool fold4 = false;                            // ... with FOUR chains per block (strips of 8 columns: sequences and partial accumulators in [t][strip of 8][row][8])
    std::vector<int> round_start_b, round_nk_b;
    int slots_used = 0;
};

// the four-chain flavour of the two-chain fold kernel: ring lengths 6 .. 24 (radius <= 40: one band entry per lane fits the LDS beside the
// buffers), strips of 8 columns -- one granule per lane of the scale wave, one block per strip and chain quad
constexpr int FOLD4_NK_MIN = 6, FOLD4_NK_MAX = 24;
inline bool fold4_geometry(int strips16, int cus) { return 2 * strips16 <= blc::MAX_STRIPS && 2 * strips16 <= cus; }

// change-point batches: the two passes restart at the same places (backward step t restarts <=> forward step t + 1 does: unit-spaced
// time stamps, transitionModels.py:316-317)
inline bool chain_restarts_aligned(const ChainProgram &prog, int64_t B, int64_t T) {
    bool aligned = true;
    for (int64_t b = 0; b < B && aligned; ++b)
        for (int64_t t = 0; t + 1 < T && aligned; ++t)
            aligned = (prog.kindB[(size_t)t * B + b] != SRC_PREV) == (prog.kindF[(size_t)(t + 1) * B + b] != SRC_PREV);
    return aligned;
}

inline ChainFold chain_fold_plan(const ChainFacts &F, const ChainOptions &O, const ChainProgram &prog, const TapTable &taps, const ChainResPlan &cp,
                                 bool tab, bool ax1, bool clamp) {
    ChainFold f;
    // (the separate fold reads pairs of cells: an even number of columns; the fused fold's partials take any grid -- fold_parts_kernel)
    f.post_private = F.accumulate && F.full && !F.keep && !F.carry && ((F.G & 1) == 0 || cp.pad || ax1) && F.acc_aligned;
    // (a restart inside a FILTERING chain would need sum(alpha T(reset)) for the predicted sums: such batches store and fold separately)
    // (clamped batches store and fold afterwards: the predicted sums of the fused fold do not survive a clamp)
    f.fused = f.post_private && !cp.mixed && !clamp && O.fuse_accumulate;
    // (the two-chain kernel has no table / both-axes flavour)
    const bool two_ok = !tab && !ax1 && !F.chain_means && fold2_shape(cp.ntw) && O.fold2;
    // change-point batches: the predicted sums survive a restart only through the two-chain fold kernel's restart rule, and only if the
    // two passes restart at the same places
    // (the both-axes kernels' fold has no restart rule: such batches store and fold separately -- ADVICE r05)
    if (f.fused && cp.has_reset) f.fused = two_ok && O.fold2_cp && chain_restarts_aligned(prog, F.B, F.T);
    f.slots_used = (int)std::min<int64_t>(cp.cpr, F.B);
    if (f.fused && two_ok) {
        f.fold2 = true;
        const int per = 2 * cp.cpr;
        for (int64_t s0 = 0; s0 < F.B; s0 += per) {
            const int64_t s1 = std::min<int64_t>(F.B, s0 + per);
            const int tp = cp.tap_id[cp.order[s1 - 1]];                   // (sorted by radius: the last chain of the round is its widest)
            const int r0 = std::max(4, ((tp >= 0 ? taps.lw[tp] : 0) + 3) / 4 * 4);
            f.round_start_b.push_back((int)s0);
            f.round_nk_b.push_back(prog.LW0 == 0 ? 4 : (blc::TM + 2 * r0) / 4);          // (4: the no-stencil variant)
        }
        f.round_start_b.push_back((int)F.B);
        f.slots_used = (int)std::min<int64_t>(cp.cpr, (F.B + 1) / 2);
    }
    // FOUR chains per accumulator cell (8 + 16 / 4 = 12 B per chain, cell and step): filtering batches without restarts on an exact geometry,
    // every round's ring within 6 .. 24 -- one round beyond it and the whole batch keeps the two-chain kernel (one layout per batch)
    if (f.fold2 && O.fold4 && !cp.pad && !cp.has_reset && prog.LW0 > 0 && F.B >= O.fold4_min_chains && fold4_geometry(cp.strips, F.cus())) {
        const int quads = F.cus() / (2 * cp.strips), per = 4 * quads;
        std::vector<int> rs, rnk;
        bool ok = true;
        for (int64_t s0 = 0; s0 < F.B && ok; s0 += per) {
            const int64_t s1 = std::min<int64_t>(F.B, s0 + per);
            const int tp = cp.tap_id[cp.order[s1 - 1]];                   // (sorted by radius: the last chain of the round is its widest)
            const int r0 = std::max(4, ((tp >= 0 ? taps.lw[tp] : 0) + 3) / 4 * 4);
            const int nk = (blc::TM + 2 * r0) / 4;
            ok = nk >= FOLD4_NK_MIN && nk <= FOLD4_NK_MAX;
            rs.push_back((int)s0);
            rnk.push_back(nk);
        }
        if (ok) {
            rs.push_back((int)F.B);
            f.fold4 = true;
            f.round_start_b = std::move(rs); f.round_nk_b = std::move(rnk);
            f.slots_used = (int)std::min<int64_t>(quads, (F.B + 3) / 4);
        }
    }
    return f;
}

// A grid smaller than the geometry: only fits whose sequences are private to the fit (strip-major, padded) -- evidence-only fits and full
// fits of hyper- / change-point studies (folded in the backward kernel, or stored and folded by accumulate_pad_kernel) -- ...
// (the both-axes kernels keep their sequences in two alternating strip-major layouts: never the API's, also on an exact geometry)
inline bool chain_needs_depad(const ChainFacts &F, const ChainResPlan &cp, bool ax1, bool post_private) {
    return (cp.pad || ax1) && !(F.evidence_only || post_private);
}
inline double chain_depad_bytes(const ChainFacts &F, long long Gk) { return (double)F.B * (double)F.T * (double)Gk * 8.0; }
// ... or, at the price of a second sequence in memory (`admitted`: chain_admits of chain_depad_bytes), any fit: the posteriors are copied out
// of the padded layout afterwards (<= 512 rows: every flavour has a padded storing kernel; 1024 rows: forward passes only).  -> depad;
// false: the batch keeps the launch-per-step kernels.  Either way nothing folds in the backward kernel.
inline bool chain_padding_rule(const ChainFacts &F, const ChainOptions &O, const ChainResPlan &cp, bool admitted, ChainFold &f) {
    f.fused = false; f.fold2 = false; f.fold4 = false;
    return O.chain_depad && (cp.ntw <= 4 || !F.full) && admitted;
}

// the folding flavours that do not exist -> false: the batch keeps the launch-per-step kernels
// (<= 512 rows: what the two-chain kernel does not fold -- per-chain means asked for through the C-ABI, option fold2 = 0 -- is stored and
//  folded separately: the Gaussian one-chain kernel has no folding flavour there (round 6).  The tabulated one has, on exact
//  geometries; 1024 rows: the one-chain kernel is the only folding one, exact and padded; the both-axes kernels fold on padded grids too)
inline bool chain_fold_settle(const ChainFacts &F, const ChainResPlan &cp, bool tab, bool ax1, ChainFold &f) {
    if (f.fused && !f.fold2 && cp.ntw <= 4 && !ax1 && (cp.pad || !tab)) f.fused = false;
    if (cp.pad && cp.ntw > 4 && F.full && !f.fused) { f.fold2 = false; return false; }
    return true;
}

// ---- stage 4: the shared prefix of change-point chains --------------------------------------------------------------------------------------
// Change-point batches without a stencil whose backward pass folds: the chains are identical up to their first restart.  The chain
// with the LATEST first restart stores all its states; every other chain stores only from its own first restart on, and the
// folding backward pass reads the earlier ones from that chain (same values bit for bit: same kernel, same strips, same lagged
// scales).  Halves the forward pass's stores, and the backward pass's reads of those states hit the cache (the chains of a launch
// read the same rows at about the same time).  (Only when nothing overwrites the stored states: the fused fold.)
// The same chains need not COMPUTE that prefix either (a restart consumes the reset distribution, not the chain's past): with
// skip_prefix a chain's forward pass begins at its first restart, the sums of its earlier steps are copied from the providing chain
// (forward_ok).  Also for evidence-only fits, which store nothing.  C5: 250 chains x 1000 steps -> 125 k chain-steps of 250 k.
struct ChainPrefix {
    bool share = false, skip = false;              // ChainRun::share_prefix / skip_prefix
    int prov = 0;                                  // the chain that stores / computes everything
    long long saved = 0;                           // chain-steps not stored (0: no plan)
    std::vector<int> tfirst, tsh;                  // per chain: its first restart (T: none); the steps it leaves to the providing chain
};

inline ChainPrefix chain_prefix_plan(const ChainFacts &F, const ChainOptions &O, const ChainProgram &prog, const ChainResPlan &cp, bool ax1, bool fused) {
    ChainPrefix P;
    const int64_t T = F.T, B = F.B;
    const bool may_share = fused && O.share_prefix;
    const bool may_skip = (fused || F.evidence_only) && O.skip_prefix;
    // (series fits: the chains differ from their FIRST step on -- each observes its own data --, nothing of a prefix is anybody else's)
    if (F.series) return P;
    if (!((may_share || may_skip) && cp.has_reset && prog.LW0 == 0 && !cp.mixed && !ax1 && B >= 2)) return P;      // (blc::chainax_kernel reads neither tshare nor skip_prefix)
    P.tfirst.assign((size_t)B, (int)T);
    bool plain = true;
    for (int64_t b = 0; b < B && plain; ++b) {
        plain = prog.kindF[b] == SRC_PRIOR && cp.tap_id[b] < 0 && cp.tap_id1[b] < 0;
        for (int64_t t = 1; t < T; ++t)
            if (prog.kindF[(size_t)t * B + b] != SRC_PREV) { P.tfirst[b] = (int)t; break; }
    }
    if (!plain) return P;
    for (int64_t b = 1; b < B; ++b) if (P.tfirst[b] > P.tfirst[P.prov]) P.prov = (int)b;
    P.tsh.assign((size_t)B, 0);
    for (int64_t b = 0; b < B; ++b)
        if (b != P.prov) { P.tsh[b] = std::min(P.tfirst[b], P.tfirst[P.prov]); P.saved += P.tsh[b]; }
    if (P.saved > 0) { P.share = may_share || may_skip; P.skip = may_skip; }
    return P;
}

// ---- series fits on two-parameter grids: route or fail ----------------------------------------------------------------------------------------
// Only blc::chain_kernel and blc::chainax_kernel read a chain's OWN records / anchors / table.  Every other route of a batch -- the
// time-resident kernel of a single chain, the launch-per-step kernels, the clamping chain kernels, and the launch-per-step repeat after a
// chain-resident pass gave up or failed a check -- reads the batch's shared tables, which hold series 0.  -> nullptr: the batch may run
// (`chain_on`: ChainRun took it; `clamp`: on its clamping kernels; `repeat`: its passes ask for a repeat on other kernels); else why the
// fit has to fail (the caller then runs its loop)
inline const char *series_route_refusal(bool series, int ndim, bool chain_on, bool clamp, bool repeat) {
    if (!series || ndim != 2) return nullptr;
    if (!chain_on) return "the chain-resident kernels do not take this batch";
    if (clamp) return "the batch would run on the clamping chain-resident kernels";
    if (repeat) return "a chain-resident pass gave up or failed its check";
    return nullptr;
}

// ---- behind the passes: where the batch's posteriors are and in which layout the separate fold reads them (finish_batch, blhip.hip) ----------
// Only the chain kernels store anything but [t][row][column]: a batch that was planned and then declined (`on` is false; post_private,
// pad and depad describe the plan, not what ran) and a batch the launch-per-step kernels repeated after a failed check
// (`resident_failed`) left their posteriors row-major in blhip_ctx::post.
enum ChainFoldLayout {
    FOLD_ROW_MAJOR = 0,                            // [t][row][column]: accumulate_kernel / accumulate2_kernel / accumulate_small_kernel
    FOLD_STRIP_MAJOR = 1,                          // [t][column / 16][row][16] on the exact geometry: accumulate2_kernel with sm_n0 = the grid's rows
    FOLD_PADDED = 2,                               // ... on the padded geometry, or the both-axes kernels' alternating layouts: accumulate_pad_kernel
};
struct ChainFoldSource {
    int layout = FOLD_ROW_MAJOR;
    int sm_n0 = 0;                                 // FOLD_STRIP_MAJOR: rows per strip (FoldJob::sm_n0); 0 otherwise
    bool through_depad = false;                    // the posteriors reach blhip_ctx::post through depad_kernel (row-major there); false: the passes wrote the buffer themselves
};

inline ChainFoldSource chain_fold_source(bool on, bool resident_failed, bool post_private, bool pad, bool ax1, bool depad, int n0) {
    ChainFoldSource s;
    if (!on || resident_failed) return s;
    s.through_depad = depad;
    if (depad) return s;
    if (pad || ax1) s.layout = FOLD_PADDED;
    else if (post_private) { s.layout = FOLD_STRIP_MAJOR; s.sm_n0 = n0; }
    return s;
}

// ---- what a launch moves and computes BY CONSTRUCTION (blhip_timing: fwd / bwd _hbm_bytes, _flops) -----------------------------------------
struct ChainLaunch {
    int nslots = 0;                                // chains of the launch
    long long Gk = 0; int64_t T = 0;
    bool bwd = false, fold_now = false, two = false;       // a backward launch; ... that folds; ... with two chains per block
    bool quad = false;                                     // ... with four (the QUAD flavour: `two` holds as well)
    bool ax1 = false, tab = false, evidence_only = false;
    int nk = 4;                                    // ring length (4: no stencil)
    bool share_prefix = false, skip_prefix = false;
    const int *tshare = nullptr, *chains = nullptr;        // the shared steps of the launch's chains: tshare[chains[q]], q < nslots
};
struct ChainLaunchCost { double bytes, flops; };
inline int chain_band_radius(int nk) { return (4 * nk - blc::TM) / 2; }

// HBM: only what the fit keeps -- forward the stored state (8 B; nothing for evidence-only fits), backward the stored state in + the
// posterior out (16 B) or + the read-modify-write of the partial accumulator (24 B; shared by the two chains of a block of the two-chain
// fold kernel: 8 + 16 / 2 = 16 B; by four chains of its QUAD flavour: 8 + 16 / 4 = 12 B).  epi_flop / band_flop: per cell, the launch's epilogue and one band product of radius
// chain_band_radius(nk) (blhip_book.hpp: EPI_FWD_FLOP / EPI_BWD_FLOP, band_stencil_flop)
inline ChainLaunchCost chain_launch_cost(const ChainLaunch &L, double epi_flop, double band_flop) {
    double cells = (double)L.nslots * L.Gk * L.T;
    if (!L.bwd && L.skip_prefix)               // (chain-steps the forward pass does not run)
        for (int q = 0; q < L.nslots; ++q) cells -= (double)L.tshare[L.chains[q]] * L.Gk;
    double bytes = L.bwd ? (L.fold_now ? (L.quad ? 8.0 + 16.0 * ((L.nslots + 3) / 4) / (double)L.nslots : L.two ? 8.0 + 16.0 * ((L.nslots + 1) / 2) / (double)L.nslots : 24.0) : 16.0) : (L.evidence_only ? 0.0 : 8.0);
    // (both-axes kernels: the transposing exchange of a step leaves the XCD's L2 as well -- 8 written + 8 read;
    //  with the blocks of a chain on one XCD the reads mostly hit that L2: the PMC counters say what really moves)
    if (L.ax1) bytes += 16.0;
    double shared = 0.0;                                  // stored states not written (forward) / read once per launch instead of once per chain (backward)
    if (L.share_prefix && (L.bwd ? L.fold_now : !L.evidence_only)) {
        long long sum = 0, mx = 0;
        for (int q = 0; q < L.nslots; ++q) { const long long v = L.tshare[L.chains[q]]; sum += v; mx = std::max(mx, v); }
        shared = (double)(L.bwd ? sum - mx : sum) * L.Gk * 8.0;
    }
    // (tabulated likelihood: the table of the pass is read once per launch -- its chains read the same rows at about the same time)
    const double table = L.tab ? (double)L.T * L.Gk * 8.0 : 0.0;
    return {cells * bytes - shared + table, cells * ((L.nk > 4 ? band_flop * (L.ax1 ? 2.0 : 1.0) : 0.0) + epi_flop)};
}
