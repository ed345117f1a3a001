// The paths of a batch, one struct per path; do_fit (blhip.hip) sets the one up that runs a batch, calls its passes and knows nothing of its
// buffers.  Here: BatchEnv, what every path reads of the batch, and the resident paths (kernels: blhip_resident.hpp, blhip_chainres.hpp)
// with their eligibility, buffers, launches and the host-side checks after each pass.  The 1-D paths: blhip_fit_row1d.hpp; the
// launch-per-step path: blhip_fit_step.hpp.  Included by blhip.hip INSIDE its anonymous namespace, after the helpers it uses
// (DeviceTables, DeviceMeta, GeometryPlan, ChainProgram, TapTable, plan_ / launch_ functions, resident_unlag / chain_unlag, BatchOutcome).
#pragma once

// ---- what the paths of a batch need to know about it ----------------------------------------------------------------------------------
struct BatchEnv {
    blhip_ctx *ctx; const blhip_problem *p; hipStream_t st;
    Geometry g; long long G; int64_t T, B, c0; int d, rec_len;
    FitFlags ff;
    const DeviceTables *DT; const DeviceMeta *M; const ChainProgram *prog; const TapTable *taps;
    const GeometryPlan *gp;       // which kernel family the batch would take without the resident paths, and its block geometry
    Tile tile;                    // ... the tile of the launch-per-step and 1-D kernels: tile.nblk partial-sum slots per (step, chain, sum)
    double step0;                 // lattice step of the row axis (likelihood recurrence)
    double *d_post;               // the batch's sequence buffer (null: evidence-only)
    double *d_pp[2];              // the two state buffers, B x G each (evidence-only forward passes, every backward pass)
    const double *d_carry_src;    // BLHIP_RESUME: step 0 reads each chain's carried (normalised) state ...
    const double *d_unit;         // ... and these "previous partial sums", which add up to 1
    const double *log_w;          // log weights of ALL chains of the call (accumulate)
    bool chain_means;             // the caller asked for per-chain posterior means
    std::vector<hipEvent_t> *fold_ev = nullptr;      // start / end events of fold kernels nobody waits for (do_fit reads them after its last batch)
    int64_t bi = 0;               // index of the batch in the call
    bool allow_chainres = true;   // false: a repeated batch (its first attempt poisoned the carried partial accumulators)
    Trace *tr = nullptr;          // option trace: host phases on stderr
    void mark(const char *what) const { if (tr) tr->mark(what); }
};

// The resident backward kernels normalise every posterior by a PREDICTED sum (self-adjoint stencil identity); the host accepts the
// batch only if the prediction reproduces the reduced sums to this relative tolerance, three decades inside the parity bar of the
// posteriors (1e-9) -- the prediction is a running product of two rounded factors per step, so its error grows with the number of
// steps: a few ulp per step at worst (observed ~1e-14 at T = 2000); else: the launch-per-step kernels
inline double pred_rtol(int64_t T) { return 1e-12 + 2e-15 * (double)T; }

// Bound of every in-kernel wait of a resident launch.  A block that is not co-resident never arrives, so the bound IS the cost of the
// failure a user on a shared GPU meets first: it scales with the pass (20 x the predicted pass time at ~15 us per step, at least 250 ms)
// instead of a flat 2 s.  (50 ms was tried: four test processes sharing ONE GPU -- pytest -n 4 -- starve each other's blocks for longer than
// that and the paths gave up spuriously.)  Option resident_timeout_s > 0 overrides.
inline double resident_timeout_s(blhip_ctx *ctx, int64_t T) {
    const double opt = ctx->option("resident_timeout_s", 0.0);
    return opt > 0.0 ? opt : std::max(0.25, 20.0 * 15e-6 * (double)T);
}

// did a block of a resident launch time out waiting for a peer (not every block co-resident)?  -> the context stops using the paths
// (force: a test pretends that a block gave up -- chain_force_fail_stage 3; the same side effects as a real give-up)
bool resident_gave_up(blhip_ctx *ctx, hipStream_t st, const unsigned *d_abort, bool force = false) {
    ctx->pinS.ensure(64);
    unsigned *h = reinterpret_cast<unsigned *>(ctx->pinS.as<char>());
    HIPCHECK(hipMemcpyAsync(h, d_abort, 4, hipMemcpyDeviceToHost, st));
    sync_stream(ctx, st);
    // (option resident_force_abort: the tests of the fall-back pretend that a block gave up)
    if (*h != 0u || force || ctx->option("resident_force_abort", 0.0) != 0.0) {
        ctx->resident_last_reason = *h != 0u ? BLHIP_FALLBACK_GAVE_UP : BLHIP_FALLBACK_FORCED;
        if (ctx->resident.ok && ctx->option("quiet", 0.0) == 0.0)
            std::fprintf(stderr, "[blhip] a resident launch gave up waiting for a peer block (its blocks were not all co-resident: a shared or "
                                 "partitioned GPU?); this batch is repeated and the context continues with the launch-per-step kernels\n");
        ctx->resident.gave_up();
        return true;
    }
    return false;
}

// Is the chip ours?  A grid of one block per CU with the resident kernels' footprint; every block counts itself in and waits (bounded)
// for the others.  -> false: not all of them were on the chip together -- another process holds CUs, or the device is partitioned: a
// resident launch would sit out its time-out (>= 0.25 s) before the fit fell back.  ~15 us when the chip is free.
bool chip_is_ours(blhip_ctx *ctx) {
    hipStream_t st = ctx->stream;
    ctx->pinS.ensure((8 + 256) * sizeof(unsigned));
    unsigned *h = reinterpret_cast<unsigned *>(ctx->pinS.as<char>());
    DevBuf &d = ctx->probebuf;
    const size_t pbytes = (8 + 256) * sizeof(unsigned);
    d.ensure(pbytes);
    HIPCHECK(hipMemsetAsync(d.p, 0, pbytes, st));
    const unsigned nb = (unsigned)std::min(ctx->num_cus, 256);
    const size_t lds = 150 * 1024;
    arm_kernel(reinterpret_cast<const void *>(&blr::residency_probe_kernel<0>));
    const unsigned long long ticks = (unsigned long long)(std::max(1e-4, ctx->option("resident_probe_timeout_s", 0.002)) * 1e8);
    BL_LAUNCH(blr::residency_probe_kernel<0>, dim3(nb), dim3(512), lds, st, d.as<unsigned>(), nb, ticks);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(h, d.p, pbytes, hipMemcpyDeviceToHost, st));
    sync_stream(ctx, st);
    // the dispatch order the both-axes kernels count on: blocks b, b + 8, b + 16, ... on ONE XCD, eight different ones for b = 0 .. 7
    bool order = nb >= 8;
    for (unsigned b = 0; b < nb && order; ++b) order = h[8 + b] != 0u && h[8 + b] == h[8 + (b & 7u)];
    for (unsigned a = 0; a < 8 && order; ++a)
        for (unsigned c = a + 1; c < 8 && order; ++c) order = h[8 + a] != h[8 + c];
    ctx->xcd_order_ok = order;
    return h[0] == nb && h[1] == 0u && ctx->option("resident_probe_force_busy", 0.0) == 0.0;
}

// Before a fit that may take a resident path: on the context's first fit, when the paths are re-armed after a give-up, and at most once
// per resident_probe_interval_s (1 s) otherwise.  A busy chip parks the resident paths exactly as a give-up does (retry after 8, 16, ..
// fits) -- at the price of the probe's bound (2 ms), not of a launch's.
void probe_residency(blhip_ctx *ctx) {
    if (!ctx->resident.ok || ctx->option("resident_probe", 1.0) == 0.0) return;
    const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    if (ctx->probe_last >= 0.0 && now - ctx->probe_last < ctx->option("resident_probe_interval_s", 1.0)) return;
    ctx->probe_last = now;
    const bool ours = chip_is_ours(ctx);
    ctx->timing.resident_probe = ours ? 1 : 2;
    if (ours) return;
    if (!ctx->probe_announced && ctx->option("quiet", 0.0) == 0.0)
        std::fprintf(stderr, "[blhip] the GPU is not exclusively ours (a one-block-per-CU probe did not get all its blocks onto the chip within "
                             "%.1f ms: another process, or a partitioned device); fits run on the launch-per-step kernels until a later probe finds it free\n",
                     1e3 * std::max(1e-4, ctx->option("resident_probe_timeout_s", 0.002)));
    ctx->probe_announced = true;
    ctx->resident.gave_up();
    ctx->resident_last_reason = BLHIP_FALLBACK_BUSY;
    ctx->timing.resident_fallback_reason = BLHIP_FALLBACK_BUSY;
}

// ---- the time-resident path of a single-chain batch: one launch per pass instead of one per step (blhip_resident.hpp) -----------------
struct ResidentRun {
    bool on = false;
    ResidentPlan rp;
    blr::ResParams RQ{};
    int nblk = 0;                                  // partial-sum slots per (step, sum): one per tile
    std::vector<double> rowsumF;                   // forward pass: the actual sums of the stored rows
    std::vector<double> sfwd;                      // the forward pass's scales s_k (backward: predicted posterior sums)
    double *d_sfwd = nullptr;
    unsigned *d_abort = nullptr;
    size_t flag_bytes = 0;

    // eligibility (one chain, Gaussian model with the likelihood recurrence, the same radius <= 8 kernels at every step) + buffers
    void setup(const BatchEnv &E, int64_t n_chains, bool fast, bool use_rec, size_t &psz) {
        blhip_ctx *ctx = E.ctx;
        const ChainProgram &prog = *E.prog;
        const TapTable &taps = *E.taps;
        const int64_t T = E.T;
        const bool full = E.ff.full;
        double w0[blr::R + 1] = {1.0}, w1[blr::R + 1] = {1.0};
        // (a caller-supplied backward message: the predicted posterior sums assume the uniform one)
        // (the likelihood: the Gaussian recurrence, or -- every other model -- the (T, G) table: blr::Res TAB, tiles of up to 64 x 64)
        const bool gauss = E.p->obs_model == BLHIP_OM_GAUSSIAN && use_rec && E.d <= blr::DMAX;
        const bool tab = E.p->obs_model == BLHIP_OM_TABLE && E.DT->lik != nullptr && ctx->option("resident_table", 1.0) != 0.0;
        if (fast && n_chains == 1 && (gauss || tab) && !E.ff.resume && !E.ff.carry && !E.p->backward_init &&
            prog.LW0 <= blr::R && prog.LW1 <= blr::R && ctx->option("resident", 1.0) != 0.0 && ctx->resident.ok &&
            plan_resident(E.g.n0, E.g.n1, std::min(ctx->num_cus, 256), rp)) {
            on = prog.kindF[0] == SRC_PRIOR && (!full || prog.kindB[T - 1] == SRC_UNIFORM);
            // (the padded 128 x 128 BACKWARD kernel spills 231 registers: 2000 x 1100, backward step 40 - 45 us against 26.8 us with one
            //  launch per step -- full fits of such grids keep the launch-per-step kernels, evidence-only / forward-only fits do not)
            if (rp.pad && rp.TR == 128 && full) on = false;
            if (tab && rp.TR == 128) on = false;
            const int k0 = T > 1 ? prog.tapF0[1] : -1, k1 = T > 1 ? prog.tapF1[1] : -1;
            for (int64_t t = 1; t < T && on; ++t)
                on = prog.kindF[t] == SRC_PREV && prog.tapF0[t] == k0 && prog.tapF1[t] == k1;
            for (int64_t t = 0; t < T - 1 && on && full; ++t)
                on = prog.kindB[t] == SRC_PREV && prog.tapB0[t] == k0 && prog.tapB1[t] == k1;
            if (on) {
                for (int k = 1; k <= blr::R; ++k) w0[k] = w1[k] = 0.0;
                if (k0 >= 0) for (int k = 0; k <= taps.lw[k0]; ++k) w0[k] = taps.w[taps.off[k0] + k];
                if (k1 >= 0) for (int k = 0; k <= taps.lw[k1]; ++k) w1[k] = taps.w[taps.off[k1] + k];
            }
        }
        if (!on) return;
        const size_t nt = (size_t)rp.ntiles;
        // the halo strips hold TAGGED elements (the value with a one-bit tag in its sign bit): the tags are what the consumers poll
        const size_t n_cols = 2 * nt * 2 * blr::R * rp.TR, n_rows = 2 * nt * 2 * blr::R * rp.TC;
        const size_t b_cols = carve_size(n_cols * 8), b_rows = carve_size(n_rows * 8);
        const size_t b_w = carve_size(2 * (blr::R + 1) * 8) + carve_size((size_t)T * 8);
        flag_bytes = b_cols + b_rows + carve_size(blr::NSLOT * nt * 4 * 8) + carve_size(64);
        ctx->resx.ensure(b_w + flag_bytes);
        char *rc = ctx->resx.as<char>();
        double *d_w = carve<double>(rc, 2 * (blr::R + 1));
        d_sfwd = carve<double>(rc, (size_t)T);
        RQ.cols = carve<double>(rc, n_cols);              // (everything polled is contiguous from here on: one memset per launch)
        RQ.rows = carve<double>(rc, n_rows);
        RQ.cols_bytes = (unsigned)(n_cols * 8); RQ.rows_bytes = (unsigned)(n_rows * 8);
        RQ.gran = carve<unsigned long long>(rc, blr::NSLOT * nt * 4);
        d_abort = carve<unsigned>(rc, 16);
        RQ.abort_word = d_abort;
        double hw[2 * (blr::R + 1)];
        for (int k = 0; k <= blr::R; ++k) { hw[k] = w0[k]; hw[blr::R + 1 + k] = w1[k]; }
        HIPCHECK(hipMemcpyAsync(d_w, hw, sizeof hw, hipMemcpyHostToDevice, E.st));
        sync_stream(ctx, E.st);
        RQ.w0 = d_w; RQ.w1 = d_w + blr::R + 1;
        RQ.n0 = E.g.n0; RQ.n1 = E.g.n1; RQ.tr = rp.tr; RQ.tc = rp.tc; RQ.ntiles = rp.ntiles; RQ.T = (int)T; RQ.d = tab ? 0 : E.d; RQ.rec_len = E.rec_len;
        RQ.lik = tab ? E.DT->lik : nullptr;
        RQ.lag = std::max(1, std::min(blr::MAXLAG, (int)ctx->option("resident_lag", 2.0)));
        RQ.m0 = E.DT->m0; RQ.m1 = E.DT->m1; RQ.colA = E.DT->colA; RQ.colB = E.DT->colB; RQ.rec = E.DT->rec; RQ.step0 = E.step0;
        RQ.timeout_ticks = (unsigned long long)(resident_timeout_s(ctx, T) * 1e8);      // wall_clock64: 100 MHz
        // partial-sum slots per step: one per tile (the launch-per-step kernels are the fall-back and keep theirs)
        nblk = rp.ntiles;
        psz = std::max(psz, (size_t)T * NRED * nblk);
    }

    void launch(const BatchEnv &E, bool bwd, double *psum) {
        blhip_ctx *ctx = E.ctx;
        hipStream_t st = E.st;
        const int64_t T = E.T;
        blr::ResParams Q = RQ;
        HIPCHECK(hipMemsetAsync(RQ.cols, 0, flag_bytes, st));          // strip tags, granules, abort word: zero before EVERY launch
        HIPCHECK(hipMemsetAsync(psum, 0, (size_t)T * NRED * nblk * 8, st));
        Q.psum = psum;
        // rows of the kept sequence are normalised inside the kernel, `lag` steps behind (what the host then still scales: the
        // last / first `lag` rows)
        if (bwd) {
            // the posteriors are stored normalised: their sums follow from the forward scales and the last forward row sum
            // (blhip_resident.hpp: predicted_sum)
            sfwd.assign(T, 1.0);
            for (int64_t t = RQ.lag; t < T; ++t) sfwd[t] = 1.0 / rowsumF[t - RQ.lag];
            HIPCHECK(hipMemcpyAsync(d_sfwd, sfwd.data(), (size_t)T * 8, hipMemcpyHostToDevice, st));
            Q.sfwd = d_sfwd; Q.n_first = rowsumF[T - 1] * (1.0 / (double)E.G);
            Q.src0 = E.DT->uniform; Q.post = E.d_post; Q.store = 1; Q.means = 1; Q.normalise = 0;
        } else {
            Q.src0 = E.DT->prior; Q.post = E.ff.evidence_only ? nullptr : E.d_post; Q.store = E.ff.evidence_only ? 0 : 1;
            Q.means = E.ff.forward_only ? 1 : 0; Q.normalise = E.ff.forward_only ? 1 : 0;
        }
#ifdef BLR_PROF
        ctx->small.ensure(4 * 16 * 16 * 8);
        HIPCHECK(hipMemsetAsync(ctx->small.p, 0, 4 * 16 * 16 * 8, st));
        Q.prof = ctx->small.as<unsigned long long>();
#endif
        launch_resident(st, rp, Q, bwd);
        {   // HBM: the halo strips (2 R rows + 2 R columns of every tile, 8-byte tagged elements written and read once per step) + what the fit keeps
            const double halo = 2.0 * 8.0 * 2.0 * blr::R * (rp.TR + rp.TC) / ((double)rp.TR * rp.TC);
            const double kept = bwd ? 16.0 : (Q.store ? 8.0 : 0.0) + (Q.normalise ? 16.0 : 0.0);
            account(ctx, bwd, (double)E.G * T * (halo + kept), (double)E.G * T * (2.0 * valu_stencil_flop(blr::R) + (bwd ? EPI_BWD_FLOP : EPI_FWD_FLOP)));
        }
#ifdef BLR_PROF
        {   // development build: where a step of one interior tile spends its time (shader-clock cycles between stamps)
            unsigned long long hh[4 * 16 * 16];
            HIPCHECK(hipMemcpyAsync(hh, ctx->small.p, sizeof hh, hipMemcpyDeviceToHost, st));
            sync_stream(ctx, st);
            static const char *names[15] = {"start", "h_pre", "gath_issue", "B1", "h_walk", "book", "gather", "B2", "pubR", "v_pre", "B3", "v_walk", "sums", "B4", "pubC"};
            static const int tids[4] = {0, 128, 256, -64};
            for (int wv = 0; wv < 4; ++wv) {
                const unsigned long long *h = hh + wv * 256;
                double acc[15] = {0}; int n = 0;
                for (int q = 0; q < 16; ++q) {          // (stamps a kernel flavour does not set stay zero: the interval goes to the next one that is set)
                    if (!h[q * 16 + 14] || !h[q * 16]) continue;
                    ++n;
                    unsigned long long last = h[q * 16];
                    for (int i = 1; i < 15; ++i) if (h[q * 16 + i]) { acc[i] += (double)(h[q * 16 + i] - last); last = h[q * 16 + i]; }
                }
                std::fprintf(stderr, "[blr prof %s thread %d] %d steps:", bwd ? "bwd" : "fwd", tids[wv], n);
                double tot = 0; for (int i = 1; i < 15; ++i) { std::fprintf(stderr, " %s %.0f", names[i], n ? acc[i] / n : 0.0); tot += n ? acc[i] / n : 0.0; }
                std::fprintf(stderr, " | total %.0f\n", tot);
            }
        }
#endif
    }

    // after the forward pass: every tile made it, and the sums allow the lag to be undone
    bool forward_ok(const BatchEnv &E, double *redF) {
        if (resident_gave_up(E.ctx, E.st, d_abort)) return false;
        if (!resident_unlag(redF, E.T, RQ.lag, rowsumF)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_RANGE; return false; }
        return true;
    }

    // after the backward pass: every tile made it, the lagged scale stayed in range, and the PREDICTED sums the kernel normalised
    // the stored posteriors by reproduce the reduced ones
    bool backward_ok(const BatchEnv &E, const double *redB) {
        const int64_t T = E.T;
        if (resident_gave_up(E.ctx, E.st, d_abort)) return false;
        for (int64_t t = 0; t < T; ++t) {
            const double Ct = redB[(size_t)t * NRED + 2], Nt = redB[(size_t)t * NRED];
            if (!(Ct > 1e-150 && Ct < 1e150) || !(Nt > 1e-250)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_RANGE; return false; }
        }
        double npred = rowsumF[T - 1] * (1.0 / (double)E.G);
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t k = T - 1 - t;
            if (k > 0) npred = (k >= RQ.lag ? 1.0 / redB[(size_t)(t + RQ.lag) * NRED + 2] : 1.0) * npred / sfwd[t + 1];
            const double Nt = redB[(size_t)t * NRED];
            if (!(std::fabs(npred - Nt) <= pred_rtol(T) * Nt)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_PREDICTION; return false; }
        }
        return true;
    }
};

// ---- the chain-resident path of a batch: rounds of chains stay in LDS for a whole pass (blhip_chainres.hpp) ---------------------------
// The carried partial accumulators (blhip_ctx::PartState) -> the average posterior.  Nobody waits for the kernel here.
void flush_partials(blhip_ctx *ctx, hipStream_t st, std::vector<hipEvent_t> *later_ev) {
    blhip_ctx::PartState &ps = ctx->part;
    if (!ps.live) return;
    const double newref = std::max(ctx->acc_logref, ps.maxlw);
    const double r = ctx->acc_first ? 0.0 : std::exp(ctx->acc_logref - newref), rb = std::exp(ps.ref - newref);
    const long long G = (long long)ps.n0 * ps.n1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (later_ev) {
        HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
        later_ev->push_back(e0); later_ev->push_back(e1);
        HIPCHECK(hipEventRecord(e0, st));
    }
    for_grid_y(ctx, ps.T, [&](long long t0, unsigned nt) {
        BL_LAUNCH(fold_parts_kernel, dim3((unsigned)(((G + 1) / 2 + NTHREADS - 1) / NTHREADS), nt), dim3(NTHREADS), 0, st, ctx->acc,
                           ctx->accpart.as<double>(), (long long)ps.T * ps.Gk, ps.slots_init, ps.n0, ps.n1, ps.T, r, rb,
                           ctx->acc_first ? 1 : 0, ps.n0p, ps.Gk, ps.ax1, (int)t0, ps.sw == 8 ? 3 : 4);
    });
    HIPCHECK(hipGetLastError());
    if (later_ev) HIPCHECK(hipEventRecord(e1, st));
    ctx->timing.accumulate_launches += 1;
    ctx->acc_logref = newref; ctx->acc_first = false; ctx->acc_folded += ps.nfold;
    ps = blhip_ctx::PartState{};
}

// Tests of the fall-backs of a mixed call: options chain_force_fail_batch (a batch index of the call; -1 off) and chain_force_fail_stage
// pretend that ONE batch's host check failed -- 1: forward_ok (range), 2: backward_ok (range), 3: a give-up seen after the backward pass.
// Only what the check returns changes: no kernel argument, no in-kernel time-out.
inline bool chain_forced_fail(const BatchEnv &E, int stage) {
    return (int64_t)E.ctx->option("chain_force_fail_batch", -1.0) == E.bi && (int)E.ctx->option("chain_force_fail_stage", 0.0) == stage;
}

// What the route of the path reads (blhip_chain_plan.hpp: its decisions are pure functions of these): the options, once per batch ...
inline ChainOptions chain_options(const blhip_ctx *ctx) {
    ChainOptions O;
    auto flag = [&](const char *name) { return ctx->option(name, 1.0) != 0.0; };
    O.chain_resident = flag("chain_resident"); O.chain_table = flag("chain_table"); O.chain_ax1 = flag("chain_ax1"); O.chain_wide = flag("chain_wide");
    O.chain_clamp = (int)ctx->option("chain_clamp", 1.0);
    O.fuse_accumulate = flag("fuse_accumulate"); O.fold2 = flag("fold2"); O.fold2_cp = flag("fold2_cp"); O.chain_depad = flag("chain_depad");
    O.share_prefix = flag("share_prefix"); O.skip_prefix = flag("skip_prefix"); O.carry_partials = flag("carry_partials");
    O.chain_resident_lag = std::max(2, std::min(blc::MAXLAG, (int)ctx->option("chain_resident_lag", 4.0)));
    O.fold4 = flag("fold4"); O.fold4_min_chains = (int)ctx->option("fold4_min_chains", 32.0);
    return O;
}

// ... and the facts about the batch
inline ChainFacts chain_facts(const BatchEnv &E, bool fast, bool use_rec) {
    ChainFacts F;
    F.ndim = E.p->ndim; F.obs_model = E.p->obs_model; F.use_rec = use_rec; F.d = E.d; F.has_lik_table = E.DT->lik != nullptr;
    F.fast = fast; F.fast_but_clamp = E.gp->fast_but_clamp;
    F.has_clamp = E.prog->has_clamp; F.LW0 = E.prog->LW0; F.LW1 = E.prog->LW1;
    F.resume = E.ff.resume; F.carry = E.ff.carry; F.full = E.ff.full; F.keep = E.ff.keep; F.accumulate = E.ff.accumulate;
    F.evidence_only = E.ff.evidence_only; F.forward_only = E.ff.forward_only; F.backward_init = E.p->backward_init != nullptr;
    F.n0 = E.g.n0; F.n1 = E.g.n1; F.G = E.G; F.T = E.T; F.B = E.B;
    F.chain_means = E.chain_means; F.allow_chainres = E.allow_chainres; F.resident_ok = E.ctx->resident.ok; F.num_cus = E.ctx->num_cus;
    F.acc_aligned = ((uintptr_t)E.ctx->acc & 15) == 0;
    F.series = E.ctx->series.data != nullptr;
    return F;
}

// a memory admission: `need` bytes against a fraction of what is free + what the context already holds for the purpose
inline bool chain_mem_admits(double need, double fraction, double own_cap) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    return chain_admits(need, fraction, (double)free_b, own_cap);
}

// development: where a step of strip 0 spends its time -- shader-clock cycles between the `n` stamps of a step, waves 0 and 2 (the kernels
// wrote them to blhip_ctx::small: chain_prof_arm)
inline void chain_prof_arm(blhip_ctx *ctx, hipStream_t st, blc::ChainParams &Q) {
    ctx->small.ensure(2 * 16 * 16 * 8);
    HIPCHECK(hipMemsetAsync(ctx->small.p, 0, 2 * 16 * 16 * 8, st));
    Q.prof = ctx->small.as<unsigned long long>();
}
inline void chain_prof_dump(blhip_ctx *ctx, hipStream_t st, const char *tag, bool bwd, int nk, const char *const *names, int n) {
    unsigned long long hh[2 * 16 * 16];
    HIPCHECK(hipMemcpyAsync(hh, ctx->small.p, sizeof hh, hipMemcpyDeviceToHost, st));
    sync_stream(ctx, st);
    for (int wvi = 0; wvi < 2; ++wvi) {
        const unsigned long long *h = hh + wvi * 256;
        double acc[16] = {0}; int cnt = 0;
        for (int q = 0; q < 16; ++q) { if (!h[q * 16 + n - 1] || !h[q * 16]) continue; ++cnt; for (int i = 1; i < n; ++i) acc[i] += (double)(h[q * 16 + i] - h[q * 16 + i - 1]); }
        std::fprintf(stderr, "[%s %s NK %d wave %d] %d steps:", tag, bwd ? "bwd" : "fwd", nk, wvi ? 2 : 0, cnt);
        double tot = 0; for (int i = 1; i < n; ++i) { std::fprintf(stderr, " %s %.0f", names[i], cnt ? acc[i] / cnt : 0.0); tot += cnt ? acc[i] / cnt : 0.0; }
        std::fprintf(stderr, " | total %.0f\n", tot);
    }
}

struct ChainRun {
    bool on = false;
    ChainOptions opt;                              // the options of the batch (setup)
    ChainResPlan cp;
    blc::ChainParams CQ{};
    int *d_order = nullptr, *d_tapid = nullptr, *d_tapid1 = nullptr;      // launch order; the chains' axis-0 / axis-1 tap sets
    unsigned char *d_ckF = nullptr, *d_ckB = nullptr;      // per (step, chain): what the chain kernels consume (ChainResPlan::ckF / ckB)
    size_t gran_bytes = 0;
    unsigned *d_abort = nullptr;
    std::vector<std::vector<double>> rowsumC;      // forward pass: the actual sums of the stored rows, per chain
    std::vector<std::vector<double>> sfwdC;        // forward pass: the scales it used, per chain
    // the batch's sequence buffer is read only by this fit's own backward pass / fold: free to use the kernel's strip-major layout
    bool post_private = false;
    bool tab = false;                              // the likelihood comes out of a table (blc::chain_kernel TAB)
    bool ax1 = false;                              // walks on both parameters: blc::chainax_kernel (the distribution is transposed between the filters)
    bool clamp = false;                            // RegimeSwitch steps: blc::chain_clamp_kernel (blhip_chainclamp.hpp; a clamped step waits for the sums of the step before)
    size_t xch_bytes = 0;
    int ax_mode = -1;                              // exchange mode (-1: per launch, see pass())
    // a padded grid whose sequence is NOT private (an ordinary fit that keeps its posteriors): the kernels work on a scratch sequence on
    // the padded geometry (blhip_ctx::postpad), depad_kernel writes the grid's rows into the sequence everybody else reads
    bool depad = false;
    // fused fold: the backward kernel adds the weighted, normalised posteriors to per-slot partial accumulators instead of storing
    // them (the separate fold re-read the whole sequence at the memory roof while the backward pass of the wide bands left
    // bandwidth unused: same bytes, one pass)
    bool fused = false;
    bool fold_done = false;                        // this batch's posteriors are in the accumulator already (or in the carried partial accumulators)
    bool part_fresh0 = true;                       // the first launch of the backward pass starts the slots (false: they carry earlier batches)
    bool touched_parts = false;                    // the backward pass of this batch has written the carried slots
    // fused fold with TWO chains per block (blc::chain_fold2_kernel): the backward pass runs rounds of 2 x cpr chains of its own
    bool fold2 = false;
    // ... with FOUR (its QUAD flavour): strips of 8 columns -- the stored sequence and the partial accumulators in [t][strip of 8][row][8]
    bool fold4 = false;
    std::vector<int> round_start_b, round_nk_b;
    bool share_prefix = false;                     // change-point batches: states before a chain's first restart are stored once (see setup)
    bool skip_prefix = false;                      // ... and computed once: a chain's forward pass begins at its first restart
    int prov = 0;                                  // the chain that stores / computes everything
    long long shared_steps = 0;                    // chain-steps not stored
    int *d_tshare = nullptr;
    std::vector<int> h_tshare;
    const double *redF_keep = nullptr;             // the forward pass's reduced sums (slot 1: the restart sums of change-point batches)
    int slots_used = 0;                            // partial accumulators the backward launches write (one per block column)
    long long Gk = 0;                              // cells per distribution on the geometry the kernels work on (padded: >= G)
    double *d_fold_sfwd = nullptr, *d_fold_w = nullptr, *d_fold_inf = nullptr, *d_zeros = nullptr;
    std::vector<double> fold_lw;                   // log weight of every chain of the batch (-inf: none)
    double fold_ref = -INFINITY;                    // the reference the batch's weights are relative to (the carried slots' one where they are continued)
    double fold_max = -INFINITY;                    // the batch's largest log weight

    // The route (blhip_chain_plan.hpp decides, stage by stage) and what it needs on the device.  A batch that declines -- here or at one
    // of the memory admissions -- keeps the launch-per-step kernels; it has by then allocated and uploaded what the steps before asked for.
    void setup(const BatchEnv &E, bool fast, bool use_rec, size_t &psz) {
        const ChainProgram &prog = *E.prog;
        const ChainFacts F = chain_facts(E, fast, use_rec);
        opt = chain_options(E.ctx);
        ChainAdmit A = chain_admit(F, opt, prog);
        tab = A.tab;
        if (!A.plan) return;
        cp.r0_max = A.r0_max; cp.allow_ax1 = A.allow_ax1;
        const bool planned = plan_chainres(E.g, prog, *E.taps, F.B, F.T, F.full, F.cus(), cp);
        E.mark("  plan_chainres");
        on = chain_settle(F, opt, A, planned, cp, clamp);
        if (!on) return;
        ax1 = cp.ax1;
        Gk = (long long)cp.n0p * cp.n1p;
        upload_metadata(E);
        if (ax1 && !both_axes_buffers(E)) return decline();
        fill_params(E, psz);
        // (no-stencil batches: only their folding backward pass reads the anchors; series fits never fold: the filtering flavours only)
        if (F.series) { if (!clamp && !series_tables(E, prog.LW0 > 0)) return decline(); }
        else if (!tab && !ax1 && (prog.LW0 > 0 || F.full) && !anchor_table(E)) return decline();
        ChainFold f = chain_fold_plan(F, opt, prog, *E.taps, cp, tab, ax1, clamp);
        bool keep = true;
        if (chain_needs_depad(F, cp, ax1, f.post_private))
            keep = depad = chain_padding_rule(F, opt, cp, chain_mem_admits(chain_depad_bytes(F, Gk), 0.8, (double)E.ctx->postpad.cap), f);
        keep = keep && chain_fold_settle(F, cp, tab, ax1, f);
        post_private = f.post_private; fused = f.fused; fold2 = f.fold2; fold4 = f.fold4; slots_used = f.slots_used;
        round_start_b = std::move(f.round_start_b); round_nk_b = std::move(f.round_nk_b);
        if (!keep) return decline();
        E.mark("  fold plan");
        upload_prefix(E, chain_prefix_plan(F, opt, prog, cp, ax1, fused));
        E.mark("  prefix plan");
        if (fused) fold_buffers(E);
    }

    void decline() { on = false; ax1 = false; Gk = 0; }

    // the per-chain and per-(step, chain) metadata of the kernels, carved out of blhip_ctx::resx
    void upload_metadata(const BatchEnv &E) {
        blhip_ctx *ctx = E.ctx;
        const int64_t T = E.T, B = E.B;
        // (granule slots for 2 x cpr chains: the two-chain fold kernel runs rounds of that size; its four-chain flavour rounds of
        //  4 x floor(CUs / 2 strips) chains on twice the strips: at most twice as many granules)
        const size_t gran_n = (size_t)blc::NSLOT * 2 * cp.cpr * cp.strips * 2 * (opt.fold4 ? 2 : 1);
        gran_bytes = carve_size(gran_n * 8);
        ctx->resx.ensure(carve_size((size_t)B * 4) * 4 + gran_bytes + carve_size(64) + 2 * carve_size((size_t)T * B));
        char *rc = ctx->resx.as<char>();
        d_order = carve<int>(rc, (size_t)B);
        d_tapid = carve<int>(rc, (size_t)B);
        d_tapid1 = carve<int>(rc, (size_t)B);
        d_tshare = carve<int>(rc, (size_t)B);
        CQ.gran = carve<unsigned long long>(rc, gran_n);
        d_abort = carve<unsigned>(rc, 16);
        CQ.abort_word = d_abort;
        d_ckF = carve<unsigned char>(rc, (size_t)T * B);
        d_ckB = carve<unsigned char>(rc, (size_t)T * B);
        if (cp.has_reset) {
            HIPCHECK(hipMemcpyAsync(d_ckF, cp.ckF.data(), (size_t)T * B, hipMemcpyHostToDevice, E.st));
            HIPCHECK(hipMemcpyAsync(d_ckB, cp.ckB.data(), (size_t)T * B, hipMemcpyHostToDevice, E.st));
        }
        HIPCHECK(hipMemcpyAsync(d_order, cp.order.data(), (size_t)B * 4, hipMemcpyHostToDevice, E.st));
        HIPCHECK(hipMemcpyAsync(d_tapid, cp.tap_id.data(), (size_t)B * 4, hipMemcpyHostToDevice, E.st));
        HIPCHECK(hipMemcpyAsync(d_tapid1, cp.tap_id1.data(), (size_t)B * 4, hipMemcpyHostToDevice, E.st));
        sync_stream(ctx, E.st);
        E.mark("  chain metadata H2D");
    }

    // both-axes kernels: the exchange buffers of a launch's chain slots, [slot][2 step parities][Gk] tagged elements, and the likelihood of
    // the even time steps as a table.  -> false: they do not fit
    bool both_axes_buffers(const BatchEnv &E) {
        blhip_ctx *ctx = E.ctx;
        const int64_t T = E.T, B = E.B;
        xch_bytes = (size_t)cp.cpr * 2 * (size_t)Gk * 8;
        // the likelihood of the even time steps (epilogue in the transposed layout) as a table: an exp per cell there otherwise.  Measured
        // (profiles/r05_notes.md): single fits are latency-bound and gain (200 x 200, radius 20: 7.9 -> 7.5 us per step); launches of
        // eight chains sit on eight XCDs, every one of which fetches the table through the fabric the exchange already saturates
        // (c4_both_axes 553 -> 578 ms): one or two chains only
        const double tab_bytes = (double)((T + 1) / 2) * (double)Gk * 8.0;
        // the exchange buffers and the table are not part of chains_per_batch's budget: a long series on a large geometry declines the
        // path here instead of failing in the allocator
        // (series fits: the table of the even steps is ONE data series' -- off; every chain evaluates its likelihood from its own records)
        const bool few = B <= 2 && ctx->series.data == nullptr;
        const bool want_tab = tab || few;
        if (!chain_mem_admits((double)xch_bytes + (want_tab ? tab_bytes : 0.0), 0.8, (double)ctx->xch.cap + (double)ctx->axlik.cap)) return false;
        ctx->xch.ensure(xch_bytes);
        CQ.xch = ctx->xch.as<double>(); CQ.xch_chain = 2 * Gk; CQ.tap_id1 = d_tapid1;
        ax_mode = -1;             // (development: 0 write-through stores on any XCD, 1 one XCD per chain, 2 plain stores, 3 both = the default)
        if (tab) {          // a tabulated model: every step reads its likelihood -- the even ones out of a transposed copy
            if (tab_bytes >= CHAIN_AXLIK_MAX_BYTES) return false;
            ctx->axlik.ensure((size_t)tab_bytes);
            blcl::chainax_lik_transpose(E.st, E.DT->lik, ctx->axlik.as<double>(), cp.n0p, E.g.n0, E.g.n1, (int)T);
            HIPCHECK(hipGetLastError());
            CQ.lik = ctx->axlik.as<double>(); CQ.lik_nat = E.DT->lik;
        } else if (few && tab_bytes < CHAIN_AXLIK_MAX_BYTES) {
            ctx->axlik.ensure((size_t)tab_bytes);
            blcl::chainax_lik_table(E.st, cp.n0p, E.g.n0, E.g.n1, (int)T, E.d, E.rec_len, E.DT->m0, E.DT->colA, E.DT->colB, E.DT->rec, ctx->axlik.as<double>());
            HIPCHECK(hipGetLastError());
            CQ.lik = ctx->axlik.as<double>();
        }
        return true;
    }

    // what every launch of the batch is told (pass: round_params adds the round's)
    void fill_params(const BatchEnv &E, size_t &psz) {
        const int64_t T = E.T, B = E.B;
        CQ.n0 = cp.n0p; CQ.n1 = cp.n1p; CQ.n0t = E.g.n0; CQ.n1t = E.g.n1; CQ.strips = cp.strips; CQ.T = (int)T; CQ.d = tab ? 0 : E.d; CQ.rec_len = E.rec_len;
        CQ.lag = opt.chain_resident_lag;
        CQ.B = (int)B; CQ.nblk = cp.strips; CQ.tap_id = d_tapid; CQ.taps = E.M->taps; CQ.tap_off = E.M->off; CQ.tap_lw = E.M->lw;
        CQ.post_stride = (long long)T * Gk;
        CQ.m0 = E.DT->m0; CQ.m1 = E.DT->m1; CQ.colA = E.DT->colA; CQ.colB = E.DT->colB; CQ.rec = E.DT->rec; if (tab && !ax1) CQ.lik = E.DT->lik; CQ.step0 = E.step0;      // (both-axes kernels: CQ.lik is their table of the even steps, set by both_axes_buffers)
        CQ.timeout_ticks = (unsigned long long)(resident_timeout_s(E.ctx, T) * 1e8);
        psz = std::max(psz, (size_t)T * B * NRED * cp.strips * (opt.fold4 ? 2 : 1));      // (the four-chain fold kernel: one slot per strip of 8 columns)
    }

    // the anchors of the likelihood recurrence: the same for every chain of the batch (same data, same grid) -- tabulated once, 32 bytes
    // per lane and step (C4: 134 MB), read by the kernels a step ahead (ChainParams::anch).  -> false: the table does not fit
    bool anchor_table(const BatchEnv &E) {
        blhip_ctx *ctx = E.ctx;
        const int64_t T = E.T;
        const size_t ab = (size_t)T * blc::NW * cp.strips * 64 * 4 * sizeof(double);
        if (!chain_mem_admits((double)ab, 0.5, (double)ctx->anchbuf.cap)) return false;
        ctx->anchbuf.ensure(ab);
        blc::AnchorParams AP{};
        AP.T = (int)T; AP.d = E.d; AP.rec_len = E.rec_len; AP.strips = cp.strips; AP.rows_per_wave = cp.ntw * blc::TM; AP.n0t = E.g.n0; AP.n1t = E.g.n1;
        AP.m0 = E.DT->m0; AP.colA = E.DT->colA; AP.colB = E.DT->colB; AP.rec = E.DT->rec; AP.out = ctx->anchbuf.as<double>();
        BL_LAUNCH(blc::anchor_table_kernel, dim3((unsigned)cp.strips, (unsigned)T), dim3(blc::NT), 0, E.st, AP);
        HIPCHECK(hipGetLastError());
        CQ.anch = ctx->anchbuf.as<double>();
        E.mark("  anchor table queued");
        return true;
    }

    // Series fits (blhip_set_series): chain b of the batch observes series E.c0 + b.  The batch's records go up as rec[(b T + t) rec_len + q]
    // (build_records per series); the filtering Gaussian flavours get their anchors from anchor_table_kernel run over B T "steps" -- chain
    // b's table begins anchor_index(T, 0, strips, 0, 0) doubles behind chain b - 1's --, the table models one (T, G) table per chain from
    // lik_table_kernel run over the batch's B T data segments.  The no-stencil flavours and blc::chainax_kernel evaluate from the records.
    // The kernels re-base their pointers by ChainParams::rec_chain / anch_chain / lik_chain.  -> false: the tables do not fit
    bool series_tables(const BatchEnv &E, bool filters) {
        blhip_ctx *ctx = E.ctx;
        const blhip_problem *p = E.p;
        const int64_t T = E.T, B = E.B;
        const int om = ctx->series.om;
        if (E.c0 < 0 || E.c0 + B > ctx->series.S) fail("internal: series fit: chains [%lld, %lld) of %lld series", (long long)E.c0, (long long)(E.c0 + B), (long long)ctx->series.S);
        if (tab && ax1) return false;                     // (two table layouts per batch: no series flavour)
        const size_t per = (size_t)T * p->seg_len * p->data_dim;       // doubles of one series
        const double *mine = ctx->series.data + (size_t)E.c0 * per;   // (the batch index enters HERE: series c0 .. c0 + B - 1)
        std::vector<double> h_series;
        size_t one_len = per;
        if (tab) h_series.assign(mine, mine + (size_t)B * per);
        else {
            std::vector<double> one;
            blhip_problem q = *p;
            for (int64_t b = 0; b < B; ++b) {
                int rec_len = 0, d = 0;
                q.data = mine + (size_t)b * per;
                build_records(&q, one, rec_len, d);
                if (rec_len != E.rec_len || d != E.d || one.size() != (size_t)T * rec_len) fail("internal: series fit: record layout");
                h_series.insert(h_series.end(), one.begin(), one.end());
            }
            one_len = (size_t)T * E.rec_len;
        }
        // (doubles of y steps of anchors: blc::anchor_index(y, 0, strips, 0, 0))
        auto anch_steps = [&](long long y) { return (size_t)y * blc::NW * (size_t)cp.strips * 64 * 4; };
        const size_t anch_one = anch_steps(T);
        const bool anchors = !tab && !ax1 && filters;
        const double need = tab ? (double)B * (double)T * (double)E.G * 8.0 : (anchors ? (double)B * (double)anch_one * 8.0 : 0.0);
        if (need > 0.0 && !chain_mem_admits(need, 0.5, (double)(tab ? ctx->lik1d.cap : ctx->anchbuf.cap))) return false;
        ctx->databuf.ensure(h_series.size() * 8);
        double *d_ser = ctx->databuf.as<double>();
        HIPCHECK(hipMemcpyAsync(d_ser, h_series.data(), h_series.size() * 8, hipMemcpyHostToDevice, E.st));
        if (tab) {
            ctx->lik1d.ensure((size_t)B * T * E.G * 8);
            double *d_lik = ctx->lik1d.as<double>();
            const long long G = E.G;
            const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 2048);
            for_grid_y(ctx, (long long)B * T, [&](long long y0, unsigned ny) {
                BL_LAUNCH(lik_table_kernel, dim3(gx, ny), dim3(NTHREADS), 0, E.st, om, d_lik + (size_t)y0 * G, G, E.g.n1, p->ndim, E.DT->m0, E.DT->m1,
                          d_ser + (size_t)y0 * p->seg_len * p->data_dim, p->seg_len, p->data_dim);
            });
            HIPCHECK(hipGetLastError());
            CQ.lik = d_lik; CQ.lik_chain = (long long)T * G;
        } else {
            CQ.rec = d_ser; CQ.rec_chain = (long long)one_len;
            if (anchors) {
                ctx->anchbuf.ensure((size_t)B * anch_one * 8);
                blc::AnchorParams AP{};
                AP.d = E.d; AP.rec_len = E.rec_len; AP.strips = cp.strips; AP.rows_per_wave = cp.ntw * blc::TM; AP.n0t = E.g.n0; AP.n1t = E.g.n1;
                AP.m0 = E.DT->m0; AP.colA = E.DT->colA; AP.colB = E.DT->colB;
                for_grid_y(ctx, (long long)B * T, [&](long long y0, unsigned ny) {
                    blc::AnchorParams A = AP;
                    A.T = (int)ny; A.rec = d_ser + (size_t)y0 * E.rec_len;
                    A.out = ctx->anchbuf.as<double>() + anch_steps(y0);
                    BL_LAUNCH(blc::anchor_table_kernel, dim3((unsigned)cp.strips, ny), dim3(blc::NT), 0, E.st, A);
                });
                HIPCHECK(hipGetLastError());
                CQ.anch = ctx->anchbuf.as<double>(); CQ.anch_chain = (long long)anch_one;
            }
        }
        sync_stream(ctx, E.st);            // (the host copy of the series goes out of use)
        E.mark("  series tables queued");
        return true;
    }

    // the shared prefix of change-point chains (chain_prefix_plan): the steps every chain leaves to the providing one -> device
    void upload_prefix(const BatchEnv &E, ChainPrefix P) {
        share_prefix = P.share; skip_prefix = P.skip; prov = P.prov;
        if (P.saved <= 0) return;
        HIPCHECK(hipMemcpyAsync(d_tshare, P.tsh.data(), (size_t)E.B * 4, hipMemcpyHostToDevice, E.st));
        sync_stream(E.ctx, E.st);
        shared_steps = P.saved; h_tshare = std::move(P.tsh);
        CQ.tshare = d_tshare; CQ.bprov = prov; CQ.skip_prefix = skip_prefix ? 1 : 0;
    }

    // fused fold: the partial accumulators, one per block column of a launch, and the per-chain scales and weights of prepare_fold
    void fold_buffers(const BatchEnv &E) {
        blhip_ctx *ctx = E.ctx;
        const int64_t T = E.T, B = E.B;
        // (carried slots of earlier batches: a larger buffer or another layout takes them into the accumulator first)
        if (ctx->part.live && ((size_t)slots_used * T * Gk * 8 > ctx->accpart.cap || ctx->part.T != (int)T || ctx->part.Gk != Gk || ctx->part.n0 != E.g.n0 ||
                               ctx->part.n1 != E.g.n1 || ctx->part.n0p != cp.n0p || ctx->part.ax1 != (ax1 ? 1 : 0) || ctx->part.sw != part_width()))
            flush_partials(ctx, E.st, E.fold_ev);
        ctx->accpart.ensure((size_t)slots_used * T * Gk * 8);
        ctx->accw.ensure(carve_size((size_t)T * B * 8) + 2 * carve_size((size_t)B * 8) + carve_size(8192));
        char *wc = ctx->accw.as<char>();
        d_fold_sfwd = carve<double>(wc, (size_t)T * B);
        d_fold_w = carve<double>(wc, (size_t)B);
        d_fold_inf = carve<double>(wc, (size_t)B);
        d_zeros = carve<double>(wc, 1024);      // (8 KB: a tile's four cells are read at base + 0 / 512 / 1024 / 1536 bytes, base < 4 KB)
    }

    // columns per strip of the partial accumulators' layout
    int part_width() const { return fold4 ? blc::WCOL / 2 : blc::WCOL; }
    // partial-sum slots per (step, chain, sum) of a pass
    int pass_nblk(bool bwd) const { return (bwd && fused && fold4) ? 2 * cp.strips : cp.strips; }

    // what the launch of chains order[s0 .. s1) is told
    blc::ChainParams round_params(const BatchEnv &E, bool bwd, double *psum, int s0, int s1, bool fold_now, bool first) const {
        blc::ChainParams Q = CQ;
        Q.chain_ids = d_order + s0;
        Q.nslots = s1 - s0;
        Q.psum = psum;
        Q.src0 = bwd ? E.DT->uniform : E.DT->prior;
        Q.kinds = cp.has_reset ? (bwd ? d_ckB : d_ckF) : nullptr;
        Q.reset = E.DT->reset;
        Q.post = E.d_post;
        Q.means = bwd ? (E.chain_means ? 1 : 0) : (E.ff.forward_only ? 1 : 0);
        Q.strip_major = (post_private || cp.pad || ax1) ? 1 : 0;            // (the stored sequence is private to the fit then)
        if (fused && fold4) Q.strip_major = 2;                              // (... and read by the four-chain fold kernel: strips of 8 columns)
        if (fold_now && fold4) { Q.strips = 2 * cp.strips; Q.nblk = 2 * cp.strips; }
        if (fold_now) {
            Q.sfwd = d_fold_sfwd; Q.wchain = d_fold_w; Q.infirst = d_fold_inf;
            Q.part = E.ctx->accpart.as<double>(); Q.part_stride = (long long)E.T * Gk;
            Q.zeros = d_zeros; Q.part_fresh = (first && part_fresh0) ? 1 : 0;          // (every slot is first used by the first launch: no memset)
        }
        return Q;
    }

    // one pass: the launches of the rounds follow each other on the stream
    void pass(const BatchEnv &E, bool bwd, double *psum) {
        blhip_ctx *ctx = E.ctx;
        hipStream_t st = E.st;
        const int64_t T = E.T, B = E.B;
        HIPCHECK(hipMemsetAsync(psum, 0, (size_t)T * B * NRED * pass_nblk(bwd) * 8, st));
        HIPCHECK(hipMemsetAsync(d_abort, 0, 64, st));
        const bool fold_now = bwd && fused, two = fold_now && fold2;
        const std::vector<int> &rstart = two ? round_start_b : cp.round_start, &rnk = two ? round_nk_b : cp.round_nk;
        const bool store = fold_now ? false : (bwd || !E.ff.evidence_only);
        for (size_t r = 0; r + 1 < rstart.size(); ++r) {
            HIPCHECK(hipMemsetAsync(CQ.gran, 0, gran_bytes, st));       // tags restart with every launch
            blc::ChainParams Q = round_params(E, bwd, psum, rstart[r], rstart[r + 1], fold_now, r == 0);
            if (fold_now) touched_parts = true;
#ifdef BLC_PROF
            chain_prof_arm(ctx, st, Q);
#endif
            if (ax1) {
                HIPCHECK(hipMemsetAsync(CQ.xch, 0, xch_bytes, st));           // (tags restart with every launch)
                // the blocks of a chain on ONE XCD (block b runs on XCD b % 8 -- observed, for speed only) and plain publishing stores, which
                // keep the lines in that XCD's L2 (write-through stores drop them: MI355X_MICROARCH.md); chain_ax1_mode = 0: write-through
                // stores and the dispatch order of the other chain kernels -- nothing then depends on the placement, not even the speed
                // (the placement is checked by the co-residency probe: where block b was NOT seen on XCD b % 8 -- another partition mode, a CU
                //  mask -- the plain stores' lines would never reach a consumer on another XCD: write-through stores in dispatch order then)
                Q.xch_mode = ax_mode >= 0 ? ax_mode : (ctx->xcd_order_ok ? 3 : 0);
                const bool prof = ctx->option("chain_prof", 0.0) != 0.0;
                if (prof) chain_prof_arm(ctx, st, Q);
                launch_chainax(st, Q, rnk[r], cp.ntw, bwd, store, cp.pad);
                static const char *ax_names[6] = {"start", "filter 1 + publish", "gather", "barrier", "filter 2 + epilogue", "sums + barrier"};
                if (prof) chain_prof_dump(ctx, st, "blc ax prof", bwd, rnk[r], ax_names, 6);
            }
            else if (clamp) {
                blc::ClampParams CP{Q, bwd ? E.M->cmodeB : E.M->cmodeF, bwd ? E.M->limitB : E.M->limitF};
                launch_chain_clamp(st, CP, rnk[r], cp.ntw, bwd, bwd || !E.ff.evidence_only);
            }
            else if (two && fold4) launch_fold4(st, Q, rnk[r], cp.ntw);
            else if (two) launch_fold2(st, Q, rnk[r], cp.ntw, cp.pad);
            else launch_chain(st, Q, rnk[r], cp.ntw, bwd, store, cp.pad);
            ChainLaunch L;
            L.nslots = Q.nslots; L.Gk = Gk; L.T = T; L.bwd = bwd; L.fold_now = fold_now; L.two = two; L.quad = two && fold4; L.ax1 = ax1; L.tab = tab;
            L.evidence_only = E.ff.evidence_only; L.nk = rnk[r]; L.share_prefix = share_prefix; L.skip_prefix = skip_prefix;
            L.tshare = h_tshare.data(); L.chains = cp.order.data() + rstart[r];
            const ChainLaunchCost cost = chain_launch_cost(L, bwd ? EPI_BWD_FLOP : EPI_FWD_FLOP, band_stencil_flop(chain_band_radius(rnk[r])));
            account(ctx, bwd, cost.bytes, cost.flops);
#ifdef BLC_PROF
            static const char *names[8] = {"start", "ring", "chain0", "scale+anchor", "epi0", "tiles1..", "sums", "barrier"};
            chain_prof_dump(ctx, st, "blc prof", bwd, rnk[r], names, 8);
#endif
        }
    }

    // after the forward pass: every strip made it, and the sums of every chain allow the scales to be undone
    bool forward_ok(const BatchEnv &E, double *redF) {
        if (resident_gave_up(E.ctx, E.st, d_abort)) return false;
        if (chain_forced_fail(E, 1)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_RANGE; return false; }
        redF_keep = redF;
        if (skip_prefix)               // the steps a chain did not compute: the providing chain's sums (raw: before anybody's scales are undone)
            for (int64_t b = 0; b < E.B; ++b)
                for (int64_t t = 0; t < h_tshare[b]; ++t)
                    std::memcpy(&redF[((size_t)t * E.B + b) * NRED], &redF[((size_t)t * E.B + prov) * NRED], NRED * sizeof(double));
        if (chain_unlag_batch(redF, E.T, CQ.lag, E.B, rowsumC, sfwdC, cp.has_reset ? E.prog->kindF.data() : nullptr,
                              skip_prefix ? h_tshare.data() : nullptr, clamp ? E.prog->cmodeF.data() : nullptr) >= 0) { E.ctx->resident_last_reason = BLHIP_FALLBACK_RANGE; return false; }
        return true;
    }

    // fused fold, before the backward pass: weights relative to the batch's own reference (core.py:1358-1366: chains without a finite
    // evidence do not count), the forward scales and the sum of the last step's posterior of every chain -> device; partials zeroed
    void prepare_fold(const BatchEnv &E, const BatchOutcome &O) {
        blhip_ctx *ctx = E.ctx;
        const int64_t T = E.T, B = E.B;
        fold_lw.assign(B, -INFINITY);
        fold_ref = -INFINITY;
        for (int64_t b = 0; b < B; ++b) {
            if (O.abort_step[b] >= 0 || !std::isfinite(O.logE[b]) || !std::isfinite(E.log_w[E.c0 + b])) continue;
            fold_lw[b] = O.logE[b] + E.log_w[E.c0 + b];
            fold_ref = std::max(fold_ref, fold_lw[b]);
        }
        // the slots carry earlier batches of this call: this batch's weights take THEIR reference (a batch whose evidence towers 500
        // e-folds above it would overflow them: the carried slots go into the accumulator first and the batch starts afresh)
        fold_max = fold_ref;
        part_fresh0 = true;
        if (ctx->part.live && opt.carry_partials) {
            if (!(fold_ref - ctx->part.ref <= 500.0)) flush_partials(ctx, E.st, E.fold_ev);
            else { fold_ref = ctx->part.ref; part_fresh0 = false; }
        } else if (ctx->part.live) flush_partials(ctx, E.st, E.fold_ev);
        ctx->pinA.ensure(((size_t)T * B + 2 * (size_t)B) * 8);
        double *h = ctx->pinA.as<double>(), *hw = h + (size_t)T * B, *hi = hw + B;
        for (int64_t b = 0; b < B; ++b) {
            std::memcpy(h + (size_t)b * T, sfwdC[b].data(), (size_t)T * 8);
            // a restart of the backward pass at step t: the kernel divides by sum(alpha_t reset), which the forward pass left in slot 1
            // of step t -- handed over where the forward scale of step t + 1 would be (the identity does not use it there)
            if (cp.has_reset)
                for (int64_t t = 0; t + 1 < T; ++t)
                    if (E.prog->kindB[(size_t)t * B + b] != SRC_PREV) h[(size_t)b * T + t + 1] = redF_keep[((size_t)t * B + b) * NRED + 1];
            hw[b] = std::isfinite(fold_lw[b]) ? std::exp(fold_lw[b] - fold_ref) : 0.0;
            hi[b] = 1.0 / (rowsumC[b][T - 1] * (1.0 / (double)E.G));
        }
        HIPCHECK(hipMemcpyAsync(d_fold_sfwd, h, (size_t)T * B * 8, hipMemcpyHostToDevice, E.st));
        HIPCHECK(hipMemcpyAsync(d_fold_w, hw, (size_t)B * 8, hipMemcpyHostToDevice, E.st));
        HIPCHECK(hipMemcpyAsync(d_fold_inf, hi, (size_t)B * 8, hipMemcpyHostToDevice, E.st));
        // the slots need no memset: the first launch of the pass reads zeros instead of them (part_fresh) -- except slots it does not
        // use (a first launch with fewer chains than slots), which later launches may
        const int first_n = fold4 ? (round_start_b[1] - round_start_b[0] + 3) / 4 : fold2 ? (round_start_b[1] - round_start_b[0] + 1) / 2 : cp.round_start[1] - cp.round_start[0];
        // (carried slots: only those no earlier batch has written)
        const int have = part_fresh0 ? first_n : ctx->part.slots_init;
        if (have < slots_used)
            HIPCHECK(hipMemsetAsync(ctx->accpart.as<double>() + (size_t)have * T * Gk, 0, (size_t)(slots_used - have) * T * Gk * 8, E.st));
        HIPCHECK(hipMemsetAsync(d_zeros, 0, 8192, E.st));
    }

    // after the backward pass: every strip made it and the lagged scale of the backward state stayed in range
    bool backward_ok(const BatchEnv &E, const double *redB) {
        if (resident_gave_up(E.ctx, E.st, d_abort, chain_forced_fail(E, 3))) return false;
        if (chain_forced_fail(E, 2)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_RANGE; return false; }
        const size_t n = (size_t)E.T * E.B;             // (every record of the pass, in memory order)
        for (size_t q = 0; q < n; ++q) {
            const double *r = &redB[q * NRED];
            if (!(r[2] > 1e-150 && r[2] < 1e150) || !(r[0] > 1e-250)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_RANGE; return false; }
        }
        return true;
    }

    // fused fold, after the backward pass: the kernel normalised every posterior by its PREDICTED sum -- the prediction must
    // reproduce the reduced sums (false: the caller repeats the batch with the launch-per-step kernels; the partials are dropped);
    // then the partial accumulators go into the average posterior (running reference exponent as in prepare_fold)
    // (later_ev: the fold kernel's start / end events -- nobody waits for it here: the host's bookkeeping of this batch and the next batch's
    //  setup run beside it, do_fit reads the events after its last batch)
    bool fold(const BatchEnv &E, const double *redB, std::vector<hipEvent_t> &later_ev) {
        blhip_ctx *ctx = E.ctx;
        // (tests of the repeat after poisoned carried slots: pretend that this batch's prediction check failed)
        if ((int64_t)ctx->option("fold_force_fail_batch", -1.0) == E.bi) { ctx->resident_last_reason = BLHIP_FALLBACK_PREDICTION; return false; }
        hipStream_t st = E.st;
        const int64_t T = E.T, B = E.B;
        const long long G = E.G;
        {
            // the backward scales, in processing order k = T - 1 - t (the kernel's rule, from the sums C of its new states), and the predicted
            // sums they lead to -- step by step over all chains (the records of a step are consecutive; chain by chain every read was a
            // cache line of its own: 0.4 ms per batch of 256 x 256 beside an idle GPU); per chain the operations and their order are unchanged
            const int lag = CQ.lag;
            std::vector<double> csum((size_t)T * B), sb((size_t)T * B, 1.0), npred((size_t)B);      // [k][b]
            const double rtol = pred_rtol(T);
            for (int64_t k = 0; k < T; ++k) {
                const int64_t t = T - 1 - k;
                const double *rt = redB + (size_t)t * B * NRED;
                double *ck = &csum[(size_t)k * B], *sk = &sb[(size_t)k * B];
                for (int64_t b = 0; b < B; ++b) {
                    ck[b] = rt[b * NRED + 2];
                    if (k >= lag) sk[b] = (k - lag - 1 >= 0 ? csum[(size_t)(k - lag - 1) * B + b] : 1.0) * sb[(size_t)(k - lag) * B + b] / csum[(size_t)(k - lag) * B + b];
                    const bool restart = cp.has_reset && E.prog->kindB[(size_t)t * B + b] != SRC_PREV && k > 0;
                    if (k == 0) npred[b] = rowsumC[b][T - 1] * (1.0 / (double)G);
                    else if (restart) npred[b] = sk[b] * redF_keep[((size_t)t * B + b) * NRED + 1];
                    else npred[b] = sk[b] * npred[b] / sfwdC[b][t + 1];
                    const double Nt = rt[b * NRED];
                    if (!(std::fabs(npred[b] - Nt) <= rtol * Nt)) { E.ctx->resident_last_reason = BLHIP_FALLBACK_PREDICTION; return false; }
                }
            }
        }
        if (std::isfinite(fold_ref)) {
            // the slots stay where they are: the next batch of the call adds to them, do_fit folds them after the last one (flush_partials)
            blhip_ctx::PartState &ps = ctx->part;
            int nfold = 0;
            for (int64_t b = 0; b < B; ++b) nfold += std::isfinite(fold_lw[b]) ? 1 : 0;
            if (!ps.live) { ps = blhip_ctx::PartState{}; ps.live = true; ps.ref = fold_ref; ps.first_batch = E.bi; }
            ps.maxlw = std::max(ps.maxlw, fold_max);
            ps.slots_init = std::max(ps.slots_init, slots_used);
            ps.nfold += nfold;
            ps.n0 = E.g.n0; ps.n1 = E.g.n1; ps.T = (int)T; ps.n0p = cp.n0p; ps.ax1 = ax1 ? 1 : 0; ps.Gk = Gk; ps.sw = part_width();
            (void)later_ev; (void)G; (void)st;
        }
        fold_done = true;
        return true;
    }
};
