// The 1-D paths of a batch (kernels: blhip_fused1d.hpp, blhip_persist1d.hpp, blhip_chain1d.hpp): which of the three runs a pass, its
// parameters and buffers, the launches of both passes.  Included by blhip.hip INSIDE its anonymous namespace, after blhip_fit_paths.hpp
// (BatchEnv, resident_gave_up, resident_timeout_s).
#pragma once

struct Row1dRun {
    bool on = false;                       // the batch runs on the 1-D kernels (GeometryPlan::fused1d)
    bool chain = false;                    // one block per chain runs the whole pass (bl1c::chain1d_kernel)
    bool persist = false;                  // ONE persistent launch per pass (bl1p::persist1d_kernel); decided per attempt, see forward()
    bool gave_up_before = false;           // a persistent launch of this batch gave up: the repeat takes a launch per K steps
    bl1f::F1Params F1{};
    bl1p::P1Params P1{};
    double *d_lik1 = nullptr;              // the likelihood table the chains of the batch share
    unsigned *d_abort1 = nullptr;
    size_t p1d_bytes = 0;
    const double *d_fwd_sums = nullptr;    // the forward pass's partial sums (the chain kernel's backward launch reads them)
    const long long *d_row0 = nullptr;     // series fits: where each chain's rows begin in the batch's (B, T, n) table
    std::vector<double> h_series;          // ... the records (or data) of the batch's series, alive until the uploads are done (the pass is waited for)
    std::vector<long long> h_row0;

    void setup(const BatchEnv &E) {
        on = E.gp->fused1d;
        if (!on) return;
        chain = E.gp->chain1d;
        const DeviceTables &DT = *E.DT;
        const DeviceMeta &M = *E.M;
        F1.n = E.g.n1; F1.TJ = E.gp->f1_TJ; F1.nblk = E.tile.nblk; F1.LW = E.prog->LW1; F1.T = (int)E.T; F1.B = (int)E.B; F1.d = E.d; F1.rec_len = E.rec_len;
        F1.shared[SRC_PREV] = nullptr; F1.shared[SRC_PRIOR] = DT.prior; F1.shared[SRC_RESET] = DT.reset;
        F1.shared[SRC_UNIFORM] = DT.uniform; F1.shared[SRC_INDEP] = DT.indep;
        F1.taps = M.taps; F1.tap_off = M.off; F1.tap_lw = M.lw; F1.m1 = DT.m1; F1.colA = DT.colA; F1.rec = DT.rec; F1.lik = DT.lik;
        F1.cmode = nullptr; F1.tap_lw2 = M.lw2;
    }

    // the kernel-variant code of the pass that ran last
    int variant() const { return chain ? 9 : (persist ? 8 : 4); }

    size_t f1_lds(const BatchEnv &E, int64_t K) const {
        const int TJ = E.gp->f1_TJ, LW1 = E.prog->LW1;
        return (size_t)(4 * (TJ + 2 * K * LW1) + K * TJ + K * (LW1 + 1) + K * E.rec_len + 4 * 8 + 2 + K + 8 + K * 3 * TJ) * sizeof(double);
    }

    void forward(const BatchEnv &E, int64_t K, double *d_psF) {
        blhip_ctx *ctx = E.ctx;
        const blhip_problem *p = E.p;
        hipStream_t st = E.st;
        const int64_t T = E.T, B = E.B;
        const long long G = E.G;
        const double *d_lik = E.DT->lik;
        d_fwd_sums = d_psF;
        // 1-D grids whose blocks all fit on the chip at once: ONE persistent launch per pass (blhip_persist1d.hpp), else a launch per K steps
        // (a pass of a single superstep -- OnlineStudy.step, T <= K -- has no launch boundary to save)
        persist = !chain && !gave_up_before && ctx->resident.ok && ctx->option("persist1d", 1.0) != 0.0 && T > K &&
                  (long long)E.tile.nblk * B <= std::min(ctx->num_cus, 256);
        // (the chains of a batch see the same likelihood: tabulated once per batch by the in-kernel function itself, shared by both passes)
        // (rows beyond bl1c::NMAX: the long-row kernel has no likelihood of its own -- the table for any number of chains)
        const bool c1d_table = chain && (B >= 4 || E.g.n1 > bl1c::NMAX) && !d_lik && (p->obs_model == BLHIP_OM_POISSON || p->obs_model == BLHIP_OM_GAUSSIAN_MEAN);
        d_lik1 = nullptr;
        d_row0 = nullptr;
        if (ctx->series.data) series_table(E);
        else if (c1d_table) {
            ctx->lik1d.ensure((size_t)T * G * 8);
            d_lik1 = ctx->lik1d.as<double>();
            bl1f::F1Params Q = F1;
            build_lik1d_table(st, p->obs_model, Q, d_lik1);
        }
        if (persist) {
            const size_t xb = carve_size((size_t)2 * B * E.g.n1 * 16), gb = carve_size((size_t)2 * B * E.tile.nblk * 16);
            p1d_bytes = xb + gb + carve_size(64);
            ctx->p1d.ensure(p1d_bytes);
            char *pc = ctx->p1d.as<char>();
            P1 = bl1p::P1Params{};
            P1.xch = carve<unsigned long long>(pc, (size_t)2 * B * E.g.n1 * 2);
            P1.gran = carve<unsigned long long>(pc, (size_t)2 * B * E.tile.nblk * 2);
            d_abort1 = carve<unsigned>(pc, 16);
            P1.abort_word = d_abort1;
            P1.timeout_ticks = (unsigned long long)(resident_timeout_s(ctx, T) * 1e8);      // wall_clock64: 100 MHz
            P1.n = F1.n; P1.TJ = F1.TJ; P1.nblk = F1.nblk; P1.LW = F1.LW; P1.K = (int)K; P1.T = F1.T; P1.B = F1.B; P1.d = F1.d; P1.rec_len = F1.rec_len;
            for (int k = 0; k < 5; ++k) P1.shared[k] = F1.shared[k];
            P1.taps = F1.taps; P1.tap_off = F1.tap_off; P1.tap_lw = F1.tap_lw; P1.m1 = F1.m1; P1.colA = F1.colA; P1.rec = F1.rec; P1.lik = F1.lik;
        }
        if (chain) {
            launch_c1d(E, false, d_psF);
        } else if (persist) {
            launch_p1d(E, K, false, d_psF);
        } else {
            for (int64_t t = 0; t < T; t += K) {
                bl1f::F1Params Q = F1;
                Q.K = (int)std::min<int64_t>(K, T - t); Q.dir = 1; Q.t_first = (int)t;
                Q.srckind = E.M->kindF; Q.tap = E.M->tapF1; Q.psum = d_psF; Q.prev_slot = 0;
                Q.psum_prev = t > 0 ? d_psF + (size_t)(t - 1) * B * NRED * E.tile.nblk : E.d_unit;
                Q.store = E.ff.evidence_only ? 0 : 1; Q.means = E.ff.forward_only ? 1 : 0;
                if (E.ff.evidence_only) {
                    Q.post = nullptr; Q.src = E.d_pp[(t / K + 1) & 1]; Q.src_stride = G; Q.dst = E.d_pp[(t / K) & 1]; Q.dst_stride = G;
                } else {
                    Q.post = E.d_post; Q.post_stride = (long long)T * G; Q.dst = nullptr; Q.dst_stride = 0;
                    Q.src = E.d_post + (t > 0 ? (size_t)(t - 1) * G : 0); Q.src_stride = (long long)T * G;
                }
                if (t == 0 && E.ff.resume) { Q.src = E.d_carry_src; Q.src_stride = G; }
                launch_fused1d(st, p->obs_model, Q, false, f1_lds(E, Q.K));
            }
        }
        // 1-D paths: a row in, a row out per step (the K-steps-per-launch kernel re-reads only halos)
        account(ctx, false, (double)B * G * T * (16.0 + (d_lik ? 8.0 : 0.0)), (double)B * G * T * (valu_stencil_flop(E.prog->LW1) + EPI_FWD_FLOP));
    }

    void backward(const BatchEnv &E, int64_t K, double *d_psB) {
        const int64_t T = E.T, B = E.B;
        const long long G = E.G;
        if (chain) {
            launch_c1d(E, true, d_psB);
        } else if (persist) {
            launch_p1d(E, K, true, d_psB);
        } else {
            for (int64_t t = T - 1; t >= 0; t -= K) {
                bl1f::F1Params Q = F1;
                Q.K = (int)std::min<int64_t>(K, t + 1); Q.dir = -1; Q.t_first = (int)t;
                Q.srckind = E.M->kindB; Q.tap = E.M->tapB1; Q.psum = d_psB; Q.prev_slot = 2;
                Q.psum_prev = t < T - 1 ? d_psB + (size_t)(t + 1) * B * NRED * E.tile.nblk : nullptr;
                Q.store = 1; Q.means = 1; Q.post = E.d_post; Q.post_stride = (long long)T * G;
                const int64_t li = (T - 1 - t) / K;
                Q.src = E.d_pp[(li + 1) & 1]; Q.src_stride = G; Q.dst = E.d_pp[li & 1]; Q.dst_stride = G;
                launch_fused1d(E.st, E.p->obs_model, Q, true, f1_lds(E, Q.K));
            }
        }
        account(E.ctx, true, (double)B * G * T * (32.0 + (E.DT->lik ? 8.0 : 0.0)), (double)B * G * T * (valu_stencil_flop(E.prog->LW1) + EPI_BWD_FLOP));
    }

    // after a pass: did a block of the persistent launch time out waiting for a peer?  (the other two kernels wait for nobody)
    bool gave_up(const BatchEnv &E) {
        if (!persist || !resident_gave_up(E.ctx, E.st, d_abort1)) return false;
        gave_up_before = true;
        return true;
    }

private:
    // Series fits: chain b of the batch observes series (E.c0 + b) / H (blhip_set_series: H = 1; blhip_set_series_groups: H chains per
    // series with their own op values).  The records (the models with an in-kernel likelihood) or data (the table models) of the batch's
    // series go up once per batch, ONE launch tabulates them -- a table per SERIES, which the chains of its group share --, and the chain
    // kernel reads chain b's rows at row0[b] = ((c0 + b) / H - c0 / H) T.  A batch may begin and end inside a group (evidence-only fits
    // are cut by the library's own plan): its first and last series are then tabulated for the chains it holds of them.
    void series_table(const BatchEnv &E) {
        blhip_ctx *ctx = E.ctx;
        const blhip_problem *p = E.p;
        const int64_t T = E.T, B = E.B, H = ctx->series.H;
        const int om = ctx->series.om;
        if (!chain) fail("series fit: the batch is not one of the chain-resident 1-D kernel");
        if (H < 1 || E.c0 < 0 || E.c0 + B > ctx->series.S * H)
            fail("internal: series fit: chains [%lld, %lld) of %lld series x %lld", (long long)E.c0, (long long)(E.c0 + B), (long long)ctx->series.S, (long long)H);
        const int64_t s0 = E.c0 / H, nser = (E.c0 + B - 1) / H - s0 + 1;      // the series of the batch: s0 .. s0 + nser - 1
        const size_t per = (size_t)T * p->seg_len * p->data_dim;       // doubles of one series
        const double *mine = ctx->series.data + (size_t)s0 * per;     // (the batch index enters HERE)
        const bool records = om == BLHIP_OM_POISSON || om == BLHIP_OM_GAUSSIAN_MEAN;
        int rec_len = p->data_dim;
        if (records) {
            h_series.clear();
            std::vector<double> one;
            blhip_problem q = *p;
            q.obs_model = om;
            for (int64_t b = 0; b < nser; ++b) {
                int d = 0;
                q.data = mine + (size_t)b * per;
                build_records(&q, one, rec_len, d);
                if (rec_len != E.rec_len || d != E.d) fail("internal: series fit: record layout");
                h_series.insert(h_series.end(), one.begin(), one.end());
            }
        } else {
            h_series.assign(mine, mine + (size_t)nser * per);
        }
        h_row0.resize((size_t)B);
        for (int64_t b = 0; b < B; ++b) h_row0[(size_t)b] = (long long)((E.c0 + b) / H - s0) * T;
        ctx->databuf.ensure(carve_size(h_series.size() * 8) + carve_size((size_t)B * 8));
        char *cur = ctx->databuf.as<char>();
        double *d_ser = carve<double>(cur, h_series.size());
        long long *d_r0 = carve<long long>(cur, (size_t)B);
        HIPCHECK(hipMemcpyAsync(d_ser, h_series.data(), h_series.size() * 8, hipMemcpyHostToDevice, E.st));
        HIPCHECK(hipMemcpyAsync(d_r0, h_row0.data(), (size_t)B * 8, hipMemcpyHostToDevice, E.st));
        ctx->lik1d.ensure((size_t)nser * T * E.G * 8);
        d_lik1 = ctx->lik1d.as<double>();
        d_row0 = d_r0;
        bl1f::F1Params Q = F1;
        Q.rec = d_ser;
        Q.B = (int)nser;                  // (the table kernels' gridDim.z: the SERIES of the batch)
        for_grid_y(ctx, T, [&](long long y0, unsigned ny) { build_series_table(E.st, om, Q, d_ser, p->data_dim, d_lik1, y0, ny); });
    }

    void launch_c1d(const BatchEnv &E, bool bwd, double *psum) {
        const int64_t T = E.T;
        const DeviceMeta &M = *E.M;
        bl1f::F1Params Q = F1;
        if (d_lik1) Q.lik = d_lik1;
        Q.row0 = d_row0;
        Q.K = 1; Q.dir = bwd ? -1 : 1; Q.t_first = bwd ? (int)(T - 1) : 0; Q.psum = psum; Q.prev_slot = bwd ? 2 : 0;
        Q.srckind = bwd ? M.kindB : M.kindF; Q.tap = bwd ? M.tapB1 : M.tapF1;
        if (E.gp->shift1d) Q.cmode = bwd ? M.cmodeB : M.cmodeF;
        if (E.gp->clamp1d) { Q.limit = bwd ? M.limitB : M.limitF; Q.no_shift = E.prog->has_shift ? 0 : 1; }
        Q.store = (bwd || !E.ff.evidence_only) ? 1 : 0; Q.means = bwd ? 1 : (E.ff.forward_only ? 1 : 0);
        Q.post = (bwd || !E.ff.evidence_only) ? E.d_post : nullptr; Q.post_stride = (long long)T * E.G;
        Q.src = nullptr; Q.src_stride = 0; Q.dst = nullptr; Q.dst_stride = 0;
        // a resumed pass: step 0 (source kind SRC_PREV) consumes the carried states, normalised -- the kernel's scale is 1 there; a carried
        // pass that stores no sequence leaves the last step's row where finish_batch takes it for store_carry (K = 1: the parity of T - 1)
        if (!bwd && E.ff.resume) { Q.src = E.d_carry_src; Q.src_stride = E.G; }
        if (!bwd && E.ff.carry && E.ff.evidence_only) { Q.dst = E.d_pp[(T - 1) & 1]; Q.dst_stride = E.G; }
        Q.fwd_sums = bwd ? d_fwd_sums : nullptr;      // (where the forward launch wrote them: the same layout)
        launch_chain1d(E.st, d_lik1 ? BLHIP_OM_TABLE : E.p->obs_model, Q, bwd, 2);
    }

    void launch_p1d(const BatchEnv &E, int64_t K, bool bwd, double *psum) {
        blhip_ctx *ctx = E.ctx;
        hipStream_t st = E.st;
        const int64_t T = E.T, B = E.B;
        const DeviceMeta &M = *E.M;
        HIPCHECK(hipMemsetAsync(ctx->p1d.p, 0, p1d_bytes, st));       // tags 0, abort word 0
        bl1p::P1Params Q = P1;
        Q.dir = bwd ? -1 : 1; Q.psum = psum; Q.prev_slot = bwd ? 2 : 0;
        Q.srckind = bwd ? M.kindB : M.kindF; Q.tap = bwd ? M.tapB1 : M.tapF1;
        {   // the pass's weights spelled out per (step, chain): the kernel stages a superstep's weights with ONE load per element
            const long long TB = (long long)T * B;
            const size_t wb = carve_size((size_t)TB * (P1.LW + 1) * 8), lb = carve_size((size_t)TB * 4);
            if (wb + lb <= ((size_t)256 << 20)) {
                ctx->p1w.ensure(wb + lb);
                char *wc = ctx->p1w.as<char>();
                double *wtab = carve<double>(wc, (size_t)TB * (P1.LW + 1));
                int *lwtab = carve<int>(wc, (size_t)TB);
                const long long ne = TB * (P1.LW + 1);
                BL_LAUNCH(bl1p::build_wtab_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, Q.tap, M.lw, M.off, M.taps, TB, P1.LW, wtab, lwtab);
                HIPCHECK(hipGetLastError());
                Q.wtab = wtab; Q.lwtab = lwtab;
            }
        }
        Q.store = (bwd || !E.ff.evidence_only) ? 1 : 0; Q.means = bwd ? 1 : (E.ff.forward_only ? 1 : 0);
        Q.post = (bwd || !E.ff.evidence_only) ? E.d_post : nullptr; Q.post_stride = (long long)T * E.G;
        Q.src0 = (!bwd && E.ff.resume) ? E.d_carry_src : nullptr; Q.src0_stride = E.G;
        Q.dst = (bwd || E.ff.evidence_only) ? E.d_pp[((T - 1) / K) & 1] : nullptr; Q.dst_stride = E.G;
        launch_persist1d(st, E.p->obs_model, Q, bwd, f1_lds(E, K));
    }
};
