// The launch-per-step path of a batch (kernels: blhip_kernels.hpp + blhip_bigshift.hpp -- the generic step kernel, the stages of composed
// transitions, large shifts; blhip_fast.hpp, blhip_mfma.hpp, blhip_hwide.hpp -- the fast and matrix-pipe kernels with the wide
// pre-passes, one launch per radius bucket on the bucket streams): parameters, stage metadata, the step and the two time loops.  It is
// also what a batch is repeated on when a resident path gives up.  Included by blhip.hip INSIDE its anonymous namespace, after
// blhip_fit_paths.hpp (BatchEnv).
#pragma once

struct StepRun {
    StepParams P{};
    blf::FastParams FP{};
    StageMeta SM;                            // (composed transitions only: the stages in front of the fused step kernel)
    // per (step, stage): how many chains' stage is a large shift of a 2-D grid along axis 0 / axis 1 (blk::bigshift_kernel's chains)
    std::vector<int> big_stageF, big_stageB;
    std::vector<char> any_hF, any_hB, any_vF, any_vB;
    double *d_hsrc = nullptr, *d_vsrc = nullptr;
    bool multistream = false;
    bool mfma_h = true;
    double mfma_h_max_cells = 0.0;
    long long n_mfma[2] = {0, 0}, n_fast[2] = {0, 0};
    static constexpr int mfma_min_r0 = 8;

    void setup(const BatchEnv &E, const RowRecurrence &rr) {
        blhip_ctx *ctx = E.ctx;
        const blhip_problem *p = E.p;
        const GeometryPlan &gp = *E.gp;
        const ChainProgram &prog = *E.prog;
        const TapTable &taps = *E.taps;
        const DeviceTables &DT = *E.DT;
        const DeviceMeta &M = *E.M;
        const Geometry &g = E.g;
        const Tile &tile = E.tile;
        const int64_t T = E.T, B = E.B;
        const bool full = E.ff.full;
        if (prog.multi) {
            upload_stages(ctx, prog, B, E.G, tile.nblk, full, SM);
            auto count_big = [&](const std::vector<StepProg> &pre, std::vector<int> &cnt) {
                cnt.assign(2 * (pre.size() / (size_t)B), 0);
                for (size_t e = 0; e < pre.size(); ++e) {
                    const StepProg &q = pre[e];
                    if ((q.cmode & 15) != 6) continue;
                    if (q.t0 >= 0 && taps.lw2[q.t0] == BIGSHIFT_LW2) ++cnt[2 * (e / (size_t)B)];
                    else if (q.t1 >= 0 && taps.lw2[q.t1] == BIGSHIFT_LW2) ++cnt[2 * (e / (size_t)B) + 1];
                }
            };
            count_big(prog.preF, big_stageF);
            if (full) count_big(prog.preB, big_stageB);
        }
        P.n0 = g.n0; P.n1 = g.n1; P.TI = tile.TI; P.TJ = tile.TJ; P.LW0 = tile.LW0; P.LW1 = tile.LW1;
        P.tiles_i = tile.tiles_i; P.tiles_j = tile.tiles_j; P.nblk = tile.nblk; P.ndim = p->ndim; P.d = E.d;
        P.rec_len = E.rec_len; P.shared[SRC_PREV] = nullptr; P.shared[SRC_PRIOR] = DT.prior; P.shared[SRC_RESET] = DT.reset;
        P.shared[SRC_UNIFORM] = DT.uniform; P.shared[SRC_INDEP] = DT.indep; P.taps = M.taps; P.tap_off = M.off; P.tap_lw = M.lw; P.tap_lw2 = M.lw2;
        P.m0 = DT.m0; P.m1 = DT.m1; P.colA = DT.colA; P.colB = DT.colB; P.chains = (int)B;
        P.prev_nblk = tile.nblk;
        if (gp.fast) {
            FP.n0 = g.n0; FP.n1 = g.n1; FP.TJ = tile.TJ; FP.S = gp.fastS; FP.nseg = gp.fast_nseg;
            FP.tiles_j = tile.tiles_j; FP.nblk = tile.nblk; FP.fnblk = gp.fast_fnblk;
            FP.dump = M.dump;
            FP.mlean = (g.n0 % gp.mS == 0 && (double)E.G * 8.0 < 4.0e9 && g.n1 < (1 << 20) && g.n0 < (1 << 24)) ? 1 : 0;
            FP.mS = gp.mS; FP.mnseg = gp.m_nseg; FP.mtiles_j = gp.m_tiles_j; FP.mnblk = gp.m_nblk;
            FP.ndim = p->ndim; FP.d = E.d; FP.means = E.ff.forward_only ? 1 : 0;
            FP.shared[SRC_PREV] = nullptr; FP.shared[SRC_PRIOR] = DT.prior; FP.shared[SRC_RESET] = DT.reset;
            FP.shared[SRC_UNIFORM] = DT.uniform; FP.shared[SRC_INDEP] = DT.indep; FP.taps = M.taps; FP.tap_off = M.off; FP.tap_lw = M.lw;
            FP.m0 = DT.m0; FP.m1 = DT.m1; FP.colA = DT.colA; FP.colB = DT.colB; FP.prev_nblk = tile.nblk;
            FP.step0 = rr.step0; FP.use_rec = rr.use_rec ? 1 : 0;
        }
        // bucket streams: fork = every bucket stream waits for the main stream; join = the main stream waits for all of them
        // (only worth it when a step really has several launches: a launch on a secondary stream costs ~9 us more
        //  than a back-to-back launch on the main stream -- measured on single-chain fits)
        size_t max_ranges = 0;
        for (const auto &r : M.rangesF) max_ranges = std::max(max_ranges, r.size());
        for (const auto &r : M.rangesB) max_ranges = std::max(max_ranges, r.size());
        multistream = gp.fast && max_ranges >= 2;
        if (gp.wideH || gp.wideV) {
            any_hF.assign(T, 0); any_hB.assign(T, 0); any_vF.assign(T, 0); any_vB.assign(T, 0);
            for (int64_t t = 0; t < T; ++t)
                for (int64_t b = 0; b < B; ++b) {
                    if (gp.wideH && prog.tapF1[t * B + b] >= 0) any_hF[t] = 1;
                    if (gp.wideH && full && prog.tapB1[t * B + b] >= 0) any_hB[t] = 1;
                    if (gp.wideV && prog.tapF0[t * B + b] >= 0) any_vF[t] = 1;
                    if (gp.wideV && full && prog.tapB0[t * B + b] >= 0) any_vB[t] = 1;
                }
            ctx->hsrc.ensure((size_t)B * E.G * 8 * ((gp.wideH && gp.wideV) ? 2 : 1));
            d_hsrc = ctx->hsrc.as<double>();
            d_vsrc = (gp.wideH && gp.wideV) ? d_hsrc + (size_t)B * E.G : d_hsrc;
        }
        // both-axes launches: the matrix-pipe kernel wins while the launch is latency-bound (few cells per CU); with the chip
        // full the vector kernel's 2 x 17 FMAs per cell beat 2 x 32 band products (measured: 1024^2 12.7 vs 14.9 us,
        // 2048^2 30.0 vs 27.7 us, 4096^2 97 vs 77 us per forward step)
        mfma_h = ctx->option("mfma_h", 1.0) != 0.0;
        mfma_h_max_cells = ctx->option("mfma_h_max_cells", 2.5e6);
    }

    // the kernel-variant code of a pass that ran here: 3 where most of its launches went to the matrix pipe
    int variant(const BatchEnv &E, bool bwd) const { return (n_mfma[bwd] > 0 && n_mfma[bwd] >= n_fast[bwd]) ? 3 : (E.gp->fast ? 1 : 0); }

    void forward(const BatchEnv &E, double *d_psF) {
        const int64_t T = E.T, B = E.B;
        const long long G = E.G;
        const size_t slots = (size_t)B * NRED * E.tile.nblk;          // partial sums of one step
        fork_streams(E);
        for (int64_t t = 0; t < T; ++t) {
            if (multistream && t > 0 && !same_membership(E.M->h_orderF, E.M->rangesF, B, t - 1, t)) { join_streams(E); fork_streams(E); }
            const double *srcp; double *dstp; long long sstr, dstr;
            if (E.ff.evidence_only) {
                srcp = E.d_pp[(t + 1) & 1]; sstr = G; dstp = E.d_pp[t & 1]; dstr = G;
            } else {
                srcp = E.d_post + (t > 0 ? (size_t)(t - 1) * G : 0); sstr = (long long)T * G;
                dstp = E.d_post + (size_t)t * G; dstr = (long long)T * G;
            }
            if (t == 0 && E.ff.resume) { srcp = E.d_carry_src; sstr = G; }
            step(E, MODE_FWD, t, srcp, sstr, dstp, dstr, nullptr, 0,
                 t > 0 ? d_psF + (size_t)(t - 1) * slots : (E.ff.resume ? E.d_unit : d_psF), 0,
                 d_psF + (size_t)t * slots, E.ff.forward_only);
        }
        join_streams(E);
    }

    void backward(const BatchEnv &E, double *d_psB) {
        const int64_t T = E.T, B = E.B;
        const long long G = E.G;
        const size_t slots = (size_t)B * NRED * E.tile.nblk;
        fork_streams(E);
        for (int64_t t = T - 1; t >= 0; --t) {
            if (multistream && t < T - 1 && !same_membership(E.M->h_orderB, E.M->rangesB, B, t + 1, t)) { join_streams(E); fork_streams(E); }
            // reads c_{t+1} and the stored alpha_t, writes c_t and posterior_t
            step(E, MODE_BWD, t, E.d_pp[(t + 1) & 1], G, E.d_pp[t & 1], G, E.d_post + (size_t)t * G, (long long)T * G,
                 t < T - 1 ? d_psB + (size_t)(t + 1) * slots : d_psB, 2,
                 d_psB + (size_t)t * slots, true);
        }
        join_streams(E);
    }

private:
    void fork_streams(const BatchEnv &E) {
        if (!multistream) return;
        blhip_ctx *ctx = E.ctx;
        HIPCHECK(hipEventRecord(ctx->fork_ev, E.st));
        for (auto &bs : ctx->bstream) HIPCHECK(hipStreamWaitEvent(bs, ctx->fork_ev, 0));
    }
    void join_streams(const BatchEnv &E) {
        if (!multistream) return;
        blhip_ctx *ctx = E.ctx;
        for (int k = 0; k < blhip_ctx::NBS; ++k) {
            HIPCHECK(hipEventRecord(ctx->bev[k], ctx->bstream[k]));
            HIPCHECK(hipStreamWaitEvent(E.st, ctx->bev[k], 0));
        }
    }
    // a chain only depends on its own previous step: streams need a barrier only where bucket membership changes
    static bool same_membership(const std::vector<int> &order, const std::vector<std::vector<FastRange>> &ranges, int64_t B,
                                int64_t ta, int64_t tb) {
        if (ranges[ta].size() != ranges[tb].size()) return false;
        for (size_t k = 0; k < ranges[ta].size(); ++k)
            if (ranges[ta][k].key != ranges[tb][k].key || ranges[ta][k].count != ranges[tb][k].count) return false;
        return std::equal(order.begin() + ta * B, order.begin() + (ta + 1) * B, order.begin() + tb * B);
    }

    void step(const BatchEnv &E, int mode, int64_t t, const double *srcp, long long src_stride, double *dstp, long long dst_stride,
              double *postp, long long post_stride, const double *ps_prev, int prev_slot, double *ps_out, bool means) {
        if (E.gp->fast) step_fast(E, mode, t, srcp, src_stride, dstp, dst_stride, postp, post_stride, ps_prev, prev_slot, ps_out);
        else step_generic(E, mode, t, srcp, src_stride, dstp, dst_stride, postp, post_stride, ps_prev, prev_slot, ps_out, means);
    }

    // one launch per radius bucket of the step (fast or matrix-pipe kernel), behind the bucket's wide pre-passes
    void step_fast(const BatchEnv &E, int mode, int64_t t, const double *srcp, long long src_stride, double *dstp, long long dst_stride,
                   double *postp, long long post_stride, const double *ps_prev, int prev_slot, double *ps_out) {
        blhip_ctx *ctx = E.ctx;
        const blhip_problem *p = E.p;
        const GeometryPlan &gp = *E.gp;
        const ChainProgram &prog = *E.prog;
        const TapTable &taps = *E.taps;
        const DeviceMeta &M = *E.M;
        const Geometry &g = E.g;
        const int64_t B = E.B;
        const long long G = E.G;
        const double *d_lik = E.DT->lik;
        const bool bw = mode != MODE_FWD;
        blf::FastParams Q = FP;
        Q.src = srcp; Q.src_stride = src_stride; Q.dst = dstp; Q.dst_stride = dst_stride;
        Q.post = postp; Q.post_stride = post_stride;
        Q.srckind = (bw ? M.kindB : M.kindF) + t * B;
        Q.tap0 = (bw ? M.tapB0 : M.tapF0) + t * B;
        Q.tap1 = (bw ? M.tapB1 : M.tapF1) + t * B;
        Q.psum_prev = ps_prev; Q.prev_slot = prev_slot; Q.psum_out = ps_out;
        Q.rec = E.DT->rec + t * E.rec_len; Q.lik = d_lik ? d_lik + (size_t)t * G : nullptr;
        const int *ord = (bw ? M.orderB : M.orderF) + t * B;
        const bool prepass_step = gp.wideH && (bw ? any_hB : any_hF)[t];
        const bool prepass_v = gp.wideV && (bw ? any_vB : any_vF)[t];
        for (const FastRange &r : (bw ? M.rangesB[t] : M.rangesF[t])) {
            Q.chain_ids = ord + r.start;
            Q.u_valid = 0;
            Q.hsrc = nullptr;
            const bool prepass = prepass_step && r.pre;
            if (r.count == 1) {      // single-chain launch: hand the chain's metadata over by value
                const int64_t tb = t * B;
                const int cb = (bw ? M.h_orderB : M.h_orderF)[tb + r.start];
                const int k0 = (bw ? prog.tapB0 : prog.tapF0)[tb + cb];
                const int k1 = (bw ? prog.tapB1 : prog.tapF1)[tb + cb];
                Q.u_valid = 1; Q.u_chain = cb; Q.u_kind = (bw ? prog.kindB : prog.kindF)[tb + cb];
                Q.u_t0 = k0; Q.u_lw0 = k0 >= 0 ? taps.lw[k0] : 0; Q.u_off0 = k0 >= 0 ? taps.off[k0] : 0;
                Q.u_t1 = k1; Q.u_lw1 = k1 >= 0 ? taps.lw[k1] : 0; Q.u_off1 = k1 >= 0 ? taps.off[k1] : 0;
            }
            hipStream_t ls = multistream ? ctx->bstream[r.key] : E.st;
            if (prepass) {
                // row filter of the bucket's chains -> hsrc, on the bucket's stream: the launch below consumes it instead of its
                // sources; the buckets' streams overlap one bucket's (HBM-bound) pre-pass with another's (matrix-pipe-bound) step
                blh::HParams HP{};
                HP.n0 = g.n0; HP.n1 = g.n1; HP.tiles_j = (g.n1 + blh::CB - 1) / blh::CB; HP.lwmax = prog.LW1; HP.pitch = blh::pitch_for(prog.LW1);
                HP.src = srcp; HP.src_stride = src_stride;
                for (int k = 0; k < 5; ++k) HP.shared[k] = FP.shared[k];
                HP.chain_ids = Q.chain_ids;
                HP.srckind = Q.srckind; HP.tap1 = Q.tap1; HP.taps = M.taps; HP.tap_off = M.off; HP.tap_lw = M.lw; HP.dst = d_hsrc;
                launch_hwide(ls, HP, r.count);
                Q.hsrc = d_hsrc;
                account(ctx, bw, (double)r.count * G * 16.0, (double)r.count * G * 2.0 * (2.0 * prog.LW1 + 8.0));
            }
            if (prepass_v) {
                // column filter of the bucket's chains (after the row filter, if there is one) -> the launch below runs without a stencil
                blh::HParams VP{};
                VP.n0 = g.n0; VP.n1 = g.n1; VP.tiles_j = (g.n1 + blh::CV - 1) / blh::CV; VP.lwmax = prog.LW0;
                VP.src = srcp; VP.src_stride = src_stride; VP.presrc = Q.hsrc;
                for (int k = 0; k < 5; ++k) VP.shared[k] = FP.shared[k];
                VP.chain_ids = Q.chain_ids;
                VP.srckind = Q.srckind; VP.tap1 = Q.tap0; VP.taps = M.taps; VP.tap_off = M.off; VP.tap_lw = M.lw; VP.dst = d_vsrc;
                launch_vwide(ls, VP, r.count);
                Q.hsrc = d_vsrc;
                account(ctx, bw, (double)r.count * G * 16.0, (double)r.count * G * 2.0 * (2.0 * prog.LW0 + 8.0));
            }
            const bool on_pipe = gp.use_mfma && (r.H ? (mfma_h && (double)r.count * g.n0 * g.n1 <= mfma_h_max_cells) : r.R0 >= mfma_min_r0);
            if (on_pipe) { launch_mfma(ls, p->obs_model, mode, Q, r.R0, r.H, r.count); ++n_mfma[bw ? 1 : 0]; }
            else { launch_fast(ls, p->obs_model, mode, Q, r.R0, r.H, r.count); ++n_fast[bw ? 1 : 0]; }
            // streaming kernels: state in, state out (+ stored alpha in, posterior out backward; + a tabulated likelihood)
            const double fl = (on_pipe ? (r.R0 > 0 ? band_stencil_flop(r.R0) : 0.0) + (r.H ? band_stencil_flop(8) : 0.0)
                                       : valu_stencil_flop(r.R0) + (r.H ? valu_stencil_flop(8) : 0.0)) + (bw ? EPI_BWD_FLOP : EPI_FWD_FLOP);
            account(ctx, bw, (double)r.count * G * ((bw ? 32.0 : 16.0) + (d_lik ? 8.0 : 0.0)), (double)r.count * G * fl);
        }
    }

    // the generic step kernel, behind the stages of a composed transition
    void step_generic(const BatchEnv &E, int mode, int64_t t, const double *srcp, long long src_stride, double *dstp, long long dst_stride,
                      double *postp, long long post_stride, const double *ps_prev, int prev_slot, double *ps_out, bool means) {
        blhip_ctx *ctx = E.ctx;
        const ChainProgram &prog = *E.prog;
        const DeviceMeta &M = *E.M;
        const int64_t B = E.B;
        const long long G = E.G;
        const double *d_lik = E.DT->lik;
        const bool bw = mode != MODE_FWD;
        StepParams Q = P;
        Q.src = srcp; Q.src_stride = src_stride; Q.dst = dstp; Q.dst_stride = dst_stride;
        Q.post = postp; Q.post_stride = post_stride;
        Q.srckind = (bw ? M.kindB : M.kindF) + t * B;
        Q.tap0 = (bw ? M.tapB0 : M.tapF0) + t * B;
        Q.tap1 = (bw ? M.tapB1 : M.tapF1) + t * B;
        Q.cmode = prog.has_clamp ? (bw ? M.cmodeB : M.cmodeF) + t * B : nullptr;
        Q.limit = prog.has_clamp ? (bw ? M.limitB : M.limitF) + t * B : nullptr;
        Q.psum_prev = ps_prev; Q.prev_slot = prev_slot; Q.psum_out = ps_out;
        Q.rec = E.DT->rec + t * E.rec_len; Q.lik = d_lik ? d_lik + (size_t)t * G : nullptr;
        // composed transitions: the stages in front of the last one, each reading the one before (the first: the step's source), then
        // the fused kernel reads the last stage's output and partials the way it reads a state's (DESIGN.md "Composed transitions")
        const int nst = prog.multi ? (bw ? prog.nstB : prog.nstF)[t] : 0;
        for (int s2 = 0; s2 < nst; ++s2) {
            StepParams S = Q;
            const size_t e = (bw ? prog.offB : prog.offF)[t] + (size_t)s2 * B;
            S.src = s2 == 0 ? srcp : SM.out[(s2 - 1) & 1]; S.src_stride = s2 == 0 ? src_stride : G;
            S.dst = SM.out[s2 & 1]; S.dst_stride = G; S.post = nullptr; S.post_stride = 0;
            S.srckind = (bw ? SM.kindB : SM.kindF) + e;
            S.tap0 = (bw ? SM.tapB0 : SM.tapF0) + e; S.tap1 = (bw ? SM.tapB1 : SM.tapF1) + e;
            S.cmode = (bw ? SM.cmodeB : SM.cmodeF) + e; S.limit = (bw ? SM.limitB : SM.limitF) + e;
            S.psum_prev = s2 == 0 ? ps_prev : SM.ps[(s2 - 1) & 1]; S.psum_out = SM.ps[s2 & 1];
            S.rec = nullptr; S.lik = nullptr;
            // (chains whose stage is a large shift of a 2-D grid are blk::bigshift_kernel's, one launch per shifted axis; every
            //  kernel skips the chains that are not its own, and a launch is issued only if some chain needs it)
            const int *big = &(bw ? big_stageB : big_stageF)[2 * (e / (size_t)B)];
            const int64_t n_other = B - big[0] - big[1];
            if (n_other > 0) {
                launch_stage(E.st, S, E.tile, (int)B, bw);
                account(ctx, bw, (double)n_other * G * 16.0, (double)n_other * G * (valu_stencil_flop(prog.LW0) + valu_stencil_flop(prog.LW1)));
            }
            for (int ax = 0; ax < 2; ++ax)
                if (big[ax] > 0) {
                    launch_bigshift(E.st, S, ax, (int)B, bw);
                    account(ctx, bw, (double)big[ax] * G * 16.0, (double)big[ax] * G * BIGSHIFT_FLOP);
                }
        }
        if (nst > 0) { Q.src = SM.out[(nst - 1) & 1]; Q.src_stride = G; Q.psum_prev = SM.ps[(nst - 1) & 1]; }
        launch_step(E.st, E.p->obs_model, Q, E.tile, (int)B, mode, means);
        account(ctx, bw, (double)B * G * ((bw ? 32.0 : 16.0) + (d_lik ? 8.0 : 0.0)),
                (double)B * G * (valu_stencil_flop(prog.LW0) + valu_stencil_flop(prog.LW1) + (bw ? EPI_BWD_FLOP : EPI_FWD_FLOP)));
    }
};
