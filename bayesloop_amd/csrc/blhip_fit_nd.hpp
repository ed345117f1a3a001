// Host side of the plain N-D path (kernels: blhip_nd.hpp, blhip_nd_stages.hpp, blhip_chain_nd.hpp), laid out as do_fit's is: shared tables,
// batch plan, the metadata of a batch, NdEnv -- what the paths read of a batch --, the launch-per-step path (nd_step, nd_step_pass) and the
// chain-resident one (NdChainRun), the end of a pass, and do_fit_nd: prologue, batch loop, tail.  The transition program of a batch is
// built by blhip_nd_program.hpp, which needs no HIP call.  Included by blhip.hip INSIDE its anonymous namespace, after the helpers it uses
// (FitFlags, carry_source, upload_unit_sums, BatchOutcome, forward_ / backward_bookkeeping, fold_accumulate, keep_posterior, write_results).
#pragma once

// the chain-resident kernel of a batch (blhip_chain_nd.hpp): one block per chain, the small or the large block by the LDS need
template <int NT>
void launch_chain_nd_t(hipStream_t s, const bln::ChainNd &Q, bool bwd, size_t lds) {
    if (bwd) {
        arm_kernel(reinterpret_cast<const void *>(&bln::chain_nd_kernel<true, NT>));
        BL_LAUNCH((bln::chain_nd_kernel<true, NT>), dim3((unsigned)Q.B), dim3(NT), lds, s, Q);
    } else {
        arm_kernel(reinterpret_cast<const void *>(&bln::chain_nd_kernel<false, NT>));
        BL_LAUNCH((bln::chain_nd_kernel<false, NT>), dim3((unsigned)Q.B), dim3(NT), lds, s, Q);
    }
}
// ... and its stage flavour (NotEqual / Deterministic passes, resumed and carried fits)
template <int NT>
void launch_chain_nd_stage_t(hipStream_t s, const bln::ChainNd &Q, bool bwd, size_t lds) {
    if (bwd) {
        arm_kernel(reinterpret_cast<const void *>(&bln::chain_nd_stage_kernel<true, NT>));
        BL_LAUNCH((bln::chain_nd_stage_kernel<true, NT>), dim3((unsigned)Q.B), dim3(NT), lds, s, Q);
    } else {
        arm_kernel(reinterpret_cast<const void *>(&bln::chain_nd_stage_kernel<false, NT>));
        BL_LAUNCH((bln::chain_nd_stage_kernel<false, NT>), dim3((unsigned)Q.B), dim3(NT), lds, s, Q);
    }
}
void launch_chain_nd(hipStream_t s, const bln::ChainNd &Q, bool bwd, int threads, size_t lds, bool stages = false) {
    if (lds > bln::CHAIN_ND_LDS_LIMIT || Q.g.G > (long long)threads * bln::chain_nd_cpt(threads))
        fail("internal: chain-resident N-D kernel: %zu bytes of LDS, %lld cells on %d threads", lds, Q.g.G, threads);
    if (stages) {
        if (threads == bln::CHAIN_ND_NT_SMALL) launch_chain_nd_stage_t<bln::CHAIN_ND_NT_SMALL>(s, Q, bwd, lds);
        else launch_chain_nd_stage_t<bln::CHAIN_ND_NT_LARGE>(s, Q, bwd, lds);
    } else if (threads == bln::CHAIN_ND_NT_SMALL) launch_chain_nd_t<bln::CHAIN_ND_NT_SMALL>(s, Q, bwd, lds);
    else launch_chain_nd_t<bln::CHAIN_ND_NT_LARGE>(s, Q, bwd, lds);
    HIPCHECK(hipGetLastError());
}

// ---- what every chain of the call shares: marginals (in NdGrid), prior(s), uniform, the likelihood table ---------------------------------
struct NdTables {
    double *prior, *reset, *uniform, *indep, *lik;   // indep: null without an Independent model
};

NdTables upload_nd_tables(blhip_ctx *ctx, const blhip_problem *p, bln::NdGrid &ng) {
    hipStream_t st = ctx->stream;
    const int64_t T = p->T;
    const long long G = ng.G;
    NdTables D{};
    size_t msum = 0;
    for (int k = 0; k < p->ndim; ++k) msum += carve_size(8 * (size_t)p->n[k]);
    ctx->tables.ensure(msum + (p->indep_prior ? 4 : 3) * carve_size(8 * (size_t)G));
    char *cur = ctx->tables.as<char>();
    for (int k = 0; k < p->ndim; ++k) {
        double *dm = carve<double>(cur, (size_t)p->n[k]);
        HIPCHECK(hipMemcpyAsync(dm, p->marginal[k], 8 * (size_t)p->n[k], hipMemcpyHostToDevice, st));
        ng.m[k] = dm;
    }
    D.prior = carve<double>(cur, (size_t)G); D.reset = carve<double>(cur, (size_t)G); D.uniform = carve<double>(cur, (size_t)G);
    HIPCHECK(hipMemcpyAsync(D.prior, p->prior, 8 * (size_t)G, hipMemcpyHostToDevice, st));
    if (p->reset_prior) HIPCHECK(hipMemcpyAsync(D.reset, p->reset_prior, 8 * (size_t)G, hipMemcpyHostToDevice, st));
    if (p->backward_init) HIPCHECK(hipMemcpyAsync(D.uniform, p->backward_init, sizeof(double) * G, hipMemcpyHostToDevice, st));
    else BL_LAUNCH(fill_kernel, dim3(256), dim3(256), 0, st, D.uniform, G, 1.0 / (double)G);           // beta_T = 1/G, core.py:424-425
    if (p->indep_prior) {                             // Independent restarts from it at every step: sum 1, consumed with scale 1 (transitionModels.py:351-360)
        D.indep = carve<double>(cur, (size_t)G);
        HIPCHECK(hipMemcpyAsync(D.indep, p->indep_prior, 8 * (size_t)G, hipMemcpyHostToDevice, st));
    }
    ctx->likbuf.ensure(8 * (size_t)T * G);
    D.lik = ctx->likbuf.as<double>();
    if (p->obs_model == BLHIP_OM_PROGRAM) build_program_table(ctx, p->ndim, p->n, ng.m, T, p->data_dim, p->data, D.lik);
    else HIPCHECK(hipMemcpyAsync(D.lik, p->lik, 8 * (size_t)T * G, hipMemcpyHostToDevice, st));
    sync_stream(ctx, st);
    return D;
}

// memory plan: how many chains fit one batch (three state arrays + the stored sequence + partial sums per chain within the budget)
int64_t nd_chains_per_batch(blhip_ctx *ctx, const FitFlags &ff, int64_t n_chains, int64_t T, long long G) {
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min((double)free_b + (double)ctx->state.cap + (double)ctx->post.cap, 0.70 * (double)total_b) * 0.9;
    const double per_chain = ((ff.evidence_only ? 0.0 : (double)T) + 3.0) * (double)G * 8.0 + (double)T * NRED * 8.0 * 2 * 256.0;
    int64_t Bmax = (int64_t)std::max(1.0, std::floor(budget / per_chain));
    Bmax = std::min<int64_t>(std::min<int64_t>(Bmax, (int64_t)ctx->option("max_batch", 1024)), 65535);
    if (ff.keep && n_chains > Bmax) fail("BLHIP_KEEP_POSTERIOR: %lld chains do not fit in device memory at once", (long long)n_chains);
    if ((ff.resume || ff.carry) && n_chains > Bmax) fail("carried states: %lld chains do not fit in one batch", (long long)n_chains);
    return Bmax;
}

// ---- per-(step, chain) metadata of a batch in HBM: the program, where a step's input lives, scratch of the stages and of the tail ------
struct NdMeta {
    unsigned char *kindF, *kindB;
    int *tapF, *tapB;
    double *taps;
    int *off, *lw;
    const double **src0F, **src0B;                   // [t][b] a step's input: the chain's state, or a shared distribution at a restart
    const double **ptr_state, **ptr_tmp0, **ptr_tmp1;
    double *w, *invN;                                // (store_carry, fold_accumulate)
    // the stages' scratch (blhip_nd_stages.hpp): NotEqual's limits, block maxima and block sums, the partial sums of a stage's output
    double *limit, *bmax, *bsum, *stage_sums;

    // the carving walk; base = nullptr: run dry -> the bytes it takes
    size_t lay_out(char *base, const NdBatchProgram &P, size_t nT, int64_t B, int nblk, bool has_stage) {
        size_t at = 0;
        auto take = [&](auto *&ptr, size_t count) {
            ptr = base ? reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(base + at) : nullptr;
            at += carve_size(count * sizeof(*ptr));
        };
        const size_t ntap = P.taps.off.size() + 1;
        take(kindF, nT); take(kindB, nT);
        take(tapF, P.tapF.size()); take(tapB, P.tapB.size());
        take(taps, P.taps.w.size());
        take(off, ntap); take(lw, ntap);
        take(src0F, nT); take(src0B, nT);
        take(ptr_state, (size_t)B); take(ptr_tmp0, (size_t)B); take(ptr_tmp1, (size_t)B);
        take(w, (size_t)B); take(invN, nT);
        limit = bmax = bsum = stage_sums = nullptr;
        if (has_stage) {
            take(limit, P.limit.size()); take(bmax, (size_t)B * nblk); take(bsum, (size_t)B * nblk);
            take(stage_sums, (size_t)B * NRED * nblk);
        }
        return at;
    }
};

// what the paths of a batch read of it
struct NdEnv {
    blhip_ctx *ctx; const blhip_problem *p; hipStream_t st;
    FitFlags ff;
    bln::NdGrid ng; long long G; int64_t T, B;
    int nblk;                                        // blocks per chain of the launch-per-step kernels
    const NdFacts *F; const NdBatchProgram *prog;
    NdTables DT; NdMeta M;
    double *d_state, *d_tmp[2];                      // the chains' states and the two scratch arrays of the passes, B x G each (launch per step)
    double *d_post;                                  // the batch's sequence buffer (null: evidence-only)
    const double *d_carry_src, *d_unit;              // BLHIP_RESUME: the carried states, and "previous partial sums" that add up to 1
};

// carve + upload.  chain_nd: the batch keeps its state in LDS -- no tables of where a step's input lives
void upload_nd_meta(NdEnv &E, bool chain_nd) {
    blhip_ctx *ctx = E.ctx;
    hipStream_t st = E.st;
    const NdBatchProgram &P = *E.prog;
    const NdTables &D = E.DT;
    NdMeta &M = E.M;
    const int64_t T = E.T, B = E.B;
    const long long G = E.G;
    const size_t nT = (size_t)T * B;
    const bool has_stage = E.F->has_stage;
    const size_t mb = M.lay_out(nullptr, P, nT, B, E.nblk, has_stage);
    ctx->meta.ensure(mb);
    M.lay_out(ctx->meta.as<char>(), P, nT, B, E.nblk, has_stage);
    if (has_stage) HIPCHECK(hipMemcpyAsync(M.limit, P.limit.data(), P.limit.size() * 8, hipMemcpyHostToDevice, st));
    std::vector<const double *> src0F(chain_nd ? 0 : nT), src0B(chain_nd ? 0 : nT), pst(B), pt0(B), pt1(B);
    for (int64_t b = 0; !chain_nd && b < B; ++b) {
        pst[b] = E.d_state + (size_t)b * G; pt0[b] = E.d_tmp[0] + (size_t)b * G; pt1[b] = E.d_tmp[1] + (size_t)b * G;
        for (int64_t t = 0; t < T; ++t) {
            const size_t k = (size_t)t * B + b;
            const unsigned char kf = P.kindF[k], kb = P.kindB[k];
            src0F[k] = kf == SRC_PREV ? ((t == 0 && E.ff.resume) ? E.d_carry_src + (size_t)b * G : pst[b])
                                      : (kf == SRC_PRIOR ? D.prior : (kf == SRC_INDEP ? D.indep : D.reset));
            src0B[k] = kb == SRC_PREV ? pst[b] : (kb == SRC_UNIFORM ? D.uniform : (kb == SRC_INDEP ? D.indep : D.reset));
        }
    }
    // (the chain-resident kernel loads by the source kind and knows itself whether its chain ran a stage)
    HIPCHECK(hipMemcpyAsync(M.kindF, (has_stage && !chain_nd ? P.stepKF : P.kindF).data(), nT, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(M.kindB, (has_stage && !chain_nd ? P.stepKB : P.kindB).data(), nT, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(M.tapF, P.tapF.data(), P.tapF.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(M.tapB, P.tapB.data(), P.tapB.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(M.taps, P.taps.w.data(), P.taps.w.size() * 8, hipMemcpyHostToDevice, st));
    if (!P.taps.off.empty()) {
        HIPCHECK(hipMemcpyAsync(M.off, P.taps.off.data(), P.taps.off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.lw, P.taps.lw.data(), P.taps.lw.size() * 4, hipMemcpyHostToDevice, st));
    }
    if (!chain_nd) {
        HIPCHECK(hipMemcpyAsync(M.src0F, src0F.data(), nT * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.src0B, src0B.data(), nT * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.ptr_state, pst.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.ptr_tmp0, pt0.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.ptr_tmp1, pt1.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
    }
    sync_stream(ctx, st);
}

// ---- the launch-per-step path: per time step the passes of the transition, then the fused elementwise kernel -----------------------------
void nd_step(const NdEnv &E, bool bwd, int64_t t, const double *ps_prev, double *ps_out) {
    const NdMeta &M = E.M;
    const NdFacts &F = *E.F;
    hipStream_t st = E.st;
    const int64_t B = E.B, T = E.T;
    const long long G = E.G;
    const int nblk = E.nblk;
    const size_t nT = (size_t)T * B;
    const double *const *in = (bwd ? M.src0B : M.src0F) + (size_t)t * B;
    const int *tp = (bwd ? M.tapB : M.tapF) + (size_t)t * B;
    const std::vector<int> &htp = bwd ? E.prog->tapB : E.prog->tapF;
    int flip = 0;
    // whose partial sums the fused kernel reads its scale from: the producing step's, or those of the step's last stage
    const double *ps_scale = ps_prev;
    int scale_slot = bwd ? 2 : 0;
    for (int q = 0; q < F.npass; ++q) {
        bool any = false;
        for (int64_t b = 0; b < B && !any; ++b) any = htp[(size_t)q * nT + (size_t)t * B + b] >= 0;
        if (!any) continue;
        const blhip_op &op = E.p->ops[F.pass_ops[q]];
        const int ax = op.axis;
        const dim3 grid((unsigned)nblk, (unsigned)B);
        const int *id = tp + (size_t)q * nT;
        double *out = E.d_tmp[flip];
        if (op.kind == BLHIP_OP_GRW) {
            BL_LAUNCH(bln::filter_axis_kernel, grid, dim3(NTHREADS), 0, st, out, in, G, E.ng.n[ax], E.ng.stride[ax], id, M.taps, M.off, M.lw);
        } else if (op.kind == BLHIP_OP_NOTEQUAL) {
            BL_LAUNCH(bln::ne_max_kernel, grid, dim3(NTHREADS), 0, st, in, G, id, M.bmax);
            BL_LAUNCH(bln::ne_invert_kernel, grid, dim3(NTHREADS), 0, st, out, in, G, id, M.bmax, M.bsum);
            BL_LAUNCH(bln::ne_clamp_kernel, grid, dim3(NTHREADS), 0, st, out, G, id, M.limit + (size_t)q * B, M.bsum, ps_scale, scale_slot, M.stage_sums);
            ps_scale = M.stage_sums; scale_slot = 0;
        } else {
            BL_LAUNCH(bln::shift_axis_kernel, grid, dim3(NTHREADS), 0, st, out, in, G, E.ng.n[ax], E.ng.stride[ax], id, M.taps, M.off, M.lw, ps_scale,
                      scale_slot, M.stage_sums);
            ps_scale = M.stage_sums; scale_slot = 0;
        }
        in = flip ? M.ptr_tmp1 : M.ptr_tmp0;
        flip ^= 1;
    }
    bln::NdStep Q{};
    Q.g = E.ng; Q.B = (int)B; Q.T = (int)T; Q.nblk = nblk; Q.srcs = in; Q.kind = (bwd ? M.kindB : M.kindF) + (size_t)t * B;
    Q.psum_prev = ps_scale; Q.prev_slot = scale_slot; Q.psum_out = ps_out; Q.lik = E.DT.lik + (size_t)t * G; Q.state = E.d_state;
    Q.post = E.d_post ? E.d_post + (size_t)t * G : nullptr; Q.post_stride = (long long)T * G;
    if (bwd) BL_LAUNCH(bln::step_kernel<true>, dim3((unsigned)nblk, (unsigned)B), dim3(NTHREADS), 0, st, Q);
    else BL_LAUNCH(bln::step_kernel<false>, dim3((unsigned)nblk, (unsigned)B), dim3(NTHREADS), 0, st, Q);
}
// a pass: forward (core.py:372-411) step 0 reads the unit sums of a resumed fit, backward (core.py:424-470) step T - 1 reads no scale
void nd_step_pass(const NdEnv &E, bool bwd, double *d_ps) {
    const int64_t T = E.T;
    const size_t per_step = (size_t)E.B * NRED * E.nblk;
    if (!bwd) for (int64_t t = 0; t < T; ++t) nd_step(E, false, t, t > 0 ? d_ps + (size_t)(t - 1) * per_step : (E.d_unit ? E.d_unit : d_ps), d_ps + (size_t)t * per_step);
    else for (int64_t t = T - 1; t >= 0; --t) nd_step(E, true, t, t < T - 1 ? d_ps + (size_t)(t + 1) * per_step : d_ps, d_ps + (size_t)t * per_step);
}

// ---- the chain-resident path (blhip_chain_nd.hpp): every step of every chain of the batch in one launch per pass --------------------------
struct NdChainRun {
    bool on = false;
    bool stages = false;                             // the stage flavour: a batch with NotEqual / Deterministic passes, a resumed or carried fit
    int slot = 0;                                    // ... doubles of one of its tap slots
    // A batch of walks and restarts that is neither resumed nor carried takes chain_nd_kernel; option chain_nd: 0 off, 1 the batches the
    // cost model gives it (at least CHAIN_ND_MIN_CHAINS chains), 2 wherever it fits.  A batch with stages, a resumed or a carried one takes
    // chain_nd_stage_kernel under the same option where chain_nd_stage_route admits it; option chain_nd_stages = 0 keeps those plain.
    void setup(blhip_ctx *ctx, const NdFacts &F, const NdBatchProgram &P, const FitFlags &ff, long long G, int64_t B) {
        stages = F.has_stage || ff.resume || ff.carry;
        const int cus = std::min(ctx->num_cus, 256);
        if (stages) {
            slot = bln::chain_nd_stage_slot(P.lw_walk_max, P.lw_shift_max);
            on = bln::chain_nd_stage_route((int)ctx->option("chain_nd", 1.0), (int)ctx->option("chain_nd_stages", 1.0),
                                           bln::chain_nd_stage_fits(G, slot, F.npass, F.n_sum), G, B, P.stage_filters, P.stage_W, P.stage_sweeps,
                                           P.stage_shifts, P.stage_beyond_axis, bln::chain_nd_stage_threads(G, slot, F.npass, F.n_sum), cus);
            return;
        }
        const bool program_ok = F.npass <= bln::CHAIN_ND_MAXPASS;
        on = bln::chain_nd_route((int)ctx->option("chain_nd", 1.0), program_ok && bln::chain_nd_fits(G, P.lw_max, F.npass, F.n_sum), G, B,
                                 program_ok ? P.walks_on : 0, program_ok ? P.W_taps : 0, program_ok && P.beyond_axis,
                                 bln::chain_nd_threads(G, P.lw_max, F.npass, F.n_sum), cus);
    }
    void pass(const NdEnv &E, bool bwd, double *ps) const {
        const NdFacts &F = *E.F;
        const NdMeta &M = E.M;
        const int lw_max = E.prog->lw_max;
        bln::ChainNd Q{};
        Q.g = E.ng; Q.B = (int)E.B; Q.T = (int)E.T; Q.npass = F.npass;
        for (int q = 0; q < F.npass; ++q) { const int ax = E.p->ops[F.pass_ops[q]].axis; Q.pass_n[q] = E.ng.n[ax]; Q.pass_inner[q] = (int)E.ng.stride[ax]; }
        Q.tap_slot = stages ? slot : lw_max + 1;
        Q.kind = bwd ? M.kindB : M.kindF; Q.tap = bwd ? M.tapB : M.tapF; Q.taps = M.taps; Q.tap_off = M.off; Q.tap_lw = M.lw;
        Q.shared[SRC_PREV] = nullptr; Q.shared[SRC_PRIOR] = E.DT.prior; Q.shared[SRC_RESET] = E.DT.reset; Q.shared[SRC_UNIFORM] = E.DT.uniform;
        Q.shared[SRC_INDEP] = E.DT.indep;
        Q.lik = E.DT.lik; Q.post = E.d_post; Q.post_stride = (long long)E.T * E.G; Q.psum = ps;
        if (stages) {
            for (int q = 0; q < F.npass; ++q) Q.pass_kind[q] = (unsigned char)F.pass_kind[q];
            Q.limit = M.limit;
            Q.carry_in = !bwd && E.ff.resume ? E.d_carry_src : nullptr;
            Q.carry_out = !bwd && E.ff.carry && !E.d_post ? E.d_state : nullptr;
            launch_chain_nd(E.st, Q, bwd, bln::chain_nd_stage_threads(E.G, slot, F.npass, F.n_sum),
                            bln::chain_nd_stage_lds_doubles(E.G, slot, F.npass, F.n_sum) * sizeof(double), true);
            return;
        }
        launch_chain_nd(E.st, Q, bwd, bln::chain_nd_threads(E.G, lw_max, F.npass, F.n_sum), bln::chain_nd_lds_doubles(E.G, lw_max, F.npass, F.n_sum) * sizeof(double));
    }
};

// One pass of a batch on the path that runs it, and its end: the `nb` partial sums per (step, chain, slot) are added up -- also when
// nb == 1, the chain-resident batches; period 0: every slot is a sum, slot 6 is the 4th parameter's mean here -- and travel to the
// page-locked buffer.  ev: the pair of events around the pass.  -> the sums on the host; ms: the pass on the device
double *run_nd_pass(const NdEnv &E, const NdChainRun &CR, bool bwd, hipEvent_t *ev, DevBuf &psum, DevBuf &red, PinBuf &pin, float &ms) {
    blhip_ctx *ctx = E.ctx;
    hipStream_t st = E.st;
    const size_t n_sums = (size_t)E.T * E.B * NRED;
    double *d_ps = psum.as<double>();
    HIPCHECK(hipEventRecord(ev[0], st));
    if (CR.on) CR.pass(E, bwd, d_ps);
    else nd_step_pass(E, bwd, d_ps);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev[1], st));
    BL_LAUNCH(reduce_partials_kernel, dim3((unsigned)n_sums), dim3(NTHREADS), 0, st, d_ps, red.as<double>(), CR.on ? 1 : E.nblk, 0);
    pin.ensure(n_sums * 8);
    double *h = pin.as<double>();
    HIPCHECK(hipMemcpyAsync(h, red.p, n_sums * 8, hipMemcpyDeviceToHost, st));
    sync_stream(ctx, st);
    HIPCHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    return h;
}

// ---- grids with 3 and 4 parameters: the plain formulation (blhip_nd.hpp), the chain-resident kernel for batches (blhip_chain_nd.hpp) -----
// (streaming fits -- OnlineStudy.step, core.py:2062-2226, which has no limit on the grid's dimensions: step 0 consumes the chains' carried
//  states through the transition evaluated at resume_time, the last step's filtered distributions are kept normalised)
void do_fit_nd(blhip_ctx *ctx, const blhip_problem *p, int64_t n_chains, const double *op_values, const double *log_w, uint32_t flags,
               blhip_result *res) {
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const FitFlags ff = decode_flags(ctx, p, flags, log_w);
    const int64_t T = p->T;
    bln::NdGrid ng{};
    ng.ndim = p->ndim;
    long long G = 1;
    for (int k = p->ndim - 1; k >= 0; --k) { ng.n[k] = (int)p->n[k]; ng.stride[k] = G; G *= p->n[k]; }
    ng.G = G;
    if (ff.accumulate && (ctx->acc_T != T || ctx->acc_G != G)) fail("accumulator shape mismatch");
    double dV = 1.0;
    for (int k = 0; k < p->ndim; ++k) dV *= p->lattice[k];
    ctx->post_valid = false;
    ctx->timing = blhip_timing{};
    hipEvent_t *ev = ctx->ev;
    HIPCHECK(hipEventRecord(ev[6], st));

    const NdTables DT = upload_nd_tables(ctx, p, ng);
    const int64_t Bmax = nd_chains_per_batch(ctx, ff, n_chains, T, G);
    const double *d_carry_src = ff.resume ? carry_source(ctx, p, n_chains, G) : nullptr;
    const NdFacts F = nd_facts(p);
    nd_refuse_shifts(p, F, n_chains, op_values, ff.resume);
    ChainProgram no_clamp;                           // (the bookkeeping helpers only ask it for clamp modes)

    for (int64_t c0 = 0; c0 < n_chains; c0 += Bmax) {
        const int64_t B = std::min<int64_t>(Bmax, n_chains - c0);
        const size_t nT = (size_t)T * B;
        ctx->timing.batches += 1;
        ctx->timing.cells_per_launch = std::max<int64_t>(ctx->timing.cells_per_launch, B * G);
        ctx->timing.fwd_kernel_variant = ctx->timing.bwd_kernel_variant = 7;
        NdBatchProgram prog;
        build_nd_program(p, F, c0, B, op_values, ff.resume, dV, prog);
        NdChainRun CR;
        CR.setup(ctx, F, prog, ff, G, B);
        if (CR.on) ctx->timing.fwd_kernel_variant = ctx->timing.bwd_kernel_variant = 10;
        // ---- device buffers: a chain-resident batch keeps its state in LDS (no state / scratch arrays) and writes block totals -- one
        //      partial sum per (step, chain, slot)
        NdEnv E{};
        E.ctx = ctx; E.p = p; E.st = st; E.ff = ff; E.ng = ng; E.G = G; E.T = T; E.B = B; E.F = &F; E.prog = &prog; E.DT = DT;
        E.nblk = (int)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 256);
        E.d_carry_src = d_carry_src;
        if (!CR.on) ctx->state.ensure((size_t)3 * B * G * 8);
        else if (ff.carry && ff.evidence_only) ctx->state.ensure((size_t)B * G * 8);          // (no sequence: the kernel leaves the last states here)
        E.d_state = ctx->state.as<double>(); E.d_tmp[0] = E.d_state + (size_t)B * G; E.d_tmp[1] = E.d_state + (size_t)2 * B * G;
        if (!ff.evidence_only) { ctx->post.ensure((size_t)B * T * G * 8); E.d_post = ctx->post.as<double>(); }
        const size_t psz = nT * NRED * (CR.on ? 1 : E.nblk);
        ctx->psumF.ensure(psz * 8); ctx->redF.ensure(nT * NRED * 8);
        if (ff.full) { ctx->psumB.ensure(psz * 8); ctx->redB.ensure(nT * NRED * 8); }
        upload_nd_meta(E, CR.on);
        if (ff.resume && !CR.on) E.d_unit = upload_unit_sums(ctx, p, st, B, E.nblk, false);       // (the kernel starts from tot = 1)

        float ms = 0;
        double *redF = run_nd_pass(E, CR, false, ev, ctx->psumF, ctx->redF, ctx->pinF, ms);
        ctx->timing.forward_ms += ms; ctx->timing.forward_launches += CR.on ? 1 : T;
        BatchOutcome O;
        forward_bookkeeping(p, no_clamp, redF, B, dV, false, 1, ff.evidence_only, ff.forward_only, O);
        O.invN.assign(nT, 0.0);
        if (ff.full) {
            double *redB = run_nd_pass(E, CR, true, ev + 2, ctx->psumB, ctx->redB, ctx->pinB, ms);
            ctx->timing.backward_ms += ms; ctx->timing.backward_launches += CR.on ? 1 : T;
            backward_bookkeeping(p, no_clamp, redF, redB, B, dV, false, -1, O);
        } else if (ff.forward_only) {
            for (int64_t b = 0; b < B; ++b)
                for (int64_t t = 0; t < T; ++t) O.invN[(size_t)b * T + t] = forward_invN(redF[((size_t)t * B + b) * NRED]);
        }
        // BLHIP_CARRY: every chain's filtered distribution of the last step, normalised (core.py:2173)
        if (ff.carry) store_carry(ctx, p, B, G, redF, E.d_post ? E.d_post + (size_t)(T - 1) * G : E.d_state, E.d_post ? (long long)T * G : G, E.M.w, false);
        if (ff.accumulate) fold_accumulate(ctx, T, G, B, O, log_w + c0, E.d_post, E.M.w, E.M.invN);
        if (ff.keep) {
            Geometry g2{};
            g2.n0 = (int)p->n[0]; g2.n1 = (int)(G / p->n[0]); g2.G = G;
            keep_posterior(ctx, g2, T, B, O, 0, T);
        }
        write_results(res, p, c0, B, O, !ff.evidence_only);
    }
    HIPCHECK(hipEventRecord(ev[7], st));
    HIPCHECK(hipEventSynchronize(ev[7]));
    float tot = 0;
    HIPCHECK(hipEventElapsedTime(&tot, ev[6], ev[7]));
    ctx->timing.total_ms = tot;
}
