// Host side of the plain N-D path (kernels: blhip_nd.hpp).  Included by blhip.hip INSIDE its anonymous namespace, after the helpers
// it uses (FitFlags, TapTable, BatchOutcome, forward_ / backward_bookkeeping, fold_accumulate, keep_posterior, write_results).
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
void launch_chain_nd(hipStream_t s, const bln::ChainNd &Q, bool bwd, int threads, size_t lds) {
    if (lds > bln::CHAIN_ND_LDS_LIMIT || Q.g.G > (long long)threads * bln::chain_nd_cpt(threads))
        fail("internal: chain-resident N-D kernel: %zu bytes of LDS, %lld cells on %d threads", lds, Q.g.G, threads);
    if (threads == bln::CHAIN_ND_NT_SMALL) launch_chain_nd_t<bln::CHAIN_ND_NT_SMALL>(s, Q, bwd, lds);
    else launch_chain_nd_t<bln::CHAIN_ND_NT_LARGE>(s, Q, bwd, lds);
    HIPCHECK(hipGetLastError());
}

// ---- grids with 3 and 4 parameters: the plain formulation (blhip_nd.hpp), the chain-resident kernel for batches (blhip_chain_nd.hpp) -----
void do_fit_nd(blhip_ctx *ctx, const blhip_problem *p, int64_t n_chains, const double *op_values, const double *log_w, uint32_t flags,
               blhip_result *res) {
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const FitFlags ff = decode_flags(ctx, p, flags, log_w);
    // (streaming fits -- OnlineStudy.step, core.py:2062-2226, which has no limit on the grid's dimensions: step 0 consumes the chains'
    //  carried states through the transition evaluated at resume_time, the last step's filtered distributions are kept normalised)
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

    // ---- shared tables: marginals, prior(s), uniform, the likelihood table -------------------------------------------------------
    size_t msum = 0;
    for (int k = 0; k < p->ndim; ++k) msum += carve_size(8 * (size_t)p->n[k]);
    ctx->tables.ensure(msum + (p->indep_prior ? 4 : 3) * carve_size(8 * (size_t)G));
    char *cur = ctx->tables.as<char>();
    for (int k = 0; k < p->ndim; ++k) {
        double *dm = carve<double>(cur, (size_t)p->n[k]);
        HIPCHECK(hipMemcpyAsync(dm, p->marginal[k], 8 * (size_t)p->n[k], hipMemcpyHostToDevice, st));
        ng.m[k] = dm;
    }
    double *d_prior = carve<double>(cur, (size_t)G), *d_reset = carve<double>(cur, (size_t)G), *d_uniform = carve<double>(cur, (size_t)G);
    HIPCHECK(hipMemcpyAsync(d_prior, p->prior, 8 * (size_t)G, hipMemcpyHostToDevice, st));
    if (p->reset_prior) HIPCHECK(hipMemcpyAsync(d_reset, p->reset_prior, 8 * (size_t)G, hipMemcpyHostToDevice, st));
    if (p->backward_init) HIPCHECK(hipMemcpyAsync(d_uniform, p->backward_init, sizeof(double) * G, hipMemcpyHostToDevice, st));
    else BL_LAUNCH(fill_kernel, dim3(256), dim3(256), 0, st, d_uniform, G, 1.0 / (double)G);           // beta_T = 1/G, core.py:424-425
    double *d_indep = nullptr;                        // Independent restarts from it at every step: sum 1, consumed with scale 1 (transitionModels.py:351-360)
    if (p->indep_prior) {
        d_indep = carve<double>(cur, (size_t)G);
        HIPCHECK(hipMemcpyAsync(d_indep, p->indep_prior, 8 * (size_t)G, hipMemcpyHostToDevice, st));
    }
    ctx->likbuf.ensure(8 * (size_t)T * G);
    double *d_lik = ctx->likbuf.as<double>();
    if (p->obs_model == BLHIP_OM_PROGRAM) build_program_table(ctx, p->ndim, p->n, ng.m, T, p->data_dim, p->data, d_lik);
    else HIPCHECK(hipMemcpyAsync(d_lik, p->lik, 8 * (size_t)T * G, hipMemcpyHostToDevice, st));
    sync_stream(ctx, st);

    // ---- batches ---------------------------------------------------------------------------------------------------------------------
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min((double)free_b + (double)ctx->state.cap + (double)ctx->post.cap, 0.70 * (double)total_b) * 0.9;
    const double per_chain = ((ff.evidence_only ? 0.0 : (double)T) + 3.0) * (double)G * 8.0 + (double)T * NRED * 8.0 * 2 * 256.0;
    int64_t Bmax = (int64_t)std::max(1.0, std::floor(budget / per_chain));
    Bmax = std::min<int64_t>(std::min<int64_t>(Bmax, (int64_t)ctx->option("max_batch", 1024)), 65535);
    if (ff.keep && n_chains > Bmax) fail("BLHIP_KEEP_POSTERIOR: %lld chains do not fit in device memory at once", (long long)n_chains);
    if ((ff.resume || ff.carry) && n_chains > Bmax) fail("carried states: %lld chains do not fit in one batch", (long long)n_chains);
    const double *d_carry_src = nullptr;
    if (ff.resume) {
        auto it = ctx->carry.find(p->carry_slot);
        if (it == ctx->carry.end() || !it->second.valid) fail("BLHIP_RESUME: carry slot %d holds no state", p->carry_slot);
        if (it->second.chains != n_chains || it->second.G != G)
            fail("BLHIP_RESUME: carry slot %d holds %lld chains x %lld cells, the call has %lld x %lld", p->carry_slot,
                 (long long)it->second.chains, (long long)it->second.G, (long long)n_chains, (long long)G);
        d_carry_src = it->second.buf.as<double>();
    }
    const int nblk = (int)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 256);
    // the ops of the program that launch passes, in list order (transitionModels.py:645-649): the random walks (one filter pass each) and
    // the renormalising stages of blhip_nd_stages.hpp (NotEqual: three passes, Deterministic: one)
    std::vector<int> pass_ops;
    bool time_dependent = false, has_stage = false, has_shift = false;
    for (int k = 0; k < p->n_ops; ++k) {
        const int kind = p->ops[k].kind;
        if (kind == BLHIP_OP_GRW || kind == BLHIP_OP_NOTEQUAL || kind == BLHIP_OP_DETERMINISTIC) pass_ops.push_back(k);
        if (kind == BLHIP_OP_NOTEQUAL || kind == BLHIP_OP_DETERMINISTIC) has_stage = true;
        if (kind == BLHIP_OP_DETERMINISTIC) has_shift = true;
        if (kind == BLHIP_OP_CHANGEPOINT || kind == BLHIP_OP_BREAKPOINT || kind == BLHIP_OP_DETERMINISTIC) time_dependent = true;
    }
    const int npass = (int)pass_ops.size();
    // the time stamp the transition INTO step t is evaluated at; false: the step consumes a shared distribution, no transition
    //   forward: T_fwd(post_{t-1}, ts[t-1]), core.py:411 (step 0 of a resumed fit: at resume_time, core.py:2164-2165)
    //   backward: T_bwd(beta_{t+1} L_{t+1}, ts[t+1]) = T_fwd(., ts[t+1] - 1), core.py:467, transitionModels.py:316-317
    auto stamp = [&](int64_t t, bool fwd, double &tau) {
        if (fwd) {
            if (t == 0 && !ff.resume) return false;
            tau = t == 0 ? p->resume_time : p->timestamps[t - 1];
        } else {
            if (t == T - 1) return false;
            tau = p->timestamps[t + 1] - 1.0;
        }
        return true;
    };
    // active sub-model of a serial model at tau: the number of boundary values at or before it (transitionModels.py:768)
    auto segment_at = [&](const double *val, double tau) {
        int seg = 0;
        for (int k = 0; k < p->n_ops; ++k) {
            const blhip_op &op = p->ops[k];
            if ((op.kind == BLHIP_OP_BREAKPOINT || (op.kind == BLHIP_OP_CHANGEPOINT && (op.flags & 1))) && val[k] <= tau) seg++;
        }
        return seg;
    };
    // a Deterministic model's shift of a step, in grid cells (its 2 T DETERMINISTIC_ARG ops: forward into step 0 .. T-1, backward into them)
    auto shift_cells = [&](const double *val, int k, int64_t t, bool fwd) { return val[k + 1 + (fwd ? t : T + t)] / p->lattice[p->ops[k].axis]; };
    // Shifts beyond 12 cells per step leave what a shift-invariant stencil reproduces (SciPy's pre-padding, TapTable::get_shift); the
    // two-stage kernel for them (blhip_bigshift.hpp) is 1-D / 2-D only.  Refused for every chain before anything is launched.
    if (has_shift)
        for (int64_t c = 0; c < n_chains; ++c) {
            const double *val = op_values + c * p->n_ops;
            for (int64_t t = 0; t < T; ++t)
                for (int dir = 0; dir < 2; ++dir) {
                    double tau = 0.0;
                    if (!stamp(t, dir == 0, tau)) continue;
                    const int seg = segment_at(val, tau);
                    for (int k : pass_ops) {
                        const blhip_op &op = p->ops[k];
                        if (op.kind != BLHIP_OP_DETERMINISTIC || (op.segment >= 0 && op.segment != seg)) continue;
                        const double dd = shift_cells(val, k, t, dir == 0);
                        if (std::isnan(dd)) fail("chain %lld: Deterministic shift of step %lld is NaN", (long long)c, (long long)t);
                        if (std::fabs(dd) > 12.0)
                            fail("chain %lld, step %lld: Deterministic model shifts by %.3g grid cells in one time step; on grids with %d "
                                 "parameters up to 12 (SciPy's pre-padding) are supported", (long long)c, (long long)t, dd, p->ndim);
                    }
                }
        }
    ChainProgram no_clamp;                           // (the bookkeeping helpers only ask it for clamp modes)
    // the chain-resident kernel (blhip_chain_nd.hpp) takes a batch of walks and restarts that is neither resumed nor carried; option
    // chain_nd: 0 off, 1 the batches the cost model gives it (at least CHAIN_ND_MIN_CHAINS chains), 2 wherever it fits
    const int chain_nd_opt = (int)ctx->option("chain_nd", 1.0);
    const bool chain_nd_program = !has_stage && !ff.resume && !ff.carry && npass <= bln::CHAIN_ND_MAXPASS;
    long long n_sum = 0;
    for (int k = 0; k < p->ndim; ++k) n_sum += p->n[k];

    for (int64_t c0 = 0; c0 < n_chains; c0 += Bmax) {
        const int64_t B = std::min<int64_t>(Bmax, n_chains - c0);
        ctx->timing.batches += 1;
        ctx->timing.cells_per_launch = std::max<int64_t>(ctx->timing.cells_per_launch, B * G);
        ctx->timing.fwd_kernel_variant = ctx->timing.bwd_kernel_variant = 7;
        // ---- the program of every chain: source kind and the kernel of every pass, per step and direction ------------------------------
        TapTable taps;
        const size_t nT = (size_t)T * B;
        std::vector<unsigned char> kindF(nT, SRC_PREV), kindB(nT, SRC_PREV);
        std::vector<int> tapF((size_t)std::max(1, npass) * nT, -1), tapB((size_t)std::max(1, npass) * nT, -1);     // [pass][t][b]
        // (with stages) kind*: where a step's input comes from; stepK*: what the fused kernel is told -- SRC_PREV too when the chain ran a
        // renormalising stage at the step, whose sums it then reads its scale from; limit: [pass][b] NotEqual's 10**v dV
        std::vector<unsigned char> stepKF, stepKB;
        std::vector<double> limit;
        if (has_stage) { stepKF.assign(nT, SRC_PREV); stepKB.assign(nT, SRC_PREV); limit.assign((size_t)npass * B, 0.0); }
        for (int64_t b = 0; b < B; ++b) {
            const double *val = op_values ? op_values + (c0 + b) * p->n_ops : nullptr;
            std::vector<int> op_tap(p->n_ops, -1);
            for (int k = 0; k < p->n_ops; ++k)
                if (p->ops[k].kind == BLHIP_OP_GRW) {
                    const double ns = val[k] / p->lattice[p->ops[k].axis];                    // transitionModels.py:108
                    if (std::isnan(ns)) fail("chain %lld: GRW sigma is NaN", (long long)(c0 + b));
                    op_tap[k] = ns > 0.0 ? taps.get(p->ops[k].axis, ns) : -1;                // :110-113
                } else if (p->ops[k].kind == BLHIP_OP_NOTEQUAL) {
                    for (int q = 0; q < npass; ++q) if (pass_ops[q] == k) limit[(size_t)q * B + b] = std::pow(10.0, val[k]) * dV;      // :468
                }
            // the transition into a step, evaluated at time stamp tau (list order; only the ops of the active sub-model of a serial
            // model act, transitionModels.py:768-776; a change point and an Independent model restart from a shared distribution and
            // drop what the models before them did, :300-312, :351-360) -> true: the chain ran a renormalising stage
            auto run = [&](double tau, int64_t t, bool fwd, unsigned char &kind, int *tp, size_t stride) {
                kind = SRC_PREV;
                bool renorm = false;
                auto restart = [&](unsigned char from) {
                    kind = from; renorm = false;
                    for (int q = 0; q < npass; ++q) tp[q * stride] = -1;
                };
                restart(SRC_PREV);
                const int seg = time_dependent ? segment_at(val, tau) : 0;
                for (int k = 0; k < p->n_ops; ++k) {
                    const blhip_op &op = p->ops[k];
                    if (op.segment >= 0 && op.segment != seg) continue;
                    int q = 0;
                    while (q < npass && pass_ops[q] != k) ++q;
                    if (op.kind == BLHIP_OP_GRW) {
                        tp[q * stride] = op_tap[k];
                    } else if (op.kind == BLHIP_OP_CHANGEPOINT && !(op.flags & 1) && time_dependent && tau == val[k]) {
                        restart(SRC_RESET);
                    } else if (op.kind == BLHIP_OP_INDEPENDENT) {
                        restart(SRC_INDEP);
                    } else if (op.kind == BLHIP_OP_NOTEQUAL) {                                // transitionModels.py:462-471
                        tp[q * stride] = 0;
                        renorm = true;
                    } else if (op.kind == BLHIP_OP_DETERMINISTIC) {                           // transitionModels.py:571-583, :585-602
                        const double dd = shift_cells(val, k, t, fwd);
                        if (dd != 0.0) { tp[q * stride] = taps.get_shift(op.axis, dd); renorm = true; }      // (zero shift: the identity)
                    }
                }
                if (time_dependent)
                    for (int k = 0; k < p->n_ops; ++k) {                                      // serial change-points: after the sub-model acted, :801-813
                        const blhip_op &op = p->ops[k];
                        if (op.kind == BLHIP_OP_CHANGEPOINT && (op.flags & 1) && tau == val[k]) restart(SRC_RESET);
                    }
                return renorm;
            };
            for (int64_t t = 0; t < T; ++t) {
                const size_t k = (size_t)t * B + b;
                double tau = 0.0;
                bool rnF = false, rnB = false;
                if (stamp(t, true, tau)) rnF = run(tau, t, true, kindF[k], &tapF[k], nT);
                else kindF[k] = SRC_PRIOR;                                              // core.py:363
                if (stamp(t, false, tau)) rnB = run(tau, t, false, kindB[k], &tapB[k], nT);
                else kindB[k] = SRC_UNIFORM;
                if (has_stage) { stepKF[k] = rnF ? (unsigned char)SRC_PREV : kindF[k]; stepKB[k] = rnB ? (unsigned char)SRC_PREV : kindB[k]; }
            }
        }
        taps.w.resize(taps.w.size() + 8, 0.0);
        int lw_max = 0;
        for (int v : taps.lw) lw_max = std::max(lw_max, v);
        // the walks that have a kernel somewhere in the batch, and the taps of its slowest chain (the cost model's W)
        int walks_on = 0, W_taps = 0;
        bool beyond_axis = false;                     // a walk wider than its axis: the kernel's multi-period reflection
        // (only a program without stages is asked: there every pass is a walk and every id >= 0 a tap set of the table -- NotEqual's
        //  passes carry a flag, not an id, and have no axis)
        for (int q = 0; chain_nd_program && q < npass; ++q) {
            int lw_q = 0;
            for (size_t k = 0; k < nT; ++k) {
                const int f = tapF[(size_t)q * nT + k], r = tapB[(size_t)q * nT + k];
                if (f >= 0) lw_q = std::max(lw_q, taps.lw[f]);
                if (r >= 0) lw_q = std::max(lw_q, taps.lw[r]);
            }
            if (lw_q > 0) { walks_on += 1; W_taps += 2 * lw_q + 1; }
            if (lw_q > ng.n[p->ops[pass_ops[q]].axis]) beyond_axis = true;
        }
        const bool chain_nd = bln::chain_nd_route(chain_nd_opt, chain_nd_program && bln::chain_nd_fits(G, lw_max, npass, n_sum), G, B, walks_on, W_taps, beyond_axis,
                                                  bln::chain_nd_threads(G, lw_max, npass, n_sum), std::min(ctx->num_cus, 256));
        const int nb = chain_nd ? 1 : nblk;          // partial sums per (step, chain, slot): the resident kernel writes block totals
        if (chain_nd) ctx->timing.fwd_kernel_variant = ctx->timing.bwd_kernel_variant = 10;
        // ---- device buffers ----------------------------------------------------------------------------------------------------------
        // (a chain-resident batch keeps its state in LDS: no state / scratch arrays, no tables of where a step's input lives)
        if (!chain_nd) ctx->state.ensure((size_t)3 * B * G * 8);
        double *d_state = ctx->state.as<double>(), *d_tmp[2] = {d_state + (size_t)B * G, d_state + (size_t)2 * B * G};
        double *d_post = nullptr;
        if (!ff.evidence_only) { ctx->post.ensure((size_t)B * T * G * 8); d_post = ctx->post.as<double>(); }
        const size_t psz = (size_t)T * B * NRED * nb;
        ctx->psumF.ensure(psz * 8); ctx->redF.ensure(nT * NRED * 8);
        if (ff.full) { ctx->psumB.ensure(psz * 8); ctx->redB.ensure(nT * NRED * 8); }
        const size_t ntap = taps.off.size() + 1;
        size_t mb = 2 * carve_size(nT) + 2 * carve_size(tapF.size() * 4) + carve_size(taps.w.size() * 8) + 2 * carve_size(ntap * 4) +
                    2 * carve_size(nT * 8) + 3 * carve_size((size_t)B * 8) + carve_size((size_t)B * 8) + carve_size(nT * 8);
        if (has_stage) mb += carve_size(limit.size() * 8) + 2 * carve_size((size_t)B * nblk * 8) + carve_size((size_t)B * NRED * nblk * 8);
        ctx->meta.ensure(mb);
        char *mc = ctx->meta.as<char>();
        unsigned char *d_kindF = carve<unsigned char>(mc, nT), *d_kindB = carve<unsigned char>(mc, nT);
        int *d_tapF = carve<int>(mc, tapF.size()), *d_tapB = carve<int>(mc, tapB.size());
        double *d_taps = carve<double>(mc, taps.w.size());
        int *d_off = carve<int>(mc, ntap), *d_lw = carve<int>(mc, ntap);
        const double **d_src0F = carve<const double *>(mc, nT), **d_src0B = carve<const double *>(mc, nT);
        const double **d_ptr_state = carve<const double *>(mc, (size_t)B), **d_ptr_tmp0 = carve<const double *>(mc, (size_t)B),
                     **d_ptr_tmp1 = carve<const double *>(mc, (size_t)B);
        double *d_w = carve<double>(mc, (size_t)B), *d_invN = carve<double>(mc, nT);
        // the stages' scratch (blhip_nd_stages.hpp): NotEqual's limits, block maxima and block sums, the partial sums of a stage's output
        double *d_limit = nullptr, *d_bmax = nullptr, *d_bsum = nullptr, *d_stage_sums = nullptr;
        if (has_stage) {
            d_limit = carve<double>(mc, limit.size()); d_bmax = carve<double>(mc, (size_t)B * nblk); d_bsum = carve<double>(mc, (size_t)B * nblk);
            d_stage_sums = carve<double>(mc, (size_t)B * NRED * nblk);
            HIPCHECK(hipMemcpyAsync(d_limit, limit.data(), limit.size() * 8, hipMemcpyHostToDevice, st));
        }
        // where a step's input lives: the chain's state, or a shared distribution at a restart
        std::vector<const double *> src0F(chain_nd ? 0 : nT), src0B(chain_nd ? 0 : nT), pst(B), pt0(B), pt1(B);
        for (int64_t b = 0; !chain_nd && b < B; ++b) {
            pst[b] = d_state + (size_t)b * G; pt0[b] = d_tmp[0] + (size_t)b * G; pt1[b] = d_tmp[1] + (size_t)b * G;
            for (int64_t t = 0; t < T; ++t) {
                const size_t k = (size_t)t * B + b;
                src0F[k] = kindF[k] == SRC_PREV ? ((t == 0 && ff.resume) ? d_carry_src + (size_t)b * G : pst[b])
                                                : (kindF[k] == SRC_PRIOR ? d_prior : (kindF[k] == SRC_INDEP ? d_indep : d_reset));
                src0B[k] = kindB[k] == SRC_PREV ? pst[b] : (kindB[k] == SRC_UNIFORM ? d_uniform : (kindB[k] == SRC_INDEP ? d_indep : d_reset));
            }
        }
        HIPCHECK(hipMemcpyAsync(d_kindF, (has_stage ? stepKF : kindF).data(), nT, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_kindB, (has_stage ? stepKB : kindB).data(), nT, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_tapF, tapF.data(), tapF.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_tapB, tapB.data(), tapB.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_taps, taps.w.data(), taps.w.size() * 8, hipMemcpyHostToDevice, st));
        if (!taps.off.empty()) {
            HIPCHECK(hipMemcpyAsync(d_off, taps.off.data(), taps.off.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(d_lw, taps.lw.data(), taps.lw.size() * 4, hipMemcpyHostToDevice, st));
        }
        if (!chain_nd) {
            HIPCHECK(hipMemcpyAsync(d_src0F, src0F.data(), nT * 8, hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(d_src0B, src0B.data(), nT * 8, hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(d_ptr_state, pst.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(d_ptr_tmp0, pt0.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(d_ptr_tmp1, pt1.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
        }
        sync_stream(ctx, st);

        // one time step: the passes of the transition, then the fused elementwise kernel
        auto step = [&](bool bwd, int64_t t, const double *ps_prev, double *ps_out) {
            const double *const *in = (bwd ? d_src0B : d_src0F) + (size_t)t * B;
            const int *tp = (bwd ? d_tapB : d_tapF) + (size_t)t * B;
            const std::vector<int> &htp = bwd ? tapB : tapF;
            int flip = 0;
            // whose partial sums the fused kernel reads its scale from: the producing step's, or those of the step's last stage
            const double *ps_scale = ps_prev;
            int scale_slot = bwd ? 2 : 0;
            for (int q = 0; q < npass; ++q) {
                bool any = false;
                for (int64_t b = 0; b < B && !any; ++b) any = htp[(size_t)q * nT + (size_t)t * B + b] >= 0;
                if (!any) continue;
                const blhip_op &op = p->ops[pass_ops[q]];
                const int ax = op.axis;
                const dim3 grid((unsigned)nblk, (unsigned)B);
                const int *id = tp + (size_t)q * nT;
                if (op.kind == BLHIP_OP_GRW) {
                    BL_LAUNCH(bln::filter_axis_kernel, grid, dim3(NTHREADS), 0, st, d_tmp[flip], in, G, ng.n[ax], ng.stride[ax], id, d_taps, d_off, d_lw);
                } else if (op.kind == BLHIP_OP_NOTEQUAL) {
                    BL_LAUNCH(bln::ne_max_kernel, grid, dim3(NTHREADS), 0, st, in, G, id, d_bmax);
                    BL_LAUNCH(bln::ne_invert_kernel, grid, dim3(NTHREADS), 0, st, d_tmp[flip], in, G, id, d_bmax, d_bsum);
                    BL_LAUNCH(bln::ne_clamp_kernel, grid, dim3(NTHREADS), 0, st, d_tmp[flip], G, id, d_limit + (size_t)q * B, d_bsum, ps_scale, scale_slot,
                              d_stage_sums);
                    ps_scale = d_stage_sums; scale_slot = 0;
                } else {
                    BL_LAUNCH(bln::shift_axis_kernel, grid, dim3(NTHREADS), 0, st, d_tmp[flip], in, G, ng.n[ax], ng.stride[ax], id, d_taps, d_off, d_lw,
                              ps_scale, scale_slot, d_stage_sums);
                    ps_scale = d_stage_sums; scale_slot = 0;
                }
                in = flip ? d_ptr_tmp1 : d_ptr_tmp0;
                flip ^= 1;
            }
            bln::NdStep Q{};
            Q.g = ng; Q.B = (int)B; Q.T = (int)T; Q.nblk = nblk; Q.srcs = in; Q.kind = (bwd ? d_kindB : d_kindF) + (size_t)t * B;
            Q.psum_prev = ps_scale; Q.prev_slot = scale_slot; Q.psum_out = ps_out; Q.lik = d_lik + (size_t)t * G; Q.state = d_state;
            Q.post = d_post ? d_post + (size_t)t * G : nullptr; Q.post_stride = (long long)T * G;
            if (bwd) BL_LAUNCH(bln::step_kernel<true>, dim3((unsigned)nblk, (unsigned)B), dim3(NTHREADS), 0, st, Q);
            else BL_LAUNCH(bln::step_kernel<false>, dim3((unsigned)nblk, (unsigned)B), dim3(NTHREADS), 0, st, Q);
        };
        double *d_psF = ctx->psumF.as<double>();
        const size_t per_step = (size_t)B * NRED * nb;
        float ms = 0;
        // BLHIP_RESUME: the carried states are normalised -- the "partial sums of the step before" add up to 1
        const double *d_unit = nullptr;
        if (ff.resume) {
            std::vector<double> unit(per_step, 0.0);
            for (int64_t b = 0; b < B; ++b) unit[(size_t)b * NRED * nblk] = 1.0;
            ctx->unit.ensure(unit.size() * 8);
            HIPCHECK(hipMemcpyAsync(ctx->unit.p, unit.data(), unit.size() * 8, hipMemcpyHostToDevice, st));
            sync_stream(ctx, st);
            d_unit = ctx->unit.as<double>();
        }
        // one pass of the chain-resident kernel: every step of every chain of the batch in one launch
        auto chain_pass = [&](bool bwd, double *ps) {
            bln::ChainNd Q{};
            Q.g = ng; Q.B = (int)B; Q.T = (int)T; Q.npass = npass;
            for (int q = 0; q < npass; ++q) { const int ax = p->ops[pass_ops[q]].axis; Q.pass_n[q] = ng.n[ax]; Q.pass_inner[q] = (int)ng.stride[ax]; }
            Q.tap_slot = lw_max + 1;
            Q.kind = bwd ? d_kindB : d_kindF; Q.tap = bwd ? d_tapB : d_tapF; Q.taps = d_taps; Q.tap_off = d_off; Q.tap_lw = d_lw;
            Q.shared[SRC_PREV] = nullptr; Q.shared[SRC_PRIOR] = d_prior; Q.shared[SRC_RESET] = d_reset; Q.shared[SRC_UNIFORM] = d_uniform;
            Q.shared[SRC_INDEP] = d_indep;
            Q.lik = d_lik; Q.post = d_post; Q.post_stride = (long long)T * G; Q.psum = ps;
            launch_chain_nd(st, Q, bwd, bln::chain_nd_threads(G, lw_max, npass, n_sum), bln::chain_nd_lds_doubles(G, lw_max, npass, n_sum) * sizeof(double));
        };
        // ---- forward pass (core.py:372-411) ---------------------------------------------------------------------------------------------
        HIPCHECK(hipEventRecord(ev[0], st));
        if (chain_nd) chain_pass(false, d_psF);
        else for (int64_t t = 0; t < T; ++t) step(false, t, t > 0 ? d_psF + (size_t)(t - 1) * per_step : (d_unit ? d_unit : d_psF), d_psF + (size_t)t * per_step);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[1], st));
        BL_LAUNCH(reduce_partials_kernel, dim3((unsigned)(nT * NRED)), dim3(NTHREADS), 0, st, d_psF, ctx->redF.as<double>(), nb, 0);      // (0: every slot is a sum -- slot 6 is the 4th parameter's mean here)
        ctx->pinF.ensure(nT * NRED * 8);
        double *redF = ctx->pinF.as<double>();
        HIPCHECK(hipMemcpyAsync(redF, ctx->redF.p, nT * NRED * 8, hipMemcpyDeviceToHost, st));
        sync_stream(ctx, st);
        HIPCHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ctx->timing.forward_ms += ms; ctx->timing.forward_launches += chain_nd ? 1 : T;
        BatchOutcome O;
        forward_bookkeeping(p, no_clamp, redF, B, dV, false, 1, ff.evidence_only, ff.forward_only, O);
        O.invN.assign(nT, 0.0);
        // ---- backward pass (core.py:424-470) --------------------------------------------------------------------------------------------
        if (ff.full) {
            double *d_psB = ctx->psumB.as<double>();
            HIPCHECK(hipEventRecord(ev[2], st));
            if (chain_nd) chain_pass(true, d_psB);
            else for (int64_t t = T - 1; t >= 0; --t) step(true, t, t < T - 1 ? d_psB + (size_t)(t + 1) * per_step : d_psB, d_psB + (size_t)t * per_step);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev[3], st));
            BL_LAUNCH(reduce_partials_kernel, dim3((unsigned)(nT * NRED)), dim3(NTHREADS), 0, st, d_psB, ctx->redB.as<double>(), nb, 0);
            ctx->pinB.ensure(nT * NRED * 8);
            double *redB = ctx->pinB.as<double>();
            HIPCHECK(hipMemcpyAsync(redB, ctx->redB.p, nT * NRED * 8, hipMemcpyDeviceToHost, st));
            sync_stream(ctx, st);
            HIPCHECK(hipEventElapsedTime(&ms, ev[2], ev[3]));
            ctx->timing.backward_ms += ms; ctx->timing.backward_launches += chain_nd ? 1 : T;
            backward_bookkeeping(p, no_clamp, redF, redB, B, dV, false, -1, O);
        } else if (ff.forward_only) {
            for (int64_t b = 0; b < B; ++b)
                for (int64_t t = 0; t < T; ++t) {
                    const double n0 = redF[((size_t)t * B + b) * NRED];
                    O.invN[(size_t)b * T + t] = (n0 != 0.0 && std::isfinite(n0)) ? 1.0 / n0 : 0.0;
                }
        }
        // BLHIP_CARRY: every chain's filtered distribution of the last step, normalised (core.py:2173)
        if (ff.carry) store_carry(ctx, p, B, G, redF, d_post ? d_post + (size_t)(T - 1) * G : d_state, d_post ? (long long)T * G : G, d_w, false);
        if (ff.accumulate) fold_accumulate(ctx, T, G, B, O, log_w + c0, d_post, d_w, d_invN);
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
