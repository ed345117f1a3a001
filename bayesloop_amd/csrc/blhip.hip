// libblhip: C-ABI (include/blhip.h) + host orchestration of the forward-backward recursion on one MI355X.
//
// The host side owns what the reference's Study.fit loop owns (bayesloop/core.py:330-486): the order of steps, the
// evidence bookkeeping and the per-step transition program; the arithmetic on the grid runs in the HIP kernels of
// blhip_kernels.hpp / blhip_fast.hpp.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <exception>
#include <map>
#include <memory>
#include <unordered_map>
#include <mutex>
#include <set>
#include <string>
#include <string_view>
#include <system_error>
#include <chrono>
#include <thread>
#include <vector>

#include "../../include/blhip.h"
#include "blhip_kernels.hpp"
#include "blhip_bigshift.hpp"
#include "blhip_fast.hpp"
#include "blhip_mfma.hpp"
#include "blhip_hwide.hpp"
#include "blhip_fused1d.hpp"
#include "blhip_chain1d.hpp"
#include "blhip_persist1d.hpp"
#include "blhip_resident.hpp"
#include "blhip_chainres.hpp"
#include "blhip_chain_launch.hpp"
#include "blhip_chainclamp_plan.hpp"
#include "blhip_nd.hpp"
#include "blhip_nd_stages.hpp"
#include "blhip_chain_nd.hpp"
#include "blhip_likprog.hpp"
#include "blhip_predictive.hpp"
#include "blhip_online.hpp"
#include "blhip_query.hpp"
#include "blhip_bins.hpp"

using namespace blk;

#include "blhip_host.hpp"
#include "blhip_comm.hpp"

namespace {

#include "blhip_program.hpp"   // TapTable, Geometry, validate, build_records, build_program
#include "blhip_launch.hpp"    // Tile, launch_* (the launch tables), plan_resident
#include "blhip_chain_plan.hpp"   // plan_chainres, ChainFacts / ChainOptions and the stages of the chain-resident route on two-parameter grids (no HIP call)
#include "blhip_series.hpp"    // series_check, series_plan, series_chain_bytes: series fits (no HIP call)
#include "blhip_batch.hpp"     // plan_batches, upload_tables / _metadata, chains_per_batch, plan_geometry, folds, results
#include "blhip_book.hpp"      // resident_unlag / chain_unlag, forward_ / backward_bookkeeping, account
#include "blhip_nd_program.hpp"   // NdFacts, NdBatchProgram, build_nd_program: the transition program on grids with 3 and 4 parameters (no HIP call)
#include "blhip_fit_nd.hpp"       // do_fit_nd, NdEnv, nd_step, NdChainRun: grids with 3 and 4 parameters
#include "blhip_fit_paths.hpp"    // BatchEnv, ResidentRun, ChainRun: the resident paths of a batch
#include "blhip_fit_row1d.hpp"    // Row1dRun: the 1-D paths of a batch
#include "blhip_fit_step.hpp"     // StepRun: the launch-per-step path of a batch
#include "blhip_batch_sched.hpp"  // BatchPath, PassPlan, the tail's decisions, BatchSchedule, ResidentRetry: do_fit's batch loop (no HIP call; blhip_host.hpp has read it already)

// one batch of a fit: the paths it may run on, and what its passes and its tail share
struct BatchRun {
    BatchEnv E{};
    ResidentRun RR;
    ChainRun CR;
    Row1dRun R1;
    StepRun SR;
    BatchOutcome O;
    size_t psz = 0;                              // partial sums of a pass (doubles): the most slots any path of the batch writes
    double dV = 1.0;
    bool resident_failed = false;                // a resident pass gave up or failed a check: the launch-per-step kernels take over
    double *redF = nullptr, *redB = nullptr;     // reduced sums on the host (page-locked staging of the context)
    BatchPath path() const { return batch_path(RR.on, CR.on, R1.on, resident_failed); }      // of the next attempt / of the one that went through
};

// The end of a pass: the partial sums of its `nblk` slots are added up, and the sums travel to the page-locked buffer -- on the main
// stream, or (`beside`) on the copy stream, where nobody waits for them.  -> the host buffer
double *end_pass(blhip_ctx *ctx, hipStream_t st, hipEvent_t done, int64_t n_sums, int nblk, double *d_ps, DevBuf &red, PinBuf &pin, bool beside) {
    HIPCHECK(hipEventRecord(done, st));
    // (one slot per sum -- the kernels that give a chain ONE block: nothing to add up, the partials ARE the sums.  The published
    //  break-point study: 2 x 6 launches of T * B * NRED = 1.3 M one-value blocks, 0.48 ms each, 5.7 of a 44-ms fit)
    if (nblk > 1)
        BL_LAUNCH(reduce_partials_kernel, dim3((unsigned)n_sums), dim3(NTHREADS), 0, st, d_ps, red.as<double>(), nblk, NRED);
    pin.ensure((size_t)n_sums * 8);
    double *h = pin.as<double>();
    const void *src = nblk > 1 ? red.p : (const void *)d_ps;
    if (beside) {
        HIPCHECK(hipEventRecord(ctx->cev[0], st));
        HIPCHECK(hipStreamWaitEvent(ctx->cstream, ctx->cev[0], 0));
        HIPCHECK(hipMemcpyAsync(h, src, (size_t)n_sums * 8, hipMemcpyDeviceToHost, ctx->cstream));
        HIPCHECK(hipEventRecord(ctx->cev[1], ctx->cstream));
    } else {
        HIPCHECK(hipMemcpyAsync(h, src, (size_t)n_sums * 8, hipMemcpyDeviceToHost, st));
    }
    return h;
}

// (the timing of an attempt that is repeated is dropped)
void reset_pass_timing(blhip_ctx *ctx) {
    ctx->timing.forward_ms = ctx->timing.backward_ms = 0.0;
    ctx->timing.fwd_hbm_bytes = ctx->timing.bwd_hbm_bytes = ctx->timing.fwd_flops = ctx->timing.bwd_flops = 0.0;
    ctx->timing.forward_launches = ctx->timing.backward_launches = 0;
}

// the launches of one pass of an attempt on its path
void launch_pass(BatchRun &R, BatchPath path, bool bwd, int64_t K, double *d_ps) {
    const BatchEnv &E = R.E;
    switch (path) {
    case PATH_RESIDENT: R.RR.launch(E, bwd, d_ps); break;
    case PATH_CHAIN:
        if (bwd && R.CR.fused) { R.CR.prepare_fold(E, R.O); E.mark("  prepare_fold"); }
        R.CR.pass(E, bwd, d_ps);
        break;
    case PATH_ROW1D: if (bwd) R.R1.backward(E, K, d_ps); else R.R1.forward(E, K, d_ps); break;
    case PATH_STEP: if (bwd) R.SR.backward(E, d_ps); else R.SR.forward(E, d_ps); break;
    }
}

// The path's own check of a pass from its reduced sums, and the kernel variant the pass reports (the chain-resident backward pass: also
// the fused fold, which is queued behind its prediction check).  -> false: a resident pass gave up or failed its check
bool check_pass(BatchRun &R, BatchPath path, bool bwd, double *red) {
    const BatchEnv &E = R.E;
    int32_t &variant = bwd ? E.ctx->timing.bwd_kernel_variant : E.ctx->timing.fwd_kernel_variant;
    switch (path) {
    case PATH_RESIDENT:
        variant = 5;
        return bwd ? R.RR.backward_ok(E, red) : R.RR.forward_ok(E, red);
    case PATH_CHAIN:
        variant = R.CR.clamp ? blcp::VARIANT : 6;
        if (!(bwd ? R.CR.backward_ok(E, red) : R.CR.forward_ok(E, red))) return false;
        E.mark(bwd ? "  backward_ok" : "  forward_ok");
        if (!bwd) return true;
        if (R.CR.fused && !R.CR.fold(E, red, *E.fold_ev)) return false;
        E.mark("  prediction check + fold queued");
        return true;
    case PATH_ROW1D:
        variant = R.R1.variant();
        return !R.R1.gave_up(E);
    case PATH_STEP:
        variant = R.SR.variant(E, bwd);
        return true;
    }
    return true;
}

// forward-only fits: 1 / (the sum of each stored row), from where the path of the pass left the sums
void forward_only_invN(BatchRun &R, BatchPath path, const double *redF) {
    const int64_t T = R.E.T, B = R.E.B;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t t = 0; t < T; ++t) {
            double &inv = R.O.invN[(size_t)b * T + t];
            switch (path) {
            case PATH_RESIDENT:
                inv = forward_invN(R.RR.rowsumF[t]);
                if (t <= T - 1 - R.RR.RQ.lag) inv = 1.0;            // (already normalised by the resident kernel)
                break;
            case PATH_CHAIN: inv = forward_invN(R.CR.rowsumC[b][t]); break;
            default: inv = forward_invN(redF[((size_t)t * B + b) * NRED]); break;
            }
        }
}

// The backward pass of a full fit (core.py:424-470) behind its forward pass, with the host's checks and bookkeeping.  raw_ok: the forward
// bookkeeping's answer, which this pass still owes where it runs behind the launches (P.late_fb).  -> 1 / 0: that answer and the
// backward bookkeeping's; -1: a resident pass gave up or failed its check
int backward_pass(BatchRun &R, const int64_t K, BatchPath path, const PassPlan &P, bool raw_ok) {
    const BatchEnv &E = R.E;
    blhip_ctx *ctx = E.ctx;
    hipStream_t st = E.st;
    hipEvent_t *ev = ctx->ev;
    const int64_t T = E.T, B = E.B;
    float ms = 0;
    HIPCHECK(hipEventRecord(ev[2], st));
    double *d_psB = ctx->psumB.as<double>();
    launch_pass(R, path, true, K, d_psB);
    double *redB = R.redB = end_pass(ctx, st, ev[3], T * B * NRED, path == PATH_CHAIN ? R.CR.pass_nblk(true) : P.nblk, d_psB, ctx->redB, ctx->pinB, false);
    E.mark("backward pass queued");
    if (P.late_fb) {
        if (P.late_copy) HIPCHECK(hipEventSynchronize(ctx->cev[1]));
        raw_ok = forward_bookkeeping(E.p, *E.prog, R.redF, B, R.dV, R.R1.on, K, E.ff.evidence_only, E.ff.forward_only, R.O);
        E.mark("forward bookkeeping (behind the backward pass)");
    }
    sync_stream(ctx, st);
    E.mark("backward pass done + sums D2H");
    if (P.late_copy) {
        HIPCHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ctx->timing.forward_ms += ms;
    }
    HIPCHECK(hipEventElapsedTime(&ms, ev[2], ev[3]));
    ctx->timing.backward_ms += ms;
    ctx->timing.backward_launches += T;
    if (!check_pass(R, path, true, redB)) return -1;
    // (a batch the backward kernel folded: nobody reads its row normalisers; per-chain means only where the caller asked for them --
    //  hyper- / change-point studies take theirs from the average posterior)
    raw_ok = backward_bookkeeping(E.p, *E.prog, R.redF, redB, B, R.dV, R.R1.on, path == PATH_RESIDENT ? 0 : -1, R.O,
                                  !(path == PATH_CHAIN && R.CR.fold_done), E.chain_means) && raw_ok;
    E.mark("backward checks + fused fold + bookkeeping");
    return raw_ok ? 1 : 0;
}

// The two passes of a batch and the host's checks and bookkeeping behind each.  K: steps per launch of the K-steps-per-launch 1-D kernel.
// -> false: the batch has to be repeated -- R.resident_failed: on the launch-per-step kernels, else with K = 1.
bool run_passes(BatchRun &R, const int64_t K) {
    const BatchEnv &E = R.E;
    blhip_ctx *ctx = E.ctx;
    hipStream_t st = E.st;
    hipEvent_t *ev = ctx->ev;
    const int64_t T = E.T, B = E.B;
    float ms = 0;
    E.mark("path setup");
    // --- forward pass (core.py:372-411) ---
    HIPCHECK(hipEventRecord(ev[0], st));
    const BatchPath path = R.path();
    const PassPlan P = pass_plan(path, R.RR.nblk, R.CR.cp.strips, E.tile.nblk, E.ff.full, R.R1.chain, B, ctx->cstream != nullptr,
                                 ctx->option("late_sums", 1.0) != 0.0);
    double *d_psF = ctx->psumF.as<double>();
    launch_pass(R, path, false, K, d_psF);
    double *redF = R.redF = end_pass(ctx, st, ev[1], T * B * NRED, P.nblk, d_psF, ctx->redF, ctx->pinF, P.late_copy);
    if (P.late_copy) {
        E.mark("forward pass queued (its sums follow beside the backward pass)");
    } else {
        E.mark("forward pass queued");
        sync_stream(ctx, st);
        E.mark("forward pass done + sums D2H");
        HIPCHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ctx->timing.forward_ms += ms;
    }
    ctx->timing.forward_launches += T;
    if (!check_pass(R, path, false, redF)) { R.resident_failed = true; return false; }

    bool raw_ok = P.late_fb ? true : forward_bookkeeping(E.p, *E.prog, redF, B, R.dV, R.R1.on, K, E.ff.evidence_only, E.ff.forward_only, R.O);
    E.mark("forward checks + bookkeeping");

    R.O.invN.assign((size_t)B * T, 0.0);
    if (E.ff.full) {
        ctx->psumB.ensure(R.psz * 8);
        ctx->redB.ensure((size_t)T * B * NRED * 8);
        if (R.R1.on && !raw_ok && K > 1) return false;
        const int back = backward_pass(R, K, path, P, raw_ok);
        if (back < 0) { R.resident_failed = true; return false; }
        raw_ok = back != 0;
    } else if (E.ff.forward_only) {
        forward_only_invN(R, path, redF);
    }
    return raw_ok || K == 1;
}

// the grouped fold of a series fit (blhip_set_series_groups with BLHIP_ACCUMULATE): defined below, behind seq_row_stats
void series_group_fold(blhip_ctx *ctx, const blhip_problem *p, int64_t T, long long G, int64_t B, int64_t c0, const BatchOutcome &out,
                       const double *log_w_batch, const double *d_post, double *d_w, double *d_invN, blhip_result *res);

// The tail of a batch: carried states / average posterior / kept posterior / results.  path: the one its passes went through on, usedK:
// with that K; folded_before: a repeat after poisoned carried slots of a batch that is in the accumulator already.
void finish_batch(BatchRun &R, BatchPath path, int64_t usedK, bool folded_before, int64_t nbatch, blhip_result *res) {
    const BatchEnv &E = R.E;
    blhip_ctx *ctx = E.ctx;
    const blhip_problem *p = E.p;
    const Geometry &g = E.g;
    const ChainRun &CR = R.CR;
    const int64_t T = E.T, B = E.B;
    const long long G = E.G;
    // (what ran, not what was planned: a declined or repeated batch left row-major posteriors -- chain_fold_source, blhip_chain_plan.hpp)
    const ChainFoldSource src = chain_fold_source(CR.on, R.resident_failed, CR.post_private, CR.cp.pad, CR.ax1, CR.depad, g.n0);
    double *d_post = E.d_post;
    if (src.through_depad) {                     // (E.d_post was the kernels' scratch sequence on the padded geometry)
        d_post = ctx->post.as<double>();
        for_grid_y(ctx, (long long)B * T, [&](long long y0, unsigned ny) {
            BL_LAUNCH(depad_kernel, dim3((unsigned)((G + NTHREADS - 1) / NTHREADS), ny), dim3(NTHREADS), 0, E.st, d_post,
                               ctx->postpad.as<double>(), g.n0, g.n1, CR.cp.n0p, CR.Gk, (int)T, CR.ax1 ? 1 : 0, y0);
        });
        HIPCHECK(hipGetLastError());
    }
    if (E.ff.carry) {
        const CarriedStateSource cs = carried_state_source(E.ff.evidence_only, R.R1.on, T, usedK, G);
        store_carry(ctx, p, B, G, R.redF, (cs.state < 0 ? d_post : E.d_pp[cs.state]) + cs.offset, cs.stride, E.M->w, E.prog->has_clamp);
    }
    const FoldAction fold = fold_action(E.ff.accumulate, CR.fold_done, folded_before, nbatch, E.ff.keep, E.ff.carry);
    if (fold == FOLD_AND_WAIT || fold == FOLD_UNWAITED) {
        FoldJob lay;
        const bool padded = src.layout == FOLD_PADDED;
        if (padded) { lay.pad_n0p = CR.cp.n0p; lay.pad_n0 = g.n0; lay.pad_n1 = g.n1; lay.pad_step = CR.Gk; lay.pad_ax = CR.ax1 ? 1 : 0; }
        fold_accumulate(ctx, T, G, B, R.O, E.log_w + E.c0, d_post, E.M->w, E.M->invN, src.sm_n0, padded ? &lay : nullptr,
                        fold == FOLD_UNWAITED ? E.fold_ev : nullptr);
    }
    if (ctx->series.fold) {                      // (series in groups: each group into its own average, which becomes the kept posterior)
        series_group_fold(ctx, p, T, G, B, E.c0, R.O, E.log_w + E.c0, d_post, E.M->w, E.M->invN, res);
    } else if (E.ff.keep) {
        const RowRange rows = keep_rows(path, E.ff.full, T, R.RR.RQ.lag);
        keep_posterior(ctx, g, T, B, R.O, rows.row0, rows.row1);
    }
    E.mark("fold / keep / carry");
    write_results(res, p, E.c0, B, R.O, !E.ff.evidence_only && !ctx->series.fold);
}

// what a call of do_fit holds for every one of its batches
struct FitCall {
    blhip_ctx *ctx; const blhip_problem *p; hipStream_t st;
    FitFlags ff; Geometry g; double dV;
    int64_t n_chains, nbatch; const double *log_w; blhip_result *res;
    const DeviceTables *DT; Trace *tr;
    std::vector<hipEvent_t> *fold_ev;          // folds nobody waits for: start / end events of every one (timing)
};

// The per-(step, chain) programs of batch bi + 1 are built by a second host thread while batch bi runs -- its passes on the GPU, its
// bookkeeping on this thread (the reference's published break-point study: 23 batches of 1017 chains x 41 steps, 23 - 30 ms of
// build_program of a 90 - 130-ms fit; the builder touches only its own BatchProgram and the caller's read-only inputs, no HIP call).
struct BatchProgram { TapTable taps; ChainProgram prog; bool ready = false; std::exception_ptr err; };

class BatchPrograms {
public:
    BatchPrograms(const blhip_problem *p, const Geometry &g, const std::vector<int64_t> &batch_start, const double *op_values, bool resume)
        : p_(p), g_(g), batch_start_(batch_start), op_values_(op_values), resume_(resume) {}
    BatchPrograms(const BatchPrograms &) = delete;
    BatchPrograms &operator=(const BatchPrograms &) = delete;
    ~BatchPrograms() { join(); }                 // (also when a batch throws)

    // The program of batch bi: waits for the builder, builds the program here if nobody has, and starts batch bi + 1.  A failure of an
    // early build is raised where the build used to be: at the top of that batch.
    BatchProgram &take(int64_t bi) {
        join();
        if (!slot_[bi & 1] || !slot_[bi & 1]->ready) build(bi);
        BatchProgram &BP = *slot_[bi & 1];
        BP.ready = false;                        // (consumed: the slot is rebuilt for batch bi + 2)
        if (BP.err) std::rethrow_exception(BP.err);
        if (bi + 2 < (int64_t)batch_start_.size()) {
            try { builder_ = std::thread([this, bi] { build(bi + 1); }); }
            catch (const std::system_error &) {}        // (no thread to be had: the batch is built at its own top, as before)
        }
        return BP;
    }
    // the call goes back to an earlier batch: nothing that was built ahead is of use
    void drop() { join(); slot_[0].reset(); slot_[1].reset(); }

private:
    void join() { if (builder_.joinable()) builder_.join(); }
    void build(int64_t bj) {
        std::unique_ptr<BatchProgram> &N = slot_[bj & 1];
        N.reset(new BatchProgram());
        try { build_program(p_, g_, batch_start_[bj], batch_start_[bj + 1] - batch_start_[bj], op_values_, N->taps, N->prog, resume_); }
        catch (...) { N->err = std::current_exception(); }
        N->ready = true;
    }
    const blhip_problem *p_; const Geometry &g_; const std::vector<int64_t> &batch_start_; const double *op_values_; bool resume_;
    std::unique_ptr<BatchProgram> slot_[2];
    std::thread builder_;
};

// What the fit starts from: nothing kept or carried inside a call from the one before; the resident paths re-armed where their wait
// is over (probe_residency asks the chip first then)
void begin_fit(blhip_ctx *ctx) {
    ctx->post_valid = false;
    ctx->part = blhip_ctx::PartState{};            // (carried partial accumulators live inside one call)
    ctx->timing = blhip_timing{};
    ctx->resident_last_reason = 0;
    if (ctx->resident.fit_begins()) ctx->probe_last = -1.0;
    probe_residency(ctx);
    ctx->timing.xcd_order = ctx->xcd_order_ok ? 1 : 0;
}

// The state of batch bi -- chains [c0, c0 + B) -- of the call: its buffers, and the paths it may run on set up: the 1-D kernels, or the
// resident ones (single chain: blhip_resident.hpp; batches of chains: blhip_chainres.hpp) with the launch-per-step kernels as their fall-back
BatchRun setup_batch(const FitCall &F, int64_t bi, int64_t c0, int64_t B, BatchProgram &BP, const GeometryPlan &gp, const DeviceMeta &M, bool allow_chainres) {
    blhip_ctx *ctx = F.ctx;
    const int64_t T = F.p->T;
    const long long G = F.g.G;
    BatchRun R;
    R.dV = F.dV;
    R.psz = (size_t)T * B * NRED * gp.tile.nblk;
    ctx->psumF.ensure(R.psz * 8);
    ctx->redF.ensure((size_t)T * B * NRED * 8);
    BatchEnv &E = R.E;
    E.ctx = ctx; E.p = F.p; E.st = F.st; E.g = F.g; E.G = G; E.T = T; E.B = B; E.c0 = c0; E.d = F.DT->d; E.rec_len = F.DT->rec_len; E.ff = F.ff;
    E.DT = F.DT; E.M = &M; E.prog = &BP.prog; E.taps = &BP.taps; E.gp = &gp; E.tile = gp.tile; E.log_w = F.log_w;
    E.chain_means = F.res && F.res->posterior_mean && !ctx->series.fold;       // (a grouped fold: the means are the averages')
    E.tr = F.tr;
    E.fold_ev = F.fold_ev; E.bi = bi; E.allow_chainres = allow_chainres;
    ctx->state.ensure((size_t)2 * B * G * 8);
    E.d_pp[0] = ctx->state.as<double>();
    E.d_pp[1] = E.d_pp[0] + (size_t)B * G;
    if (!F.ff.evidence_only) {
        ctx->post.ensure((size_t)B * T * G * 8);
        E.d_post = ctx->post.as<double>();
    }
    // BLHIP_RESUME: step 0 reads each chain's carried (normalised) state; its "previous partial sums" add up to 1
    if (F.ff.resume) {
        E.d_carry_src = carry_source(ctx, F.p, F.n_chains, G);
        E.d_unit = upload_unit_sums(ctx, F.p, F.st, B, gp.tile.nblk, true);
    }
    // (fast_but_clamp: only step0 / use_rec are read, by the chain-resident clamp kernels' setup)
    const RowRecurrence rr = (gp.fast || gp.fast_but_clamp) ? plan_recurrence(ctx, F.p, F.g.n0, F.g.n1) : RowRecurrence{};
    E.step0 = rr.step0;
    R.R1.setup(E);
    if (!R.R1.on) R.SR.setup(E, rr);
    ChainRun &CR = R.CR;
    // (series fits: a call of ONE series -- the last device call of 3 + 3 + 1 -- stays on the chain kernels, which read per-chain data; the
    //  time-resident kernel reads the shared tables)
    if (!ctx->series.data) R.RR.setup(E, F.n_chains, gp.fast, rr.use_rec, R.psz);
    if (!R.RR.on) CR.setup(E, gp.fast, rr.use_rec, R.psz);
    if (R.RR.on || CR.on) ctx->psumF.ensure(R.psz * 8);
    if (CR.on && CR.depad) {                 // a padded batch that hands its posteriors out: scratch sequence for the kernels, ctx->post stays the result
        ctx->postpad.ensure((size_t)B * T * CR.Gk * 8);
        E.d_post = ctx->postpad.as<double>();
    } else if (CR.on && (CR.cp.pad || CR.ax1) && E.d_post) {      // the private sequence of a padded chain-resident batch lives on the padded geometry
        ctx->post.ensure((size_t)B * T * CR.Gk * 8);
        E.d_post = ctx->post.as<double>();
    }
    return R;
}

// The attempts of a batch, as the schedule hands them out, until its passes went through (BATCH_FINISH) or the call has to go back to an
// earlier batch (BATCH_REWIND).  usedK: in, the K of the first attempt; out, of the one that went through
BatchStep run_attempts(BatchSchedule &sched, BatchRun &R, int base_variant, int64_t &usedK) {
    blhip_ctx *ctx = R.E.ctx;
    const ChainRun &CR = R.CR;
    for (bool first = true;; first = false) {
        PassFacts f;
        f.ok = run_passes(R, usedK);
        f.resident_failed = R.resident_failed; f.cr_on = CR.on; f.touched_parts = CR.touched_parts; f.part_fresh0 = CR.part_fresh0;
        f.part_live = ctx->part.live; f.part_first_batch = ctx->part.first_batch;
        const BatchStep s = sched.after_passes(R.E.bi, f);
        if (s.action == BATCH_FINISH) {
            if (first && (R.RR.on || CR.on || ctx->timing.fwd_kernel_variant == 8)) ctx->resident.passed();
            return s;
        }
        if (s.action == BATCH_INTERNAL_ERROR) fail("internal: the launch-per-step pass failed after the resident pass gave up");
        // (series on a two-parameter grid: the kernels a repeat would run on read series 0's tables -- the caller runs its loop)
        if (const char *why = series_route_refusal(ctx->series.data != nullptr, R.E.p->ndim, CR.on, CR.clamp, true))
            fail("series fit: %s (a grid of 2 parameters, batch %lld of the call)", why, (long long)R.E.bi);
        if (s.action == BATCH_REPEAT_K1) { usedK = 1; continue; }
        // a resident pass gave up or failed: the launch-per-step kernels take over (timing of the failed attempt is dropped)
        ctx->timing.resident_fallbacks += 1;
        ctx->timing.resident_fallback_reason = ctx->resident_last_reason ? ctx->resident_last_reason : BLHIP_FALLBACK_RANGE;
        reset_pass_timing(ctx);
        if (s.action == BATCH_REWIND) {              // (the slots its backward pass has added to carry earlier batches: they are dropped)
            ctx->part = blhip_ctx::PartState{};
            return s;
        }
        ctx->timing.fwd_kernel_variant = ctx->timing.bwd_kernel_variant = base_variant;
        if (CR.on && CR.depad) R.E.d_post = ctx->post.as<double>();      // (no scratch sequence: the launch-per-step kernels write the result)
    }
}

// the folds nobody waited for: the last one(s) before anybody reads the accumulator; their time from their events
void collect_fold_times(blhip_ctx *ctx, hipStream_t st, std::vector<hipEvent_t> &fold_ev) {
    if (fold_ev.empty()) return;
    sync_stream(ctx, st);
    for (size_t k = 0; k + 1 < fold_ev.size(); k += 2) {
        float fms = 0;
        HIPCHECK(hipEventElapsedTime(&fms, fold_ev[k], fold_ev[k + 1]));
        ctx->timing.accumulate_ms += fms;
    }
    for (hipEvent_t e : fold_ev) (void)hipEventDestroy(e);
}

void do_fit(blhip_ctx *ctx, const blhip_problem *p_in, int64_t n_chains, const double *op_values,
            const double *log_w, uint32_t flags, blhip_result *res) {
    Trace tr(ctx->option("trace", 0.0) != 0.0);
    // Series armed (blhip_set_series): THIS fit takes them over, whatever becomes of it.  Chain c observes series c; problem->data is
    // ignored (the checks and the shared tables below read series 0 in its place; the recurrence's envelope every series: plan_recurrence).
    // One-parameter grids: Row1dRun::series_table; two-parameter grids: ChainRun::series_tables, and no route but the chain kernels'.
    struct SeriesScope {
        blhip_ctx *c;
        explicit SeriesScope(blhip_ctx *ctx) : c(ctx) {
            c->series.data = c->series.armed; c->series.S = c->series.armed_S; c->series.H = c->series.armed_H; c->series.grouped = c->series.armed_grouped;
            c->series.fold = false;
            c->series.armed = nullptr; c->series.armed_S = 0; c->series.armed_H = 1; c->series.armed_grouped = false;
        }
        ~SeriesScope() { c->series.data = nullptr; c->series.S = 0; c->series.H = 1; c->series.grouped = false; c->series.fold = false; }
    } series_scope(ctx);
    const bool series = ctx->series.data != nullptr;
    blhip_problem p_series;
    if (series) {
        if (!p_in) fail("problem is NULL");
        const int64_t SH = ctx->series.H;
        if (!ctx->series.grouped && n_chains != ctx->series.S)
            fail("series fit: %lld series are armed, the fit has %lld chains", (long long)ctx->series.S, (long long)n_chains);
        if (ctx->series.grouped && n_chains != ctx->series.S * SH)
            fail("series fit: %lld series in groups of %lld chains are armed, the fit has %lld chains", (long long)ctx->series.S, (long long)SH, (long long)n_chains);
        p_series = *p_in;
        p_series.data = ctx->series.data;
        p_in = &p_series;
        char why[256] = "";
        if (series_group_check(p_in, ctx->series.S, SH, (int)flags, why, (int)sizeof why) != 0) fail("series fit: %s", why);
        if (ctx->option("series_fit", 1.0) == 0.0) fail("series fit: option series_fit = 0");
        ctx->series.om = p_in->obs_model;
        // BLHIP_ACCUMULATE with groups: every group is folded into its OWN average behind the batch's passes (series_group_fold); the
        // context's accumulator (blhip_accum_*) is neither used nor changed -- the fit itself runs without the flag
        if ((flags & BLHIP_ACCUMULATE) && !(flags & BLHIP_EVIDENCE_ONLY)) {
            if (!(flags & BLHIP_KEEP_POSTERIOR)) fail("series fit: the grouped fold leaves its averages as the kept posterior: BLHIP_ACCUMULATE needs BLHIP_KEEP_POSTERIOR here");
            if (!log_w) fail("BLHIP_ACCUMULATE needs log_chain_weight");
            ctx->series.fold = true;
        }
        flags &= ~(uint32_t)BLHIP_ACCUMULATE;
    }
    validate(p_in, n_chains, op_values);
    if (p_in->ndim > 2) { ctx->prior_token = 0; do_fit_nd(ctx, p_in, n_chains, op_values, log_w, flags, res); return; }      // (that path lays the tables buffer out its own way)
    // closed-form models without an in-kernel likelihood: their (T, G) table is built on the device, the step kernels
    // then see a tabulated likelihood
    blhip_problem p_local = *p_in;
    // (... and models whose density is a program: bllp::lik_program_kernel)
    const int table_model = (p_in->obs_model >= BLHIP_OM_BERNOULLI && p_in->obs_model <= BLHIP_OM_PROGRAM) ? p_in->obs_model : 0;
    if (table_model) p_local.obs_model = BLHIP_OM_TABLE;
    const blhip_problem *p = &p_local;
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const FitFlags ff = decode_flags(ctx, p, flags, log_w);

    Geometry g{};
    if (p->ndim == 1) { g.n0 = 1; g.n1 = (int)p->n[0]; g.axis_map[0] = 1; g.axis_map[1] = 1; }
    else { g.n0 = (int)p->n[0]; g.n1 = (int)p->n[1]; g.axis_map[0] = 0; g.axis_map[1] = 1; }
    g.G = (long long)g.n0 * g.n1;
    if (ff.accumulate && (ctx->acc_T != p->T || ctx->acc_G != g.G)) fail("accumulator shape mismatch");
    double dV = 1.0;
    for (int k = 0; k < p->ndim; ++k) dV *= p->lattice[k];
    begin_fit(ctx);

    const DeviceTables DT = upload_tables(ctx, p, g, ff, table_model);
    tr.mark("tables + H2D");
    // the memory plan: the batches of the call
    const std::vector<int64_t> batch_start = plan_fit_batches(ctx, p, g, ff, n_chains, op_values);
    const int64_t nbatch = (int64_t)batch_start.size() - 1;
    ctx->timing.batches = nbatch;
    tr.mark("memory budget");
    HIPCHECK(hipEventRecord(ctx->ev[6], st));

    std::vector<hipEvent_t> fold_ev;
    const FitCall F{ctx, p, st, ff, g, dV, n_chains, nbatch, log_w, res, &DT, &tr, &fold_ev};
    BatchPrograms programs(p, g, batch_start, op_values, ff.resume);
    BatchSchedule sched(nbatch);
    while (sched.more()) {
        const int64_t bi = sched.batch(), c0 = batch_start[bi], B = batch_start[bi + 1] - c0;
        tr.mark("batch setup");
        BatchProgram &BP = programs.take(bi);
        tr.mark("build_program");
        const GeometryPlan gp = plan_geometry(ctx, p, g, BP.prog, B, DT.d, ff.resume, ff.carry, &BP.taps);
        if (series && p->ndim == 1 && !gp.chain1d)
            fail("series fit: the chain-resident 1-D kernel does not take this batch (%d cells, radius %d%s; options chain1d / chain1d_long / chain1d_shift / "
                 "chain1d_clamp / fuse1d)", g.n1, BP.prog.LW1, BP.prog.multi ? ", a composed transition" : "");
        const int base_variant = gp.fast ? 1 : (gp.fused1d ? 4 : 0);
        ctx->timing.fwd_kernel_variant = ctx->timing.bwd_kernel_variant = base_variant;
        ctx->timing.cells_per_launch = std::max<int64_t>(ctx->timing.cells_per_launch, B * g.G);
        DeviceMeta M;
        upload_metadata(ctx, p, BP.prog, BP.taps, B, ff.full, gp.fast, gp.tile.nblk, M, gp.wideH, gp.wideV, gp.hSplit, gp.hFusedMax);
        tr.mark("buckets + metadata H2D");

        BatchRun R = setup_batch(F, bi, c0, B, BP, gp, M, sched.allow_chainres(bi));
        // (series on a two-parameter grid: every route but blc::chain_kernel / blc::chainax_kernel reads series 0's tables)
        if (const char *why = series_route_refusal(series, p->ndim, R.CR.on && !R.RR.on && !R.R1.on, R.CR.clamp, false))
            fail("series fit: %s (a grid of 2 parameters, %d x %d, batch of %lld chains; options chain_resident / chain_table / chain_ax1 / chain_depad)",
                 why, g.n0, g.n1, (long long)B);
        int64_t usedK = gp.fusedK;
        if (run_attempts(sched, R, base_variant, usedK).action == BATCH_REWIND) {
            programs.drop();
            sync_stream(ctx, st);
            continue;
        }
        const BatchPath path = R.path();
        const bool went_into_slots = path == PATH_CHAIN && R.CR.fused && R.CR.fold_done && std::isfinite(R.CR.fold_ref);
        finish_batch(R, path, usedK, sched.finished(bi, went_into_slots), nbatch, res);
    }
    flush_partials(ctx, st, &fold_ev);         // the carried partial accumulators of the chain-resident fold -> the average posterior
    collect_fold_times(ctx, st, fold_ev);
    tr.mark("batches done");
    HIPCHECK(hipEventRecord(ctx->ev[7], st));
    HIPCHECK(hipEventSynchronize(ctx->ev[7]));
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]));
    tr.mark("final sync");
    ctx->timing.total_ms = ms;
}

}  // namespace

// Page-locked result arrays.  hipHostMalloc of 16 GiB takes 2.2 s (one thread allocates, zeroes and pins four million pages) -- more
// than the copy it is meant to speed up.  Here the block is an anonymous mapping pinned in PIN_CHUNK pieces (hipHostRegister faults
// the pages in and locks them: 1.06 s for 16 GiB; more threads are slower); the read-backs below copy piece by piece, so every
// DMA lands inside one registered range.  The Python side pins in the background (bayesloop_amd/engine.py: _PinnedPool).
namespace {
constexpr size_t PIN_CHUNK = (size_t)256 << 20;
struct PinnedBlock { size_t bytes; std::vector<char> ok; };
std::mutex g_pin_mu;
std::map<void *, PinnedBlock> g_pinned;

// pieces [a, b) of a host destination such that no piece crosses a chunk boundary of a block of blhip_host_alloc (any other
// destination: one piece)
template <class F> void for_pinned_pieces(void *host, size_t bytes, F &&f) {
    char *base = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pinned.upper_bound(host);
        if (it != g_pinned.begin()) {
            --it;
            if ((char *)host >= (char *)it->first && (char *)host + bytes <= (char *)it->first + it->second.bytes) base = (char *)it->first;
        }
    }
    if (!base) { f((char *)host, bytes); return; }
    char *p = (char *)host, *end = p + bytes;
    while (p < end) {
        const size_t into = (size_t)(p - base) % PIN_CHUNK;
        const size_t n = std::min<size_t>(PIN_CHUNK - into, (size_t)(end - p));
        f(p, n);
        p += n;
    }
}
}  // namespace

extern "C" {

int blhip_abi_version(void) { return BLHIP_ABI_VERSION; }

int64_t blhip_kernel_census(char *buf, int64_t cap) {
    try {
        // (the names live in ONE arena and the temporaries are reused: a string of its own per kernel was ~1500 small heap blocks allocated
        //  and freed per call -- the tests take a census around every fit)
        struct Row { size_t off, len; unsigned long long launches; };
        std::vector<Row> rows;
        std::string arena, name;
        arena.reserve((size_t)1 << 17);
        char *dm = nullptr;
        size_t dmlen = 0;
        struct FreeDm { char *&p; ~FreeDm() { std::free(p); } } free_dm{dm};
        const std::string pre = "blreg::Site<&(", post = ")>";
        for (blreg::Entry *e = blreg::head().load(std::memory_order_acquire); e; e = e->next) {
            // typeid name of blreg::Site<&kernel>: demangled "blreg::Site<&blc::chain_kernel<4, 1, false, false, false, false>(blc::ChainParams)>"
            int status = 0;
            char *r = abi::__cxa_demangle(e->mangled, dm, &dmlen, &status);      // (dm: malloc'ed, grown by the demangler as needed)
            if (r) dm = r;
            name.assign((status == 0 && r) ? r : (e->mangled ? e->mangled : "?"));
            // -> "blreg::Site<&(void blc::chain_kernel<10, 1, false, false, false, false>(blc::ChainParams))>": keep the kernel with its template arguments
            if (name.size() > pre.size() + post.size() && name.compare(0, pre.size(), pre) == 0 && name.compare(name.size() - post.size(), post.size(), post) == 0) {
                name.erase(name.size() - post.size());
                name.erase(0, pre.size());
                if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);
                if (!name.empty() && name.back() == ')') {            // the parameter list: the last top-level parenthesis group
                    int depth = 0;
                    for (size_t k = name.size(); k-- > 0;) {
                        if (name[k] == ')') ++depth;
                        else if (name[k] == '(' && --depth == 0) { name.erase(k); break; }
                    }
                }
            }
            else if (name.compare(0, 13, "blreg::Site<&") == 0 && name.back() == '>') { name.erase(name.size() - 1); name.erase(0, 13); }      // (a kernel that is no template)
            rows.push_back(Row{arena.size(), name.size(), e->launches.load(std::memory_order_relaxed)});
            arena += name;
        }
        auto view = [&](const Row &r) { return std::string_view(arena.data() + r.off, r.len); };
        std::sort(rows.begin(), rows.end(), [&](const Row &a, const Row &b) { const int c = view(a).compare(view(b)); return c != 0 ? c < 0 : a.launches < b.launches; });
        std::string out;
        out.reserve(arena.size() + 24 * rows.size());
        for (const Row &r : rows) {
            char num[24];
            const int nn = std::snprintf(num, sizeof num, "%llu", r.launches);
            out.append(num, (size_t)nn);
            out.push_back('\t');
            out.append(arena, r.off, r.len);
            out.push_back('\n');
        }
        if (buf && cap > 0) {
            const size_t n = std::min<size_t>((size_t)cap - 1, out.size());
            std::memcpy(buf, out.data(), n);
            buf[n] = 0;
        }
        return (int64_t)out.size();
    } catch (...) {
        return -1;
    }
}

int blhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

blhip_ctx *blhip_create(int device) {
    blhip_ctx *ctx = nullptr;
    try {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) fail("no HIP device visible");
        if (device < 0 || device >= n) fail("device %d out of range (%d visible)", device, n);
        HIPCHECK(hipSetDevice(device));
        ctx = new blhip_ctx();
        ctx->device = device;
        HIPCHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        for (auto &e : ctx->ev) HIPCHECK(hipEventCreate(&e));
        for (auto &bs : ctx->bstream) HIPCHECK(hipStreamCreateWithFlags(&bs, hipStreamNonBlocking));
        for (auto &e : ctx->bev) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&ctx->sync_ev, hipEventDisableTiming));
        HIPCHECK(hipStreamCreateWithFlags(&ctx->cstream, hipStreamNonBlocking));
        for (auto &e : ctx->cev) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        hipDeviceProp_t prop;
        HIPCHECK(hipGetDeviceProperties(&prop, device));
        ctx->num_cus = prop.multiProcessorCount;
        if (prop.maxGridSize[1] > 0) ctx->max_grid_y = prop.maxGridSize[1];
        std::string marketing = prop.name;
        if (marketing.find_first_not_of(' ') == std::string::npos) marketing = "AMD Instinct (name not reported by the driver)";
        ctx->name = marketing + " (" + prop.gcnArchName + ")";
        return ctx;
    } catch (const Fail &e) {
        g_create_error = e.msg;
    } catch (...) {
        g_create_error = "unknown error in blhip_create";
    }
    delete ctx;
    return nullptr;
}

void blhip_destroy(blhip_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)blhip_comm_destroy(ctx);
    ctx->commbuf.release(); ctx->pinC.release(); ctx->resx.release(); ctx->postpad.release(); ctx->accw.release(); ctx->accpart.release(); ctx->xch.release(); ctx->axlik.release(); ctx->anchbuf.release(); ctx->probebuf.release(); ctx->p1d.release(); ctx->p1w.release(); ctx->lik1d.release(); ctx->likprog_dev.release(); ctx->predws.release(); ctx->predx.release(); ctx->queryws.release(); ctx->mixseq.release(); ctx->mixw.release();
    for (DevBuf *b : {&ctx->state, &ctx->post, &ctx->psumF, &ctx->psumB, &ctx->redF, &ctx->redB, &ctx->meta,
                      &ctx->tables, &ctx->likbuf, &ctx->small, &ctx->accum_own, &ctx->stats, &ctx->mix, &ctx->unit, &ctx->databuf, &ctx->postinv})
        b->release();
    for (auto &kv : ctx->carry) kv.second.buf.release();
    ctx->pinF.release(); ctx->pinB.release(); ctx->pinS.release(); ctx->pinA.release();
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &bs : ctx->bstream)
        if (bs) { (void)hipStreamSynchronize(bs); (void)hipStreamDestroy(bs); }
    for (auto &e : ctx->bev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    if (ctx->sync_ev) (void)hipEventDestroy(ctx->sync_ev);
    if (ctx->cstream) { (void)hipStreamSynchronize(ctx->cstream); (void)hipStreamDestroy(ctx->cstream); }
    for (auto &e : ctx->cev) if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *blhip_last_error(blhip_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int blhip_device_name(blhip_ctx *ctx, char *buf, int buflen) {
    if (!ctx || !buf || buflen <= 0) return -1;
    std::snprintf(buf, (size_t)buflen, "%s", ctx->name.c_str());
    return 0;
}

int blhip_host_unlag(int scheme, double *sums, int64_t T, int lag, const unsigned char *kinds, double *scales_out) {
    if (!sums || T < 1 || lag < 1) return -1;
    try {
        std::vector<double> red((size_t)T * NRED, 0.0), rowsum, scales;
        for (int64_t t = 0; t < T; ++t) red[(size_t)t * NRED] = sums[t];
        // (scheme 2: bit 6 of a step's kind marks a clamped step -- exact scale; the other bits are its source kind as in scheme 1)
        std::vector<unsigned char> src, clamped;
        if (scheme == 2 && kinds) {
            src.resize((size_t)T); clamped.resize((size_t)T);
            for (int64_t t = 0; t < T; ++t) { src[t] = kinds[t] & 0x3f; clamped[t] = (kinds[t] & 0x40) ? 1 : 0; }
        }
        const bool ok = scheme == 0 ? resident_unlag(red.data(), T, lag, rowsum)
                      : (scheme == 2 && kinds ? chain_unlag(red.data(), T, lag, rowsum, 1, 0, &scales, src.data(), 0, clamped.data())
                                              : chain_unlag(red.data(), T, lag, rowsum, 1, 0, &scales, kinds));
        if (!ok) return 1;
        for (int64_t t = 0; t < T; ++t) sums[t] = red[(size_t)t * NRED];
        if (scales_out)
            for (int64_t t = 0; t < T; ++t) scales_out[t] = scheme == 0 ? (t >= lag ? 1.0 / rowsum[t - lag] : 1.0) : scales[t];
        return 0;
    } catch (...) {
        return -1;
    }
}

int blhip_host_rec_envelope(const blhip_problem *p, double *bound_out) {
    if (!p || p->ndim != 2 || p->obs_model != BLHIP_OM_GAUSSIAN || !p->marginal[0] || !p->marginal[1] || !p->data || p->n[0] < 2 || p->n[1] < 1 ||
        p->T < 1 || p->seg_len < 1 || p->data_dim < 1)
        return -1;
    const double b = rec_envelope_bound(p->marginal[0], (int)p->n[0], p->marginal[1], (int)p->n[1], p->data, p->T * p->seg_len, p->data_dim);
    if (bound_out) *bound_out = b;
    return b <= REC_ENVELOPE ? 1 : 0;
}

int blhip_host_poisson_direct(const blhip_problem *p, int *direct_out) {
    if (!p || p->ndim != 1 || p->obs_model != BLHIP_OM_POISSON || !p->marginal[0] || !p->data || p->n[0] < 1 || p->T < 1 || p->seg_len != 1 ||
        p->data_dim < 1)
        return -1;
    const double max_rate = max_of(p->marginal[0], p->n[0]);
    int n_direct = 0;
    for (int64_t t = 0; t < p->T; ++t) {
        const bool direct = poisson_direct_domain(p->data + t * p->data_dim, p->data_dim, max_rate);
        if (direct_out) direct_out[t] = direct ? 1 : 0;
        n_direct += direct ? 1 : 0;
    }
    return n_direct;
}

int64_t blhip_host_taps(int kind, int64_t n, const double *params, int n_params, double *out, int64_t cap, int *radius_out) {
    static const int need[4] = {1, 1, 2, 3};
    if (kind < 0 || kind > 3 || !params || n_params != need[kind]) return -1;
    for (int k = 0; k < n_params; ++k)
        if (!std::isfinite(params[k])) return -1;
    try {
        TapTable taps;
        int id = -1;
        if (kind == 0) {
            if (!(params[0] > 0.0) || params[0] > 1e6) return -1;
            id = taps.get(0, params[0]);
        } else if (kind == 1) {
            if (std::fabs(params[0]) > 12.0) return -1;
            id = taps.get_shift(0, params[0]);
        } else if (kind == 2) {
            // (the builder is O(n^2) cosines in long double: no longer than a grid axis the kernels take; transitionModels.py:202: 0 < alpha <= 2)
            if (n < 2 || n > 16384 || !(params[0] > 0.0) || !(params[1] > 0.0) || params[1] > 2.0) return -1;
            id = taps.get_alphastable(0, params[0], params[1], (int)n);
        } else {
            if (!(params[0] > 0.0) || !(params[1] > 0.0) || !(std::fabs(params[2]) < 1.0) || params[0] > 1e3 || params[1] > 1e3) return -1;
            id = taps.get2d(params[0], params[1], params[2]);
        }
        if (id < 0) {                                  // a walk of radius 0: the identity, one weight
            if (radius_out) radius_out[0] = radius_out[1] = 0;
            if (out && cap >= 1) out[0] = 1.0;
            return 1;
        }
        const int r = taps.lw[id], r1 = kind == 3 ? taps.lw2[id] : 0;
        if (radius_out) { radius_out[0] = r; radius_out[1] = r1; }
        const double *w = taps.w.data() + taps.off[id];
        std::vector<double> full;
        if (kind == 0) {                               // stored as the half kernel w[0 .. r]
            full.resize(2 * (size_t)r + 1);
            for (int k = -r; k <= r; ++k) full[(size_t)(k + r)] = w[std::abs(k)];
        } else {
            const size_t count = kind == 1 ? 2 * (size_t)r + 1 : kind == 2 ? (size_t)n : (2 * (size_t)r + 1) * (2 * (size_t)r1 + 1);
            full.assign(w, w + count);
        }
        if (out)
            for (size_t k = 0; k < full.size() && (int64_t)k < cap; ++k) out[k] = full[k];
        return (int64_t)full.size();
    } catch (...) {
        return -1;
    }
}

int blhip_host_lik_program_check(const int32_t *ops, int64_t n_ops, int64_t n_consts, int64_t n_step, int ndim, char *err, int errlen) {
    return bllp::check_program(ops, n_ops, n_consts, n_step, ndim, err, errlen);
}

int blhip_set_lik_program(blhip_ctx *ctx, const int32_t *ops, int64_t n_ops, const double *consts, int64_t n_consts,
                          const double *step_values, int64_t n_step, int64_t n_step_values) {
    return guarded(ctx, [&] {
        ctx->likprog.armed = false;
        char msg[256] = "";
        if (bllp::check_program(ops, n_ops, n_consts, n_step, BLHIP_MAX_DIM, msg, (int)sizeof msg) != 0) fail("blhip_set_lik_program: %s", msg);
        if ((n_consts > 0 && !consts) || n_step_values < 0 || (n_step_values > 0 && !step_values)) fail("blhip_set_lik_program: consts / step_values is NULL");
        if (n_step == 0 ? n_step_values != 0 : n_step_values % n_step != 0)
            fail("blhip_set_lik_program: %lld step values are no (T, data_dim, n_step = %lld) array", (long long)n_step_values, (long long)n_step);
        blhip_ctx::LikProgram &LP = ctx->likprog;
        LP.ops.assign(ops, ops + 2 * n_ops);
        LP.consts.assign(consts, consts + n_consts);
        LP.step.assign(step_values, step_values + n_step_values);
        LP.n_step = n_step;
        LP.armed = true;
    });
}

int blhip_set_series(blhip_ctx *ctx, const double *data, int64_t S) {
    return guarded(ctx, [&] {
        ctx->series.armed = nullptr; ctx->series.armed_S = 0; ctx->series.armed_H = 1; ctx->series.armed_grouped = false;
        if (!data || S < 1) fail("blhip_set_series: data is NULL or S < 1");
        ctx->series.armed = data; ctx->series.armed_S = S;
    });
}

int blhip_set_series_groups(blhip_ctx *ctx, const double *data, int64_t S, int64_t H) {
    return guarded(ctx, [&] {
        ctx->series.armed = nullptr; ctx->series.armed_S = 0; ctx->series.armed_H = 1; ctx->series.armed_grouped = false;
        if (!data || S < 1 || H < 1) fail("blhip_set_series_groups: data is NULL, S < 1 or H < 1");
        ctx->series.armed = data; ctx->series.armed_S = S; ctx->series.armed_H = H; ctx->series.armed_grouped = true;
    });
}

int blhip_host_series_group_check(const blhip_problem *problem, int64_t S, int64_t H, int flags, char *err, int errlen) {
    return series_group_check(problem, S, H, flags, err, errlen);
}

int blhip_host_series_group_plan(const blhip_problem *problem, int64_t S, int64_t H, int flags, double budget, int64_t max_batch, int64_t *plan_out,
                                 char *err, int errlen) {
    return series_group_plan(problem, S, H, flags, budget, max_batch, plan_out, err, errlen);
}

int blhip_host_series_check(const blhip_problem *problem, int64_t S, int flags, char *err, int errlen) {
    return series_check(problem, S, flags, err, errlen);
}

int blhip_host_series_plan(const blhip_problem *problem, int64_t S, int flags, double budget, int64_t *plan_out) {
    return series_plan(problem, S, flags, budget, plan_out);
}

int blhip_lik_program_eval(blhip_ctx *ctx, int ndim, const int64_t *n, const double *const *marginal, int64_t T, int data_dim,
                           const double *data, double *out) {
    return guarded(ctx, [&] {
        if (ndim < 1 || ndim > BLHIP_MAX_DIM || !n || !marginal || T < 1 || data_dim < 1 || !data || !out) fail("blhip_lik_program_eval: bad arguments");
        HIPCHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        long long G = 1;
        size_t mb = 0;
        for (int k = 0; k < ndim; ++k) {
            if (n[k] < 1 || n[k] > (1ll << 30) || !marginal[k]) fail("blhip_lik_program_eval: bad grid axis %d", k);
            G *= n[k];
            mb += carve_size(8 * (size_t)n[k]);
        }
        ScopedDevBuf grid, table;
        grid.ensure(mb);
        table.ensure(8 * (size_t)T * G);
        char *cur = grid.as<char>();
        const double *dm[BLHIP_MAX_DIM] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < ndim; ++k) {
            double *d = carve<double>(cur, (size_t)n[k]);
            HIPCHECK(hipMemcpyAsync(d, marginal[k], 8 * (size_t)n[k], hipMemcpyHostToDevice, st));
            dm[k] = d;
        }
        build_program_table(ctx, ndim, n, dm, T, data_dim, data, table.as<double>());
        HIPCHECK(hipMemcpyAsync(out, table.p, 8 * (size_t)T * G, hipMemcpyDeviceToHost, st));
        sync_stream(ctx, st);
    });
}

int blhip_set_option(blhip_ctx *ctx, const char *key, double value) {
    if (!ctx || !key) return -1;
    // "resident_ok": the context's memory of a resident launch that gave up (its blocks were not all co-resident) -- settable so that
    // a caller (the tests of the fall-back) can re-arm the resident paths
    if (std::strcmp(key, "resident_ok") == 0) { ctx->resident.set_ok(value != 0.0); return 0; }
    if (std::strcmp(key, "resident_retry_after") == 0) { ctx->resident.retry_after = std::max(1, (int)value); return 0; }
    // (a key the library never reads is an error, not a silent no-op: an A/B run over a removed option measured nothing -- ADVICE r05)
    static const char *const known[] = {
        "bins_gw", "bins_sb", "bins_slab", "carry_partials", "chain1d", "chain1d_clamp", "chain1d_long", "chain1d_shift", "chain_ax1", "chain_clamp", "chain_depad", "chain_prof", "chain_resident", "chain_resident_lag",
        "chain_force_fail_batch", "chain_force_fail_stage", "chain_nd", "chain_nd_stages", "chain_table", "chain_wide", "comm_reduce_mode", "fast", "fast_S", "fold2", "fold2_cp", "fold4", "fold4_min_chains", "fold_force_fail_batch", "fuse1d", "fuse_accumulate", "late_sums", "lik_program", "max_batch",
        "mem_budget_bytes", "mfma", "mfma_S", "mfma_h", "mfma_h_max_cells", "online_block", "parser_device", "parser_pair_max", "peer_copy_mode", "persist1d", "predictive", "quiet", "recurrence", "resident",
        "resident_force_abort", "resident_lag", "resident_probe", "resident_probe_force_busy", "resident_probe_interval_s", "resident_probe_timeout_s",
        "resident_table", "resident_timeout_s", "series_fit", "share_prefix", "short_first_batch", "skip_prefix", "trace", "wide_h",
        "wide_h_fused_max", "wide_h_split", "wide_v"};
    bool ok = false;
    for (const char *k : known) ok = ok || std::strcmp(key, k) == 0;
    if (!ok) {
        ctx->err = std::string("blhip_set_option: unknown option '") + key + "' (README.md lists the options the library reads)";
        return -1;
    }
    ctx->opt[key] = value;
    return 0;
}

int blhip_synchronize(blhip_ctx *ctx) {
    return guarded(ctx, [&] {
        HIPCHECK(hipSetDevice(ctx->device));
        sync_stream(ctx, ctx->stream);
    });
}

int blhip_fit(blhip_ctx *ctx, const blhip_problem *problem, int64_t n_chains, const double *op_values,
              const double *log_chain_weight, uint32_t flags, blhip_result *result) {
    return guarded(ctx, [&] { do_fit(ctx, problem, n_chains, op_values, log_chain_weight, flags, result); });
}

int blhip_bandwidth_probe(blhip_ctx *ctx, int64_t bytes, int iterations, double *gb_per_s) {
    return guarded(ctx, [&] {
        if (!gb_per_s || bytes < (1 << 20) || iterations < 1) fail("blhip_bandwidth_probe: bad arguments");
        HIPCHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const long long n2 = bytes / 16;
        ScopedDevBuf a, b;          // (released on every exit path, also when a HIPCHECK below throws)
        a.ensure((size_t)n2 * 16); b.ensure((size_t)n2 * 16);
        BL_LAUNCH(fill_kernel, dim3(2048), dim3(256), 0, st, a.as<double>(), n2 * 2, 1.0);
        const unsigned gx = (unsigned)((n2 + 4 * NTHREADS - 1) / (4 * NTHREADS));
        double best = 0.0;
        for (int variant = 0; variant < 2; ++variant) {
            auto go = [&](const double2 *src, double2 *dst) {
                if (variant) BL_LAUNCH(copy16_kernel<true>, dim3(gx), dim3(NTHREADS), 0, st, src, dst, n2);
                else BL_LAUNCH(copy16_kernel<false>, dim3(gx), dim3(NTHREADS), 0, st, src, dst, n2);
            };
            go(a.as<double2>(), b.as<double2>());                                                   // warm-up
            HIPCHECK(hipEventRecord(ctx->ev[4], st));
            for (int k = 0; k < iterations; ++k) go((k & 1) ? b.as<double2>() : a.as<double2>(), (k & 1) ? a.as<double2>() : b.as<double2>());
            HIPCHECK(hipEventRecord(ctx->ev[5], st));
            HIPCHECK(hipGetLastError());
            sync_stream(ctx, st);
            float ms = 0;
            HIPCHECK(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
            best = std::max(best, 2.0 * (double)n2 * 16.0 * iterations / ((double)ms * 1e-3) / 1e9);
        }
        for (int variant = 0; variant < 2; ++variant) {
            // a store-only stream (what the no-stencil forward chain kernel does) can run above the copy rate: the calibrated peak is
            // the best of the streams measured
            auto go = [&](double2 *dst, double v) {
                if (variant) BL_LAUNCH(fill16_kernel<true>, dim3(gx), dim3(NTHREADS), 0, st, dst, n2, v);
                else BL_LAUNCH(fill16_kernel<false>, dim3(gx), dim3(NTHREADS), 0, st, dst, n2, v);
            };
            go(b.as<double2>(), 2.0);
            HIPCHECK(hipEventRecord(ctx->ev[4], st));
            for (int k = 0; k < iterations; ++k) go((k & 1) ? a.as<double2>() : b.as<double2>(), 3.0);
            HIPCHECK(hipEventRecord(ctx->ev[5], st));
            HIPCHECK(hipGetLastError());
            sync_stream(ctx, st);
            float ms = 0;
            HIPCHECK(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
            best = std::max(best, (double)n2 * 16.0 * iterations / ((double)ms * 1e-3) / 1e9);
        }
        *gb_per_s = best;
    });
}

int blhip_last_timing(blhip_ctx *ctx, blhip_timing *out) {
    if (!ctx || !out) return -1;
    *out = ctx->timing;
    out->resident_armed = ctx->resident.ok ? 1 : 0;
    return 0;
}

void *blhip_host_alloc(size_t bytes) {
    if (bytes == 0) return nullptr;
    const size_t len = (bytes + 4095) / 4096 * 4096;
    void *p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) return nullptr;
    const size_t nchunk = (len + PIN_CHUNK - 1) / PIN_CHUNK;
    PinnedBlock blk{len, std::vector<char>(nchunk, 0)};
    int nthreads = 1;      // (measured, 16 GiB: 1 thread 1.06 s, 4: 1.8 s, 16: 2.1 s -- the page-table lock serialises them; hipHostMalloc: 2.2 s)
    if (const char *e = std::getenv("BLHIP_PIN_THREADS")) nthreads = std::max(1, std::atoi(e));
    nthreads = (int)std::min<size_t>((size_t)nthreads, nchunk);
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        (void)hipSetDevice(dev);
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= nchunk) break;
            char *c = (char *)p + k * PIN_CHUNK;
            const size_t n = std::min(PIN_CHUNK, len - k * PIN_CHUNK);
            if (hipHostRegister(c, n, hipHostRegisterDefault) == hipSuccess) blk.ok[k] = 1;
            else (void)hipGetLastError();
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    bool all = true;
    for (char o : blk.ok) all = all && o;
    if (!all) {
        for (size_t k = 0; k < nchunk; ++k) if (blk.ok[k]) (void)hipHostUnregister((char *)p + k * PIN_CHUNK);
        munmap(p, len);
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pinned[p] = std::move(blk);
    return p;
}

void blhip_host_free(void *p) {
    if (!p) return;
    PinnedBlock blk;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pinned.find(p);
        if (it == g_pinned.end()) return;
        blk = std::move(it->second);
        g_pinned.erase(it);
    }
    for (size_t k = 0; k < blk.ok.size(); ++k) (void)hipHostUnregister((char *)p + k * PIN_CHUNK);
    munmap(p, blk.bytes);
}

int blhip_posterior_read(blhip_ctx *ctx, int64_t chain, int64_t t0, int64_t t1, double *host_out) {
    return guarded(ctx, [&] {
        if (!ctx->post_valid) fail("no posterior kept (run blhip_fit with BLHIP_KEEP_POSTERIOR)");
        ensure_post_scaled(ctx);
        if (chain < 0 || chain >= ctx->post_chains || t0 < 0 || t1 > ctx->post_T || t0 > t1 || !host_out)
            fail("blhip_posterior_read: bad range");
        HIPCHECK(hipSetDevice(ctx->device));
        const char *src = reinterpret_cast<const char *>(ctx->post.as<double>() + ((size_t)chain * ctx->post_T + t0) * ctx->post_G);
        for_pinned_pieces(host_out, (size_t)(t1 - t0) * ctx->post_G * 8, [&](char *dst, size_t n) {
            HIPCHECK(hipMemcpyAsync(dst, src + (dst - (char *)host_out), n, hipMemcpyDeviceToHost, ctx->stream));
        });
        sync_stream(ctx, ctx->stream);
    });
}

int blhip_posterior_devptr(blhip_ctx *ctx, void **devptr, int64_t *chain_stride, int64_t *step_stride) {
    return guarded(ctx, [&] {
        if (!ctx->post_valid) fail("no posterior kept");
        ensure_post_scaled(ctx);
        sync_stream(ctx, ctx->stream);
        if (devptr) *devptr = ctx->post.p;
        if (chain_stride) *chain_stride = ctx->post_T * ctx->post_G;
        if (step_stride) *step_stride = ctx->post_G;
    });
}

int blhip_posterior_release(blhip_ctx *ctx) {
    return guarded(ctx, [&] {
        HIPCHECK(hipSetDevice(ctx->device));
        ctx->post_valid = false;
        ctx->post.release();
    });
}

namespace {
struct SeqView { const double *p; int64_t T; int n0, n1; };
SeqView sequence_view(blhip_ctx *ctx, int source, int64_t chain) {
    if (source == 0) {
        if (!ctx->post_valid) fail("no posterior kept (run blhip_fit with BLHIP_KEEP_POSTERIOR)");
        if (chain < 0 || chain >= ctx->post_chains) fail("chain out of range");
        ensure_post_scaled(ctx);
        return SeqView{ctx->post.as<double>() + (size_t)chain * ctx->post_T * ctx->post_G, ctx->post_T, ctx->post_n0, ctx->post_n1};
    }
    if (source == 1) {
        if (!ctx->acc_active || !ctx->acc_final) fail("accumulator not finalised");
        return SeqView{ctx->acc, ctx->acc_T, ctx->acc_n0, ctx->acc_n1};
    }
    fail("bad source %d", source);
}
}  // namespace

int blhip_posterior_marginal(blhip_ctx *ctx, int source, int64_t chain, int keep_axis, double *host_out) {
    return guarded(ctx, [&] {
        if (!host_out) fail("host_out is NULL");
        HIPCHECK(hipSetDevice(ctx->device));
        const SeqView v = sequence_view(ctx, source, chain);
        const bool one_d = v.n0 == 1;
        if (keep_axis < 0 || keep_axis > (one_d ? 0 : 1)) fail("keep_axis out of range");
        const int nk = one_d ? v.n1 : (keep_axis == 0 ? v.n0 : v.n1);
        ctx->stats.ensure((size_t)v.T * nk * 8);
        double *d_out = ctx->stats.as<double>();
        hipStream_t st = ctx->stream;
        if (one_d) {
            HIPCHECK(hipMemcpyAsync(d_out, v.p, (size_t)v.T * nk * 8, hipMemcpyDeviceToDevice, st));
        } else if (keep_axis == 0) {
            for_grid_y(ctx, v.T, [&](long long t0, unsigned nt) {
                BL_LAUNCH(marginal_rows_kernel, dim3(v.n0, nt), dim3(NTHREADS), 0, st, v.p + (size_t)t0 * v.n0 * v.n1, d_out + (size_t)t0 * nk, v.n0, v.n1);
            });
        } else {
            for_grid_y(ctx, v.T, [&](long long t0, unsigned nt) {
                BL_LAUNCH(marginal_cols_kernel, dim3((v.n1 + NTHREADS - 1) / NTHREADS, nt), dim3(NTHREADS), 0, st,
                                   v.p + (size_t)t0 * v.n0 * v.n1, d_out + (size_t)t0 * nk, v.n0, v.n1);
            });
        }
        HIPCHECK(hipMemcpyAsync(host_out, d_out, (size_t)v.T * nk * 8, hipMemcpyDeviceToHost, st));
        sync_stream(ctx, st);
    });
}

int blhip_posterior_time_average(blhip_ctx *ctx, int source, int64_t chain, double *host_out) {
    return guarded(ctx, [&] {
        if (!host_out) fail("host_out is NULL");
        HIPCHECK(hipSetDevice(ctx->device));
        const SeqView v = sequence_view(ctx, source, chain);
        const long long G = (long long)v.n0 * v.n1;
        ctx->stats.ensure((size_t)G * 8);
        double *d_out = ctx->stats.as<double>();
        hipStream_t st = ctx->stream;
        BL_LAUNCH(time_average_kernel, dim3((unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 4096)),
                           dim3(NTHREADS), 0, st, v.p, d_out, G, (int)v.T);
        HIPCHECK(hipMemcpyAsync(host_out, d_out, (size_t)G * 8, hipMemcpyDeviceToHost, st));
        sync_stream(ctx, st);
    });
}

int blhip_host_predictive_plan(int64_t G, int64_t T, int64_t X, int average, double budget, int64_t *plan_out) {
    if (!plan_out) return -1;
    blpp::PredPlan P;
    const bool ok = blpp::predictive_plan(G, T, X, average != 0, budget, P);
    if (!ok && P.min_budget_bytes == 0) return -1;
    plan_out[0] = P.slab; plan_out[1] = P.n_slabs; plan_out[2] = P.rows_per_chunk; plan_out[3] = P.n_chunks;
    plan_out[4] = P.workspace_bytes; plan_out[5] = P.min_budget_bytes;
    return ok ? 0 : 1;
}

int blhip_posterior_predictive(blhip_ctx *ctx, int source, int64_t chain, int64_t t0, int64_t t1, int average, const blhip_problem *model,
                               const double *x, int64_t n_x, const double *x_step, const double *host_rows, double *host_out) {
    return guarded(ctx, [&] {
        if (!model) fail("blhip_posterior_predictive: model is NULL");
        if (!host_out) fail("blhip_posterior_predictive: host_out is NULL");
        if (n_x < 1 || n_x > (1ll << 31)) fail("blhip_posterior_predictive: n_x = %lld", (long long)n_x);
        if (!host_rows && !x) fail("blhip_posterior_predictive: x is NULL");
        HIPCHECK(hipSetDevice(ctx->device));
        const SeqView v = sequence_view(ctx, source, chain);
        if (t0 < 0 || t1 > v.T || t0 >= t1 || t1 - t0 >= (1ll << 31)) fail("blhip_posterior_predictive: bad range [%lld, %lld) of %lld steps", (long long)t0, (long long)t1, (long long)v.T);
        const long long G = (long long)v.n0 * v.n1;
        const int ndim = model->ndim, om = model->obs_model;
        if (ndim < 1 || ndim > BLHIP_MAX_DIM) fail("blhip_posterior_predictive: ndim = %d", ndim);
        long long Gm = 1;
        for (int k = 0; k < ndim; ++k) {
            if (model->n[k] < 1 || model->n[k] > (1ll << 30)) fail("blhip_posterior_predictive: bad grid axis %d", k);
            Gm *= model->n[k];
        }
        if (Gm != G) fail("blhip_posterior_predictive: the grid of the model (%lld cells) does not match the sequence (%lld cells)", Gm, G);
        // ---- where the likelihood rows come from
        enum { ROWS_HOST, ROWS_FORMULA, ROWS_TABLE, ROWS_PROGRAM } how = ROWS_HOST;
        if (!host_rows) {
            if (om == BLHIP_OM_GAUSSIAN || om == BLHIP_OM_POISSON) how = ROWS_FORMULA;
            else if (om == BLHIP_OM_BERNOULLI || om == BLHIP_OM_LAPLACE || om == BLHIP_OM_WHITE_NOISE) how = ROWS_TABLE;
            else if (om == BLHIP_OM_PROGRAM) how = ROWS_PROGRAM;
            else fail("blhip_posterior_predictive: observation model %d has no likelihood rows on the device: host_rows is required", om);
            const int want_dim = (om == BLHIP_OM_GAUSSIAN || om == BLHIP_OM_LAPLACE) ? 2 : 1;
            if (how != ROWS_PROGRAM && ndim != want_dim) fail("blhip_posterior_predictive: observation model %d has %d parameter(s), the grid %d", om, want_dim, ndim);
            for (int k = 0; k < ndim; ++k)
                if (!model->marginal[k]) fail("blhip_posterior_predictive: marginal[%d] is NULL", k);
            for (int64_t j = 0; j < n_x; ++j)
                if (!std::isfinite(x[j])) fail("blhip_posterior_predictive: x[%lld] is not finite (host_rows takes such values)", (long long)j);
            if (om == BLHIP_OM_POISSON) {
                if (!x_step) fail("blhip_posterior_predictive: Poisson needs k! of every value in x_step");
                for (int64_t j = 0; j < n_x; ++j)
                    if (x[j] < 0.0 || x[j] != std::floor(x[j]) || !std::isfinite(x_step[j]) || !(x_step[j] >= 1.0))
                        fail("blhip_posterior_predictive: Poisson value x[%lld] = %g is outside the direct formula (host_rows takes it)", (long long)j, x[j]);
            }
            if (how == ROWS_PROGRAM && ctx->likprog.armed && ctx->likprog.n_step > 0 && !x_step) fail("blhip_posterior_predictive: the armed program has STEP values, x_step is NULL");
        }
        // ---- the plan: what of the budget the rows of a chunk and the partial results take
        const int64_t Tr = t1 - t0, Tn = average ? 1 : Tr;
        size_t free_b = 0, total_b = 0;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        const double budget = std::min((double)free_b + (double)ctx->predws.cap, ctx->option("mem_budget_bytes", 0.70 * (double)total_b)) * 0.9;
        blpp::PredPlan PL;
        if (!blpp::predictive_plan(G, Tn, n_x, average != 0, budget, PL))
            fail("blhip_posterior_predictive: a workspace budget of %.0f bytes is below the %lld bytes the smallest plan needs", budget, PL.min_budget_bytes);
        ctx->predws.ensure((size_t)PL.workspace_bytes);
        char *ws = ctx->predws.as<char>();
        double *d_out = reinterpret_cast<double *>(ws + PL.off_out), *d_avg = reinterpret_cast<double *>(ws + PL.off_avg);
        double *d_rows = reinterpret_cast<double *>(ws + PL.off_rows), *d_part = reinterpret_cast<double *>(ws + PL.off_part);
        hipStream_t st = ctx->stream;
        // ---- x, k!, the marginal grids
        double *d_x = nullptr, *d_kf = nullptr;
        const double *dm[BLHIP_MAX_DIM] = {nullptr, nullptr, nullptr, nullptr};
        if (how != ROWS_HOST) {
            size_t xb = 2 * carve_size((size_t)n_x * 8);
            for (int k = 0; k < ndim; ++k) xb += carve_size(8 * (size_t)model->n[k]);
            ctx->predx.ensure(xb);
            char *cur = ctx->predx.as<char>();
            d_x = carve<double>(cur, (size_t)n_x);
            d_kf = carve<double>(cur, (size_t)n_x);
            HIPCHECK(hipMemcpyAsync(d_x, x, (size_t)n_x * 8, hipMemcpyHostToDevice, st));
            if (om == BLHIP_OM_POISSON) HIPCHECK(hipMemcpyAsync(d_kf, x_step, (size_t)n_x * 8, hipMemcpyHostToDevice, st));
            for (int k = 0; k < ndim; ++k) {
                double *d = carve<double>(cur, (size_t)model->n[k]);
                HIPCHECK(hipMemcpyAsync(d, model->marginal[k], 8 * (size_t)model->n[k], hipMemcpyHostToDevice, st));
                dm[k] = d;
            }
        }
        // ---- the left operand
        const double *d_post = v.p + (size_t)t0 * G;
        if (average) {
            BL_LAUNCH(blpp::average_rows_kernel, dim3((unsigned)std::min<long long>((G + 255) / 256, 4096)), dim3(256), 0, st, d_post, d_avg, G, (int)Tr);
            d_post = d_avg;
        }
        const long long ttiles = (Tn + blpp::TM - 1) / blpp::TM;
        const int n1 = (int)model->n[ndim - 1];
        const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 2048);
        for (int64_t c0 = 0; c0 < n_x; c0 += PL.rows_per_chunk) {
            const int xc = (int)std::min<int64_t>(PL.rows_per_chunk, n_x - c0);
            if (how == ROWS_HOST) {
                HIPCHECK(hipMemcpyAsync(d_rows, host_rows + (size_t)c0 * G, (size_t)xc * G * 8, hipMemcpyHostToDevice, st));
            } else if (how == ROWS_FORMULA) {
                BL_LAUNCH(blpp::tabulate_rows_kernel, dim3(gx, (unsigned)xc), dim3(256), 0, st, om, d_rows, G, n1, dm[0], dm[ndim - 1], d_x + c0, d_kf + c0);
            } else if (how == ROWS_TABLE) {
                BL_LAUNCH(lik_table_kernel, dim3(gx, (unsigned)xc), dim3(NTHREADS), 0, st, om, d_rows, G, n1, ndim, dm[0],
                          dm[ndim - 1], d_x + c0, 1, 1);
            } else {
                build_program_table(ctx, ndim, model->n, dm, xc, 1, x + c0, d_rows, x_step ? x_step + (size_t)c0 * ctx->likprog.n_step : nullptr);
            }
            blpp::ContractParams Q{};
            Q.post = d_post; Q.rows = d_rows; Q.part = d_part; Q.G = G; Q.slab = PL.slab; Q.T = (int)Tn; Q.xc = xc;
            Q.wide = (G % 2 == 0 && ((uintptr_t)d_post & 15) == 0 && ((uintptr_t)d_rows & 15) == 0) ? 1 : 0;
            for_grid_y(ctx, ttiles, [&](long long y0, unsigned ny) {
                Q.tile0 = y0;
                BL_LAUNCH(blpp::contract_kernel, dim3((unsigned)PL.n_slabs, ny), dim3(64), 0, st, Q);
            });
            BL_LAUNCH(blpp::combine_kernel, dim3((unsigned)(((long long)Tn * xc + 255) / 256)), dim3(256), 0, st, d_part, d_out, (int)PL.n_slabs, (long long)Tn, xc,
                      (long long)n_x, (long long)c0);
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(host_out, d_out, (size_t)Tn * n_x * 8, hipMemcpyDeviceToHost, st));
        sync_stream(ctx, st);
    });
}

int blhip_host_query_check(const blhip_query *query, int64_t n_steps, char *err, int errlen) { return blq::check_query(query, n_steps, err, errlen); }

int blhip_host_query_plan(int64_t G, int64_t n_steps, int64_t n_series, int64_t n_b, int b_const, int64_t fixed_bytes, double budget, int64_t *plan_out) {
    if (!plan_out) return -1;
    blq::QueryPlan P;
    const bool ok = blq::query_plan(G, n_steps, n_series, n_b, b_const != 0, fixed_bytes, budget, P);
    if (!ok && P.min_budget_bytes == 0) return -1;
    plan_out[0] = P.slab; plan_out[1] = P.n_slabs; plan_out[2] = P.steps_per_chunk; plan_out[3] = P.n_chunks;
    plan_out[4] = P.workspace_bytes; plan_out[5] = P.min_budget_bytes;
    return ok ? 0 : 1;
}

int blhip_posterior_query(blhip_ctx *ctx, int source, int64_t chain, const int64_t *steps, int64_t n_steps, const blhip_query *query, double *host_out) {
    return guarded(ctx, [&] {
        // ---- everything that can be refused is refused before the first launch
        if (!host_out) fail("blhip_posterior_query: host_out is NULL");
        if (!steps) fail("blhip_posterior_query: steps is NULL");
        char msg[256] = "";
        if (blq::check_query(query, n_steps, msg, (int)sizeof msg) != 0) fail("blhip_posterior_query: %s", msg);
        const blhip_query &q = *query;
        HIPCHECK(hipSetDevice(ctx->device));
        const SeqView v = sequence_view(ctx, source, chain);
        for (int64_t s = 0; s < n_steps; ++s)
            if (steps[s] < 0 || steps[s] >= v.T) fail("blhip_posterior_query: steps[%lld] = %lld is outside the %lld rows of the sequence", (long long)s, (long long)steps[s], (long long)v.T);
        const long long G = (long long)v.n0 * v.n1;
        long long Gq = 1;
        for (int k = 0; k < q.ndim; ++k) Gq *= q.n[k];
        if (Gq != G) fail("blhip_posterior_query: the grid of the query (%lld cells) does not match the sequence (%lld cells)", Gq, G);
        const bool pairs = q.n_b > 0, b_const = q.b_const != 0, with_series = q.n_series > 0;
        // ---- the plan: what does not depend on the step, then the steps of a chunk
        const size_t nc = (size_t)std::max(1, q.n_consts), nbv = pairs ? std::max<size_t>(1, (size_t)q.n_bcols * q.n_b) : 1;
        size_t fixed = carve_size((size_t)q.n_ops * 8) + carve_size(nc * 8) + carve_size(nbv * 8) + carve_size((pairs && b_const ? (size_t)q.n_b : 1) * 8);
        for (int k = 0; k < q.ndim; ++k) fixed += carve_size(8 * (size_t)q.n[k]);
        size_t free_b = 0, total_b = 0;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        const double budget = std::min((double)free_b + (double)ctx->queryws.cap, ctx->option("mem_budget_bytes", 0.70 * (double)total_b)) * 0.9;
        blq::QueryPlan PL;
        if (!blq::query_plan(G, n_steps, q.n_series, pairs ? q.n_b : 0, b_const, (long long)fixed, budget, PL))
            fail("blhip_posterior_query: a workspace budget of %.0f bytes is below the %lld bytes the smallest plan needs", budget, PL.min_budget_bytes);
        if (PL.n_slabs > 0x7fffffffLL || (PL.steps_per_chunk + blq::SB - 1) / blq::SB > ctx->max_grid_y) fail("blhip_posterior_query: the plan's grid does not fit one launch");
        ctx->queryws.ensure((size_t)PL.workspace_bytes);
        char *ws = ctx->queryws.as<char>(), *cur = ws;
        hipStream_t st = ctx->stream;
        blq::QueryParams P{};
        {
            bllp::Instr *d_ops = carve<bllp::Instr>(cur, (size_t)q.n_ops);
            double *d_consts = carve<double>(cur, nc), *d_bval = carve<double>(cur, nbv), *d_bconst = carve<double>(cur, pairs && b_const ? (size_t)q.n_b : 1);
            HIPCHECK(hipMemcpyAsync(d_ops, q.ops, (size_t)q.n_ops * 8, hipMemcpyHostToDevice, st));
            if (q.n_consts > 0) HIPCHECK(hipMemcpyAsync(d_consts, q.consts, (size_t)q.n_consts * 8, hipMemcpyHostToDevice, st));
            if (pairs && q.n_bcols > 0) HIPCHECK(hipMemcpyAsync(d_bval, q.b_values, (size_t)q.n_bcols * q.n_b * 8, hipMemcpyHostToDevice, st));
            if (pairs && b_const) HIPCHECK(hipMemcpyAsync(d_bconst, q.b_prob, (size_t)q.n_b * 8, hipMemcpyHostToDevice, st));
            for (int k = 0; k < q.ndim; ++k) {
                double *d = carve<double>(cur, (size_t)q.n[k]);
                HIPCHECK(hipMemcpyAsync(d, q.marginal[k], 8 * (size_t)q.n[k], hipMemcpyHostToDevice, st));
                P.m[k] = d;
                P.n[k] = (int)q.n[k];
            }
            P.ops = d_ops; P.consts = d_consts; P.bval = d_bval; P.bprob = d_bconst;
        }
        if ((size_t)(cur - ws) != fixed) fail("blhip_posterior_query: internal: the fixed uploads take %lld bytes, planned %lld", (long long)(cur - ws), (long long)fixed);
        long long *d_steps = reinterpret_cast<long long *>(ws + PL.off_steps);
        double *d_series = reinterpret_cast<double *>(ws + PL.off_series), *d_bprob = reinterpret_cast<double *>(ws + PL.off_bprob);
        double *d_part = reinterpret_cast<double *>(ws + PL.off_part), *d_out = reinterpret_cast<double *>(ws + PL.off_out);
        P.series = d_series; P.steps = d_steps; P.post = v.p; P.part = d_part;
        P.G = G; P.slab = PL.slab; P.nb = pairs ? q.n_b : 0;
        P.n_ops = q.n_ops; P.n_series = q.n_series; P.ndim = q.ndim; P.rel = q.relation; P.b_const = b_const ? 1 : 0;
        if (pairs && !b_const) P.bprob = d_bprob;
        static_assert(sizeof(long long) == sizeof(int64_t), "steps are uploaded as they come");
        for (int64_t c0 = 0; c0 < n_steps; c0 += PL.steps_per_chunk) {
            const int S = (int)std::min<int64_t>(PL.steps_per_chunk, n_steps - c0);
            HIPCHECK(hipMemcpyAsync(d_steps, steps + c0, (size_t)S * 8, hipMemcpyHostToDevice, st));
            if (with_series) HIPCHECK(hipMemcpyAsync(d_series, q.series + (size_t)c0 * q.n_series, (size_t)S * q.n_series * 8, hipMemcpyHostToDevice, st));
            if (pairs && !b_const) HIPCHECK(hipMemcpyAsync(d_bprob, q.b_prob + (size_t)c0 * q.n_b, (size_t)S * q.n_b * 8, hipMemcpyHostToDevice, st));
            P.S = S;
            const unsigned ny = (unsigned)((S + blq::SB - 1) / blq::SB);      // (the plan keeps a chunk's step blocks within one launch)
            const dim3 grid((unsigned)PL.n_slabs, ny);
            if (pairs) {
                if (with_series) BL_LAUNCH(blq::query_pairs_kernel<true>, grid, dim3(blq::NT), 0, st, P);
                else BL_LAUNCH(blq::query_pairs_kernel<false>, grid, dim3(blq::NT), 0, st, P);
            } else {
                if (with_series) BL_LAUNCH(blq::query_rows_kernel<true>, grid, dim3(blq::NT), 0, st, P);
                else BL_LAUNCH(blq::query_rows_kernel<false>, grid, dim3(blq::NT), 0, st, P);
            }
            BL_LAUNCH(blq::combine_kernel, dim3((unsigned)((S + blq::NT - 1) / blq::NT)), dim3(blq::NT), 0, st, d_part, d_out, (int)PL.n_slabs, S, pairs ? 1 : 0);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(host_out + c0, d_out, (size_t)S * 8, hipMemcpyDeviceToHost, st));
            sync_stream(ctx, st);       // (the chunk's uploads are overwritten by the next one)
        }
    });
}

int blhip_host_bins_check(const int32_t *bin, int64_t G, int64_t n_bins, char *err, int errlen) { return blb::check_bins(bin, G, n_bins, err, errlen); }

int blhip_host_bins_plan(const int32_t *bin, int64_t G, int64_t n_bins, int64_t n_steps, double budget, int64_t *plan_out) {
    if (!plan_out || G < 1 || G > 0x7fffffffLL || n_bins < 1 || n_bins > 0x7fffffffLL) return -1;
    const blb::Shape sh;
    blb::Order O;
    O.slab = sh.slab; O.n_slabs = (G + sh.slab - 1) / sh.slab; O.gw = sh.gw_max;
    if (bin && (blb::check_bins(bin, G, n_bins, nullptr, 0) != 0 || !blb::order(bin, G, n_bins, sh.slab, sh.gw_max, O))) return -1;
    blb::BinsPlan P;
    const bool ok = blb::bins_plan(n_bins, O.n_runs, O.table_bytes(), n_steps, sh.sb, budget, P);
    if (!ok && P.min_budget_bytes == 0) return -1;
    const int64_t v[12] = {O.slab, O.n_slabs, sh.sb, O.gw, O.n_runs, O.n_groups, O.table_bytes(), P.steps_per_chunk, P.n_chunks, P.workspace_bytes,
                           P.min_budget_bytes, O.lds_bytes(sh.sb)};
    for (int k = 0; k < 12; ++k) plan_out[k] = v[k];
    return ok ? 0 : 1;
}

int blhip_posterior_bins(blhip_ctx *ctx, int source, int64_t chain, const int64_t *steps, int64_t n_steps, const int32_t *bin, int64_t G, int64_t n_bins,
                         double *host_out) {
    return guarded(ctx, [&] {
        // ---- everything that can be refused is refused before the first launch
        if (!host_out) fail("blhip_posterior_bins: host_out is NULL");
        if (!steps) fail("blhip_posterior_bins: steps is NULL");
        if (n_steps < 1 || n_steps > (1ll << 31)) fail("blhip_posterior_bins: n_steps = %lld", (long long)n_steps);
        char msg[256] = "";
        if (blb::check_bins(bin, G, n_bins, msg, (int)sizeof msg) != 0) fail("blhip_posterior_bins: %s", msg);
        HIPCHECK(hipSetDevice(ctx->device));
        const SeqView v = sequence_view(ctx, source, chain);
        for (int64_t s = 0; s < n_steps; ++s)
            if (steps[s] < 0 || steps[s] >= v.T) fail("blhip_posterior_bins: steps[%lld] = %lld is outside the %lld rows of the sequence", (long long)s, (long long)steps[s], (long long)v.T);
        if ((long long)v.n0 * v.n1 != G) fail("blhip_posterior_bins: the map (%lld cells) does not match the sequence (%lld cells)", (long long)G, (long long)v.n0 * v.n1);
        // ---- the order of the map and the plan
        const blb::Shape sh = blb::shape(ctx->option("bins_slab", (double)blb::SLAB), ctx->option("bins_sb", blb::SB), ctx->option("bins_gw", blb::GW));
        blb::Order O;
        if (!blb::order(bin, G, n_bins, sh.slab, sh.gw_max, O)) fail("blhip_posterior_bins: the tables of this map do not fit 32-bit indices");
        size_t free_b = 0, total_b = 0;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        const double budget = std::min((double)free_b + (double)ctx->queryws.cap, ctx->option("mem_budget_bytes", 0.70 * (double)total_b)) * 0.9;
        blb::BinsPlan PL;
        if (!blb::bins_plan(n_bins, O.n_runs, O.table_bytes(), n_steps, sh.sb, budget, PL))
            fail("blhip_posterior_bins: a workspace budget of %.0f bytes is below the %lld bytes the smallest plan needs", budget, PL.min_budget_bytes);
        const long long lds = O.lds_bytes(sh.sb);
        if (O.n_slabs > 0x7fffffffLL || (PL.steps_per_chunk + sh.sb - 1) / sh.sb > ctx->max_grid_y || lds > blb::LDS_BYTES_MAX)
            fail("blhip_posterior_bins: the plan's grid does not fit one launch");
        ctx->queryws.ensure((size_t)PL.workspace_bytes);
        char *ws = ctx->queryws.as<char>(), *cur = ws;
        hipStream_t st = ctx->stream;
        long long *d_slabs = carve<long long>(cur, O.slabs.size());
        int *d_tab = carve<int>(cur, O.tab.size());
        if ((long long)(cur - ws) != O.table_bytes()) fail("blhip_posterior_bins: internal: the tables take %lld bytes, planned %lld", (long long)(cur - ws), O.table_bytes());
        HIPCHECK(hipMemcpyAsync(d_slabs, O.slabs.data(), O.slabs.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(d_tab, O.tab.data(), O.tab.size() * 4, hipMemcpyHostToDevice, st));
        long long *d_steps = reinterpret_cast<long long *>(ws + PL.off_steps);
        double *d_part = reinterpret_cast<double *>(ws + PL.off_part), *d_out = reinterpret_cast<double *>(ws + PL.off_out);
        blb::BinsParams P{};
        P.post = v.p; P.steps = d_steps; P.slabs = d_slabs;
        P.perm = d_tab + O.off_perm; P.gdst = d_tab + O.off_gdst; P.multi = d_tab + O.off_multi;
        P.part = d_part;
        P.G = G; P.slab = O.slab; P.R = O.n_runs; P.n_slabs = O.n_slabs;
        P.sb = sh.sb; P.gw = O.gw; P.slots = (int)O.max_slots;
        P.wide = (G % 2 == 0 && ((uintptr_t)v.p & 15) == 0) ? 1 : 0;
        if (lds > 64 * 1024) blerr::arm_kernel(reinterpret_cast<const void *>(blb::bins_kernel));
        static_assert(sizeof(long long) == sizeof(int64_t), "steps are uploaded as they come");
        for (int64_t c0 = 0; c0 < n_steps; c0 += PL.steps_per_chunk) {
            const long long S = std::min<int64_t>(PL.steps_per_chunk, n_steps - c0);
            HIPCHECK(hipMemcpyAsync(d_steps, steps + c0, (size_t)S * 8, hipMemcpyHostToDevice, st));
            P.S = (int)S;
            if (O.n_runs > 0)      // (a map that leaves every cell out has nothing to add: the combine kernel writes the zeros)
                BL_LAUNCH(blb::bins_kernel, dim3((unsigned)O.n_slabs, (unsigned)((S + sh.sb - 1) / sh.sb)), dim3(blb::NT), (size_t)lds, st, P);
            BL_LAUNCH(blb::bins_combine_kernel, dim3((unsigned)((S * n_bins + blb::NT - 1) / blb::NT)), dim3(blb::NT), 0, st, d_part, d_tab + O.off_binptr,
                      d_tab + O.off_binruns, d_out, O.n_runs, S, (long long)n_bins);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(host_out + (size_t)c0 * n_bins, d_out, (size_t)S * n_bins * 8, hipMemcpyDeviceToHost, st));
            sync_stream(ctx, st);       // (the chunk's steps are overwritten by the next one)
        }
    });
}

int blhip_carry_mix(blhip_ctx *ctx, int slot, int64_t n_chains, const double *weights, int accumulate) {
    return guarded(ctx, [&] {
        if (!weights) fail("weights is NULL");
        HIPCHECK(hipSetDevice(ctx->device));
        auto it = ctx->carry.find(slot);
        if (it == ctx->carry.end() || !it->second.valid) fail("blhip_carry_mix: carry slot %d holds no state", slot);
        blhip_ctx::Carry &cs = it->second;
        if (cs.chains != n_chains) fail("blhip_carry_mix: slot %d holds %lld chains, got %lld weights", slot, (long long)cs.chains, (long long)n_chains);
        if (accumulate && ctx->mix_G != cs.G) fail("blhip_carry_mix: accumulating %lld cells into a mix of %lld", (long long)cs.G, (long long)ctx->mix_G);
        hipStream_t st = ctx->stream;
        ctx->mix.ensure((size_t)cs.G * 8);
        ctx->mix_G = cs.G;
        ctx->small.ensure((size_t)n_chains * 8);
        HIPCHECK(hipMemcpyAsync(ctx->small.p, weights, (size_t)n_chains * 8, hipMemcpyHostToDevice, st));
        const unsigned gx = (unsigned)std::min<long long>((cs.G + NTHREADS - 1) / NTHREADS, 8192);
        BL_LAUNCH(carry_mix_kernel, dim3(gx), dim3(NTHREADS), 0, st, ctx->mix.as<double>(), cs.buf.as<double>(),
                           (long long)cs.G, (int)n_chains, ctx->small.as<double>(), accumulate ? 1 : 0);
        HIPCHECK(hipGetLastError());
        sync_stream(ctx, st);
    });
}

int blhip_carry_read(blhip_ctx *ctx, int slot, int64_t chain, double *host_out) {
    return guarded(ctx, [&] {
        if (!host_out) fail("host_out is NULL");
        HIPCHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        if (chain < 0) {
            if (ctx->mix_G <= 0) fail("blhip_carry_read: no mix computed");
            HIPCHECK(hipMemcpyAsync(host_out, ctx->mix.p, (size_t)ctx->mix_G * 8, hipMemcpyDeviceToHost, st));
        } else {
            auto it = ctx->carry.find(slot);
            if (it == ctx->carry.end() || !it->second.valid) fail("blhip_carry_read: carry slot %d holds no state", slot);
            if (chain >= it->second.chains) fail("blhip_carry_read: chain %lld of %lld", (long long)chain, (long long)it->second.chains);
            HIPCHECK(hipMemcpyAsync(host_out, it->second.buf.as<double>() + (size_t)chain * it->second.G, (size_t)it->second.G * 8,
                                    hipMemcpyDeviceToHost, st));
        }
        sync_stream(ctx, st);
    });
}

int blhip_carry_write(blhip_ctx *ctx, int slot, int64_t n_chains, int64_t G, const double *host_in) {
    return guarded(ctx, [&] {
        if (!host_in || n_chains < 1 || G < 1 || slot < 0) fail("blhip_carry_write: bad arguments");
        HIPCHECK(hipSetDevice(ctx->device));
        blhip_ctx::Carry &cs = ctx->carry[slot];
        cs.buf.ensure((size_t)n_chains * G * 8);
        HIPCHECK(hipMemcpyAsync(cs.buf.p, host_in, (size_t)n_chains * G * 8, hipMemcpyHostToDevice, ctx->stream));
        sync_stream(ctx, ctx->stream);
        cs.chains = n_chains; cs.G = G; cs.valid = true;
        cs.maxv.assign(n_chains, 0.0);           // (NotEqual inverts around the maximum of the carried state)
        for (int64_t b = 0; b < n_chains; ++b) {
            double m = -INFINITY;
            for (int64_t c = 0; c < G; ++c) m = std::max(m, host_in[b * G + c]);
            cs.maxv[b] = m;
        }
    });
}

int blhip_carry_release(blhip_ctx *ctx, int slot) {
    return guarded(ctx, [&] {
        HIPCHECK(hipSetDevice(ctx->device));
        if (slot < 0) {
            for (auto &kv : ctx->carry) kv.second.buf.release();
            ctx->carry.clear(); ctx->mix.release(); ctx->mix_G = 0;
        } else {
            auto it = ctx->carry.find(slot);
            if (it != ctx->carry.end()) { it->second.buf.release(); ctx->carry.erase(it); }
        }
    });
}

int blhip_accum_begin(blhip_ctx *ctx, int64_t T, int64_t G, void *external_devptr) {
    return guarded(ctx, [&] {
        if (T < 1 || G < 1) fail("blhip_accum_begin: bad shape");
        HIPCHECK(hipSetDevice(ctx->device));
        if (external_devptr) {
            ctx->acc = reinterpret_cast<double *>(external_devptr);
        } else {
            ctx->accum_own.ensure((size_t)T * G * 8);
            ctx->acc = ctx->accum_own.as<double>();
        }
        ctx->acc_T = T; ctx->acc_G = G; ctx->acc_folded = 0;
        ctx->acc_logref = -std::numeric_limits<double>::infinity();
        ctx->acc_active = true; ctx->acc_final = false; ctx->acc_first = true;
    });
}

int blhip_accum_state(blhip_ctx *ctx, double *log_ref, void **devptr, int64_t *n_folded) {
    return guarded(ctx, [&] {
        if (!ctx->acc_active) fail("no active accumulator");
        if (log_ref) *log_ref = ctx->acc_logref;
        if (devptr) *devptr = ctx->acc;
        if (n_folded) *n_folded = ctx->acc_folded;
    });
}

int blhip_accum_rescale(blhip_ctx *ctx, double new_log_ref) {
    return guarded(ctx, [&] {
        if (!ctx->acc_active) fail("no active accumulator");
        HIPCHECK(hipSetDevice(ctx->device));
        const long long n = (long long)ctx->acc_T * ctx->acc_G;
        if (ctx->acc_first) {
            // nothing folded on this rank: contributes zeros
            BL_LAUNCH(fill_kernel, dim3(1024), dim3(256), 0, ctx->stream, ctx->acc, n, 0.0);
            ctx->acc_first = false;
        } else {
            if (new_log_ref < ctx->acc_logref) fail("blhip_accum_rescale: new reference below the current one");
            const double r = std::exp(ctx->acc_logref - new_log_ref);
            if (r != 1.0)
                BL_LAUNCH(scale_all_kernel, dim3(2048), dim3(NTHREADS), 0, ctx->stream, ctx->acc, n, r);
        }
        ctx->acc_logref = new_log_ref;
        sync_stream(ctx, ctx->stream);
    });
}

int blhip_accum_fold_host(blhip_ctx *ctx, const double *posterior, double log_weight) {
    return guarded(ctx, [&] {
        if (!ctx->acc_active) fail("blhip_accum_fold_host without blhip_accum_begin");
        if (ctx->acc_final) fail("blhip_accum_fold_host: the accumulator is finalised");
        if (!posterior) fail("posterior is NULL");
        if (!std::isfinite(log_weight)) return;                 // np.isfinite(logEvidence) guard, a zero hyper-prior (core.py:1358, :1364)
        HIPCHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const int64_t T = ctx->acc_T;
        const long long G = ctx->acc_G;
        ctx->post_valid = false;                                  // (the sequence buffer is the staging area)
        ctx->post.ensure((size_t)T * G * 8);
        for_pinned_pieces(const_cast<double *>(posterior), (size_t)T * G * 8, [&](char *src, size_t n) {
            HIPCHECK(hipMemcpyAsync(ctx->post.as<char>() + (src - (const char *)posterior), src, n, hipMemcpyHostToDevice, st));
        });
        BatchOutcome O;
        O.logE.assign(1, log_weight);
        O.abort_step.assign(1, -1);
        O.abort_phase.assign(1, 0);
        O.invN.assign((size_t)T, 1.0);                             // (rows arrive normalised)
        const double zero = 0.0;
        ctx->small.ensure(carve_size(8) + carve_size((size_t)T * 8));
        char *cur = ctx->small.as<char>();
        double *d_w = carve<double>(cur, 1), *d_invN = carve<double>(cur, (size_t)T);
        fold_accumulate(ctx, T, G, 1, O, &zero, ctx->post.as<double>(), d_w, d_invN);
    });
}

namespace {
// per-step sums [sum A, sum A grid_0, sum A grid_1] of the accumulator -> page-locked host memory (T, 3) (+ T spare doubles
// behind them); d_inv: T doubles of device scratch
struct RowStats { double *red, *d_inv; };      // red: (T, RS_W) page-locked, + T spare doubles behind it
constexpr int RS_W = 1 + bln::MAXD;
// (A: any (T, G) array on the device -- the accumulator, or plane 0 of the history of an online block)
RowStats seq_row_stats(blhip_ctx *ctx, const blhip_problem *p, const double *A, int64_t T, int64_t G) {
    if (!p) fail("problem is NULL");
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    bln::NdGrid ng{};
    ng.ndim = p->ndim;
    long long Gp = 1;
    for (int k = p->ndim - 1; k >= 0; --k) { ng.n[k] = (int)p->n[k]; ng.stride[k] = Gp; Gp *= p->n[k]; }
    ng.G = Gp;
    if (Gp != G) fail("sequence / grid mismatch: the problem's grid has %lld cells, the rows %lld", Gp, (long long)G);
    const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 256);
    size_t bytes = carve_size((size_t)T * RS_W * gx * 8) + carve_size((size_t)T * RS_W * 8) + carve_size((size_t)T * 8);
    for (int k = 0; k < p->ndim; ++k) bytes += carve_size(8 * (size_t)p->n[k]);
    ctx->stats.ensure(bytes);
    char *cur = ctx->stats.as<char>();
    double *d_part = carve<double>(cur, (size_t)T * RS_W * gx);
    double *d_red = carve<double>(cur, (size_t)T * RS_W);
    double *d_inv = carve<double>(cur, (size_t)T);
    for (int k = 0; k < p->ndim; ++k) {
        double *dm = carve<double>(cur, (size_t)p->n[k]);
        HIPCHECK(hipMemcpyAsync(dm, p->marginal[k], 8 * (size_t)p->n[k], hipMemcpyHostToDevice, st));
        ng.m[k] = dm;
    }
    for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
        BL_LAUNCH(bln::row_stats_kernel, dim3(gx, nt), dim3(NTHREADS), 0, st, A + (size_t)t0 * G, ng, d_part + (size_t)t0 * 5 * gx);
    });
    BL_LAUNCH(reduce_partials_kernel, dim3((unsigned)(T * RS_W)), dim3(NTHREADS), 0, st, d_part, d_red, (int)gx, 0);
    ctx->pinS.ensure((size_t)T * (RS_W + 1) * 8);
    double *red = ctx->pinS.as<double>();
    HIPCHECK(hipMemcpyAsync(red, d_red, (size_t)T * RS_W * 8, hipMemcpyDeviceToHost, st));
    sync_stream(ctx, st);
    return RowStats{red, d_inv};
}
RowStats accum_row_stats(blhip_ctx *ctx, const blhip_problem *p) {
    if (!ctx->acc_active) fail("no active accumulator");
    if (!p) fail("problem is NULL");
    const RowStats rs = seq_row_stats(ctx, p, ctx->acc, ctx->acc_T, ctx->acc_G);
    ctx->acc_n0 = p->ndim == 1 ? 1 : (int)p->n[0];
    ctx->acc_n1 = (int)(ctx->acc_G / ctx->acc_n0);
    return rs;
}

// The grouped fold of a series fit (blhip_set_series_groups + BLHIP_ACCUMULATE; HyperStudy.fitMany): the batch holds whole groups of H
// chains, group s is folded into its own average
//     A[s][t][cell] = sum_h w[s, h] max(post[s, h][t][cell] invN[s, h][t], 1e-300),   w = exp(logE + log hyper-prior - ref_s)
// (reference core.py:1358-1366 per series; ref_s: the maximum over the group's valid chains -- prepare_fold's rules: an aborted chain, a
// non-finite evidence or a -inf weight contributes nothing).  One launch (blk::series_group_fold_kernel); a group is complete within its
// batch, so there is no running reference and no rescale.  The averages are then row-normalised and their means formed as
// blhip_accum_finalize does (seq_row_stats over S_b T rows, core.py:1379-1382, :1416-1419), and they become the kept posterior:
// post_chains = S_b.  A group nobody contributed to is all NaN (0 / 0), as the reference leaves it.  The means of the averages go to
// res->posterior_mean[(c0 / H + s) * ndim * T ...]: series s of the call where chain s's would stand; the chains' own are not formed.
void series_group_fold(blhip_ctx *ctx, const blhip_problem *p, int64_t T, long long G, int64_t B, int64_t c0, const BatchOutcome &out,
                       const double *log_w_batch, const double *d_post, double *d_w, double *d_invN, blhip_result *res) {
    const int64_t H = ctx->series.H;
    if (H < 1 || c0 % H != 0 || B % H != 0) fail("series fit: the grouped fold needs whole groups of %lld chains in its batch (chains %lld .. %lld)", (long long)H, (long long)c0, (long long)(c0 + B));
    if (d_post != ctx->post.as<double>()) fail("internal: series fit: the grouped fold reads the batch's row-major sequences");
    const int64_t Sb = B / H;
    if (Sb > 65535) fail("internal: series fit: %lld groups in one batch", (long long)Sb);
    hipStream_t st = ctx->stream;
    ctx->pinA.ensure(((size_t)B + (size_t)T * B) * 8);
    double *h_w = ctx->pinA.as<double>(), *h_invN = h_w + B;
    for (int64_t s = 0; s < Sb; ++s) {
        double ref = -INFINITY;
        for (int64_t h = 0; h < H; ++h) {
            const int64_t b = s * H + h;
            const bool valid = out.abort_step[b] < 0 && std::isfinite(out.logE[b]) && std::isfinite(log_w_batch[b]);
            h_w[b] = valid ? out.logE[b] + log_w_batch[b] : -INFINITY;
            if (valid && h_w[b] > ref) ref = h_w[b];
        }
        for (int64_t h = 0; h < H; ++h) {
            const int64_t b = s * H + h;
            h_w[b] = (std::isfinite(h_w[b]) && std::isfinite(ref)) ? std::exp(h_w[b] - ref) : 0.0;
        }
    }
    std::memcpy(h_invN, out.invN.data(), (size_t)T * B * 8);
    HIPCHECK(hipMemcpyAsync(d_w, h_w, (size_t)B * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_invN, h_invN, (size_t)T * B * 8, hipMemcpyHostToDevice, st));
    ctx->postpad.ensure((size_t)Sb * T * G * 8);            // (free here: one-parameter grids have no padded geometry)
    double *A = ctx->postpad.as<double>();
    const bool v2 = (G & 1) == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)d_post & 15) == 0;
    const unsigned gx = (unsigned)((G + (v2 ? 127 : 63)) / (v2 ? 128 : 64));
    HIPCHECK(hipEventRecord(ctx->ev[4], st));
    for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
        const dim3 grid(gx, nt, (unsigned)Sb);
        if (v2) BL_LAUNCH(series_group_fold_kernel<true>, grid, dim3(NTHREADS), 0, st, A, d_post, (int)H, G, (int)T, d_w, d_invN, (int)t0);
        else BL_LAUNCH(series_group_fold_kernel<false>, grid, dim3(NTHREADS), 0, st, A, d_post, (int)H, G, (int)T, d_w, d_invN, (int)t0);
    });
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ctx->ev[5], st));
    ctx->timing.accumulate_launches += 1;
    // the averages' row sums and first moments: S_b T rows of G cells, as the accumulator's T
    const int64_t rows = Sb * T;
    const RowStats rs = seq_row_stats(ctx, p, A, rows, G);               // (waits for the stream)
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
    ctx->timing.accumulate_ms += ms;
    double *inv = rs.red + (size_t)rows * RS_W;
    for (int64_t r = 0; r < rows; ++r) {
        const double sum = rs.red[r * RS_W];
        inv[r] = 1.0 / sum;
        if (res && res->posterior_mean) {
            const int64_t s = c0 / H + r / T, t = r % T;
            for (int k = 0; k < p->ndim; ++k) res->posterior_mean[((size_t)s * p->ndim + k) * T + t] = rs.red[r * RS_W + 1 + k] / sum;
        }
    }
    // ... and they take the batch's place as the kept posterior, normalised by the launch every series fit's rows are
    HIPCHECK(hipMemcpyAsync(ctx->post.p, A, (size_t)rows * G * 8, hipMemcpyDeviceToDevice, st));
    ctx->postinv.ensure((size_t)rows * 8);
    HIPCHECK(hipMemcpyAsync(ctx->postinv.p, inv, (size_t)rows * 8, hipMemcpyHostToDevice, st));
    ctx->post_valid = true; ctx->post_scaled = false; ctx->post_chains = Sb; ctx->post_T = T; ctx->post_G = G;
    ctx->post_series = true;
    ctx->post_row0 = 0; ctx->post_row1 = T;
    ctx->post_n0 = 1; ctx->post_n1 = (int)G;
    ensure_post_scaled(ctx);
    sync_stream(ctx, st);
}
}  // namespace

int blhip_accum_row_stats(blhip_ctx *ctx, const blhip_problem *p, double *host_out) {
    return guarded(ctx, [&] {
        if (!host_out) fail("host_out is NULL");
        if (!ctx->acc_active) fail("no active accumulator");
        if (!p) fail("problem is NULL");
        const int64_t T = ctx->acc_T;
        const int w = 1 + p->ndim;
        if (ctx->acc_first) { std::fill(host_out, host_out + T * w, 0.0); return; }
        const double *red = accum_row_stats(ctx, p).red;
        for (int64_t t = 0; t < T; ++t)
            for (int k = 0; k < w; ++k) host_out[t * w + k] = red[t * RS_W + k];
    });
}

int blhip_accum_finalize(blhip_ctx *ctx, const blhip_problem *p, double *posterior_mean) {
    return guarded(ctx, [&] {
        if (!ctx->acc_active) fail("no active accumulator");
        if (ctx->acc_first) fail("blhip_accum_finalize: nothing was accumulated");
        const RowStats rs = accum_row_stats(ctx, p);
        double *red = rs.red, *d_inv = rs.d_inv;
        hipStream_t st = ctx->stream;
        const int64_t T = ctx->acc_T, G = ctx->acc_G;
        double *inv = red + (size_t)T * RS_W;
        for (int64_t t = 0; t < T; ++t) {
            inv[t] = 1.0 / red[t * RS_W];                                        // core.py:1379-1382
            if (posterior_mean)
                for (int k = 0; k < p->ndim; ++k) posterior_mean[k * T + t] = red[t * RS_W + 1 + k] / red[t * RS_W];   // :1416-1419
        }
        HIPCHECK(hipMemcpyAsync(d_inv, inv, T * 8, hipMemcpyHostToDevice, st));
        const unsigned gs = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 4096);
        for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
            BL_LAUNCH(scale_rows_kernel, dim3(gs, nt), dim3(NTHREADS), 0, st, ctx->acc + (size_t)t0 * G, (long long)G, d_inv + t0);
        });
        sync_stream(ctx, st);
        ctx->acc_final = true;
    });
}

int blhip_accum_read(blhip_ctx *ctx, int64_t t0, int64_t t1, double *host_out) {
    return guarded(ctx, [&] {
        if (!ctx->acc_active) fail("no active accumulator");
        if (t0 < 0 || t1 > ctx->acc_T || t0 > t1 || !host_out) fail("blhip_accum_read: bad range");
        HIPCHECK(hipSetDevice(ctx->device));
        const char *src = reinterpret_cast<const char *>(ctx->acc + (size_t)t0 * ctx->acc_G);
        for_pinned_pieces(host_out, (size_t)(t1 - t0) * ctx->acc_G * 8, [&](char *dst, size_t n) {
            HIPCHECK(hipMemcpyAsync(dst, src + (dst - (char *)host_out), n, hipMemcpyDeviceToHost, ctx->stream));
        });
        sync_stream(ctx, ctx->stream);
    });
}

int blhip_accum_end(blhip_ctx *ctx) {
    return guarded(ctx, [&] {
        ctx->acc_active = false;
        ctx->acc = nullptr;
    });
}

// ---- blocks of an online study (blhip_online.hpp) ---------------------------------------------------------------------------------
int blhip_host_online_block_plan(int ndim, const int64_t *n, int64_t chains, int64_t planes, int64_t N, double budget, int64_t *plan_out) {
    if (!plan_out) return -1;
    blo::BlockPlan P;
    const bool ok = blo::online_block_plan(ndim, n, chains, planes, N, budget, P);
    if (!ok && P.min_budget_bytes == 0) return -1;
    plan_out[0] = P.steps; plan_out[1] = P.n_chunks; plan_out[2] = P.chunk_bytes; plan_out[3] = P.min_budget_bytes;
    return ok ? 0 : 1;
}

int blhip_mem_budget(blhip_ctx *ctx, double *bytes_out) {
    return guarded(ctx, [&] {
        if (!bytes_out) fail("blhip_mem_budget: bytes_out is NULL");
        HIPCHECK(hipSetDevice(ctx->device));
        size_t free_b = 0, total_b = 0;
        HIPCHECK(hipMemGetInfo(&free_b, &total_b));
        // (as chains_per_batch: the context's reusable buffers count as available; the history planes are part of what a block plans)
        *bytes_out = std::min((double)free_b + (double)ctx->state.cap + (double)ctx->post.cap + (double)ctx->accpart.cap + (double)ctx->mixseq.cap,
                              ctx->option("mem_budget_bytes", 0.70 * (double)total_b)) * 0.9;
    });
}

int blhip_mix_sequence(blhip_ctx *ctx, int source, int64_t plane, int64_t n_planes, int64_t n_chains, int64_t T, const double *weights, int accumulate) {
    return guarded(ctx, [&] {
        if (!weights) fail("blhip_mix_sequence: weights is NULL");
        if (n_planes < 1 || plane < 0 || plane >= n_planes) fail("blhip_mix_sequence: plane %lld of %lld", (long long)plane, (long long)n_planes);
        HIPCHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const double *seq = nullptr;
        long long cs = 0;
        int64_t B = 0, Ts = 0, G = 0;
        if (source == 0) {
            if (!ctx->post_valid) fail("blhip_mix_sequence: no posterior kept (run blhip_fit with BLHIP_FORWARD_ONLY | BLHIP_KEEP_POSTERIOR)");
            ensure_post_scaled(ctx);             // (a fit normalises the rows it keeps before it returns: the lazy row scale is 1 here)
            B = ctx->post_chains; Ts = ctx->post_T; G = ctx->post_G;
            seq = ctx->post.as<double>(); cs = (long long)Ts * G;
        } else if (source == 1) {
            if (plane != 0 || n_planes < 2) fail("blhip_mix_sequence: the planes 1 .. n_planes - 1 are mixed into plane 0");
            if (ctx->mixseq_planes != n_planes || ctx->mixseq_T < 1) fail("blhip_mix_sequence: the history holds %lld planes, the call names %lld", (long long)ctx->mixseq_planes, (long long)n_planes);
            B = n_planes - 1; Ts = ctx->mixseq_T; G = ctx->mixseq_G;
            cs = (long long)Ts * G; seq = ctx->mixseq.as<double>() + cs;
        } else fail("blhip_mix_sequence: bad source %d", source);
        if (B != n_chains || Ts != T) fail("blhip_mix_sequence: the sequence has %lld chains x %lld steps, the weights %lld x %lld", (long long)B, (long long)Ts, (long long)n_chains, (long long)T);
        if (B >= (1ll << 31) || T >= (1ll << 31)) fail("blhip_mix_sequence: too many chains / steps");
        const bool same = ctx->mixseq_planes == n_planes && ctx->mixseq_T == T && ctx->mixseq_G == G && ctx->mixseq.p;
        if (!same) {
            // a new history: nothing of an old one can be accumulated onto or read as another plane
            if (accumulate || source == 1) fail("blhip_mix_sequence: no history of %lld planes x %lld steps x %lld cells to accumulate onto", (long long)n_planes, (long long)T, (long long)G);
            ctx->mixseq.ensure((size_t)n_planes * T * G * 8);
            ctx->mixseq_planes = n_planes; ctx->mixseq_T = T; ctx->mixseq_G = G;
        }
        ctx->mixw.ensure((size_t)T * B * 8);
        HIPCHECK(hipMemcpyAsync(ctx->mixw.p, weights, (size_t)T * B * 8, hipMemcpyHostToDevice, st));
        blo::MixParams Q{};
        Q.seq = seq; Q.chain_stride = cs; Q.H = ctx->mixseq.as<double>() + (size_t)plane * T * G; Q.w = ctx->mixw.as<double>();
        Q.G = G; Q.B = (int)B; Q.accumulate = accumulate ? 1 : 0;
        // 16-byte loads where every row base allows them: G even makes every row offset (b T + t) G even
        const bool wide = (G % 2 == 0) && ((uintptr_t)Q.seq & 15) == 0 && ((uintptr_t)Q.H & 15) == 0;
        const long long per_row = wide ? G / 2 : G;
        const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((per_row + NTHREADS - 1) / NTHREADS, 4096));
        for_grid_y(ctx, T, [&](long long y0, unsigned ny) {
            Q.t0 = y0;
            if (wide) BL_LAUNCH(blo::mix_sequence_kernel<true>, dim3(gx, ny), dim3(NTHREADS), 0, st, Q);
            else BL_LAUNCH(blo::mix_sequence_kernel<false>, dim3(gx, ny), dim3(NTHREADS), 0, st, Q);
        });
        HIPCHECK(hipGetLastError());
        sync_stream(ctx, st);                    // (the caller's weights go out of use)
    });
}

int blhip_mix_means(blhip_ctx *ctx, const blhip_problem *p, double *host_out) {
    return guarded(ctx, [&] {
        if (!host_out) fail("blhip_mix_means: host_out is NULL");
        if (!p) fail("blhip_mix_means: problem is NULL");
        if (ctx->mixseq_planes < 1 || !ctx->mixseq.p) fail("blhip_mix_means: no history (blhip_mix_sequence)");
        if (p->ndim < 1 || p->ndim > BLHIP_MAX_DIM) fail("blhip_mix_means: ndim = %d", p->ndim);
        for (int k = 0; k < p->ndim; ++k)
            if (!p->marginal[k] || p->n[k] < 1) fail("blhip_mix_means: bad grid axis %d", k);
        const int64_t T = ctx->mixseq_T;
        const double *red = seq_row_stats(ctx, p, ctx->mixseq.as<double>(), T, ctx->mixseq_G).red;
        for (int64_t t = 0; t < T; ++t)
            for (int k = 0; k < p->ndim; ++k) host_out[t * p->ndim + k] = red[t * RS_W + 1 + k];
    });
}

int blhip_mix_read(blhip_ctx *ctx, int64_t plane, int64_t t0, int64_t t1, double *host_out) {
    return guarded(ctx, [&] {
        if (ctx->mixseq_planes < 1 || !ctx->mixseq.p) fail("blhip_mix_read: no history (blhip_mix_sequence)");
        if (plane < 0 || plane >= ctx->mixseq_planes || t0 < 0 || t1 > ctx->mixseq_T || t0 > t1 || !host_out) fail("blhip_mix_read: bad range");
        HIPCHECK(hipSetDevice(ctx->device));
        const int64_t G = ctx->mixseq_G;
        const char *src = reinterpret_cast<const char *>(ctx->mixseq.as<double>() + ((size_t)plane * ctx->mixseq_T + t0) * G);
        for_pinned_pieces(host_out, (size_t)(t1 - t0) * G * 8, [&](char *dst, size_t n) {
            HIPCHECK(hipMemcpyAsync(dst, src + (dst - (char *)host_out), n, hipMemcpyDeviceToHost, ctx->stream));
        });
        sync_stream(ctx, ctx->stream);
    });
}

int blhip_carry_copy(blhip_ctx *ctx, int src_slot, int dst_slot) {
    return guarded(ctx, [&] {
        if (dst_slot < 0 || src_slot == dst_slot) fail("blhip_carry_copy: bad slots %d -> %d", src_slot, dst_slot);
        auto it = ctx->carry.find(src_slot);
        if (it == ctx->carry.end() || !it->second.valid) fail("blhip_carry_copy: carry slot %d holds no state", src_slot);
        HIPCHECK(hipSetDevice(ctx->device));
        blhip_ctx::Carry &dst = ctx->carry[dst_slot];          // (std::map: inserting leaves `it` valid)
        const blhip_ctx::Carry &src = it->second;
        const size_t bytes = (size_t)src.chains * src.G * 8;
        dst.buf.ensure(bytes);
        HIPCHECK(hipMemcpyAsync(dst.buf.p, src.buf.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        sync_stream(ctx, ctx->stream);
        dst.chains = src.chains; dst.G = src.G; dst.maxv = src.maxv; dst.valid = true;
    });
}

}  // extern "C"
