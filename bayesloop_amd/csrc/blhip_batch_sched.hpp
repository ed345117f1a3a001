// The host-only decisions of do_fit's batch loop (blhip.hip): which path an attempt of a batch runs on (BatchPath), what its passes do
// with their sums (PassPlan), what the tail of the batch does (keep_rows, carried_state_source, fold_action), which batch runs next and
// whether it folds (BatchSchedule), and when a context whose resident launch gave up tries the resident paths again (ResidentRetry).
// Plain values in, plain structs out: no HIP call, no blhip_ctx; tests/host/batch_sched_main.cpp builds a stand-alone program around
// this header (tests/test_batch_sched_host.py).
// Included INSIDE the anonymous namespace of blhip_host.hpp (blhip_ctx holds a ResidentRetry) and listed with the other host headers
// of blhip.hip; needs <algorithm>, <cstdint> and <vector> in front of it.
#pragma once

// ---- the path an attempt of a batch runs on ---------------------------------------------------------------------------------------------
// What RAN, not what was planned: a batch whose resident pass gave up or failed a check (resident_failed) repeats on the 1-D kernels or
// the launch-per-step kernels, whatever its ResidentRun / ChainRun say.
enum BatchPath { PATH_RESIDENT, PATH_CHAIN, PATH_ROW1D, PATH_STEP };

inline BatchPath batch_path(bool rr_on, bool cr_on, bool r1_on, bool resident_failed) {
    if (rr_on && !resident_failed) return PATH_RESIDENT;
    if (cr_on && !resident_failed) return PATH_CHAIN;
    return r1_on ? PATH_ROW1D : PATH_STEP;
}

// ---- the sums of an attempt's passes ----------------------------------------------------------------------------------------------------
struct PassPlan {
    int nblk = 1;                 // partial-sum slots per (step, sum) of the attempt
    // the launch-per-step backward pass of a batch of chains needs nothing of the forward pass's host bookkeeping: it is done while the
    // GPU runs that pass -- 11 ms of the published break-point study's fit, 23 batches of 1017 chains
    bool late_fb = false;
    // ... and nobody waits for its sums either: they travel to the host on the copy stream BESIDE the backward pass (10 MB per batch of
    // the break-point study, 2.4 of its 42 ms over PCIe with the chip idle)
    bool late_copy = false;
};

// r1_chain: the 1-D batch runs the chain kernel, not the K-steps-per-launch one; late_sums: the option of that name
inline PassPlan pass_plan(BatchPath path, int resident_nblk, int chain_strips, int tile_nblk, bool full, bool r1_chain, int64_t B,
                          bool copy_stream, bool late_sums) {
    PassPlan P;
    P.nblk = path == PATH_RESIDENT ? resident_nblk : (path == PATH_CHAIN ? chain_strips : tile_nblk);
    P.late_fb = full && (path == PATH_STEP || (path == PATH_ROW1D && r1_chain)) && B >= 64;
    P.late_copy = P.late_fb && copy_stream && late_sums;
    return P;
}

// ---- the tail of a batch ----------------------------------------------------------------------------------------------------------------
// rows [row0, row1) of a kept sequence that keep_posterior has to normalise: the resident kernel normalised in place (invN = 1 there)
// every row of a full fit, and all but the last `lag` rows of a forward pass
struct RowRange { int64_t row0, row1; };

inline RowRange keep_rows(BatchPath path, bool full, int64_t T, int lag) {
    RowRange r{0, T};
    if (path == PATH_RESIDENT) {
        if (full) r.row1 = 0;
        else r.row0 = std::max<int64_t>(0, T - lag);
    }
    return r;
}

// where store_carry finds each chain's final state: the last row of the batch's sequence, or (evidence-only: nothing is stored) the
// state buffer the last launch wrote -- the 1-D kernels alternate per launch of usedK steps, the others per step
struct CarriedStateSource {
    int state = -1;               // 0 / 1: BatchEnv::d_pp[state]; -1: the sequence
    int64_t offset = 0;           // cells from the start of that buffer
    int64_t stride = 0;           // cells from one chain's state to the next one's
};

inline CarriedStateSource carried_state_source(bool evidence_only, bool r1_on, int64_t T, int64_t usedK, long long G) {
    CarriedStateSource s;
    if (!evidence_only) { s.offset = (T - 1) * G; s.stride = T * G; }
    else { s.state = (int)((r1_on ? (T - 1) / usedK : T - 1) & 1); s.stride = G; }
    return s;
}

enum FoldAction {
    FOLD_NOT_ASKED,               // the fit does not accumulate
    FOLD_SKIPPED,                 // the backward kernel folded this batch, or it was folded before (a repeat after poisoned carried slots)
    FOLD_AND_WAIT,
    FOLD_UNWAITED,                // many small batches: nobody waits for a batch's fold; the last one is waited for with the stream
};

inline FoldAction fold_action(bool accumulate, bool fold_done, bool folded_before, int64_t nbatch, bool keep, bool carry) {
    if (!accumulate) return FOLD_NOT_ASKED;
    if (fold_done || folded_before) return FOLD_SKIPPED;
    return (nbatch >= 4 && !keep && !carry) ? FOLD_UNWAITED : FOLD_AND_WAIT;
}

// ---- which batch runs next, and whether it folds ----------------------------------------------------------------------------------------
// A batch whose passes fail is repeated: in place on the launch-per-step kernels (a resident pass gave up or failed a check), in place
// with K = 1 (the raw sums of the K-steps-per-launch 1-D kernel failed), or -- its failed backward pass has added to partial accumulators
// that carry EARLIER batches of the call -- together with those batches: the slots are dropped and the call goes back to the first batch
// they carried, with the chain-resident path off up to the failed batch.
enum BatchAction { BATCH_FINISH, BATCH_REPEAT_ON_STEP_KERNELS, BATCH_REPEAT_K1, BATCH_REWIND, BATCH_INTERNAL_ERROR };
struct BatchStep { BatchAction action; int64_t from; };      // from: BATCH_REWIND, the batch the call goes back to

// what the passes of an attempt left behind
struct PassFacts {
    bool ok = true;               // run_passes' answer
    bool resident_failed = false;
    bool cr_on = false;           // the batch was set up on the chain-resident path ...
    bool touched_parts = false;   // ... its backward pass has written the carried slots ...
    bool part_fresh0 = true;      // ... which it had started itself (false: they carry earlier batches)
    bool part_live = false;       // blhip_ctx::PartState: the slots hold contributions that are not in the accumulator yet ...
    int64_t part_first_batch = 0; // ... of the batches from this one on
};

class BatchSchedule {
public:
    explicit BatchSchedule(int64_t nbatch) : nbatch_(nbatch), in_slots_((size_t)std::max<int64_t>(nbatch, 0), 0) {}

    bool more() const { return next_ < nbatch_; }
    int64_t batch() const { return next_; }
    // false: a batch of a range that is repeated after poisoned carried slots
    bool allow_chainres(int64_t bi) const { return bi > fallback_until_; }

    BatchStep after_passes(int64_t bi, const PassFacts &f) {
        // (the K = 1 repeat's own answer was never looked at: run_passes(K = 1) says true unless a 1-D resident launch gave up)
        if (f.ok || attempt_ == AFTER_K1) return {BATCH_FINISH, bi};
        if (attempt_ == ON_STEP_KERNELS) return {BATCH_INTERNAL_ERROR, bi};
        if (!f.resident_failed) { attempt_ = AFTER_K1; return {BATCH_REPEAT_K1, bi}; }
        if (f.cr_on && f.touched_parts && !f.part_fresh0) {
            // Batches of the range that were folded directly into the accumulator (not chain-resident, or repeated in place) are in the
            // average posterior already: their repeat skips the fold (finished)
            const int64_t from = f.part_live ? f.part_first_batch : bi;
            refold_before_ = fallback_until_ = bi;
            next_ = from;
            return {BATCH_REWIND, from};
        }
        attempt_ = ON_STEP_KERNELS;
        return {BATCH_REPEAT_ON_STEP_KERNELS, bi};
    }

    // The batch goes on to its tail.  went_into_slots: its contribution went into the carried partial accumulators (a fused fold with a
    // finite reference), not into the accumulator itself.  -> the fold is skipped: a repeat of a batch that is in the accumulator already
    bool finished(int64_t bi, bool went_into_slots) {
        const bool refold_skip = bi < refold_before_ && !in_slots_[(size_t)bi];
        in_slots_[(size_t)bi] = went_into_slots ? 1 : 0;
        next_ = bi + 1;
        attempt_ = FIRST;
        return refold_skip;
    }

private:
    enum Attempt { FIRST, ON_STEP_KERNELS, AFTER_K1 };
    int64_t nbatch_, next_ = 0;
    Attempt attempt_ = FIRST;
    int64_t fallback_until_ = -1;     // batches up to this one repeat on the launch-per-step kernels
    int64_t refold_before_ = -1;      // batches below this one that a repeat re-runs are folded again only if in_slots_
    std::vector<char> in_slots_;      // per batch of the call: see finished
};

// ---- when the resident paths are tried again --------------------------------------------------------------------------------------------
// A resident launch that gave up (its blocks were not all co-resident: another process held CUs), or a probe that found the chip busy,
// parks the resident paths of the context; they are tried again after `retry_after` further fits (one hiccup must not cost 1.4 - 2 x for
// the life of the process), and the wait doubles with every give-up in a row: 8, 16, ... 1024.
struct ResidentRetry {
    bool ok = true;
    int retry_after = 8, fits_since = 0;
    long long giveups = 0;

    // -> re-armed now (the caller asks the chip first: probe_residency)
    bool fit_begins() {
        if (ok || ++fits_since < retry_after) return false;
        ok = true;
        fits_since = 0;
        return true;
    }
    void gave_up() {
        ok = false;
        fits_since = 0;
        giveups += 1;
        if (giveups > 1) retry_after = std::min(1024, 2 * retry_after);
    }
    // a resident pass went through: the next give-up starts from the short wait again (the wait doubles with give-ups IN A ROW only)
    void passed() { retry_after = 8; giveups = 0; }
    // option resident_ok
    void set_ok(bool v) {
        ok = v;
        fits_since = 0;
        if (v) passed();
    }
};
