// Stand-alone host program around bayesloop_amd/csrc/blhip_batch_sched.hpp: the host-only decisions of do_fit's batch loop (blhip.hip).
// It launches nothing and runs on a CPU.
//     hipcc -std=c++17 --offload-arch=gfx950 tests/host/batch_sched_main.cpp -o batch_sched && ./batch_sched script=S,D,P
// Arguments, key=value, answered in their order:
//   script=L,L,..[/fresh]  one call of do_fit, a letter per batch for the outcome of its FIRST attempt where the chain-resident path is allowed:
//                            S  passes, the backward kernel folds it into the carried slots     D  passes, folded directly (not chain-resident)
//                            E  a resident check fails before the backward pass                 P  ... after the backward pass has written the slots
//                            K  the raw sums of the K-steps-per-launch 1-D pass fail            an X behind E / P: the repeat in place fails too
//                          A batch of a repeated range (chain-resident not allowed) and every repeat in place pass and fold directly.
//                          fresh: the batch whose fused fold flushes the carried slots first and starts them afresh (none: -1); a fused fold
//                          that finds no live slots starts them too.
//                          -> per attempt "attempt BATCH ALLOW_CHAINRES ACTION FROM REFOLD_SKIP" (FROM: of REWIND, REFOLD_SKIP: of FINISH, else -),
//                          then "ledger" with how often each batch reached the accumulator and "ok 0 / 1" (each exactly once)
//   exhaustive=N           every script of 1 .. N batches over S D E P, times every fresh batch: "exhaustive scripts bad longest" (longest: attempts)
//   ledger=op,op,..        the ledger alone, fed by hand: dB a direct fold of batch B, fB a fused fold, x the slots are dropped, + they are
//                          flushed; n=B batches -> the "ledger" line of it
//   path=rr_on,cr_on,r1_on,resident_failed                                         -> "path NAME"
//   pass=path,resident_nblk,chain_strips,tile_nblk,full,r1_chain,B,copy_stream,late_sums   -> "pass nblk late_fb late_copy"
//   keep=path,full,T,lag                                                           -> "keep row0 row1"
//   carry=evidence_only,r1_on,T,usedK,G                                            -> "carry state offset stride"
//   fold=accumulate,fold_done,folded_before,nbatch,keep,carry                      -> "fold NAME"
//   retry=op,op,..         a ResidentRetry: g gave_up, p passed, f fit_begins, s0 / s1 set_ok, rN retry_after = N (the option)
//                          -> per op "retry OP ok retry_after fits_since giveups rearmed" (rearmed: fit_begins' answer, else 0)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
#include "../../bayesloop_amd/csrc/blhip_batch_sched.hpp"

std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out(1);
    for (char c : s) { if (c == sep) out.emplace_back(); else out.back() += c; }
    return out;
}

std::vector<long long> numbers(const std::string &s) {
    std::vector<long long> v;
    for (const std::string &x : split(s, ',')) v.push_back(std::atoll(x.c_str()));
    return v;
}

const char *PATHS[] = {"RESIDENT", "CHAIN", "ROW1D", "STEP"};
const char *ACTIONS[] = {"FINISH", "REPEAT_ON_STEP_KERNELS", "REPEAT_K1", "REWIND", "INTERNAL_ERROR"};
const char *FOLDS[] = {"NOT_ASKED", "SKIPPED", "AND_WAIT", "UNWAITED"};

// what reaches the accumulator: a direct fold adds to it, a fused fold adds to the slots, a rewind drops the slots, a flush (a batch that
// starts them afresh, the end of the call) adds them to the accumulator
struct Ledger {
    std::vector<int> acc, slots;
    explicit Ledger(size_t n) : acc(n, 0), slots(n, 0) {}
    void direct(int64_t b) { acc[(size_t)b] += 1; }
    void fused(int64_t b) { slots[(size_t)b] += 1; }
    void drop() { std::fill(slots.begin(), slots.end(), 0); }
    void flush() { for (size_t b = 0; b < acc.size(); ++b) { acc[b] += slots[b]; slots[b] = 0; } }
    bool once() const { return std::all_of(acc.begin(), acc.end(), [](int k) { return k == 1; }); }
    void print() const {
        std::printf("ledger");
        for (int k : acc) std::printf(" %d", k);
        std::printf(" ok %d\n", once() ? 1 : 0);
    }
};

struct Batch { char first = 'D'; bool repeat_fails = false; };

// do_fit's loop around a BatchSchedule with the device taken out: the letters say what the passes answer, the ledger what was folded.
// -> attempts (-1: the script did not end within `limit`, -2: the schedule answered the internal error)
int run_script(const std::vector<Batch> &script, int64_t fresh, Ledger &led, bool print, int limit = 1000) {
    const int64_t n = (int64_t)script.size();
    BatchSchedule sched(n);
    bool live = false;                           // blhip_ctx::PartState
    int64_t first_batch = 0;
    int attempts = 0;
    auto line = [&](int64_t bi, bool allow, const BatchStep &s, int skip) {
        if (!print) return;
        std::printf("attempt %lld %d %s", (long long)bi, allow ? 1 : 0, ACTIONS[s.action]);
        if (s.action == BATCH_REWIND) std::printf(" %lld", (long long)s.from); else std::printf(" -");
        if (skip >= 0) std::printf(" %d\n", skip); else std::printf(" -\n");
    };
    while (sched.more()) {
        const int64_t bi = sched.batch();
        const bool allow = sched.allow_chainres(bi);
        const char what = allow ? script[(size_t)bi].first : 'D';
        PassFacts f;
        bool went_into_slots = false;
        if (what == 'S' || what == 'P') {        // the chain-resident backward pass with the fused fold (ChainRun::prepare_fold, ::fold)
            if (live && bi == fresh) { led.flush(); live = false; }
            f.cr_on = true; f.touched_parts = true; f.part_fresh0 = !live;
            f.ok = what == 'S';
            f.resident_failed = !f.ok;
        } else if (what == 'E') { f.cr_on = true; f.ok = false; f.resident_failed = true; }
        else if (what == 'K') { f.ok = false; }
        f.part_live = live; f.part_first_batch = first_batch;
        for (;;) {
            if (++attempts > limit) return -1;
            const BatchStep s = sched.after_passes(bi, f);
            if (s.action == BATCH_FINISH) {
                if (what == 'S' && f.ok && !f.resident_failed) {
                    went_into_slots = true;
                    if (!live) { live = true; first_batch = bi; }
                    led.fused(bi);
                }
                const bool skip = sched.finished(bi, went_into_slots);
                if (!went_into_slots && !skip) led.direct(bi);
                line(bi, allow, s, skip ? 1 : 0);
                break;
            }
            line(bi, allow, s, -1);
            if (s.action == BATCH_INTERNAL_ERROR) return -2;
            if (s.action == BATCH_REWIND) { led.drop(); live = false; break; }
            // a repeat in place: passes and folds directly -- unless the script says that the launch-per-step kernels fail too
            f.ok = !(s.action == BATCH_REPEAT_ON_STEP_KERNELS && script[(size_t)bi].repeat_fails);
        }
    }
    led.flush();
    return attempts;
}

std::vector<Batch> parse_script(const std::string &s) {
    std::vector<Batch> v;
    for (const std::string &w : split(s, ',')) {
        Batch b;
        if (w.empty() || !std::strchr("SDEPK", w[0])) { std::fprintf(stderr, "script: unknown outcome '%s'\n", w.c_str()); std::exit(2); }
        b.first = w[0];
        b.repeat_fails = w.size() > 1 && w[1] == 'X';
        v.push_back(b);
    }
    return v;
}

void exhaustive(int nmax) {
    const char letters[] = {'S', 'D', 'E', 'P'};
    long long scripts = 0, bad = 0;
    int longest = 0;
    for (int n = 1; n <= nmax; ++n) {
        long long combos = 1;
        for (int k = 0; k < n; ++k) combos *= 4;
        for (long long c = 0; c < combos; ++c)
            for (int64_t fresh = -1; fresh < n; ++fresh) {
                std::vector<Batch> script((size_t)n);
                std::string name;
                long long r = c;
                for (int k = 0; k < n; ++k) { script[(size_t)k].first = letters[r % 4]; name += letters[r % 4]; r /= 4; }
                Ledger led((size_t)n);
                const int attempts = run_script(script, fresh, led, false);
                ++scripts;
                longest = std::max(longest, attempts);
                if (attempts < 0 || !led.once()) {
                    ++bad;
                    std::printf("bad %s/%lld attempts %d ", name.c_str(), (long long)fresh, attempts);
                    led.print();
                }
            }
    }
    std::printf("exhaustive %lld %lld %d\n", scripts, bad, longest);
}

void retry(const std::string &ops) {
    ResidentRetry r;
    for (const std::string &op : split(ops, ',')) {
        bool rearmed = false;
        if (op == "g") r.gave_up();
        else if (op == "p") r.passed();
        else if (op == "f") rearmed = r.fit_begins();
        else if (op == "s0" || op == "s1") r.set_ok(op == "s1");
        else if (op.size() > 1 && op[0] == 'r') r.retry_after = std::max(1, std::atoi(op.c_str() + 1));
        else { std::fprintf(stderr, "retry: unknown op '%s'\n", op.c_str()); std::exit(2); }
        std::printf("retry %s %d %d %d %lld %d\n", op.c_str(), r.ok ? 1 : 0, r.retry_after, r.fits_since, r.giveups, rearmed ? 1 : 0);
    }
}

}  // namespace

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        const char *eq = std::strchr(argv[a], '=');
        if (!eq) { std::fprintf(stderr, "expected key=value, got '%s'\n", argv[a]); return 2; }
        const std::string key(argv[a], (size_t)(eq - argv[a])), val(eq + 1);
        if (key == "script") {
            const std::vector<std::string> parts = split(val, '/');
            const std::vector<Batch> script = parse_script(parts[0]);
            Ledger led(script.size());
            const int attempts = run_script(script, parts.size() > 1 ? std::atoll(parts[1].c_str()) : -1, led, true);
            if (attempts == -1) std::printf("endless\n");
            else if (attempts == -2) std::printf("internal error\n");
            else led.print();
        } else if (key == "exhaustive") {
            exhaustive(std::atoi(val.c_str()));
        } else if (key == "ledger") {
            const std::vector<std::string> ops = split(val, ',');
            size_t n = 0;
            for (const std::string &op : ops) if (op.compare(0, 2, "n=") == 0) n = (size_t)std::atoll(op.c_str() + 2);
            Ledger led(n);
            for (const std::string &op : ops) {
                const int64_t b = op.size() > 1 ? std::atoll(op.c_str() + 1) : 0;
                if ((op[0] == 'd' || op[0] == 'f') && (b < 0 || (size_t)b >= n)) { std::fprintf(stderr, "ledger: batch %lld of %zu\n", (long long)b, n); return 2; }
                if (op[0] == 'd') led.direct(b);
                else if (op[0] == 'f') led.fused(b);
                else if (op == "x") led.drop();
                else if (op == "+") led.flush();
            }
            led.print();
        } else if (key == "path") {
            const std::vector<long long> v = numbers(val);
            if (v.size() != 4) return 2;
            std::printf("path %s\n", PATHS[batch_path(v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0)]);
        } else if (key == "pass") {
            const std::vector<long long> v = numbers(val);
            if (v.size() != 9 || v[0] < 0 || v[0] > 3) return 2;
            const PassPlan P = pass_plan((BatchPath)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0, v[5] != 0, v[6], v[7] != 0, v[8] != 0);
            std::printf("pass %d %d %d\n", P.nblk, P.late_fb ? 1 : 0, P.late_copy ? 1 : 0);
        } else if (key == "keep") {
            const std::vector<long long> v = numbers(val);
            if (v.size() != 4 || v[0] < 0 || v[0] > 3) return 2;
            const RowRange r = keep_rows((BatchPath)v[0], v[1] != 0, v[2], (int)v[3]);
            std::printf("keep %lld %lld\n", (long long)r.row0, (long long)r.row1);
        } else if (key == "carry") {
            const std::vector<long long> v = numbers(val);
            if (v.size() != 5 || v[3] < 1) return 2;
            const CarriedStateSource s = carried_state_source(v[0] != 0, v[1] != 0, v[2], v[3], v[4]);
            std::printf("carry %d %lld %lld\n", s.state, (long long)s.offset, (long long)s.stride);
        } else if (key == "fold") {
            const std::vector<long long> v = numbers(val);
            if (v.size() != 6) return 2;
            std::printf("fold %s\n", FOLDS[fold_action(v[0] != 0, v[1] != 0, v[2] != 0, v[3], v[4] != 0, v[5] != 0)]);
        } else if (key == "retry") {
            retry(val);
        } else {
            std::fprintf(stderr, "unknown key '%s'\n", key.c_str());
            return 2;
        }
    }
    return 0;
}
