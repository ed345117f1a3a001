// Host-side infrastructure of libblhip: error handling, device / page-locked buffers, the context object.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <limits>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/blhip.h"

#include "blhip_err.hpp"

namespace {

using blerr::Fail;
using blerr::fail;
using blerr::arm_kernel;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        release();
        HIPCHECK(hipMalloc(&p, bytes));
        cap = bytes;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// a DevBuf that is not a member of the context: released when the scope is left, also by an exception (HIPCHECK throws)
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};

// page-locked host staging: a hipMemcpyAsync to / from pageable memory is staged by the runtime behind blocking waits whose
// wake-up is quantised (10-ms steps seen on a 6 KB read-back: 20-27 ms per call instead of 0.5 ms)
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        release();
        HIPCHECK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        cap = bytes;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

thread_local std::string g_create_error;

#include "blhip_batch_sched.hpp"    // ResidentRetry (no HIP call)

}  // namespace

struct blhip_ctx {
    int device = 0;
    long long max_grid_y = 65535;        // hipDeviceProp_t::maxGridSize[1] of the device (blhip_create); see for_grid_y
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    // radius buckets of a batch are independent pipelines: one stream per bucket key, joined with events
    static constexpr int NBS = 18;       // (>= the keys of bucket_step)
    hipStream_t bstream[NBS] = {};
    hipEvent_t bev[NBS] = {};
    hipEvent_t fork_ev = nullptr, sync_ev = nullptr;
    std::string err;
    std::string name;
    std::map<std::string, double> opt;
    // reusable device buffers
    DevBuf state, post, psumF, psumB, redF, redB, meta, tables, likbuf, small, accum_own, stats;
    // kept posterior of the last fit
    bool post_valid = false;
    bool post_scaled = true;     // false: the kept rows still carry their raw sums; postinv holds 1 / sum per (chain, step)
    DevBuf postinv;
    int64_t post_chains = 0, post_T = 0, post_G = 0;
    bool post_series = false;    // kept by a series fit (blhip_set_series): the rows of all chains are normalised in one launch
    int64_t post_row0 = 0, post_row1 = 0;        // rows of the kept sequence that still carry their raw sums
    int post_n0 = 1, post_n1 = 1, acc_n0 = 1, acc_n1 = 1;
    // accumulator
    bool acc_active = false, acc_final = false, acc_first = true;
    double *acc = nullptr;
    int64_t acc_T = 0, acc_G = 0, acc_folded = 0;
    double acc_logref = -std::numeric_limits<double>::infinity();
    blhip_timing timing = {};
    // carried states of streaming fits (BLHIP_CARRY / BLHIP_RESUME): slot -> (chains, G) normalised distributions
    struct Carry { DevBuf buf; int64_t chains = 0, G = 0; bool valid = false; std::vector<double> maxv; };
    std::map<int, Carry> carry;
    DevBuf mix, unit, databuf;
    PinBuf pinA;                 // weights of the average-posterior folds
    PinBuf pinF, pinB, pinS;     // host staging of the reduced sums (forward, backward) and of small read-backs
    int64_t mix_G = 0;
    // blocks of an online study (blhip_online.hpp): history planes [plane][t][cell] -- plane 0 is the mixture over every chain of every
    // transition model, the others one model's mixture each -- and the device copy of a call's weights
    DevBuf mixseq, mixw;
    int64_t mixseq_T = 0, mixseq_G = 0, mixseq_planes = 0;
    // multi-GPU exchange (blhip_comm.hpp): RCCL communicator of this context's device, staging buffers
    void *comm = nullptr;        // ncclComm_t
    int comm_world = 1, comm_rank = 0;
    double comm_reduce_ms = 0.0;   // HIP-event time of the last blhip_comm_reduce_accum
    DevBuf commbuf;
    PinBuf pinC;
    // time-resident path (blhip_resident.hpp): halo strips / flags, and whether every tile was co-resident so far
    DevBuf resx;
    // a resident launch that gave up (its blocks were not all co-resident: another process held CUs) parks the resident paths; they
    // are tried again after `resident.retry_after` further fits, and the wait doubles with every give-up in a row (8, 16, ... 1024)
    ResidentRetry resident;
    int resident_last_reason = 0;                  // BLHIP_FALLBACK_* of the last resident batch that fell back
    int num_cus = 0;
    DevBuf accw;                 // device copies of the fused fold's per-chain scales and weights (ChainRun::fold_buffers)
    DevBuf postpad;              // padded strip-major sequence of a chain-resident batch whose posteriors are handed out (de-padded into post);
                                 // the grouped fold of a series fit (one-parameter grids, which never pad): its (series of the batch, T, n) averages before they become the kept posterior
    DevBuf hsrc;                 // the axis-1 pre-pass's output of one step (blhip_hwide.hpp)
    DevBuf stagebuf, stagemeta;  // composed transitions: two stage outputs (+ their partials) of a step, the stages' per-chain programs (blhip_batch.hpp)
    DevBuf p1d, p1w;             // hand-off buffers / weight table of the persistent 1-D kernel (blhip_persist1d.hpp)
    DevBuf lik1d;                // (T, n) likelihood table the chains of a 1-D batch share (blhip_chain1d.hpp); series fits: (B, T, n), one table per chain
    // Series fits (blhip_set_series): `armed` arms the next blhip_fit, which takes the arrays over (`data` != nullptr while that fit runs:
    // chain c observes series c) and disarms.  om: the caller's observation model (the fit itself may see BLHIP_OM_TABLE).  The records /
    // data and the row offsets of a batch go to `databuf`.
    // Groups (blhip_set_series_groups): H chains per series -- chain c observes series c / H; `grouped`: armed that way, the one arming
    // whose fit may carry BLHIP_ACCUMULATE (the grouped fold, blhip_series.hpp).  blhip_set_series is H = 1, not grouped.
    struct SeriesFit {
        const double *armed = nullptr; int64_t armed_S = 0, armed_H = 1; bool armed_grouped = false;
        const double *data = nullptr; int64_t S = 0, H = 1; bool grouped = false; int om = 0;
        bool fold = false;       // the running fit folds every group into its own average (series_group_fold)
    } series;
    // the likelihood program blhip_set_lik_program armed for the problems whose obs_model is BLHIP_OM_PROGRAM (blhip_likprog.hpp): host
    // copies of its arrays, and the device buffer a table build uploads them to
    struct LikProgram { std::vector<int32_t> ops; std::vector<double> consts, step; int64_t n_step = 0; bool armed = false; } likprog;
    DevBuf likprog_dev;
    DevBuf predws, predx;        // the posterior predictive (blhip_predictive.hpp): likelihood rows of a chunk of x + split-K partials + result; x, k!, grids
    DevBuf queryws;              // parser queries at many steps, every call uploads all it reads: probabilities (blhip_query.hpp): program, tables, B's columns, the steps of a
                                 // chunk + partials + result; distributions (blhip_bins.hpp): the order of the map, the steps of a chunk + partials + result
    DevBuf accpart;              // partial accumulators of the fused fold (one per launch slot of the chain-resident kernel)
    // The partial accumulators are CARRIED from batch to batch of one blhip_fit call (round 6): the batches' weights share the reference of
    // the first one, the slots go into the average posterior once, after the call's last batch (fold_parts_kernel read 8 + 2 sequences of
    // T x G cells per batch: 4 x 4 ms of BASELINE C5's 226).  A batch that fails its checks after its backward pass has written the slots
    // poisons them: the call repeats the batches since `first_batch` on the launch-per-step kernels (do_fit).
    struct PartState {
        bool live = false;                  // the slots hold contributions that are not in the accumulator yet
        double ref = -std::numeric_limits<double>::infinity();       // ... weighted relative to this log weight
        double maxlw = -std::numeric_limits<double>::infinity();     // largest log weight among them
        int slots_init = 0;                 // slots written so far (a batch that uses more zeroes the new ones)
        int nfold = 0;                      // chains they hold
        int64_t first_batch = 0;            // first batch of the call with contributions in them
        int n0 = 0, n1 = 0, T = 0, n0p = 0, ax1 = 0; long long Gk = 0;      // layout (fold_parts_kernel's arguments)
        int sw = 16;                        // ... columns per strip: 16, or 8 where the four-chain fold kernel wrote them
    } part;
    DevBuf anchbuf;              // the anchors of the likelihood recurrence of a chain-resident batch, tabulated once per batch (blc::anchor_table_kernel)
    DevBuf axlik;                // ... its likelihood table of the even time steps (transposed layout): ceil(T / 2) x n0p^2 doubles
    DevBuf xch;                  // exchange buffers of the both-axes chain-resident kernel (blhip_chainax.hpp): [slot][2 step parities][Gk]
    hipStream_t cstream = nullptr;      // copy stream: the forward pass's sums travel to the host beside the backward pass (do_fit: late_copy)
    hipEvent_t cev[2] = {nullptr, nullptr};
    // the co-residency probe (blr::residency_probe_kernel): when it last ran (steady-clock seconds, < 0: never / run it again), what it saw
    DevBuf probebuf;
    double probe_last = -1.0;
    bool xcd_order_ok = true;
    bool probe_announced = false;
    // the prior the tables buffer holds (blhip_problem.prior_token): uploaded again only when the caller's token, the grid or the place changes
    unsigned long long prior_token = 0;
    const double *prior_dev = nullptr;
    long long prior_G = 0;

    double option(const char *k, double dflt) const {
        auto it = opt.find(k);
        return it == opt.end() ? dflt : it->second;
    }
};

namespace {

// Wait for a stream by polling an event: hipStreamSynchronize blocks on an interrupt whose wake-up is quantised (~10 ms
// steps measured on long waits: 15-25 ms of wall time per fit on top of a 365 ms device timeline).
struct Trace {
    bool on; std::chrono::steady_clock::time_point t0;
    explicit Trace(bool o) : on(o), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[blhip trace] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// A launch whose gridDim.y counts time steps, rows of a sequence or chains x steps: the device takes at most max_grid_y (65 536 on gfx950)
// per launch, a long 1-D series or a kept batch of many chains has more -- launch(y0, ny) once per piece of at most that many.
template <class F>
void for_grid_y(const blhip_ctx *ctx, long long ny, F &&launch) {
    const long long lim = std::max<long long>(1, ctx->max_grid_y);
    for (long long y0 = 0; y0 < ny; y0 += lim) launch(y0, (unsigned)std::min<long long>(lim, ny - y0));
}

void sync_stream(blhip_ctx *ctx, hipStream_t st) {
    HIPCHECK(hipEventRecord(ctx->sync_ev, st));
    for (;;) {
        const hipError_t e = hipEventQuery(ctx->sync_ev);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) HIPCHECK(e);
        std::this_thread::yield();
    }
}

template <class T> T *carve(char *&cur, size_t count) {
    T *p = reinterpret_cast<T *>(cur);
    cur += ((count * sizeof(T) + 255) / 256) * 256;
    return p;
}
size_t carve_size(size_t bytes) { return ((bytes + 255) / 256) * 256; }

template <class F> int guarded(blhip_ctx *ctx, F &&f) {
    if (!ctx) return -1;
    try {
        f();
        return 0;
    } catch (const Fail &e) {
        ctx->err = e.msg;
    } catch (const std::exception &e) {
        ctx->err = e.what();
    } catch (...) {
        ctx->err = "unknown error";
    }
    return -1;
}

}  // namespace
