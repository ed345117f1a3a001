// The transition program of a batch on grids with 3 and 4 parameters: which source every (step, chain) consumes and which tap set every
// pass of every chain filters with, serial segments, change-points, Independent restarts, the renormalising stages (reference:
// transitionModels.py:300-312, :351-360, :462-471, :571-602, :768-813; core.py:411, :467, :2164-2165).  No HIP call: do_fit_nd
// (blhip_fit_nd.hpp) uploads and runs what this builds, tests/host/nd_program_main.cpp prints it on a CPU.
// Needs include/blhip.h, SrcKind (blhip_kernels.hpp), fail (blhip_err.hpp) and TapTable (blhip_taps.hpp) in front of it; in the library it
// is included by blhip.hip INSIDE its anonymous namespace.
#pragma once

// what the op list says once per call.  pass_ops: the ops that launch passes, in list order (transitionModels.py:645-649) -- the random
// walks (one filter pass each) and the renormalising stages of blhip_nd_stages.hpp (NotEqual: three passes, Deterministic: one)
struct NdFacts {
    std::vector<int> pass_ops;
    int npass = 0;
    bool time_dependent = false, has_stage = false, has_shift = false;
    long long n_sum = 0;                             // sum of the axis lengths (the chain-resident kernel keeps the grid values in LDS)
    std::vector<int> pass_kind;                      // per pass: 0 a walk, 1 NotEqual, 2 a Deterministic shift (bln::CHAIN_ND_WALK ..)
};

inline NdFacts nd_facts(const blhip_problem *p) {
    NdFacts F;
    for (int k = 0; k < p->n_ops; ++k) {
        const int kind = p->ops[k].kind;
        if (kind == BLHIP_OP_GRW || kind == BLHIP_OP_NOTEQUAL || kind == BLHIP_OP_DETERMINISTIC) {
            F.pass_ops.push_back(k);
            F.pass_kind.push_back(kind == BLHIP_OP_GRW ? 0 : (kind == BLHIP_OP_NOTEQUAL ? 1 : 2));
        }
        if (kind == BLHIP_OP_NOTEQUAL || kind == BLHIP_OP_DETERMINISTIC) F.has_stage = true;
        if (kind == BLHIP_OP_DETERMINISTIC) F.has_shift = true;
        if (kind == BLHIP_OP_CHANGEPOINT || kind == BLHIP_OP_BREAKPOINT || kind == BLHIP_OP_DETERMINISTIC) F.time_dependent = true;
    }
    F.npass = (int)F.pass_ops.size();
    for (int k = 0; k < p->ndim; ++k) F.n_sum += p->n[k];
    return F;
}

// the time stamp the transition INTO step t is evaluated at; false: the step consumes a shared distribution, no transition
//   forward: T_fwd(post_{t-1}, ts[t-1]), core.py:411 (step 0 of a resumed fit: at resume_time, core.py:2164-2165)
//   backward: T_bwd(beta_{t+1} L_{t+1}, ts[t+1]) = T_fwd(., ts[t+1] - 1), core.py:467, transitionModels.py:316-317
inline bool nd_stamp(const blhip_problem *p, bool resume, int64_t t, bool fwd, double &tau) {
    if (fwd) {
        if (t == 0 && !resume) return false;
        tau = t == 0 ? p->resume_time : p->timestamps[t - 1];
    } else {
        if (t == p->T - 1) return false;
        tau = p->timestamps[t + 1] - 1.0;
    }
    return true;
}

// active sub-model of a serial model at tau: the number of boundary values at or before it (transitionModels.py:768)
inline int nd_segment_at(const blhip_problem *p, const double *val, double tau) {
    int seg = 0;
    for (int k = 0; k < p->n_ops; ++k) {
        const blhip_op &op = p->ops[k];
        if ((op.kind == BLHIP_OP_BREAKPOINT || (op.kind == BLHIP_OP_CHANGEPOINT && (op.flags & 1))) && val[k] <= tau) seg++;
    }
    return seg;
}

// a Deterministic model's shift of a step, in grid cells (its 2 T DETERMINISTIC_ARG ops: forward into step 0 .. T-1, backward into them)
inline double nd_shift_cells(const blhip_problem *p, const double *val, int k, int64_t t, bool fwd) {
    return val[k + 1 + (fwd ? t : p->T + t)] / p->lattice[p->ops[k].axis];
}

// Shifts beyond 12 cells per step leave what a shift-invariant stencil reproduces (SciPy's pre-padding, TapTable::get_shift); the
// two-stage kernel for them (blhip_bigshift.hpp) is 1-D / 2-D only.  Refused for every chain before anything is launched.
inline void nd_refuse_shifts(const blhip_problem *p, const NdFacts &F, int64_t n_chains, const double *op_values, bool resume) {
    if (!F.has_shift) return;
    for (int64_t c = 0; c < n_chains; ++c) {
        const double *val = op_values + c * p->n_ops;
        for (int64_t t = 0; t < p->T; ++t)
            for (int dir = 0; dir < 2; ++dir) {
                double tau = 0.0;
                if (!nd_stamp(p, resume, t, dir == 0, tau)) continue;
                const int seg = nd_segment_at(p, val, tau);
                for (int k : F.pass_ops) {
                    const blhip_op &op = p->ops[k];
                    if (op.kind != BLHIP_OP_DETERMINISTIC || (op.segment >= 0 && op.segment != seg)) continue;
                    const double dd = nd_shift_cells(p, val, k, t, dir == 0);
                    if (std::isnan(dd)) fail("chain %lld: Deterministic shift of step %lld is NaN", (long long)c, (long long)t);
                    if (std::fabs(dd) > 12.0)
                        fail("chain %lld, step %lld: Deterministic model shifts by %.3g grid cells in one time step; on grids with %d "
                             "parameters up to 12 (SciPy's pre-padding) are supported", (long long)c, (long long)t, dd, p->ndim);
                }
            }
    }
}

// the program of the chains [c0, c0 + B): source kind and the tap set of every pass, per step and direction
struct NdBatchProgram {
    TapTable taps;                                   // (taps.w ends in 8 zero doubles of padding)
    std::vector<unsigned char> kindF, kindB;         // [t][b] where a step's input comes from
    std::vector<int> tapF, tapB;                     // [pass][t][b] tap-set id (a NotEqual pass: 0 = on), -1: the pass leaves the chain alone
    // (with stages) stepK*: what the fused kernel is told -- SRC_PREV too when the chain ran a renormalising stage at the step, whose sums
    // it then reads its scale from; limit: [pass][b] NotEqual's 10**v dV
    std::vector<unsigned char> stepKF, stepKB;
    std::vector<double> limit;
    int lw_max = 0;                                  // widest radius of the table
    // inputs of the chain-resident kernel's cost model, of a program without stages only (there every pass is a walk and every id >= 0 a
    // tap set of the table -- NotEqual's passes carry a flag, not an id, and have no axis): the walks that have a kernel somewhere in the
    // batch, the taps of its slowest chain, a walk wider than its axis (the kernel's multi-period reflection)
    int walks_on = 0, W_taps = 0;
    bool beyond_axis = false;
    // what the stage flavour of the chain-resident kernel is handed, of every program: the widest radius among the walks' tap sets and
    // among the shifts' (a shift's slot holds 2 lw + 1 weights); and the inputs of ITS cost model, over the passes that are on somewhere
    // in the batch -- the launches the plain path spends per step (one per walk, three per NotEqual, one per shift, and the fused step
    // kernel), the taps of the slowest chain (2 x the widest radius + 1 per walk and per shift), the walks and shifts among them, the
    // sweeps over its cells the kernel adds (three per NotEqual, one per shift), the shifts among the filters, a walk wider than its axis
    int lw_walk_max = 0, lw_shift_max = 0;
    int stage_launches = 1, stage_W = 0, stage_filters = 0, stage_sweeps = 0, stage_shifts = 0;
    bool stage_beyond_axis = false;
};

// The transition of chain values `val` into a step, evaluated at time stamp tau (list order; only the ops of the active sub-model of a
// serial model act, transitionModels.py:768-776; a change point and an Independent model restart from a shared distribution and drop
// what the models before them did, :300-312, :351-360).  tp[q * stride]: the tap id of pass q.  -> true: the chain ran a renormalising stage
inline bool nd_transition(const blhip_problem *p, const NdFacts &F, const double *val, const std::vector<int> &op_tap, TapTable &taps, double tau,
                          int64_t t, bool fwd, unsigned char &kind, int *tp, size_t stride) {
    bool renorm = false;
    auto restart = [&](unsigned char from) {
        kind = from; renorm = false;
        for (int q = 0; q < F.npass; ++q) tp[q * stride] = -1;
    };
    restart(SRC_PREV);
    const int seg = F.time_dependent ? nd_segment_at(p, val, tau) : 0;
    for (int k = 0; k < p->n_ops; ++k) {
        const blhip_op &op = p->ops[k];
        if (op.segment >= 0 && op.segment != seg) continue;
        int q = 0;
        while (q < F.npass && F.pass_ops[q] != k) ++q;
        if (op.kind == BLHIP_OP_GRW) {
            tp[q * stride] = op_tap[k];
        } else if (op.kind == BLHIP_OP_CHANGEPOINT && !(op.flags & 1) && F.time_dependent && tau == val[k]) {
            restart(SRC_RESET);
        } else if (op.kind == BLHIP_OP_INDEPENDENT) {
            restart(SRC_INDEP);
        } else if (op.kind == BLHIP_OP_NOTEQUAL) {                                // transitionModels.py:462-471
            tp[q * stride] = 0;
            renorm = true;
        } else if (op.kind == BLHIP_OP_DETERMINISTIC) {                           // transitionModels.py:571-583, :585-602
            const double dd = nd_shift_cells(p, val, k, t, fwd);
            if (dd != 0.0) { tp[q * stride] = taps.get_shift(op.axis, dd); renorm = true; }      // (zero shift: the identity)
        }
    }
    if (F.time_dependent)
        for (int k = 0; k < p->n_ops; ++k) {                                      // serial change-points: after the sub-model acted, :801-813
            const blhip_op &op = p->ops[k];
            if (op.kind == BLHIP_OP_CHANGEPOINT && (op.flags & 1) && tau == val[k]) restart(SRC_RESET);
        }
    return renorm;
}

inline void build_nd_program(const blhip_problem *p, const NdFacts &F, int64_t c0, int64_t B, const double *op_values, bool resume, double dV,
                             NdBatchProgram &P) {
    const int64_t T = p->T;
    const int npass = F.npass;
    const size_t nT = (size_t)T * B;
    P = NdBatchProgram();
    P.kindF.assign(nT, SRC_PREV); P.kindB.assign(nT, SRC_PREV);
    P.tapF.assign((size_t)std::max(1, npass) * nT, -1); P.tapB.assign((size_t)std::max(1, npass) * nT, -1);
    if (F.has_stage) { P.stepKF.assign(nT, SRC_PREV); P.stepKB.assign(nT, SRC_PREV); P.limit.assign((size_t)npass * B, 0.0); }
    std::vector<int> op_tap(p->n_ops, -1);
    for (int64_t b = 0; b < B; ++b) {
        const double *val = op_values ? op_values + (c0 + b) * p->n_ops : nullptr;
        std::fill(op_tap.begin(), op_tap.end(), -1);
        for (int k = 0; k < p->n_ops; ++k)
            if (p->ops[k].kind == BLHIP_OP_GRW) {
                const double ns = val[k] / p->lattice[p->ops[k].axis];                    // transitionModels.py:108
                if (std::isnan(ns)) fail("chain %lld: GRW sigma is NaN", (long long)(c0 + b));
                op_tap[k] = ns > 0.0 ? P.taps.get(p->ops[k].axis, ns) : -1;              // :110-113
            } else if (p->ops[k].kind == BLHIP_OP_NOTEQUAL) {
                for (int q = 0; q < npass; ++q) if (F.pass_ops[q] == k) P.limit[(size_t)q * B + b] = std::pow(10.0, val[k]) * dV;      // :468
            }
        for (int64_t t = 0; t < T; ++t) {
            const size_t k = (size_t)t * B + b;
            double tau = 0.0;
            bool rnF = false, rnB = false;
            if (nd_stamp(p, resume, t, true, tau)) rnF = nd_transition(p, F, val, op_tap, P.taps, tau, t, true, P.kindF[k], &P.tapF[k], nT);
            else P.kindF[k] = SRC_PRIOR;                                            // core.py:363
            if (nd_stamp(p, resume, t, false, tau)) rnB = nd_transition(p, F, val, op_tap, P.taps, tau, t, false, P.kindB[k], &P.tapB[k], nT);
            else P.kindB[k] = SRC_UNIFORM;
            if (F.has_stage) { P.stepKF[k] = rnF ? (unsigned char)SRC_PREV : P.kindF[k]; P.stepKB[k] = rnB ? (unsigned char)SRC_PREV : P.kindB[k]; }
        }
    }
    P.taps.w.resize(P.taps.w.size() + 8, 0.0);
    for (int v : P.taps.lw) P.lw_max = std::max(P.lw_max, v);
    for (int q = 0; !F.has_stage && q < npass; ++q) {
        int lw_q = 0;
        for (size_t k = 0; k < nT; ++k) {
            const int f = P.tapF[(size_t)q * nT + k], r = P.tapB[(size_t)q * nT + k];
            if (f >= 0) lw_q = std::max(lw_q, P.taps.lw[f]);
            if (r >= 0) lw_q = std::max(lw_q, P.taps.lw[r]);
        }
        if (lw_q > 0) { P.walks_on += 1; P.W_taps += 2 * lw_q + 1; }
        if (lw_q > p->n[p->ops[F.pass_ops[q]].axis]) P.beyond_axis = true;
    }
    for (int q = 0; q < npass; ++q) {
        const int pk = F.pass_kind[q];
        bool on = false;
        int lw_q = 0;
        for (size_t k = 0; k < nT; ++k) {
            const int f = P.tapF[(size_t)q * nT + k], r = P.tapB[(size_t)q * nT + k];
            on = on || f >= 0 || r >= 0;
            if (pk == 1) continue;                                                  // (NotEqual's 0 is a flag, not a tap set)
            if (f >= 0) lw_q = std::max(lw_q, P.taps.lw[f]);
            if (r >= 0) lw_q = std::max(lw_q, P.taps.lw[r]);
        }
        if (pk == 0) P.lw_walk_max = std::max(P.lw_walk_max, lw_q);
        if (pk == 2) P.lw_shift_max = std::max(P.lw_shift_max, lw_q);
        if (pk == 1 && on) { P.stage_launches += 3; P.stage_sweeps += 3; }
        if (pk != 1 && lw_q > 0) { P.stage_launches += 1; P.stage_filters += 1; P.stage_W += 2 * lw_q + 1; P.stage_sweeps += pk == 2 ? 1 : 0; P.stage_shifts += pk == 2 ? 1 : 0; }
        if (pk == 0 && lw_q > p->n[p->ops[F.pass_ops[q]].axis]) P.stage_beyond_axis = true;
    }
}
