// The transition program of a batch: validation of a blhip_problem, the per-step data records, and build_program -- per (step, chain) what a
// step consumes and filters with, on grids with one and two parameters (3 and 4: blhip_nd_program.hpp); the tap tables of the models' kernels: blhip_taps.hpp
// (reference: transitionModels.py:96-118, :289-317, :632-662, :756-818; core.py:411, :467).
// Part of libblhip's host side: included by blhip.hip INSIDE its anonymous namespace (one translation unit; the split is by subject, not by linkage).
#pragma once

#include "blhip_taps.hpp"      // TapTable

struct Geometry {
    int n0, n1;          // internal rows / cols
    int axis_map[2];     // ABI parameter index -> internal axis
    long long G;
};

void validate(const blhip_problem *p, int64_t n_chains, const double *op_values) {
    if (!p) fail("problem is NULL");
    if (p->ndim < 1 || p->ndim > BLHIP_MAX_DIM) fail("ndim must be 1 .. %d (got %d)", BLHIP_MAX_DIM, p->ndim);
    if (p->ndim > 2) {            // the plain N-D path (blhip_nd.hpp)
        if (p->obs_model != BLHIP_OM_TABLE && p->obs_model != BLHIP_OM_PROGRAM)
            fail("grids with %d parameters need a caller-evaluated likelihood table (BLHIP_OM_TABLE) or a likelihood program (BLHIP_OM_PROGRAM)", p->ndim);
        // (the stages of blhip_nd_stages.hpp carry NotEqual and Deterministic; Independent, break-points and serial models are host-side
        //  bookkeeping of do_fit_nd.  The reference itself refuses AlphaStableRandomWalk beyond two parameters, transitionModels.py:213-215)
        for (int k = 0; k < p->n_ops; ++k) {
            const int kind = p->ops[k].kind;
            if (kind == BLHIP_OP_REGIMESWITCH || kind == BLHIP_OP_ALPHASTABLE || kind == BLHIP_OP_BIVARIATE)
                fail("grids with %d parameters do not support RegimeSwitch / AlphaStableRandomWalk / BivariateRandomWalk transition models "
                     "(op %d has kind %d)", p->ndim, k, kind);
        }
    }
    for (int k = 0; k < p->ndim; ++k) {
        if (p->n[k] < 1) fail("grid size n[%d] = %lld", k, (long long)p->n[k]);
        if (!p->marginal[k]) fail("marginal[%d] is NULL", k);
        if (p->n[k] > (1ll << 30)) fail("grid axis too long");
    }
    if (p->T < 1) fail("T must be >= 1");
    if (!p->data || !p->timestamps || !p->prior) fail("data / timestamps / prior must not be NULL");
    if (n_chains < 1) fail("n_chains must be >= 1");
    if (p->n_ops < 0 || (p->n_ops > 0 && !p->ops)) fail("bad transition program");
    if (p->n_ops > 0 && !op_values) fail("op_values is NULL");
    bool has_cp = false;
    for (int k = 0; k < p->n_ops; ++k) {
        const blhip_op &op = p->ops[k];
        if (op.kind == BLHIP_OP_GRW) {
            if (op.axis < 0 || op.axis >= p->ndim) fail("GRW op %d: axis %d out of range", k, op.axis);
        } else if (op.kind == BLHIP_OP_CHANGEPOINT) {
            has_cp = true;
        } else if (op.kind == BLHIP_OP_INDEPENDENT) {
            if (!p->indep_prior) fail("INDEPENDENT op needs indep_prior");
        } else if (op.kind == BLHIP_OP_DETERMINISTIC) {
            if (op.axis < 0 || op.axis >= p->ndim) fail("DETERMINISTIC op %d: axis %d out of range", k, op.axis);
            for (int64_t q = 1; q <= 2 * p->T; ++q)
                if (k + q >= p->n_ops || p->ops[k + q].kind != BLHIP_OP_DETERMINISTIC_ARG)
                    fail("DETERMINISTIC op %d must be followed by 2 T = %lld DETERMINISTIC_ARG ops (the shifts per step)", k, (long long)(2 * p->T));
        } else if (op.kind == BLHIP_OP_ALPHASTABLE) {
            if (op.axis < 0 || op.axis >= p->ndim) fail("ALPHASTABLE op %d: axis %d out of range", k, op.axis);
            if (k + 1 >= p->n_ops || p->ops[k + 1].kind != BLHIP_OP_ALPHASTABLE_ARG)
                fail("ALPHASTABLE op %d must be followed by an ALPHASTABLE_ARG op (alpha)", k);
        } else if (op.kind == BLHIP_OP_BIVARIATE) {
            if (p->ndim != 2) fail("BIVARIATE op %d needs a 2-parameter grid", k);
            if (k + 2 >= p->n_ops || p->ops[k + 1].kind != BLHIP_OP_BIVARIATE_ARG || p->ops[k + 2].kind != BLHIP_OP_BIVARIATE_ARG)
                fail("BIVARIATE op %d must be followed by two BIVARIATE_ARG ops (sigma2, rho)", k);
        } else if (op.kind != BLHIP_OP_STATIC && op.kind != BLHIP_OP_REGIMESWITCH && op.kind != BLHIP_OP_BREAKPOINT &&
                   op.kind != BLHIP_OP_NOTEQUAL && op.kind != BLHIP_OP_BIVARIATE_ARG && op.kind != BLHIP_OP_ALPHASTABLE_ARG &&
                   op.kind != BLHIP_OP_DETERMINISTIC_ARG) {
            fail("op %d: unknown kind %d", k, op.kind);
        }
    }
    if (has_cp && !p->reset_prior) fail("CHANGEPOINT op needs reset_prior");
    switch (p->obs_model) {
        case BLHIP_OM_POISSON:
            if (p->ndim != 1) fail("Poisson model has 1 parameter");
            if (p->seg_len != 1) fail("Poisson model has segment length 1");
            break;
        case BLHIP_OM_GAUSSIAN:
            if (p->ndim != 2) fail("Gaussian model has 2 parameters");
            if (p->seg_len != 1) fail("Gaussian model has segment length 1");
            break;
        case BLHIP_OM_GAUSSIAN_MEAN:
            if (p->ndim != 1) fail("GaussianMean model has 1 parameter");
            if (p->seg_len != 1 || p->data_dim != 2) fail("GaussianMean data must be (T, 1, 2)");
            break;
        case BLHIP_OM_TABLE:
            if (!p->lik) fail("BLHIP_OM_TABLE needs lik");
            break;
        case BLHIP_OM_PROGRAM:
            if (p->seg_len != 1) fail("BLHIP_OM_PROGRAM: likelihood programs have segment length 1");
            break;
        case BLHIP_OM_BERNOULLI: case BLHIP_OM_WHITE_NOISE:
            if (p->ndim != 1 || p->seg_len != 1) fail("Bernoulli / white-noise models have 1 parameter and segment length 1");
            break;
        case BLHIP_OM_LAPLACE:
            if (p->ndim != 2 || p->seg_len != 1) fail("Laplace model has 2 parameters and segment length 1");
            break;
        case BLHIP_OM_AR1: case BLHIP_OM_SCALED_AR1:
            if (p->ndim != 2 || p->seg_len != 2) fail("AR1 models have 2 parameters and segment length 2");
            break;
        default: fail("unknown observation model %d", p->obs_model);
    }
    if (p->data_dim < 1) fail("data_dim must be >= 1");
}

// ---- the direct domain of the Poisson likelihood ------------------------------------------------------------------------------------------
// blk::likelihood<OM_POISSON> forms lambda^k exp(-lambda) / k! factor by factor (observationModels.py:502).  That is sound only while each
// factor is an ordinary float64: k! is inf from k = 171 on, lambda^k overflows beyond ln(DBL_MAX) = 709.78, exp(-lambda) leaves the normal
// range beyond lambda = 708.39.  A record is in the direct domain when every count is at most POISSON_MAX_COUNT, max count * ln(max rate)
// stays below POISSON_MAX_LOG_POW (9 below the overflow threshold: pow()'s and log()'s own rounding are many orders smaller) and the
// largest rate is at most POISSON_MAX_RATE (exp(-708) = 3.3e-308, normal).  Every other record is evaluated in log space:
// exp(k ln(lambda) - lambda - ln k!), with ln k! from lgammal_r in long double, rounded to float64 once.  counts: the dd values of one record, NaN values count for nothing.
constexpr double POISSON_MAX_COUNT = 170.0, POISSON_MAX_LOG_POW = 700.0, POISSON_MAX_RATE = 708.0;

inline bool poisson_direct_domain(const double *counts, int dd, double max_rate) {
    double kmax = 0.0;
    for (int k = 0; k < dd; ++k)
        if (!std::isnan(counts[k])) kmax = std::max(kmax, counts[k]);
    if (kmax > POISSON_MAX_COUNT || !(max_rate <= POISSON_MAX_RATE)) return false;
    return kmax == 0.0 || max_rate <= 1.0 || kmax * std::log(max_rate) <= POISSON_MAX_LOG_POW;
}

inline double max_of(const double *v, int64_t n) {
    double m = -std::numeric_limits<double>::infinity();
    for (int64_t j = 0; j < n; ++j) m = std::max(m, v[j]);
    return m;
}

// per-step records consumed by blk::likelihood<>
void build_records(const blhip_problem *p, std::vector<double> &rec, int &rec_len, int &d) {
    const int64_t T = p->T;
    const int dd = p->data_dim;
    if (p->obs_model == BLHIP_OM_GAUSSIAN) {
        d = dd; rec_len = dd;
        rec.assign(p->data, p->data + T * dd);
    } else if (p->obs_model == BLHIP_OM_GAUSSIAN_MEAN) {
        d = 1; rec_len = 3;
        rec.resize(T * 3);
        for (int64_t t = 0; t < T; ++t) {
            const double x = p->data[t * 2], s = p->data[t * 2 + 1];
            const bool miss = std::isnan(x) || std::isnan(s);
            rec[t * 3 + 0] = miss ? std::numeric_limits<double>::quiet_NaN() : x;
            rec[t * 3 + 1] = 1.0 / (2.0 * s * s);
            rec[t * 3 + 2] = 0.5 * std::log(2.0 * M_PI * s * s);
        }
    } else if (p->obs_model == BLHIP_OM_POISSON) {
        d = dd; rec_len = 2 * dd;
        rec.resize(T * 2 * dd);
        const double max_rate = max_of(p->marginal[0], p->n[0]);
        for (int64_t t = 0; t < T; ++t) {
            for (int k = 0; k < dd; ++k) {
                const double c = p->data[t * dd + k];
                if (!std::isnan(c) && (c < 0 || c != std::floor(c))) fail("Poisson data must be non-negative integers (step %lld)", (long long)t);
            }
            const bool direct = poisson_direct_domain(p->data + t * dd, dd, max_rate);
            for (int k = 0; k < dd; ++k) {
                const double c = p->data[t * dd + k];
                double f = direct ? 1.0 : 0.0;
                if (!std::isnan(c)) {
                    if (direct) for (double q = 2.0; q <= c; q += 1.0) f *= q;
                    else { int sign; f = (double)lgammal_r((long double)c + 1.0L, &sign); }      // (long double, rounded once; no global signgam)
                }
                rec[(t * dd + k) * 2] = c;
                rec[(t * dd + k) * 2 + 1] = direct ? f : -f;      // (the sign bit selects the log-space route: -0.0 for k <= 1 and for NaN)
            }
        }
    } else {
        d = 1; rec_len = 1;
        rec.assign(T, 0.0);
    }
}

struct StepProg {
    unsigned char kind = SRC_PREV, cmode = 0;   // cmode: 0 none, 1 clamp the source (before the stencil), 2 clamp after it
    int t0 = -1, t1 = -1;
    double limit = 0.0;
};
constexpr unsigned char STAGE_NEXT_NE = 16;     // (a pre-stage's cmode bit: the stage after it is a NotEqual model)

struct ChainProgram {
    // per (step, chain): source kind, tap ids per internal axis, clamp mode/limit (RegimeSwitch); forward and backward
    std::vector<unsigned char> kindF, kindB, cmodeF, cmodeB;
    std::vector<int> tapF0, tapF1, tapB0, tapB1;
    std::vector<double> limitF, limitB;
    int LW0 = 0, LW1 = 0;
    bool has_clamp = false;
    bool whole_row = false;      // a two-stage spline shift (Deterministic, |d| > 12): a block needs the whole row of a 1-D grid
    bool other_clamp = false;    // has_clamp for another reason than a Deterministic model's shift (mode 6)
    bool dense_clamp = false;    // ... than a shift or the clamps of RegimeSwitch / NotEqual: AlphaStable- / BivariateRandomWalk (modes 5 / 4: zero boundary, dense kernels)
    bool has_shift = false;      // a Deterministic model
    // Composed transitions (a CombinedTransitionModel whose sub-models do not fit into ONE step of the generic kernel, transitionModels.py:
    // 632-662): the transition of a (step, chain) is a list of stages applied in list order.  The fused step kernel applies the LAST one,
    // blk::step_kernel<.., MODE_STAGE_*> (the stage kernel) the ones in front of it.  Step t (per direction) runs nst[t] stages in front of
    // the fused kernel for EVERY chain of the batch -- a chain with fewer gets identity stages (copies) at the front -- and the fused kernel
    // then reads the last stage's output (kind SRC_PREV).  Stage s of step t, chain b: pre[off[t] + s B + b]; its cmode may carry
    // STAGE_NEXT_NE.  Empty unless `multi`, which sets has_clamp too (the kernels' clamp bookkeeping carries the stages' scales).
    bool multi = false;
    std::vector<int> nstF, nstB;
    std::vector<size_t> offF, offB;
    std::vector<StepProg> preF, preB;
};

void build_program(const blhip_problem *p, const Geometry &g, int64_t c0, int64_t B, const double *op_values,
                   TapTable &taps, ChainProgram &prog, bool resume) {
    const int64_t T = p->T;
    const int nops = p->n_ops;
    const size_t nT = (size_t)T * B;
    prog.kindF.assign(nT, SRC_PREV); prog.kindB.assign(nT, SRC_PREV);
    prog.cmodeF.assign(nT, 0); prog.cmodeB.assign(nT, 0);
    prog.limitF.assign(nT, 0.0); prog.limitB.assign(nT, 0.0);
    prog.tapF0.assign(nT, -1); prog.tapF1.assign(nT, -1);
    prog.tapB0.assign(nT, -1); prog.tapB1.assign(nT, -1);
    prog.LW0 = prog.LW1 = 0;
    prog.has_clamp = false;
    prog.whole_row = false;
    prog.other_clamp = false;
    prog.dense_clamp = false;
    prog.has_shift = false;
    prog.multi = false;
    prog.nstF.clear(); prog.nstB.clear(); prog.offF.clear(); prog.offB.clear(); prog.preF.clear(); prog.preB.clear();
    double dV = 1.0;
    for (int k = 0; k < p->ndim; ++k) dV *= p->lattice[k];
    // the ops a step's program is made of (the *_ARG ops only carry values of the op in front of them: a Deterministic model has 2 T of
    // them, and the per-(step, chain) walk below would spend its time skipping them -- 23 400 chains x 41 steps x 2 x 87 ops measured)
    std::vector<int> real_ops;
    for (int k = 0; k < nops; ++k) {
        const int kind = p->ops[k].kind;
        if (kind != BLHIP_OP_DETERMINISTIC_ARG && kind != BLHIP_OP_BIVARIATE_ARG && kind != BLHIP_OP_ALPHASTABLE_ARG) real_ops.push_back(k);
    }
    // (a chain's T steps are T entries B apart in each of the ten arrays: written chain by chain that is one cache line per entry --
    //  half of the 30 ms this function took for the 23 400 chains x 41 steps of the published break-point study.  The steps of GROUP
    //  chains are collected first and written out as runs of GROUP consecutive entries)
    // (no more entries than the batch has chains: constructing 64 x T records for the ONE chain of a long single-chain fit -- C2: T = 10 000,
    //  2 x 15 MB -- was 8 ms of its 43-ms fit)
    constexpr int GROUP = 64;
    const size_t group_rows = (size_t)std::min<int64_t>(GROUP, std::max<int64_t>(B, 1));
    std::vector<StepProg> gF(group_rows * T), gB(group_rows * T);
    auto flush_group = [&](int64_t b0, int64_t nb) {
        for (int64_t t = 0; t < T; ++t) {
            const size_t k0 = (size_t)t * B + b0;
            for (int64_t q = 0; q < nb; ++q) {
                const StepProg &f = gF[(size_t)q * T + t], &r = gB[(size_t)q * T + t];
                prog.kindF[k0 + q] = f.kind; prog.tapF0[k0 + q] = f.t0; prog.tapF1[k0 + q] = f.t1; prog.cmodeF[k0 + q] = f.cmode; prog.limitF[k0 + q] = f.limit;
                prog.kindB[k0 + q] = r.kind; prog.tapB0[k0 + q] = r.t0; prog.tapB1[k0 + q] = r.t1; prog.cmodeB[k0 + q] = r.cmode; prog.limitB[k0 + q] = r.limit;
            }
        }
    };
    std::vector<int> op_tap(nops, -1), op_axis(nops, -1);
    // (see `at` below) the ops that bound segments or fire at a time stamp; per chain: the program of each segment, walked once
    std::vector<int> bound_ops;
    for (int k : real_ops)
        if (p->ops[k].kind == BLHIP_OP_BREAKPOINT || p->ops[k].kind == BLHIP_OP_CHANGEPOINT) bound_ops.push_back(k);
    std::vector<StepProg> seg_prog(bound_ops.size() + 1);
    std::vector<std::vector<StepProg>> seg_pre(bound_ops.size() + 1);       // (the stages in front of seg_prog's: see ChainProgram::multi)
    std::vector<char> seg_cached(bound_ops.size() + 1, 0), det_in_seg(bound_ops.size() + 1, 0);
    // (step, chain) transitions with stages in front of the last one, collected here (composed batches only) and laid out after the walk
    struct PreRec { int64_t t, b; std::vector<StepProg> st; };
    std::vector<PreRec> recF, recB;
    std::vector<StepProg> stat_pre, scratch_pre, resume_pre;
    const std::vector<StepProg> no_pre;
    for (int64_t b = 0; b < B; ++b) {
        const double *val = op_values ? op_values + (c0 + b) * nops : nullptr;
        // tap ids of this chain's GRW ops
        std::fill(op_tap.begin(), op_tap.end(), -1); std::fill(op_axis.begin(), op_axis.end(), -1);
        bool time_dependent = false;
        for (int k = 0; k < nops; ++k) {
            const blhip_op &op = p->ops[k];
            if (op.kind == BLHIP_OP_GRW) {
                const int ax = g.axis_map[op.axis];
                const double ns = val[k] / p->lattice[op.axis];            // transitionModels.py:108
                op_axis[k] = ax;
                op_tap[k] = (ns > 0.0) ? taps.get(ax, ns) : -1;            // :110-113 (sigma <= 0: copy)
                if (std::isnan(ns)) fail("chain %lld: GRW sigma is NaN", (long long)(c0 + b));
            } else if (op.kind == BLHIP_OP_CHANGEPOINT || op.kind == BLHIP_OP_BREAKPOINT) {
                time_dependent = true;
            } else if (op.kind == BLHIP_OP_REGIMESWITCH || op.kind == BLHIP_OP_NOTEQUAL) {
                prog.has_clamp = true; prog.other_clamp = true;
            } else if (op.kind == BLHIP_OP_DETERMINISTIC) {
                time_dependent = true;                       // a different shift at every step
                op_axis[k] = g.axis_map[op.axis];
                prog.has_clamp = true;                       // (mode 6 of the generic kernel)
                prog.has_shift = true;
            } else if (op.kind == BLHIP_OP_ALPHASTABLE) {
                const double c = val[k] / p->lattice[op.axis], alpha = val[k + 1];          // transitionModels.py:170-176
                if (std::isnan(c) || std::isnan(alpha)) fail("chain %lld: AlphaStableRandomWalk parameters are NaN", (long long)(c0 + b));
                op_axis[k] = g.axis_map[op.axis];
                op_tap[k] = taps.get_alphastable(op_axis[k], c, alpha, (int)p->n[op.axis]);
                prog.has_clamp = true; prog.other_clamp = true; prog.dense_clamp = true;      // (mode 5 of the generic kernel: zero boundary + renormalisation)
            } else if (op.kind == BLHIP_OP_BIVARIATE) {
                // transitionModels.py:881-885; a singular covariance makes scipy.stats.multivariate_normal raise in the reference
                const double n1 = val[k] / p->lattice[0], n2 = val[k + 1] / p->lattice[1], rho = val[k + 2];
                if (!(n1 > 0.0) || !(n2 > 0.0) || !(std::fabs(rho) < 1.0))
                    fail("chain %lld: BivariateRandomWalk needs sigma1, sigma2 > 0 and |rho| < 1", (long long)(c0 + b));
                op_tap[k] = taps.get2d(n1, n2, rho);
                prog.has_clamp = true; prog.other_clamp = true; prog.dense_clamp = true;      // (mode 4 of the generic kernel: dense kernel + renormalisation)
            }
        }
        // the transition from one step to the next, evaluated at time stamp tau (list order, transitionModels.py:645-649)
        // -> the last stage; `pre` receives the stages in front of it (a composition the current stage cannot absorb closes it: `close`)
        auto run = [&](std::vector<StepProg> &pre, double tau, bool have_tau, int64_t step = -1, bool fwd = true) {
            StepProg sp;
            pre.clear();
            int seg = 0;                                                   // active sub-model of a serial model (:768)
            if (have_tau)
                for (int k : real_ops) {
                    const blhip_op &op = p->ops[k];
                    if ((op.kind == BLHIP_OP_BREAKPOINT || (op.kind == BLHIP_OP_CHANGEPOINT && (op.flags & 1))) && val[k] <= tau) seg++;
                }
            bool filtered = false;
            auto close = [&]() { pre.push_back(sp); sp = StepProg(); filtered = false; };      // the next stage reads this one's output
            for (int k : real_ops) {
                const blhip_op &op = p->ops[k];
                if (op.segment >= 0 && op.segment != seg) continue;
                switch (op.kind) {
                    case BLHIP_OP_GRW: {
                        if (op_tap[k] < 0) break;
                        // (after a RegimeSwitch that clamps a filtered distribution, a Bivariate- / AlphaStableRandomWalk, a Deterministic
                        //  model or another walk on the same parameter: a new stage)
                        if (sp.cmode == 2 || sp.cmode == 4 || sp.cmode == 5 || (op_axis[k] == 0 ? sp.t0 : sp.t1) >= 0) close();
                        (op_axis[k] == 0 ? sp.t0 : sp.t1) = op_tap[k];
                        filtered = true;
                        break;
                    }
                    case BLHIP_OP_CHANGEPOINT:
                        if (!(op.flags & 1) && have_tau && tau == val[k]) {      // transitionModels.py:300-312 (drops the stages before it)
                            sp = StepProg(); sp.kind = SRC_RESET; filtered = false; pre.clear();
                        }
                        break;
                    case BLHIP_OP_INDEPENDENT:                                    // transitionModels.py:351-360
                        sp = StepProg(); sp.kind = SRC_INDEP; filtered = false; pre.clear();
                        break;
                    case BLHIP_OP_DETERMINISTIC: {                                // transitionModels.py:571-583, :585-602
                        if (step < 0) break;                                      // (the time-independent template program)
                        const double dd = val[k + 1 + (fwd ? step : T + step)] / p->lattice[op.axis];
                        if (std::isnan(dd)) fail("chain %lld: Deterministic shift of step %lld is NaN", (long long)(c0 + b), (long long)step);
                        if (std::fabs(dd) > 12.0 && g.n0 == 1 && (double)g.n1 > 16000.0)
                            fail("chain %lld, step %lld: Deterministic model shifts by %.3g grid cells in one time step; on 1-D grids beyond 16000 "
                                 "points the step and stage kernels support up to 12 (SciPy's pre-padding)",
                                 (long long)(c0 + b), (long long)step, dd);
                        if (std::fabs(dd) > 12.0 && g.n0 != 1) {
                            // a large shift on a 2-D grid: a stage of its own (blk::bigshift_kernel), nothing fused into it -- the stage in
                            // front of it is closed if it holds anything, and what follows (at least the identity the fused step kernel
                            // applies, reading 1 / D from this stage's partials) starts a new one
                            const long long nline = op_axis[k] == 0 ? g.n0 : g.n1;
                            if (nline > BIGSHIFT_MAX_LINE)
                                fail("chain %lld, step %lld: Deterministic model shifts by %.3g grid cells in one time step along an axis of %lld "
                                     "points; on grids with two parameters shifts beyond 12 cells (SciPy's pre-padding) are supported on axes of "
                                     "up to %d points", (long long)(c0 + b), (long long)step, dd, nline, BIGSHIFT_MAX_LINE);
                            if (sp.t0 >= 0 || sp.t1 >= 0 || sp.cmode != 0) close();
                            (op_axis[k] == 0 ? sp.t0 : sp.t1) = taps.get_bigshift2(dd);
                            sp.cmode = 6;
                            close();
                            break;
                        }
                        if (dd != 0.0) {                                          // zero shift: identity (its renormalisation is a no-op)
                            if ((op_axis[k] == 0 ? sp.t0 : sp.t1) >= 0 || (sp.cmode != 0 && sp.cmode != 6)) close();
                            int &slot = op_axis[k] == 0 ? sp.t0 : sp.t1;
                            if (std::fabs(dd) > 12.0) { slot = taps.get_bigshift(dd); prog.whole_row = true; }
                            else slot = taps.get_shift(op_axis[k], dd);
                            sp.cmode = 6;
                        }
                        filtered = true;
                        break;
                    }
                    case BLHIP_OP_ALPHASTABLE: {                                  // transitionModels.py:167-187
                        if (sp.cmode != 0 || filtered) close();
                        sp.cmode = 5;
                        (op_axis[k] == 0 ? sp.t0 : sp.t1) = op_tap[k];
                        filtered = true;
                        break;
                    }
                    case BLHIP_OP_BIVARIATE:                                      // transitionModels.py:880-891
                        if (sp.cmode != 0 || filtered) close();
                        sp.cmode = 4;
                        sp.t0 = op_tap[k];
                        filtered = true;
                        break;
                    case BLHIP_OP_NOTEQUAL:                                       // transitionModels.py:462-471
                        // (it inverts around the maximum and the sum of its input, which the kernels know of a state or a stage's
                        //  output: after a restart the shared distribution is copied by an identity stage first)
                        if (sp.cmode != 0 || filtered || sp.kind != SRC_PREV) close();
                        sp.cmode = 3;
                        sp.limit = std::pow(10.0, val[k]) * dV;
                        break;
                    case BLHIP_OP_REGIMESWITCH:                                   // transitionModels.py:405-410
                        if (sp.cmode != 0) close();
                        sp.cmode = filtered ? 2 : 1;
                        sp.limit = std::pow(10.0, val[k]) * dV;
                        break;
                    default: break;
                }
            }
            if (have_tau)
                for (int k : real_ops) {                                          // serial change-points, :801-813
                    const blhip_op &op = p->ops[k];
                    if (op.kind == BLHIP_OP_CHANGEPOINT && (op.flags & 1) && tau == val[k]) { sp = StepProg(); sp.kind = SRC_RESET; pre.clear(); }
                }
            auto radii = [&](const StepProg &q) {
                if (q.t0 >= 0) prog.LW0 = std::max(prog.LW0, taps.lw[q.t0]);
                if (q.cmode == 4) prog.LW1 = std::max(prog.LW1, taps.lw2[q.t0]);
                if (q.t1 >= 0) prog.LW1 = std::max(prog.LW1, taps.lw[q.t1]);
            };
            radii(sp);
            for (const StepProg &q : pre) radii(q);
            return sp;
        };
        const StepProg stat = run(stat_pre, 0.0, false);       // the program when nothing depends on the time stamp
        // A step's program depends on its time stamp through (1) the active sub-model of a serial model = how many break- / serial
        // change-points lie at or before it, (2) a change-point AT it, (3) the step index of a Deterministic model in the active part.
        // Steps that share (1), have no (2) and no (3) share their program: it is walked once per chain and segment -- two thirds of the
        // (chain, step) pairs of the published break-point study sit in Static segments (build_program 28 -> 15 ms of a 92-ms fit).
        const std::vector<StepProg> *pre_of = &no_pre;       // (set by `at`: the stages in front of the program it returns)
        auto at = [&](double tau, int64_t step, bool fwd) -> StepProg {
            int seg = 0;
            bool event = false;
            for (int k : bound_ops) {
                const blhip_op &op = p->ops[k];
                const bool serial = op.kind == BLHIP_OP_BREAKPOINT || (op.flags & 1);
                if (serial && val[k] <= tau) seg++;
                if (op.kind == BLHIP_OP_CHANGEPOINT && tau == val[k]) event = true;
            }
            if (event || det_in_seg[seg]) { pre_of = &scratch_pre; return run(scratch_pre, tau, true, step, fwd); }
            if (!seg_cached[seg]) { seg_prog[seg] = run(seg_pre[seg], tau, true, step, fwd); seg_cached[seg] = 1; }
            pre_of = &seg_pre[seg];
            return seg_prog[seg];
        };
        if (time_dependent) {
            std::fill(seg_cached.begin(), seg_cached.end(), 0);
            std::fill(det_in_seg.begin(), det_in_seg.end(), 0);
            for (int k : real_ops)
                if (p->ops[k].kind == BLHIP_OP_DETERMINISTIC)
                    for (size_t sg = 0; sg < det_in_seg.size(); ++sg)
                        if (p->ops[k].segment < 0 || (size_t)p->ops[k].segment == sg) det_in_seg[sg] = 1;
        }
        for (int64_t t = 0; t < T; ++t) {
            // forward step t consumes T_fwd(post_{t-1}, ts[t-1])   core.py:411
            StepProg f; f.kind = SRC_PRIOR;
            const std::vector<StepProg> *fpre = &no_pre, *rpre = &no_pre;
            if (t > 0) { pre_of = &stat_pre; f = time_dependent ? at(p->timestamps[t - 1], t, true) : stat; fpre = pre_of; }
            else if (resume) { f = run(resume_pre, p->resume_time, true, 0, true); fpre = &resume_pre; }   // continues a carried state (OnlineStudy.step, core.py:2164-2165)
            if (!fpre->empty()) recF.push_back(PreRec{t, b, *fpre});
            // backward step t consumes T_bwd(beta_{t+1} L_{t+1}, ts[t+1]) = T_fwd(., ts[t+1] - 1)   core.py:467, transitionModels.py:316-317
            StepProg r; r.kind = SRC_UNIFORM;
            if (t < T - 1) { pre_of = &stat_pre; r = time_dependent ? at(p->timestamps[t + 1] - 1.0, t, false) : stat; rpre = pre_of; }
            if (!rpre->empty()) recB.push_back(PreRec{t, b, *rpre});
            gF[(size_t)(b % GROUP) * T + t] = f; gB[(size_t)(b % GROUP) * T + t] = r;
        }
        if (b % GROUP == GROUP - 1 || b == B - 1) flush_group(b - b % GROUP, b % GROUP + 1);
    }
    if (recF.empty() && recB.empty()) return;
    // ---- composed transitions: the per-step stage tables (ChainProgram::multi) ----
    prog.multi = true;
    prog.has_clamp = true;
    auto lay_out = [&](std::vector<PreRec> &recs, std::vector<int> &nst, std::vector<size_t> &off, std::vector<StepProg> &pre,
                       std::vector<unsigned char> &kind, std::vector<int> &tap0, std::vector<int> &tap1, std::vector<unsigned char> &cmode,
                       std::vector<double> &limit) {
        nst.assign(T, 0);
        off.assign(T + 1, 0);
        for (const PreRec &r : recs) nst[r.t] = std::max(nst[r.t], (int)r.st.size());
        for (int64_t t = 0; t < T; ++t) off[t + 1] = off[t] + (size_t)nst[t] * B;
        pre.assign(off[T], StepProg());
        std::vector<int> which(recs.empty() ? 0 : nT, -1);
        for (size_t q = 0; q < recs.size(); ++q) which[(size_t)recs[q].t * B + recs[q].b] = (int)q;
        std::vector<StepProg> list;
        for (int64_t t = 0; t < T; ++t) {
            const int n = nst[t];
            if (n == 0) continue;
            for (int64_t b = 0; b < B; ++b) {
                const size_t e = (size_t)t * B + b;
                StepProg last; last.kind = kind[e]; last.t0 = tap0[e]; last.t1 = tap1[e]; last.cmode = cmode[e]; last.limit = limit[e];
                const int q = which[e];
                const int np = q >= 0 ? (int)recs[q].st.size() : 0;
                // identity stages in front (copies of the source), then the chain's own stages, then the last one (the fused kernel's)
                list.assign((size_t)(n - np), StepProg());
                if (q >= 0) list.insert(list.end(), recs[q].st.begin(), recs[q].st.end());
                list.push_back(last);
                list[0].kind = (n - np > 0) ? (np > 0 ? recs[q].st[0].kind : last.kind) : list[0].kind;
                for (size_t k = 1; k < list.size(); ++k) list[k].kind = SRC_PREV;
                for (int s2 = 0; s2 < n; ++s2) {
                    StepProg st = list[s2];
                    if ((list[s2 + 1].cmode & 15) == 3) st.cmode |= STAGE_NEXT_NE;
                    pre[off[t] + (size_t)s2 * B + b] = st;
                }
                kind[e] = SRC_PREV;
            }
        }
    };
    lay_out(recF, prog.nstF, prog.offF, prog.preF, prog.kindF, prog.tapF0, prog.tapF1, prog.cmodeF, prog.limitF);
    lay_out(recB, prog.nstB, prog.offB, prog.preB, prog.kindB, prog.tapB0, prog.tapB1, prog.cmodeB, prog.limitB);
}
