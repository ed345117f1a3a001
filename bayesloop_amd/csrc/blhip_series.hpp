// Series fits (blhip_set_series; Study.fitMany of bayesloop_amd): a batch of chains of the chain-resident 1-D kernel (blhip_chain1d.hpp) in
// which chain c observes its OWN data series -- the user's loop `for d in series: S.loadData(d); S.fit()` around Study.fit (reference
// core.py:330-486) as one blhip_fit.  What this file holds needs no GPU and no context: which problems the path admits (the one copy of
// the rules: blhip_host_series_check, do_fit and the Python side ask it) and its memory plan (blhip_host_series_plan; chains_per_batch
// counts a chain with the same figure).  The device side: bl1c::series_lik_kernel / series_table_kernel build the batch's (B, T, n)
// likelihood table, Row1dRun::series_table (blhip_fit_row1d.hpp) uploads the series and launches them.
// Part of libblhip's host side: included by blhip.hip INSIDE its anonymous namespace.
#pragma once

// bytes of one chain of a series batch: state ping-pong, the stored sequence, partial sums (as chains_per_batch counts any chain) + the
// chain's own (T, n) likelihood table
inline double series_chain_bytes(int64_t T, long long n, bool evidence_only) {
    return (evidence_only ? 2.0 : (double)T + 2.0) * (double)n * 8.0 + (double)T * NRED * 8.0 * 2 * 64.0 + (double)T * (double)n * 8.0;
}

// 0: the series path admits the problem; 1: it does not, the reason in err.  What depends on the chains' hyper-parameter values -- the
// radius of their walks against the row length and the LDS of a CU -- is left to the fit itself (plan_geometry), which fails with the reason.
inline int series_check(const blhip_problem *p, int64_t S, int flags, char *err, int errlen) {
    auto no = [&](const char *fmt, auto... a) { if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a...); return 1; };
    if (err && errlen > 0) err[0] = 0;
    if (!p) return no("the problem is NULL");
    if (S < 1) return no("%lld series", (long long)S);
    if (flags & (BLHIP_RESUME | BLHIP_CARRY | BLHIP_ACCUMULATE)) return no("BLHIP_RESUME / BLHIP_CARRY / BLHIP_ACCUMULATE do not go with series");
    if (p->ndim != 1) return no("a grid of %d parameters (series fits run on one-parameter grids)", p->ndim);
    switch (p->obs_model) {
        case BLHIP_OM_POISSON: case BLHIP_OM_GAUSSIAN_MEAN: case BLHIP_OM_BERNOULLI: case BLHIP_OM_WHITE_NOISE: break;
        case BLHIP_OM_TABLE: return no("BLHIP_OM_TABLE: a caller-evaluated likelihood table is one series' table");
        case BLHIP_OM_PROGRAM: return no("BLHIP_OM_PROGRAM: likelihood programs are armed per fit, not per series");
        default: return no("observation model %d has no table the device builds from the data records of a one-parameter grid", p->obs_model);
    }
    if (p->seg_len != 1) return no("segment length %d", p->seg_len);
    if (p->data_dim < 1 || (p->obs_model == BLHIP_OM_GAUSSIAN_MEAN && p->data_dim != 2)) return no("data dimension %d", p->data_dim);
    if (p->T < 1) return no("T = %lld", (long long)p->T);
    if (p->n[0] < 2 || p->n[0] > bl1c::NMAX_LONG) return no("a row of %lld cells (the chain-resident 1-D kernel takes 2 .. %d)", (long long)p->n[0], bl1c::NMAX_LONG);
    if (p->backward_init) return no("a backward_init message");
    if (p->n_ops < 0 || (p->n_ops > 0 && !p->ops)) return no("a bad transition program");
    for (int k = 0; k < p->n_ops; ++k) {
        const int kind = p->ops[k].kind;
        if (kind == BLHIP_OP_ALPHASTABLE || kind == BLHIP_OP_BIVARIATE)
            return no("op %d: AlphaStableRandomWalk / BivariateRandomWalk run on the launch-per-step kernel only", k);
        if ((flags & BLHIP_SERIES_RAGGED) && kind != BLHIP_OP_STATIC && kind != BLHIP_OP_GRW && kind != BLHIP_OP_REGIMESWITCH)
            return no("op %d (kind %d) depends on the time stamp or restarts the chain: series of different lengths or time stamps need a "
                      "program of Static / GaussianRandomWalk / RegimeSwitch ops", k, kind);
        if ((flags & BLHIP_SERIES_RAGGED) && p->ops[k].segment >= 0)
            return no("op %d belongs to a serial model: series of different lengths or time stamps need a time-independent program", k);
    }
    return 0;
}

// plan_out (4 values): chains per batch, batches, bytes of such a batch, the smallest budget accepted (one chain).  0; -1: bad arguments
// or a problem series_check refuses; 1: a budget below the minimum (plan_out[3] is still written).  Batch b covers the chains
// [b * per, min(S, (b + 1) * per)).  At most SERIES_MAX_BATCH chains per batch: the library's default for batches on 1-D grids.
constexpr int64_t SERIES_MAX_BATCH = 4096;
inline int series_plan(const blhip_problem *p, int64_t S, int flags, double budget, int64_t *plan_out) {
    if (!plan_out || series_check(p, S, flags, nullptr, 0) != 0 || !(budget >= 0.0)) return -1;
    const double per = series_chain_bytes(p->T, p->n[0], (flags & BLHIP_EVIDENCE_ONLY) != 0);
    plan_out[0] = plan_out[1] = plan_out[2] = 0;
    plan_out[3] = (int64_t)std::ceil(per);
    if (budget < (double)plan_out[3]) return 1;
    const int64_t B = std::min<int64_t>(std::min<int64_t>(S, SERIES_MAX_BATCH), (int64_t)std::floor(budget / per));
    plan_out[0] = B;
    plan_out[1] = (S + B - 1) / B;
    plan_out[2] = (int64_t)std::ceil(per * (double)B);
    return 0;
}
