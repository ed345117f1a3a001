// Series fits (blhip_set_series; Study.fitMany of bayesloop_amd): a batch of chains in which chain c observes its OWN data series -- the
// user's loop `for d in series: S.loadData(d); S.fit()` around Study.fit (reference core.py:330-486) as one blhip_fit.  One-parameter
// grids: chains of the chain-resident 1-D kernel (blhip_chain1d.hpp); two-parameter grids: chains of the chain-resident kernels
// blc::chain_kernel / blc::chainax_kernel (blhip_chainres.hpp, blhip_chainax.hpp), which re-base their records / anchors / likelihood table
// per chain (ChainParams::rec_chain, anch_chain, lik_chain).  What this file holds needs no GPU and no context: which problems the path
// admits (the one copy of the rules: blhip_host_series_check, do_fit and the Python side ask it) and its memory plan
// (blhip_host_series_plan; chains_per_batch counts a chain with the same figure).  The device side: bl1c::series_lik_kernel /
// series_table_kernel build the (B, T, n) likelihood table of a 1-D batch, Row1dRun::series_table (blhip_fit_row1d.hpp) uploads the series
// and launches them; ChainRun::series_tables (blhip_fit_paths.hpp) uploads a 2-D batch's series and builds its anchors or tables.
// Part of libblhip's host side: included by blhip.hip INSIDE its anonymous namespace, after blhip_chain_plan.hpp (the rows and strips the
// chain-resident kernels take).
#pragma once

// the geometry the chain-resident kernels lay a two-parameter chain out on (plan_chainres: rows 128 / 256 / 384 / 512 / 1024, columns a
// multiple of 16; walks on both parameters: the next square of 128 / 256 / 512) and what a series fit reads of the transition program
struct Series2dShape {
    bool both = false;                             // GaussianRandomWalks on both parameters: blc::chainax_kernel
    long long n0p = 0, n1p = 0, Gk = 0;
    int strips = 0;
    bool pad = false;
};
inline Series2dShape series_shape_2d(const blhip_problem *p) {
    Series2dShape s;
    const long long n0 = p->n[0], n1 = p->n[1];
    bool w0 = false, w1 = false;
    for (int k = 0; k < p->n_ops; ++k)
        if (p->ops[k].kind == BLHIP_OP_GRW) { if (p->ops[k].axis == 0) w0 = true; else w1 = true; }
    s.both = w0 && w1;
    // (the planner's own rule: chain_geometry, blhip_chain_plan.hpp; sizes beyond what series_check_2d admits are only ever refused)
    const ChainGeometry cg = chain_geometry((int)std::min<long long>(n0, 1 << 20), (int)std::min<long long>(n1, 1 << 20), s.both);
    s.n0p = cg.n0p; s.n1p = cg.n1p;
    s.Gk = s.n0p * s.n1p;
    s.strips = (int)(s.n1p / blc::WCOL);
    s.pad = s.n0p != n0 || s.n1p != n1;
    return s;
}

// Bytes of one chain of a series batch.  om: the observation model of the caller's problem (do_fit hands table models on as
// BLHIP_OM_TABLE).  One-parameter grids: state ping-pong, the stored sequence, partial sums (as chains_per_batch counts any chain) + the
// chain's own (T, n) likelihood table.  Two-parameter grids, on the padded geometry Gk: state ping-pong and stored sequence, partial
// sums, the de-padding copy (T, G) where the grid is padded or the both-axes kernels run and the fit keeps its sequence
// (chain_needs_depad), the chain's data, and its anchors -- T x NW x strips x 64 lanes x 32 bytes: the Gaussian model without a walk on
// the second parameter -- or its (T, G) likelihood table (the table models).
inline double series_chain_bytes(const blhip_problem *p, int om, bool evidence_only) {
    const double T = (double)p->T, sums = T * NRED * 8.0 * 2 * 64.0;
    if (p->ndim == 1) {
        const double n = (double)p->n[0];
        return (evidence_only ? 2.0 : T + 2.0) * n * 8.0 + sums + T * n * 8.0;
    }
    const Series2dShape s = series_shape_2d(p);
    const double G = (double)p->n[0] * (double)p->n[1], Gk = (double)s.Gk;
    double bytes = (evidence_only ? 2.0 : T + 2.0) * Gk * 8.0 + sums;
    if ((s.pad || s.both) && !evidence_only) bytes += T * G * 8.0;
    bytes += T * (double)p->seg_len * (double)p->data_dim * 8.0;
    if (om == BLHIP_OM_GAUSSIAN) { if (!s.both) bytes += T * (double)blc::NW * (double)s.strips * 64.0 * 32.0; }
    else bytes += T * G * 8.0;
    return bytes;
}

// two-parameter grids: the envelope of the chain-resident kernels a series fit may take.  What depends on the chains' hyper-parameter
// values (the radius of a walk against the band and the grid) is left to the fit itself, which fails with the reason.
inline int series_check_2d(const blhip_problem *p, int flags, char *err, int errlen) {
    auto no = [&](const char *fmt, auto... a) {
        if (err && errlen > 0) {
            const int k = std::snprintf(err, (size_t)errlen, "a grid of 2 parameters ");
            if constexpr (sizeof...(a) == 0) { if (k > 0 && k < errlen) std::snprintf(err + k, (size_t)(errlen - k), "%s", fmt); }
            else if (k > 0 && k < errlen) std::snprintf(err + k, (size_t)(errlen - k), fmt, a...);
        }
        return 1;
    };
    const long long n0 = p->n[0], n1 = p->n[1];
    const int om = p->obs_model;
    const bool table = om == BLHIP_OM_LAPLACE || om == BLHIP_OM_AR1 || om == BLHIP_OM_SCALED_AR1;
    if (om != BLHIP_OM_GAUSSIAN && !table)
        return no("with observation model %d (series fits take the Gaussian, Laplace, AR1 and ScaledAR1 models there)", om);
    if (flags & BLHIP_SERIES_RAGGED)
        return no("and series of different lengths or time stamps (series fits there take series of one length and one set of time stamps)");
    if (p->seg_len != (om == BLHIP_OM_AR1 || om == BLHIP_OM_SCALED_AR1 ? 2 : 1)) return no("and segment length %d", p->seg_len);
    if (p->data_dim < 1 || (om == BLHIP_OM_GAUSSIAN && p->data_dim > blc::DMAX)) return no("and data dimension %d", p->data_dim);
    if (p->T < 1) return no("and T = %lld", (long long)p->T);
    if (!chain_rows_ok((int)std::min<long long>(n0, 1 << 20)) || (table && n0 > 512))
        return no("with %lld rows (series fits take the chain-resident geometries: %d .. %d rows, table models up to 512)", n0, CHAIN_MIN_ROWS, CHAIN_TALL_ROWS);
    if (n1 < 1 || n1 > (long long)blc::WCOL * blc::MAX_STRIPS)
        return no("with %lld columns (series fits take the chain-resident geometries: 1 .. %d columns)", n1, blc::WCOL * blc::MAX_STRIPS);
    if (p->backward_init) return no("and a backward_init message");
    if (p->n_ops < 0 || (p->n_ops > 0 && !p->ops)) return no("and a bad transition program");
    for (int k = 0; k < p->n_ops; ++k) {
        const int kind = p->ops[k].kind;
        if (kind == BLHIP_OP_REGIMESWITCH || kind == BLHIP_OP_NOTEQUAL)
            return no("and op %d: RegimeSwitch / NotEqual (the clamping chain-resident kernels take no series)", k);
        if (kind != BLHIP_OP_STATIC && kind != BLHIP_OP_GRW && kind != BLHIP_OP_CHANGEPOINT && kind != BLHIP_OP_BREAKPOINT)
            return no("and op %d (kind %d): series fits there take Static, GaussianRandomWalk, ChangePoint and BreakPoint ops", k, kind);
    }
    const Series2dShape s = series_shape_2d(p);
    if (s.both && table) return no("and walks on both parameters of a tabulated model (observation model %d)", om);
    if (s.both && (std::max(n0, n1) > 512 || std::min(n0, n1) < CHAIN_MIN_ROWS))
        return no("of %lld x %lld and walks on both parameters (the both-axes kernels take %d .. 512 rows and columns)", n0, n1, CHAIN_MIN_ROWS);
    // (chain_padding_rule: a padded 1024-row geometry stores on forward passes only -- a full fit of it would be declined after the uploads)
    if (s.pad && s.n0p > 512 && !(flags & (BLHIP_EVIDENCE_ONLY | BLHIP_FORWARD_ONLY)))
        return no("of %lld x %lld, padded inside 1024 rows, and a full fit (the padded 1024-row kernels keep no backward pass's sequence: forwardOnly / evidenceOnly fits only)", n0, n1);
    if (table && !chain_table_geometry_ok((int)s.n0p, s.pad)) return no("with %lld rows, padded, and a tabulated model (no chain-resident kernel)", n0);
    return 0;
}

// 0: the series path admits the problem; 1: it does not, the reason in err.  What depends on the chains' hyper-parameter values -- the
// radius of their walks against the row length and the LDS of a CU -- is left to the fit itself (plan_geometry), which fails with the reason.
inline int series_check(const blhip_problem *p, int64_t S, int flags, char *err, int errlen) {
    auto no = [&](const char *fmt, auto... a) { if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a...); return 1; };
    if (err && errlen > 0) err[0] = 0;
    if (!p) return no("the problem is NULL");
    if (S < 1) return no("%lld series", (long long)S);
    if (flags & (BLHIP_RESUME | BLHIP_CARRY | BLHIP_ACCUMULATE)) return no("BLHIP_RESUME / BLHIP_CARRY / BLHIP_ACCUMULATE do not go with series");
    if (p->ndim == 2) return series_check_2d(p, flags, err, errlen);
    if (p->ndim != 1) return no("a grid of %d parameters (series fits run on one- and two-parameter grids)", p->ndim);
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
// [b * per, min(S, (b + 1) * per)).  At most SERIES_MAX_BATCH chains per batch on a one-parameter grid, SERIES_MAX_BATCH_2D on a
// two-parameter one: the library's defaults for batches on such grids (option max_batch).
constexpr int64_t SERIES_MAX_BATCH = 4096, SERIES_MAX_BATCH_2D = 1024;
inline int series_plan(const blhip_problem *p, int64_t S, int flags, double budget, int64_t *plan_out) {
    if (!plan_out || series_check(p, S, flags, nullptr, 0) != 0 || !(budget >= 0.0)) return -1;
    const double per = series_chain_bytes(p, p->obs_model, (flags & BLHIP_EVIDENCE_ONLY) != 0);
    plan_out[0] = plan_out[1] = plan_out[2] = 0;
    plan_out[3] = (int64_t)std::ceil(per);
    if (budget < (double)plan_out[3]) return 1;
    const int64_t cap = p->ndim == 1 ? SERIES_MAX_BATCH : SERIES_MAX_BATCH_2D;
    int64_t fit = (int64_t)std::min(std::floor(budget / per), 4.0e18);
    // (two-parameter grids: plan_batches cuts batches of 16 and more chains to a multiple of 8 -- whole launches; a batch that keeps its
    //  sequences must be ONE batch of the fit)
    if (p->ndim == 2 && fit >= 16) fit -= fit % 8;
    const int64_t B = std::min<int64_t>(std::min<int64_t>(S, cap), fit);
    plan_out[0] = B;
    plan_out[1] = (S + B - 1) / B;
    plan_out[2] = (int64_t)std::ceil(per * (double)B);
    return 0;
}

// ---- series in groups (blhip_set_series_groups; HyperStudy.fitMany of bayesloop_amd) ------------------------------------------------------
// S series x H chains: chain c observes series c / H with the op values of its own row -- a hyper-study per series, the user's loop
// `for d in series: H.loadData(d); H.fit()` around HyperStudy.fit (reference core.py:1247-1441).  One-parameter grids only.  The chains
// of a group share the series' (T, n) likelihood table (Row1dRun::series_table), and with BLHIP_ACCUMULATE each group is folded into its
// own average (series_group_fold, blhip.hip), which becomes the kept posterior.  H = 1 is blhip_set_series: the rules and the plan above.
inline int series_group_check(const blhip_problem *p, int64_t S, int64_t H, int flags, char *err, int errlen) {
    auto no = [&](const char *fmt, auto... a) { if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a...); return 1; };
    if (err && errlen > 0) err[0] = 0;
    if (H == 1) return series_check(p, S, flags, err, errlen);
    if (!p) return no("the problem is NULL");
    if (H < 1) return no("groups of %lld chains", (long long)H);
    if (p->ndim != 1) return no("a grid of %d parameters (groups of chains per series run on one-parameter grids)", p->ndim);
    if (H > SERIES_MAX_BATCH) return no("groups of %lld chains (a batch of the chain-resident 1-D kernel holds at most %lld)", (long long)H, (long long)SERIES_MAX_BATCH);
    // (BLHIP_ACCUMULATE: the grouped fold, decided by the fit; every other rule is a single chain's)
    return series_check(p, S, flags & ~BLHIP_ACCUMULATE, err, errlen);
}

// Bytes of one group: H chains as series_chain_bytes counts them, less the H - 1 likelihood tables they do not own, plus -- a fit that
// keeps posteriors -- the group's (T, n) average.
inline double series_group_bytes(const blhip_problem *p, int64_t H, bool evidence_only) {
    const double table = (double)p->T * (double)p->n[0] * 8.0;
    return (double)H * series_chain_bytes(p, p->obs_model, evidence_only) - (double)(H - 1) * table + (evidence_only ? 0.0 : table);
}

// plan_out (4 values): groups per batch, batches, bytes of such a batch, the smallest budget accepted (one group).  A batch of a fit that
// keeps posteriors holds WHOLE groups, at most `cap` chains (the 1-D batch cap SERIES_MAX_BATCH, or the caller's smaller option
// max_batch; <= 0: the library's).  0; -1: bad arguments or a problem series_group_check refuses; 1: a group beyond the cap or the budget,
// the reason in err (plan_out[3] is still written) -- the caller runs its loop.  H = 1: series_plan's figures under the same cap.
inline int series_group_plan(const blhip_problem *p, int64_t S, int64_t H, int flags, double budget, int64_t cap, int64_t *plan_out, char *err, int errlen) {
    auto no = [&](const char *fmt, auto... a) { if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a...); return 1; };
    if (err && errlen > 0) err[0] = 0;
    if (!plan_out || series_group_check(p, S, H, flags, nullptr, 0) != 0 || !(budget >= 0.0)) return -1;
    if (cap <= 0 || cap > SERIES_MAX_BATCH) cap = SERIES_MAX_BATCH;
    if (H == 1) {
        const int rc = series_plan(p, S, flags & ~BLHIP_ACCUMULATE, budget, plan_out);
        if (rc == 1) return no("a memory budget of %.0f bytes is below one series (%lld bytes)", budget, (long long)plan_out[3]);
        if (rc == 0 && plan_out[0] > cap) {
            const double per = series_chain_bytes(p, p->obs_model, (flags & BLHIP_EVIDENCE_ONLY) != 0);
            plan_out[0] = cap; plan_out[1] = (S + cap - 1) / cap; plan_out[2] = (int64_t)std::ceil(per * (double)cap);
        }
        return rc;
    }
    const double per = series_group_bytes(p, H, (flags & BLHIP_EVIDENCE_ONLY) != 0);
    plan_out[0] = plan_out[1] = plan_out[2] = 0;
    plan_out[3] = (int64_t)std::ceil(per);
    if (H > cap) return no("a group of %lld chains is beyond the batch cap of %lld chains (option max_batch)", (long long)H, (long long)cap);
    if (budget < (double)plan_out[3]) return no("a memory budget of %.0f bytes is below one group of %lld chains (%lld bytes)", budget, (long long)H, (long long)plan_out[3]);
    const int64_t fit = (int64_t)std::min(std::floor(budget / per), 4.0e18);
    const int64_t Gb = std::min<int64_t>(std::min<int64_t>(S, cap / H), fit);
    plan_out[0] = Gb;
    plan_out[1] = (S + Gb - 1) / Gb;
    plan_out[2] = (int64_t)std::ceil(per * (double)Gb);
    return 0;
}
