// A batch of chains on the device: batch plan and memory plan, shared tables and per-(step, chain) metadata (uploads), which kernel family runs the
// batch (plan_geometry; plan_chainres: blhip_chain_plan.hpp), the average-posterior folds, kept posteriors, carried states (carry_source, upload_unit_sums: also the N-D path's), results.
// Part of libblhip's host side: included by blhip.hip INSIDE its anonymous namespace (one translation unit; the split is by subject, not by linkage).
#pragma once

// normalise the kept posterior rows (core.py:389 / :441) (eagerly at the end of the fit, or on first access with option lazy_normalise)
void ensure_post_scaled(blhip_ctx *ctx) {
    if (!ctx->post_valid || ctx->post_scaled) return;
    HIPCHECK(hipSetDevice(ctx->device));
    const long long G = ctx->post_G;
    const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 4096);
    // (rows [post_row0, post_row1) only: the time-resident kernel has normalised the others itself)
    const int64_t r0 = ctx->post_row0, nrows = ctx->post_row1 - ctx->post_row0;
    // (a series fit keeps thousands of chains of a hundred rows each: a launch per chain was more than half of its kernel time.  The
    //  chains' rows follow each other: every row of every chain in one launch per max_grid_y rows)
    if (ctx->post_series && r0 == 0 && nrows == ctx->post_T && nrows > 0) {
        for_grid_y(ctx, (long long)ctx->post_chains * nrows, [&](long long y0, unsigned ny) {
            BL_LAUNCH(scale_rows_kernel, dim3(gx, ny), dim3(NTHREADS), 0, ctx->stream, ctx->post.as<double>() + (size_t)y0 * G, G, ctx->postinv.as<double>() + y0);
        });
        HIPCHECK(hipGetLastError());
        ctx->post_scaled = true;
        return;
    }
    for (int64_t b = 0; b < ctx->post_chains && nrows > 0; ++b)
        for_grid_y(ctx, nrows, [&](long long y0, unsigned ny) {
            BL_LAUNCH(scale_rows_kernel, dim3(gx, ny), dim3(NTHREADS), 0, ctx->stream,
                               ctx->post.as<double>() + ((size_t)b * ctx->post_T + r0 + y0) * G, G, ctx->postinv.as<double>() + b * ctx->post_T + r0 + y0);
        });
    HIPCHECK(hipGetLastError());
    ctx->post_scaled = true;
}

// axis-0 radius bucket of a chain as bucket_step() will see it (0: no filter, k: radius in (8 (k - 1), 8 k]); -1 if it cannot be told
// from the op values alone
int chain_bucket(const blhip_problem *p, const double *val) {
    int r0 = 0;
    for (int k = 0; k < p->n_ops; ++k) {
        const blhip_op &op = p->ops[k];
        if (op.kind == BLHIP_OP_GRW) {
            if (p->ndim == 2 && op.axis == 0) {
                const double ns = val[k] / p->lattice[0];
                if (!(ns >= 0.0) || ns > 1e6) return -1;
                r0 = std::max(r0, (int)(4.0 * ns + 0.5));
            }
        } else if (op.kind != BLHIP_OP_STATIC) {
            return -1;                               // (other models: their launches are not bucketed by radius)
        }
    }
    return r0 == 0 ? 0 : (r0 + 7) / 8;
}

// -> start index of every batch (+ n_chains at the end): equal shares of at most Bmax chains, each cut moved to the nearest change of
// radius bucket within the slack the memory budget leaves
std::vector<int64_t> plan_batches(const blhip_problem *p, int64_t n_chains, const double *op_values, int64_t Bmax, bool align) {
    // batches of a multiple of 8 chains: whole launches of the chain-resident kernel (8 chains per launch on 512-column grids)
    if (Bmax >= 16) Bmax -= Bmax % 8;
    const int64_t nbatch = (n_chains + Bmax - 1) / Bmax;
    int64_t even = (n_chains + nbatch - 1) / nbatch;
    if (nbatch > 1 && even >= 16) even = std::min(Bmax, (even + 7) / 8 * 8);
    std::vector<int64_t> start;
    for (int64_t c = 0; c < n_chains; c += even) start.push_back(c);
    start.push_back(n_chains);
    if (!align || (int64_t)start.size() != nbatch + 1 || nbatch < 2 || !op_values || p->n_ops == 0) return start;
    std::vector<int> bucket(n_chains);
    for (int64_t c = 0; c < n_chains; ++c) {
        bucket[c] = chain_bucket(p, op_values + c * p->n_ops);
        if (bucket[c] < 0) return start;
    }
    for (int64_t b = 1; b < nbatch; ++b) {
        // candidates: bucket changes between the previous cut and the next one; the batches on both sides must stay <= Bmax
        int64_t best = -1;
        for (int64_t c = start[b - 1] + 1; c < start[b + 1]; ++c) {
            if (bucket[c] == bucket[c - 1]) continue;
            if (c - start[b - 1] > Bmax || start[b + 1] - c > Bmax) continue;
            if (best < 0 || std::llabs(c - start[b]) < std::llabs(best - start[b])) best = c;
        }
        if (best >= 0) start[b] = best;
    }
    return start;
}

// One more cut where the axis-0 radius of a hyper-grid crosses the largest band of the matrix-pipe / chain-resident kernels (40): the
// chains below it keep those kernels, the chains above it take the column pre-pass (blh::vwide_kernel) -- without the cut ONE wide chain
// would route its whole batch through the pre-pass.  Only for grids sorted that way (every chain before the cut <= 40 < every chain after).
void split_wide_axis0(const blhip_problem *p, int64_t n_chains, const double *op_values, std::vector<int64_t> &start, int r_max) {
    if (p->ndim != 2 || !op_values || p->n_ops == 0 || n_chains < 2) return;
    auto radius0 = [&](int64_t c) {
        int r0 = 0;
        for (int k = 0; k < p->n_ops; ++k) {
            const blhip_op &op = p->ops[k];
            if (op.kind == BLHIP_OP_GRW && op.axis == 0) {
                const double ns = op_values[c * p->n_ops + k] / p->lattice[0];
                if (!(ns >= 0.0) || ns > 1e6) return -1;
                r0 = std::max(r0, (int)(4.0 * ns + 0.5));
            }
        }
        return r0;
    };
    int64_t cut = -1;
    for (int64_t c = 0; c < n_chains; ++c) {
        const int r = radius0(c);
        if (r < 0) return;
        if (r > r_max) { if (cut < 0) cut = c; }
        else if (cut >= 0) return;                   // a narrow chain after a wide one: not sorted by radius
    }
    if (cut <= 0) return;
    for (int64_t v : start) if (v == cut) return;
    start.insert(std::upper_bound(start.begin(), start.end(), cut), cut);
}

// ---- the phases of a fit: flags, shared tables (upload), memory plan; then per batch: program, geometry, metadata, forward pass +
//      evidence bookkeeping, backward pass + bookkeeping, carried states / average posterior / kept posterior, results ------------
struct FitFlags {
    bool evidence_only, forward_only, full, keep, accumulate, resume, carry;
};

FitFlags decode_flags(blhip_ctx *ctx, const blhip_problem *p, uint32_t flags, const double *log_w) {
    FitFlags f{};
    f.evidence_only = flags & BLHIP_EVIDENCE_ONLY;
    f.forward_only = (flags & BLHIP_FORWARD_ONLY) && !f.evidence_only;
    f.full = !f.evidence_only && !f.forward_only;
    f.keep = (flags & BLHIP_KEEP_POSTERIOR) && !f.evidence_only;
    f.accumulate = (flags & BLHIP_ACCUMULATE) && !f.evidence_only;
    f.resume = flags & BLHIP_RESUME;
    f.carry = flags & BLHIP_CARRY;
    if (f.resume || f.carry) {
        if (f.full) fail("BLHIP_RESUME / BLHIP_CARRY need a forward-only or evidence-only fit");
        if (p->carry_slot < 0) fail("carry_slot must be >= 0");
    }
    if (f.accumulate && !ctx->acc_active) fail("BLHIP_ACCUMULATE without blhip_accum_begin");
    if (f.accumulate && !log_w) fail("BLHIP_ACCUMULATE needs log_chain_weight");
    return f;
}

// ---- the envelope of the Gaussian likelihood recurrence ----------------------------------------------------------------------------------------
// The recurrence kernels carry the likelihood as mantissa * 2^exponent and add the exponents of the anchor (a0), of the ratio (d1) and of the
// curvature (d2) in `int`, and blmath::exp_mn clamps its argument to +-1.4e9.  Both are harmless only while every argument a kernel can
// form stays small: this bounds |a0| + steps |d1| + steps^2 / 2 |d2| over every record, every std column and every row of the lattice
// continued REC_PAD_ROWS rows beyond either end of the grid (the padded tiles of the resident and chain kernels run the recurrence through
// rows outside the grid), for the longest anchor interval (REC_MAX_STEPS steps of REC_MAX_STRIDE rows).  A fit whose bound exceeds
// REC_ENVELOPE takes the per-cell exponential flavours (exact zeros where the likelihood underflows).  1e9 log2(e) = 1.44e9 < 2^31.
constexpr double REC_ENVELOPE = 1.0e9;
constexpr int REC_PAD_ROWS = 256, REC_MAX_STRIDE = 4, REC_MAX_STEPS = 32;

inline double rec_envelope_bound(const double *m0, int n0, const double *s, int n1, const double *data, int64_t n_rec, int dd) {
    if (n0 < 2 || n1 < 1) return 0.0;
    const double step = std::fabs((m0[n0 - 1] - m0[0]) / (double)(n0 - 1));
    const double lo = std::min(m0[0], m0[n0 - 1]) - REC_PAD_ROWS * step, hi = std::max(m0[0], m0[n0 - 1]) + REC_PAD_ROWS * step;
    double D = 0.0, dn = 0.0;
    for (int64_t t = 0; t < n_rec; ++t) {
        double n = 0.0;
        for (int k = 0; k < dd; ++k) {
            const double x = data[t * dd + k];
            if (x == x) {
                n += 1.0;
                D = std::max(D, std::max(std::fabs(x - lo), std::fabs(x - hi)));
            }
        }
        dn = std::max(dn, n);
    }
    double cA = 0.0, cB = 0.0;
    for (int j = 0; j < n1; ++j) {
        cA = std::max(cA, 1.0 / (2.0 * s[j] * s[j]));
        cB = std::max(cB, std::fabs(0.5 * std::log(2.0 * M_PI * s[j] * s[j])));
    }
    const double H = REC_MAX_STRIDE * step;
    const double b = dn * (D * D * cA + cB) + REC_MAX_STEPS * (2.0 * cA * H * dn * D) + 0.5 * REC_MAX_STEPS * REC_MAX_STEPS * (2.0 * cA * dn * H * H);
    return b == b ? b : INFINITY;          // (a NaN bound -- a zero or NaN std -- is no envelope)
}

// May the fast, resident and chain-resident kernels run the likelihood recurrence along the rows of this grid, and with which row step?
struct RowRecurrence { double step0 = 0.0; bool use_rec = false; };

RowRecurrence plan_recurrence(blhip_ctx *ctx, const blhip_problem *p, int n0, int n1) {
    RowRecurrence rr;
    // likelihood recurrence along rows needs an equally spaced row axis (to rounding)
    const double *m0h = p->marginal[0];
    const double step = (m0h[n0 - 1] - m0h[0]) / (double)(n0 - 1);
    double dev = 0.0, mx = 0.0;
    for (int i = 0; i < n0; ++i) {
        dev = std::max(dev, std::fabs(m0h[i] - (m0h[0] + i * step)));
        mx = std::max(mx, std::fabs(m0h[i]));
    }
    rr.step0 = step;
    rr.use_rec = p->obs_model == BLHIP_OM_GAUSSIAN && dev <= 8.0 * 2.3e-16 * mx && ctx->option("recurrence", 1.0) != 0.0;
    // ... and arguments inside its envelope (exponents are added in int, exp_mn clamps): beyond it the per-cell exponential
    // (series fits: p->data is the (S, T, seg_len, data_dim) block of ALL the call's series -- the bound is over every record of every one)
    const int64_t n_rec = (ctx->series.data ? ctx->series.S : 1) * p->T * p->seg_len;
    if (rr.use_rec && !(rec_envelope_bound(m0h, n0, p->marginal[1], n1, p->data, n_rec, p->data_dim) <= REC_ENVELOPE)) rr.use_rec = false;
    return rr;
}

// ---- BLHIP_OM_PROGRAM: the (T, G) likelihood table from the program the context is armed with (bllp::lik_program_kernel) ---------------------
// d_marginal: the marginal grids on the device, n[k] values each; data: (T, data_dim) on the host; d_lik: (T, G) on the device.  The
// program's arrays, the step values and the data go into one buffer of the context; queued on the context's stream, not waited for.
// step_values: (T, data_dim, n_step) STEP values that go with THIS data instead of the armed ones (the posterior predictive tabulates the
// program for observation values that are no data of the fit); NULL: the armed ones.
void build_program_table(blhip_ctx *ctx, int ndim, const int64_t *n, const double *const *d_marginal, int64_t T, int data_dim,
                         const double *data, double *d_lik, const double *step_values = nullptr) {
    const blhip_ctx::LikProgram &LP = ctx->likprog;
    if (ctx->option("lik_program", 1.0) == 0.0) fail("BLHIP_OM_PROGRAM: option lik_program = 0 keeps the caller-evaluated table (BLHIP_OM_TABLE)");
    if (!LP.armed) fail("BLHIP_OM_PROGRAM: no likelihood program is armed (blhip_set_lik_program)");
    if (ndim < 1 || ndim > bllp::MAX_DIM || T < 1 || data_dim < 1 || !data || !d_lik) fail("BLHIP_OM_PROGRAM: bad grid / data");
    const int64_t n_ops = (int64_t)LP.ops.size() / 2, n_consts = (int64_t)LP.consts.size();
    char msg[256] = "";
    if (bllp::check_program(LP.ops.data(), n_ops, n_consts, LP.n_step, ndim, msg, (int)sizeof msg) != 0) fail("%s", msg);
    const size_t n_stepv = (size_t)(T * data_dim * LP.n_step);
    if (!step_values && (int64_t)LP.step.size() != T * data_dim * LP.n_step)
        fail("BLHIP_OM_PROGRAM: the armed program carries %lld step values, the problem needs (T, data_dim, n_step) = (%lld, %d, %lld)",
             (long long)LP.step.size(), (long long)T, data_dim, (long long)LP.n_step);
    long long G = 1;
    for (int k = 0; k < ndim; ++k) {
        if (n[k] < 1 || n[k] > (1ll << 30) || !d_marginal[k]) fail("BLHIP_OM_PROGRAM: bad grid axis %d", k);
        G *= n[k];
    }
    for (int64_t pc = 0; pc < n_ops; ++pc)           // a tabulated function of one parameter spans that parameter's axis
        if (LP.ops[2 * pc] == bllp::OP_AXIS && (int64_t)(LP.ops[2 * pc + 1] >> 2) + n[LP.ops[2 * pc + 1] & 3] > n_consts)
            fail("BLHIP_OM_PROGRAM: op %lld: AXIS table of parameter %d (%lld values from constant %d) runs past the %lld constants",
                 (long long)pc, LP.ops[2 * pc + 1] & 3, (long long)n[LP.ops[2 * pc + 1] & 3], LP.ops[2 * pc + 1] >> 2, (long long)n_consts);
    hipStream_t st = ctx->stream;
    const size_t nd = (size_t)T * data_dim;
    ctx->likprog_dev.ensure(carve_size(LP.ops.size() * 4) + carve_size(std::max<size_t>(1, LP.consts.size()) * 8) +
                            carve_size(std::max<size_t>(1, n_stepv) * 8) + carve_size(nd * 8));
    char *cur = ctx->likprog_dev.as<char>();
    bllp::Instr *d_ops = carve<bllp::Instr>(cur, (size_t)n_ops);
    double *d_consts = carve<double>(cur, std::max<size_t>(1, LP.consts.size())), *d_step = carve<double>(cur, std::max<size_t>(1, n_stepv)),
           *d_data = carve<double>(cur, nd);
    HIPCHECK(hipMemcpyAsync(d_ops, LP.ops.data(), LP.ops.size() * 4, hipMemcpyHostToDevice, st));
    if (!LP.consts.empty()) HIPCHECK(hipMemcpyAsync(d_consts, LP.consts.data(), LP.consts.size() * 8, hipMemcpyHostToDevice, st));
    if (n_stepv) HIPCHECK(hipMemcpyAsync(d_step, step_values ? step_values : LP.step.data(), n_stepv * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_data, data, nd * 8, hipMemcpyHostToDevice, st));
    bllp::LikProgParams P{};
    P.ops = d_ops; P.consts = d_consts; P.G = G; P.n_ops = (int)n_ops; P.n_step = (int)LP.n_step; P.dd = data_dim; P.ndim = ndim;
    for (int k = 0; k < ndim; ++k) { P.m[k] = d_marginal[k]; P.n[k] = (int)n[k]; }
    const unsigned gx = (unsigned)std::min<long long>((G + bllp::NT - 1) / bllp::NT, 2048);
    for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
        bllp::LikProgParams Q = P;
        Q.step = d_step + (size_t)t0 * data_dim * LP.n_step; Q.data = d_data + (size_t)t0 * data_dim; Q.lik = d_lik + (size_t)t0 * G;
        BL_LAUNCH(bllp::lik_program_kernel, dim3(gx, nt), dim3(bllp::NT), 0, st, Q);
    });
    HIPCHECK(hipGetLastError());
}

// what every chain of the call shares, resident in HBM for the duration of the call
struct DeviceTables {
    double *m0, *m1, *colA, *colB, *rec, *prior, *reset, *uniform, *indep, *lik;
    int rec_len, d;
};

// upload: marginal grids, per-column likelihood constants, per-step data records, prior(s); the (T, G) likelihood table of the
// closed-form table models is built on the device (table_model != 0), a caller-evaluated one (BLHIP_OM_TABLE) is copied
DeviceTables upload_tables(blhip_ctx *ctx, const blhip_problem *p, const Geometry &g, const FitFlags &ff, int table_model) {
    hipStream_t st = ctx->stream;
    const int64_t T = p->T;
    const long long G = g.G;
    DeviceTables D{};
    std::vector<double> rec;
    build_records(p, rec, D.rec_len, D.d);
    std::vector<double> colA(g.n1, 0.0), colB(g.n1, 0.0);
    const double *mcol = p->ndim == 1 ? p->marginal[0] : p->marginal[1];
    if (p->obs_model == BLHIP_OM_GAUSSIAN)
        for (int j = 0; j < g.n1; ++j) {
            const double s = mcol[j];
            colA[j] = 1.0 / (2.0 * s * s);
            colB[j] = 0.5 * std::log(2.0 * M_PI * s * s);
        }
    if (p->obs_model == BLHIP_OM_POISSON)
        for (int j = 0; j < g.n1; ++j) colA[j] = std::exp(-mcol[j]);

    size_t tb = 0;
    tb += carve_size(sizeof(double) * std::max(1, g.n0)) + 3 * carve_size(sizeof(double) * g.n1);
    tb += carve_size(sizeof(double) * rec.size()) + 4 * carve_size(sizeof(double) * G);
    ctx->tables.ensure(tb);
    char *cur = ctx->tables.as<char>();
    D.m0 = carve<double>(cur, std::max(1, g.n0));
    D.m1 = carve<double>(cur, g.n1);
    D.colA = carve<double>(cur, g.n1);
    D.colB = carve<double>(cur, g.n1);
    D.rec = carve<double>(cur, rec.size());
    D.prior = carve<double>(cur, G);
    D.reset = carve<double>(cur, G);
    D.uniform = carve<double>(cur, G);
    D.indep = carve<double>(cur, G);
    if (p->ndim == 2) HIPCHECK(hipMemcpyAsync(D.m0, p->marginal[0], sizeof(double) * g.n0, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(D.m1, mcol, sizeof(double) * g.n1, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(D.colA, colA.data(), sizeof(double) * g.n1, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(D.colB, colB.data(), sizeof(double) * g.n1, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(D.rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, st));
    // (the prior of a study that is fitted again: the caller's token says the content is the one this place already holds)
    const bool prior_resident = p->prior_token != 0 && p->prior_token == ctx->prior_token && D.prior == ctx->prior_dev && G == ctx->prior_G;
    if (!prior_resident) HIPCHECK(hipMemcpyAsync(D.prior, p->prior, sizeof(double) * G, hipMemcpyHostToDevice, st));
    ctx->prior_token = p->prior_token; ctx->prior_dev = D.prior; ctx->prior_G = G;
    if (p->reset_prior) HIPCHECK(hipMemcpyAsync(D.reset, p->reset_prior, sizeof(double) * G, hipMemcpyHostToDevice, st));
    if (p->indep_prior) HIPCHECK(hipMemcpyAsync(D.indep, p->indep_prior, sizeof(double) * G, hipMemcpyHostToDevice, st));
    if (ff.full) {
        // beta_T = 1/G   core.py:424-425 -- or the caller's backward message (blhip_problem.backward_init)
        if (p->backward_init) HIPCHECK(hipMemcpyAsync(D.uniform, p->backward_init, sizeof(double) * G, hipMemcpyHostToDevice, st));
        else BL_LAUNCH(fill_kernel, dim3(256), dim3(256), 0, st, D.uniform, G, 1.0 / (double)G);
    }
    D.lik = nullptr;
    if (p->obs_model == BLHIP_OM_TABLE) {
        ctx->likbuf.ensure(sizeof(double) * T * G);
        D.lik = ctx->likbuf.as<double>();
        if (table_model == BLHIP_OM_PROGRAM) {
            const double *dm[BLHIP_MAX_DIM] = {p->ndim == 2 ? D.m0 : D.m1, D.m1, nullptr, nullptr};
            build_program_table(ctx, p->ndim, p->n, dm, T, p->data_dim, p->data, D.lik);
        } else if (table_model) {
            const size_t nd = (size_t)T * p->seg_len * p->data_dim;
            ctx->databuf.ensure(nd * 8);
            HIPCHECK(hipMemcpyAsync(ctx->databuf.p, p->data, nd * 8, hipMemcpyHostToDevice, st));
            const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 2048);
            for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
                BL_LAUNCH(lik_table_kernel, dim3(gx, nt), dim3(NTHREADS), 0, st, table_model, D.lik + (size_t)t0 * G, (long long)G, g.n1,
                                   p->ndim, D.m0, D.m1, ctx->databuf.as<double>() + (size_t)t0 * p->seg_len * p->data_dim, p->seg_len, p->data_dim);
            });
            HIPCHECK(hipGetLastError());
        } else {
            HIPCHECK(hipMemcpyAsync(D.lik, p->lik, sizeof(double) * T * G, hipMemcpyHostToDevice, st));
        }
    }
    sync_stream(ctx, st);   // the host vectors above go out of use
    return D;
}

// memory plan: how many chains fit one batch (state ping-pong + the stored sequence + partial sums per chain within the budget)
// (the rows the chain-resident kernels take: CHAIN_MIN_ROWS .. CHAIN_TALL_ROWS, blhip_chain_plan.hpp)
static_assert(blo::PAD_ROWS_MIN == CHAIN_MIN_ROWS && blo::PAD_ROWS_MAX == CHAIN_TALL_ROWS && blo::PAD_COLS == blc::WCOL && blo::PAD_ROWS == 128,
              "blo::online_block_plan counts a chain's cells as chains_per_batch does");

// BLHIP_RESUME: the carried states the call continues, (n_chains, G) on the device; refused unless the slot holds that shape
const double *carry_source(blhip_ctx *ctx, const blhip_problem *p, int64_t n_chains, long long G) {
    auto it = ctx->carry.find(p->carry_slot);
    if (it == ctx->carry.end() || !it->second.valid) fail("BLHIP_RESUME: carry slot %d holds no state", p->carry_slot);
    if (it->second.chains != n_chains || it->second.G != G)
        fail("BLHIP_RESUME: carry slot %d holds %lld chains x %lld cells, the call has %lld x %lld", p->carry_slot,
             (long long)it->second.chains, (long long)it->second.G, (long long)n_chains, (long long)G);
    return it->second.buf.as<double>();
}

// BLHIP_RESUME: the carried states are normalised -- the "partial sums of the step before" step 0, [B][NRED][nblk], add up to 1 in every
// slot.  slot6_max: slot 6 is the maximum of the carried state (1-D / 2-D: NotEqual inverts around it; N-D: a sum like the others)
const double *upload_unit_sums(blhip_ctx *ctx, const blhip_problem *p, hipStream_t st, int64_t B, int nblk, bool slot6_max) {
    std::vector<double> unit((size_t)B * NRED * nblk, 0.0);
    const std::vector<double> &mv = ctx->carry[p->carry_slot].maxv;
    for (int64_t b = 0; b < B; ++b)
        for (int k = 0; k < NRED; ++k)
            unit[((size_t)b * NRED + k) * nblk] = (k == 6 && slot6_max && (int64_t)mv.size() == B) ? mv[b] : 1.0;
    ctx->unit.ensure(unit.size() * 8);
    HIPCHECK(hipMemcpyAsync(ctx->unit.p, unit.data(), unit.size() * 8, hipMemcpyHostToDevice, st));
    sync_stream(ctx, st);
    return ctx->unit.as<double>();
}

int64_t chains_per_batch(blhip_ctx *ctx, const blhip_problem *p, const Geometry &g, const FitFlags &ff, int64_t n_chains) {
    const int64_t T = p->T;
    const long long G = g.G;
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    // (every reusable buffer of the context counts as available, so that the plan -- and with it the buffer sizes -- is the same from
    //  fit to fit: a plan that changed between two fits of one study re-allocated the 100-GB sequence buffer, 5 s)
    double budget = std::min((double)free_b + (double)ctx->state.cap + (double)ctx->post.cap + (double)ctx->accpart.cap,
                             ctx->option("mem_budget_bytes", 0.70 * (double)total_b)) * 0.9;
    // the chain-resident kernels lay their sequences out on a padded geometry (rows 128 / 256 / 512, columns a multiple of 16)
    double Gk = (double)G;
    // (rows to the next multiple of 128 -- also for 513 .. 896 rows, which the kernels lay out on 1024: the figure every fit's batches
    //  have been cut with; chain_geometry, the planner's rule, would change the batch sizes of existing fits on such grids.  Series fits
    //  do not read it: series_chain_bytes below counts with chain_geometry)
    if (p->ndim == 2 && chain_rows_ok(g.n0))
        Gk = (double)((g.n0 + 127) / 128 * 128) * (double)((g.n1 + blc::WCOL - 1) / blc::WCOL * blc::WCOL);
    {   // walks on both parameters: the transposing kernels lay their sequences out on a SQUARE geometry (blhip_chainax.hpp)
        bool w0 = false, w1 = false;
        for (int k = 0; k < p->n_ops; ++k)
            if (p->ops[k].kind == BLHIP_OP_GRW) { if (g.axis_map[p->ops[k].axis] == 0) w0 = true; else w1 = true; }
        if (p->ndim == 2 && w0 && w1 && std::max(g.n0, g.n1) <= 512) {
            const double n = (double)chain_square_side(g.n0, g.n1);
            Gk = std::max(Gk, n * n);
        }
    }
    // the partial accumulators of the fused fold (ChainRun::fold_buffers: one (T, G) slot per block column of a launch) come out of the same memory
    // -- only where the chain-resident path can be taken at all (else they are never allocated: a narrow grid with a long series
    //    gave up its whole budget to 128 slots it never used and ran one chain per batch), and never more than half of the budget
    if (ff.accumulate && ff.full && p->ndim == 2 && p->obs_model == BLHIP_OM_GAUSSIAN && chain_rows_ok(g.n0) &&
        g.n1 >= 1 && g.n1 <= 16 * blc::MAX_STRIPS && ctx->option("chain_resident", 1.0) != 0.0 && ctx->resident.ok) {
        const double slots = std::max(1, std::min(ctx->num_cus, 256) / ((g.n1 + blc::WCOL - 1) / blc::WCOL));
        budget -= std::min(0.5 * budget, std::min<double>(slots, (double)n_chains) * (double)T * Gk * 8.0);
    }
    // (series fits: + the chain's own (T, n) likelihood table -- series_chain_bytes, the figure blhip_host_series_plan counts with)
    const double per_chain = ctx->series.data ? series_chain_bytes(p, ctx->series.om, ff.evidence_only)
                                              : (ff.evidence_only ? 2.0 : (double)T + 2.0) * Gk * 8.0 + (double)T * NRED * 8.0 * 2 * 64.0 /*partials, rough*/;
    int64_t Bmax = (int64_t)std::max(1.0, std::floor(budget / per_chain));
    // (1-D grids: a chain is a few KB and a batch of the chain-resident 1-D kernel costs a fixed ~1 ms of launches, syncs and read-backs --
    //  the reference's published break-point study, 23 400 chains: 61 ms with batches of 1024, 52 with 4096, 54 with 8192)
    Bmax = std::min<int64_t>(Bmax, (int64_t)ctx->option("max_batch", p->ndim == 1 ? 4096 : 1024));
    Bmax = std::min<int64_t>(Bmax, 65535);
    if (ff.keep && n_chains > Bmax) fail("BLHIP_KEEP_POSTERIOR: %lld chains do not fit in device memory at once", (long long)n_chains);
    if ((ff.resume || ff.carry) && n_chains > Bmax) fail("carried states: %lld chains do not fit in one batch", (long long)n_chains);
    if (ff.resume) (void)carry_source(ctx, p, n_chains, G);
    return Bmax;
}

// ---- batches: at most Bmax chains each, cut where the axis-0 radius bucket changes.  A bucket cut by a batch boundary becomes
//      two under-filled launches per step (round 1: the 107-chain radius-24 bucket of the C4 study ran as 36 + 71 chains at
//      4.1 TB/s); hyper-grids are usually monotone in the random-walk width, so contiguous cuts suffice.
// -> batch_start: batch b holds the chains [batch_start[b], batch_start[b + 1])
std::vector<int64_t> plan_fit_batches(blhip_ctx *ctx, const blhip_problem *p, const Geometry &g, const FitFlags &ff, int64_t n_chains,
                                      const double *op_values) {
    const int64_t Bmax = chains_per_batch(ctx, p, g, ff, n_chains);
    // (cuts on radius-bucket boundaries serve the launch-per-step kernels; grids the chain-resident kernel takes keep whole launches)
    const bool chain_shape = p->ndim == 2 && (p->obs_model == BLHIP_OM_GAUSSIAN || (p->obs_model == BLHIP_OM_TABLE && g.n0 <= 512)) && chain_rows_ok(g.n0) && g.n1 <= 16 * blc::MAX_STRIPS &&
                             ctx->option("chain_resident", 1.0) != 0.0 && ctx->resident.ok;
    std::vector<int64_t> batch_start = plan_batches(p, n_chains, op_values, Bmax, !chain_shape);
    // (the cut: 40; grids the chain-resident kernels take: 80)
    const bool chain_wide = chain_shape && p->obs_model == BLHIP_OM_GAUSSIAN && ctx->option("chain_wide", 1.0) != 0.0;
    if (!ff.keep && !ff.resume && !ff.carry && ctx->option("wide_v", 1.0) != 0.0)
        split_wide_axis0(p, n_chains, op_values, batch_start, chain_wide ? CHAIN_R0_MAX : FAST_R0_MAX);
    // Batches of thousands of chains (1-D studies: the published break-point study runs 6 x 3900): the per-(step, chain) program of batch
    // bi + 1 is built by a second host thread while batch bi runs -- all but the FIRST one's, 3.9 ms of a 42-ms fit with the GPU idle.  A
    // short first batch (1024 chains: 0.7 ms of program) starts the pipeline earlier.
    if (batch_start.size() >= 2 && batch_start[1] - batch_start[0] >= 2048 && !ff.keep && !ff.resume && !ff.carry &&
        ctx->option("short_first_batch", 1.0) != 0.0)
        batch_start.insert(batch_start.begin() + 1, batch_start[0] + 1024);
    return batch_start;
}

// which kernel family runs a batch and with what block geometry (segment lengths from a small cost model: long segments read every
// element once + 2 R0 halo rows per segment, short ones give enough blocks to fill 256 CUs when there are few chains)
struct GeometryPlan {
    bool shift1d = false;        // the chain-resident 1-D kernel's flavours with spline shifts (Deterministic steps) / clamps (RegimeSwitch, NotEqual)
    bool clamp1d = false;        // ... the one with clamps (CL = 2)
    bool fast = false, fused1d = false, use_mfma = false;
    bool fast_but_clamp = false;  // fast in everything but ChainProgram::has_clamp, with a walk on the first parameter only (blc::chain_clamp_kernel's candidates)
    bool chain1d = false;         // 1-D batches: one block per chain runs the whole pass (blhip_chain1d.hpp); bookkeeping of a K = 1 fused pass
    bool wideH = false;           // axis-1 walks wider than the fused kernels' halo: row filter as a pre-pass per step (blhip_hwide.hpp)
    bool wideV = false;           // axis-0 walks wider than the matrix-pipe kernels' largest band: column filter as a pre-pass, no stencil left
    bool hSplit = false;          // wideH: chains of the batch whose axis-1 filter is absent (or narrow: hFusedMax > 0) keep their fused kernels
    int hFusedMax = 0;
    int64_t fusedK = 1;
    int f1_TJ = 128;
    Tile tile{};
    int fastS = 0, fast_nseg = 1, fast_fnblk = 1, mS = 0, m_nseg = 1, m_tiles_j = 1, m_nblk = 1;
};

GeometryPlan plan_geometry(blhip_ctx *ctx, const blhip_problem *p, const Geometry &g, const ChainProgram &prog, int64_t B, int d,
                       bool resume, bool carry, const TapTable *taps = nullptr) {
    GeometryPlan gp;
    const int64_t T = p->T;
    // fast path (blhip_fast.hpp) when the whole batch qualifies, otherwise the generic LDS-tile kernel
    const bool wide_h_ok = prog.LW1 <= blh::HW_MAX && prog.LW1 < g.n1 && ctx->option("wide_h", 1.0) != 0.0;
    const bool wide_v = prog.LW0 > FAST_R0_MAX && prog.LW0 <= blh::VW_MAX && prog.LW0 < g.n0 && wide_h_ok && ctx->option("wide_v", 1.0) != 0.0;
    gp.fast = p->ndim == 2 && (p->obs_model == BLHIP_OM_GAUSSIAN || p->obs_model == BLHIP_OM_TABLE) &&
                      ctx->option("fast", 1.0) != 0.0 && !prog.has_clamp && (prog.LW0 <= FAST_R0_MAX || wide_v) &&
                      (prog.LW1 <= blf::R1MAX || wide_h_ok) &&
                      g.n0 >= (wide_v ? 0 : ((prog.LW0 + 7) / 8) * 8) + 2 * blf::CH && g.n1 >= 2 * blf::R1MAX && d <= blf::DMAX;
    gp.fast_but_clamp = p->ndim == 2 && p->obs_model == BLHIP_OM_GAUSSIAN && ctx->option("fast", 1.0) != 0.0 && prog.has_clamp &&
                        prog.LW0 <= FAST_R0_MAX && prog.LW1 == 0 && g.n0 >= ((prog.LW0 + 7) / 8) * 8 + 2 * blf::CH && g.n1 >= 2 * blf::R1MAX && d <= blf::DMAX;
    gp.wideV = gp.fast && wide_v;
    gp.wideH = gp.fast && (prog.LW1 > blf::R1MAX || (gp.wideV && prog.LW1 > 0));       // (with a column pre-pass every filter runs as a pre-pass)
    // Chains of such a batch WITHOUT an axis-1 filter (a hyper-grid that includes the width 0) skip the pre-pass: it would be a copy.
    // wide_h_fused_max = 8: chains with a narrow filter keep the fused kernels' own axis-1 part as well -- 15 % fewer bytes on
    // extra.c4_both_axes but no faster (the fused both-axes kernels at radii up to 40 are bound by the fp64 pipe: 5.44e10 -> 5.47e10), so
    // the default sends every filter through the pre-pass.
    bool any_narrow = false;
    gp.hFusedMax = std::min(blf::R1MAX, std::max(0, (int)ctx->option("wide_h_fused_max", 0.0)));
    if (gp.wideH && !gp.wideV && taps && ctx->option("wide_h_split", 1.0) != 0.0) {
        bool any_none = false;
        for (size_t e = 0; e < prog.tapF1.size() && !(any_narrow && any_none); ++e) {
            const int k = prog.tapF1[e];
            if (k < 0) any_none = true; else if (gp.hFusedMax > 0 && taps->lw[k] <= gp.hFusedMax) any_narrow = true;
        }
        gp.hSplit = any_narrow || any_none;
    }
    // (programs whose only clamp mode is a Deterministic model's spline shift: the chain-resident kernel has a flavour for them
    //  -- bl1c::chain1d_kernel SHIFT --, the K-steps-per-launch and persistent kernels have not: chain1d or the generic kernel)
    // (round 6: ... and the one with the clamps of RegimeSwitch / NotEqual -- bl1c::chain1d_kernel CL = 2; the dense zero-boundary kernels of
    //  the AlphaStable walk keep the generic kernel)
    // (composed transitions -- ChainProgram::multi -- run on the launch-per-step generic kernel only: has_clamp keeps them off the fast paths,
    //  the condition below off the 1-D ones)
    const bool shift1d = p->ndim == 1 && prog.has_clamp && !prog.dense_clamp && ctx->option("chain1d_shift", 1.0) != 0.0 &&
                         (!prog.other_clamp || ctx->option("chain1d_clamp", 1.0) != 0.0);
    if (p->ndim == 1 && !gp.fast && !prog.multi && (!prog.has_clamp || shift1d) && ctx->option("fuse1d", 8.0) >= 1.0 &&
        (p->obs_model == BLHIP_OM_POISSON || p->obs_model == BLHIP_OM_GAUSSIAN_MEAN || p->obs_model == BLHIP_OM_TABLE)) {
        gp.f1_TJ = 128;
        gp.fusedK = std::max<int64_t>(1, std::min<int64_t>((int64_t)ctx->option("fuse1d", 8.0), T));
        // keep the redundantly recomputed halo (K * LW cells per side) within ~4x the owned cells and the window in LDS
        while (gp.fusedK > 1 && (gp.fusedK * prog.LW1 > 2 * gp.f1_TJ || (size_t)(gp.f1_TJ + 2 * gp.fusedK * prog.LW1) * 32 > 96 * 1024)) --gp.fusedK;
        gp.fused1d = (size_t)(gp.f1_TJ + 2 * gp.fusedK * prog.LW1) * 32 + (size_t)gp.fusedK * gp.f1_TJ * 32 + 4096 <= 150 * 1024;
        // Batches of chains: one block per chain for the whole pass when that is cheaper per step than the alternatives.  Per step
        // (shader cycles; measured with tools/probe.py chain1d, profiles/r04_notes.md): the chain's row is filtered out of ONE CU's LDS --
        // n (2 lw + 1) 16-byte operand pairs at 128 B per clock, ~1 k cycles of barrier / sums / likelihood -- and ceil(B / CUs) blocks
        // share a CU one after the other; the K-steps-per-launch path costs a launch (~14 k cycles) every K steps, the persistent
        // one (all blocks of all chains on the chip at once) ~4 k (K > 1) / ~7 k (K = 1: a hand-off per step) per step.
        const double c1d_mode = ctx->option("chain1d", 1.0);
        if (shift1d) gp.fused1d = true;              // (decided below: without the chain-resident kernel the batch keeps the generic one)
        // (rows of bl1c::NMAX + 1 .. NMAX_LONG cells: the long-row flavour and its lean LDS layout -- option chain1d_long; shorter rows are
        //  decided by the layout of their own kernel, also where only the lean one would fit them)
        const bool long_row = g.n1 > bl1c::NMAX;
        const bool c1d_fits = long_row ? g.n1 <= bl1c::NMAX_LONG && ctx->option("chain1d_long", 1.0) != 0.0 &&
                                             bl1c::lds_doubles_long(g.n1, prog.LW1, shift1d) * 8 <= 150 * 1024
                                       : bl1c::lds_doubles(g.n1, prog.LW1, shift1d) * 8 <= 150 * 1024;
        // (resumed / carried fits -- blocks of an online study: the forward flavours without clamp stages read step 0 from the carried states
        //  and leave the last step's row where store_carry takes it; T >= 2 only, so that every one-step call keeps the route it had)
        const bool c1d_stream_ok = (!resume && !carry) || (T >= 2 && !shift1d);
        if (gp.fused1d && c1d_mode != 0.0 && c1d_stream_ok && prog.LW1 < g.n1 && c1d_fits) {
            // microseconds per time step of the whole batch, fitted to tools/probe.py chain1d (profiles/r04_notes.md): a block's step =
            // 1.5 us + 1.0 ns per cell (likelihood from the shared table; 2.2 ns with Poisson's pow() in the kernel) + 44 ps per cell and
            // tap (the stencil's operand pairs come out of ONE CU's LDS at ~9 per clock), blocks beyond the chip's capacity queue up;
            // persistent K-step kernel (all blocks of all chains on the chip at once) 1.7 us + 40 ns per cell of radius; a launch per K
            // steps 1.5 us + (29 + 0.63 radius) ps per cell of the batch
            const int cus = std::min(ctx->num_cus, 256);
            const double n = g.n1, lw = prog.LW1;
            // (rows longer than a block: two cells per thread share their operand pairs, 21 ps per cell and tap -- launch_chain1d)
            const double tap_us = g.n1 > bl1c::NT && true ? 2.1e-5 : 4.4e-5;
            // (long rows, refitted to 18 shapes of 4608 / 8192 cells -- profiles/chain1d_long_notes.md: 1.4 us + 0.82 ns per cell, always from
            //  the table, + 19.3 ps per cell and tap; the constants above over-estimated those by up to 54 %)
            const double est_c1d = long_row ? (double)((B + cus - 1) / cus) * (1.4 + n * 0.00082 + n * (2.0 * lw + 1.0) * 1.93e-5)
                                            : (double)((B + cus - 1) / cus) * (1.5 + n * (B >= 4 ? 0.0010 : 0.0022) + n * (2.0 * lw + 1.0) * tap_us);
            const int nblk_f = (g.n1 + gp.f1_TJ - 1) / gp.f1_TJ;
            const bool p1d_ok = ctx->option("persist1d", 1.0) != 0.0 && (long long)nblk_f * B <= cus && T > gp.fusedK;
            const double est_other = p1d_ok ? 1.7 + 0.04 * lw : 1.5 + (double)B * n * (29.0 + 0.63 * lw) * 1e-6;
            // (shift1d: the alternative is a launch per step.  A single chain takes the kernel too when the model says so -- rows of a few
            //  hundred cells with a narrow stencil: 200 cells, radius 27: 2.4 against 2.8 us per step)
            // (clamps without a Deterministic model -- the reference's regime-switch tutorial is ONE such chain: a step of a few hundred cells
            //  costs the block ~2 us against a launch of the generic kernel)
            // (series fits -- blhip_set_series -- have no other kernel: the cost model does not apply, the envelope above does)
            gp.chain1d = ctx->series.data != nullptr || c1d_mode == 2.0 || (shift1d && (B >= 2 || !prog.has_shift)) || (!shift1d && est_c1d < est_other);
            if (gp.chain1d) { gp.fusedK = 1; gp.f1_TJ = g.n1; }
        }
        if (shift1d && !gp.chain1d) gp.fused1d = false;
        gp.shift1d = shift1d && gp.chain1d;
        gp.clamp1d = gp.shift1d && prog.other_clamp;
    }
    if (gp.fast) {
        gp.tile.TI = blf::CH; gp.tile.LW0 = gp.wideV ? 0 : prog.LW0; gp.tile.LW1 = (prog.LW1 > 0 && (!gp.wideH || (gp.hSplit && any_narrow))) ? blf::R1MAX : 0;
        gp.tile.TJ = blf::BW - 2 * gp.tile.LW1;
        gp.tile.tiles_j = (g.n1 + gp.tile.TJ - 1) / gp.tile.TJ;
        // rows per block segment: long segments read every element once (+ 2*R0 halo rows per segment), short ones
        // give enough blocks to fill 256 CUs when there are few chains.  Model: cost = waves * blocks_per_CU * rows.
        const long long colblocks = (long long)gp.tile.tiles_j * B;
        const int R0 = (prog.LW0 == 0 || gp.wideV) ? 0 : ((prog.LW0 + 7) / 8) * 8;
        double best = 1e300;
        const int forceS = (int)ctx->option("fast_S", 0);
        for (int k = 1; k <= 4; k *= 2) {
            const double pen = k == 1 ? 1.6 : (k == 2 ? 1.15 : 1.0);
            for (int ns = 1; ns <= std::max(1, g.n0 / 16); ++ns) {
                int S = ((g.n0 + ns - 1) / ns + blf::CH - 1) / blf::CH * blf::CH;
                const int real = (g.n0 + S - 1) / S;
                const long long blocks = colblocks * real;
                const long long waves = (blocks + 256LL * k - 1) / (256LL * k);
                const double cost = pen * (double)waves * k * (S + 2.0 * R0 + 4.0);
                if (cost < best - 1e-9) { best = cost; gp.fastS = S; gp.fast_nseg = real; }
            }
        }
        if (forceS > 0) { gp.fastS = (forceS + blf::CH - 1) / blf::CH * blf::CH; gp.fast_nseg = (g.n0 + gp.fastS - 1) / gp.fastS; }
        gp.tile.tiles_i = gp.fast_nseg;
        gp.fast_fnblk = gp.tile.tiles_j * gp.fast_nseg;
        // geometry of the matrix-pipe kernel (64-column strips, segments of mS rows, mS a multiple of 16)
        {
            gp.m_tiles_j = (g.n1 + blm::BCOL - 1) / blm::BCOL;
            const long long mcol = (long long)gp.m_tiles_j * B;
            double mbest = 1e300;
            for (int k = 1; k <= 4; ++k) {                     // resident blocks per CU
                const double pen = k == 1 ? 1.5 : (k == 2 ? 1.15 : 1.0);
                for (int ns = 1; ns <= std::max(1, g.n0 / 32); ++ns) {
                    int S = ((g.n0 + ns - 1) / ns + blm::SEG_Q - 1) / blm::SEG_Q * blm::SEG_Q;
                    if (S > blm::MS_MAX) continue;
                    const int real = (g.n0 + S - 1) / S;
                    const long long blocks = mcol * real;
                    const long long waves = (blocks + 256LL * k - 1) / (256LL * k);
                    const double cost = pen * (double)waves * k * (S + 1.0 * R0 + 24.0);
                    if (cost < mbest - 1e-9) { mbest = cost; gp.mS = S; gp.m_nseg = real; }
                }
            }
            const int forceM = (int)ctx->option("mfma_S", 0);
            if (forceM > 0) { gp.mS = std::min(blm::MS_MAX, (forceM + blm::SEG_Q - 1) / blm::SEG_Q * blm::SEG_Q); gp.m_nseg = (g.n0 + gp.mS - 1) / gp.mS; }
            if (gp.mS == 0) { gp.mS = blm::MS_MAX; gp.m_nseg = (g.n0 + gp.mS - 1) / gp.mS; }
            gp.m_nblk = gp.m_tiles_j * gp.m_nseg;
        }
        gp.use_mfma = ctx->option("mfma", 1.0) != 0.0;
        gp.tile.nblk = gp.use_mfma ? std::max(gp.fast_fnblk, gp.m_nblk) : gp.fast_fnblk;
        gp.tile.lds_bytes = 0;
    } else if (gp.fused1d) {
        gp.tile.TI = 1; gp.tile.TJ = gp.f1_TJ; gp.tile.LW0 = 0; gp.tile.LW1 = prog.LW1; gp.tile.tiles_i = 1;
        gp.tile.tiles_j = (g.n1 + gp.f1_TJ - 1) / gp.f1_TJ; gp.tile.nblk = gp.tile.tiles_j; gp.tile.lds_bytes = 0;
    } else {
        gp.tile = choose_tile(ctx, g, prog.LW0, prog.LW1, prog.whole_row);
        if (prog.whole_row && gp.tile.tiles_j != 1) fail("internal: a two-stage spline shift needs the whole row in one tile");
    }
    return gp;
}

// per-(step, chain) metadata of a batch in HBM: source kinds, tap-set ids, clamp modes, the per-step launch order of the radius buckets,
// the tap table; plus scratch the finalisation kernels use
struct DeviceMeta {
    unsigned char *kindF, *kindB, *cmodeF, *cmodeB;
    double *limitF, *limitB;
    int *tapF0, *tapF1, *tapB0, *tapB1, *orderF, *orderB;
    double *taps;
    int *off, *lw, *lw2;
    double *invN, *w, *dump;
    // host copies the launch loop reads
    std::vector<int> h_orderF, h_orderB;
    std::vector<std::vector<FastRange>> rangesF, rangesB;
};

void upload_metadata(blhip_ctx *ctx, const blhip_problem *p, const ChainProgram &prog, TapTable &taps, int64_t B, bool full, bool fast, int nblk,
                     DeviceMeta &M, bool wideH = false, bool wideV = false, bool h_split = false, int h_fused_max = 0) {
    hipStream_t st = ctx->stream;
    const int64_t T = p->T;
    const size_t nT = (size_t)T * B;
    taps.w.resize(taps.w.size() + 64, 0.0);      // zero padding: the fast kernels read up to R0 weights per tap set
    size_t mb = 4 * carve_size(nT) + 6 * carve_size(nT * sizeof(int)) + carve_size(taps.w.size() * 8 + 8) +
                3 * carve_size(taps.off.size() * 4 + 4) + 4 * carve_size(sizeof(double) * nT) + carve_size(8 * B) + carve_size(8 * 4 * NTHREADS);
    ctx->meta.ensure(mb);
    char *cur = ctx->meta.as<char>();
    M.kindF = carve<unsigned char>(cur, nT); M.kindB = carve<unsigned char>(cur, nT);
    M.cmodeF = carve<unsigned char>(cur, nT); M.cmodeB = carve<unsigned char>(cur, nT);
    M.limitF = carve<double>(cur, nT); M.limitB = carve<double>(cur, nT);
    M.tapF0 = carve<int>(cur, nT); M.tapF1 = carve<int>(cur, nT);
    M.tapB0 = carve<int>(cur, nT); M.tapB1 = carve<int>(cur, nT);
    M.orderF = carve<int>(cur, nT); M.orderB = carve<int>(cur, nT);
    M.taps = carve<double>(cur, taps.w.size() + 1);
    M.off = carve<int>(cur, taps.off.size() + 1); M.lw = carve<int>(cur, taps.off.size() + 1);
    M.lw2 = carve<int>(cur, taps.off.size() + 1);
    M.invN = carve<double>(cur, nT);
    (void)carve<double>(cur, nT);
    M.w = carve<double>(cur, B);
    M.dump = carve<double>(cur, 4 * NTHREADS);   // (the halo wave of an H block spreads its dummy stores over 8 x 64 slots)
    HIPCHECK(hipMemcpyAsync(M.kindF, prog.kindF.data(), nT, hipMemcpyHostToDevice, st));
    // (what a batch does not use is not copied: on 1-D grids every walk acts on the internal column axis -- the row-axis tap ids are all -1, a
    //  memset --, and the clamp levels exist only for RegimeSwitch / NotEqual: the published break-point study, 23 400 chains x 41 steps with
    //  Deterministic shifts only, uploaded 6.7 MB of metadata per batch from pageable memory, 0.9 ms each, 2.7 MB of it zeros)
    const bool one_d = p->ndim == 1;
    if (one_d) HIPCHECK(hipMemsetAsync(M.tapF0, 0xFF, nT * 4, st));
    else HIPCHECK(hipMemcpyAsync(M.tapF0, prog.tapF0.data(), nT * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(M.tapF1, prog.tapF1.data(), nT * 4, hipMemcpyHostToDevice, st));
    if (prog.has_clamp) {
        HIPCHECK(hipMemcpyAsync(M.cmodeF, prog.cmodeF.data(), nT, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.cmodeB, prog.cmodeB.data(), nT, hipMemcpyHostToDevice, st));
        if (prog.other_clamp) {
            HIPCHECK(hipMemcpyAsync(M.limitF, prog.limitF.data(), nT * 8, hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(M.limitB, prog.limitB.data(), nT * 8, hipMemcpyHostToDevice, st));
        } else {
            HIPCHECK(hipMemsetAsync(M.limitF, 0, nT * 8, st));
            HIPCHECK(hipMemsetAsync(M.limitB, 0, nT * 8, st));
        }
    }
    if (full) {
        HIPCHECK(hipMemcpyAsync(M.kindB, prog.kindB.data(), nT, hipMemcpyHostToDevice, st));
        if (one_d) HIPCHECK(hipMemsetAsync(M.tapB0, 0xFF, nT * 4, st));
        else HIPCHECK(hipMemcpyAsync(M.tapB0, prog.tapB0.data(), nT * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.tapB1, prog.tapB1.data(), nT * 4, hipMemcpyHostToDevice, st));
    }
    if (fast) {
        // a launch with fewer than ~128 blocks leaves most of the 256 CUs idle: a radius bucket with fewer blocks joins the next one
        const long long min_blocks = 128;
        const int min_chains = (int)std::min<long long>(B, (min_blocks + (long long)nblk - 1) / nblk);
        // (wideH: the axis-1 filters wider than the fused kernels' 8 columns run in the pre-pass, and the fused kernels of those chains are
        //  launched without an axis-1 part; chains of the same step with a narrow filter or none keep their fused kernels -- unless the
        //  step also has the axis-0 pre-pass, or with wide_h_split = 0: then every chain of the step goes through the pre-pass)
        const std::vector<int> no_h((wideH || wideV) ? (size_t)B : 0, -1);
        auto all_pre = [&](std::vector<FastRange> &rs) { if (wideH && !h_split) for (auto &r : rs) r.pre = true; };
        M.h_orderF.resize(nT); M.rangesF.resize(T);
        for (int64_t t = 0; t < T; ++t) {
            bucket_step(wideV ? no_h.data() : &prog.tapF0[t * B], (wideH && !h_split) ? no_h.data() : &prog.tapF1[t * B], taps.lw, (int)B, &M.h_orderF[t * B], M.rangesF[t], min_chains,
                        h_split ? h_fused_max : -1);
            all_pre(M.rangesF[t]);
        }
        HIPCHECK(hipMemcpyAsync(M.orderF, M.h_orderF.data(), nT * 4, hipMemcpyHostToDevice, st));
        if (full) {
            M.h_orderB.resize(nT); M.rangesB.resize(T);
            for (int64_t t = 0; t < T; ++t) {
                bucket_step(wideV ? no_h.data() : &prog.tapB0[t * B], (wideH && !h_split) ? no_h.data() : &prog.tapB1[t * B], taps.lw, (int)B, &M.h_orderB[t * B], M.rangesB[t], min_chains,
                            h_split ? h_fused_max : -1);
                all_pre(M.rangesB[t]);
            }
            HIPCHECK(hipMemcpyAsync(M.orderB, M.h_orderB.data(), nT * 4, hipMemcpyHostToDevice, st));
        }
    }
    if (!taps.w.empty()) {
        HIPCHECK(hipMemcpyAsync(M.taps, taps.w.data(), taps.w.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.off, taps.off.data(), taps.off.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.lw, taps.lw.data(), taps.lw.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(M.lw2, taps.lw2.data(), taps.lw2.size() * 4, hipMemcpyHostToDevice, st));
    }
}

// the stages of composed transitions (ChainProgram::multi) in HBM: per direction, per (step, stage, chain) source kind, tap ids, clamp mode
// and level (pre[off[t] + s B + b]); plus the two ping-pong stage outputs of a step (B x G each) and their partials (B x NRED x nblk each)
struct StageMeta {
    unsigned char *kindF = nullptr, *kindB = nullptr, *cmodeF = nullptr, *cmodeB = nullptr;
    int *tapF0 = nullptr, *tapF1 = nullptr, *tapB0 = nullptr, *tapB1 = nullptr;
    double *limitF = nullptr, *limitB = nullptr;
    double *out[2] = {nullptr, nullptr}, *ps[2] = {nullptr, nullptr};
};

void upload_stages(blhip_ctx *ctx, const ChainProgram &prog, int64_t B, long long G, int nblk, bool full, StageMeta &S) {
    hipStream_t st = ctx->stream;
    const size_t nF = prog.preF.size(), nB = full ? prog.preB.size() : 0;
    const size_t n1 = std::max<size_t>(std::max(nF, nB), 1);
    const size_t mb = 2 * (2 * carve_size(n1) + 2 * carve_size(n1 * 4) + carve_size(n1 * 8));
    ctx->stagemeta.ensure(mb);
    char *cur = ctx->stagemeta.as<char>();
    auto put = [&](const std::vector<StepProg> &v, size_t n, unsigned char *&kind, unsigned char *&cmode, int *&t0, int *&t1, double *&lim) {
        kind = carve<unsigned char>(cur, std::max<size_t>(n, 1)); cmode = carve<unsigned char>(cur, std::max<size_t>(n, 1));
        t0 = carve<int>(cur, std::max<size_t>(n, 1)); t1 = carve<int>(cur, std::max<size_t>(n, 1)); lim = carve<double>(cur, std::max<size_t>(n, 1));
        if (n == 0) return;
        std::vector<unsigned char> hk(n), hc(n);
        std::vector<int> h0(n), h1(n);
        std::vector<double> hl(n);
        for (size_t e = 0; e < n; ++e) { hk[e] = v[e].kind; hc[e] = v[e].cmode; h0[e] = v[e].t0; h1[e] = v[e].t1; hl[e] = v[e].limit; }
        HIPCHECK(hipMemcpyAsync(kind, hk.data(), n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(cmode, hc.data(), n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(t0, h0.data(), n * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(t1, h1.data(), n * 4, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(lim, hl.data(), n * 8, hipMemcpyHostToDevice, st));
        sync_stream(ctx, st);                     // (the host vectors go out of scope)
    };
    put(prog.preF, nF, S.kindF, S.cmodeF, S.tapF0, S.tapF1, S.limitF);
    put(prog.preB, nB, S.kindB, S.cmodeB, S.tapB0, S.tapB1, S.limitB);
    const size_t outd = (size_t)B * G, psd = (size_t)B * NRED * nblk;
    ctx->stagebuf.ensure(2 * (outd + psd) * 8);
    double *base = ctx->stagebuf.as<double>();
    S.out[0] = base; S.out[1] = base + outd; S.ps[0] = base + 2 * outd; S.ps[1] = base + 2 * outd + psd;
}

// host-side results of one batch of chains
struct BatchOutcome {
    std::vector<double> logE, local, means, invN;    // (B,), (B, T), (B, ndim, T), (B, T): 1 / row sum of the stored sequence
    std::vector<int64_t> abort_step;
    std::vector<int32_t> abort_phase;
};

// BLHIP_CARRY: keep every chain's filtered distribution of the last step, normalised (core.py:2173)
void store_carry(blhip_ctx *ctx, const blhip_problem *p, int64_t B, long long G, const double *redF, const double *fin, long long fstr,
                 double *d_w, bool has_clamp) {
    hipStream_t st = ctx->stream;
    const int64_t T = p->T;
    blhip_ctx::Carry &cs = ctx->carry[p->carry_slot];
    cs.buf.ensure((size_t)B * G * 8);
    std::vector<double> inv(B);
    for (int64_t b = 0; b < B; ++b) inv[b] = 1.0 / redF[((size_t)(T - 1) * B + b) * NRED];
    HIPCHECK(hipMemcpyAsync(d_w, inv.data(), B * 8, hipMemcpyHostToDevice, st));
    const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 4096);
    BL_LAUNCH(carry_store_kernel, dim3(gx, (unsigned)B), dim3(NTHREADS), 0, st, cs.buf.as<double>(), fin, fstr, G, d_w);
    sync_stream(ctx, st);
    cs.chains = B; cs.G = G; cs.valid = true;
    cs.maxv.clear();
    if (has_clamp)                               // clamp batches run the generic kernel, which reports the state maximum
        for (int64_t b = 0; b < B; ++b) cs.maxv.push_back(redF[((size_t)(T - 1) * B + b) * NRED + 6] * inv[b]);
}

// fold the batch into the average posterior (core.py:1358-1366): linear accumulator with a running reference exponent.
// Two halves: prepare_fold turns the batch's evidences into weights (staged in h_w / h_invN, which must stay valid until the launch has consumed them) and
// advances the accumulator's reference; launch_fold copies them to the device and runs the pass on `st`.
struct FoldJob {
    const double *d_post = nullptr;
    int64_t B = 0;
    double *h_w = nullptr, *h_invN = nullptr;        // host staging (B), (T * B)
    double *d_w = nullptr, *d_invN = nullptr;        // device copies
    double r = 0.0;                                  // factor of what the accumulator already holds
    int first = 0;
    int sm_n0 = 0;                                   // > 0: d_post is in the chain-resident kernel's strip-major layout (rows per strip)
    int pad_n0p = 0, pad_n0 = 0, pad_n1 = 0;         // > 0: ... on a padded geometry (rows per strip n0p; the grid's true sizes)
    int pad_ax = 0;                                  //      ... in the alternating layouts of the both-axes kernels (blk::ax_layout_b)
    long long pad_step = 0;                          //      doubles per time step of a chain's sequence there
};

bool prepare_fold(blhip_ctx *ctx, int64_t T, int64_t B, const BatchOutcome &out, const double *log_w_batch, FoldJob &job) {
    double newref = ctx->acc_logref;
    std::vector<double> lw(B, -INFINITY);
    std::vector<char> valid(B, 0);
    for (int64_t b = 0; b < B; ++b) {
        // np.isfinite(logEvidence) guard (core.py:1358); a zero hyper-prior contributes log(0) = -inf, i.e. nothing
        valid[b] = out.abort_step[b] < 0 && std::isfinite(out.logE[b]) && std::isfinite(log_w_batch[b]);
        if (!valid[b]) continue;
        lw[b] = out.logE[b] + log_w_batch[b];
        if (lw[b] > newref) newref = lw[b];
    }
    if (!std::isfinite(newref)) return false;
    int nfold = 0;
    for (int64_t b = 0; b < B; ++b) {
        job.h_w[b] = valid[b] ? std::exp(lw[b] - newref) : 0.0;
        nfold += valid[b] ? 1 : 0;
    }
    std::memcpy(job.h_invN, out.invN.data(), (size_t)T * B * 8);
    job.r = ctx->acc_first ? 0.0 : std::exp(ctx->acc_logref - newref);
    job.first = ctx->acc_first ? 1 : 0;
    job.B = B;
    ctx->timing.accumulate_launches += 1;
    ctx->acc_logref = newref;
    ctx->acc_first = false;
    ctx->acc_folded += nfold;
    return true;
}

void launch_fold(blhip_ctx *ctx, int64_t T, long long G, const FoldJob &job, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    const int64_t B = job.B;
    HIPCHECK(hipMemcpyAsync(job.d_w, job.h_w, B * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(job.d_invN, job.h_invN, (size_t)T * B * 8, hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(ev0, st));
    // (steps [t0, t0 + nt) per launch: the accumulator, the sequences and the row normalisers invN[b * T + t] all move by t0 steps)
    if (job.pad_n0p > 0) {
        for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
            BL_LAUNCH(accumulate_pad_kernel, dim3((unsigned)((G + NTHREADS - 1) / NTHREADS), nt), dim3(NTHREADS), 0, st, ctx->acc,
                               job.d_post, (long long)T * job.pad_step, (int)B, job.pad_n0, job.pad_n1, (int)T, job.d_w, job.d_invN, job.r, job.first,
                               job.pad_n0p, job.pad_step, job.pad_ax, (int)t0);
        });
    } else if (job.sm_n0 == 0 && B >= 16 && ((G / 2 + NTHREADS - 1) / NTHREADS) * T < 1024) {        // small grids: too few blocks with a thread per cell
        for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
            BL_LAUNCH(accumulate_small_kernel, dim3((unsigned)((G + 63) / 64), nt), dim3(NTHREADS), 0, st, ctx->acc + (size_t)t0 * G, job.d_post + (size_t)t0 * G,
                               (long long)T * G, (int)B, G, (int)T, job.d_w, job.d_invN + t0, job.r, job.first);
        });
    } else if ((G & 1) == 0 && ((uintptr_t)ctx->acc & 15) == 0) {
        const unsigned gx2 = (unsigned)((G / 2 + NTHREADS - 1) / NTHREADS);
        for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
            BL_LAUNCH(accumulate2_kernel, dim3(gx2, nt), dim3(NTHREADS), 0, st, ctx->acc + (size_t)t0 * G, job.d_post + (size_t)t0 * G,
                               (long long)T * G, (int)B, G, (int)T, job.d_w, job.d_invN + t0, job.r, job.first, job.sm_n0);
        });
    } else {
        if (job.sm_n0 > 0) fail("internal: strip-major sequences need an even number of cells and a 16-byte aligned accumulator");
        const unsigned gx = (unsigned)std::min<long long>((G + NTHREADS - 1) / NTHREADS, 4096);
        for_grid_y(ctx, T, [&](long long t0, unsigned nt) {
            BL_LAUNCH(accumulate_kernel, dim3(gx, nt), dim3(NTHREADS), 0, st, ctx->acc + (size_t)t0 * G, job.d_post + (size_t)t0 * G,
                               (long long)T * G, (int)B, G, (int)T, job.d_w, job.d_invN + t0, job.r, job.first);
        });
    }
    HIPCHECK(hipEventRecord(ev1, st));
}

// the whole fold on the main stream, waited for
// (later_ev: do not wait -- the fold stays in front of whatever the stream runs next, e.g. the next batch's metadata uploads and forward
//  pass; its two timing events are appended for the caller to read after the stream has drained.  The page-locked staging of the weights is
//  reused by the next batch's fold only after that batch's passes have been waited for, on the same stream.)
void fold_accumulate(blhip_ctx *ctx, int64_t T, long long G, int64_t B, const BatchOutcome &out, const double *log_w_batch, const double *d_post,
                     double *d_w, double *d_invN, int sm_n0 = 0, const FoldJob *layout = nullptr, std::vector<hipEvent_t> *later_ev = nullptr) {
    ctx->pinA.ensure(((size_t)B + (size_t)T * B) * 8);
    FoldJob job;
    if (layout) job = *layout;
    job.sm_n0 = sm_n0;
    job.h_w = ctx->pinA.as<double>(); job.h_invN = job.h_w + B;
    job.d_w = d_w; job.d_invN = d_invN; job.d_post = d_post;
    if (!prepare_fold(ctx, T, B, out, log_w_batch, job)) return;
    if (later_ev) {
        hipEvent_t e0, e1;
        HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
        later_ev->push_back(e0); later_ev->push_back(e1);
        launch_fold(ctx, T, G, job, ctx->stream, e0, e1);
        return;
    }
    launch_fold(ctx, T, G, job, ctx->stream, ctx->ev[4], ctx->ev[5]);
    sync_stream(ctx, ctx->stream);
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
    ctx->timing.accumulate_ms += ms;
}

// the batch's sequence stays on the device as the kept posterior; rows [row0, row1) still carry their raw sums (core.py:389 / :441)
void keep_posterior(blhip_ctx *ctx, const Geometry &g, int64_t T, int64_t B, const BatchOutcome &out, int64_t row0, int64_t row1) {
    hipStream_t st = ctx->stream;
    ctx->postinv.ensure((size_t)T * B * 8);
    HIPCHECK(hipMemcpyAsync(ctx->postinv.p, out.invN.data(), (size_t)T * B * 8, hipMemcpyHostToDevice, st));
    sync_stream(ctx, st);
    ctx->post_valid = true; ctx->post_scaled = false; ctx->post_chains = B; ctx->post_T = T; ctx->post_G = g.G;
    ctx->post_series = ctx->series.data != nullptr;
    ctx->post_row0 = row0; ctx->post_row1 = row1;
    ctx->post_n0 = g.n0; ctx->post_n1 = g.n1;
    // normalised now, as part of the fit (core.py:441 is inside Study.fit)
    ensure_post_scaled(ctx); sync_stream(ctx, st);
}

void write_results(blhip_result *res, const blhip_problem *p, int64_t c0, int64_t B, const BatchOutcome &out, bool with_means) {
    if (!res) return;
    const int64_t T = p->T;
    for (int64_t b = 0; b < B; ++b) {
        if (res->log_evidence) res->log_evidence[c0 + b] = out.logE[b];
        if (res->abort_step) res->abort_step[c0 + b] = out.abort_step[b];
        if (res->abort_phase) res->abort_phase[c0 + b] = out.abort_phase[b];
        if (res->local_evidence)
            std::memcpy(res->local_evidence + (size_t)(c0 + b) * T, &out.local[(size_t)b * T], T * 8);
        if (res->posterior_mean && with_means)
            std::memcpy(res->posterior_mean + (size_t)(c0 + b) * p->ndim * T, &out.means[(size_t)b * p->ndim * T], (size_t)p->ndim * T * 8);
    }
}
