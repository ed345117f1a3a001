// Probability queries of the parser at many time steps in one call:  out[s] = sum over the cells (pairs of cells) where  f REL 0  holds of the
// probability of the cell (pair) at step steps[s] -- bl.Parser / Study.eval with a vector of time stamps (reference bayesloop/parser.py:256-440:
// the quantities of a query, their element-wise and outer-product arithmetic, "lhs REL rhs" as "-1*(rhs)+lhs REL 0" and the sum of the
// probabilities where it holds; core.py:604-621: Study.eval), whose users loop the scalar call over every time stamp.
//
// f is a small postfix program in the instruction set of the likelihood programs (blhip_likprog.hpp) over
//   space A   the parameter grid of the study whose posterior sequence lives on the device: PARAM k (the marginal grid value of axis k at the
//             cell), AXIS (a function of ONE parameter the host tabulated along its axis with the very NumPy call the scalar path uses)
//   space B   (pair queries) a second, independent quantity held by the host -- another study's parameters, a hyper-grid: BCOL k (column k of
//             b_values at the B cell: a value column or a host-evaluated function of B alone)
//   STEP j    value j of the current step (a series bound to a name, or a function of series alone the host evaluated)
//   CONST i, ADD MUL DIV NEG ABS SQRT EXP LOG POW POWI COS SIN, LT LE EQ.
// The interpreter executes one IEEE operation per op: nothing is contracted, + - * / sqrt round once as in NumPy.  NaN REL 0 is false.
//
//  * query_rows_kernel<SERIES> (one space): grid = (slabs of cells, blocks of SB steps).  A thread walks the cells of its slab NT apart; without
//    STEP values the indicator of a cell is evaluated ONCE and reused for the SB steps of the block (SERIES = false), otherwise per step.  It adds
//    post[steps[s]][cell] where the indicator holds -- consecutive lanes read consecutive cells of a row, every selected row is read once -- and
//    the block writes one partial per (slab, step).
//  * query_pairs_kernel<SERIES> (two spaces): a thread owns ONE A cell; B's probabilities of the block's steps are staged in LDS, BJ cells at a
//    time (every lane reads the same LDS word: a broadcast); acc[s] += pB[s][j] where the indicator of the pair (i, j) holds, evaluated once per
//    step block (per step with SERIES).  acc[s] * pA[s][i] is reduced over the block.  The G_a x G_b space is never materialised.  The
//    normaliser of the outer product (parser.py:239-243: prob / prob.sum()) is formed beside it: (sum_i pA)(sum_j pB) per block.
//  * combine_kernel adds the partials of the slabs in ascending order (and divides by the normaliser for pairs).  No floating-point atomics: two
//    calls on the same inputs return the same bits.
//
// The host-only part (QueryPlan, query_plan, check_query) has no HIP call in it.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/blhip.h"
#include "blhip_likprog.hpp"

namespace blq {

constexpr int NT = 256;                    // threads of a block
constexpr int SB = 16;                     // steps of a block
constexpr int BJ = 256;                    // B cells of an LDS tile (SB x BJ doubles = 32 KiB)
constexpr long long SLAB_MIN = 1024;       // shortest slab of the one-space kernel (a multiple of NT)
constexpr long long SLABS_MAX = 4096;
constexpr long long BLOCKS_WANTED = 2048;  // slabs x step blocks the plan aims for (256 CUs x 8 blocks)
constexpr long long STEPS_MAX = 32768ll * SB;      // most steps of a chunk: its step blocks are the gridDim.y of one launch
constexpr long long ALIGN = 256;
constexpr int OP_BCOL = 32;                // beyond bllp's codes: column arg of b_values at the B cell
enum : int { REL_LT = 0, REL_LE = 1, REL_EQ = 2, REL_GT = 3, REL_GE = 4 };

struct QueryPlan {
    long long slab = 0;               // A cells per block along x (pairs: NT, one cell per thread)
    long long n_slabs = 0;
    long long steps_per_chunk = 0;    // steps whose uploads and partials are resident at a time
    long long n_chunks = 0;
    long long workspace_bytes = 0;
    long long min_budget_bytes = 0;   // the smallest budget the plan accepts (one step per chunk)
    // the places inside the workspace (bytes): what does not depend on the step first
    long long off_steps = 0, off_series = 0, off_bprob = 0, off_part = 0, off_out = 0;
};

inline long long round_up(long long v, long long q) { return (v + q - 1) / q * q; }

// G cells of A, n_steps steps, n_series STEP values per step, n_b cells of B (0: one space), b_const: B's probabilities do not change with the
// step (they are then part of fixed_bytes), fixed_bytes: the uploads that do not depend on the step.  -> false: bad arguments or a budget below
// min_budget_bytes (which is filled in whenever the arguments are good).
inline bool query_plan(long long G, long long n_steps, long long n_series, long long n_b, bool b_const, long long fixed_bytes, double budget, QueryPlan &P) {
    P = QueryPlan{};
    if (G < 1 || n_steps < 1 || n_series < 0 || n_b < 0 || fixed_bytes < 0 || G > (1ll << 40) || n_steps > (1ll << 31) || n_series > (1ll << 20) ||
        n_b > (1ll << 31) || fixed_bytes > (1ll << 46))
        return false;
    const bool pairs = n_b > 0;
    if (pairs) {
        P.slab = NT;
    } else {
        const long long nsb = (n_steps + SB - 1) / SB;
        long long want = (BLOCKS_WANTED + nsb - 1) / nsb;
        want = want < 1 ? 1 : (want > SLABS_MAX ? SLABS_MAX : want);
        P.slab = round_up((G + want - 1) / want, NT);
        if (P.slab < SLAB_MIN) P.slab = SLAB_MIN;
    }
    P.n_slabs = (G + P.slab - 1) / P.slab;
    const long long fixed = round_up(fixed_bytes, ALIGN);
    const long long np = pairs ? 2 : 1;
    auto need = [&](long long s, long long *off) {
        long long o[5];
        o[0] = fixed;                                                   // steps (int64)
        o[1] = o[0] + round_up(s * 8, ALIGN);                            // series
        o[2] = o[1] + round_up(s * (n_series > 0 ? n_series : 1) * 8, ALIGN);       // B's probabilities per step
        o[3] = o[2] + round_up((pairs && !b_const ? s * n_b : 1) * 8, ALIGN);       // partials
        o[4] = o[3] + round_up(P.n_slabs * np * s * 8, ALIGN);           // out
        if (off) for (int k = 0; k < 5; ++k) off[k] = o[k];
        return o[4] + round_up(s * 8, ALIGN);
    };
    P.min_budget_bytes = need(1, nullptr);
    if (!(budget >= (double)P.min_budget_bytes)) return false;
    long long s = n_steps < STEPS_MAX ? n_steps : STEPS_MAX;
    if ((double)need(s, nullptr) > budget) {
        // bisect for the largest count of steps that fits, then whole step blocks where there are several
        long long lo = 1, hi = s;
        while (lo < hi) {
            const long long mid = lo + (hi - lo + 1) / 2;
            if ((double)need(mid, nullptr) <= budget) lo = mid; else hi = mid - 1;
        }
        s = lo > SB ? lo / SB * SB : lo;
    }
    P.steps_per_chunk = s;
    P.n_chunks = (n_steps + s - 1) / s;
    long long off[5];
    P.workspace_bytes = need(s, off);
    P.off_steps = off[0]; P.off_series = off[1]; P.off_bprob = off[2]; P.off_part = off[3]; P.off_out = off[4];
    return true;
}

// ---- host-only validation of a query (no HIP call) -> 0, or -1 with a message in err ---------------------------------------------------------
inline int check_query(const blhip_query *q, int64_t n_steps, char *err, int errlen) {
    auto bad = [&](const char *fmt, long long a, long long b, long long c) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a, b, c);
        return -1;
    };
    if (!q) return bad("query: query is NULL", 0, 0, 0);
    if (n_steps < 1 || n_steps > (1ll << 31)) return bad("query: n_steps = %lld", n_steps, 0, 0);
    if (!q->ops || q->n_ops < 1) return bad("query: no ops", 0, 0, 0);
    if (q->n_ops > bllp::MAX_OPS) return bad("query: %lld ops (at most %lld)", q->n_ops, bllp::MAX_OPS, 0);
    if (q->n_consts < 0 || q->n_series < 0 || q->n_series > (1 << 20)) return bad("query: bad table size", 0, 0, 0);
    if (q->n_consts > 0 && !q->consts) return bad("query: consts is NULL", 0, 0, 0);
    if (q->n_series > 0 && !q->series) return bad("query: series is NULL", 0, 0, 0);
    if (q->relation < REL_LT || q->relation > REL_GE) return bad("query: relation code %lld (0 .. 4)", q->relation, 0, 0);
    if (q->ndim < 1 || q->ndim > BLHIP_MAX_DIM) return bad("query: %lld parameters (1 .. %lld)", q->ndim, BLHIP_MAX_DIM, 0);
    for (int k = 0; k < q->ndim; ++k) {
        if (q->n[k] < 1 || q->n[k] > (1ll << 30)) return bad("query: bad grid axis %lld", k, 0, 0);
        if (!q->marginal[k]) return bad("query: marginal[%lld] is NULL", k, 0, 0);
    }
    if (q->n_b < 0 || q->n_b > (1ll << 31) || q->n_bcols < 0 || q->n_bcols > (1 << 20)) return bad("query: bad B space", 0, 0, 0);
    if (q->n_b > 0 && !q->b_prob) return bad("query: b_prob is NULL", 0, 0, 0);
    if (q->n_b > 0 && q->n_bcols > 0 && !q->b_values) return bad("query: b_values is NULL", 0, 0, 0);
    // the program: bllp's stack discipline and index ranges over a copy whose BCOL pushes stand in as DATA pushes; what a query has no
    // meaning for (DATA, AND, SELECT) is refused first
    std::vector<int32_t> ops((size_t)q->n_ops * 2);
    for (int64_t pc = 0; pc < q->n_ops; ++pc) {
        const int code = q->ops[2 * pc], arg = q->ops[2 * pc + 1];
        ops[2 * pc] = code; ops[2 * pc + 1] = arg;
        if (code == bllp::OP_DATA || code == bllp::OP_AND || code == bllp::OP_SELECT) return bad("query: op %lld: code %lld is not part of a query program", pc, code, 0);
        if (code == OP_BCOL) {
            if (q->n_b < 1) return bad("query: op %lld: BCOL without a B space", pc, 0, 0);
            if (arg < 0 || arg >= q->n_bcols) return bad("query: op %lld: BCOL %lld out of range (%lld columns)", pc, arg, q->n_bcols);
            ops[2 * pc] = bllp::OP_DATA; ops[2 * pc + 1] = 0;
        }
        if (code == bllp::OP_AXIS && arg >= 0 && (arg & 3) < q->ndim && (long long)(arg >> 2) + q->n[arg & 3] > q->n_consts)
            return bad("query: op %lld: AXIS table at %lld runs past the %lld constants", pc, arg >> 2, q->n_consts);
    }
    if (bllp::check_program(ops.data(), q->n_ops, q->n_consts, q->n_series, q->ndim, err, errlen) != 0) return -1;
    if (q->n_series > 0)
        for (int64_t k = 0; k < n_steps * q->n_series; ++k)
            if (!std::isfinite(q->series[k])) return bad("query: series value %lld is not finite", k, 0, 0);
    return 0;
}

// ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
struct QueryParams {
    const bllp::Instr *ops;          // uniform across the launch: read through the scalar path
    const double *consts;
    const double *series;            // (S, n_series) of the chunk
    const long long *steps;          // (S) rows of the sequence
    const double *post;              // row 0 of the sequence
    const double *m[bllp::MAX_DIM];  // marginal grids of A
    const double *bval;              // (n_bcols, nb)
    const double *bprob;             // (S, nb) of the chunk, or (1, nb) with b_const
    double *part;                    // rows: (n_slabs, S); pairs: (n_slabs, 2, S) -- weighted count, normaliser
    long long G, slab, nb;
    int n[bllp::MAX_DIM];
    int n_ops, n_series, ndim, S, rel, b_const;
};

struct Cell { int idx[bllp::MAX_DIM]; double g[bllp::MAX_DIM]; };

static __device__ __forceinline__ Cell locate(const QueryParams &P, long long c) {
    Cell L;
#pragma unroll
    for (int k = 0; k < bllp::MAX_DIM; ++k) { L.idx[k] = 0; L.g[k] = 0.0; }
    if (P.G <= 0x7fffffffLL) {
        unsigned r = (unsigned)c;
#pragma unroll
        for (int k = bllp::MAX_DIM - 1; k >= 0; --k)
            if (k < P.ndim) { const unsigned q = r / (unsigned)P.n[k]; L.idx[k] = (int)(r - q * (unsigned)P.n[k]); r = q; }
    } else {
        long long r = c;
#pragma unroll
        for (int k = bllp::MAX_DIM - 1; k >= 0; --k)
            if (k < P.ndim) { const long long q = r / P.n[k]; L.idx[k] = (int)(r - q * P.n[k]); r = q; }
    }
#pragma unroll
    for (int k = 0; k < bllp::MAX_DIM; ++k)
        if (k < P.ndim) L.g[k] = P.m[k][L.idx[k]];
    return L;
}

// f at the cell L of A, the cell j of B (uniform across the block) and the step values sv: bllp's interpreter without DATA / AND / SELECT
static __device__ __forceinline__ double evaluate(const QueryParams &P, const Cell &L, long long j, bllp::uniform_doubles sv) {
    const bllp::uniform_instrs ops = (bllp::uniform_instrs)P.ops;
    const bllp::uniform_doubles consts = (bllp::uniform_doubles)P.consts;
    const bllp::uniform_doubles bval = (bllp::uniform_doubles)P.bval;
    bllp::Stack st;
    double top = 0.0;
    int sp = 0;                                    // values on the stack, the top one in `top`
    for (int pc = 0; pc < P.n_ops; ++pc) {
        const int code = __builtin_amdgcn_readfirstlane(ops[pc].code), arg = __builtin_amdgcn_readfirstlane(ops[pc].arg);
        if (code <= bllp::OP_AXIS || code == OP_BCOL) {            // pushes
            if (sp > 0) st.put(sp - 1, top);
            ++sp;
            if (code == bllp::OP_CONST) top = consts[arg];
            else if (code == bllp::OP_PARAM) top = arg == 0 ? L.g[0] : (arg == 1 ? L.g[1] : (arg == 2 ? L.g[2] : L.g[3]));
            else if (code == bllp::OP_STEP) top = sv[arg];
            else if (code == OP_BCOL) top = bval[(long long)arg * P.nb + j];
            else {
                const int ax = arg & 3;
                top = P.consts[(arg >> 2) + (ax == 0 ? L.idx[0] : (ax == 1 ? L.idx[1] : (ax == 2 ? L.idx[2] : L.idx[3])))];
            }
        } else if (code == bllp::OP_NEG) top = -top;
        else if (code == bllp::OP_ABS) top = fabs(top);
        else if (code == bllp::OP_SQRT) top = sqrt(top);
        else if (code == bllp::OP_EXP) top = exp(top);
        else if (code == bllp::OP_LOG) top = log(top);
        else if (code == bllp::OP_COS) top = cos(top);
        else if (code == bllp::OP_SIN) top = sin(top);
        else if (code == bllp::OP_POWI) top = arg == 2 ? top * top : bllp::powi(top, arg);
        else {                                     // binary: a = the value below the top, b = the top
            const double a = st.get(sp - 2), b = top;
            --sp;
            if (code == bllp::OP_ADD) top = a + b;
            else if (code == bllp::OP_MUL) top = a * b;
            else if (code == bllp::OP_DIV) top = a / b;
            else if (code == bllp::OP_POW) top = pow(a, b);
            else if (code == bllp::OP_LT) top = a < b ? 1.0 : 0.0;
            else if (code == bllp::OP_LE) top = a <= b ? 1.0 : 0.0;
            else top = a == b ? 1.0 : 0.0;          // OP_EQ
        }
    }
    return top;
}

// v REL 0; false for a NaN, as NumPy's comparison
static __device__ __forceinline__ bool holds(int rel, double v) {
    return rel == REL_LT ? v < 0.0 : (rel == REL_LE ? v <= 0.0 : (rel == REL_EQ ? v == 0.0 : (rel == REL_GT ? v > 0.0 : v >= 0.0)));
}

// sum of v over the block in a fixed order (lanes by halving, then the waves in ascending order); the result is valid in thread 0.
// red: NT / 64 doubles of LDS nobody else touches between the two barriers
static __device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) s += red[w];
    return s;
}

// grid = (slabs of cells, blocks of SB steps)
template <bool SERIES>
static __global__ __launch_bounds__(NT) void query_rows_kernel(const QueryParams P) {
#pragma clang fp contract(off)
    __shared__ double red[NT / 64];
    const int s0 = (int)blockIdx.y * SB, ns = min(SB, P.S - s0);
    const long long lo = (long long)blockIdx.x * P.slab, hi = min(P.G, lo + P.slab);
    const bllp::uniform_doubles series = (bllp::uniform_doubles)P.series;
    double acc[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) acc[s] = 0.0;
    for (long long c = lo + threadIdx.x; c < hi; c += NT) {
        const Cell L = locate(P, c);
        bool ind0 = false;
        if (!SERIES) ind0 = holds(P.rel, evaluate(P, L, 0, series));
#pragma unroll
        for (int s = 0; s < SB; ++s) {
            if (s < ns) {                            // (block-uniform)
                const bool ind = SERIES ? holds(P.rel, evaluate(P, L, 0, series + (long long)(s0 + s) * P.n_series)) : ind0;
                const double p = P.post[P.steps[s0 + s] * P.G + c];
                acc[s] += ind ? p : 0.0;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) {
        if (s < ns) {
            const double v = block_sum(acc[s], red);
            if (threadIdx.x == 0) P.part[(long long)blockIdx.x * P.S + s0 + s] = v;
        }
    }
}

// grid = (blocks of NT cells of A, blocks of SB steps)
template <bool SERIES>
static __global__ __launch_bounds__(NT) void query_pairs_kernel(const QueryParams P) {
#pragma clang fp contract(off)
    __shared__ double pb[SB][BJ];
    __shared__ double red[NT / 64];
    const int s0 = (int)blockIdx.y * SB, ns = min(SB, P.S - s0);
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const bool valid = i < P.G;
    const Cell L = locate(P, valid ? i : P.G - 1);          // (a thread past the grid evaluates the last cell; its weight is zero)
    const bllp::uniform_doubles series = (bllp::uniform_doubles)P.series;
    double acc[SB], col[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) { acc[s] = 0.0; col[s] = 0.0; }
    for (long long j0 = 0; j0 < P.nb; j0 += BJ) {
        const int nj = (int)min((long long)BJ, P.nb - j0);
        __syncthreads();
        // stage B's probabilities of the block's steps: thread x takes column j0 + x of every row (and keeps that column's share of the row sums)
#pragma unroll
        for (int s = 0; s < SB; ++s) {
            if (s < ns) {
                const double v = (int)threadIdx.x < nj ? P.bprob[(P.b_const ? 0ll : (long long)(s0 + s)) * P.nb + j0 + threadIdx.x] : 0.0;
                pb[s][threadIdx.x] = v;
                col[s] += v;
            }
        }
        __syncthreads();
        for (int jj = 0; jj < nj; ++jj) {
            bool ind0 = false;
            if (!SERIES) ind0 = holds(P.rel, evaluate(P, L, j0 + jj, series));
#pragma unroll
            for (int s = 0; s < SB; ++s) {
                if (s < ns) {
                    const bool ind = SERIES ? holds(P.rel, evaluate(P, L, j0 + jj, series + (long long)(s0 + s) * P.n_series)) : ind0;
                    acc[s] += ind ? pb[s][jj] : 0.0;
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) {
        if (s < ns) {
            const double pa = valid ? P.post[P.steps[s0 + s] * P.G + i] : 0.0;
            const double count = block_sum(valid ? pa * acc[s] : 0.0, red);
            const double sum_a = block_sum(pa, red);
            const double sum_b = block_sum(col[s], red);
            if (threadIdx.x == 0) {
                P.part[((long long)blockIdx.x * 2 + 0) * P.S + s0 + s] = count;
                P.part[((long long)blockIdx.x * 2 + 1) * P.S + s0 + s] = sum_a * sum_b;
            }
        }
    }
}

// out[s] = sum over the slabs, in ascending order, of the partial counts (pairs: divided by the sum of the partial normalisers); one thread per step
static __global__ __launch_bounds__(NT) void combine_kernel(const double *part, double *out, int n_slabs, int S, int pairs) {
#pragma clang fp contract(off)
    const int s = (int)blockIdx.x * NT + threadIdx.x;
    if (s >= S) return;
    const long long np = pairs ? 2 : 1;
    double count = part[s];
    for (int k = 1; k < n_slabs; ++k) count += part[(long long)k * np * S + s];
    if (pairs) {
        double norm = part[S + s];
        for (int k = 1; k < n_slabs; ++k) norm += part[((long long)k * 2 + 1) * S + s];
        count = count / norm;
    }
    out[s] = count;
}

}   // namespace blq
