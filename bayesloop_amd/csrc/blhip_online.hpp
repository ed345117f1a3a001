// Blocks of an online study (OnlineStudy.stepMany, bayesloop_amd/core.py): what a block of N data points needs beside the resumed,
// carried N-step fits the library runs anyway -- the evidence-weighted mixture over chains with weights that change from step to step
// (the reference forms it once per data point, core.py:2194-2211), and the cut of a long block along TIME so that the kept sequence of
// its widest transition model and the history buffer stay within the memory budget.
#pragma once
#include "blhip_kernels.hpp"

namespace blo {

using blk::NTHREADS;

// ---- time chunks (host only) -----------------------------------------------------------------------------------------------------------
// A resumed fit needs all chains of a transition model in ONE batch, so a block is cut along time.  What a chunk of `steps` steps holds on
// the device: the kept sequence of the widest model (chains x steps rows of the grid as the fit lays it out, its row normalisers and the
// partial sums of the step kernels as chains_per_batch counts them), its state ping-pong (2 rows per chain), and `planes` history planes of
// (steps, G) cells.
struct BlockPlan {
    int64_t steps = 0;            // steps per chunk (the last chunk may be shorter)
    int64_t n_chunks = 0;
    int64_t chunk_bytes = 0;      // what a chunk of `steps` steps takes
    int64_t min_budget_bytes = 0; // ... and one of a single step: the smallest budget accepted
};

// (two-parameter grids of PAD_ROWS_MIN .. PAD_ROWS_MAX rows: the memory plan of a fit counts the chain-resident kernels' padded geometry --
//  chains_per_batch; the constants are held to that file's by static_asserts where both are visible, blhip_batch.hpp)
constexpr int PAD_ROWS_MIN = 32, PAD_ROWS_MAX = 1024, PAD_ROWS = 128, PAD_COLS = 16;

inline int64_t block_cells(int ndim, const int64_t *n, int64_t &G) {
    G = 1;
    for (int k = 0; k < ndim; ++k) G *= n[k];
    int64_t Gk = G;
    if (ndim == 2 && n[0] >= PAD_ROWS_MIN && n[0] <= PAD_ROWS_MAX) Gk = ((n[0] + PAD_ROWS - 1) / PAD_ROWS * PAD_ROWS) * ((n[1] + PAD_COLS - 1) / PAD_COLS * PAD_COLS);
    return Gk;
}

inline double block_bytes(int64_t G, int64_t Gk, int64_t chains, int64_t planes, int64_t steps) {
    const double per_chain = ((double)steps + 2.0) * (double)Gk * 8.0 + (double)steps * blk::NRED * 8.0 * 2 * 64.0;
    return (double)chains * per_chain + (double)planes * (double)steps * (double)G * 8.0;
}

// -> false: bad arguments (min_budget_bytes = 0) or a budget below one step (min_budget_bytes says how much one step takes)
inline bool online_block_plan(int ndim, const int64_t *n, int64_t chains, int64_t planes, int64_t N, double budget, BlockPlan &P) {
    P = BlockPlan{};
    if (ndim < 1 || ndim > 4 || !n || chains < 1 || planes < 0 || N < 1 || !(budget == budget)) return false;
    for (int k = 0; k < ndim; ++k)
        if (n[k] < 1 || n[k] > (1ll << 30)) return false;
    int64_t G = 1;
    const int64_t Gk = block_cells(ndim, n, G);
    const double one = block_bytes(G, Gk, chains, planes, 1);
    if (!(one < 9.0e18)) return false;
    P.min_budget_bytes = (int64_t)std::ceil(one);
    if (budget < one) return false;
    // bytes(steps) is linear in steps: the largest count whose bytes fit, found by bisection on the formula itself (no rounding of a quotient)
    int64_t lo = 1, hi = N;
    if (block_bytes(G, Gk, chains, planes, N) <= budget) lo = N;
    while (lo < hi - 1 && lo != N) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (block_bytes(G, Gk, chains, planes, mid) <= budget) lo = mid; else hi = mid;
    }
    P.steps = lo;
    P.n_chunks = (N + lo - 1) / lo;
    P.chunk_bytes = (int64_t)std::ceil(block_bytes(G, Gk, chains, planes, lo));
    return true;
}

// ---- the time-varying mixture --------------------------------------------------------------------------------------------------------
//   H[t][cell] = (accumulate ? H[t][cell] : 0) + sum_b w[t][b] * seq[b][t][cell]          b ascending, one fma per term
// seq: B sequences of T rows of G cells in the plain layout of the launch-per-step, 1-D and N-D paths ([b][t][cell], chain_stride
// cells between chains) -- the kept posterior of a forward-only fit, normalised -- or planes of the history buffer itself.  A streaming
// kernel: 8 (B T G + T G) bytes, every cell of seq read once, H written once (read once more with `accumulate`).  blockIdx.y is the time
// step; a thread owns a run of cells of that step (WIDE: two, loaded as 16 bytes -- G even, every row base 16-byte aligned; else one) and
// loops over the chains four at a time, so that four independent loads per lane are in flight before the first fma needs its operand.
// No atomics, a fixed order of the sum: two calls on the same inputs give the same bits.
struct MixParams {
    const double *seq; long long chain_stride;
    double *H;
    const double *w;             // (T, B)
    long long G; int B; int accumulate;
    long long t0;                // first time step of this launch (gridDim.y is limited)
};

template <bool WIDE>
__global__ __launch_bounds__(NTHREADS) void mix_sequence_kernel(const MixParams P) {
    const long long t = P.t0 + blockIdx.y;
    const double *w = P.w + t * P.B;
    const long long cs = P.chain_stride;
    if (WIDE) {
        const long long G2 = P.G / 2;
        const double2 *row = reinterpret_cast<const double2 *>(P.seq + t * P.G);
        const long long cs2 = cs / 2;
        double2 *out = reinterpret_cast<double2 *>(P.H + t * P.G);
        for (long long c = (long long)blockIdx.x * NTHREADS + threadIdx.x; c < G2; c += (long long)gridDim.x * NTHREADS) {
            double2 s = P.accumulate ? out[c] : make_double2(0.0, 0.0);
            int b = 0;
            for (; b + 4 <= P.B; b += 4) {
                const double2 p0 = row[(long long)b * cs2 + c], p1 = row[(long long)(b + 1) * cs2 + c];
                const double2 p2 = row[(long long)(b + 2) * cs2 + c], p3 = row[(long long)(b + 3) * cs2 + c];
                const double w0 = w[b], w1 = w[b + 1], w2 = w[b + 2], w3 = w[b + 3];
                s.x = fma(w0, p0.x, s.x); s.y = fma(w0, p0.y, s.y);
                s.x = fma(w1, p1.x, s.x); s.y = fma(w1, p1.y, s.y);
                s.x = fma(w2, p2.x, s.x); s.y = fma(w2, p2.y, s.y);
                s.x = fma(w3, p3.x, s.x); s.y = fma(w3, p3.y, s.y);
            }
            for (; b < P.B; ++b) {
                const double2 p = row[(long long)b * cs2 + c];
                s.x = fma(w[b], p.x, s.x); s.y = fma(w[b], p.y, s.y);
            }
            out[c] = s;
        }
    } else {
        const double *row = P.seq + t * P.G;
        double *out = P.H + t * P.G;
        for (long long c = (long long)blockIdx.x * NTHREADS + threadIdx.x; c < P.G; c += (long long)gridDim.x * NTHREADS) {
            double s = P.accumulate ? out[c] : 0.0;
            int b = 0;
            for (; b + 4 <= P.B; b += 4) {
                const double p0 = row[(long long)b * cs + c], p1 = row[(long long)(b + 1) * cs + c];
                const double p2 = row[(long long)(b + 2) * cs + c], p3 = row[(long long)(b + 3) * cs + c];
                s = fma(w[b], p0, s); s = fma(w[b + 1], p1, s); s = fma(w[b + 2], p2, s); s = fma(w[b + 3], p3, s);
            }
            for (; b < P.B; ++b) s = fma(w[b], row[(long long)b * cs + c], s);
            out[c] = s;
        }
    }
}

}  // namespace blo
