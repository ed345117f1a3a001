// Posterior predictive on the device:  P[t][j] = sum_cell L(x_j | theta_cell) * post[t][cell]  -- Study.simulate for a range of time steps
// (or the time average) and a list of observation values, reference core.py:566-597.
//
// The operation is a dense contraction (T x G) . (G x X) in fp64 whose left operand, the posterior sequence, already lives in HBM, and
// whose right operand, the likelihood rows L(x_j | .), is what the library tabulates when it fits with x_j as the datum.  It goes to the
// fp64 matrix pipe (v_mfma_f64_16x16x4_f64), one wave per (tile of 16 time steps, slab of cells):
//
//  * Both operands are contiguous along the cell axis K, and a dot product does not care in which order K is walked.  Lane (r = lane & 15,
//    q = lane >> 4) loads a RUN of 8 consecutive doubles of "its" row -- row r of the time tile for A, row r of an x tile for B -- starting
//    at cell k0 + 8 q.  Issue i of the 8 MFMAs of a step multiplies element i of every lane's run: its four k indices are the cells
//    k0 + 8 q + i, q = 0 .. 3.  A and B use the same map, so every cell of the 32 of a step meets its partner exactly once; a row gets 256
//    contiguous bytes per wave and step, and nothing is staged in LDS.
//  * D: lane (r, q), register g holds P[t = q + 4 g][x = r] of the tile (the f64 form's own map, not the f32 one).
//  * A wave keeps the accumulators of ALL x tiles of a chunk (up to NXT = 8 tiles, 128 values): a posterior row is read from HBM once
//    per chunk of x values, by one wave; the likelihood rows are read once per tile of 16 time steps.
//  * Split K: blockIdx.x is the slab of cells.  The partial results go to part[slab][t][x]; combine_kernel adds the slabs in ascending
//    order, one thread per output.  No floating-point atomics anywhere: two calls on the same inputs give the same bits.
//  * Ragged edges: a row past the last time step / x value of its tile reads the last valid row again (the result is not stored); a run
//    that crosses the end of the slab reads zeros for BOTH operands beyond it.  No padded copy of anything.
//
// The time average is formed first (average_rows_kernel, compensated summation: the average carries two roundings, whatever T), then
// contracted as a sequence of one row.
//
// The host-only part (PredPlan, predictive_plan) has no HIP in it: tests/host/predictive_plan_main.cpp builds it alone.
#pragma once
#include <cstdint>

namespace blpp {

constexpr int TM = 16;             // time steps per tile (MFMA M)
constexpr int XT = 16;             // x values per tile (MFMA N)
constexpr int NXT = 8;             // x tiles a wave accumulates: at most NXT * XT rows per chunk
constexpr int RUN = 8;             // consecutive cells a lane loads per step
constexpr int KSTEP = 4 * RUN;     // cells per step of a wave
constexpr long long SLAB_MIN = 256;      // shortest slab worth a block of its own (a multiple of KSTEP)
constexpr long long SLABS_MAX = 1024;    // most slabs of a launch
constexpr long long WAVES_WANTED = 2048; // slabs x time tiles the plan aims for (256 CUs x 8 waves)
constexpr size_t ALIGN = 256;

struct PredPlan {
    long long slab = 0;            // cells per slab (a multiple of KSTEP); the last slab may be shorter
    long long n_slabs = 0;         // blocks along K
    long long rows_per_chunk = 0;  // x values whose likelihood rows are resident at a time (1 .. NXT * XT)
    long long n_chunks = 0;
    long long workspace_bytes = 0; // out + average row + likelihood rows + split-K partials
    long long min_budget_bytes = 0;      // the smallest budget the plan accepts (one row per chunk)
    // the places inside the workspace (bytes)
    long long off_out = 0, off_avg = 0, off_rows = 0, off_part = 0;
};

inline long long round_up(long long v, long long q) { return (v + q - 1) / q * q; }

// G cells, T output rows (1 with `average`), X observation values, `budget` bytes of workspace.  -> false: bad arguments or a budget below
// min_budget_bytes (which is filled in whenever the arguments are good).
inline bool predictive_plan(long long G, long long T, long long X, bool average, double budget, PredPlan &P) {
    P = PredPlan{};
    if (G < 1 || T < 1 || X < 1 || G > (1ll << 40) || T > (1ll << 31) || X > (1ll << 31)) return false;
    const long long ttiles = (T + TM - 1) / TM;
    long long want = (WAVES_WANTED + ttiles - 1) / ttiles;
    want = want < 1 ? 1 : (want > SLABS_MAX ? SLABS_MAX : want);
    long long slab = round_up((G + want - 1) / want, KSTEP);
    if (slab < SLAB_MIN) slab = SLAB_MIN;
    P.slab = slab;
    P.n_slabs = (G + slab - 1) / slab;
    const long long out_b = round_up(T * X * 8, ALIGN), avg_b = average ? round_up(G * 8, ALIGN) : 0;
    auto need = [&](long long rows) { return out_b + avg_b + round_up(rows * G * 8, ALIGN) + round_up(P.n_slabs * T * rows * 8, ALIGN); };
    P.min_budget_bytes = need(1);
    if (!(budget >= (double)P.min_budget_bytes)) return false;
    long long rows = X < NXT * XT ? X : NXT * XT;
    while (rows > 1 && (double)need(rows) > budget) {
        // (whole x tiles while there are several; below one tile, one value at a time)
        rows = rows > XT ? round_up(rows, XT) - XT : rows - 1;
    }
    P.rows_per_chunk = rows;
    P.n_chunks = (X + rows - 1) / rows;
    P.workspace_bytes = need(rows);
    P.off_out = 0;
    P.off_avg = out_b;
    P.off_rows = out_b + avg_b;
    P.off_part = P.off_rows + round_up(rows * G * 8, ALIGN);
    return true;
}

}   // namespace blpp

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace blpp {

typedef double d4 __attribute__((ext_vector_type(4)));

struct ContractParams {
    const double *post;            // row 0 of the time range (or the one average row)
    const double *rows;            // (xc, G) likelihood rows of the chunk
    double *part;                  // (n_slabs, T, xc) partial results
    long long G, slab;
    int T, xc;                     // rows of `post` in the range, x values of the chunk
    long long tile0;               // first time tile of this launch (for_grid_y)
    int wide;                      // both operands 16-byte aligned with G even: runs are loaded as 4 x 16 bytes
};

// one lane's run of RUN cells from `p`; cells at or beyond `left` (what is left of the slab from p on) read as zero
template <bool FULL, bool WIDE>
__device__ __forceinline__ void load_run(double (&v)[RUN], const double *p, long long left) {
    if (FULL && WIDE) {
        const double2 *p2 = reinterpret_cast<const double2 *>(p);
#pragma unroll
        for (int i = 0; i < RUN / 2; ++i) { const double2 w = p2[i]; v[2 * i] = w.x; v[2 * i + 1] = w.y; }
    } else if (FULL) {
#pragma unroll
        for (int i = 0; i < RUN; ++i) v[i] = p[i];
    } else {
#pragma unroll
        for (int i = 0; i < RUN; ++i) v[i] = i < left ? p[i] : 0.0;
    }
}

// one step of a wave: KSTEP cells of its time tile against the same cells of every x tile of the chunk.  pb: the rows of the full x tiles,
// pb_last: those of the last one (whose rows past the chunk's end are its last row once more)
template <bool FULL, bool WIDE>
__device__ __forceinline__ void contract_step(d4 (&acc)[NXT], const double *pa, const double *pb, const double *pb_last, long long xstride, int nxt,
                                              long long left) {
    double a[RUN], b[RUN];
    load_run<FULL, WIDE>(a, pa, left);
#pragma unroll
    for (int xt = 0; xt < NXT; ++xt) {
        if (xt < nxt) {                              // (wave-uniform)
            load_run<FULL, WIDE>(b, (xt < nxt - 1 ? pb : pb_last) + xt * xstride, left);
#pragma unroll
            for (int i = 0; i < RUN; ++i) acc[xt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[i], acc[xt], 0, 0, 0);
        }
    }
}

// grid = (slabs, time tiles of this launch), block = one wave
static __global__ __launch_bounds__(64) void contract_kernel(const ContractParams P) {
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const long long slab = blockIdx.x;
    const long long k_lo = slab * P.slab, k_hi = min(P.G, k_lo + P.slab);
    const long long t0 = (P.tile0 + blockIdx.y) * TM;
    const int nxt = (P.xc + XT - 1) / XT;
    // (a row past the end of its tile: the last valid row once more; its results are not stored)
    const long long ta = min(t0 + r, (long long)P.T - 1);
    const int xr_last = min((nxt - 1) * XT + r, P.xc - 1) - (nxt - 1) * XT;
    const double *pa = P.post + ta * P.G + k_lo + RUN * q;
    const double *pb = P.rows + (long long)r * P.G + k_lo + RUN * q;
    const double *pb_last = P.rows + (long long)xr_last * P.G + k_lo + RUN * q;
    const long long xstride = (long long)XT * P.G;

    d4 acc[NXT];
#pragma unroll
    for (int xt = 0; xt < NXT; ++xt) acc[xt] = d4{0.0, 0.0, 0.0, 0.0};

    long long k = k_lo;
    if (P.wide)
        for (; k + KSTEP <= k_hi; k += KSTEP, pa += KSTEP, pb += KSTEP, pb_last += KSTEP) contract_step<true, true>(acc, pa, pb, pb_last, xstride, nxt, 0);
    else
        for (; k + KSTEP <= k_hi; k += KSTEP, pa += KSTEP, pb += KSTEP, pb_last += KSTEP) contract_step<true, false>(acc, pa, pb, pb_last, xstride, nxt, 0);
    // the ragged end of the slab (of the grid): cells at or beyond k_hi count as zero in both operands
    if (k < k_hi) contract_step<false, false>(acc, pa, pb, pb_last, xstride, nxt, k_hi - (k + RUN * q));

    // D: register g of lane (r, q) is P[t0 + q + 4 g][xt * XT + r]
    double *out = P.part + slab * (long long)P.T * P.xc;
#pragma unroll
    for (int xt = 0; xt < NXT; ++xt) {
        if (xt < nxt) {
            const int x = xt * XT + r;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long long t = t0 + q + 4 * g;
                if (t < P.T && x < P.xc) out[t * P.xc + x] = acc[xt][g];
            }
        }
    }
}

// out[t][col0 + x] = sum over the slabs, in ascending order, of part[slab][t][x];  one thread per (t, x) of the chunk
static __global__ __launch_bounds__(256) void combine_kernel(const double *part, double *out, int n_slabs, long long T, int xc, long long out_stride,
                                                      long long col0) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, n = T * xc;
    if (e >= n) return;
    double s = part[e];
    for (int k = 1; k < n_slabs; ++k) s += part[(long long)k * n + e];
    const long long t = e / xc, x = e - t * xc;
    out[t * out_stride + col0 + x] = s;
}

// out[c] = (sum_t p[t][c]) / T with the sum compensated (Neumaier): the result carries the rounding of the sum and of the division, not T
static __global__ __launch_bounds__(256) void average_rows_kernel(const double *p, double *out, long long G, int T) {
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < G; c += (long long)gridDim.x * 256) {
        double s = 0.0, comp = 0.0;
        for (int t = 0; t < T; ++t) {
            const double v = p[(long long)t * G + c];
            const double u = s + v;
            comp += fabs(s) >= fabs(v) ? (s - u) + v : (v - u) + s;
            s = u;
        }
        out[c] = (s + comp) / (double)T;
    }
}

// Likelihood rows of the two models whose fit evaluates the likelihood inside the step kernels: rows[j][cell] = pdf(grid, [x_j]),
// observationModels.py restated operation by operation (no contraction of a product into the following sum).
//   om 2 Gaussian (:101-103): exp(-((x - mean) ** 2) / (2 std ** 2) - .5 log(2 pi std ** 2))
//   om 1 Poisson  (:78-80):   rate ** k * exp(-rate) / k!,   k! as a double from the host (kfact)
// grid = (blocks over the cells, x values of the chunk)
static __global__ __launch_bounds__(256) void tabulate_rows_kernel(int om, double *rows, long long G, int n1, const double *m0, const double *m1,
                                                            const double *x, const double *kfact) {
#pragma clang fp contract(off)
    const long long j = blockIdx.y;
    const double xj = x[j];
    double *row = rows + j * G;
    if (om == 2) {
        for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < G; c += (long long)gridDim.x * 256) {
            const double mu = m0[c / n1], s = m1[c % n1];
            const double d = xj - mu, s2 = s * s;
            row[c] = exp(-(d * d) / (2.0 * s2) - 0.5 * log((2.0 * M_PI) * s2));
        }
    } else {
        const double kf = kfact[j];
        for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < G; c += (long long)gridDim.x * 256) {
            const double rate = m1[c];
            row[c] = pow(rate, xj) * exp(-rate) / kf;
        }
    }
}

}   // namespace blpp
#endif
