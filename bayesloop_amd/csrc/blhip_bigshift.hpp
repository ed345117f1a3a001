// The large-shift stage of 2-D grids: a Deterministic model that moves the distribution by more than 12 grid cells in one time step
// (transitionModels.py:559-606 -> scipy.ndimage.shift(order = 3, mode = 'nearest'), then a renormalisation).  Beyond its 12 pre-padded
// samples SciPy extends the spline COEFFICIENTS by their edge values, which no shift-invariant stencil reproduces (blhip_program.hpp:
// TapTable::get_bigshift): every line along the shifted axis is prefiltered as a whole and the cubic B-spline is evaluated at the shifted
// coordinates with the coefficient index clamped -- what the `big1` branch of blk::step_kernel does for the one row of a 1-D grid
// (oracle/bl_oracle.py: spline_shift_nearest).
//
// One STAGE of a composed transition (DESIGN.md "Composed transitions"): transition only, input scale and block partials in the stage
// contract of blk::step_kernel's stage modes, so that the next stage or the fused step kernel consumes its output without knowing which
// kernel produced it.  grid = (nbb, B), block = 256; a block takes L = ceil(lines / nbb) ADJACENT lines, line-major in LDS:
//     c[L][pitch] doubles + 16 of scratch; the pitch (bigshift_pitch) spreads the lanes of a half-wave over the 64 LDS banks.
// AXIS = 1: lines are rows (contiguous); a wave loads, prefilters and evaluates its own lines.  AXIS = 0: lines are columns (stride n1); the
// block's L adjacent columns make every row read and every row written ONE contiguous segment of L doubles.
// A chain whose stage is not a large shift along AXIS is not this kernel's: its blocks return at once.  Block k writes slot k of the
// chain's [NRED][nblk] partials (nbb <= nblk: launch_bigshift), block 0 zeroes the slots behind nbb.
#pragma once

namespace blk {

constexpr int BIGSHIFT_MAX_LINE = 16384;  // points along the shifted axis: one padded line has to fit into a CU's LDS

// doubles from one line of N = n + 24 coefficients to the next in LDS.  The prefilter's lanes stay inside ONE line (odd chunks: spline_chunk).
// AXIS 1 loads and samples line by line as well: any pitch, odd.  AXIS 0: the 32 lanes of a half-wave cover Lp = 2^s columns x 32 / Lp
// consecutive positions, addresses column * pitch + position -- with pitch = 32 / Lp (mod 32) they fall into 32 different 8-byte bank pairs.
__host__ __device__ __forceinline__ int bigshift_pitch(int N, int L, int axis) {
    if (axis == 1) return N | 1;
    int Lp = 1;
    while (Lp < L) Lp <<= 1;
    const int r = Lp >= 32 ? 1 : 32 / Lp;
    return N + ((r - N) & 31);
}

template <int AXIS, bool BWD>
__global__ __launch_bounds__(NTHREADS) void bigshift_kernel(const StepParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.y;
    const int tp = AXIS == 0 ? P.tap0[b] : P.tap1[b];
    if ((P.cmode[b] & 15) != 6 || tp < 0 || P.tap_lw2[tp] != BIGSHIFT_LW2) return;       // (another kernel's chain)
    const int n = AXIS == 0 ? P.n0 : P.n1, lines = AXIS == 0 ? P.n1 : P.n0;
    const int nbb = gridDim.x, blk = blockIdx.x;
    const int L = (lines + nbb - 1) / nbb;
    const int l0 = blk * L, nl = max(0, min(L, lines - l0));
    const int N = n + 24, pitch = bigshift_pitch(N, L, AXIS);
    double *c = lds;
    double *red = lds + (size_t)L * pitch;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int sh = L > 1 ? 32 - __clz(L - 1) : 0, Lp = 1 << sh;       // AXIS 0: a thread's (position, column) = (idx >> sh, idx & (Lp - 1))

    const int kind = P.srckind[b];
    const double *src = kind == SRC_PREV ? P.src + (long long)b * P.src_stride : P.shared[kind];
    // the scale a stage reads its input in (blk::step_kernel): the producer's lazy normaliser; backward the clamp bookkeeping's slot 5
    double scale = 1.0;
    if (kind == SRC_PREV)
        scale = 1.0 / sum_partials(P.psum_prev + ((long long)b * NRED + (BWD ? 5 : P.prev_slot)) * P.prev_nblk, P.prev_nblk, red);
    const double d = P.taps[P.tap_off[tp]];

    // ---- 1: the lines, extended by SciPy's 12 edge samples per side, times the prefilter's gain -> LDS ---------------------------------
    if (AXIS == 1) {
        for (int l = w; l < nl; l += NTHREADS / 64) {
            const double *row = src + (long long)(l0 + l) * P.n1;
            for (int q = lane; q < N; q += 64) c[(size_t)l * pitch + q] = SPLINE_GAIN * row[min(max(q - 12, 0), n - 1)];
        }
    } else {
        for (int idx = threadIdx.x; idx < (N << sh); idx += NTHREADS) {
            const int q = idx >> sh, l = idx & (Lp - 1);
            if (l < nl) c[(size_t)l * pitch + q] = SPLINE_GAIN * src[(long long)min(max(q - 12, 0), n - 1) * P.n1 + l0 + l];
        }
    }
    __syncthreads();
    // ---- 2: spline coefficients of every padded line by SciPy's recursion, one wave per line -------------------------------------------
    {
        const SplineK K = spline_k_compute(N, lane);
        for (int l = w; l < nl; l += NTHREADS / 64) spline_prefilter_wave(c + (size_t)l * pitch, N, lane, K);
    }
    __syncthreads();
    // ---- 3: the B-spline at the shifted coordinates, coefficient index clamped (the operation order of blk::step_kernel's big1 branch) --
    double sU = 0.0, sMax = 0.0;
    auto sample = [&](int l, int i) {
        const double *cl = c + (size_t)l * pitch;
        const double pp = (double)i - d + 12.0;                      // sampled coordinate in the padded line
        const double fl = floor(pp);
        const int k0 = (int)fmax(fmin(fl, 1.0e9), -1.0e9);
        double o = 0.0;
        for (int dk = -1; dk <= 2; ++dk) {
            const double a = fabs(pp - (fl + (double)dk));
            const double b3 = a < 1.0 ? 2.0 / 3.0 - a * a + a * a * a * 0.5 : (a < 2.0 ? (2.0 - a) * (2.0 - a) * (2.0 - a) / 6.0 : 0.0);
            const long long kk = (long long)k0 + dk;
            o = fma(b3, cl[kk < 0 ? 0 : (kk > N - 1 ? N - 1 : (int)kk)], o);
        }
        const double u = o * scale;                                  // the stage's output in the reference's scale
        sU += u;
        sMax = fmax(sMax, u);
        return u;
    };
    double *dst = P.dst + (long long)b * P.dst_stride;
    if (AXIS == 1) {
        for (int l = w; l < nl; l += NTHREADS / 64)
            for (int i = lane; i < n; i += 64) dst[(long long)(l0 + l) * P.n1 + i] = sample(l, i);
    } else {
        for (int idx = threadIdx.x; idx < (n << sh); idx += NTHREADS) {
            const int i = idx >> sh, l = idx & (Lp - 1);
            if (l < nl) dst[(long long)i * P.n1 + l0 + l] = sample(l, i);
        }
    }
    // ---- partials: a Deterministic stage renormalises by D = sum u (slots 0 and 5); slot 2 = sum u; slot 6 = max u -----------------------
    double *out = P.psum_out + (long long)b * NRED * P.nblk;
    const double D = block_sum(sU, red);
    const double mx = block_max(sMax, red);
    if (threadIdx.x == 0) { out[blk] = D; out[2 * P.nblk + blk] = D; out[5 * P.nblk + blk] = D; out[6 * P.nblk + blk] = mx; }
    if (blk == 0)
        for (int k = nbb + threadIdx.x; k < P.nblk; k += NTHREADS) { out[k] = 0.0; out[2 * P.nblk + k] = 0.0; out[5 * P.nblk + k] = 0.0; out[6 * P.nblk + k] = 0.0; }
}

}  // namespace blk
