// Renormalising stages of the plain N-D path (blhip_nd.hpp): NotEqual (transitionModels.py:462-471) and Deterministic
// (transitionModels.py:571-602) on grids with 3 and 4 parameters.  A stage sits in the list of a step's passes like a random walk's
// filter_axis_kernel: blockIdx.y = chain of the batch, srcs[b] = where chain b's input lives, dst = [B][G].  Both maps are invariant
// to the scale of their input and end with a division by the sum of their output, which stays lazy: a stage writes u and the
// per-block partial sums of u into slot 0 of `sums` ([B][NRED][nblk], the layout of a step's partial sums), and the fused
// bln::step_kernel reads 1 / sum u as its scale exactly as it reads a producing step's slot.
// Chains of one batch differ in what they do at a step (other segments of a serial model, a restart): a chain without the stage
// (id[b] < 0) passes through BY COPY -- its values, and the partial sums its scale is read from (sums_in, slot_in) -- so that the
// kernels behind it need no per-chain special case.  Every launch has gridDim.x == nblk.
#pragma once
#include "blhip_nd.hpp"

namespace bln {

// NotEqual, pass 1 of 3: block maxima of the chains that run the stage  (bmax: [B][nblk])
static __global__ __launch_bounds__(NTHREADS) void ne_max_kernel(const double *const *srcs, long long G, const int *id, double *bmax) {
    __shared__ double red[NTHREADS / 64 + 1];
    const int b = blockIdx.y;
    if (id[b] < 0) return;
    const double *src = srcs[b];
    double m = -INFINITY;
    for (long long e = (long long)blockIdx.x * NTHREADS + threadIdx.x; e < G; e += (long long)gridDim.x * NTHREADS) m = fmax(m, src[e]);
    m = blk::block_max(m, red);
    if (threadIdx.x == 0) bmax[(long long)b * gridDim.x + blockIdx.x] = m;
}

// NotEqual, pass 2 of 3: out = max(x) - x (:465) and the block sums of out -- the first divisor is the sum of the INVERTED values,
// as in the reference (G max - sum x cancels where the distribution is flat)  (bsum: [B][nblk])
static __global__ __launch_bounds__(NTHREADS) void ne_invert_kernel(double *dst, const double *const *srcs, long long G, const int *id,
                                                                    const double *bmax, double *bsum) {
    __shared__ double red[NTHREADS / 64 + 1];
    const int b = blockIdx.y;
    const double *src = srcs[b];
    double *out = dst + (long long)b * G;
    const bool on = id[b] >= 0;
    double mx = 0.0;
    if (on) {
        double m = -INFINITY;
        for (int k = threadIdx.x; k < (int)gridDim.x; k += NTHREADS) m = fmax(m, bmax[(long long)b * gridDim.x + k]);
        mx = blk::block_max(m, red);
    }
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NTHREADS + threadIdx.x; e < G; e += (long long)gridDim.x * NTHREADS) {
        const double v = on ? mx - src[e] : src[e];
        out[e] = v;
        s += v;
    }
    if (!on) return;
    s = blk::block_sum(s, red);
    if (threadIdx.x == 0) bsum[(long long)b * gridDim.x + blockIdx.x] = s;
}

// NotEqual, pass 3 of 3, in place: out /= sum(out); cells below limit = 10**v dV set to it (:466-470); the block sums of the result
static __global__ __launch_bounds__(NTHREADS) void ne_clamp_kernel(double *buf, long long G, const int *id, const double *limit, const double *bsum,
                                                                   const double *sums_in, int slot_in, double *sums) {
    __shared__ double red[NTHREADS / 64 + 1];
    const int b = blockIdx.y, nblk = gridDim.x;
    double *slot = sums + (long long)b * NRED * nblk;
    if (id[b] < 0) {
        if (threadIdx.x == 0) slot[blockIdx.x] = sums_in[((long long)b * NRED + slot_in) * nblk + blockIdx.x];
        return;
    }
    const double total = blk::sum_partials(bsum + (long long)b * nblk, nblk, red);
    const double lim = limit[b];
    double *u = buf + (long long)b * G;
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NTHREADS + threadIdx.x; e < G; e += (long long)gridDim.x * NTHREADS) {
        double v = u[e] / total;
        v = v < lim ? lim : v;
        u[e] = v;
        s += v;
    }
    s = blk::block_sum(s, red);
    if (threadIdx.x == 0) slot[blockIdx.x] = s;
}

// Deterministic: scipy.ndimage.shift(order=3, mode='nearest') of one axis as the cardinal-spline stencil TapTable::get_shift builds
// (2 lw + 1 asymmetric weights, out[i] = sum_m w[m + lw] ext[i + m], accumulated like the generic step kernel does) over the
// extension blk::extend_index(rule 2) gives; the block sums of the result.  id[b]: the tap set of chain b at this step.
static __global__ __launch_bounds__(NTHREADS) void shift_axis_kernel(double *dst, const double *const *srcs, long long G, int n, long long inner,
                                                                     const int *id, const double *taps, const int *tap_off, const int *tap_lw,
                                                                     const double *sums_in, int slot_in, double *sums) {
    __shared__ double red[NTHREADS / 64 + 1];
    const int b = blockIdx.y, nblk = gridDim.x;
    const double *src = srcs[b];
    double *out = dst + (long long)b * G;
    double *slot = sums + (long long)b * NRED * nblk;
    const int tid = id[b];
    if (tid < 0) {
        for (long long e = (long long)blockIdx.x * NTHREADS + threadIdx.x; e < G; e += (long long)gridDim.x * NTHREADS) out[e] = src[e];
        if (threadIdx.x == 0) slot[blockIdx.x] = sums_in[((long long)b * NRED + slot_in) * nblk + blockIdx.x];
        return;
    }
    const int lw = tap_lw[tid];
    const double *w = taps + tap_off[tid] + lw;
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NTHREADS + threadIdx.x; e < G; e += (long long)gridDim.x * NTHREADS) {
        const int i = (int)((e / inner) % n);
        const long long base = e - (long long)i * inner;
        double acc = 0.0;
        for (int m = -lw; m <= lw; ++m) acc = fma(w[m], src[base + (long long)blk::extend_index(i + m, n, 2) * inner], acc);
        out[e] = acc;
        s += acc;
    }
    s = blk::block_sum(s, red);
    if (threadIdx.x == 0) slot[blockIdx.x] = s;
}

}  // namespace bln
