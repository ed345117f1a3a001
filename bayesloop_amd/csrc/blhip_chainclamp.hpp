// RegimeSwitch inside the chain-resident kernel on two-parameter grids: blc::chain_clamp_kernel, the clamp flavour of the one-axis
// blc::chain_kernel (blhip_chainres.hpp: column strips of 16 columns x all rows, the state in LDS for a whole pass, bands on the fp64 matrix
// pipe, the Gaussian likelihood by recurrence).  What differs:
//
//  * a step of blc::chain_kernel is linear in its input, so it divides by a normaliser that is `lag` steps old and nobody waits for a sum.
//    A RegimeSwitch (transitionModels.py:405-410) is not linear: it raises every cell of the NORMALISED distribution below `limit` to
//    `limit`.  In the state's units the threshold is limit x (the chain's sum over ALL strips at the step before): a clamped step waits
//    for the granules of the step before it from every strip of its chain -- the scale wave reads them (bounded spin, abort word: exactly
//    the lagged wait's), adds them in its one fixed order (every strip of a chain forms the same bits) and hands the sum to the block
//    through LDS and one more barrier.  A step in mode 0 does not wait;
//  * forward the sum is the granule blc::chain_kernel publishes (sum slot 0).  Backward the reference clamps beta_norm L
//    (core.py:467): the threshold is limit x sum(beta) of the step before, which is NOT the published sum of beta L -- the backward
//    passes publish a second granule per step, the sum of beta (sum slot 5: what blk::step_kernel reports there), in the unused half of
//    the granule buffer (the half the two-chain fold kernel's rounds would use);
//  * a clamped step runs at the EXACT scale (lag 0): s_k = 1 / S_(k-1), the sum of the state of the step before (backward: of beta L, the
//    first granule, read in the same wait) -- the value it has waited for anyway.  The scale wave writes it where the lagged rule reads the scales from, so the steps in mode 0 behind it continue with
//    s_k = S_(k-lag-1) s_(k-lag) / S_(k-lag) whatever mixture of modes the chain runs; chain_unlag (blhip_book.hpp) mirrors the rule;
//  * mode 1 (RegimeSwitch in front of the walk, or alone: NK = 4) clamps the source in LDS (registers: NK = 4) in front of the ring reads
//    -- the wait is exposed; mode 2 (behind the walk) clamps the products, the wait is taken BEHIND the products of all the wave's tiles;
//  * the mass of the clamped distribution (the reference renormalises by it, :410) goes to sum slot 1 forward, in the reference's units;
//    padded cells stay zero and count in no sum.
//
// PAD semantics throughout (a grid that fills its geometry is a padded grid without padding); ring lengths 4 (no stencil), 8 .. 24 in
// steps of 4; <= 512 rows; three passes: forward without storing, forward storing, backward storing.  No restarts, no tabulated
// likelihood, no fold (full hyper-studies store and fold afterwards).
#pragma once
#include "blhip_chainres.hpp"

namespace blc {

struct ClampParams {
    ChainParams C;                // (blc::chain_kernel's argument block, unchanged: geometry, taps, sequences, sums, granules, abort word)
    const unsigned char *cmode;   // [T][B] of the pass's direction: 0 none, 1 RegimeSwitch on the source, 2 RegimeSwitch behind the walk
    const double *limit;          // [T][B] the minimal probability per cell (10^log10pMin x the cell's volume)
};

constexpr int CLAMP_NRED = 6;     // sums per block and step: N, U / S, C, M0, M1, B
template <int NK, int NTW>
constexpr size_t lds_doubles_clamp() { return (size_t)2 * NW * NTW * TM * WCOL + NK * 64 + NW * NTW * TM + 2 * NW * 4 * CLAMP_NRED + NSLOT + 8; }

template <int NK, int NTW, bool BWD, bool STORE>
__global__ __launch_bounds__(NT, 1) void chain_clamp_kernel(const ClampParams PP) {
    static_assert(NTW >= 1 && NTW <= 4, "geometries of 128 .. 512 rows");
    static_assert(NK == 4 || (NK >= 8 && NK <= 24 && NK % 4 == 0), "ring lengths 4 (no stencil), 8 .. 24 in steps of 4");
    static_assert(!BWD || STORE, "the backward pass stores its posteriors");
    const ChainParams &P = PP.C;
    constexpr int R0 = (4 * NK - TM) / 2;
    constexpr int N0 = NW * NTW * TM;
    constexpr int XSZ = N0 * WCOL;
    constexpr bool FILTER = NK > 4;
    const int n0t = P.n0t, n1t = P.n1t;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *const X = lds;                          // [2][N0][16]
    double *const As = X + 2 * XSZ;                 // [NK][64]   A operand: W[m][k] = w(|k - R0 - m|)
    double *const m0s = As + NK * 64;               // [N0]       row coordinates
    double *const red = m0s + N0;                   // [2][NW * 4][CLAMP_NRED] row sums of the waves, double-buffered by step parity
    double *const scal = red + 2 * NW * 4 * CLAMP_NRED;      // [NSLOT] the scales s_j of the steps around the current one
    double *const xs = scal + NSLOT;                // [2] the sums a clamped step has waited for

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cs = blockIdx.x / P.strips, tj = blockIdx.x - cs * P.strips;
    const int b = sldi(P.chain_ids, cs);
    const int tap = sldi(P.tap_id, b);
    const int lw0 = tap >= 0 ? sldi(P.tap_lw, tap) : 0;
    const long long o0 = tap >= 0 ? sldi(P.tap_off, tap) : 0;
    const int gj = tj * WCOL + (lane & 15);
    const long long G = (long long)P.n0 * P.n1;

    // ---- prologue: identity band (the first step consumes its source unfiltered), row coordinates, first source -> LDS -----------------
    if (FILTER) for (int e = tid; e < NK * 64; e += NT) As[e] = band_distance(e, R0) == 0 ? 1.0 : 0.0;
    for (int e = tid; e < N0; e += NT) m0s[e] = P.m0[min(e, n0t - 1)];
    if (tid < NSLOT) scal[tid] = 1.0;
    if (FILTER) for (int e = tid; e < XSZ; e += NT) {
        const int row = e >> 4, col = tj * WCOL + (e & 15);
        X[e] = (row < n0t && col < n1t) ? P.src0[(long long)row * n1t + col] : 0.0;
    }
    const bool colok = gj < n1t;
    const int gjc = min(gj, n1t - 1);
    const double g1 = P.m1[gjc];
    const double cA = P.colA[gjc], cB = P.colB[gjc];
    double *const pchain = P.post + (long long)b * P.post_stride;
    const unsigned rowx8 = P.strip_major ? (unsigned)WCOL * 8u : (unsigned)P.n1 * 8u;
    const unsigned strip0 = P.strip_major ? (unsigned)tj * (unsigned)(P.n0 * WCOL * 8) : (unsigned)tj * (unsigned)(WCOL * 8);
    const int row0 = wv * (NTW * TM);
    auto fresh_lane = [&]() { int l = lane; asm volatile("" : "+v"(l)); return l; };
    auto cell_off = [&](int l, int it, int r) { return __umul24(row0 + it * TM + (l >> 4) + 4 * r, rowx8) + strip0 + (unsigned)(l & 15) * 8u; };

    const int t_first = BWD ? P.T - 1 : 0;
    double xd[DMAX], xn[DMAX];
#pragma unroll
    for (int q = 0; q < DMAX; ++q) xd[q] = q < P.d ? P.rec[(long long)t_first * P.rec_len + q] : __builtin_nan("");
    double al[BWD ? NTW : 1][4];                    // backward: the stored alpha of the lane's cells, requested a whole step ahead
    if (BWD) {
#pragma unroll
        for (int it = 0; it < NTW; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) al[BWD ? it : 0][r] = blm::ld32(pchain + (long long)t_first * G, cell_off(lane, it, r));
    }
    double stt[FILTER ? 1 : NTW][4];                // NK = 4: the state of the lane's cells never leaves its registers
    if (!FILTER) {
#pragma unroll
        for (int it = 0; it < NTW; ++it)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + it * TM + (lane >> 4) + 4 * r;
                const bool in = row < n0t && colok;
                stt[it][r] = in ? P.src0[in ? (long long)row * n1t + gj : 0] : 0.0;
            }
    }
    if (wv == SCALE_WAVE || wv == 5 || wv == 0 || wv == NW - 1) __builtin_amdgcn_s_setprio(2);
    bool dead = false;
    typedef const double __attribute__((address_space(3))) *lds_cp;
    unsigned long long gq0 = 0ull, gq1 = 0ull;
    double Sprev = 1.0;
    double mq = 1.0, iq = 1.0, dn_prev = -1.0;
    int nq = 0;
    constexpr bool ANCT = FILTER;                   // (the anchors of the likelihood recurrence come out of the fit's table: ChainParams::anch)
    AnchorEntry anc{1.0, 1.0, 0.0, 0.0};
    if constexpr (ANCT) anc = anchor_load(P.anch, t_first, wv, P.strips, tj, lane);
    // the granules a clamped step waits for: forward the sums blc::chain_kernel publishes, backward the second set (sums of beta)
    unsigned long long *const gran_x = P.gran + (BWD ? (((long long)NSLOT * P.nslots * P.strips) << 1) : 0ll);
    int cm_n = 0;                                   // clamp mode and limit of the step in flight (the first step of a pass has no transition)
    double lim_n = 0.0;
    __syncthreads();
    constexpr bool HOISTA = FILTER && NTW >= 2 && NK <= (BWD ? 20 : 24);
    double Aw[(HOISTA && NK > 3) ? NK - 3 : 1];

    // the sums of step k - 1 from every strip of the chain -> xs[0] (what the threshold is made of: forward the sum of the state, backward
    // the sum of beta) and xs[1] (what the step divides by: the sum of the state in both directions -- backward the sum of beta L, so
    // that the new beta sums to the clamped distribution's mass, >= 1, as the reference's normalised beta does: a scale of
    // 1 / sum(beta) left it smaller by sum(beta L) / sum(beta), and the stored posteriors that much closer to the subnormal range);
    // every wave of the block leaves with them
    auto wait_sums = [&](int k) {
        if (wv == SCALE_WAVE) {
            const unsigned long long want = (unsigned long long)(unsigned)k;
            const bool mine = lane < P.strips;
            const long long gofs = (((long long)((k - 1) & (NSLOT - 1)) * P.nslots + cs) * P.strips + (mine ? lane : 0)) << 1;
            const unsigned long long *ge = gran_x + gofs, *gc = P.gran + gofs;
            unsigned long long q0 = 0ull, q1 = 0ull, c0 = 0ull, c1 = 0ull;
            bool ok = !mine;
            auto fetch = [&]() {
                q0 = blr::ld_u64(ge); q1 = blr::ld_u64(ge + 1);
                if (BWD) { c0 = blr::ld_u64(gc); c1 = blr::ld_u64(gc + 1); } else { c0 = q0; c1 = q1; }
                ok = (q0 >> 32) == want && (q1 >> 32) == want && (c0 >> 32) == want && (c1 >> 32) == want;
            };
            if (!dead) {
                if (mine) fetch();
                if (!__all(ok)) {
                    const unsigned long long t0 = blr::now_ticks();
                    for (unsigned spins = 1; !__all(ok); ++spins) {
                        if (!ok) fetch();
                        blr::nap();
                        if ((spins & 255u) == 0u) {
                            if (blr::ld_flag(P.abort_word) != 0u) { dead = true; break; }
                            if (blr::now_ticks() - t0 > P.timeout_ticks) { blr::st_flag(P.abort_word, 1u); dead = true; break; }
                        }
                    }
                }
            }
            const double v = (mine && !dead) ? __longlong_as_double((long long)((q0 & 0xffffffffull) | (q1 << 32))) : 0.0;
            const double vc = (mine && !dead) ? __longlong_as_double((long long)((c0 & 0xffffffffull) | (c1 << 32))) : 0.0;
            const double Sg = blk::wave_sum(v);
            const double Sc = BWD ? blk::wave_sum(vc) : Sg;
            if (lane == 0) {
                xs[0] = dead ? 1.0 : Sg;
                xs[1] = dead ? 1.0 : Sc;
                scal[k & (NSLOT - 1)] = dead ? 1.0 : 1.0 / Sc;          // the exact scale, where the lagged rule of later steps reads it
            }
        }
        __syncthreads();
        return xs[0];
    };

    for (int k = 0; k < P.T; ++k) {
        const int t = BWD ? P.T - 1 - k : k;
        const int tn = (k + 1 < P.T) ? (BWD ? t - 1 : t + 1) : t;
        const int cm = cm_n;
        const double lim = lim_n;
        if (k + 1 < P.T) {
            cm_n = __builtin_amdgcn_readfirstlane((int)PP.cmode[(long long)tn * P.B + b]);
            lim_n = PP.limit[(long long)tn * P.B + b];
        }
        // ---- the scale wave: the lagged sums of the steps in mode 0 (blc::chain_kernel's rule) ---------------------------------------------
        const bool scale_wave = wv == SCALE_WAVE;
        const int jn = k + 1;
        const bool need = scale_wave && jn >= P.lag && jn < P.T;
        const unsigned long long *gp = P.gran + ((((long long)((jn - P.lag) & (NSLOT - 1)) * P.nslots + cs) * P.strips + lane) << 1);
        const bool mine = need && lane < P.strips;
        const unsigned long long hq0 = gq0, hq1 = gq1;
        if (scale_wave && jn + 1 >= P.lag && jn + 1 < P.T && lane < P.strips) {
            const unsigned long long *gn = P.gran + ((((long long)((jn + 1 - P.lag) & (NSLOT - 1)) * P.nslots + cs) * P.strips + lane) << 1);
            gq0 = blr::ld_u64(gn); gq1 = blr::ld_u64(gn + 1);
        }
        double *const pnext = pchain + (long long)tn * G;
#pragma unroll
        for (int q = 0; q < DMAX; ++q) xn[q] = q < P.d ? P.rec[(long long)tn * P.rec_len + q] : __builtin_nan("");
        AnchorEntry anc_next{1.0, 1.0, 0.0, 0.0};
        if constexpr (ANCT) anc_next = anchor_load(P.anch, tn, wv, P.strips, tj, fresh_lane());

        double *S = X + (k & 1) * XSZ;
        double *D = X + ((k + 1) & 1) * XSZ;
        double Sx = 1.0, thr = 0.0, sU = 0.0;
        // ---- mode 1: RegimeSwitch on the source (in front of the walk, or alone) ------------------------------------------------------------
        if (cm == 1) {
            Sx = wait_sums(k);
            thr = lim * Sx;
            const int l = fresh_lane(), g = l >> 4, c = l & 15;
#pragma unroll
            for (int it = 0; it < NTW; ++it)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int li = row0 + it * TM + g + 4 * r;
                    const bool in = colok && li < n0t;
                    double v = FILTER ? S[li * WCOL + c] : stt[FILTER ? 0 : it][r];
                    v = in ? (v < thr ? thr : v) : 0.0;
                    if (FILTER) S[li * WCOL + c] = v; else stt[FILTER ? 0 : it][r] = v;
                    sU += v;
                }
            if (FILTER) __syncthreads();
        }

        // ---- ring over the source state, banded products of all the wave's tiles -----------------------------------------------------------
        const bool edge = row0 < R0 || row0 + NTW * TM + R0 > n0t;          // (the reflection is at the grid's true last row)
        constexpr bool WHOLE_RING = FILTER && !BWD;
        constexpr int NRING = WHOLE_RING ? NK + 4 * (NTW - 1) : NK;
        double Bv[NRING];
        if (FILTER) {
            const int l = fresh_lane(), g = l >> 4, c = l & 15;
            if (edge) {
#pragma unroll
                for (int kb = 0; kb < NRING; ++kb) Bv[kb] = S[reflect1(row0 - R0 + 4 * kb + g, n0t) * WCOL + c];
            } else {
                const double *s0 = S + (row0 - R0 + g) * WCOL + c;
#pragma unroll
                for (int kb = 0; kb < NRING; ++kb) Bv[kb] = s0[kb * 4 * WCOL];
            }
        }
        if (HOISTA && k <= 1) {
            const int l = fresh_lane();
            lds_cp Al = (lds_cp)((const char __attribute__((address_space(3))) *)(lds_cp)As + (unsigned)l * 8u);
#pragma unroll
            for (int q = 0; q < NK - 3; ++q) Aw[q] = Al[q * 64];
        }
        d4 accs[NTW];
#pragma unroll
        for (int it = 0; it < NTW; ++it) {
            const int i = row0 + it * TM;
            const int l = fresh_lane(), g = l >> 4, c = l & 15;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            if (!FILTER) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = stt[FILTER ? 0 : it][r];
            } else {
                lds_cp Al = (lds_cp)((const char __attribute__((address_space(3))) *)(lds_cp)As + (unsigned)l * 8u);
                if constexpr (WHOLE_RING && HOISTA) {
                    acc = it == 0 ? band_products_w<NK, 0, NRING>(Aw, Bv) : (it == 1 ? band_products_w<NK, (NTW > 1 ? 4 : 0), NRING>(Aw, Bv) :
                          (it == 2 ? band_products_w<NK, (NTW > 2 ? 8 : 0), NRING>(Aw, Bv) : band_products_w<NK, (NTW > 3 ? 12 : 0), NRING>(Aw, Bv)));
                } else if constexpr (WHOLE_RING) {
                    acc = it == 0 ? band_products<NK, 0, NRING, 64>(Al, Bv) : (it == 1 ? band_products<NK, (NTW > 1 ? 4 : 0), NRING, 64>(Al, Bv) :
                          (it == 2 ? band_products<NK, (NTW > 2 ? 8 : 0), NRING, 64>(Al, Bv) : band_products<NK, (NTW > 3 ? 12 : 0), NRING, 64>(Al, Bv)));
                } else if constexpr (HOISTA) {
                    acc = band_products_w<NK, 0, NK>(Aw, Bv);
                } else {
                    acc = band_products<NK, 0, NK, 64>(Al, Bv);
                }
            }
            accs[it] = acc;
            // advance the sliding ring by one tile
            if (FILTER && !WHOLE_RING && it + 1 < NTW) {
#pragma unroll
                for (int kb = 0; kb < NK - 4; ++kb) Bv[kb] = Bv[kb + 4];
                if (edge) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) Bv[NK - 4 + q] = S[reflect1(i + TM + R0 + 4 * q + g, n0t) * WCOL + c];
                } else {
                    const double *s1 = S + (i + TM + R0 + g) * WCOL + c;
#pragma unroll
                    for (int q = 0; q < 4; ++q) Bv[NK - 4 + q] = s1[q * 4 * WCOL];
                }
            }
        }

        // ---- the scale of this step; the scale wave prepares the next step's lagged one ------------------------------------------------------
        double scale = scal[k & (NSLOT - 1)];
        if (scale_wave) {
            double sj = 1.0;
            if (need) {
                const unsigned long long want = (unsigned long long)(unsigned)(jn - P.lag + 1);
                unsigned long long q0 = hq0, q1 = hq1;
                bool ok = !mine || ((q0 >> 32) == want && (q1 >> 32) == want);
                if (!dead && !__all(ok)) {
                    const unsigned long long t0 = blr::now_ticks();
                    for (unsigned spins = 1; !__all(ok); ++spins) {
                        if (!ok) { q0 = blr::ld_u64(gp); q1 = blr::ld_u64(gp + 1); ok = (q0 >> 32) == want && (q1 >> 32) == want; }
                        blr::nap();
                        if ((spins & 255u) == 0u) {
                            if (blr::ld_flag(P.abort_word) != 0u) { dead = true; break; }
                            if (blr::now_ticks() - t0 > P.timeout_ticks) { blr::st_flag(P.abort_word, 1u); dead = true; break; }
                        }
                    }
                }
                const double v = mine ? __longlong_as_double((long long)((q0 & 0xffffffffull) | (q1 << 32))) : 0.0;
                const double Sg = blk::wave_sum(v);
                sj = dead ? 1.0 : Sprev * scal[(jn - P.lag) & (NSLOT - 1)] / Sg;
                Sprev = Sg;
            }
            if (lane == 0) scal[jn & (NSLOT - 1)] = sj;
        }
        // ---- mode 2: RegimeSwitch behind the walk -- the wait comes behind the products --------------------------------------------------------
        if (cm == 2) { Sx = wait_sums(k); thr = lim * Sx; }
        if (cm != 0) scale = 1.0 / xs[1];             // (bit for bit what the scale wave has written to scal[k])

        // ---- anchors of the stride-4 likelihood recurrence of this lane's rows (blc::chain_kernel's) ------------------------------------------
        double mE = 1.0, mR = 1.0, iE = 1.0, iR = 1.0;
        int nE = 0, nR = 0;
        {
            const int l = fresh_lane(), g = l >> 4;
            double dn;
            if constexpr (ANCT) {
                anchor_unpack(anc, mE, nE, mR, nR);
                dn = anc.dn;
            } else {
                double a0, d1;
                anchor_terms(xd[0], xd[1], xd[2], xd[3], m0s[row0 + g], m0s[row0 + g + 4], cA, cB, a0, d1, dn);
                exp_mn(a0, mE, nE);
                exp_mn(d1, mR, nR);
            }
            if (dn != dn_prev) {
                const double d2 = -32.0 * cA * dn * P.step0 * P.step0;
                int tmp;
                exp_mn(d2, mq, nq);
                if (BWD) exp_mn(-d2, iq, tmp);
                dn_prev = dn;
            }
            if (BWD) { iE = blmath::inv_m(mE); iR = blmath::inv_m(mR); }
            else mE *= scale;
        }

        // ---- epilogue ---------------------------------------------------------------------------------------------------------------------------
        double sN = 0.0, sS = 0.0, sC = 0.0, sM0 = 0.0, sM1 = 0.0, sB = 0.0;
        double *const pstep = pchain + (long long)t * G;
#pragma unroll
        for (int it = 0; it < NTW; ++it) {
            const int i = row0 + it * TM;
            const int l = fresh_lane(), g = l >> 4, c = l & 15;
            d4 acc = accs[it];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = i + g + 4 * r;
                const bool in = colok && li < n0t;                         // (cells outside the grid stay zero and out of every sum)
                const double Lv = ldexp(mE, nE);
                const unsigned off = cell_off(l, it, r);
                double u = in ? acc[r] : 0.0;
                if (cm == 2) { u = in ? (u < thr ? thr : u) : 0.0; sU += u; }
                if (!BWD) {
                    const double a = u * Lv;
                    if (FILTER) D[li * WCOL + c] = a; else stt[FILTER ? 0 : it][r] = a;
                    if (STORE) stnt(pstep, off, a);
                    sN += a;
                    acc[r] = a;
                } else {
                    const double beta = u * scale;
                    const double p = al[BWD ? it : 0][r] * beta;
                    const double cn = beta * Lv;
                    const double pl = !in ? 0.0 : nan_if(Lv == 0.0, ldexp(p * iE, -nE));
                    if (FILTER) D[li * WCOL + c] = cn; else stt[FILTER ? 0 : it][r] = cn;
                    stnt(pstep, off, p);
                    sN += p;
                    sS += pl;
                    sC += cn;
                    sB += beta;
                    acc[r] = p;
                }
                mE *= mR; nE += nR;
                mR *= mq; nR += nq;
                if (BWD) { iE *= iR; iR *= iq; }
            }
            if (BWD) {
#pragma unroll
                for (int r = 0; r < 4; ++r) al[BWD ? it : 0][r] = ldnt(pnext, cell_off(l, it, r));
            }
            if ((BWD || STORE) && P.means) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { sM0 = fma(acc[r], m0s[i + g + 4 * r], sM0); sM1 = fma(acc[r], g1, sM1); }
            }
        }

        // ---- sums: waves -> LDS; behind the barrier wave 5 adds them up, writes the strip's partial sums and publishes the granules -----------
        // forward: N, U (the clamped distribution's mass in the reference's units), M0, M1; backward: N, S, C, M0, M1, B (the sum of beta)
        const double v[CLAMP_NRED] = {sN, BWD ? sS : sU * scale, BWD ? sC : sM0, BWD ? sM0 : sM1, BWD ? sM1 : 0.0, BWD ? sB : 0.0};
        constexpr int NV = BWD ? 6 : 4;
        double *rk = red + (k & 1) * (NW * 4 * CLAMP_NRED);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            double x = v[q];
            x = blk::dpp_add<0x111, 0xf>(x);
            x = blk::dpp_add<0x112, 0xf>(x);
            x = blk::dpp_add<0x114, 0xf>(x);
            x = blk::dpp_add<0x118, 0xf>(x);
            if ((lane & 15) == 15) rk[(wv * 4 + (lane >> 4)) * CLAMP_NRED + q] = x;
        }
        __syncthreads();
        if (FILTER && k == 0) {            // the chain's band replaces the identity of the first step
            for (int e = tid; e < NK * 64; e += NT) {
                const int a = band_distance(e, R0);
                As[e] = a == 0 ? (lw0 > 0 ? P.taps[o0] : 1.0) : (a <= lw0 ? P.taps[o0 + a] : 0.0);
            }
            __syncthreads();
        }
        if (wv == 5 && lane < NV) {
            double tot = 0.0;
#pragma unroll
            for (int w = 0; w < NW * 4; ++w) tot += rk[w * CLAMP_NRED + lane];
            const int slot = BWD ? lane : (lane < 2 ? lane : lane + 1);                          // forward: N, U, M0, M1 -> slots 0, 1, 3, 4
            const bool wanted = BWD ? (lane < 3 || lane == 5 || P.means != 0) : (lane == 0 || (lane == 1 ? cm != 0 : P.means != 0));
            if (wanted) P.psum[(((long long)t * P.B + b) * NRED + slot) * P.nblk + tj] = tot;
            if (lane == (BWD ? 2 : 0) || (BWD && lane == 5)) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(tot);
                const unsigned long long tag = (unsigned long long)(unsigned)(k + 1) << 32;
                unsigned long long *gw = (BWD && lane == 5 ? gran_x : P.gran) + ((((long long)(k & (NSLOT - 1)) * P.nslots + cs) * P.strips + tj) << 1);
                blr::st_u64(gw, tag | (bits & 0xffffffffull));
                blr::st_u64(gw + 1, tag | (bits >> 32));
            }
        }
#pragma unroll
        for (int q = 0; q < DMAX; ++q) xd[q] = xn[q];
        if constexpr (ANCT) anc = anc_next;
    }
}

}   // namespace blc
