// Chain-resident kernel for chain batches on grids with 3 and 4 parameters: one block per chain of the batch, the chain's distribution in
// LDS for a whole pass, ONE launch per pass (the 1-D counterpart is bl1c::chain1d_kernel, blhip_chain1d.hpp).  The plain path
// (blhip_nd.hpp) launches one filter_axis_kernel per random walk and one step_kernel per time step and direction, each of which moves
// the [B][G] state through HBM / L2; on grids of a few thousand cells that is launch latency and little else.
//
// Blocks never wait for each other: no cooperative launch, no flags, no spin-waits -- a launch cannot hang through co-residency, and a
// batch may hold any number of chains.
//
// Per step the block does what do_fit_nd's `step` does for its chain, in the same per-cell arithmetic:
//   source    SRC_PREV: the LDS state, with the lazy scale 1 / (sum of the step before) applied in the epilogue; any other kind: the shared
//             distribution (prior, reset prior, uniform, Independent's prior) is loaded from global memory, scale 1
//   walks     the program's random walks in list order, each along its axis, ping-pong between the two LDS buffers; centre tap first,
//             then the pairs from the outermost inward (filter_axis_kernel); a pass without a kernel for this chain (sigma = 0, a serial
//             segment that is not active) is skipped -- the plain kernel copies there, which is the same values
//   epilogue  step_kernel's: p = x L, posterior = a_t x, c = x L, the seven sums
// The result differs from the plain path's only through the order in which the normaliser's (and the other sums') partial sums are added.
// Batches with NotEqual or Deterministic passes and resumed / carried fits take the stage flavour of the same body,
// chain_nd_stage_kernel (below).
//
// LDS layout (doubles): buf[2][G] | taps[npass][LWMAX + 1] | grid values of every parameter | red[RED].  Every walk of the program has a
// tap slot of its own; the block stages a slot only when the chain's tap id on that pass CHANGES (a hyper-study's chain keeps its sigma: once
// per pass; a serial model: at its boundaries), so a pass costs one barrier and no global load.  LWMAX is the widest radius of the batch's tap
// table WHATEVER the axis length is -- a walk whose radius exceeds its axis keeps all its taps in LDS (multi-period reflection needs every
// one of them), and a batch whose widest tap set does not fit beside 2 G stays on the plain path.
//
// Latency: a step of a few thousand cells is a few hundred LDS reads per thread, so every global load inside the step's dependency chain
// shows.  The per-step metadata (source kind, the tap ids of all passes: lane q of every wave holds pass q's) is loaded one step ahead; the
// likelihood (and, backward, the stored a_t) of the thread's cells is loaded into registers BEFORE the passes and consumed in the epilogue
// (at most CPT cells per thread: the envelope bounds G by CPT x NT); the grid values of the mean sums come from LDS.
//
// Banks (64 banks x 4 B on gfx950: a double covers two; ds_read_b64 is served half a wave at a time): lanes own consecutive cells e, and
// a neighbour along any axis is e +- j * inner -- the SAME offset for every lane that does not cross a reflecting border.  So a wave reads
// 64 consecutive doubles shifted by a constant, for inner = 1 and for inner a multiple of 32 alike: conflict-free, as the centre read is.
// Lanes that reflect at a border (inner = 1: the lanes within j of a row end; larger inner: whole runs of `inner` lanes) read a second run
// of consecutive addresses; the two runs of one half-wave can overlap in banks, at most a 2-way conflict, for inner = 1 only on the
// half-waves that hold a row end.  The tap weight is one address for the whole wave (broadcast).
#pragma once
#include "blhip_nd.hpp"

namespace bln {

constexpr int CHAIN_ND_NT_SMALL = 256;              // threads of a block whose LDS need lets several blocks share a CU
constexpr int CHAIN_ND_NT_LARGE = 1024;
constexpr size_t CHAIN_ND_SMALL_BYTES = 32 * 1024;  // up to here the small block: 5+ blocks per CU by LDS
constexpr int CHAIN_ND_RED = 7 * (CHAIN_ND_NT_LARGE / 64) + 8;
constexpr int CHAIN_ND_MAXPASS = 8;                 // random walks of a program the kernel's parameter block holds
constexpr size_t CHAIN_ND_LDS_LIMIT = 150 * 1024;   // what the host allows a block elsewhere (plan_geometry)
constexpr int CHAIN_ND_MIN_CHAINS = 16;             // floor of the default route (a condition, not a measurement)

// cells a thread holds the likelihood of in registers: the envelope keeps G <= CPT x NT (256 threads: LDS <= 32 KB -> G <= 1987 <= 8 x 256;
// 1024 threads: LDS <= 150 KB -> G <= 9538 <= 10 x 1024)
constexpr int chain_nd_cpt(int nt) { return nt == CHAIN_ND_NT_SMALL ? 8 : 10; }

// doubles of LDS a block needs: the two state buffers, one tap slot of the batch's widest radius per walk, the grid values of the
// parameters (n_sum = n_0 + .. + n_{d-1}), the reduction scratch
inline size_t chain_nd_lds_doubles(long long G, int lw_max, int npass, long long n_sum) {
    return 2 * (size_t)G + (size_t)(npass < 0 ? 0 : npass) * ((size_t)(lw_max < 0 ? 0 : lw_max) + 1) + (size_t)(n_sum < 0 ? 0 : n_sum) + CHAIN_ND_RED;
}
inline bool chain_nd_fits(long long G, int lw_max, int npass, long long n_sum) {
    return G >= 1 && npass <= CHAIN_ND_MAXPASS && chain_nd_lds_doubles(G, lw_max, npass, n_sum) * sizeof(double) <= CHAIN_ND_LDS_LIMIT;
}
inline int chain_nd_threads(long long G, int lw_max, int npass, long long n_sum) {
    return chain_nd_lds_doubles(G, lw_max, npass, n_sum) * sizeof(double) <= CHAIN_ND_SMALL_BYTES ? CHAIN_ND_NT_SMALL : CHAIN_ND_NT_LARGE;
}
// the largest number of cells the envelope admits beside the taps and the grid values
inline long long chain_nd_max_cells(int lw_max, int npass, long long n_sum) {
    const long long room = (long long)(CHAIN_ND_LDS_LIMIT / sizeof(double)) - (long long)(npass < 0 ? 0 : npass) * ((long long)(lw_max < 0 ? 0 : lw_max) + 1) -
                           (n_sum < 0 ? 0 : n_sum) - CHAIN_ND_RED;
    return room < 2 ? 0 : room / 2;
}
// The cost model of the default route, microseconds per time step and pass direction (profiles/chain_nd_notes.md: fitted to HyperStudy
// full fits at T = 256 against a build of the parent commit).  W = sum over the walks that have a kernel in the batch of (2 x the walk's
// widest radius in the batch + 1): the taps of the batch's slowest chain, which is what a round of blocks waits for.
//   plain path  4.7 per launch (walks + 1) + 0.3 per tap beyond radius 3 (its blocks are bound by the taps' 64-bit index arithmetic)
//               + 27 per million cells of the batch
//   kernel      rounds of blocks x (5 + 0.125 x W per thousand cells), rounds = ceil(B / (CUs x blocks per CU)): 4 blocks of 256
//               threads, 1 of 1024
// The kernel takes a batch of at least CHAIN_ND_MIN_CHAINS chains for which 1.25 x kernel <= plain: the margin keeps the classes that were
// measured slower (8000 and more cells at 16 chains) and their neighbourhood on the plain path.  A batch with a walk whose radius exceeds
// its axis (the multi-period reflection with its integer remainders per tap) stays there too: 16 chains of radius 40 on an axis of 18 ran
// the backward pass 3 % slower than the plain path.
inline double chain_nd_plain_us(long long G, long long B, int walks, int W) {
    const int wide = W - 7 * walks;
    return 4.7 * (walks + 1) + 0.3 * (wide > 0 ? wide : 0) + 27e-6 * (double)B * (double)G;
}
inline double chain_nd_kernel_us(long long G, long long B, int W, int threads, int cus) {
    const long long slots = (long long)(cus < 1 ? 1 : cus) * (threads == CHAIN_ND_NT_SMALL ? 4 : 1);
    return (double)((B + slots - 1) / slots) * (5.0 + 0.125e-3 * (double)W * (double)G);
}
// option chain_nd: 0 off, 1 the cost model, 2 wherever the envelope admits the batch
inline bool chain_nd_route(int option, bool envelope, long long G, long long B, int walks, int W, bool beyond_axis, int threads, int cus) {
    if (!envelope || option == 0) return false;
    if (option >= 2) return true;
    return B >= CHAIN_ND_MIN_CHAINS && !beyond_axis && 1.25 * chain_nd_kernel_us(G, B, W, threads, cus) <= chain_nd_plain_us(G, B, walks, W);
}

// ---- the stage flavour (chain_nd_stage_kernel): batches with NotEqual / Deterministic passes, resumed and carried fits -------------------
enum { CHAIN_ND_WALK = 0, CHAIN_ND_NOTEQUAL = 1, CHAIN_ND_SHIFT = 2 };      // what a pass of the program is

// doubles of one tap slot there: a walk keeps its half kernel (radius + 1), a shift all 2 lw + 1 weights of its asymmetric stencil
// (lw = ceil|d| + 34 <= 46 for the shifts of up to 12 cells the N-D path admits).  NotEqual needs nothing beside the reduction scratch.
inline int chain_nd_stage_slot(int lw_walk, int lw_shift) {
    const int a = (lw_walk < 0 ? 0 : lw_walk) + 1, b = lw_shift > 0 ? 2 * lw_shift + 1 : 0;
    return a > b ? a : b;
}
// doubles of LDS a block needs: as chain_nd_lds_doubles, with one slot of `slot` doubles per pass of the program
inline size_t chain_nd_stage_lds_doubles(long long G, int slot, int npass, long long n_sum) {
    return 2 * (size_t)G + (size_t)(npass < 0 ? 0 : npass) * (size_t)(slot < 1 ? 1 : slot) + (size_t)(n_sum < 0 ? 0 : n_sum) + CHAIN_ND_RED;
}
inline bool chain_nd_stage_fits(long long G, int slot, int npass, long long n_sum) {
    return G >= 1 && npass <= CHAIN_ND_MAXPASS && chain_nd_stage_lds_doubles(G, slot, npass, n_sum) * sizeof(double) <= CHAIN_ND_LDS_LIMIT;
}
inline int chain_nd_stage_threads(long long G, int slot, int npass, long long n_sum) {
    return chain_nd_stage_lds_doubles(G, slot, npass, n_sum) * sizeof(double) <= CHAIN_ND_SMALL_BYTES ? CHAIN_ND_NT_SMALL : CHAIN_ND_NT_LARGE;
}
inline long long chain_nd_stage_max_cells(int slot, int npass, long long n_sum) {
    const long long room = (long long)(CHAIN_ND_LDS_LIMIT / sizeof(double)) - (long long)(npass < 0 ? 0 : npass) * (long long)(slot < 1 ? 1 : slot) -
                           (n_sum < 0 ? 0 : n_sum) - CHAIN_ND_RED;
    return room < 2 ? 0 : room / 2;
}
// The cost model of the stage flavour's default route, in the shape of chain_nd_route's: microseconds per time step and direction, fitted
// to HyperStudy full fits at T = 256 against the plain path (profiles/chain_nd_notes.md).  Over the passes that are on in the batch:
//   filters  walks and shifts (one launch each on the plain path); W: taps of the batch's slowest chain, 2 x radius + 1 per filter
//   sweeps   sweeps over the chain's cells the kernel adds per step: three per NotEqual (its three launches on the plain path: ne_max,
//            ne_invert, ne_clamp), one per shift (the sum of its output); shifts: the shifts among the filters
//   plain path  4.7 per filter and for the fused step kernel + 2.5 per NotEqual launch (small kernels) + 0.3 per tap beyond radius 3
//               + 20 per million cells of the batch
//   kernel      rounds of blocks x (5 (256 threads) or 7 (1024) + (0.125 x W + 0.2 x sweeps) per thousand cells)
// The kernel takes a batch of at least CHAIN_ND_MIN_CHAINS chains WITHOUT a shift for which 1.25 x kernel <= plain: NotEqual alone and
// walk + NotEqual were measured faster on the kernel in every class (1260, 2160, 8000 cells x 16, 64, 256 chains), and so were resumed and
// carried blocks.  A batch with a Deterministic shift that is on stays on the plain path by default: its 2 (ceil|d| + 34) + 1 taps per
// cell were measured slower on the kernel at 1260 cells x 16 and 64 chains and at 8000 cells x 16 and 64 chains (faster at 2160 cells and
// at 256 chains); chain_nd = 2 takes it.
constexpr bool CHAIN_ND_STAGE_MEASURED = true;
inline double chain_nd_stage_plain_us(long long G, long long B, int filters, int W, int sweeps, int shifts) {
    const int wide = W - 7 * filters;
    return 4.7 * (filters + 1) + 2.5 * (sweeps - shifts) + 0.3 * (wide > 0 ? wide : 0) + 20e-6 * (double)B * (double)G;
}
inline double chain_nd_stage_kernel_us(long long G, long long B, int W, int sweeps, int threads, int cus) {
    const long long slots = (long long)(cus < 1 ? 1 : cus) * (threads == CHAIN_ND_NT_SMALL ? 4 : 1);
    return (double)((B + slots - 1) / slots) * ((threads == CHAIN_ND_NT_SMALL ? 5.0 : 7.0) + (0.125e-3 * (double)W + 0.2e-3 * (double)sweeps) * (double)G);
}
// options chain_nd (0 off, 1 the default rule, 2 wherever the envelope admits the batch) and chain_nd_stages (0: such batches keep the
// plain path, 1: they follow chain_nd)
inline bool chain_nd_stage_route(int option, int stages_option, bool envelope, long long G, long long B, int filters, int W, int sweeps, int shifts,
                                 bool beyond_axis, int threads, int cus) {
    if (!envelope || option == 0 || stages_option == 0) return false;
    if (option >= 2) return true;
    if (!CHAIN_ND_STAGE_MEASURED) return false;
    return B >= CHAIN_ND_MIN_CHAINS && shifts == 0 && !beyond_axis &&
           1.25 * chain_nd_stage_kernel_us(G, B, W, sweeps, threads, cus) <= chain_nd_stage_plain_us(G, B, filters, W, sweeps, shifts);
}

struct ChainNd {
    NdGrid g;
    int B, T, npass;
    int pass_n[CHAIN_ND_MAXPASS], pass_inner[CHAIN_ND_MAXPASS];      // the walks' axes: length and cells between neighbours
    int tap_slot;                // LWMAX + 1: doubles of one tap slot (one slot per walk)
    const unsigned char *kind;   // [T][B] source kind of the step
    const int *tap;              // [npass][T][B] tap id of the pass, -1: none
    const double *taps; const int *tap_off, *tap_lw;
    const double *shared[5];     // by source kind: SRC_PRIOR, SRC_RESET, SRC_UNIFORM, SRC_INDEP (0 unused)
    const double *lik;           // (T, G)
    double *post; long long post_stride;       // [B][T][G]: forward: a_t out (null: not kept); backward: a_t in -> posterior out
    double *psum;                // [T][B][NRED] (nblk = 1): the block's totals
    // the stage flavour alone (chain_nd_stage_kernel)
    unsigned char pass_kind[CHAIN_ND_MAXPASS];   // CHAIN_ND_WALK / _NOTEQUAL / _SHIFT
    const double *limit;         // [npass][B] NotEqual's 10**v dV
    const double *carry_in;      // [B][G] resumed fit: what forward step 0 of kind SRC_PREV continues (normalised: tot = 1); null otherwise
    double *carry_out;           // [B][G] carried fit that keeps no sequence: the last forward state, as the sequence would hold it; null otherwise
};

// e / d for 0 <= e < 2^23, d >= 1, with rd ~ 1 / d (two roundings: |rd d - 1| <= 2^-23): e converts exactly, the float product is within
// e / d x 2^-22 + 2^-24 x e / d < 1 of the quotient while the quotient is below 2^22, and the one correction then makes it exact.  Here
// e < G <= 10 240 (launch_chain_nd checks it).
__device__ __forceinline__ int small_div(int e, int d, float rd) {
    int q = (int)((float)e * rd);
    const int r = e - q * d;
    q += r >= d ? 1 : 0;
    q -= r < 0 ? 1 : 0;
    return q;
}

__device__ __forceinline__ int reflect_any32(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// maximum over a block of NW waves; valid in every thread; red: NW doubles
template <int NW>
__device__ __forceinline__ double chain_nd_block_max(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) s = fmax(s, red[k]);
    return s;
}

// The body of both kernels.  STG: the stage flavour (chain_nd_stage_kernel) -- NotEqual and Deterministic passes, resumed and carried fits;
// without it the code is chain_nd_kernel's as it always was.
template <bool BWD, int NT, bool STG>
__device__ __forceinline__ void chain_nd_body(const ChainNd &P) {
    constexpr int CPT = chain_nd_cpt(NT);
    extern __shared__ double lds_nd[];
    const int G = (int)P.g.G;
    double *buf0 = lds_nd, *buf1 = lds_nd + G;
    double *tapw = lds_nd + 2 * (size_t)G;
    double *mg = tapw + (size_t)P.npass * P.tap_slot;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int T = P.T, B = P.B;
    float rdn[MAXD];
    int moff[MAXD];
    int n_sum = 0;
#pragma unroll
    for (int k = 0; k < MAXD; ++k) {
        rdn[k] = k < P.g.ndim ? 1.0f / (float)P.g.n[k] : 1.0f;
        moff[k] = n_sum;
        if (k < P.g.ndim) {
            for (int i = tid; i < P.g.n[k]; i += NT) mg[n_sum + i] = P.g.m[k][i];
            n_sum += P.g.n[k];
        }
    }
    double *red = mg + n_sum;
    double *cur = buf0, *oth = buf1;
    double tot = 1.0;
    // lane q of every wave: the tap id in slot q (-2: nothing staged yet) and its radius
    int slot_id = -2, slot_lw = 0;
    double *po = P.post ? P.post + (long long)b * P.post_stride : nullptr;
    const int t0 = BWD ? T - 1 : 0;
    int kind = P.kind[(size_t)t0 * B + b];
    int ids = lane < P.npass ? P.tap[((size_t)lane * T + t0) * B + b] : -1;
    __syncthreads();                                  // (the grid values)
    for (int step = 0; step < T; ++step) {
        const int t = BWD ? T - 1 - step : step;
        // the next step's metadata and this step's likelihood: in flight while the passes run out of LDS
        int kind_next = SRC_PREV, ids_next = -1;
        if (step + 1 < T) {
            const int tn = BWD ? t - 1 : t + 1;
            kind_next = P.kind[(size_t)tn * B + b];
            if (lane < P.npass) ids_next = P.tap[((size_t)lane * T + tn) * B + b];
        }
        const double *lik = P.lik + (size_t)t * G;
        double *pt = po ? po + (size_t)t * G : nullptr;
        // (the stage flavour's large block has 128 registers a thread and its stage loops beside the 2 x CPT doubles: there the stored a_t
        //  are loaded behind the passes -- one more global latency per backward step, and no spill)
        constexpr bool A_EARLY = !(STG && NT == CHAIN_ND_NT_LARGE);
        double L[CPT], A[BWD ? CPT : 1];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = tid + k * NT;
            L[k] = e < G ? lik[e] : 0.0;
            if (BWD && A_EARLY) A[k] = e < G ? pt[e] : 0.0;
        }
        double scale = 1.0;
        if (kind == SRC_PREV) {
            scale = 1.0 / tot;
            if constexpr (STG && !BWD) {
                if (step == 0 && P.carry_in) {                // (a resumed fit: tot is still 1)
                    const double *cin = P.carry_in + (size_t)b * G;
                    for (int e = tid; e < G; e += NT) cur[e] = cin[e];
                }
            }
        } else {
            const double *sh = P.shared[kind];
            for (int e = tid; e < G; e += NT) cur[e] = sh[e];
        }
        // (STG) the sum of the output of the chain's last stage of this step: the epilogue's scale is its inverse.  `staged`, like every
        // branch below that holds a barrier, depends on the chain's metadata of the step alone: uniform for the block
        bool staged = false;
        double stage_sum = 1.0;
        for (int q = 0; q < P.npass; ++q) {
            const int id = __builtin_amdgcn_readlane(ids, q);
            if (id < 0) continue;
            const int pk = STG ? (int)P.pass_kind[q] : CHAIN_ND_WALK;
            if constexpr (STG) {
                if (pk == CHAIN_ND_NOTEQUAL) {
                    // ne_max / ne_invert / ne_clamp_kernel on the chain's cells, in place: every thread touches the cells it owns (the last
                    // pass, the load or the epilogue wrote them from this thread); the reductions hold the barriers
                    double m = -INFINITY;
                    for (int e = tid; e < G; e += NT) m = fmax(m, cur[e]);
                    m = chain_nd_block_max<NT / 64>(m, red);
                    double sv[1] = {0.0};
                    for (int e = tid; e < G; e += NT) {
                        const double v = m - cur[e];
                        cur[e] = v;
                        sv[0] += v;
                    }
                    blk::block_sums<1, NT / 64>(sv, red);
                    const double total = sv[0], lim = P.limit[(size_t)q * B + b];
                    double su[1] = {0.0};
                    for (int e = tid; e < G; e += NT) {
                        double v = cur[e] / total;
                        v = v < lim ? lim : v;
                        cur[e] = v;
                        su[0] += v;
                    }
                    blk::block_sums<1, NT / 64>(su, red);
                    stage_sum = su[0];
                    staged = true;
                    continue;
                }
            }
            double *w = tapw + (size_t)q * P.tap_slot;
            if (id != __builtin_amdgcn_readlane(slot_id, q)) {
                // (slot q was last read in an earlier step's pass q: barriers in between; the barrier below publishes it)
                const int nlw = P.tap_lw[id];
                const double *wg = P.taps + P.tap_off[id];
                const int nw = STG && pk == CHAIN_ND_SHIFT ? 2 * nlw : nlw;       // a shift: all 2 lw + 1 weights
                for (int j = tid; j <= nw; j += NT) w[j] = wg[j];
                if (lane == q) { slot_id = id; slot_lw = nlw; }
            }
            const int lw = __builtin_amdgcn_readlane(slot_lw, q);
            if (lw == 0) continue;
            __syncthreads();
            const int n = P.pass_n[q], inner = P.pass_inner[q];
            const float rn = 1.0f / (float)n, ri = 1.0f / (float)inner;
            if (STG && pk == CHAIN_ND_SHIFT) {
                // shift_axis_kernel: out[i] = sum_m w[m + lw] ext[i + m] over blk::extend_index(rule 2), m ascending, fma -- the same
                // cells in the same order, so the same bits per cell
                const double *wc = w + lw;
                double sv[1] = {0.0};
                for (int e = tid; e < G; e += NT) {
                    const int r = small_div(e, inner, ri);
                    const int i = r - small_div(r, n, rn) * n;
                    const double *row = cur + (e - i * inner);
                    // blk::extend_index(i + m, n, 2) for consecutive m without a remainder per tap: y = the position of i + m in the
                    // period 2 (n + 24) of the padded row's half-sample reflection, walked along with m
                    const int np = n + 24, per = 2 * np;
                    int y = (i - lw + 12) % per;
                    y += y < 0 ? per : 0;
                    double acc = 0.0;
#pragma unroll 1
                    for (int m = -lw; m <= lw; ++m) {
                        const int k = y < np ? y : per - 1 - y;
                        acc = fma(wc[m], row[min(max(k - 12, 0), n - 1) * inner], acc);
                        y = y + 1 == per ? 0 : y + 1;
                    }
                    oth[e] = acc;
                    sv[0] += acc;
                }
                blk::block_sums<1, NT / 64>(sv, red);
                stage_sum = sv[0];
                staged = true;
            } else if (lw <= n) {
                for (int e = tid; e < G; e += NT) {
                    const int r = small_div(e, inner, ri);
                    const int i = r - small_div(r, n, rn) * n;
                    const double *row = cur + (e - i * inner);
                    double acc = cur[e] * w[0];
                    for (int j = lw; j >= 1; --j) {
                        int lo = i - j, hi = i + j;
                        lo = lo < 0 ? -lo - 1 : lo;
                        hi = hi >= n ? 2 * n - 1 - hi : hi;
                        acc += (row[lo * inner] + row[hi * inner]) * w[j];
                    }
                    oth[e] = acc;
                }
            } else {
                for (int e = tid; e < G; e += NT) {
                    const int r = small_div(e, inner, ri);
                    const int i = r - small_div(r, n, rn) * n;
                    const double *row = cur + (e - i * inner);
                    double acc = cur[e] * w[0];
                    for (int j = lw; j >= 1; --j)
                        acc += (row[reflect_any32(i - j, n) * inner] + row[reflect_any32(i + j, n) * inner]) * w[j];
                    oth[e] = acc;
                }
            }
            double *sw = cur; cur = oth; oth = sw;
        }
        if constexpr (STG) {
            if (staged) scale = 1.0 / stage_sum;
        }
        // the epilogue touches the cells the thread itself wrote last (same e -> thread map in the load, the passes and here)
        if constexpr (BWD && !A_EARLY) {
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int e = tid + k * NT;
                A[k] = e < G ? pt[e] : 0.0;
            }
        }
        double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double *co = nullptr;
        if constexpr (STG && !BWD) co = (step == T - 1 && P.carry_out) ? P.carry_out + (size_t)b * G : nullptr;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = tid + k * NT;
            if (e < G) {
                const double x = cur[e] * scale;
                double p;
                if (!BWD) {
                    p = x * L[k];
                    cur[e] = p;
                    if (pt) pt[e] = p;
                    if constexpr (STG) {
                        if (co) co[e] = p;
                    }
                } else {
                    p = A[BWD ? k : 0] * x;
                    const double cn = x * L[k];
                    pt[e] = p;
                    cur[e] = cn;
                    s[1] += p / L[k];
                    s[2] += cn;
                }
                s[0] += p;
                int rem = e;
#pragma unroll
                for (int d = MAXD - 1; d >= 0; --d)
                    if (d < P.g.ndim) {
                        const int qn = small_div(rem, P.g.n[d], rdn[d]);
                        s[3 + d] += p * mg[moff[d] + rem - qn * P.g.n[d]];
                        rem = qn;
                    }
            }
        }
        blk::block_sums<7, NT / 64>(s, red);
        tot = BWD ? s[2] : s[0];
        if (tid == 0) {
            double *out = P.psum + ((size_t)t * B + b) * NRED;
#pragma unroll
            for (int k = 0; k < 7; ++k) out[k] = s[k];
        }
        kind = kind_next;
        ids = ids_next;
    }
}

template <bool BWD, int NT>
__global__ __launch_bounds__(NT) void chain_nd_kernel(const ChainNd P) {
    chain_nd_body<BWD, NT, false>(P);
}

// The stage flavour: what chain_nd_kernel does, and per step, for its chain, what nd_step does with blhip_nd_stages.hpp --
//   NotEqual       (transitionModels.py:462-471) block maximum, v = max - x, u = v / sum v with the cells below limit = 10**value dV set to
//                  it, sum u: three sweeps over the chain's cells in LDS, in place
//   Deterministic  (:571-602) the asymmetric stencil of TapTable::get_shift along the op's axis (2 lw + 1 weights in the pass's tap slot)
//                  and the sum of the result
// After a stage the epilogue's scale is 1 / (sum of the chain's last stage of the step); a walk behind a stage acts on the stage's output
// unscaled (linear), as filter_axis_kernel does.  A chain that runs no stage at a step keeps 1 / tot: every chain has its block, nothing is
// copied through.  Forward step 0 of a resumed fit loads the chain's carried state (sum 1); a carried fit that keeps no sequence
// writes its last forward state to carry_out.
template <bool BWD, int NT>
__global__ __launch_bounds__(NT) void chain_nd_stage_kernel(const ChainNd P) {
    chain_nd_body<BWD, NT, true>(P);
}

}  // namespace bln
