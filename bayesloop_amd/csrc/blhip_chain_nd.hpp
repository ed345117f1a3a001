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

template <bool BWD, int NT>
__global__ __launch_bounds__(NT) void chain_nd_kernel(const ChainNd P) {
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
        double L[CPT], A[BWD ? CPT : 1];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int e = tid + k * NT;
            L[k] = e < G ? lik[e] : 0.0;
            if (BWD) A[k] = e < G ? pt[e] : 0.0;
        }
        double scale = 1.0;
        if (kind == SRC_PREV) {
            scale = 1.0 / tot;
        } else {
            const double *sh = P.shared[kind];
            for (int e = tid; e < G; e += NT) cur[e] = sh[e];
        }
        for (int q = 0; q < P.npass; ++q) {
            const int id = __builtin_amdgcn_readlane(ids, q);
            if (id < 0) continue;
            double *w = tapw + (size_t)q * P.tap_slot;
            if (id != __builtin_amdgcn_readlane(slot_id, q)) {
                // (slot q was last read in an earlier step's pass q: barriers in between; the barrier below publishes it)
                const int nlw = P.tap_lw[id];
                const double *wg = P.taps + P.tap_off[id];
                for (int j = tid; j <= nlw; j += NT) w[j] = wg[j];
                if (lane == q) { slot_id = id; slot_lw = nlw; }
            }
            const int lw = __builtin_amdgcn_readlane(slot_lw, q);
            if (lw == 0) continue;
            __syncthreads();
            const int n = P.pass_n[q], inner = P.pass_inner[q];
            const float rn = 1.0f / (float)n, ri = 1.0f / (float)inner;
            if (lw <= n) {
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
        // the epilogue touches the cells the thread itself wrote last (same e -> thread map in the load, the passes and here)
        double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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

}  // namespace bln
