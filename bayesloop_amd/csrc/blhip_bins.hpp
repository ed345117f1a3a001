// Distribution queries of the parser at many time steps in one call:  out[s][b] = sum of post[steps[s]][c] over the cells c with bin[c] == b --
// bl.Parser / Study.eval WITHOUT a relation and with a vector of time stamps (reference bayesloop/parser.py:399-418: the binned distribution of
// a derived quantity), whose users loop the scalar call over every time stamp.  For a query over the parameters of ONE study the values, the
// bins and the bin of every cell do not depend on the step: the host bins the grid once (bayesloop_amd/parser.py: _binning) and hands the map.
//
// No floating-point atomics and no order that depends on scheduling.  The order of the additions is fixed by the map alone:
//   * the cells are cut into slabs of `slab`; the host orders the cells of a slab stably by bin (order()): a RUN is the cells of one bin in one
//     slab, in ascending cell order.  Runs are numbered by (slab, bin).
//   * a run is cut into GROUPS of gw cells, the last one padded with an index that points at a zero word.  One thread adds one group from its
//     first cell to its last -- so a bin with 131 841 cells and a bin with one cost their threads the same -- and the groups of a run that has
//     several are added in ascending order by a second stage (one thread per run and step: at most slab / gw additions).
//   * bins_kernel: grid = (slabs, blocks of sb steps).  The block stages its slab of the sb rows in LDS with coalesced loads (16 bytes per
//     lane where the rows are 16-byte aligned), then reads LDS through the permutation, so every selected row is read from HBM once.  It
//     writes one partial per (step, run).
//   * bins_combine_kernel adds the runs of a bin in ascending slab order (one thread per (step, bin)); a bin no slab touches is 0.
// gw is chosen per map: 1 if every run is one cell, else the power of two >= the mean run length within [2, gw_max] -- a map of singletons
// (a 1-D grid under a monotone function) does not read gw - 1 zero words per cell.
//
// The host-only part (check_bins, Order, order(), bins_plan) has no HIP call in it: tests/host/bins_plan_main.cpp runs it stand-alone.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace blb {

constexpr int NT = 256;                        // threads of a block
constexpr int SB_MAX = 16;                     // most steps of a block (the accumulators of a thread)
constexpr int SB = 8;                          // steps of a block                    } measured: profiles/parser_bins_notes.md (slab 256 / 512 / 1024,
constexpr long long SLAB = 1024;               // cells of a slab (even)              } sb 4 / 8 / 16, gw 4 / 8 / 16: the longer slab has fewer runs;
constexpr int GW = 8;                          // widest group                        } sb and gw made no difference beyond the noise)
constexpr long long SLAB_MIN = 64, SLAB_MAX = 4096;
constexpr int GW_LIMIT = 16;
constexpr long long LDS_BYTES_MAX = 160 * 1024;
constexpr long long ALIGN = 256;
constexpr long long STEP_BLOCKS_MAX = 32768;   // step blocks of a chunk: the gridDim.y of one launch

inline long long round_up(long long v, long long q) { return (v + q - 1) / q * q; }

// the shape a call runs with: the defaults above, or what a caller asks for, brought into the ranges the kernel is written for (an even slab;
// at most SB_MAX steps; a power-of-two group width; the worst map -- runs of gw + 1 cells: slab slots -- fits the LDS of a CU)
struct Shape { long long slab = SLAB; int sb = SB, gw_max = GW; };
inline Shape shape(double slab, double sb, double gw) {
    Shape s;
    s.slab = std::min(SLAB_MAX, std::max(SLAB_MIN, (long long)slab)) / 2 * 2;
    s.sb = (int)std::min<double>(SB_MAX, std::max(1.0, sb));
    int g = 1;
    while (g * 2 <= (int)std::min<double>(GW_LIMIT, std::max(1.0, gw))) g *= 2;
    s.gw_max = g;
    while (8ll * s.sb * (2 * s.slab + 2) > LDS_BYTES_MAX) s.slab = s.slab / 4 * 2;
    return s;
}

// ---- host-only validation (no HIP call) -> 0, or -1 with a message in err ----------------------------------------------------------------------
inline int check_bins(const int32_t *bin, int64_t G, int64_t n_bins, char *err, int errlen) {
    auto bad = [&](const char *fmt, long long a, long long b, long long c) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a, b, c);
        return -1;
    };
    if (!bin) return bad("bins: bin is NULL", 0, 0, 0);
    if (G < 1 || G > 0x7fffffffLL) return bad("bins: G = %lld", G, 0, 0);
    if (n_bins < 1 || n_bins > 0x7fffffffLL) return bad("bins: n_bins = %lld", n_bins, 0, 0);
    for (int64_t c = 0; c < G; ++c)
        if (bin[c] < -1 || bin[c] >= n_bins) return bad("bins: bin[%lld] = %lld is outside -1 .. %lld", c, bin[c], n_bins - 1);
    return 0;
}

// ---- the order of a map ---------------------------------------------------------------------------------------------------------------------
struct Order {
    long long G = 0, n_bins = 0, slab = 0, n_slabs = 0;
    int gw = 1;
    long long n_runs = 0, n_groups = 0, n_multi = 0, max_slots = 0, cells_in = 0;
    std::vector<long long> slabs;      // [2][n_slabs + 1]: the first group of every slab, then the first several-group run of every slab
    // int32 tables, one upload: perm [n_groups * gw] -- per slab [gw][groups of the slab]: the slab-local cell of place j of a group, `slab` = the
    // zero word; gdst [n_groups]: >= 0 the run whose only group this is, else -1 - slot (slab-local); multi [n_multi][3]: run, first slot, groups;
    // bin_ptr [n_bins + 1] and bin_runs [n_runs]: the runs of every bin in ascending slab order
    std::vector<int32_t> tab;
    long long off_perm = 0, off_gdst = 0, off_multi = 0, off_binptr = 0, off_binruns = 0;
    long long table_bytes() const { return round_up((long long)slabs.size() * 8, ALIGN) + round_up((long long)tab.size() * 4, ALIGN); }
    long long lds_bytes(int sb) const { return 8ll * sb * (slab + 2 + max_slots); }
};

// bin: a checked map (check_bins).  -> false: the tables would not fit int32 indices
inline bool order(const int32_t *bin, long long G, long long n_bins, long long slab, int gw_max, Order &O) {
    O = Order{};
    O.G = G; O.n_bins = n_bins; O.slab = slab; O.n_slabs = (G + slab - 1) / slab;
    std::vector<int32_t> cnt((size_t)n_bins, 0), touched;
    touched.reserve((size_t)std::min(slab, n_bins));
    // pass 1: the runs and the cells that have a bin -> the group width
    for (long long k = 0; k < O.n_slabs; ++k) {
        const long long lo = k * slab, hi = std::min(G, lo + slab);
        touched.clear();
        for (long long c = lo; c < hi; ++c)
            if (bin[c] >= 0) { ++O.cells_in; if (cnt[(size_t)bin[c]]++ == 0) touched.push_back(bin[c]); }
        O.n_runs += (long long)touched.size();
        for (int32_t b : touched) cnt[(size_t)b] = 0;
    }
    O.gw = 1;
    if (O.n_runs > 0 && O.cells_in > O.n_runs) {
        O.gw = 2;
        while (O.gw < gw_max && (long long)O.gw * O.n_runs < O.cells_in) O.gw *= 2;
    }
    const int gw = O.gw;
    // pass 2: groups per slab
    O.slabs.assign((size_t)(2 * (O.n_slabs + 1)), 0);
    long long *goff = O.slabs.data(), *moff = O.slabs.data() + O.n_slabs + 1;
    for (long long k = 0; k < O.n_slabs; ++k) {
        const long long lo = k * slab, hi = std::min(G, lo + slab);
        touched.clear();
        for (long long c = lo; c < hi; ++c)
            if (bin[c] >= 0 && cnt[(size_t)bin[c]]++ == 0) touched.push_back(bin[c]);
        long long groups = 0, multi = 0, slots = 0;
        for (int32_t b : touched) {
            const long long n = (cnt[(size_t)b] + gw - 1) / gw;
            groups += n;
            if (n > 1) { ++multi; slots += n; }
            cnt[(size_t)b] = 0;
        }
        goff[k + 1] = goff[k] + groups;
        moff[k + 1] = moff[k] + multi;
        O.max_slots = std::max(O.max_slots, slots);
    }
    O.n_groups = goff[O.n_slabs];
    O.n_multi = moff[O.n_slabs];
    O.off_perm = 0;
    O.off_gdst = O.off_perm + O.n_groups * gw;
    O.off_multi = O.off_gdst + O.n_groups;
    O.off_binptr = O.off_multi + 3 * O.n_multi;
    O.off_binruns = O.off_binptr + n_bins + 1;
    const long long total = O.off_binruns + O.n_runs;
    if (total > 0x7fffffffLL) return false;
    O.tab.assign((size_t)total, 0);
    int32_t *perm = O.tab.data() + O.off_perm, *gdst = O.tab.data() + O.off_gdst, *multi = O.tab.data() + O.off_multi;
    int32_t *bin_ptr = O.tab.data() + O.off_binptr, *bin_runs = O.tab.data() + O.off_binruns;
    std::fill(perm, perm + O.n_groups * gw, (int32_t)slab);
    // pass 3: the tables
    std::vector<int32_t> run_bin((size_t)O.n_runs), place((size_t)n_bins, 0);      // place[b]: the next padded place of bin b inside the slab
    long long run = 0, m = 0;
    for (long long k = 0; k < O.n_slabs; ++k) {
        const long long lo = k * slab, hi = std::min(G, lo + slab), ng = goff[k + 1] - goff[k];
        touched.clear();
        for (long long c = lo; c < hi; ++c)
            if (bin[c] >= 0 && cnt[(size_t)bin[c]]++ == 0) touched.push_back(bin[c]);
        std::sort(touched.begin(), touched.end());
        long long g = 0, slot = 0;
        for (int32_t b : touched) {
            const long long n = (cnt[(size_t)b] + gw - 1) / gw;
            place[(size_t)b] = (int32_t)(g * gw);
            run_bin[(size_t)run] = b;
            if (n == 1) {
                gdst[goff[k] + g] = (int32_t)run;
            } else {
                for (long long i = 0; i < n; ++i) gdst[goff[k] + g + i] = (int32_t)(-1 - (slot + i));
                multi[3 * m] = (int32_t)run; multi[3 * m + 1] = (int32_t)slot; multi[3 * m + 2] = (int32_t)n;
                slot += n;
                ++m;
            }
            g += n;
            ++run;
            cnt[(size_t)b] = 0;
        }
        int32_t *pk = perm + goff[k] * gw;
        for (long long c = lo; c < hi; ++c) {
            if (bin[c] < 0) continue;
            const long long p = place[(size_t)bin[c]]++;
            pk[(p % gw) * ng + p / gw] = (int32_t)(c - lo);
        }
    }
    // the runs of every bin: a counting sort of the run numbers by bin (stable: ascending slabs)
    for (long long r = 0; r < O.n_runs; ++r) ++bin_ptr[run_bin[(size_t)r] + 1];
    for (long long b = 0; b < n_bins; ++b) bin_ptr[b + 1] += bin_ptr[b];
    std::vector<int32_t> at(bin_ptr, bin_ptr + n_bins);
    for (long long r = 0; r < O.n_runs; ++r) bin_runs[at[(size_t)run_bin[(size_t)r]]++] = (int32_t)r;
    return true;
}

// out (n_rows, n_bins): the rows (n_rows, G) added in the order the kernels add them -- the host restatement the stand-alone program prints
inline void ordered_sums(const Order &O, const double *rows, long long n_rows, double *out) {
    const int32_t *perm = O.tab.data() + O.off_perm, *gdst = O.tab.data() + O.off_gdst, *multi = O.tab.data() + O.off_multi;
    const int32_t *bin_ptr = O.tab.data() + O.off_binptr, *bin_runs = O.tab.data() + O.off_binruns;
    const long long *goff = O.slabs.data(), *moff = O.slabs.data() + O.n_slabs + 1;
    std::vector<double> part((size_t)std::max<long long>(1, O.n_runs)), gs((size_t)std::max<long long>(1, O.max_slots));
    for (long long s = 0; s < n_rows; ++s) {
        const double *row = rows + s * O.G;
        for (long long k = 0; k < O.n_slabs; ++k) {
            const long long lo = k * O.slab, ng = goff[k + 1] - goff[k];
            const int32_t *pk = perm + goff[k] * O.gw;
            for (long long g = 0; g < ng; ++g) {
                double acc = 0.0;
                for (int j = 0; j < O.gw; ++j) { const int32_t c = pk[j * ng + g]; acc += c == O.slab ? 0.0 : row[lo + c]; }
                const int32_t d = gdst[goff[k] + g];
                if (d >= 0) part[(size_t)d] = acc; else gs[(size_t)(-1 - d)] = acc;
            }
            for (long long q = moff[k]; q < moff[k + 1]; ++q) {
                double sum = gs[(size_t)multi[3 * q + 1]];
                for (int32_t i = 1; i < multi[3 * q + 2]; ++i) sum += gs[(size_t)(multi[3 * q + 1] + i)];
                part[(size_t)multi[3 * q]] = sum;
            }
        }
        for (long long b = 0; b < O.n_bins; ++b) {
            double sum = 0.0;
            for (int32_t i = bin_ptr[b]; i < bin_ptr[b + 1]; ++i) sum += part[(size_t)bin_runs[i]];
            out[s * O.n_bins + b] = sum;
        }
    }
}

// ---- the plan: what of the budget the steps of a chunk take ------------------------------------------------------------------------------------
struct BinsPlan {
    long long steps_per_chunk = 0, n_chunks = 0, workspace_bytes = 0, min_budget_bytes = 0;
    long long off_steps = 0, off_part = 0, off_out = 0;      // behind the tables
};

// n_runs runs and table_bytes of tables (Order), n_steps steps in blocks of sb.  -> false: bad arguments, or a budget below min_budget_bytes
// (which is filled in whenever the arguments are good)
inline bool bins_plan(long long n_bins, long long n_runs, long long table_bytes, long long n_steps, int sb, double budget, BinsPlan &P) {
    P = BinsPlan{};
    if (n_bins < 1 || n_bins > 0x7fffffffLL || n_runs < 0 || n_runs > 0x7fffffffLL || table_bytes < 0 || table_bytes > (1ll << 46) || n_steps < 1 ||
        n_steps > (1ll << 31) || sb < 1 || sb > SB_MAX)
        return false;
    const long long fixed = round_up(table_bytes, ALIGN);
    auto need = [&](long long s, long long *off) {
        long long o[3];
        o[0] = fixed;                                                        // steps (int64)
        o[1] = o[0] + round_up(s * 8, ALIGN);                                // partials (s, n_runs)
        if ((double)s * (double)(n_runs + n_bins) * 8.0 > 4e18) return 1ll << 62;      // (beyond any budget, and beyond int64 below)
        o[2] = o[1] + round_up(std::max<long long>(1, s * n_runs) * 8, ALIGN);      // out (s, n_bins)
        if (off) for (int k = 0; k < 3; ++k) off[k] = o[k];
        return o[2] + round_up(s * n_bins * 8, ALIGN);
    };
    P.min_budget_bytes = need(1, nullptr);
    if (!(budget >= (double)P.min_budget_bytes)) return false;
    long long s = std::min(n_steps, STEP_BLOCKS_MAX * sb);
    // (the combine kernel's grid: one thread per (step, bin) of the chunk)
    s = std::max<long long>(1, std::min(s, (0x7fffffffLL * NT) / n_bins));
    if ((double)need(s, nullptr) > budget) {
        long long lo = 1, hi = s;
        while (lo < hi) {
            const long long mid = lo + (hi - lo + 1) / 2;
            if ((double)need(mid, nullptr) <= budget) lo = mid; else hi = mid - 1;
        }
        s = lo > sb ? lo / sb * sb : lo;
    }
    P.steps_per_chunk = s;
    P.n_chunks = (n_steps + s - 1) / s;
    long long off[3];
    P.workspace_bytes = need(s, off);
    P.off_steps = off[0]; P.off_part = off[1]; P.off_out = off[2];
    return true;
}

#ifdef __HIPCC__
// ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------
struct BinsParams {
    const double *post;              // row 0 of the sequence
    const long long *steps;          // (S) rows of the sequence
    const long long *slabs;          // Order::slabs
    const int *perm, *gdst, *multi;
    double *part;                    // (S, R)
    long long G, slab, R, n_slabs;
    int S, sb, gw, slots, wide;      // slots: Order::max_slots; wide: every staged row starts 16-byte aligned and has an even length
};

// grid = (slabs, blocks of sb steps); dynamic LDS: sb rows of slab + 2 doubles (word `slab` of a row is the zero the padding points at), then
// sb rows of `slots` group sums
static __global__ __launch_bounds__(NT) void bins_kernel(const BinsParams P) {
    extern __shared__ __attribute__((aligned(16))) double bins_lds[];
    const long long k = blockIdx.x;
    const int s0 = (int)blockIdx.y * P.sb, ns = min(P.sb, P.S - s0), tid = (int)threadIdx.x;
    const long long lo = k * P.slab;
    const int len = (int)min(P.slab, P.G - lo), stride = (int)P.slab + 2;
    double *gs = bins_lds + (long long)P.sb * stride;
    for (int s = 0; s < ns; ++s) {
        const double *row = P.post + P.steps[s0 + s] * P.G + lo;
        double *dst = bins_lds + s * stride;
        if (P.wide) {
            for (int i = tid; i < len / 2; i += NT) reinterpret_cast<double2 *>(dst)[i] = reinterpret_cast<const double2 *>(row)[i];
        } else {
            for (int i = tid; i < len; i += NT) dst[i] = row[i];
        }
        if (tid == 0) dst[P.slab] = 0.0;
    }
    __syncthreads();
    const long long g0 = P.slabs[k];
    const int ng = (int)(P.slabs[k + 1] - g0);
    const int *pm = P.perm + g0 * P.gw;
    for (int g = tid; g < ng; g += NT) {
        double acc[SB_MAX];
#pragma unroll
        for (int s = 0; s < SB_MAX; ++s) acc[s] = 0.0;
        for (int j = 0; j < P.gw; ++j) {
            const int c = pm[j * ng + g];
#pragma unroll
            for (int s = 0; s < SB_MAX; ++s)
                if (s < ns) acc[s] += bins_lds[s * stride + c];
        }
        const int d = P.gdst[g0 + g];
#pragma unroll
        for (int s = 0; s < SB_MAX; ++s) {
            if (s < ns) {
                if (d >= 0) P.part[(long long)(s0 + s) * P.R + d] = acc[s];
                else gs[s * P.slots + (-1 - d)] = acc[s];
            }
        }
    }
    const long long m0 = P.slabs[P.n_slabs + 1 + k];
    const int nm = (int)(P.slabs[P.n_slabs + 2 + k] - m0);
    if (nm == 0) return;                                   // (block-uniform)
    __syncthreads();
    for (int q = tid; q < nm * ns; q += NT) {
        const int s = q / nm;
        const int *mr = P.multi + 3 * (m0 + q % nm);
        const double *v = gs + s * P.slots + mr[1];
        double sum = v[0];
        for (int i = 1; i < mr[2]; ++i) sum += v[i];
        P.part[(long long)(s0 + s) * P.R + mr[0]] = sum;
    }
}

// out[s][b] = the partials of the runs of bin b, added in ascending slab order; one thread per (step, bin)
static __global__ __launch_bounds__(NT) void bins_combine_kernel(const double *part, const int *bin_ptr, const int *bin_runs, double *out, long long R, long long S,
                                                                 long long n_bins) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= S * n_bins) return;
    const long long s = idx / n_bins, b = idx - s * n_bins;
    double sum = 0.0;
    for (int i = bin_ptr[b]; i < bin_ptr[b + 1]; ++i) sum += part[s * R + bin_runs[i]];
    out[idx] = sum;
}
#endif

}   // namespace blb
