// Likelihood programs: the density of a plug-in observation model (bl.om.SymPy, bl.om.SciPy) as a small postfix program over the data
// point and the grid's parameters, compiled from the SymPy expression on the host (bayesloop_amd/likprogram.py) and evaluated per cell
// by ONE kernel, which writes the (T, G) table the table flavours of the fit kernels read (reference: observationModels.py:35-56 --
// the likelihood of a step is the product over the data dimensions of the density; a NaN datum contributes the factor 1).
//
// One {int32 code, int32 arg} record per op:
//   pushes      CONST i (consts[i]), PARAM k (the marginal grid value of axis k at the cell), DATA (the datum of the current data
//               dimension), STEP j (value j of the current (step, data dimension): a data-only subtree the host evaluated),
//               AXIS a (arg = axis | offset << 2: consts[offset + index of the cell along that axis] -- a function of ONE parameter
//               the host tabulated along its axis, e.g. the normalisation of Student's t as a function of its degrees of freedom)
//   arithmetic  ADD MUL DIV NEG ABS SQRT EXP LOG POW COS SIN, POWI n (integer exponent |n| <= 64 by multiplications: **2 is x * x)
//   logic       LT LE EQ (1.0 / 0.0), AND, SELECT (a b c -> c != 0 ? a : b)
// at most MAX_OPS ops, stack depth at most MAX_STACK; a program leaves exactly one value.
//
// Compiler's report for gfx950 (-Rpass-analysis=kernel-resource-usage) and what the interpreter costs: DESIGN.md 4.3b.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

namespace bllp {

enum : int {
    OP_CONST = 0, OP_PARAM = 1, OP_DATA = 2, OP_STEP = 3, OP_AXIS = 4,
    OP_ADD = 5, OP_MUL = 6, OP_DIV = 7, OP_NEG = 8, OP_ABS = 9, OP_SQRT = 10, OP_EXP = 11, OP_LOG = 12, OP_POW = 13, OP_COS = 14, OP_SIN = 15,
    OP_POWI = 16, OP_LT = 17, OP_LE = 18, OP_EQ = 19, OP_AND = 20, OP_SELECT = 21, OP_COUNT = 22
};
constexpr int MAX_OPS = 256, MAX_STACK = 16, MAX_POWI = 64, MAX_DIM = 4;
constexpr int NT = 256;

struct Instr { int32_t code, arg; };

// what is uniform across a launch and never written by it -- the program, the constants, the rows of data and step values -- is read
// through the CONSTANT address space: scalar loads into SGPRs, one per wave
typedef const __attribute__((address_space(4))) double *uniform_doubles;
typedef const __attribute__((address_space(4))) Instr *uniform_instrs;

// ---- host-only validation (no HIP call): stack discipline and index ranges --------------------------------------------------------
// -> 0, or -1 with a message in err.  AXIS offsets are checked against n_consts here and against the axis length when a grid is known.
inline int check_program(const int32_t *ops, int64_t n_ops, int64_t n_consts, int64_t n_step, int ndim, char *err, int errlen) {
    auto bad = [&](const char *fmt, long long a, long long b, long long c) {
        if (err && errlen > 0) std::snprintf(err, (size_t)errlen, fmt, a, b, c);
        return -1;
    };
    if (!ops || n_ops < 1) return bad("likelihood program: no ops", 0, 0, 0);
    if (n_ops > MAX_OPS) return bad("likelihood program: %lld ops (at most %lld)", n_ops, MAX_OPS, 0);
    if (ndim < 1 || ndim > MAX_DIM) return bad("likelihood program: %lld parameters (1 .. %lld)", ndim, MAX_DIM, 0);
    if (n_consts < 0 || n_step < 0) return bad("likelihood program: negative table size", 0, 0, 0);
    int depth = 0;
    for (int64_t pc = 0; pc < n_ops; ++pc) {
        const int code = ops[2 * pc], arg = ops[2 * pc + 1];
        int need = 0, push = 0;
        switch (code) {
            case OP_CONST: if (arg < 0 || arg >= n_consts) return bad("likelihood program: op %lld: CONST %lld out of range (%lld constants)", pc, arg, n_consts); push = 1; break;
            case OP_PARAM: if (arg < 0 || arg >= ndim) return bad("likelihood program: op %lld: PARAM %lld out of range (%lld parameters)", pc, arg, ndim); push = 1; break;
            case OP_DATA: push = 1; break;
            case OP_STEP: if (arg < 0 || arg >= n_step) return bad("likelihood program: op %lld: STEP %lld out of range (%lld step values)", pc, arg, n_step); push = 1; break;
            case OP_AXIS:
                if (arg < 0 || (arg & 3) >= ndim) return bad("likelihood program: op %lld: AXIS of parameter %lld (%lld parameters)", pc, arg & 3, ndim);
                if ((arg >> 2) >= n_consts) return bad("likelihood program: op %lld: AXIS offset %lld out of range (%lld constants)", pc, arg >> 2, n_consts);
                push = 1; break;
            case OP_ADD: case OP_MUL: case OP_DIV: case OP_POW: case OP_LT: case OP_LE: case OP_EQ: case OP_AND: need = 2; push = 1; break;
            case OP_NEG: case OP_ABS: case OP_SQRT: case OP_EXP: case OP_LOG: case OP_COS: case OP_SIN: need = 1; push = 1; break;
            case OP_POWI: if (arg < -MAX_POWI || arg > MAX_POWI) return bad("likelihood program: op %lld: POWI exponent %lld (|n| <= %lld)", pc, arg, MAX_POWI); need = 1; push = 1; break;
            case OP_SELECT: need = 3; push = 1; break;
            default: return bad("likelihood program: op %lld: unknown code %lld", pc, code, 0);
        }
        if (depth < need) return bad("likelihood program: op %lld: stack underflow (needs %lld values, has %lld)", pc, need, depth);
        depth += push - need;
        if (depth > MAX_STACK) return bad("likelihood program: op %lld: stack depth %lld (at most %lld)", pc, depth, MAX_STACK);
    }
    if (depth != 1) return bad("likelihood program: leaves %lld values on the stack (must leave one)", depth, 0, 0);
    return 0;
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------------
struct LikProgParams {
    const Instr *ops;            // uniform across the launch: read through the scalar path
    const double *consts;
    const double *step;          // (T, dd, n_step) of the launch's first row
    const double *data;          // (T, dd) of the launch's first row (segment length 1)
    double *lik;                 // (T, G) of the launch's first row
    const double *m[MAX_DIM];    // marginal grids
    long long G;
    int n[MAX_DIM];
    int n_ops, n_step, dd, ndim;
};

// x^n by squaring: |n| - 1 multiplications at most (+ the reciprocal of a negative exponent)
static __device__ __forceinline__ double powi(double x, int n) {
    unsigned e = n < 0 ? 0u - (unsigned)n : (unsigned)n;
    double r = 1.0, b = x;
    bool first = true;
    while (e) {
        if (e & 1u) { r = first ? b : r * b; first = false; }
        e >>= 1;
        if (e) b *= b;
    }
    return n < 0 ? 1.0 / r : r;
}

// The stack below its top lives in registers: sp, the opcode and its argument are wave-uniform (scalar loads of the program), so every
// access is one of MAX_STACK - 1 NAMED slots chosen by a scalar branch.  (An array, even one indexed only by literals inside an if-chain on
// the index, is turned back into a run-time-indexed array by the optimiser and placed in scratch: 128 B per lane in the compiler's report.)
#define BLLP_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14)
struct Stack {
#define BLLP_DECL(k) double s##k;
    BLLP_SLOTS(BLLP_DECL)
#undef BLLP_DECL
    __device__ __forceinline__ double get(int i) const {
        switch (i) {
#define BLLP_GET(k) case k: return s##k;
            BLLP_SLOTS(BLLP_GET)
#undef BLLP_GET
        }
        return 0.0;
    }
    __device__ __forceinline__ void put(int i, double v) {
        switch (i) {
#define BLLP_PUT(k) case k: s##k = v; break;
            BLLP_SLOTS(BLLP_PUT)
#undef BLLP_PUT
        }
    }
};
static_assert(MAX_STACK == 16, "BLLP_SLOTS lists MAX_STACK - 1 slots");

// grid = (chunks of cells, rows of T); consecutive lanes own consecutive cells of the last parameter (a wave stores 512 B)
static __global__ __launch_bounds__(NT) void lik_program_kernel(const LikProgParams P) {
    const long long t = blockIdx.y;
    const uniform_instrs ops = (uniform_instrs)P.ops;
    const uniform_doubles consts = (uniform_doubles)P.consts;
    const uniform_doubles xrow = (uniform_doubles)(P.data + t * P.dd);
    const uniform_doubles srow = (uniform_doubles)(P.step + t * P.dd * P.n_step);
    double *__restrict__ out = P.lik + t * P.G;
    for (long long c = (long long)blockIdx.x * NT + threadIdx.x; c < P.G; c += (long long)gridDim.x * NT) {
        // one decomposition per cell: the indices along the axes (last parameter fastest) and the marginal values there
        int idx[MAX_DIM] = {0, 0, 0, 0};
        double g[MAX_DIM] = {0.0, 0.0, 0.0, 0.0};
        if (P.G <= 0x7fffffffLL) {
            unsigned r = (unsigned)c;
#pragma unroll
            for (int k = MAX_DIM - 1; k >= 0; --k)
                if (k < P.ndim) { const unsigned q = r / (unsigned)P.n[k]; idx[k] = (int)(r - q * (unsigned)P.n[k]); r = q; }
        } else {
            long long r = c;
#pragma unroll
            for (int k = MAX_DIM - 1; k >= 0; --k)
                if (k < P.ndim) { const long long q = r / P.n[k]; idx[k] = (int)(r - q * P.n[k]); r = q; }
        }
#pragma unroll
        for (int k = 0; k < MAX_DIM; ++k)
            if (k < P.ndim) g[k] = P.m[k][idx[k]];
        double L = 1.0;
        for (int k = 0; k < P.dd; ++k) {
            const double x = xrow[k];
            if (x != x) continue;                      // a NaN datum: the factor 1 (observationModels.py:49-54)
            const uniform_doubles sv = srow + (long long)k * P.n_step;
            Stack st;
            double top = 0.0;
            int sp = 0;                                // values on the stack, the top one in `top`
            for (int pc = 0; pc < P.n_ops; ++pc) {
                const int code = __builtin_amdgcn_readfirstlane(ops[pc].code), arg = __builtin_amdgcn_readfirstlane(ops[pc].arg);
                if (code <= OP_AXIS) {                 // pushes
                    if (sp > 0) st.put(sp - 1, top);
                    ++sp;
                    if (code == OP_CONST) top = consts[arg];
                    else if (code == OP_PARAM) top = arg == 0 ? g[0] : (arg == 1 ? g[1] : (arg == 2 ? g[2] : g[3]));
                    else if (code == OP_DATA) top = x;
                    else if (code == OP_STEP) top = sv[arg];
                    else {
                        const int ax = arg & 3;
                        top = P.consts[(arg >> 2) + (ax == 0 ? idx[0] : (ax == 1 ? idx[1] : (ax == 2 ? idx[2] : idx[3])))];
                    }
                } else if (code == OP_NEG) top = -top;
                else if (code == OP_ABS) top = fabs(top);
                else if (code == OP_SQRT) top = sqrt(top);
                else if (code == OP_EXP) top = exp(top);
                else if (code == OP_LOG) top = log(top);
                else if (code == OP_COS) top = cos(top);
                else if (code == OP_SIN) top = sin(top);
                else if (code == OP_POWI) top = arg == 2 ? top * top : powi(top, arg);
                else if (code == OP_SELECT) {
                    const double b = st.get(sp - 2), a = st.get(sp - 3);
                    top = top != 0.0 ? a : b;
                    sp -= 2;
                } else {                               // binary: a = the value below the top, b = the top
                    const double a = st.get(sp - 2), b = top;
                    --sp;
                    if (code == OP_ADD) top = a + b;
                    else if (code == OP_MUL) top = a * b;
                    else if (code == OP_DIV) top = a / b;
                    else if (code == OP_POW) top = pow(a, b);
                    else if (code == OP_LT) top = a < b ? 1.0 : 0.0;
                    else if (code == OP_LE) top = a <= b ? 1.0 : 0.0;
                    else if (code == OP_EQ) top = a == b ? 1.0 : 0.0;
                    else top = (a != 0.0 && b != 0.0) ? 1.0 : 0.0;      // OP_AND
                }
            }
            L *= top;
        }
        out[c] = L;
    }
}

}   // namespace bllp
