"""
A likelihood program (bayesloop_amd/likprogram.py, csrc/blhip_likprog.hpp) interpreted in longdouble with a running error bound, in the
style of tests/highprec.py: every stack value is a pair (v, e), v the longdouble value of the program's own sequence of operations on its
float64 inputs and e >= |a float64 evaluation - v|, an absolute first-order bound WITHOUT slack.

Counts (u = 2**-53), as DESIGN.md 4.3b states them:
    + * / sqrt      1 u of the result, the operands' bounds carried through (|b| e_a + |a| e_b; e_a / |b| + |a| e_b / b^2; e_a / (2 sqrt a))
    neg abs         exact
    exp             1 u + its conditioning: the argument's ABSOLUTE bound is the result's relative one (v expm1(e_a))
    log             1 u + e_a / |a|
    pow             2 u + |y| e_x / |x| + |ln x| e_y relative
    powi n          |n| - 1 multiplications (+ 1 for the reciprocal of a negative exponent): that many u, + |n| e_x / |x| relative
    cos sin         C_TRIG u of the result + e_a absolute (|d cos| <= |d arg|); C_TRIG: twice the largest error MEASURED on the GPU over
                    the tests' argument range [-40, 40] (tests/LIKELIHOOD_PROGRAMS.md), no count of the library's algorithm exists here
    CONST           the rounded operations of a host that forms the constant from the expression (Program.const_ops), in u of its value
    PARAM DATA STEP AXIS     inputs, taken as given (STEP / AXIS values are evaluated on the host by the reference's own functions)
    LT LE EQ AND SELECT      exact (the operands of the comparisons in these densities are inputs and constants)
    every product / quotient additionally one subnormal step TINY
The product over the data dimensions of a step: one more u per factor.  The device is held to TWICE this bound (the project's
convention for the likelihood kernels), a float64 numpy evaluation and the model's own pdf to the bound itself.
"""
import numpy as np

from bayesloop_amd import _abi

U = 2.0 ** -53
TINY = 2.0 ** -1074
LD = np.longdouble
EXTENDED = np.finfo(np.longdouble).nmant >= 63
C_TRIG = 2.1          # twice the 1.031 u (cos) / 1.018 u (sin) measured on the MI355X against longdouble on [-40, 40], rounded up
SMALL = 1e-290        # cells whose longdouble value is below this (or not finite) are compared by class only
DEVICE_SLACK = 2.0


def _powi(x, n):
    e, r, b = abs(int(n)), None, x
    while e:
        if e & 1:
            r = b if r is None else r * b
        e >>= 1
        if e:
            b = b * b
    if r is None:
        r = np.ones_like(x)
    return LD(1) / r if n < 0 else r


def interpret(program, marginal, x, step_values=None):
    """-> (v, e): the density of ONE datum on the grid (shape of the marginals, last parameter fastest) in longdouble, and the bound."""
    nd = len(marginal)
    shape = tuple(len(m) for m in marginal)

    def along(v, k):
        idx = [None] * nd
        idx[k] = slice(None)
        return np.broadcast_to(np.asarray(v, dtype=LD)[tuple(idx)], shape)
    g = [along(m, k) for k, m in enumerate(marginal)]
    if step_values is None:
        step_values = program.step_values(np.array([x]))[0]
    tabs = [along(np.asarray(f(np.asarray(marginal[k], dtype=np.float64)), dtype=np.float64) * np.ones(len(marginal[k])), k)
            for k, f in program.axis_functions]
    u, tiny = LD(U), LD(TINY)
    zero = np.zeros(shape, dtype=LD)
    full = lambda c: np.full(shape, LD(c), dtype=LD)          # noqa: E731
    st = []
    with np.errstate(all='ignore'):
        for code, arg in program.ops:
            if code == _abi.LP_CONST:
                c = float(program.consts[arg])
                st.append((full(c), full(abs(c) * U * program.const_ops[arg]) if c == c and abs(c) != np.inf else zero))
            elif code == _abi.LP_PARAM:
                st.append((g[arg], zero))
            elif code == _abi.LP_DATA:
                st.append((full(x), zero))
            elif code == _abi.LP_STEP:
                st.append((full(step_values[arg]), zero))
            elif code == _abi.LP_AXIS:
                st.append((tabs[arg], zero))
            elif code == _abi.LP_SELECT:
                (c, _), (b, eb), (a, ea) = st.pop(), st.pop(), st.pop()
                st.append((np.where(c != 0, a, b), np.where(c != 0, ea, eb)))
            elif code == _abi.LP_NEG:
                a, ea = st.pop()
                st.append((-a, ea))
            elif code == _abi.LP_ABS:
                a, ea = st.pop()
                st.append((np.abs(a), ea))
            elif code == _abi.LP_SQRT:
                a, ea = st.pop()
                v = np.sqrt(a)
                st.append((v, ea / (2 * v) + u * v))
            elif code == _abi.LP_EXP:
                a, ea = st.pop()
                v = np.exp(a)
                st.append((v, np.where(v == 0, LD(0), v * (np.expm1(np.minimum(ea, LD(11000))) + u)) + tiny))
            elif code == _abi.LP_LOG:
                a, ea = st.pop()
                v = np.log(a)
                st.append((v, ea / np.abs(a) + u * np.abs(v)))
            elif code in (_abi.LP_COS, _abi.LP_SIN):
                a, ea = st.pop()
                v = np.cos(a) if code == _abi.LP_COS else np.sin(a)
                st.append((v, ea + C_TRIG * u * np.abs(v)))
            elif code == _abi.LP_POWI:
                a, ea = st.pop()
                v = _powi(a, arg)
                n = abs(int(arg))
                st.append((v, np.abs(v) * (n * ea / np.abs(a) + (max(n - 1, 0) + (1 if arg < 0 else 0)) * u) + tiny))
            else:
                (b, eb), (a, ea) = st.pop(), st.pop()
                if code == _abi.LP_ADD:
                    v = a + b
                    st.append((v, ea + eb + u * np.abs(v)))
                elif code == _abi.LP_MUL:
                    v = a * b
                    st.append((v, np.abs(b) * ea + np.abs(a) * eb + ea * eb + u * np.abs(v) + tiny))
                elif code == _abi.LP_DIV:
                    v = a / b
                    st.append((v, ea / np.abs(b) + np.abs(v) * eb / np.maximum(np.abs(b) - eb, tiny) + u * np.abs(v) + tiny))
                elif code == _abi.LP_POW:
                    v = np.power(a, b)
                    st.append((v, np.abs(v) * (np.abs(b) * ea / np.abs(a) + np.abs(np.log(a)) * eb + 2 * u) + tiny))
                else:
                    one = LD(1)
                    v = {_abi.LP_LT: lambda: (a < b) * one, _abi.LP_LE: lambda: (a <= b) * one, _abi.LP_EQ: lambda: (a == b) * one,
                         _abi.LP_AND: lambda: ((a != 0) & (b != 0)) * one}[code]()
                    st.append((v, zero))
    assert len(st) == 1
    return st[0]


def likelihood(program, marginal, segment):
    """processedPdf of one time step (observationModels.py:35-56) -> (L, E): the product over the non-NaN data dimensions."""
    shape = tuple(len(m) for m in marginal)
    L, E = np.ones(shape, dtype=LD), np.zeros(shape, dtype=LD)
    with np.errstate(all='ignore'):
        for x in np.asarray(segment, dtype=np.float64).reshape(-1):
            if x == x:
                v, e = interpret(program, marginal, float(x))
                L, E = L * v, np.abs(v) * E + np.abs(L) * e + E * e + LD(U) * np.abs(L * v) + LD(TINY)
    return L, E


def table(program, marginal, data):
    """(T, data_dim) data -> (L (T, *grid), E (T, *grid))"""
    rows = [likelihood(program, marginal, seg) for seg in np.asarray(data, dtype=np.float64)]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def classes(want):
    """Cells compared by class only: the longdouble value is below SMALL in magnitude or not finite."""
    w = np.asarray(want)
    return ~np.isfinite(w) | (np.abs(w) < SMALL)


def compare(got, want, bound, slack=1.0):
    """-> (worst |got - want| / (slack bound) over the cells compared by value, fraction of cells compared by class, whether every such
    cell has the class of its longdouble value: NaN, +-inf, or below 10 SMALL -- zero and subnormal included)."""
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(want))
    w = np.asarray(want)
    cls = classes(w)
    with np.errstate(all='ignore'):
        err = np.abs(np.asarray(got, dtype=LD) - w)
        q = np.where(err == 0, LD(0), err / (LD(slack) * np.asarray(bound, dtype=LD)))
        q = np.where(np.isnan(q), LD(np.inf), q)
        worst = float(np.max(np.where(cls, LD(0), q))) if q.size else 0.0
        same = np.where(np.isnan(w), np.isnan(got), np.where(np.isinf(w), got == w.astype(np.float64), np.abs(got) < 10 * SMALL))
    return worst, float(np.mean(cls)), bool(np.all(same | ~cls))
