"""
Likelihood programs: the density of a ``bl.om.SymPy`` / ``bl.om.SciPy`` observation model as a small postfix program over the data
point and the grid's parameters, evaluated per cell by ONE HIP kernel (``bllp::lik_program_kernel``, csrc/blhip_likprog.hpp) instead
of once per time step by the lambdified density on the host (reference observationModels.py:35-56, :272-391).

:func:`compile_density` walks the SymPy expression tree:

* numeric subtrees are folded into float64 constants (``CONST``); ``Pow`` with an integer exponent becomes ``POWI`` (``x**2`` is
  ``x * x``, as in numpy), with exponent +-1/2 ``SQRT``; ``Piecewise`` becomes a chain of ``SELECT``;
* a subtree of the data point alone that holds anything outside the instruction set (``factorial(x)``, ``binomial(10, x)``,
  ``Contains(x, Integers)``) is HOISTED: it is evaluated on the host, per (time step, data dimension), by the same lambdify modules the
  model's own density uses, and enters the program as a ``STEP`` value -- bit-identical to the reference;
* with ``axis_functions=True`` (bl.om.SciPy) a subtree of ONE parameter alone that holds a function outside the set (``loggamma(df)``)
  is tabulated along that parameter's axis on the host and read as an ``AXIS`` operand;
* anything else outside the set (``besseli(0, k)`` of a parameter in VonMises) makes the density uncompilable: ``None``, and the model
  keeps the host-evaluated table.
"""
from __future__ import annotations

import numpy as np

from . import _abi

_PUSH = (_abi.LP_CONST, _abi.LP_PARAM, _abi.LP_DATA, _abi.LP_STEP, _abi.LP_AXIS)
_UNARY = (_abi.LP_NEG, _abi.LP_ABS, _abi.LP_SQRT, _abi.LP_EXP, _abi.LP_LOG, _abi.LP_COS, _abi.LP_SIN, _abi.LP_POWI)
_BINARY = (_abi.LP_ADD, _abi.LP_MUL, _abi.LP_DIV, _abi.LP_POW, _abi.LP_LT, _abi.LP_LE, _abi.LP_EQ, _abi.LP_AND)
NAMES = ('CONST', 'PARAM', 'DATA', 'STEP', 'AXIS', 'ADD', 'MUL', 'DIV', 'NEG', 'ABS', 'SQRT', 'EXP', 'LOG', 'POW', 'COS', 'SIN', 'POWI',
         'LT', 'LE', 'EQ', 'AND', 'SELECT')


class _Unsupported(Exception):
    pass


def powi(x, n):
    """x**n by squaring, the multiplications of the device's POWI (n = 2: x * x)."""
    e, r, b = abs(int(n)), None, x
    while e:
        if e & 1:
            r = b if r is None else r * b
        e >>= 1
        if e:
            b = b * b
    if r is None:
        r = np.ones_like(x)
    return 1.0 / r if n < 0 else r


class Program:
    """ops: (n_ops, 2) int32 [code, arg]; consts: float64; const_ops: per constant, the rounded float64 operations a host that forms it
    from the expression (lambdify) performs -- what tests/likprogram_ref.py counts for it; step_functions: one callable f(x) per STEP
    value; axis_functions: [(parameter index, callable f(marginal grid))] behind the AXIS operands, whose arg holds the function's index
    until :meth:`bind` places its table among the constants."""

    def __init__(self, ops, consts, const_ops, step_functions, axis_functions, n_params):
        self.ops = np.asarray(ops, dtype=np.int32).reshape(-1, 2)
        self.consts = np.asarray(consts, dtype=np.float64)
        self.const_ops = list(const_ops)
        self.step_functions = list(step_functions)
        self.axis_functions = list(axis_functions)
        self.n_params = n_params

    @property
    def n_step(self):
        return len(self.step_functions)

    def step_values(self, data):
        """data (T, data_dim) -> (T, data_dim, n_step) float64; a NaN datum (a factor of 1, never evaluated) gets zeros."""
        data = np.asarray(data, dtype=np.float64)
        out = np.zeros(data.shape + (self.n_step,))
        for i, x in np.ndenumerate(data):
            if x == x:
                for j, f in enumerate(self.step_functions):
                    out[i + (j,)] = float(f(x))
        return out

    def bind(self, marginal):
        """-> (ops, consts) as the library takes them: the tables of the AXIS operands, evaluated on the marginal grids, appended to the
        constants and the operands' args set to axis | offset << 2."""
        if not self.axis_functions:
            return self.ops, self.consts
        consts, offsets = [self.consts], []
        at = len(self.consts)
        for k, f in self.axis_functions:
            tab = np.asarray(f(np.asarray(marginal[k], dtype=np.float64)), dtype=np.float64) * np.ones(len(marginal[k]))
            offsets.append(at)
            consts.append(tab)
            at += len(tab)
        ops = self.ops.copy()
        for row in ops:
            if row[0] == _abi.LP_AXIS:
                k = self.axis_functions[row[1]][0]
                row[1] = k | (offsets[row[1]] << 2)
        return ops, np.concatenate(consts)

    def evaluate(self, marginal, x, step_values=None, dtype=np.float64):
        """The density of ONE datum x on the grid of the marginal values (last parameter fastest), by the program's own order of
        operations in `dtype` arithmetic: what the kernel computes per cell and data dimension."""
        shape = [len(m) for m in marginal]
        nd = len(marginal)

        def along(v, k):
            idx = [None] * nd
            idx[k] = slice(None)
            return np.asarray(v, dtype=dtype)[tuple(idx)]
        g = [along(m, k) for k, m in enumerate(marginal)]
        if step_values is None:
            step_values = self.step_values(np.array([x]))[0]
        axis_tabs = [along(np.asarray(f(np.asarray(marginal[k], dtype=np.float64)), dtype=np.float64) * np.ones(len(marginal[k])), k)
                     for k, f in self.axis_functions]
        st = []
        with np.errstate(all='ignore'):
            for code, arg in self.ops:
                if code == _abi.LP_CONST:
                    st.append(np.asarray(self.consts[arg], dtype=dtype))
                elif code == _abi.LP_PARAM:
                    st.append(g[arg])
                elif code == _abi.LP_DATA:
                    st.append(np.asarray(x, dtype=dtype))
                elif code == _abi.LP_STEP:
                    st.append(np.asarray(step_values[arg], dtype=dtype))
                elif code == _abi.LP_AXIS:
                    st.append(axis_tabs[arg])
                elif code == _abi.LP_SELECT:
                    c, b, a = st.pop(), st.pop(), st.pop()
                    st.append(np.where(c != 0, a, b))
                elif code in _UNARY:
                    a = st.pop()
                    st.append({_abi.LP_NEG: lambda: -a, _abi.LP_ABS: lambda: np.abs(a), _abi.LP_SQRT: lambda: np.sqrt(a),
                               _abi.LP_EXP: lambda: np.exp(a), _abi.LP_LOG: lambda: np.log(a), _abi.LP_COS: lambda: np.cos(a),
                               _abi.LP_SIN: lambda: np.sin(a), _abi.LP_POWI: lambda: powi(a, arg)}[code]())
                else:
                    b, a = st.pop(), st.pop()
                    one = np.asarray(1.0, dtype=dtype)
                    st.append({_abi.LP_ADD: lambda: a + b, _abi.LP_MUL: lambda: a * b, _abi.LP_DIV: lambda: a / b,
                               _abi.LP_POW: lambda: np.power(a, b), _abi.LP_LT: lambda: (a < b) * one, _abi.LP_LE: lambda: (a <= b) * one,
                               _abi.LP_EQ: lambda: (a == b) * one, _abi.LP_AND: lambda: ((a != 0) & (b != 0)) * one}[code]())
        assert len(st) == 1
        return np.broadcast_to(st[0], shape).astype(dtype)

    def likelihood(self, marginal, segment, dtype=np.float64):
        """processedPdf of one time step (observationModels.py:35-56): the product over the data dimensions, a NaN datum counting 1."""
        L = np.ones([len(m) for m in marginal], dtype=dtype)
        for x in np.asarray(segment, dtype=np.float64).reshape(-1):
            if x == x:
                L = L * self.evaluate(marginal, x, dtype=dtype)
        return L

    def __str__(self):
        return ' '.join(NAMES[c] + (str(a) if c in _PUSH[:2] + _PUSH[3:] + (_abi.LP_POWI,) else '') for c, a in self.ops)


def _host_function(symbol, e, modules):
    """A subtree of one symbol as a host function of float64 values: the lambdified subtree (the reference's own way to evaluate it);
    where the printer has no numpy form for a node (Contains(x, Integers), binomial(10, x) in some SymPy versions) or the generated code
    fails, SymPy's own evaluation at the exact rational value of the float."""
    import sympy
    try:
        fast = sympy.lambdify([symbol], e, modules=modules)
    except Exception:           # noqa: BLE001 -- whatever the printer raises for a node it does not know
        fast = None

    def exact(v):
        r = e.subs(symbol, sympy.Rational(float(v)) if float(v) != int(float(v)) else sympy.Integer(int(float(v))))
        if r in (sympy.true, sympy.false):
            return 1.0 if r is sympy.true else 0.0
        return float(sympy.N(r, 30))

    def f(v):
        if fast is not None:
            try:
                with np.errstate(all='ignore'):
                    return np.asarray(fast(v), dtype=np.float64)
            except Exception:   # noqa: BLE001
                pass
        return np.vectorize(exact, otypes=[np.float64])(v)
    return f


def stack_depth(ops):
    """(largest depth, final depth) of a program; raises ValueError on underflow."""
    depth = top = 0
    for code, _ in ops:
        need = 0 if code in _PUSH else 1 if code in _UNARY else 3 if code == _abi.LP_SELECT else 2
        if depth < need:
            raise ValueError('stack underflow')
        depth += 1 - need
        top = max(top, depth)
    return top, depth


def compile_density(expr, x, parameters, modules=None, axis_functions=False):
    """expr: the SymPy expression of the density in the data symbol `x` and the symbols `parameters` (in the order of the grid's axes).
    modules: the lambdify modules the hoisted subtrees are evaluated with (default: numpy + SciPy's factorial / Bessel function, as
    bl.om.SymPy's own density).  Returns a :class:`Program`, or None when the tree holds anything outside the instruction set after
    hoisting, needs more than 256 ops or a stack deeper than 16."""
    import sympy
    from sympy.logic.boolalg import BooleanTrue, BooleanFalse, And
    from sympy.core.relational import Lt, Le, Gt, Ge, Eq, Ne
    if modules is None:
        from scipy.special import factorial, iv
        modules = ['numpy', {'factorial': factorial, 'besseli': iv}]
    parameters = list(parameters)
    known = set(parameters) | {x}
    ops, consts, const_ops, step_fns, step_keys, axis_fns, axis_keys = [], [], [], [], [], [], []
    in_set = (sympy.Add, sympy.Mul, sympy.Pow, sympy.exp, sympy.log, sympy.Abs, sympy.cos, sympy.sin, sympy.Piecewise, sympy.Symbol,
              sympy.Number, sympy.NumberSymbol, Lt, Le, Gt, Ge, Eq, Ne, And, BooleanTrue, BooleanFalse)

    def inside(e):
        return all(isinstance(n, in_set) for n in sympy.preorder_traversal(e))

    def const(value, nops):
        value = float(value)
        for i, c in enumerate(consts):
            if (c == value and np.signbit(c) == np.signbit(value)) or (c != c and value != value):
                const_ops[i] = max(const_ops[i], nops)
                ops.append((_abi.LP_CONST, i))
                return
        consts.append(value)
        const_ops.append(nops)
        ops.append((_abi.LP_CONST, len(consts) - 1))

    def fold(e):
        """a numeric subtree -> (float64 value, rounded operations of a host that forms it operation by operation)"""
        if e is sympy.true:
            return 1.0, 0
        if e is sympy.false:
            return 0.0, 0
        if e.is_Rational:
            v = float(e)
            return v, 0 if sympy.Rational(v) == e else 1
        v = complex(sympy.N(e, 40))
        if v.imag != 0:
            raise _Unsupported('complex constant %s' % e)
        return v.real, 1 + sum(1 for _ in sympy.preorder_traversal(e))

    def emit(e):
        free = e.free_symbols
        if not free.issubset(known):
            raise _Unsupported('unknown symbols in %s' % e)
        if not free:
            const(*fold(e))
        elif e == x:
            ops.append((_abi.LP_DATA, 0))
        elif e in parameters:
            ops.append((_abi.LP_PARAM, parameters.index(e)))
        elif free == {x} and not inside(e):
            # a data-only subtree with something outside the instruction set: evaluated on the host per (step, data dimension)
            if e not in step_keys:
                step_keys.append(e)
                step_fns.append(_host_function(x, e, modules))
            ops.append((_abi.LP_STEP, step_keys.index(e)))
        elif axis_functions and len(free) == 1 and x not in free and not inside(e):
            # a subtree of one parameter with something outside the set: tabulated along that parameter's axis on the host
            if e not in axis_keys:
                axis_keys.append(e)
                axis_fns.append((parameters.index(next(iter(free))), _host_function(next(iter(free)), e, modules)))
            ops.append((_abi.LP_AXIS, axis_keys.index(e)))
        elif isinstance(e, sympy.Add):
            numeric = [a for a in e.args if not a.free_symbols]
            rest = [a for a in e.args if a.free_symbols]
            for i, a in enumerate(rest):
                emit(a)
                if i:
                    ops.append((_abi.LP_ADD, 0))
            if numeric:
                const(*fold(sympy.Add(*numeric)))
                ops.append((_abi.LP_ADD, 0))
        elif isinstance(e, sympy.Mul):
            numeric = [a for a in e.args if not a.free_symbols]
            num, den = [], []
            for a in e.args:
                if not a.free_symbols:
                    continue
                if isinstance(a, sympy.Pow) and a.exp.is_number and a.exp.is_real and a.exp < 0:
                    den.append(sympy.Pow(a.base, -a.exp))
                else:
                    num.append(a)
            c, cops = fold(sympy.Mul(*numeric)) if numeric else (1.0, 0)

            def product(factors):
                for i, a in enumerate(factors):
                    emit(a)
                    if i:
                        ops.append((_abi.LP_MUL, 0))
            if num:
                product(num)
                if c == -1.0:
                    ops.append((_abi.LP_NEG, 0))
                elif c != 1.0:
                    const(c, cops)
                    ops.append((_abi.LP_MUL, 0))
            else:
                const(c, cops)
            if den:
                product(den)
                ops.append((_abi.LP_DIV, 0))
        elif isinstance(e, sympy.exp):
            emit(e.args[0])
            ops.append((_abi.LP_EXP, 0))
        elif isinstance(e, sympy.Pow):
            b, p = e.base, e.exp
            if b == sympy.E:
                emit(p)
                ops.append((_abi.LP_EXP, 0))
            elif p.is_Integer and abs(int(p)) <= _abi.LP_MAX_POWI:
                emit(b)
                ops.append((_abi.LP_POWI, int(p)))
            elif p == sympy.Rational(1, 2) or p == sympy.Rational(-1, 2):
                emit(b)
                ops.append((_abi.LP_SQRT, 0))
                if p < 0:
                    ops.append((_abi.LP_POWI, -1))
            else:
                emit(b)
                emit(p)
                ops.append((_abi.LP_POW, 0))
        elif isinstance(e, (sympy.log, sympy.Abs, sympy.cos, sympy.sin)):
            if len(e.args) != 1:
                raise _Unsupported(str(e))
            emit(e.args[0])
            ops.append(({sympy.log: _abi.LP_LOG, sympy.Abs: _abi.LP_ABS, sympy.cos: _abi.LP_COS, sympy.sin: _abi.LP_SIN}[type(e)], 0))
        elif isinstance(e, sympy.Piecewise):
            def chain(pairs):
                (val, cond), rest = pairs[0], pairs[1:]
                if cond is sympy.true:
                    emit(val)
                    return
                emit(val)
                if rest:
                    chain(rest)
                else:
                    const(float('nan'), 0)            # numpy.select's default where no condition holds
                emit(cond)
                ops.append((_abi.LP_SELECT, 0))
            chain(list(e.args))
        elif isinstance(e, (Lt, Le, Gt, Ge, Eq, Ne)):
            a, b = e.args
            if isinstance(e, (Gt, Ge)):
                a, b = b, a
            if isinstance(e, Ne):
                const(1.0, 0)
            emit(a)
            emit(b)
            ops.append((_abi.LP_LT if isinstance(e, (Lt, Gt)) else _abi.LP_LE if isinstance(e, (Le, Ge)) else _abi.LP_EQ, 0))
            if isinstance(e, Ne):
                ops.append((_abi.LP_NEG, 0))
                ops.append((_abi.LP_ADD, 0))
        elif isinstance(e, And):
            for i, a in enumerate(e.args):
                emit(a)
                if i:
                    ops.append((_abi.LP_AND, 0))
        else:
            raise _Unsupported('%s is outside the instruction set' % type(e).__name__)

    try:
        emit(sympy.sympify(expr))
        top, final = stack_depth(ops)
    except (_Unsupported, ValueError, TypeError):
        return None
    if final != 1 or top > _abi.LP_MAX_STACK or len(ops) > _abi.LP_MAX_OPS:
        return None
    return Program(ops, consts, const_ops, step_fns, axis_fns, len(parameters))


# ---- bl.om.SciPy: the distributions whose closed form is written here ------------------------------------------------------------------
# Each entry: the density / mass function in the data symbol x, loc, scale (continuous ones) and the distribution's shape parameters, as
# scipy.stats evaluates it.  A distribution is listed only if its program, evaluated in numpy, agrees with SciPy's own pdf / pmf within
# the program's counted bound plus 8 u on the test grids (tests/test_likprogram.py; tests/LIKELIHOOD_PROGRAMS.md lists the ones refused).

def scipy_density(name):
    """-> (expression, x, {parameter name: symbol}) of scipy.stats.<name>, or None when the distribution is not on the list."""
    import sympy
    x, loc, scale = sympy.Symbol('x', real=True), sympy.Symbol('loc', real=True), sympy.Symbol('scale', positive=True)
    z = (x - loc) / scale
    pi = sympy.pi
    if name == 'norm':
        return sympy.exp(-z ** 2 / 2) / sympy.sqrt(2 * pi) / scale, x, {'loc': loc, 'scale': scale}
    if name == 'expon':
        return sympy.Piecewise((sympy.exp(-z) / scale, z >= 0), (0, True)), x, {'loc': loc, 'scale': scale}
    if name == 'laplace':
        return sympy.exp(-sympy.Abs(z)) / 2 / scale, x, {'loc': loc, 'scale': scale}
    if name == 'cauchy':
        return 1 / (pi * (1 + z ** 2)) / scale, x, {'loc': loc, 'scale': scale}
    if name == 'poisson':
        mu = sympy.Symbol('mu', positive=True)
        k = x - loc
        # scipy.stats.poisson._pmf: exp(xlogy(k, mu) - gammaln(k + 1) - mu); zero off the non-negative integers
        pmf = sympy.exp(k * sympy.log(mu) - sympy.loggamma(k + 1) - mu)
        return sympy.Piecewise((pmf, sympy.And(k >= 0, sympy.Eq(sympy.floor(k), k))), (0, True)), x, {'mu': mu, 'loc': loc}
    if name == 't':
        df = sympy.Symbol('df', positive=True)
        # scipy.stats.t._logpdf: log(poch(df / 2, 1 / 2)) - (log(df) + log(pi)) / 2 - (df + 1) / 2 log1p(z^2 / df); the first term, a
        # function of df alone, is tabulated along the df axis by SciPy's own poch (an AXIS operand)
        logpdf = (sympy.log(sympy.RisingFactorial(df / 2, sympy.Rational(1, 2))) - (sympy.log(df) + sympy.log(pi)) / 2
                  - (df + 1) / 2 * sympy.log(1 + z ** 2 / df))
        return sympy.exp(logpdf) / scale, x, {'df': df, 'loc': loc, 'scale': scale}
    return None
