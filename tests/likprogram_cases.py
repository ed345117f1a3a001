"""The densities, grids and data of the likelihood-program tests (tests/test_likprogram.py on the CPU, tests/test_likprogram_gpu.py on the
GPU): one list, so that the CPU test shows the counted bound to be one the reference itself meets on exactly the cells the GPU test reads.

Grid shapes: the smallest that exercise the kernel's index maps -- 37 cells, 33 x 19, 5 x 7 x 6 (and 3 x 4 x 5 x 3 for the four-parameter
expression): odd sizes, no multiple of the wave, more than one axis length per dimension.  Every grid is an open interval chosen so that
fewer than 5 % of a case's cells fall below 1e-290 (those are compared by class only)."""
import numpy as np

SHAPES = {1: (37,), 2: (33, 19), 3: (5, 7, 6), 4: (3, 4, 5, 3)}
NAN = float('nan')

REAL = [0.6, 1.7, 2.9, 1.1, 2.2]                  # T = 5, one data dimension
REAL2 = [[0.6, 1.7], [NAN, 2.9], [1.1, NAN], [2.2, 0.4]]           # T = 4, two data dimensions, one NaN in each
SIGNED = [-1.3, 0.4, 2.6, -0.2, 1.5]
SIGNED2 = [[-1.3, 0.4], [NAN, 2.6], [-0.2, NAN], [1.5, 0.9]]
COUNTS = [3.0, 0.0, 7.0, 1.0, 12.0]
COUNTS2 = [[3.0, 0.0], [NAN, 7.0], [1.0, NAN], [12.0, 2.0]]
TRIALS = [1.0, 4.0, 2.0, 1.0, 6.0]                # (Geometric: k >= 1)
TRIALS2 = [[1.0, 4.0], [NAN, 2.0], [1.0, NAN], [6.0, 3.0]]
BITS = [1.0, 0.0, 1.0, 1.0, 0.0]
BITS2 = [[1.0, 0.0], [NAN, 1.0], [0.0, NAN], [1.0, 1.0]]
TENS = [3.0, 10.0, 0.0, 7.0, 5.0]                 # (Binomial(10, p))
TENS2 = [[3.0, 10.0], [NAN, 0.0], [7.0, NAN], [5.0, 4.0]]


def open_grid(lo, hi, n):
    return np.linspace(lo, hi, n + 2)[1:-1]


def _sympy_models():
    import sympy
    import sympy.stats as st
    s = lambda name: sympy.Symbol(name, real=True)            # noqa: E731
    p = lambda name: sympy.Symbol(name, positive=True)        # noqa: E731
    mu, x0, a_, b_, m_ = s('mu'), s('x0'), s('a'), s('b'), s('m')
    sig, rate, bb, gam, al, be, xm, pp, lam, ss, aa, dp = (p(n) for n in ('sigma', 'rate', 'b', 'gamma', 'alpha', 'beta', 'xm', 'p', 'lamda', 's', 'a', 'dp'))
    return [
        # name, random variable, [(parameter name, lo, hi)], data (T = 5), data (T = 4, two dimensions)
        ('Normal', st.Normal('rv', mu, sig), [('mu', -2, 3), ('sigma', 0.1, 2)], SIGNED, SIGNED2),
        ('Exponential', st.Exponential('rv', rate), [('rate', 0.1, 5)], REAL, REAL2),
        ('Laplace', st.Laplace('rv', mu, bb), [('mu', -2, 3), ('b', 0.1, 2)], SIGNED, SIGNED2),
        ('Cauchy', st.Cauchy('rv', x0, gam), [('x0', -2, 3), ('gamma', 0.1, 2)], SIGNED, SIGNED2),
        ('LogNormal', st.LogNormal('rv', mu, sig), [('mu', -1, 1), ('sigma', 0.2, 1.5)], REAL, REAL2),
        ('Weibull', st.Weibull('rv', al, be), [('alpha', 0.5, 3), ('beta', 0.5, 3)], REAL, REAL2),
        ('Rayleigh', st.Rayleigh('rv', sig), [('sigma', 0.3, 3)], REAL, REAL2),
        ('Logistic', st.Logistic('rv', mu, ss), [('mu', -2, 3), ('s', 0.2, 2)], SIGNED, SIGNED2),
        ('Pareto', st.Pareto('rv', xm, al), [('xm', 0.05, 0.35), ('alpha', 0.5, 4)], REAL, REAL2),
        ('Geometric', st.Geometric('rv', pp), [('p', 0.02, 0.98)], TRIALS, TRIALS2),
        ('Poisson', st.Poisson('rv', lam), [('lamda', 0.2, 12)], COUNTS, COUNTS2),
        ('Uniform', st.Uniform('rv', a_, b_), [('a', -3, -1.2), ('b', 2.5, 4)], SIGNED, SIGNED2),
        ('Bernoulli', st.Bernoulli('rv', pp), [('p', 0.02, 0.98)], BITS, BITS2),
        ('Binomial', st.Binomial('rv', 10, pp), [('p', 0.02, 0.98)], TENS, TENS2),
        ('Frechet', st.Frechet('rv', aa, ss, m_), [('a', 0.5, 3), ('s', 0.5, 2), ('m', -1, 0.3)], REAL, REAL2),
        ('Dagum', st.Dagum('rv', dp, aa, bb), [('dp', 0.5, 3), ('a', 0.5, 3), ('b', 0.5, 2)], REAL, REAL2),
    ]


def _scipy_models():
    import scipy.stats as ss
    return [
        ('scipy.norm', ss.norm, [('loc', -2, 3), ('scale', 0.1, 2)], {}, SIGNED, SIGNED2),
        ('scipy.expon', ss.expon, [('scale', 0.2, 4)], {'loc': 0.25}, REAL, REAL2),
        ('scipy.laplace', ss.laplace, [('loc', -2, 3), ('scale', 0.1, 2)], {}, SIGNED, SIGNED2),
        ('scipy.cauchy', ss.cauchy, [('loc', -2, 3), ('scale', 0.1, 2)], {}, SIGNED, SIGNED2),
        ('scipy.poisson', ss.poisson, [('mu', 0.2, 12)], {'loc': 0}, COUNTS, COUNTS2),
        ('scipy.t', ss.t, [('df', 1.5, 9), ('loc', -2, 3), ('scale', 0.1, 2)], {}, SIGNED, SIGNED2),
    ]


class Case:
    """model: the bl.om model (None where the installed SymPy cannot lambdify the density, so that bl.om.SymPy cannot be constructed --
    Binomial's Contains(x, Integers) under SymPy 1.14: the expression is then compiled directly, and `pdf` is the lambdified branch of
    the density's Piecewise that holds on the data of the case, every datum being an integer in 0 .. 10)."""

    def __init__(self, name, model, params, data1, data2, expression=None, pdf=None):
        self.name, self.model, self.expression, self._pdf = name, model, expression, pdf
        shape = SHAPES[len(params)]
        self.marginal = [open_grid(lo, hi, n) for (_, lo, hi), n in zip(params, shape)]
        self.data = {1: np.array(data1, dtype=float).reshape(-1, 1), 2: np.array(data2, dtype=float)}

    @property
    def grid(self):
        return np.meshgrid(*self.marginal, indexing='ij')

    def program(self):
        if self.model is not None:
            return self.model.likelihoodProgram()
        from bayesloop_amd import likprogram
        expr, x, symbols = self.expression
        return likprogram.compile_density(expr, x, symbols)

    def own_likelihood(self, segment):
        """the model's own processedPdf of one step (lambdified / SciPy), on the case's grid"""
        shape = [len(m) for m in self.marginal]
        if self.model is not None:
            seg = np.asarray(segment, dtype=float).reshape(1, -1)
            return np.asarray(self.model.processedPdf(self.grid, seg if seg.shape[1] > 1 else seg[0]), dtype=float) * np.ones(shape)
        L = np.ones(shape)
        for v in np.asarray(segment, dtype=float).reshape(-1):
            if v == v:
                L = L * self._pdf(v, *self.grid)
        return L


_CASES = []


def cases():
    """[Case]: every bl.om.SymPy density of the list and every bl.om.SciPy distribution written out in bayesloop_amd/likprogram.py."""
    if not _CASES:
        import bayesloop_amd as bl
        import contextlib
        import io
        for name, rv, params, d1, d2 in _sympy_models():
            args = []
            for pn, lo, hi in params:
                args += [pn, None]
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    om = bl.om.SymPy(rv, *args, determineJeffreysPrior=False)
                _CASES.append(Case(name, om, params, d1, d2))
            except Exception:       # noqa: BLE001 -- the density cannot be lambdified by the installed SymPy
                import sympy
                import sympy.abc
                from sympy.stats import density
                assert name == 'Binomial', name
                expr = density(rv)(sympy.abc.x)
                symbols = [s for pn, _, _ in params for s in expr.free_symbols if str(s) == pn]
                _CASES.append(Case(name, None, params, d1, d2, expression=(expr, sympy.abc.x, symbols),
                                   pdf=sympy.lambdify([sympy.abc.x] + symbols, expr.args[0][0], modules=['scipy', 'numpy'])))
        for name, rv, params, fixed, d1, d2 in _scipy_models():
            args = []
            for pn, lo, hi in params:
                args += [pn, None]
            _CASES.append(Case(name, bl.om.SciPy(rv, *args, fixedParameters=fixed), params, d1, d2))
    return _CASES


def case_names():
    return [n for n, *_ in _sympy_models()] + [n for n, *_ in _scipy_models()]


def four_parameter_expression():
    """No density of the list has four parameters: a Normal density times a Cauchy-shaped factor, in (mu, sigma, a, b), compiled directly.
    -> (expression, x, [symbols], marginal grids, data T = 5, data T = 4 x 2)"""
    import sympy
    x = sympy.Symbol('x', real=True)
    mu, sig, a, b = sympy.Symbol('mu', real=True), sympy.Symbol('sigma', positive=True), sympy.Symbol('a', positive=True), sympy.Symbol('b', positive=True)
    expr = sympy.exp(-(x - mu) ** 2 / (2 * sig ** 2)) / (sympy.sqrt(2 * sympy.pi) * sig) * a / (1 + b * x ** 2)
    marg = [open_grid(lo, hi, n) for (lo, hi), n in zip([(-2, 3), (0.2, 2), (0.5, 2), (0.1, 3)], SHAPES[4])]
    return expr, x, [mu, sig, a, b], marg, np.array(SIGNED).reshape(-1, 1), np.array(SIGNED2)
