"""Likelihood programs on the CPU: the compiler (bayesloop_amd/likprogram.py), its numpy evaluation and the models' own pdfs against the
longdouble interpreter of tests/likprogram_ref.py, the fall-backs, what Study._compile emits, and the library's host-only validation.
Bounds, figures and the lists of admitted / refused distributions: tests/LIKELIHOOD_PROGRAMS.md."""
import ctypes

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi, likprogram

import likprogram_cases as lc
import likprogram_ref as ref
from oracle_engine import OracleEngine

pytestmark = pytest.mark.skipif(not ref.EXTENDED, reason='needs a long double wider than float64')

CLASS_CAP = 0.05


@pytest.fixture(scope='module')
def reference_tables():
    """(case name, data dimensions) -> (program, L, E): computed once, shared, never modified"""
    out = {}
    for c in lc.cases():
        p = c.program()
        for dd in (1, 2):
            out[c.name, dd] = (p,) + (ref.table(p, c.marginal, c.data[dd]) if p is not None else (None, None))
    return out


def _check_call(ops, n_consts, n_step, ndim):
    lib = _abi.load()
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 2)
    err = ctypes.create_string_buffer(256)
    rc = lib.blhip_host_lik_program_check(ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(ops), n_consts, n_step, ndim, err, 256)
    return rc, err.value.decode()


@pytest.mark.parametrize('dd', [1, 2])
@pytest.mark.parametrize('name', lc.case_names())
def test_program_and_own_pdf_lie_within_the_counted_bound(name, dd, reference_tables):
    """BOTH the program evaluated in float64 numpy and the model's own pdf (lambdified / SciPy) lie within the counted bound of the
    longdouble value, on exactly the grids and data the GPU test uses: the bound is one the reference itself meets.  Largest
    |error| / bound measured here: program 0.71 (Laplace), own pdf 0.71 (Laplace) / 0.66 (scipy.stats.norm); largest relative errors:
    470 u (Normal at sigma = 0.15: the exponent reaches 330), 271 u (Weibull), 180 u (Frechet) -- conditioning, which the bound counts."""
    c = [c for c in lc.cases() if c.name == name][0]
    p, L, E = reference_tables[name, dd]
    assert p is not None, 'the density does not compile'
    rc, msg = _check_call(p.bind(c.marginal)[0], len(p.bind(c.marginal)[1]), p.n_step, len(c.marginal))
    assert rc == 0, msg
    got = np.array([p.likelihood(c.marginal, seg) for seg in c.data[dd]])
    own = np.array([c.own_likelihood(seg) for seg in c.data[dd]])
    for what, val in (('program', got), ('own pdf', own)):
        worst, frac, same = ref.compare(val, L, E)
        print('%s / %s, %d data dimension(s): worst |error| / bound %.3f, %.1f %% of the cells by class' % (name, what, dd, worst, 100 * frac))
        assert frac <= CLASS_CAP, '%s: %.1f %% of the cells are compared by class only' % (name, 100 * frac)
        assert same, '%s: %s differs in class (zero / subnormal, inf, NaN) from the longdouble value' % (name, what)
        assert worst <= 1.0, '%s: %s misses the counted bound by a factor of %.3g' % (name, what, worst)
    if name.startswith('scipy.'):
        # the acceptance rule of the SciPy list: program against SciPy's own pdf / pmf within the counted bound plus 8 u
        with np.errstate(all='ignore'):
            excess = np.abs(got - own) - (np.asarray(E, dtype=float) + 8 * ref.U * np.abs(own))
        assert not (excess[~ref.classes(L)] > 0).any(), '%s is outside the acceptance rule of the SciPy list' % name


def test_four_parameter_expression():
    expr, x, symbols, marg, d1, d2 = lc.four_parameter_expression()
    import sympy
    p = likprogram.compile_density(expr, x, symbols)
    own = sympy.lambdify([x] + symbols, expr, modules='numpy')
    grid = np.meshgrid(*marg, indexing='ij')
    for data in (d1, d2):
        L, E = ref.table(p, marg, data)
        got = np.array([p.likelihood(marg, seg) for seg in data])
        ownv = np.array([np.prod([own(v, *grid) for v in seg if v == v], axis=0) * np.ones(L.shape[1:]) for seg in data])
        for val in (got, ownv):
            worst, frac, same = ref.compare(val, L, E)
            assert worst <= 1.0 and frac <= CLASS_CAP and same, (worst, frac, same)


def test_compiler_forms():
    """Piecewise -> SELECT chain, integer powers -> POWI, +-1/2 -> SQRT, folded rationals, hoisted data-only subtrees."""
    import sympy
    x, a, b = sympy.Symbol('x'), sympy.Symbol('a', positive=True), sympy.Symbol('b', positive=True)
    codes = lambda p: [int(c) for c, _ in p.ops]         # noqa: E731
    p = likprogram.compile_density(sympy.Piecewise((a, x < 0), (b, x < 1), (0, True)), x, [a, b])
    assert codes(p).count(_abi.LP_SELECT) == 2
    p = likprogram.compile_density(a ** 3 / sympy.sqrt(b) + x ** 2, x, [a, b])
    assert [int(v) for c, v in p.ops if c == _abi.LP_POWI] in ([3, 2], [2, 3]) and _abi.LP_SQRT in codes(p) and _abi.LP_POW not in codes(p)
    p = likprogram.compile_density(sympy.Rational(1, 3) * a * sympy.Rational(3, 4), x, [a])
    assert list(p.consts) == [0.25] and p.const_ops == [0]
    p = likprogram.compile_density(a ** x / sympy.factorial(x), x, [a])
    assert p.n_step == 1 and p.step_values(np.array([[4.0], [float('nan')]])).tolist() == [[[24.0]], [[0.0]]]
    np.testing.assert_allclose(p.evaluate([np.array([2.0])], 4.0), [16.0 / 24.0], rtol=1e-15)
    # a function of one parameter outside the set: refused for SymPy models, an AXIS table with axis_functions
    assert likprogram.compile_density(sympy.loggamma(a) * x, x, [a]) is None
    p = likprogram.compile_density(sympy.loggamma(a) * x, x, [a, b], axis_functions=True, modules=['scipy', 'numpy'])
    ops, consts = p.bind([np.array([1.5, 2.5, 3.5]), np.array([1.0])])
    k = [int(v) for c, v in ops if c == _abi.LP_AXIS][0]
    assert k & 3 == 0 and len(consts) == (k >> 2) + 3


def test_uncompilable_densities_keep_the_host_table():
    """VonMises (besseli(0, k) of a parameter) and a SciPy distribution outside the list compile to None; the study then fits through the
    host table exactly as before: _compile hands the model's own pdf over as a table, and the fit agrees with the oracle."""
    import contextlib
    import io
    import sympy
    import sympy.stats as st
    import scipy.stats
    import cases
    import compare
    import oracle_adapter as oa
    mu, k = sympy.Symbol('mu'), sympy.Symbol('k', positive=True)
    with contextlib.redirect_stdout(io.StringIO()):
        vm = bl.om.SymPy(st.VonMises('rv', mu, k), 'mu', bl.cint(-1, 1, 9), 'k', bl.oint(0.5, 3, 7), determineJeffreysPrior=False)
    assert vm.likelihoodProgram() is None
    assert bl.om.SciPy(scipy.stats.gumbel_r, 'loc', bl.cint(-1, 1, 9), 'scale', bl.oint(0.5, 3, 7)).likelihoodProgram() is None
    assert bl.om.SciPy(scipy.stats.gamma, 'a', bl.oint(0.5, 3, 7), fixedParameters={'loc': 0, 'scale': 1}).likelihoodProgram() is None

    class Stub(OracleEngine):
        lik_programs = True                      # even an engine that takes programs gets the table: there is no program
    prev = bl.set_engine(Stub())
    try:
        S = bl.Study()
        S.loadData(np.array([0.3, -0.2, 0.5, 0.1, -0.4]), silent=True)
        S.setOM(vm, silent=True)
        S.setTM(bl.tm.GaussianRandomWalk('s', 0.2, target='mu'), silent=True)
        S._formatData()
        problem, _ = S._compile()
        assert problem.obs_model == _abi.OM_TABLE and problem.lik_program is None
        want = np.array([vm.processedPdf(S.grid, seg) for seg in S.formattedData])
        assert np.array_equal(problem.lik, want)
        S.fit(silent=True)
        assert np.isfinite(S.logEvidence)
        c = dict(study='Study', data=('series', 40, 8),
                 om=('SciPy:gumbel_r', [('loc', ('cint', -3.0, 3.0, 16)), ('scale', ('oint', 0.2, 2.5, 12))], 'default'),
                 tm=('GRW', 's_loc', 0.5, 'loc', None))
        c['om'] = (c['om'][0], [(n, cases._g(*v)) for n, v in c['om'][1]], c['om'][2])
        S = cases.build(bl, c)
        with np.errstate(all='ignore'):
            S.fit(silent=True)
            gold = oa.run(c)
        compare.check(dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence, posteriorSequence=S.posteriorSequence,
                           posteriorMeanValues=S.posteriorMeanValues),
                      dict(logEvidence=gold['logEvidence'], localEvidence=gold['localEvidence'], posteriorSequence=np.asarray(gold['posteriorSequence']),
                           posteriorMeanValues=np.asarray(gold['posteriorMeanValues'])), compare.ORACLE_TOL)
    finally:
        bl.set_engine(prev)


def test_compile_emits_a_program_only_for_an_engine_that_takes_one():
    import likprogram_studies as ls
    prev = bl.set_engine(OracleEngine())
    try:
        S = ls.normal_study(bl, sizes=(12, 5), T=6)
        S._formatData()
        problem, _ = S._compile()
        assert problem.obs_model == _abi.OM_TABLE and problem.lik_program is None and problem.lik.shape == (6, 12, 5)

        class Stub(OracleEngine):
            lik_programs = True
        bl.set_engine(Stub())
        problem, _ = S._compile()
        assert problem.obs_model == _abi.OM_PROGRAM and problem.lik is None
        ops, consts, step = problem.lik_program
        assert step.shape == (6, 1, 0) and ops.dtype == np.int32 and ops.shape[1] == 2
        P = ls.poisson_study(bl, n=11, T=7)
        P._formatData()
        problem, _ = P._compile()
        assert problem.obs_model == _abi.OM_PROGRAM and problem.lik is None and problem.lik_program[2].shape == (7, 1, 1)
        import math
        np.testing.assert_array_equal(problem.lik_program[2][:, 0, 0], [float(math.factorial(int(v))) for v in np.asarray(P.formattedData).reshape(-1)])
        stub = bl.get_engine()
        stub.options = {'lik_program': 0.0}               # the option keeps the host table
        problem, _ = P._compile()
        assert problem.obs_model == _abi.OM_TABLE and problem.lik is not None and problem.lik_program is None
    finally:
        bl.set_engine(prev)


def test_host_check_accepts_compiled_programs_and_rejects_broken_ones():
    C, P, D, S_, ADD, SEL = _abi.LP_CONST, _abi.LP_PARAM, _abi.LP_DATA, _abi.LP_STEP, _abi.LP_ADD, _abi.LP_SELECT
    for c in lc.cases():
        p = c.program()
        ops, consts = p.bind(c.marginal)
        assert _check_call(ops, len(consts), p.n_step, len(c.marginal))[0] == 0, c.name
    ok = [(D, 0), (P, 0), (ADD, 0)]
    assert _check_call(ok, 0, 0, 1)[0] == 0
    bad = {
        'stack underflow': ([(D, 0), (ADD, 0)], 0, 0, 1),
        'underflow of SELECT': ([(D, 0), (D, 0), (SEL, 0)], 0, 0, 1),
        'depth 17': ([(D, 0)] * 17 + [(ADD, 0)] * 16, 0, 0, 1),
        '257 ops': ([(D, 0)] + [(_abi.LP_NEG, 0)] * 256, 0, 0, 1),
        'CONST out of range': ([(C, 2)], 2, 0, 1),
        'negative CONST': ([(C, -1)], 2, 0, 1),
        'STEP out of range': ([(S_, 1)], 0, 1, 1),
        'PARAM out of range': ([(P, 2)], 0, 0, 2),
        'AXIS of a parameter the grid does not have': ([(_abi.LP_AXIS, 1)], 4, 0, 1),
        'AXIS offset out of range': ([(_abi.LP_AXIS, 0 | (4 << 2))], 4, 0, 1),
        'POWI exponent 65': ([(D, 0), (_abi.LP_POWI, 65)], 0, 0, 1),
        'two values left': ([(D, 0), (D, 0)], 0, 0, 1),
        'nothing left': ([], 0, 0, 1),
        'unknown code': ([(D, 0), (22, 0)], 0, 0, 1),
    }
    for what, (ops, nc, ns, nd) in bad.items():
        rc, msg = _check_call(np.array(ops, dtype=np.int32).reshape(-1, 2), nc, ns, nd)
        assert rc != 0 and msg, what
    assert _check_call([(D, 0)] * 16 + [(ADD, 0)] * 15, 0, 0, 1)[0] == 0          # depth 16 is the limit, not beyond it
    assert _check_call([(D, 0)] + [(_abi.LP_NEG, 0)] * 255, 0, 0, 1)[0] == 0      # ... and 256 ops
