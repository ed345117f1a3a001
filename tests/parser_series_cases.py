"""The studies and queries of the vector-t parser tests (tests/test_parser_series_host.py, tests/test_parser_series.py) and of the
generator of their fixture (tests/golden/gen_parser_series_golden.py): every builder takes the package to build with, so the reference
and this package build the same studies."""
import contextlib
import io
import warnings

import numpy as np

import test_parser as tp


def _quiet():
    stack = contextlib.ExitStack()
    stack.enter_context(contextlib.redirect_stdout(io.StringIO()))
    stack.enter_context(np.errstate(all='ignore'))
    stack.enter_context(warnings.catch_warnings())
    warnings.simplefilter('ignore')
    return stack


def coal(b):
    S = b.Study()
    S.loadExampleData()
    S.setOM(b.om.Poisson('accident_rate', b.oint(0, 6, 200)))
    S.setTM(b.tm.GaussianRandomWalk('sigma', 0.2, target='accident_rate'))
    with _quiet():
        S.fit()
    return (S,)


GAUSS_DATA = np.random.RandomState(7).normal(1.0, 0.8, 34) + np.linspace(-0.5, 0.9, 34)


def gauss(b):
    S = b.Study()
    S.loadData(GAUSS_DATA)
    S.setOM(b.om.Gaussian('mean', b.cint(-1, 3, 24), 'std', b.oint(0, 2, 20)))
    S.setTM(b.tm.CombinedTransitionModel(b.tm.GaussianRandomWalk('s1', 0.15, target='mean'), b.tm.GaussianRandomWalk('s2', 0.05, target='std')))
    with _quiet():
        S.fit()
    return (S,)


def two(b):
    with _quiet():
        return tp.two_studies(b)


def hyper(b):
    with _quiet():
        return tp.hyper_studies(b)


def hyper_alone(b):
    """The HyperStudy of tp.hyper_studies on its own: on a GPU engine its average posterior is then still resident when it is queried."""
    H = b.HyperStudy()
    H.loadData(tp.D15)
    H.setOM(b.om.Gaussian('mean', b.cint(0, 6, 12), 'std', b.oint(0.2, 2, 9)))
    H.setTM(b.tm.CombinedTransitionModel(b.tm.GaussianRandomWalk('sigma', b.cint(0, 0.4, 4), target='mean'), b.tm.RegimeSwitch('pmin', [-5, -2])))
    with _quiet():
        H.fit()
    return (H,)


def changepoint_alone(b):
    """The ChangepointStudy of tp.hyper_studies on its own."""
    S = b.ChangepointStudy()
    S.loadData(np.array([1, 1, 2, 1, 4, 5, 4, 5]))
    S.setOM(b.om.Poisson('lam', b.oint(0, 8, 40)))
    S.setTM(b.tm.ChangePoint('tc', 'all'))
    with _quiet():
        S.fit()
    return (S,)


BUILDERS = dict(coal=coal, gauss=gauss, two=two, hyper=hyper, hyper_alone=hyper_alone, changepoint_alone=changepoint_alone)
GAUSS_C = np.round(0.4 + 0.03 * np.arange(len(GAUSS_DATA)) + 0.2 * np.sin(np.arange(len(GAUSS_DATA))), 6)

# name -> (studies, query, series or None, index spaces, the kernel a HipEngine plan takes or None)
CASES = {
    'coal_lt': ('coal', 'accident_rate < 1', None, 1, 'rows'),
    'gauss_ratio': ('gauss', 'mean/std > 1', None, 1, 'rows'),
    'gauss_series': ('gauss', '(mean - c)/std > 1', {'c': GAUSS_C}, 1, 'rows'),
    'gauss_sincos': ('gauss', 'sin(mean) + cos(std) > 1', None, 1, 'rows'),
    'gauss_exp': ('gauss', 'exp(mean/std) > 2', None, 1, 'rows'),
    'gauss_pow': ('gauss', 'std^mean > 1', None, 1, 'rows'),
    'two_product': ('two', 'rate*rate2 >= 4', None, 2, 'pairs'),
    'two_difference': ('two', 'rate - rate2 > 0', None, 2, 'pairs'),
    'hyper_product': ('hyper', 'mean*sigma > 0.5', None, 2, 'pairs'),
    'changepoint': ('hyper', 'tc - lam > 0', None, 2, 'pairs'),
    'online': ('hyper', 'nu*sw < 0.6', None, 2, None),           # an OnlineStudy keeps its history on the host: the loop
}


def textual(query, series, i):
    """The query of step i as the tutorials write it: every series name replaced by repr of its value."""
    import re
    for name, values in (series or {}).items():
        query = re.sub(r'\b%s\b' % name, repr(float(values[i])), query)
    return query
