"""The studies of the end-to-end likelihood-program tests (tests/test_likprogram_gpu.py), written against the API bayesloop_amd shares with
the reference so that tests/golden/gen_likprogram_golden.py can build the SAME studies from the reference package."""
import numpy as np


def series(n, seed, kind='real'):
    rng = np.random.RandomState(seed)
    if kind == 'counts':
        return rng.poisson(3.0 + 2.0 * np.sin(np.arange(n) / 9.0)).astype(float)
    if kind == 'positive':
        return 0.3 + rng.gamma(2.0, 0.7, n)
    return 0.5 + 0.8 * np.sin(np.arange(n) / 5.0) + 0.6 * rng.randn(n)


def _sympy_om(bl, which, sizes):
    import sympy
    import sympy.stats as st
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        if which == 'normal':
            mu, sig = sympy.Symbol('mu'), sympy.Symbol('sigma', positive=True)
            return bl.om.SymPy(st.Normal('rv', mu, sig), 'mu', bl.cint(-2, 3, sizes[0]), 'sigma', bl.oint(0.2, 2.5, sizes[1]),
                               determineJeffreysPrior=False)
        if which == 'poisson':
            lam = sympy.Symbol('lamda', positive=True)
            return bl.om.SymPy(st.Poisson('rv', lam), 'lamda', bl.oint(0, 9, sizes[0]), determineJeffreysPrior=False)
        a, s, m = sympy.Symbol('a', positive=True), sympy.Symbol('s', positive=True), sympy.Symbol('m')
        return bl.om.SymPy(st.Frechet('rv', a, s, m), 'a', bl.cint(1, 4, sizes[0]), 's', bl.cint(0.5, 3, sizes[1]), 'm', bl.cint(-1.5, 0.2, sizes[2]),
                           determineJeffreysPrior=False)


def normal_study(bl, sizes=(128, 16), T=14, hyper=False):
    S = bl.HyperStudy() if hyper else bl.Study()
    S.loadData(series(T, 3), silent=True)
    S.setOM(_sympy_om(bl, 'normal', sizes), silent=True)
    S.setTM(bl.tm.GaussianRandomWalk('s', bl.cint(0.05, 0.35, 4) if hyper else 0.15, target='mu'), silent=True)
    return S


def poisson_changepoint_study(bl, n=200, T=24):
    S = bl.ChangepointStudy()
    S.loadData(series(T, 5, 'counts'), silent=True)
    S.setOM(_sympy_om(bl, 'poisson', (n,)), silent=True)
    S.setTM(bl.tm.ChangePoint('tc', 'all'), silent=True)
    return S


def poisson_study(bl, n=61, T=16):
    S = bl.Study()
    S.loadData(series(T, 5, 'counts'), silent=True)
    S.setOM(_sympy_om(bl, 'poisson', (n,)), silent=True)
    S.setTM(bl.tm.GaussianRandomWalk('s', 0.3, target='lamda'), silent=True)
    return S


def frechet_study(bl, sizes=(6, 8, 5), T=10):
    S = bl.Study()
    S.loadData(series(T, 7, 'positive'), silent=True)
    S.setOM(_sympy_om(bl, 'frechet', sizes), silent=True)
    S.setTM(bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('sa', 0.2, target='a'), bl.tm.GaussianRandomWalk('ss', 0.1, target='s')), silent=True)
    return S


def scipy_t_study(bl, sizes=(5, 16, 12), T=10):
    import scipy.stats
    S = bl.Study()
    S.loadData(series(T, 11), silent=True)
    S.setOM(bl.om.SciPy(scipy.stats.t, 'df', bl.cint(2, 8, sizes[0]), 'loc', bl.cint(-2, 3, sizes[1]), 'scale', bl.oint(0.2, 2.5, sizes[2])), silent=True)
    S.setTM(bl.tm.GaussianRandomWalk('s', 0.2, target='loc'), silent=True)
    return S


GOLDEN = {'likprogram_normal2d': lambda bl: normal_study(bl, sizes=(40, 12), T=12),
          'likprogram_poisson1d': poisson_study,
          'likprogram_frechet3d': frechet_study}


def results(S):
    out = dict(logEvidence=np.float64(S.logEvidence), localEvidence=np.asarray(S.localEvidence, dtype=float),
               posteriorMeanValues=np.asarray(S.posteriorMeanValues, dtype=float), posteriorSequence=np.asarray(S.posteriorSequence, dtype=float))
    if hasattr(S, 'logEvidenceList') and len(np.atleast_1d(S.logEvidenceList)):
        out['logEvidenceList'] = np.asarray(S.logEvidenceList, dtype=float)
    return out
