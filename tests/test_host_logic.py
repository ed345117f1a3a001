"""Host-side logic of bayesloop_amd (grid/prior construction, transition-program compilation, hyper-grid plumbing,
ChangepointStudy masking, evidence algebra) on CPU: the product's study classes run with the oracle-backed TEST DOUBLE
engine (tests/oracle_engine.py) and must reproduce the reference's golden vectors."""
import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import oracle_adapter as oa
from oracle_engine import OracleEngine


@pytest.fixture(autouse=True)
def oracle_engine():
    prev = bl.set_engine(OracleEngine())
    yield
    bl.set_engine(prev)


def result_of(S, case):
    c = cases.CASES[case]
    res = dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence)
    kw = c.get('fit', {})
    if not kw.get('evidenceOnly', False) and np.isfinite(S.logEvidence):
        res['posteriorSequence'] = S.posteriorSequence
        res['posteriorMeanValues'] = S.posteriorMeanValues
    for key in ('logEvidenceList', 'hyperParameterDistribution', 'hyperGridValues', 'flatHyperPriorValues',
                'hyperGridConstant', 'mask'):
        if hasattr(S, key) and getattr(S, key) is not None and len(np.atleast_1d(getattr(S, key))) > 0:
            res[key] = np.asarray(getattr(S, key))
    return res


FAST = [k for k, c in cases.CASES.items() if not c.get('slow')]


@pytest.mark.parametrize('case', FAST)
def test_study_classes_reproduce_reference(case, capsys):
    S = cases.build(bl, case)
    with np.errstate(all='ignore'):
        S.fit(**{k: v for k, v in cases.fit_kwargs(case).items()})
    gold = oa.load_golden(case)
    np.testing.assert_array_equal(S.marginalGrid[0], gold['marginal0'])
    np.testing.assert_allclose(S.latticeConstant, gold['latticeConstant'], rtol=0, atol=0)
    compare.check(result_of(S, case), gold, compare.ORACLE_TOL, case_tol=cases.CASES[case].get('tol'))


def test_reference_test_expectations_through_accessors():
    """tests/test_hyperstudy.py:32-59 of the reference, verbatim expectations, via the accessor methods."""
    S = cases.build(bl, 'kat_hyper_1hp')
    S.fit(silent=True)
    np.testing.assert_allclose(S.getParameterDistributions('mean', density=False)[1][:, 5],
                               [0.017242, 0.014581, 0.012691, 0.011705, 0.011586], rtol=1e-04)
    np.testing.assert_allclose(S.getParameterMeanValues('mean'), [2.92089, 2.952597, 3., 3.047403, 3.07911], rtol=1e-05)
    np.testing.assert_almost_equal(S.logEvidence, -16.0629517262, decimal=5)
    x, p = S.getHyperParameterDistribution('sigma')
    np.testing.assert_allclose(np.array([x, p]), [[0., 0.2], [0.43828499, 0.56171501]], rtol=1e-05)


def test_study_accessors_reference_test_study():
    """tests/test_study.py:32-52 of the reference (default estimated 1000-point grid)."""
    S = cases.build(bl, 'kat_study_1hp')
    S.fit(silent=True)
    np.testing.assert_allclose(S.getParameterDistributions('rate', density=False)[1][:, 250],
                               [0.000417, 0.000386, 0.000356, 0.000336, 0.000332], rtol=1e-02)
    np.testing.assert_allclose(S.getParameterMeanValues('rate'),
                               [3.073534, 3.08179, 3.093091, 3.104016, 3.111173], rtol=1e-02)


def test_configuration_errors():
    S = bl.Study(silent=True)
    with pytest.raises(bl.ConfigurationError):
        S.fit()
    S.loadData(np.array([1, 2, 3]), silent=True)
    with pytest.raises(bl.ConfigurationError):
        S.fit()
    S.setOM(bl.om.Poisson('rate', bl.oint(0, 6, 50)), silent=True)
    with pytest.raises(bl.ConfigurationError):
        S.fit()
    with pytest.raises(bl.ConfigurationError):
        S.set(bl.om.Poisson('a', bl.oint(0, 1, 5)), bl.om.Poisson('b', bl.oint(0, 1, 5)), silent=True)
    with pytest.raises(bl.ConfigurationError):
        bl.tm.GaussianRandomWalk('sigma', 0.1)          # no target
    with pytest.raises(bl.ConfigurationError):
        bl.tm.Deterministic(lambda t, slope: slope * t, target='rate')      # hyper-parameters need default values
    with pytest.raises(bl.ConfigurationError):
        bl.tm.Deterministic(lambda t, slope=1: slope * t)                   # no target
    S.setTM(bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s', 0.1, target='rate'),
                                          bl.tm.GaussianRandomWalk('s', 0.2, target='rate')), silent=True)
    with pytest.raises(bl.ConfigurationError):
        S.fit(silent=True)                               # duplicate hyper-parameter names


def test_table_likelihood_path_matches_native_models():
    """A user-defined observation model (plug-in pdf) goes through the likelihood-table path."""
    class MyPoisson(bl.om.ObservationModel):
        def __init__(self, name, value):
            self.name = 'my poisson'
            self.segmentLength = 1
            self.multiplyLikelihoods = True
            self.parameterNames = [name]
            self.parameterValues = [value]
            self.prior = lambda x: np.sqrt(1. / x)

        def pdf(self, grid, dataSegment):
            import math
            return (grid[0] ** dataSegment[0]) * np.exp(-grid[0]) / math.factorial(int(dataSegment[0]))

    S = bl.Study(silent=True)
    S.loadData(cases.D15, silent=True)
    S.set(MyPoisson('rate', bl.oint(0, 6, 100)), bl.tm.GaussianRandomWalk('sigma', 0.2, target='rate'), silent=True)
    S.fit(silent=True)
    np.testing.assert_allclose(S.logEvidence, -10.323144246611964, rtol=1e-13)


def test_pickle_roundtrip_materialises_posterior():
    import pickle
    S = cases.build(bl, 'kat_grw')
    S.fit(silent=True)
    S2 = pickle.loads(pickle.dumps(S))
    np.testing.assert_array_equal(S2.posteriorSequence, S.posteriorSequence)
    assert S2.logEvidence == S.logEvidence


def test_device_side_reductions_equal_host_reductions():
    """getParameterDistributions / getParameterDistribution use the engine's reductions while the posterior is still on
    the device; they must equal reductions of the materialised array."""
    for case in ('c3_small', 'c4_2hp'):
        S = cases.build(bl, case)
        S.fit(silent=True)
        assert S._posterior_pending is not None
        x, m0 = S.getParameterDistributions('mean', density=False)
        x1, m1 = S.getParameterDistributions('std')
        xa, avg = S.getParameterDistribution('avg', 'mean')
        xt, pt = S.getParameterDistribution(S.formattedTimestamps[3], 'std', density=False)
        assert S._posterior_pending is not None           # nothing was materialised
        post = S.posteriorSequence
        np.testing.assert_allclose(m0, post.sum(axis=2), rtol=1e-13)
        np.testing.assert_allclose(m1, post.sum(axis=1) / S.latticeConstant[1], rtol=1e-13)
        np.testing.assert_allclose(avg, post.mean(axis=0).sum(axis=1) / S.latticeConstant[0], rtol=1e-13)
        np.testing.assert_allclose(pt, post[3].sum(axis=0), rtol=1e-13)


def test_simulate_matches_reference_golden_host_side():
    """Study.simulate (core.py:566-597) over the test double (row / time-average reads of the posterior handle)."""
    gold = oa.load_golden('simulate')
    for case in ('c1_coal', 'kat_gaussian'):
        S = cases.build(bl, case)
        with np.errstate(all='ignore'):
            S.fit(**cases.fit_kwargs(case))
        x = gold[case + '_x']
        np.testing.assert_allclose(S.simulate(x), gold[case + '_avg'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(S.simulate(x, t=float(gold[case + '_t'])), gold[case + '_at'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(S.simulate(x, density=True), gold[case + '_avg_density'], rtol=1e-9, atol=1e-300)
    S = bl.Study(silent=True)
    S.loadData(np.array([1, 0, 1, 0, 0]), silent=True)
    S.set(bl.om.AR1('rho', bl.oint(-1, 1, 20), 'sigma', bl.oint(0, 1, 20)), bl.tm.Static(), silent=True)
    with pytest.raises(NotImplementedError):
        S.simulate([0.])


def test_scipy_sympy_numpy_observation_models_reference_kats():
    """bl.om.SymPy / SciPy / NumPy (reference tests/test_observationmodels.py:11-120): plug-in likelihoods through the
    table path; the reference's own log-evidence values, same tolerance (decimal=5)."""
    scipy_stats = pytest.importorskip('scipy.stats')
    sympy_stats = pytest.importorskip('sympy.stats')
    from sympy import Symbol

    def logE(L, data=np.array([1, 2, 3, 4, 5])):
        S = bl.Study(silent=True)
        S.loadData(data, silent=True)
        S.setOM(L, silent=True)
        S.setTM(bl.tm.Static(), silent=True)
        S.fit(silent=True)
        return S.logEvidence

    rate = Symbol('rate', positive=True)
    np.testing.assert_almost_equal(logE(bl.om.SymPy(sympy_stats.Poisson('poisson', rate), 'rate', bl.oint(0, 7, 100))),
                                   -10.238278174965238, decimal=5)
    mu, std = Symbol('mu'), Symbol('std', positive=True)
    np.testing.assert_almost_equal(logE(bl.om.SymPy(sympy_stats.Normal('norm', mu, std), 'mu', bl.cint(0, 7, 200), 'std',
                                                    bl.oint(0, 1, 200), prior=lambda x, y: 1.)), -13.663836264357226, decimal=5)
    np.testing.assert_almost_equal(logE(bl.om.SciPy(scipy_stats.poisson, 'mu', bl.oint(0, 7, 100), fixedParameters={'loc': 0})),
                                   -10.238278174965238, decimal=5)
    np.testing.assert_almost_equal(logE(bl.om.SciPy(scipy_stats.norm, 'loc', bl.cint(0, 7, 200), 'scale', bl.oint(0, 1, 200))),
                                   -13.663836264357225, decimal=5)

    def likelihood(data, mu):
        x, s = data
        return np.exp((x - mu) ** 2. / (2 * s ** 2.)) / np.sqrt(2 * np.pi * s ** 2.)
    np.testing.assert_almost_equal(logE(bl.om.NumPy(likelihood, 'mu', bl.oint(0, 7, 100)),
                                        np.array([[1, 0.5], [2, 0.5], [3, 0.5], [4, 1.], [5, 1.]])), 148.92056578058387, decimal=5)
    # the symbolic Jeffreys prior the reference intends (1/sqrt(rate) for a Poisson rate)
    from bayesloop_amd.observationModels import jeffreys_prior_of
    expr, f = jeffreys_prior_of(sympy_stats.Poisson('poisson', rate))
    assert str(expr) == '1/sqrt(rate)' and abs(f(4.0) - 0.5) < 1e-15
    with pytest.raises(bl.ConfigurationError):
        bl.om.SciPy(np.random, 'mu', bl.oint(0, 7, 100))
    with pytest.raises(bl.ConfigurationError):
        bl.om.SciPy(scipy_stats.norm, 'wrong', bl.oint(0, 7, 100))


def test_save_load_roundtrip(tmp_path):
    """bl.save / bl.load (reference fileIO.py:10-37, tests/test_fileio.py): a fitted study with a lambda prior survives."""
    S = bl.HyperStudy(silent=True)
    S.loadData(np.array([1, 2, 3, 4, 5]), silent=True)
    S.setOM(bl.om.Gaussian('mean', bl.cint(0, 6, 20), 'sigma', bl.oint(0, 2, 20), prior=lambda m, s: 1 / s ** 3), silent=True)
    S.setTM(bl.tm.GaussianRandomWalk('s', [0.1, 0.3], target='mean'), silent=True)
    S.fit(silent=True)
    path = str(tmp_path / 'study.bl')
    bl.save(path, S)
    R = bl.load(path)
    assert R.logEvidence == S.logEvidence
    np.testing.assert_array_equal(R.posteriorSequence, S.posteriorSequence)
    np.testing.assert_array_equal(R.hyperParameterDistribution, S.hyperParameterDistribution)
    assert R.observationModel.prior(1.0, 2.0) == 1 / 8.
    R.fit(silent=True)                     # the loaded study can be fitted again
    assert abs(R.logEvidence - S.logEvidence) < 1e-12


def test_jeffreys_helpers():
    """bl.getJeffreysPrior / bl.computeJeffreysPriorAR1 (reference bayesloop/jeffreys.py): the closed form of Uhlig's prior."""
    sympy_stats = pytest.importorskip('sympy.stats')
    from sympy import Symbol
    expr, f = bl.getJeffreysPrior(sympy_stats.Poisson('p', Symbol('rate', positive=True)))
    assert str(expr) == '1/sqrt(rate)' and abs(f(4.0) - 0.5) < 1e-15
    data = np.array([0.3, -0.2, 0.5, 0.1, -0.4])
    for om, scaled in ((bl.om.AR1, False), (bl.om.ScaledAR1, True)):
        S = bl.Study(silent=True)
        S.loadData(data, silent=True)
        S.setOM(om('rho', bl.oint(-1, 1, 30), 'sigma', bl.oint(0, 2, 25)), silent=True)
        p = bl.computeJeffreysPriorAR1(S, t=2)
        r, s = S.grid
        if scaled:
            s = s * np.sqrt(1 - r ** 2)
        want = np.exp(-data[1] ** 2 * (1 - r ** 2) / (2 * s ** 2)) / s ** 2 * np.sqrt(4 * r ** 2 / (1 - r ** 2) + 2 * (len(data) + 1))
        np.testing.assert_allclose(p, want / want.sum(), rtol=1e-13)
        assert abs(p.sum() - 1) < 1e-12
    S = bl.Study(silent=True)
    S.loadData(data, silent=True)
    S.setOM(bl.om.Poisson('rate', bl.oint(0, 6, 20)), silent=True)
    with pytest.raises(bl.ConfigurationError):
        bl.computeJeffreysPriorAR1(S)


def test_accessors_accept_keyword_arguments():
    """The reference's accessors take their arguments by keyword as well (core.py:864-1002, 1535-1694); the plot decorator must
    not swallow them (every call below used to raise TypeError: missing positional argument)."""
    S = cases.build(bl, 'kat_hyper_1hp')
    S.fit(silent=True)
    x0, p0 = S.getParameterDistribution(S.formattedTimestamps[2], 'mean')
    x1, p1 = S.getParameterDistribution(t=S.formattedTimestamps[2], name='mean')
    x2, p2 = S.getParameterDistribution(S.formattedTimestamps[2], name='mean', density=False)
    np.testing.assert_array_equal(p0, p1)
    np.testing.assert_allclose(p2, p0 * S.latticeConstant[0], rtol=1e-13)
    np.testing.assert_array_equal(S.getParameterDistributions(name='mean')[1], S.getParameterDistributions('mean')[1])
    np.testing.assert_array_equal(S.getPDs(name='mean', density=False)[1], S.getParameterDistributions('mean', density=False)[1])
    np.testing.assert_array_equal(S.getHyperParameterDistribution(name='sigma')[1], S.getHyperParameterDistribution('sigma')[1])
    np.testing.assert_array_equal(S.getHPD(name='sigma')[1], S.getHPD('sigma')[1])
    S2 = cases.build(bl, 'c4_2hp')
    S2.fit(silent=True)
    names = list(S2.flatHyperParameterNames[:2])
    a = S2.getJointHyperParameterDistribution(names)
    b = S2.getJointHyperParameterDistribution(names=names)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    C = cases.build(bl, 'kat_changepointstudy')
    C.fit(silent=True)
    cp = [n for n in C.flatHyperParameterNames]
    if len(cp) >= 2:
        np.testing.assert_array_equal(C.getDurationDistribution(names=cp[:2])[1], C.getDurationDistribution(cp[:2])[1])


def test_evidence_only_refit_keeps_the_previous_posterior():
    """Study.fit(evidenceOnly=True) after a full fit: the reference keeps the previous posteriorSequence (core.py:355-356)."""
    S = cases.build(bl, 'c1_coal')
    S.fit(silent=True)
    logE = S.logEvidence
    S.fit(evidenceOnly=True, silent=True)
    assert S.logEvidence == logE
    gold = oa.load_golden('c1_coal')
    np.testing.assert_allclose(S.posteriorSequence, gold['posteriorSequence'], rtol=1e-9, atol=1e-15)
    x, p = S.getParameterDistribution(1900, 'rate')
    assert np.isfinite(p).all()


def test_online_study_survives_pickling():
    """A pickled / copied OnlineStudy carries its per-chain filter states along and continues stepping independently of the
    original (reference fileIO.py:10-37)."""
    import pickle
    data = np.array([1.0, 2.0, 3.0, 2.0, 4.0, 3.0])

    def make():
        O = bl.OnlineStudy(storeHistory=True, silent=True)
        O.set(bl.om.Poisson('rate', bl.oint(0, 6, 50)), silent=True)
        O.add('static', bl.tm.Static())
        O.add('grw', bl.tm.GaussianRandomWalk('sigma', [0.1, 0.3], target='rate'))
        return O
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        A = make()
        for x in data[:3]:
            A.step(x)
        B = pickle.loads(pickle.dumps(A))
        for x in data[3:]:
            B.step(x)             # the copy goes on ...
        for x in data[3:]:
            A.step(x)             # ... and so does the original, from its own state
        R = make()
        for x in data:
            R.step(x)
    for O in (A, B):
        np.testing.assert_allclose(O.logEvidence, R.logEvidence, rtol=1e-12)
        np.testing.assert_allclose(O.marginalizedPosterior, R.marginalizedPosterior, rtol=1e-12)
        np.testing.assert_allclose(O.transitionModelDistribution, R.transitionModelDistribution, rtol=1e-12)
    del B
    with contextlib.redirect_stdout(io.StringIO()):
        A.step(2.0)               # releasing the copy's slots must not touch the original's
    assert np.isfinite(A.logEvidence)


# ---- the scale algebra of the resident kernels (include/blhip.h: blhip_host_unlag) -- pure host code of libblhip.so ---------------------

from scale_rules import simulate_sums as _simulate_sums      # (tests/highprec.py forms its bounds from the same restatement)


@pytest.mark.parametrize('scheme,lag', [(0, 1), (0, 2), (1, 2), (1, 3), (1, 4)])
def test_host_recovers_the_normalisers_from_lagged_sums(scheme, lag):
    import ctypes
    from bayesloop_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(100 * scheme + lag)
    T = 400
    norms = np.exp(rng.normal(-3.0, 1.5, T))                    # what core.py:385 would see
    S, s = _simulate_sums(norms, lag, scheme)
    sums, scales = S.copy(), np.zeros(T)
    assert lib.blhip_host_unlag(scheme, _abi.dptr(sums), T, lag, None, _abi.dptr(scales)) == 0
    np.testing.assert_allclose(sums, norms, rtol=1e-12)
    np.testing.assert_allclose(scales, s, rtol=1e-12)


def test_scale_from_the_lagged_normaliser_stays_bounded_where_the_lagged_sum_diverges():
    """Dividing by the SUM of step k - lag is a feedback loop x_k = x_(k-1) - x_(k-lag) + nu in the log domain: bounded (period 6) for
    lag 2, exponentially unstable for lag 3 (|roots of r^3 - r^2 + 1| = 1.15).  Dividing by the NORMALISER of step k - lag leaves
    the product of the last `lag` normalisers in the state, whatever the lag (blhip_chainres.hpp)."""
    rng = np.random.default_rng(7)
    T = 400
    norms = np.exp(rng.normal(-2.0, 0.3, T))
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        S_sum3, _ = _simulate_sums(norms, 3, 0)
    assert not np.all(np.isfinite(S_sum3)) or np.nanmax(np.abs(np.log(S_sum3[np.isfinite(S_sum3) & (S_sum3 > 0)]))) > 300.0
    S_sum2, _ = _simulate_sums(norms, 2, 0)
    assert np.max(np.abs(np.log(S_sum2))) < 40.0
    for lag in (2, 3, 4):
        S, _ = _simulate_sums(norms, lag, 1)
        want = np.array([np.prod(norms[max(0, k - lag + 1):k + 1]) for k in range(T)])
        np.testing.assert_allclose(S, want, rtol=1e-10)


def test_host_unlag_with_restarts_and_out_of_range_sums():
    import ctypes
    from bayesloop_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(11)
    T, lag = 60, 4
    norms = np.exp(rng.normal(-3.0, 1.0, T))
    kinds = np.zeros(T, dtype=np.uint8)
    kinds[[17, 18, 40]] = 2                                     # blk::SRC_RESET: change points (transitionModels.py:300-312)
    S, s = _simulate_sums(norms, lag, 1, kinds)
    sums = S.copy()
    assert lib.blhip_host_unlag(1, _abi.dptr(sums), T, lag, kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), None) == 0
    np.testing.assert_allclose(sums, norms, rtol=1e-12)
    bad = S.copy()
    bad[30] = 1e-200                                            # a run of extreme outliers: the fit falls back to the launch-per-step kernels
    assert lib.blhip_host_unlag(1, _abi.dptr(bad), T, lag, None, None) == 1


def _long_schedules():
    import long_series_cases as ls
    return list(ls.SCHEDULES)


@pytest.mark.parametrize('schedule', _long_schedules())
def test_host_unlag_at_the_long_series_schedules(schedule):
    """the host's inverse against the restated rules at the normaliser schedules of tests/long_series_cases.py, not only at random ones: the
    lagged sum (scheme 0), the lagged normaliser (1) and the same with clamped steps at the exact scale (2: bit 6 of a step's kind), each with
    and without a restart history (change points behind steps 5 and 9).  Where a simulated sum leaves (1e-150, 1e150) the host must say so."""
    import ctypes
    import long_series_cases as ls
    from bayesloop_amd import _abi
    lib = _abi.load()
    norms = np.exp2(ls.exponents(schedule).astype(np.float64)) * np.random.default_rng(23).uniform(0.9, 1.1, ls.steps_of(schedule))
    T = len(norms)
    restarts, clamped = np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.uint8)
    restarts[[6, 10]] = 2                                        # blk::SRC_RESET
    clamped[[3, 7, 8, 12]] = 1
    seen = set()
    for scheme, lags in ((0, (1, 2, 3)), (1, (2, 3, 4)), (2, (2, 3, 4))):
        for lag in lags:
            for kinds in ((None,) if scheme == 0 else (None, restarts)):
                with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
                    S, s = _simulate_sums(norms, lag, scheme, kinds, clamped if scheme == 2 else None)
                packed = None
                if scheme == 2:
                    packed = ((np.zeros(T, dtype=np.uint8) if kinds is None else kinds) | (clamped << 6)).astype(np.uint8)
                elif kinds is not None:
                    packed = kinds
                ptr = None if packed is None else packed.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))
                ok = True
                for x in S:                                     # (the host stops at the first sum out of range; the ones behind it may be anything)
                    if not 1e-150 < x < 1e150:
                        ok = False
                        break
                sums, scales = S.copy(), np.zeros(T)
                rc = lib.blhip_host_unlag(scheme, _abi.dptr(sums), T, lag, ptr, _abi.dptr(scales))
                assert rc == (0 if ok else 1), (schedule, scheme, lag, kinds is not None, S)
                seen.add(ok)
                if ok:
                    np.testing.assert_allclose(sums, norms, rtol=1e-12)
                    np.testing.assert_allclose(scales, s, rtol=1e-12)
    assert True in seen and (False in seen) == (schedule not in ('flat', 'burst_mild')), (schedule, seen)      # both answers of the host are walked, but on the two mild schedules


@pytest.mark.parametrize('schedule', _long_schedules())
def test_a_changed_scale_rule_moves_the_normalisers_beyond_any_bound(schedule):
    """Can tests/test_long_series.py fail?  Two of the arithmetic changes a kernel could carry, RESTATED on the sums (no kernel is changed or
    run): what the host's inverse then makes of them, against the 1e-12 the bounds of logEvidence and local_evidence leave a normaliser.
      (a) the chain-resident scale without S_(k-lag-1):  s_k = s_(k-lag) / S_(k-lag).  Invisible in three steps (k < lag), wrong from step lag + 1;
      (b) a K-steps-per-launch pass whose later launches start at scale 1 instead of 1 / S of the step before."""
    import long_series_cases as ls
    from bayesloop_amd import _abi
    lib = _abi.load()
    norms = np.exp2(ls.exponents(schedule).astype(np.float64)) * np.random.default_rng(23).uniform(0.9, 1.1, ls.steps_of(schedule))
    T, lag = len(norms), 4
    S, s = np.zeros(T), np.ones(T)
    with np.errstate(all='ignore'):
        for k in range(T):                                          # (a)
            if k >= lag:
                s[k] = s[k - lag] / S[k - lag]
            S[k] = (S[k - 1] if k else 1.0) * s[k] * norms[k]
    if np.all((S > 1e-150) & (S < 1e150)):
        sums = S.copy()
        assert lib.blhip_host_unlag(1, _abi.dptr(sums), T, lag, None, None) == 0
        err = np.abs(sums / norms - 1.0)
        assert np.all(err[:lag + 1] < 1e-12) and np.all(err[lag + 1:] > 1e-3), (schedule, err)
        assert np.all(np.abs(sums[:3] / norms[:3] - 1.0) < 1e-12)       # three steps: nothing to see
    K = 6                                                           # (b): forward_bookkeeping divides an inner step by the raw sum before it
    raw = np.array([np.prod(norms[k - k % K:k + 1]) for k in range(T)])
    wrong = raw.copy()
    wrong[K:] = [raw[k] * raw[K * (k // K) - 1] for k in range(K, T)]      # the launch went on from the un-normalised state
    with np.errstate(all='ignore'):
        got = np.array([wrong[k] if k % K == 0 else wrong[k] / wrong[k - 1] for k in range(T)])
        err = np.abs(got / norms - 1.0)
    assert np.all(err[:K] < 1e-12) and np.all(~(err[K::K] <= 1e-3)), (schedule, err)


# ---- which Gaussian fits take the likelihood recurrence (include/blhip.h: blhip_host_rec_envelope) -- pure host code of libblhip.so ------

def _rec_envelope(mean, std, recs):
    """(accepted, bound) as the library decides it for a two-parameter Gaussian problem with these grids and records (T, d)"""
    import ctypes
    from bayesloop_amd import _abi
    grids = [np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(std, dtype=np.float64)]
    recs = np.ascontiguousarray(recs, dtype=np.float64)
    cp = _abi.Problem()                                   # (what the decision reads of a problem: grids and data; no device, no context)
    cp.ndim, cp.obs_model, cp.T, cp.seg_len, cp.data_dim = 2, _abi.OM_GAUSSIAN, len(recs), 1, recs.shape[1]
    for k in range(2):
        cp.n[k] = len(grids[k])
        cp.marginal[k] = _abi.dptr(grids[k])
    cp.data = _abi.dptr(recs)
    out = ctypes.c_double()
    rc = _abi.load().blhip_host_rec_envelope(ctypes.byref(cp), ctypes.byref(out))
    return rc, out.value


def test_recurrence_envelope_of_the_issue_cases():
    """x = -100 against a std column of 1e-3 on linspace(-8, 8, 128) (anchor exponent -2.02e9: two int additions from wrapping) and
    s = 2e-4 with a datum at the grid's edge (the clamp of exp_mn bites) are refused; the benchmark-like grids are accepted"""
    mean = np.linspace(-8, 8, 128)
    wide = np.linspace(0, 4, 18)[1:-1]
    assert _rec_envelope(mean, wide, [[0.3], [-1.2]])[0] == 1
    assert _rec_envelope(mean, np.append(wide, 1e-3), [[-100.0]])[0] == 0
    assert _rec_envelope(mean, np.append(wide, 2e-4), [[8.0]])[0] == 0
    assert _rec_envelope(mean, wide, [[float('nan')], [0.5]])[0] == 1            # NaN values count for nothing
    assert _rec_envelope(mean, wide, [[float('nan')]])[0] == 1
    assert _rec_envelope(mean, np.append(wide, 0.0), [[0.5]])[0] == 0             # a zero std: no envelope
    # the bound covers what the kernels can form: anchor argument + 32 first differences + 512 second differences over 4 rows, on the
    # lattice continued 256 rows beyond either end -- each below exp_mn's clamp, their exponents' sum inside int
    rc, bound = _rec_envelope(mean, [0.05], [[8.0, -8.0]])
    step, cA = 16.0 / 127, 1.0 / (2 * 0.05 ** 2)
    far = 8.0 + 256 * step + 8.0
    assert bound >= 2 * far ** 2 * cA + 32 * (2 * cA * 4 * step * 2 * far) + 512 * (2 * cA * 2 * (4 * step) ** 2) and rc == 1
    assert bound * 1.4426950408889634 < 2.0 ** 31 - 1 and bound <= 1.4e9


def test_recurrence_envelope_matches_its_restatement():
    """tests/likelihood_cases.py restates the decision for the census expectations of tests/test_likelihood_kernels.py: the same bound to
    rounding and the same verdict on every grid and record of that file"""
    import likelihood_cases as lc
    n_ref = 0
    for n0, n1 in ((140, 90), (128, 64), (32, 32), (48, 40), (128, 16), (100, 20), (100, 90), (24, 20)):
        for case in lc.CASES:
            mean, std, recs = lc.mean_grid(n0), lc.std_of(case, n1, n0), lc.records(case, n0)
            for rows in ([0], [1], [2], [0, 1], [0, 1, 2]):
                rc, bound = _rec_envelope(mean, std, recs[rows])
                want = lc.envelope_bound(mean, std, recs[rows])
                assert abs(bound - want) <= 1e-12 * want, (n0, n1, case, rows, bound, want)
                assert rc == (1 if lc.recurrence_accepted(mean, std, recs[rows]) else 0)
                n_ref += rc == 0
    assert n_ref > 100                                                            # (both verdicts occur)
    # the case just inside the envelope is admitted with its three records and sits within 2 % of the edge
    for n0, n1 in ((140, 90), (32, 32), (128, 16)):
        rc, bound = _rec_envelope(lc.mean_grid(n0), lc.std_of('envelope_edge', n1, n0), lc.records('envelope_edge', n0))
        assert rc == 1 and 0.97e9 < bound <= 1e9, (n0, n1, bound)


# ---- observation models with three parameters: the Python surface (grid, program, accessors) through the test double -------------------

def test_three_parameter_models_host_logic():
    pytest.importorskip('scipy.stats')
    om = ('SciPy:t', [('df', ('cint', 2.0, 9.0, 5)), ('loc', ('cint', -3.0, 3.0, 12)), ('scale', ('oint', 0.2, 2.5, 10))], 'default')
    c = dict(study='Study', data=('series', 82, 8), om=om,
             tm=('Combined', [('GRW', 's_loc', 0.6, 'loc', None), ('GRW', 's_scale', 0.25, 'scale', None)]))
    S = cases.build(bl, c)
    S.fit(silent=True)
    with np.errstate(all='ignore'):
        want = oa.run(c)
    assert list(S.gridSize) == [5, 12, 10] and len(S.grid) == 3 and S.grid[0].shape == (5, 12, 10)
    assert abs(S.logEvidence - want['logEvidence']) <= 1e-12 * abs(want['logEvidence'])
    np.testing.assert_allclose(np.asarray(S.posteriorSequence), want['posteriorSequence'], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(S.posteriorMeanValues, want['posteriorMeanValues'], rtol=1e-12)
    for k, name in enumerate(S.observationModel.parameterNames):           # marginals of every parameter (core.py:915, 979-980)
        axes = tuple(a + 1 for a in range(3) if a != k)
        np.testing.assert_allclose(S.getParameterDistributions(name, density=False)[1], want['posteriorSequence'].sum(axis=axes), rtol=1e-12)
    x, p = S.getParameterDistribution(3, 'loc', density=False)
    np.testing.assert_allclose(p, want['posteriorSequence'][3].sum(axis=(0, 2)), rtol=1e-12)

    h = dict(study='HyperStudy', data=('series', 89, 7), om=om, tm=('GRW', 's_loc', ('cint', 0, 1.2, 5), 'loc', None))
    H = cases.build(bl, h)
    H.fit(silent=True)
    with np.errstate(all='ignore'):
        wh = oa.run(h)
    assert abs(H.logEvidence - wh['logEvidence']) <= 1e-12 * abs(wh['logEvidence'])
    np.testing.assert_allclose(H.hyperParameterDistribution, wh['hyperParameterDistribution'], rtol=1e-10)
    np.testing.assert_allclose(H.posteriorMeanValues, wh['posteriorMeanValues'], rtol=1e-10)

    # transition models the N-D path does not run are refused BEFORE any device work (as every configuration problem)
    bad = dict(study='Study', data=('series', 82, 6), om=om, tm=('RS', 'log10pMin', -4, None))
    B = cases.build(bl, bad)
    with pytest.raises(bl.exceptions.ConfigurationError):
        B.fit(silent=True)


def test_deterministic_shifts_of_many_parameter_sets_equal_the_per_set_evaluation():
    """Deterministic.shifts_many (one broadcast call of the user's function over parameter sets x time stamps: what a hyper-study over
    break-points evaluates per unique (parameters, offset) pair) returns exactly what shifts() returns per set -- for a function that
    broadcasts, and, through the fall-back, for one written for scalars only (reference transitionModels.py:573-577, :592-596, :770-776)."""
    import numpy as np
    import bayesloop_amd as bl
    rng = np.random.default_rng(5)
    ts = np.arange(1851., 1892.)

    def linear(t, slope=0.0):
        return slope * t

    def scalar_only(t, slope=0.0, level=0.0):
        if np.ndim(t) != 0 or np.ndim(slope) != 0:          # (a function that refuses arrays)
            raise TypeError('scalars only')
        return level + slope * max(t, 0.0)

    for fn, names in ((linear, ['slope']), (scalar_only, ['slope', 'level'])):
        m = bl.tm.Deterministic(fn, target='rate')
        rows = rng.uniform(-2, 2, size=(7, len(names)))
        offs = rng.integers(1855, 1880, 7).astype(float)
        for t_offsets in (None, offs):
            many = m.shifts_many(names, rows, ts, -1.0, t_offsets=t_offsets)
            assert many.shape == (7, 2 * len(ts))
            for u in range(7):
                one = m.shifts(dict(zip(names, rows[u])), ts, -1.0, t_offset=None if t_offsets is None else t_offsets[u])
                assert np.array_equal(many[u], one, equal_nan=True)


def test_deterministic_function_that_takes_arrays_but_is_not_elementwise():
    """Advisor finding (round 4): a user function that accepts an array of time stamps need not be elementwise (here it subtracts the
    FIRST stamp it is handed).  The reference calls it per scalar (transitionModels.py:573-577): the vectorised evaluation is cross-checked
    against scalar calls and falls back to them."""
    def f(t, slope=0.0):
        t = np.asarray(t, dtype=float)
        return slope * (t - t.ravel()[0]) + slope * t          # array input: depends on the batch; scalar input: slope * t
    m = bl.tm.Deterministic(f, target='rate')
    ts = np.arange(10.)
    got = m.shifts({'slope': 0.5}, ts, -1.0, t_offset=0.0)
    ref = bl.tm.Deterministic(lambda t, slope=0.0: slope * t, target='rate').shifts({'slope': 0.5}, ts, -1.0, t_offset=0.0)
    assert np.array_equal(got, ref)


def test_online_study_refuses_user_defined_transition_models():
    """Advisor finding (round 4): OnlineStudy has no host-transition path; a user-defined model (or a built-in subclass that overrides
    computeForwardPrior) must raise ConfigurationError, not TypeError / silently run the base class's device program."""
    from bayesloop_amd.exceptions import ConfigurationError

    class Mine(bl.tm.TransitionModel):
        hyperParameterNames = []
        hyperParameterValues = []

        def computeForwardPrior(self, posterior, t):
            return posterior

    class Override(bl.tm.GaussianRandomWalk):
        def computeForwardPrior(self, posterior, t):
            return posterior
    import contextlib, io
    for tm in (Mine(), Override('sigma', 0.1, target='rate'), bl.tm.CombinedTransitionModel(bl.tm.Static(), Override('sigma', 0.1, target='rate'))):
        with contextlib.redirect_stdout(io.StringIO()):
            O = bl.OnlineStudy(storeHistory=True, silent=True)
            O.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)), silent=True)
            O.add('m', tm)
            with pytest.raises(ConfigurationError, match='user-defined'):
                O.step(1.0)


# ---- a hyper-study to which no chain contributes (every logEvidence -inf): the reference's average posterior and its means are all NaN
#      (core.py:1375-1382, :1416-1419), the hyper-parameter distribution NaN, the evidence -inf -- on the device path (dist.sharded_hyper_fit)
#      and on the host-transition path (HyperStudy._fitHostTransitionHyper); the accumulator is closed and owned by nobody afterwards

def no_chain_case():
    # a zero normaliser at step 2 in every chain (500 lies ~1000 standard deviations off the grid)
    return dict(study='HyperStudy', data=np.array([0.2, 0.1, 500.0, 0.3, -0.1]),
                om=('Gaussian', [('mean', ('cint', -2, 2, 32)), ('std', ('oint', 0, 0.5, 32))], 'default'),
                tm=('GRW', 'sigma', [0.05, 0.1, 0.2], 'mean', None))


def host_walk(values):
    """A user-defined random walk (plain NumPy / SciPy, reference plug-in interface): HyperStudy.fit takes the host-transition path."""
    import plugin_models
    return plugin_models.make(bl.tm)['LeakyRandomWalk']('sigma', values, 'leak', 0.0, target='mean')


def check_no_chain_result(S, want):
    assert S.logEvidence == want['logEvidence'] == -np.inf
    wp = np.asarray(want['posteriorSequence'])
    assert np.all(np.isnan(wp)) and np.all(np.isnan(want['posteriorMeanValues']))
    for post in (np.asarray(S.posteriorSequence), np.asarray(S.averagePosteriorSequence)):
        assert post.shape == wp.shape and np.all(np.isnan(post))
    means = np.asarray(S.posteriorMeanValues, dtype=float)
    assert means.shape == np.asarray(want['posteriorMeanValues']).shape and np.all(np.isnan(means))
    np.testing.assert_array_equal(np.isnan(S.hyperParameterDistribution), np.isnan(want['hyperParameterDistribution']))
    assert np.all(np.isneginf(S.logEvidenceList)) and np.all(np.isneginf(want['logEvidenceList']))


@pytest.mark.parametrize('host_transition', [False, True])
def test_hyper_study_without_a_contributing_chain(host_transition):
    from bayesloop_amd import transitionModels as tmm
    c = no_chain_case()
    with np.errstate(all='ignore'):
        want = oa.run(c)
    S = cases.build(bl, c)
    if host_transition:
        S.set(host_walk([0.05, 0.1, 0.2]), silent=True)
    assert tmm.needs_host_transition(S.transitionModel) == host_transition
    with np.errstate(all='ignore'):
        S.fit(silent=True)
    check_no_chain_result(S, want)
    assert getattr(bl.get_engine(), '_accum_owner', None) is None


def test_host_transition_hyper_study_closes_the_accumulator_when_a_fit_raises():
    """An exception inside the per-point loop of the host-transition path leaves no accumulator open and owned by the study."""
    eng = bl.get_engine()
    ended = []
    orig_end = eng.accum_end
    eng.accum_end = lambda: (ended.append(1), orig_end())[1]

    walk = host_walk([0.05, 0.1, 0.2])
    forward = walk.computeForwardPrior

    def failing(posterior, t):
        if walk.hyperParameterValues[0] > 0.15:
            raise RuntimeError('user model failed')
        return forward(posterior, t)
    walk.computeForwardPrior = failing

    S = bl.HyperStudy(silent=True)
    S.loadData(cases.series(5, 12), silent=True)
    S.set(bl.om.Gaussian('mean', bl.cint(-4, 4, 24), 'std', bl.oint(0, 3, 16)), walk, silent=True)
    with pytest.raises(RuntimeError, match='user model failed'):
        S.fit(silent=True)
    assert ended == [1]
    assert getattr(eng, '_accum_owner', None) is None


# ---- the host's tap builders (include/blhip.h: blhip_host_taps) against the longdouble restatements of tests/highprec.py, over the parameters
#      tests/test_step_transitions.py uses: the GPU file takes the RESTATED weights, so the library's own are pinned here -------------------------------

def _host_taps(kind, params, n=0):
    import ctypes
    from bayesloop_amd import _abi
    lib = _abi.load()
    p = np.ascontiguousarray(params, dtype=np.float64)
    rad = (ctypes.c_int * 2)()
    count = lib.blhip_host_taps(kind, n, _abi.dptr(p), len(p), None, 0, rad)
    if count < 0:
        return None, None
    out = np.full(count + 1, -7.0)
    assert lib.blhip_host_taps(kind, n, _abi.dptr(p), len(p), _abi.dptr(out), count, rad) == count
    assert out[count] == -7.0                                          # nothing written beyond `cap`
    return out[:count], (rad[0], rad[1])


def _step_parameters():
    """(walk sigmas, shifts, (c, alpha, n), (sigma1, sigma2, rho)) of every chain of tests/step_transition_cases.py"""
    import step_transition_cases as sc
    walks, shifts, stable, dense = set(), set(), set(), set()
    for c in sc.CASES.values():
        for params in c['chains']:
            for m, p in zip(c['models'], params):
                if m[0] == 'walk' and p:
                    walks.add(sc.sigma_of(p))
                elif m[0] == 'shift':
                    shifts.update(abs(d) * s for d in (p if isinstance(p, tuple) else (p,)) for s in (1, -1) if 0 < abs(d) <= 12)
                elif m[0] == 'as':
                    stable.add((p[0], p[1], c['shape'][m[1]]))
                elif m[0] == 'biv':
                    dense.add(p)
    return sorted(walks), sorted(shifts), sorted(stable), sorted(dense)


def test_host_tap_builders_against_the_restatements():
    import highprec as hp
    walks, shifts, stable, dense = _step_parameters()
    assert len(walks) >= 20 and len(shifts) >= 8 and len(stable) == 9 and len(dense) == 3
    worst = {}

    def hold(what, got, want, bound):
        q = hp.worst(got, want, hp.SLACK * bound)
        worst[what] = max(worst.get(what, 0.0), q)
        assert q <= 1.0, (what, q, hp.worst_at(got, want, hp.SLACK * bound))

    for s in walks:
        r, w, e = hp.gaussian_walk_taps(s)
        got, rad = _host_taps(0, [s])
        assert rad == (r, 0) and len(got) == 2 * r + 1, (s, rad)
        hold('walk', got, w, e)
    for d in shifts:
        K, e, _ = hp.small_shift_taps(d)
        got, rad = _host_taps(1, [d])
        assert rad == (hp.shift_stencil_radius(d), 0) and len(got) == len(K), (d, rad)
        hold('shift', got, K, e)
    for c, alpha, n in stable:
        k, e = hp.alphastable_taps(c, alpha, n)
        got, rad = _host_taps(2, [c, alpha], n)
        assert rad == (n - 1, 0) and len(got) == n
        hold('alphastable', got, k, e)
    for s1, s2, rho in dense:
        k, e = hp.bivariate_taps(s1, s2, rho)
        got, rad = _host_taps(3, [s1, s2, rho])
        assert rad == (k.shape[0] // 2, k.shape[1] // 2) and len(got) == k.size
        hold('bivariate', got.reshape(k.shape), k, e)
    print('host tap builders, worst error / bound: ' + ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))


def test_host_taps_rejects_what_no_builder_takes():
    assert _host_taps(0, [0.05])[0].tolist() == [1.0]                  # radius 0: the identity
    for kind, params, n in ((4, [1.0], 0), (-1, [1.0], 0), (0, [1.0, 2.0], 0), (0, [float('nan')], 0), (0, [-1.0], 0), (1, [12.5], 0),
                            (2, [1.0, 1.5], 1), (2, [1.0, 1.5], 16385), (2, [1.0, 0.0], 24), (2, [1.0, 2.5], 24), (2, [-1.0, 1.5], 24), (3, [1.0, 1.0, 1.0], 0), (3, [0.0, 1.0, 0.5], 0)):
        assert _host_taps(kind, params, n)[0] is None, (kind, params, n)


# ---- which Poisson records take the direct route (include/blhip.h: blhip_host_poisson_direct) -- pure host code of libblhip.so -------------

def _poisson_direct(rates, recs):
    """(return code, per-record verdicts) as the library decides them for a Poisson problem with this rate grid and these records (T, d)"""
    import ctypes
    from bayesloop_amd import _abi
    rates = np.ascontiguousarray(rates, dtype=np.float64)
    recs = np.ascontiguousarray(recs, dtype=np.float64)
    cp = _abi.Problem()
    cp.ndim, cp.obs_model, cp.T, cp.seg_len, cp.data_dim = 1, _abi.OM_POISSON, len(recs), 1, recs.shape[1]
    cp.n[0] = len(rates)
    cp.marginal[0] = _abi.dptr(rates)
    cp.data = _abi.dptr(recs)
    out = (ctypes.c_int * len(recs))()
    rc = _abi.load().blhip_host_poisson_direct(ctypes.byref(cp), out)
    return rc, list(out)


def test_poisson_direct_domain_of_the_issue_cases():
    """the coal-mining counts stay on the direct route (bit-identical results); counts of 171 and more, k = 150 on rates up to 300 and any count on
    rates beyond 708 leave it; NaN counts are ignored; each threshold from both sides"""
    nan = float('nan')
    tut = np.linspace(0, 6, 1002)[1:-1]
    assert _poisson_direct(tut, [[0], [6], [nan]]) == (3, [1, 1, 1])
    assert _poisson_direct(tut, [[170], [171], [nan]]) == (2, [1, 0, 1])
    r300 = np.linspace(0, 300, 301)[1:]
    assert _poisson_direct(r300, [[122], [123], [150], [200]]) == (1, [1, 0, 0, 0])        # 122 ln 300 = 695.9, 123 ln 300 = 701.6
    assert _poisson_direct(r300, [[6, 171], [6, nan], [nan, 171]]) == (1, [0, 1, 0])      # the record's largest count decides for all of its values
    assert _poisson_direct([0.5, 708.0], [[0], [1], [107]]) == (2, [1, 1, 0])               # 107 ln 708 = 702.1
    assert _poisson_direct([0.5, 708.5], [[0], [1]]) == (0, [0, 0])                          # exp(-708.5) is subnormal
    assert _poisson_direct([0.0, 1.0], [[170]]) == (1, [1])                                  # rates up to 1: lambda^k cannot overflow
    import ctypes
    from bayesloop_amd import _abi
    assert _abi.load().blhip_host_poisson_direct(None, None) == -1


def test_poisson_direct_domain_matches_its_restatement():
    """tests/observation_cases.py restates the decision for the bounds of tests/test_observation_kernels.py: the same verdict on every grid and
    record of that file, alone and in sequences"""
    import observation_cases as oc
    n_direct = n_log = 0
    for case in oc.POISSON_CASES:
        for n in (300, 600):
            rates, recs = oc.poisson_rates(case, n), oc.poisson_records(case)
            for rows in ([0], [1], [2], [0, 1], [0, 1, 2]):
                rc, verdicts = _poisson_direct(rates, recs[rows])
                want = [1 if oc.direct_domain(rates, recs[k]) else 0 for k in rows]
                assert verdicts == want and rc == sum(want), (case, n, rows, verdicts, want)
                n_direct += sum(want)
                n_log += len(want) - sum(want)
    assert n_direct > 50 and n_log > 50                                             # (both verdicts occur)
