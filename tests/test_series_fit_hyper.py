"""
HyperStudy.fitMany / ChangepointStudy.fitMany on a real MI355X: a hyper-study per data series as ONE device call per batch of series
(blhip_set_series_groups: a group of H chains of the chain-resident 1-D kernel per series over one likelihood table per series, each group
folded into its own average by blk::series_group_fold_kernel).

Every case compares, per series, logEvidence, localEvidence, logEvidenceList, hyperParameterDistribution, the means and the whole average
sequence with the CPU oracle's fit of that series ALONE and with the loop over fit on the same build, both at the project's parity bar
(compare.GPU_TOL), and reads the kernel census: the series table kernel, the chain-resident 1-D kernel and the grouped fold ran, no
per-step kernel did.  The shapes are the smallest that reach each code path.
"""
import math
import pickle
import re

import numpy as np
import pytest

import bayesloop_amd as bl
import compare
from conftest import kernel_census
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

PER_STEP = ('blk::step_kernel', 'step_kernel', 'bl1f::fused1d_kernel', 'bl1p::persist1d_kernel')
SERIES = ('bl1c::series_lik_kernel', 'bl1c::series_table_kernel')
CHAIN = ('bl1c::chain1d_kernel', 'bl1c::chain1d_long_kernel')
FOLD = 'blk::series_group_fold_kernel'
OTHER_FOLDS = ('blk::accumulate_kernel', 'blk::accumulate_small_kernel', 'blk::accumulate2_kernel', 'blk::accumulate_pad_kernel')


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


class Launched:
    """with Launched() as k: ... ; k.count[family] = launches inside, k.names = the instantiations launched"""

    @staticmethod
    def _now():
        return {name: c for c, name in kernel_census()}

    def __enter__(self):
        self.before = self._now()
        self.count, self.names = {}, []
        return self

    def __exit__(self, *exc):
        after = self._now()
        self.names = sorted(k for k in after if after[k] > self.before[k])
        for k in self.names:
            fam = re.sub(r'<.*', '', k)
            self.count[fam] = self.count.get(fam, 0) + after[k] - self.before[k]

    def fast_path(self, table='bl1c::series_lik_kernel', chain='bl1c::chain1d_kernel', calls=1, fold=True):
        """a table per batch, the chain-resident kernel, the grouped fold once per batch that keeps posteriors; no per-step kernel, no
        other fold"""
        assert self.count.get(table, 0) >= calls, self.count
        assert self.count.get(chain, 0) >= calls, self.count
        assert self.count.get(FOLD, 0) == (calls if fold else 0), self.count
        assert not [f for f in self.count if f in PER_STEP + OTHER_FOLDS], self.count
        assert not [f for f in self.count if f in SERIES + CHAIN and f not in (table, chain)], self.count

    def loop(self):
        assert not [f for f in self.count if f in SERIES or f == FOLD], self.count


def result_of(S, kw):
    """what a fit left on a hyper-study, as compare.check takes it"""
    res = dict(logEvidence=S.logEvidence, localEvidence=np.array(S.localEvidence), logEvidenceList=np.array(S.logEvidenceList, dtype=float))
    if S.hyperParameterDistribution is not None:
        res['hyperParameterDistribution'] = np.array(S.hyperParameterDistribution)
    if not kw.get('evidenceOnly') and np.isfinite(S.logEvidence):
        res['posteriorMeanValues'] = np.array(S.posteriorMeanValues)
        res['posteriorSequence'] = np.array(S.posteriorSequence)
    return res


def alone(make, data, stamps=None, oracle=True, **kw):
    """the fit of one series alone: the CPU oracle's, or the same build's (the loop a user writes)"""
    prev = bl.set_engine(OracleEngine()) if oracle else None
    try:
        S = make()
        S.loadData(np.asarray(data), timestamps=stamps, silent=True)
        with np.errstate(all='ignore'):
            S.fit(silent=True, **kw)
        return result_of(S, kw)
    finally:
        if oracle:
            bl.set_engine(prev)


def entry(R, s):
    res = dict(logEvidence=R.logEvidence[s], localEvidence=R.localEvidence[s], logEvidenceList=R.logEvidenceList[s])
    if R.hyperParameterDistribution[s] is not None:
        res['hyperParameterDistribution'] = R.hyperParameterDistribution[s]
    if not R.evidenceOnly and np.isfinite(R.logEvidence[s]):
        res['posteriorMeanValues'] = R.posteriorMeanValues[s]
        res['posteriorSequence'] = R.averagePosteriorSequence(s)
    return res


def at_the_bar(R, golds):
    assert isinstance(R, bl.HyperSeriesFits) and len(R) == len(golds)
    for s, gold in enumerate(golds):
        res = entry(R, s)
        assert ('hyperParameterDistribution' in res) == ('hyperParameterDistribution' in gold)
        if 'hyperParameterDistribution' in gold:
            assert np.shape(res['hyperParameterDistribution']) == np.shape(gold['hyperParameterDistribution'])
        if 'posteriorSequence' in gold:
            assert np.shape(res['posteriorSequence']) == gold['posteriorSequence'].shape
            assert np.shape(res['posteriorMeanValues']) == gold['posteriorMeanValues'].shape
        compare.check(res, gold, compare.GPU_TOL)


_GOLD = {}


def golds_of(key, make, series, stamps=None, oracle=True, **kw):
    """the fits of a case's series alone, computed once"""
    k = (key, oracle, tuple(sorted(kw.items())))
    if k not in _GOLD:
        _GOLD[k] = [alone(make, d, None if stamps is None else stamps[s], oracle=oracle, **kw) for s, d in enumerate(series)]
    return _GOLD[k]


def both_bars(R, key, make, series, stamps=None, **kw):
    """the oracle's fit of every series alone, and the loop on the same build"""
    at_the_bar(R, golds_of(key, make, series, stamps, True, **kw))
    at_the_bar(R, golds_of(key, make, series, stamps, False, **kw))


def counts(seed, lengths, rate=2.0):
    rng = np.random.RandomState(seed)
    return [rng.poisson(rate + s, size=k).astype(float) for s, k in enumerate(lengths)]       # (series differ: a wrong row offset shows)


def walk(n, sigmas, cls=None):
    def make():
        S = (cls or bl.HyperStudy)(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, n)), bl.tm.GaussianRandomWalk('sigma', sigmas, target='rate'), silent=True)
        return S
    return make


MODES = [{}, dict(forwardOnly=True), dict(evidenceOnly=True)]
MODE_IDS = ['full', 'forwardOnly', 'evidenceOnly']


# ---- the shapes of the fold and of the chain kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('n, S, sigmas, T', [
    (37, 5, [0.1, 0.2, 0.4], 6),                     # an odd row (8-byte loads), fewer chains than sub-groups
    (64, 3, bl.cint(0, 1, 7), 8),                    # an even row (16-byte loads), uneven sub-groups: 2 + 2 + 2 + 1; sigma = 0, the identity
    (64, 3, bl.cint(0, 1, 20), 8),                   # ... even sub-groups: 5 each
    (600, 2, [0.02, 0.04, 0.06, 0.08, 0.1], 4),      # more cells than the chain kernel's block: two cells per thread; 5 cell tiles of the fold
], ids=['n37-H3', 'n64-H7', 'n64-H20', 'n600-H5'])
def test_poisson_walk(n, S, sigmas, T, kw):
    make, series = walk(n, sigmas), counts(n + len(sigmas), [T] * S)
    St = make()
    St.loadData(series[0], silent=True)
    before = [np.array(v) for v in St._unpackAllHyperParameters()]
    with Launched() as k:
        R = St.fitMany(series, silent=True, **kw)
    k.fast_path(fold=not kw.get('evidenceOnly'))
    assert R.lastTiming['fwd_kernel_variant'] == 9
    if not kw.get('evidenceOnly'):
        assert any(FOLD + ('<true>' if n % 2 == 0 else '<false>') in nm for nm in k.names), k.names
    both_bars(R, ('walk', n, len(sigmas)), make, series, **kw)
    # the study is left as it was
    assert np.array_equal(St.rawData, series[0]) and St.hyperParameterDistribution is None and St.logEvidenceList == []
    assert all(np.array_equal(a, b) for a, b in zip(before, St._unpackAllHyperParameters()))
    values, dist = R.getHyperParameterDistribution(S - 1, 'sigma')
    assert np.array_equal(values, sigmas) and np.allclose(dist, R.hyperParameterDistribution[S - 1] * R.study(S - 1).hyperGridConstant[0], rtol=1e-15)


# ---- two hyper-parameters ------------------------------------------------------------------------------------------------------------------
def two_hyper():
    S = bl.HyperStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 50)),
          bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('sigma', [0.1, 0.2, 0.4], target='rate'), bl.tm.RegimeSwitch('log10pMin', [-7, -3])),
          silent=True)
    return S


def test_two_hyper_parameters():
    series = counts(50, [7] * 4)
    with Launched() as k:
        R = two_hyper().fitMany(series, silent=True)
    k.fast_path()
    assert any(re.search(r'chain1d_kernel<100, (true|false), 1, 2>', nm) for nm in k.names), k.names        # the clamp flavour
    both_bars(R, 'two hyper', two_hyper, series)
    for s in (0, 3):
        W = two_hyper()
        W.loadData(series[s], silent=True)
        W.fit(silent=True)
        x, y, joint = R.getJointHyperParameterDistribution(s, ['sigma', 'log10pMin'])
        x0, y0, joint0 = W.getJointHyperParameterDistribution(['sigma', 'log10pMin'])
        assert np.array_equal(x, x0) and np.array_equal(y, y0) and joint.shape == (3, 2)
        assert np.allclose(joint, joint0, rtol=1e-9, atol=0)
        assert np.allclose(R.getJointHyperParameterDistribution(s, ['log10pMin', 'sigma'])[2], joint.T, rtol=0, atol=0)


# ---- batches -------------------------------------------------------------------------------------------------------------------------------
def test_batches_of_whole_groups_and_batches_through_groups(hip_engine):
    """S = 5, H = 3.  max_batch = 6: a full fit runs 2 + 2 + 1 groups, a device call each, the earlier batches' averages copied out.
    max_batch = 4, evidence-only: ONE call whose batches cut through the groups -- chains 0-3, 4-7, ... -- so a batch's first chain
    enters the table rows as (c0 + b) / H - c0 / H."""
    sigmas = [0.1, 0.2, 0.4]
    make, series = walk(37, sigmas), counts(7, [6] * 5)
    whole = make().fitMany(series, silent=True)
    whole_e = make().fitMany(series, evidenceOnly=True, silent=True)
    try:
        hip_engine.set_option('max_batch', 6)
        with Launched() as k:
            R = make().fitMany(series, silent=True)
        k.fast_path(calls=3)
        assert k.count['bl1c::series_lik_kernel'] == 3 and R._device is not None and R._device[1:3] == (4, 1)
        hip_engine.set_option('max_batch', 4)
        with Launched() as k:
            E = make().fitMany(series, evidenceOnly=True, silent=True)
        k.fast_path(calls=4, fold=False)
        assert E.lastTiming['batches'] == 4
    finally:
        hip_engine.set_option('max_batch', 4096)
    both_bars(R, 'batches', make, series)
    both_bars(E, 'batches', make, series, evidenceOnly=True)
    assert np.array_equal(R.logEvidence, whole.logEvidence) and np.array_equal(E.logEvidence, whole_e.logEvidence)
    for s in range(5):
        assert np.array_equal(R.logEvidenceList[s], whole.logEvidenceList[s]) and np.array_equal(E.logEvidenceList[s], whole_e.logEvidenceList[s])
        assert np.array_equal(R.posteriorMeanValues[s], whole.posteriorMeanValues[s])
        assert np.array_equal(R.averagePosteriorSequence(s), whole.averagePosteriorSequence(s))


# ---- ragged series ---------------------------------------------------------------------------------------------------------------------------
def test_ragged_series(capfd):
    """lengths 7, 5, 6 with per-series time stamps: padded steps (NaN at the end) change nothing above rounding, their entries are cut"""
    make = walk(37, [0.1, 0.2, 0.4])
    series = counts(3, [7, 5, 6])
    stamps = [np.arange(7) + 10.0, np.arange(5) * 2.0, np.arange(6) + 1.0]
    with Launched() as k:
        R = make().fitMany(series, timestamps=stamps, silent=True)
    k.fast_path()
    assert [len(le) for le in R.localEvidence] == [7, 5, 6] and [m.shape for m in R.posteriorMeanValues] == [(1, 7), (1, 5), (1, 6)]
    assert [R.averagePosteriorSequence(s).shape for s in range(3)] == [(7, 37), (5, 37), (6, 37)]
    both_bars(R, 'ragged', make, series, stamps=stamps)
    assert all(np.array_equal(a, b) for a, b in zip(R.formattedTimestamps, stamps))

    # ... a ChangePoint in the model: the program depends on the time stamp, the call takes the loop and says why
    def cp():
        S = bl.HyperStudy(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, 37)),
              bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('sigma', [0.1, 0.2, 0.4], target='rate'), bl.tm.ChangePoint('tChange', 3)), silent=True)
        return S
    stamps = [np.arange(7.0), np.arange(5.0), np.arange(6.0)]
    bl.Study._series_loop_announced = frozenset()
    capfd.readouterr()
    with Launched() as k:
        R = cp().fitMany(series, timestamps=stamps, silent=True)
    k.loop()
    err = capfd.readouterr().err
    assert err.count('fitMany runs the loop over HyperStudy.fit') == 1 and 'series of different lengths or time stamps' in err
    both_bars(R, 'ragged changepoint', cp, series, stamps=stamps)


# ---- ChangepointStudy ------------------------------------------------------------------------------------------------------------------------
def one_changepoint():
    S = bl.ChangepointStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 37)), bl.tm.ChangePoint('tc', 'all'), silent=True)
    return S


def two_changepoints():
    S = bl.ChangepointStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 37)),
          bl.tm.CombinedTransitionModel(bl.tm.ChangePoint('t1', [2, 4, 6]), bl.tm.ChangePoint('t2', [2, 4, 6])), silent=True)
    return S


def test_changepoint_study_over_all_time_steps():
    series = counts(8, [8] * 3)
    St = one_changepoint()
    with Launched() as k:
        R = St.fitMany(series, silent=True)
    k.fast_path()
    assert [len(h) for h in R.hyperParameterDistribution] == [7, 7, 7]
    both_bars(R, 'tc all', one_changepoint, series)
    assert St.transitionModel.hyperParameterValues[0] == 'all'                 # the study is left as it was
    values, dist = R.getHyperParameterDistribution(1, 'tc')
    assert np.array_equal(values, np.arange(7)) and abs(np.sum(dist) - 1.0) < 1e-12


def test_changepoint_study_mask_and_duration():
    """two change-points over [2, 4, 6]^2: the mask keeps 3 of 9 combinations, the distribution is scattered back to all 9"""
    series = counts(9, [8] * 3)
    with Launched() as k:
        R = two_changepoints().fitMany(series, silent=True)
    k.fast_path()
    assert [len(h) for h in R.hyperParameterDistribution] == [9, 9, 9] and [len(le) for le in R.logEvidenceList] == [3, 3, 3]
    both_bars(R, 'two cp', two_changepoints, series)
    for s in range(3):
        W = two_changepoints()
        W.loadData(series[s], silent=True)
        W.fit(silent=True)
        T1 = R.study(s)
        assert np.array_equal(T1.mask, W.mask) and int(np.sum(T1.mask)) == 3
        assert np.array_equal(T1.flatHyperPriorValues, W.flatHyperPriorValues) and np.array_equal(T1.hyperGridValues, W.hyperGridValues)
        d1, p1 = T1.getDurationDistribution(['t1', 't2'])
        d0, p0 = W.getDurationDistribution(['t1', 't2'])
        assert np.array_equal(d1, d0) and np.allclose(p1, p0, rtol=1e-9, atol=0)


# ---- chains that do not contribute -----------------------------------------------------------------------------------------------------------
# Bernoulli on linspace(0, 1, 5) with prior [1, 0, 0, 0, 1]; [1, 0, 1] rules out p = 0 and p = 1, the only cells the prior allows, so its
# sigma = 0 chain stops with a zero normaliser.  WIDE = 0.3 is a walk of radius 5 on the row of 5 cells: outside the envelope of the
# chain-resident 1-D kernel (radius < n), so the library refuses the batch and the call takes the loop, saying so.  NARROW = 0.05 (radius 1)
# is the same case inside the envelope: the grouped fold's own validity rules run.
WIDE, NARROW = 0.3, 0.05
CERTAIN = [np.array([1.0, 1.0, 1.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0])]


def certain(sigma, hyper_prior=None):
    def make():
        S = bl.HyperStudy(silent=True)
        S.set(bl.om.Bernoulli('p', np.linspace(0.0, 1.0, 5), prior=np.array([1.0, 0.0, 0.0, 0.0, 1.0])),
              bl.tm.GaussianRandomWalk('sigma', [0., sigma], target='p', prior=hyper_prior), silent=True)
        return S
    return make


def certain_fit(make, sigma, capfd):
    bl.Study._series_loop_announced = frozenset()
    capfd.readouterr()
    with Launched() as k:
        R = make().fitMany(CERTAIN, silent=True)
    err = capfd.readouterr().err
    if sigma == NARROW:
        k.fast_path(table='bl1c::series_table_kernel')
        assert 'fitMany runs the loop' not in err
    else:
        k.loop()
        assert err.count('fitMany runs the loop') == 1 and 'the chain-resident 1-D kernel does not take this batch (5 cells, radius 5' in err, err
    return R


@pytest.mark.parametrize('sigma', [WIDE, NARROW], ids=['radius5_of_5_cells', 'radius1'])
def test_a_chain_that_stops_contributes_nothing(sigma, capfd):
    """the sigma = 0 chain of [1, 0, 1] stops: the other chain alone makes the average"""
    make = certain(sigma)
    R = certain_fit(make, sigma, capfd)
    assert R.logEvidenceList[1][0] == -np.inf and np.isfinite(R.logEvidenceList[1][1])
    assert R.hyperParameterDistribution[1][0] == 0.0 and abs(R.hyperParameterDistribution[1][1] - 1.0 / sigma) < 1e-9 / sigma
    if sigma == WIDE:
        assert abs(R.logEvidenceList[1][1] - -3.159241429231785) < 1e-9 and abs(R.hyperParameterDistribution[1][1] - 3.3333333333) < 1e-9
    assert np.all(np.isfinite(R.averagePosteriorSequence(1))) and np.isfinite(R.logEvidence[1])
    both_bars(R, ('certain', sigma), make, CERTAIN)


@pytest.mark.parametrize('sigma', [WIDE, NARROW], ids=['radius5_of_5_cells', 'radius1'])
def test_a_series_nobody_contributes_to_is_nan(sigma, capfd):
    """hyper-prior [1, 0]: the walking chain has weight log(0), the sigma = 0 chain of [1, 0, 1] stops -- nothing contributes"""
    make = certain(sigma, [1., 0.])
    R = certain_fit(make, sigma, capfd)
    assert R.logEvidence[1] == -np.inf and np.all(np.isnan(R.hyperParameterDistribution[1]))
    assert R.averagePosteriorSequence(1).shape == (3, 5) and np.all(np.isnan(R.averagePosteriorSequence(1)))
    assert np.all(np.isnan(R.posteriorMeanValues[1]))
    for oracle in (True, False):
        g = golds_of(('certain 10', sigma), make, CERTAIN, None, oracle)
        assert g[1]['logEvidence'] == -np.inf and np.all(np.isnan(g[1]['hyperParameterDistribution']))
        for s in (0, 2):                                 # the other two series are unaffected
            compare.check(entry(R, s), g[s], compare.GPU_TOL)
        fin = np.isfinite(g[1]['logEvidenceList'])
        assert np.array_equal(np.isfinite(R.logEvidenceList[1]), fin)
        assert np.allclose(R.logEvidenceList[1][fin], g[1]['logEvidenceList'][fin], rtol=1e-9, atol=0)
    unaffected = certain(sigma)().fitMany(CERTAIN, silent=True)
    for s in (0, 2):
        assert np.array_equal(unaffected.logEvidenceList[s], R.logEvidenceList[s])


# ---- who owns the kept averages ---------------------------------------------------------------------------------------------------------------
def test_ownership_pickling_and_reads():
    make, series = walk(37, [0.1, 0.2, 0.4]), counts(21, [6] * 3)
    golds = golds_of('owner', make, series)
    S = make()
    S.loadData(series[2], silent=True)
    S.fit(silent=True)
    assert S._posterior_pending is not None                        # the study's average is on the device
    R = S.fitMany(series, silent=True)
    compare.check(result_of(S, {}), golds[2], compare.GPU_TOL)     # ... and was not lost to fitMany's device call
    assert np.array_equal(S.rawData, series[2])
    assert R._device is not None                                   # R's averages are on the device
    values, dist = R.getParameterDistributions(1, 'rate')          # ... reduced there
    assert np.allclose(dist * S.latticeConstant[0], R.averagePosteriorSequence(1), rtol=1e-13, atol=0)
    assert np.array_equal(R.getParameterMeanValues(1, 'rate'), R.posteriorMeanValues[1][0])
    S.fit(silent=True)                                             # a fit on the same engine: R's averages are copied out first
    assert R._device is None
    at_the_bar(R, golds)
    values2, dist2 = R.getParameterDistributions(1, 'rate')        # ... and read from the host
    assert np.array_equal(values, values2) and np.allclose(dist, dist2, rtol=1e-13, atol=0)
    R2 = pickle.loads(pickle.dumps(make().fitMany(series, silent=True)))
    assert isinstance(R2, bl.HyperSeriesFits) and R2._device is None
    at_the_bar(R2, golds)
    compare.check(result_of(R2.study(0), {}), golds[0], compare.GPU_TOL)


# ---- calls that take the loop ------------------------------------------------------------------------------------------------------------------
def test_option_and_group_size_send_the_call_to_the_loop(hip_engine, capfd):
    make, series = walk(37, [0.1, 0.2, 0.4]), counts(5, [6] * 3)
    for key, off, on, why in (('series_fit', 0, 1, 'option series_fit is 0'), ('max_batch', 2, 4096, 'a group of 3 chains is beyond the batch cap of 2')):
        bl.Study._series_loop_announced = frozenset()
        capfd.readouterr()
        hip_engine.set_option(key, off)
        try:
            with Launched() as k:
                R = make().fitMany(series, silent=True)
                R2 = make().fitMany(series, silent=True)
        finally:
            hip_engine.set_option(key, on)
        k.loop()
        err = capfd.readouterr().err
        assert err.count('fitMany runs the loop') == 1 and why in err, err
        both_bars(R, 'refused', make, series)
        at_the_bar(R2, golds_of('refused', make, series))


def test_one_hyper_grid_point_takes_the_path_of_a_plain_study():
    """at most one combination of hyper-parameter values: fit switches to Study.fit, fitMany to Study.fitMany's device path"""
    make, series = walk(37, [0.2]), counts(5, [6] * 3)
    St = make()
    with Launched() as k:
        R = St.fitMany(series, silent=True)
    assert k.count.get('bl1c::series_lik_kernel', 0) == 1 and FOLD not in k.count, k.count
    assert isinstance(R, bl.HyperSeriesFits) and R.hyperParameterDistribution == [None] * 3 and [len(le) for le in R.logEvidenceList] == [0, 0, 0]
    both_bars(R, 'one point', make, series)
    assert St.transitionModel.hyperParameterValues[0] == [0.2]


def test_two_parameter_grid_takes_the_loop(capfd):
    def make():
        S = bl.HyperStudy(silent=True)
        S.set(bl.om.Gaussian('mean', bl.cint(-2, 2, 33), 'std', bl.oint(0, 2, 32)), bl.tm.GaussianRandomWalk('sigma', [0.1, 0.2], target='mean'), silent=True)
        return S
    rng = np.random.RandomState(2)
    series = [rng.normal(0.0, 1.0, size=k) for k in (5, 3)]
    bl.Study._series_loop_announced = frozenset()
    capfd.readouterr()
    with Launched() as k:
        R = make().fitMany(series, silent=True)
    k.loop()
    err = capfd.readouterr().err
    assert err.count('fitMany runs the loop') == 1 and 'a grid of 2 parameters' in err
    both_bars(R, 'two parameters', make, series)


# ---- the fold alone ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, sigmas', [(37, [0.1, 0.2, 0.4]), (64, bl.cint(0, 1, 20))], ids=['n37-H3', 'n64-H20'])
def test_the_fold_against_longdouble(hip_engine, n, sigmas):
    """The same S H chains fitted with their sequences kept and no fold; sum_h w max(p, 1e-300), row-normalised, formed in np.longdouble
    from those per-chain sequences and evidences; the device's averages against it.  Bound, relative per cell: (H + 4) 2^-53 -- H
    products and additions, the normalising sum's share, one division.  (The weights are the library's own double values:
    exp(logE + log prior - max) by the C library's exp, which math.exp calls too.)"""
    S, T, H = 3, 8, len(sigmas)
    make, series = walk(n, sigmas), counts(n, [T] * S)
    W = make()._seriesWorker()
    W.loadData(series[0], silent=True)
    W._formatData()
    W._createSeriesHyperGrid()
    W._setAllHyperParameters(W.hyperGridValues[0])
    problem, program = W._compile(silent=True)
    W._setAllHyperParameters(W.flatHyperParameters)
    ov = np.tile(W._opValueMatrix(program, np.asarray(W.hyperGridValues, dtype=float)), (S, 1))
    log_w = np.tile(np.log(np.asarray(W.flatHyperPriorValues, dtype=float)), S)
    data = np.stack(series).reshape(S, T, 1, 1)
    res = hip_engine.fit_series_groups(problem, data, H, ov, keep_posterior=True)
    chains = np.stack([np.array(hip_engine.posterior(c, T, [n])) for c in range(S * H)]).reshape(S, H, T, n)
    with Launched() as k:
        folded = hip_engine.fit_series_groups(problem, data, H, ov, keep_posterior=True, accumulate=True, log_chain_weight=log_w)
    assert k.count.get(FOLD, 0) == 1, k.count
    assert np.array_equal(folded.log_evidence, res.log_evidence) and folded.posterior_mean.shape == (S, 1, T)
    bound = (H + 4) * 2.0 ** -53
    worst = 0.0
    for s in range(S):
        lw = res.log_evidence[s * H:(s + 1) * H] + log_w[s * H:(s + 1) * H]
        w = np.array([math.exp(v - np.max(lw)) for v in lw], dtype=np.longdouble)
        want = np.sum(w[:, None, None] * np.maximum(chains[s].astype(np.longdouble), np.longdouble(1e-300)), axis=0)
        want = want / np.sum(want, axis=1, keepdims=True)
        got = np.array(hip_engine.posterior(s, T, [n])).astype(np.longdouble)
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
    print('fold n = %d, H = %d: worst relative error %.3e = %.2f x 2^-53 (bound %d x 2^-53)' % (n, H, worst, worst * 2.0 ** 53, H + 4))
    assert worst <= bound
    hip_engine.release_posterior(None)
