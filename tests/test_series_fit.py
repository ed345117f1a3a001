"""
Study.fitMany on a real MI355X: many data series on a one-parameter grid as ONE device call per batch of series (blhip_set_series: a chain
of the chain-resident 1-D kernel per series, over a (B, T, n) likelihood table built by bl1c::series_lik_kernel / series_table_kernel).

Every case compares, per series, logEvidence, localEvidence, the posterior means and the whole posterior sequence with the CPU oracle's
fit of that series ALONE, at the project's parity bar (compare.GPU_TOL).  The shapes are the smallest that reach each code path.
"""
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

    def fast_path(self, table, chain, calls=1):
        """the series table kernel and the chain-resident kernel (a table per batch, a launch per pass), no per-step kernel"""
        assert self.count.get(table, 0) >= calls, self.count
        assert self.count.get(chain, 0) >= calls, self.count
        assert not [f for f in self.count if f in PER_STEP], self.count
        assert not [f for f in self.count if f in SERIES + CHAIN and f not in (table, chain)], self.count


def oracle_alone(make, data, stamps=None, **kw):
    """the oracle's fit of one series alone, as compare.check takes it"""
    prev = bl.set_engine(OracleEngine())
    try:
        S = make()
        S.loadData(np.asarray(data), timestamps=stamps, silent=True)
        S.fit(silent=True, **kw)
        gold = dict(logEvidence=S.logEvidence, localEvidence=np.array(S.localEvidence))
        if not kw.get('evidenceOnly') and np.isfinite(S.logEvidence):
            gold['posteriorMeanValues'] = np.array(S.posteriorMeanValues)
            gold['posteriorSequence'] = np.array(S.posteriorSequence)
        return gold
    finally:
        bl.set_engine(prev)


def entry(R, s):
    res = dict(logEvidence=R.logEvidence[s], localEvidence=R.localEvidence[s])
    if not R.evidenceOnly and np.isfinite(R.logEvidence[s]):
        res['posteriorMeanValues'] = R.posteriorMeanValues[s]
        res['posteriorSequence'] = R.posteriorSequence(s)
    return res


def at_the_bar(R, golds):
    assert len(R) == len(golds)
    for s, gold in enumerate(golds):
        res = entry(R, s)
        if 'posteriorSequence' in gold:
            assert np.shape(res['posteriorSequence']) == gold['posteriorSequence'].shape
        compare.check(res, gold, compare.GPU_TOL)


def poisson(n, sigma=0.2):
    def make():
        S = bl.Study(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, n)), bl.tm.GaussianRandomWalk('sigma', sigma, target='rate'), silent=True)
        return S
    return make


def counts(seed, lengths, rate=2.0):
    rng = np.random.RandomState(seed)
    return [rng.poisson(rate + s, size=k).astype(float) for s, k in enumerate(lengths)]       # (series differ: a wrong row offset shows)


_GOLD = {}


def golds_of(key, make, series, stamps=None, **kw):
    """the oracle's fits of a case, computed once"""
    k = (key, tuple(sorted(kw.items())))
    if k not in _GOLD:
        _GOLD[k] = [oracle_alone(make, d, None if stamps is None else stamps[s], **kw) for s, d in enumerate(series)]
    return _GOLD[k]


# ---- the shapes of the chain kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, S, T, chain', [
    (37, 5, 6, 'bl1c::chain1d_kernel'),          # a row shorter than a block, radius 5
    (300, 3, 5, 'bl1c::chain1d_kernel'),         # more cells than the table kernel's block has threads
    (600, 2, 4, 'bl1c::chain1d_kernel'),         # more cells than the chain kernel's block: two cells per thread (M = 2)
    (4097, 2, 4, 'bl1c::chain1d_long_kernel'),   # the long-row kernel, which has no likelihood but the table; an odd row: 8-byte stores
])
def test_poisson_series(n, S, T, chain):
    make, series = poisson(n), counts(n, [T] * S)
    St = make()
    St.loadData(series[0], silent=True)
    with Launched() as k:
        R = St.fitMany(series, silent=True)
    k.fast_path('bl1c::series_lik_kernel', chain)
    assert R.lastTiming['fwd_kernel_variant'] == 9 and R.lastTiming['bwd_kernel_variant'] == 9
    if n == 600:
        assert any('chain1d_kernel<100, false, 2, 0>' in nm for nm in k.names), k.names
    at_the_bar(R, golds_of(('poisson', n), make, series))
    # the accessors read the device-resident sequences
    values, dist = R.getParameterDistributions(1, 'rate')
    assert np.allclose(dist * St.latticeConstant[0], R.posteriorSequence(1), rtol=1e-13, atol=0)
    assert np.array_equal(R.getParameterMeanValues(1, 'rate'), R.posteriorMeanValues[1][0])


def gaussian_mean():
    S = bl.Study(silent=True)
    S.set(bl.om.GaussianMean('mean', bl.cint(-3, 3, 65)), bl.tm.GaussianRandomWalk('sigma', 0.3, target='mean'), silent=True)
    return S


def bernoulli():
    S = bl.Study(silent=True)
    S.set(bl.om.Bernoulli('p', bl.oint(0, 1, 65)), bl.tm.GaussianRandomWalk('sigma', 0.05, target='p'), silent=True)
    return S


def white_noise():
    S = bl.Study(silent=True)
    S.set(bl.om.WhiteNoise('std', bl.oint(0, 3, 65)), bl.tm.GaussianRandomWalk('sigma', 0.1, target='std'), silent=True)
    return S


def _model_series(which):
    rng = np.random.RandomState(11)
    if which == 'gaussian_mean':       # data points (value, standard deviation)
        return [np.stack([rng.normal(0.3 * s, 1.0, size=5), rng.uniform(0.5, 1.5, size=5)], axis=1) for s in range(4)]
    if which == 'bernoulli':
        return [(rng.uniform(size=5) < 0.2 + 0.2 * s).astype(float) for s in range(4)]
    return [rng.normal(0.0, 0.5 + 0.5 * s, size=5) for s in range(4)]


@pytest.mark.parametrize('which, make, table', [('gaussian_mean', gaussian_mean, 'bl1c::series_lik_kernel'),
                                                ('bernoulli', bernoulli, 'bl1c::series_table_kernel'),
                                                ('white_noise', white_noise, 'bl1c::series_table_kernel')])
def test_every_table_builder(which, make, table):
    series = _model_series(which)
    series[2] = series[2].copy()
    series[2][1] = np.nan                                          # (missing data inside a series is ordinary input)
    with Launched() as k:
        R = make().fitMany(series, silent=True)
    k.fast_path(table, 'bl1c::chain1d_kernel')
    at_the_bar(R, golds_of(which, make, series))


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def test_batches_of_three(hip_engine):
    """7 series in batches of 3 + 3 + 1: the batch's first chain enters the series index, and the results do not depend on the batch size.
    Evidence-only: the batches of ONE blhip_fit; with sequences: a device call per batch, the earlier batches' sequences copied out."""
    make, series = poisson(37), counts(5, [6] * 7)
    whole = make().fitMany(series, silent=True)
    whole_e = make().fitMany(series, evidenceOnly=True, silent=True)
    hip_engine.set_option('max_batch', 3)
    try:
        with Launched() as k:
            R = make().fitMany(series, silent=True)
        k.fast_path('bl1c::series_lik_kernel', 'bl1c::chain1d_kernel', calls=3)
        assert k.count['bl1c::series_lik_kernel'] == 3
        with Launched() as k:
            E = make().fitMany(series, evidenceOnly=True, silent=True)
        k.fast_path('bl1c::series_lik_kernel', 'bl1c::chain1d_kernel', calls=3)
        assert E.lastTiming['batches'] == 3
    finally:
        hip_engine.set_option('max_batch', 4096)
    at_the_bar(R, golds_of('batches', make, series))
    at_the_bar(E, golds_of('batches', make, series, evidenceOnly=True))
    assert np.array_equal(R.logEvidence, whole.logEvidence) and np.array_equal(E.logEvidence, whole_e.logEvidence)
    for s in range(7):
        assert np.array_equal(R.localEvidence[s], whole.localEvidence[s]) and np.array_equal(E.localEvidence[s], whole_e.localEvidence[s])
        assert np.array_equal(R.posteriorMeanValues[s], whole.posteriorMeanValues[s])
        assert np.array_equal(R.posteriorSequence(s), whole.posteriorSequence(s))


# ---- padding, missing data, clamps -------------------------------------------------------------------------------------------------------
def regime():
    S = bl.Study(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 37)),
          bl.tm.CombinedTransitionModel(bl.tm.Static(), bl.tm.GaussianRandomWalk('sigma', 0.2, target='rate'), bl.tm.RegimeSwitch('log10pMin', -7)),
          silent=True)
    return S


def test_ragged_series_with_a_clamp():
    """lengths 6, 4, 1 and a NaN inside the longest: padded steps (NaN at the end) change nothing above rounding; the clamp flavour (CL = 2)"""
    series = counts(3, [6, 4, 1])
    series[0][2] = np.nan
    with Launched() as k:
        R = regime().fitMany(series, silent=True)
    k.fast_path('bl1c::series_lik_kernel', 'bl1c::chain1d_kernel')
    assert any(re.search(r'chain1d_kernel<100, (true|false), 1, 2>', nm) for nm in k.names), k.names
    assert [len(le) for le in R.localEvidence] == [6, 4, 1] and [m.shape for m in R.posteriorMeanValues] == [(1, 6), (1, 4), (1, 1)]
    at_the_bar(R, golds_of('ragged', regime, series))
    # per-series time stamps that differ ride on the same time-independent program
    stamps = [np.arange(6) + 10.0, np.arange(4) * 2.0, np.array([5.0])]
    R2 = regime().fitMany(series, timestamps=stamps, silent=True)
    at_the_bar(R2, golds_of('ragged', regime, series))
    assert all(np.array_equal(a, b) for a, b in zip(R2.formattedTimestamps, stamps))


def changepoint():
    S = bl.Study(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 37)),
          bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('sigma', 0.2, target='rate'), bl.tm.ChangePoint('tChange', 1903)), silent=True)
    return S


@pytest.mark.parametrize('kw', [{}, dict(forwardOnly=True), dict(evidenceOnly=True)], ids=['full', 'forwardOnly', 'evidenceOnly'])
def test_time_dependent_program_of_equal_series(kw, capfd):
    """equal lengths and stamps: a ChangePoint at a fixed stamp runs on the fast path; so do forwardOnly and evidenceOnly"""
    series, stamps = counts(9, [6] * 4), np.arange(1900, 1906)
    with Launched() as k:
        R = changepoint().fitMany(series, timestamps=stamps, silent=True, **kw)
    k.fast_path('bl1c::series_lik_kernel', 'bl1c::chain1d_kernel')
    at_the_bar(R, golds_of('changepoint', changepoint, series, stamps=[stamps] * 4, **kw))
    # ... and ragged series of such a model take the loop, which is as right
    bl.Study._series_loop_announced = frozenset()
    with Launched() as k:
        R = changepoint().fitMany(series[:2] + [series[2][:4]], timestamps=[stamps, stamps, stamps[:4]], silent=True, **kw)
    assert not [f for f in k.count if f in SERIES], k.count
    assert 'fitMany runs the loop' in capfd.readouterr().err
    at_the_bar(R, golds_of('changepoint ragged', changepoint, series[:2] + [series[2][:4]], stamps=[stamps, stamps, stamps[:4]], **kw))


# ---- a zero normaliser in one series ---------------------------------------------------------------------------------------------------------
def certain():
    S = bl.Study(silent=True)
    S.set(bl.om.Bernoulli('p', np.linspace(0.0, 1.0, 5), prior=np.array([1.0, 0.0, 0.0, 0.0, 1.0])), bl.tm.Static(), silent=True)
    return S


def test_zero_normaliser_in_one_series(capsys):
    series = [np.array([1.0, 1.0, 1.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0])]      # (the second: p = 0 and p = 1 both ruled out)
    with Launched() as k:
        R = certain().fitMany(series, silent=True)
    k.fast_path('bl1c::series_table_kernel', 'bl1c::chain1d_kernel')
    assert R.logEvidence[1] == -np.inf and R.posteriorSequence(1) is None and R.study(1).logEvidence == -np.inf
    at_the_bar(R, golds_of('certain', certain, series))


# ---- who owns the kept posterior ---------------------------------------------------------------------------------------------------------------
def test_ownership_of_the_kept_posterior_in_both_directions():
    make, series = poisson(37), counts(21, [6] * 3)
    golds = golds_of('owner', make, series)
    S = make()
    S.loadData(series[2], silent=True)
    S.fit(silent=True)
    assert S._posterior_pending is not None                        # the study's sequence is on the device
    R = S.fitMany(series, silent=True)
    assert S._posterior_pending is None                            # ... copied out by fitMany's device call, not dropped
    compare.check(dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence, posteriorMeanValues=S.posteriorMeanValues,
                       posteriorSequence=S.posteriorSequence), golds[2], compare.GPU_TOL)
    assert np.array_equal(S.rawData, series[2])
    assert R._device is not None                                   # R's sequences are on the device
    S.fit(silent=True)                                             # a fit on the same engine: R's sequences are copied out first
    assert R._device is None
    at_the_bar(R, golds)
    R2 = pickle.loads(pickle.dumps(make().fitMany(series, silent=True)))
    at_the_bar(R2, golds)
    T1 = R2.study(0)
    compare.check(dict(logEvidence=T1.logEvidence, localEvidence=T1.localEvidence, posteriorMeanValues=T1.posteriorMeanValues,
                       posteriorSequence=T1.posteriorSequence), golds[0], compare.GPU_TOL)


# ---- the same kernel, the same table values: bit for bit ----------------------------------------------------------------------------------------
def test_bit_for_bit_with_single_fits(hip_engine):
    """chain1d = 2 sends a single fit to the chain-resident kernel as well: entry s of fitMany and a fit of series s alone run the same
    kernel flavour on the same likelihood values (the table's are those of the in-kernel function), and chains do not interact."""
    make, series = poisson(37), counts(33, [6] * 4)
    R = make().fitMany(series, silent=True)
    hip_engine.set_option('chain1d', 2)
    try:
        for s, d in enumerate(series):
            S = make()
            S.loadData(d, silent=True)
            S.fit(silent=True)
            assert S.lastTiming['fwd_kernel_variant'] == 9
            assert R.logEvidence[s] == S.logEvidence
            assert np.array_equal(R.localEvidence[s], S.localEvidence)
            assert np.array_equal(R.posteriorMeanValues[s], S.posteriorMeanValues)
            assert np.array_equal(R.posteriorSequence(s), S.posteriorSequence)
    finally:
        hip_engine.set_option('chain1d', 1)


# ---- calls that take the loop ------------------------------------------------------------------------------------------------------------------
def test_two_parameter_model_launches_what_the_loop_launches(capfd):
    def make():
        S = bl.Study(silent=True)
        S.set(bl.om.Gaussian('mean', bl.cint(-2, 2, 33), 'std', bl.oint(0, 2, 32)), bl.tm.GaussianRandomWalk('sigma', 0.2, target='mean'), silent=True)
        return S
    rng = np.random.RandomState(2)
    series = [rng.normal(0.0, 1.0, size=k) for k in (5, 3)]
    bl.Study._series_loop_announced = frozenset()
    with Launched() as k:
        R = make().fitMany(series, silent=True)
    err = capfd.readouterr().err
    assert err.count('fitMany runs the loop') == 1 and 'Gaussian' in err
    with Launched() as k2:
        for d in series:
            S = make()
            S.loadData(d, silent=True)
            S.fit(silent=True)
            S.posteriorSequence
    assert k.count == k2.count and not [f for f in k.count if f in SERIES]
    at_the_bar(R, golds_of('two parameters', make, series))


def test_option_and_envelope_send_the_call_to_the_loop(hip_engine, capfd):
    make, series = poisson(37), counts(5, [6] * 3)
    golds = golds_of('refused', make, series)
    for key, off, on in (('series_fit', 0, 1), ('chain1d', 0, 1)):         # the option itself; the chain-resident kernel switched off
        bl.Study._series_loop_announced = frozenset()
        hip_engine.set_option(key, off)
        try:
            with Launched() as k:
                R = make().fitMany(series, silent=True)
        finally:
            hip_engine.set_option(key, on)
        assert not [f for f in k.count if f in SERIES], (key, k.count)
        assert 'fitMany runs the loop' in capfd.readouterr().err
        at_the_bar(R, golds)
    R = make().fitMany(series[:1], silent=True)                             # fewer than SERIES_MIN
    at_the_bar(R, golds[:1])
