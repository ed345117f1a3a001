"""
Study.fitMany without a GPU: the admission rules and the memory plan of the series path (blhip_host_series_check / _plan through ctypes:
host-only, no context), and fitMany itself on the oracle-backed engine, where every call runs the loop -- results per series equal to the
user's loop, the study untouched, the result picklable, the loop announced once.
"""
import ctypes as C
import pickle

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.core import Study
from oracle_engine import OracleEngine


# ---- blhip_host_series_check / blhip_host_series_plan --------------------------------------------------------------------------------
def problem(om=_abi.OM_POISSON, n=(200,), T=10, data_dim=1, seg_len=1, ops=((_abi.OP_GRW, 0),), lik=False):
    keep = []
    p = _abi.Problem()
    p.ndim, p.obs_model, p.T, p.seg_len, p.data_dim = len(n), om, T, seg_len, data_dim
    for k, nk in enumerate(n):
        m = np.linspace(0.1, 6.0, nk)
        keep.append(m)
        p.n[k], p.marginal[k], p.lattice[k] = nk, _abi.dptr(m), m[1] - m[0]
    G = int(np.prod(n))
    data, ts, prior = np.ones(T * seg_len * data_dim), np.arange(T, dtype=float), np.ones(G) / G
    keep += [data, ts, prior]
    p.data, p.timestamps, p.prior = _abi.dptr(data), _abi.dptr(ts), _abi.dptr(prior)
    if lik:
        table = np.ones(T * G)
        keep.append(table)
        p.lik = _abi.dptr(table)
    arr = (_abi.Op * max(1, len(ops)))()
    for k, op in enumerate(ops):
        arr[k].kind, arr[k].axis, arr[k].segment, arr[k].flags = op[0], op[1], op[2] if len(op) > 2 else -1, 0
    keep.append(arr)
    p.n_ops, p.ops = len(ops), arr
    return p, keep


def check(p, S=8, flags=0):
    err = C.create_string_buffer(400)
    rc = _abi.load().blhip_host_series_check(C.byref(p), S, flags, err, 400)
    return rc, err.value.decode()


@pytest.mark.parametrize('om, dd', [(_abi.OM_POISSON, 1), (_abi.OM_GAUSSIAN_MEAN, 2), (_abi.OM_BERNOULLI, 1), (_abi.OM_WHITE_NOISE, 1)])
def test_check_admits_the_four_one_parameter_models(om, dd):
    p, keep = problem(om=om, data_dim=dd)
    assert check(p) == (0, '')
    assert check(p, flags=_abi.FORWARD_ONLY | _abi.KEEP_POSTERIOR) == (0, '')
    assert check(p, flags=_abi.EVIDENCE_ONLY | _abi.SERIES_RAGGED) == (0, '')


@pytest.mark.parametrize('kw, flags, word', [
    (dict(n=(20, 30), om=_abi.OM_GAUSSIAN), 0, 'grid of 2 parameters'),
    (dict(om=_abi.OM_TABLE, lik=True), 0, 'BLHIP_OM_TABLE'),
    (dict(om=_abi.OM_PROGRAM), 0, 'BLHIP_OM_PROGRAM'),
    (dict(n=(8193,)), 0, 'row of 8193 cells'),
    (dict(), _abi.RESUME, 'BLHIP_RESUME'),
    (dict(), _abi.CARRY | _abi.EVIDENCE_ONLY, 'BLHIP_CARRY'),
    (dict(), _abi.ACCUMULATE, 'BLHIP_ACCUMULATE'),
    (dict(ops=((_abi.OP_GRW, 0), (_abi.OP_CHANGEPOINT, 0))), _abi.SERIES_RAGGED, 'depends on the time stamp'),
    (dict(ops=((_abi.OP_GRW, 0, 0), (_abi.OP_BREAKPOINT, 0), (_abi.OP_STATIC, 0, 1))), _abi.SERIES_RAGGED, 'time'),
    (dict(ops=((_abi.OP_ALPHASTABLE, 0), (_abi.OP_ALPHASTABLE_ARG, 0))), 0, 'AlphaStable'),
])
def test_check_refuses_with_a_reason(kw, flags, word):
    p, keep = problem(**kw)
    rc, why = check(p, flags=flags)
    assert rc == 1 and word in why, (rc, why)


def test_check_takes_the_longest_row_and_time_dependent_programs_of_equal_series():
    p, keep = problem(n=(8192,))
    assert check(p)[0] == 0
    p, keep = problem(ops=((_abi.OP_GRW, 0), (_abi.OP_CHANGEPOINT, 0)))
    assert check(p)[0] == 0                      # (equal lengths and stamps: any program the chain-resident kernel runs)
    assert _abi.load().blhip_host_series_check(C.byref(p), 8, 0, None, 0) == 0
    assert _abi.load().blhip_host_series_check(None, 8, 0, None, 0) == 1


def plan(p, S, flags, budget):
    out = (C.c_int64 * 4)()
    rc = _abi.load().blhip_host_series_plan(C.byref(p), S, flags, float(budget), out)
    return rc, [int(v) for v in out]


@pytest.mark.parametrize('flags', [0, _abi.EVIDENCE_ONLY])
def test_plan_stays_in_its_budget_and_covers_every_series_once(flags):
    T, n = 110, 200
    p, keep = problem(T=T, n=(n,))
    rc, (per, batches, nbytes, least) = plan(p, 1, flags, 1e12)
    assert rc == 0 and (per, batches) == (1, 1) and nbytes == least
    # a chain: its state ping-pong, the stored sequence unless evidence-only, the partial sums -- and its own (T, n) likelihood table
    rows = 2 if flags else T + 2
    assert least == rows * n * 8 + T * 7 * 8 * 2 * 64 + T * n * 8
    for S in (1, 2, 7, 100, 4096, 4097, 10000):
        for budget in (least, 3 * least + 5, 64 * least, 1e13):
            rc, (per, batches, nbytes, least2) = plan(p, S, flags, budget)
            assert rc == 0 and least2 == least
            assert 1 <= per <= min(S, 4096) and nbytes <= budget and nbytes == per * least
            cover = np.zeros(S, dtype=int)
            for b in range(batches):
                cover[b * per:min(S, (b + 1) * per)] += 1
            assert np.all(cover == 1) and (batches - 1) * per < S
            assert per == min(S, 4096, int(budget // least))       # (no batch smaller than the budget allows)
    rc, out = plan(p, 5, flags, least - 1)
    assert rc == 1 and out[3] == least and out[0] == 0
    assert plan(p, 5, flags | _abi.RESUME, 1e12)[0] == -1
    p2, keep2 = problem(n=(20, 30), om=_abi.OM_GAUSSIAN)
    assert plan(p2, 5, 0, 1e12)[0] == -1


# ---- fitMany on the oracle-backed engine ----------------------------------------------------------------------------------------------
@pytest.fixture
def oracle_engine():
    eng = OracleEngine()
    prev = bl.set_engine(eng)
    yield eng
    bl.set_engine(prev)


def poisson_study():
    S = bl.Study(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 40)), bl.tm.GaussianRandomWalk('sigma', 0.3, target='rate'), silent=True)
    return S


def gaussian_study():
    S = bl.Study(silent=True)
    S.set(bl.om.Gaussian('mean', bl.cint(-2, 2, 9), 'std', bl.oint(0, 2, 8)),
          bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s1', 0.3, target='mean'), bl.tm.GaussianRandomWalk('s2', 0.2, target='std')), silent=True)
    return S


RNG = np.random.RandomState(7)
COUNTS = [RNG.poisson(2.0, size=k).astype(float) for k in (6, 4, 1, 6)]
COUNTS[0][2] = np.nan
VALUES = [RNG.normal(0.0, 1.0, size=k) for k in (5, 3, 5)]


def loop(make, series, stamps=None, **kw):
    """what the user's loop leaves on a study, series by series"""
    out = []
    for s, d in enumerate(series):
        S = make()
        S.loadData(d, timestamps=None if stamps is None else stamps[s], silent=True)
        S.fit(silent=True, **kw)
        out.append(dict(logEvidence=S.logEvidence, localEvidence=np.array(S.localEvidence), means=np.array(S.posteriorMeanValues),
                        post=S.posteriorSequence, stamps=np.array(S.formattedTimestamps)))
    return out


def same(R, want):
    assert len(R) == len(want)
    assert np.array_equal(R.logEvidence, [w['logEvidence'] for w in want])
    assert np.array_equal(R.log10Evidence, R.logEvidence / np.log(10))
    for s, w in enumerate(want):
        assert np.array_equal(R.localEvidence[s], w['localEvidence'], equal_nan=True)
        assert np.array_equal(R.posteriorMeanValues[s], w['means'])
        assert np.array_equal(R.formattedTimestamps[s], w['stamps'])
        post = R.posteriorSequence(s)
        assert (post is None and w['post'] is None) or np.array_equal(post, w['post'])


@pytest.mark.parametrize('make, series', [(poisson_study, COUNTS), (gaussian_study, VALUES)], ids=['poisson_ragged', 'two_parameters'])
@pytest.mark.parametrize('kw', [{}, dict(forwardOnly=True), dict(evidenceOnly=True)], ids=['full', 'forwardOnly', 'evidenceOnly'])
def test_fitmany_equals_the_loop(oracle_engine, make, series, kw):
    S = make()
    S.loadData(series[0], silent=True)
    R = S.fitMany(series, silent=True, **kw)
    assert isinstance(R, bl.SeriesFits)
    same(R, loop(make, series, **kw))
    if not kw.get('evidenceOnly'):
        name = S.observationModel.parameterNames[0]
        for s in range(len(series)):
            T1 = R.study(s)
            values, dist = R.getParameterDistributions(s, name)
            v1, d1 = T1.getParameterDistributions(name)
            assert np.array_equal(values, v1) and np.array_equal(dist, d1) and dist.shape[0] == len(series[s])
            assert np.array_equal(R.getParameterMeanValues(s, name), T1.getParameterMeanValues(name))
            assert np.array_equal(T1.rawData, series[s], equal_nan=True) and T1.logEvidence == R.logEvidence[s]


def test_fitmany_time_stamps_shared_and_per_series(oracle_engine):
    series = [COUNTS[0], COUNTS[3]]
    shared = np.arange(1900, 1906)
    S = poisson_study()
    R = S.fitMany(series, timestamps=shared, silent=True)
    same(R, loop(poisson_study, series, stamps=[shared, shared]))
    each = [np.arange(10, 16), np.arange(6) * 2.0]
    R = S.fitMany(series, timestamps=each, silent=True)
    same(R, loop(poisson_study, series, stamps=each))
    with pytest.raises(bl.ConfigurationError):
        S.fitMany(series, timestamps=each[:1], silent=True)


def test_fitmany_leaves_the_study_as_it_was(oracle_engine):
    S = poisson_study()
    S.loadData(COUNTS[3], silent=True)
    S.fit(silent=True)
    assert S._posterior_pending is not None           # (the study's own sequence is still the engine's)
    before = dict(raw=S.rawData.copy(), stamps=np.array(S.rawTimestamps), logE=S.logEvidence, local=np.array(S.localEvidence),
                  means=np.array(S.posteriorMeanValues), formatted=np.array(S.formattedData))
    R = S.fitMany(COUNTS, silent=True)
    assert np.array_equal(S.rawData, before['raw']) and np.array_equal(S.rawTimestamps, before['stamps'])
    assert np.array_equal(S.formattedData, before['formatted'])
    assert S.logEvidence == before['logE'] and np.array_equal(S.localEvidence, before['local'])
    assert np.array_equal(S.posteriorMeanValues, before['means'])
    want = loop(poisson_study, [COUNTS[3]])[0]
    assert np.array_equal(S.posteriorSequence, want['post'])       # (brought to the host before the engine was reused, not dropped)
    same(R, loop(poisson_study, COUNTS))
    S.fit(silent=True)                                             # ... and a fit right after leaves R's results alone
    same(R, loop(poisson_study, COUNTS))


def test_series_fits_pickle(oracle_engine):
    S = poisson_study()
    R = S.fitMany(COUNTS, silent=True)
    R2 = pickle.loads(pickle.dumps(pickle.loads(pickle.dumps(R))))
    same(R2, loop(poisson_study, COUNTS))
    assert np.array_equal(R2.study(1).posteriorSequence, R.posteriorSequence(1))
    assert R2._device is None


def test_zero_normaliser_in_one_series(oracle_engine, capsys):
    def make():
        S = bl.Study(silent=True)
        S.set(bl.om.Bernoulli('p', np.array([0.0, 1.0]), prior=lambda p: np.ones_like(p)), bl.tm.Static(), silent=True)
        return S
    series = [np.array([1.0, 1.0, 1.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, 0.0])]       # (the second: no p in {0, 1} gives both outcomes)
    R = make().fitMany(series, silent=True)
    assert R.logEvidence[1] == -np.inf and np.all(np.isfinite(R.logEvidence[[0, 2]]))
    assert R.posteriorSequence(1) is None and R.study(1).logEvidence == -np.inf
    want = loop(make, series)
    for s in (0, 2):
        assert R.logEvidence[s] == want[s]['logEvidence'] and np.array_equal(R.posteriorSequence(s), want[s]['post'])


def test_the_loop_is_announced_once(oracle_engine, capsys):
    Study._series_loop_announced = frozenset()
    S = poisson_study()
    S.fitMany(COUNTS, silent=True)
    S.fitMany(COUNTS[:2], silent=True)
    poisson_study().fitMany(COUNTS, silent=True)
    err = capsys.readouterr().err
    assert err.count('fitMany runs the loop over Study.fit') == 1, err
    assert 'the engine has no series fits' in err


def test_fitmany_needs_models_and_series(oracle_engine):
    with pytest.raises(bl.ConfigurationError):
        bl.Study(silent=True).fitMany(COUNTS, silent=True)
    with pytest.raises(bl.ConfigurationError):
        poisson_study().fitMany([], silent=True)
    R = poisson_study().fitMany(COUNTS, silent=True)
    with pytest.raises(IndexError):
        R.posteriorSequence(len(COUNTS))
