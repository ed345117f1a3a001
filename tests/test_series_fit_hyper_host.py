"""
HyperStudy.fitMany / ChangepointStudy.fitMany without a GPU.

The admission rule and the memory plan of series fits in groups (blhip_set_series_groups) through a stand-alone host program around
blhip_series.hpp (tests/host/series_group_main.cpp) and through ctypes (blhip_host_series_group_check / _plan: host-only, no context).

fitMany itself on the oracle-backed engine, where every call runs the loop, and on a double of the grouped device path built from the
oracle (one oracle hyper-fit per series behind fit_series_groups): the books HyperSeriesFits keeps per series, ChangepointStudy's mask
and re-weighting, the padding of ragged series, batches -- all equal to the user's loop; the study is left as it was.
"""
import ctypes as C
import dataclasses
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.core import Study
from bayesloop_amd.engine import FitResult
from oracle_engine import OracleEngine
from recording_engine import RecordingEngine
from test_series_fit_host import plan, problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the host-only plan: tests/host/series_group_main.cpp ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def group_program(tmp_path_factory):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    exe = str(tmp_path_factory.mktemp('series_group') / 'series_group')
    src = os.path.join(ROOT, 'tests', 'host', 'series_group_main.cpp')
    subprocess.run([hipcc, '-std=c++17', '--offload-arch=gfx950', src, '-o', exe], check=True, capture_output=True, text=True, timeout=300)

    def run(T, n, H, S, evidence_only=False, budget=1e13, cap=0, ndim=1):
        out = subprocess.run([exe] + [str(v) for v in (T, n, H, S, int(evidence_only), repr(float(budget)), cap, ndim)], check=True,
                             capture_output=True, text=True).stdout.splitlines()
        head, body, why = out[0].split(' | ')
        w = body.split()
        res = dict(check=int(head.split()[1]), rc=int(w[1]), groups=int(w[3]), batches=int(w[5]), bytes=int(w[7]), least=int(w[9]), chain=int(w[11]), why=why)
        if len(out) > 1:
            res['series_plan'] = [int(v) for v in out[1].split()[1:]]
        return res
    return run


def chain_bytes(T, n, evidence_only):
    """a chain of a series fit, restated: state ping-pong, the stored sequence unless evidence-only, the partial sums, its likelihood table"""
    return ((2 if evidence_only else T + 2) * n * 8) + T * 7 * 8 * 2 * 64 + T * n * 8


def group_bytes(T, n, H, evidence_only):
    """a group: H such chains, less the H - 1 tables they do not own, plus -- a fit that keeps posteriors -- one (T, n) average"""
    return H * chain_bytes(T, n, evidence_only) - (H - 1) * T * n * 8 + (0 if evidence_only else T * n * 8)


@pytest.mark.parametrize('evidence_only', [False, True], ids=['full', 'evidenceOnly'])
def test_group_plan_counts_whole_groups(group_program, evidence_only):
    T, n = 110, 200
    for H in (2, 3, 20, 100, 4096):
        least = group_bytes(T, n, H, evidence_only)
        for S in (1, 2, 7, 512, 5000):
            for budget in (least, 3 * least + 5, 1e13):
                r = group_program(T, n, H, S, evidence_only, budget)
                assert r['check'] == 0 and r['rc'] == 0 and r['why'] == '', r
                assert r['chain'] == chain_bytes(T, n, evidence_only) and r['least'] == least
                # whole groups, at most 4096 chains, inside the budget, no batch smaller than those allow, every series once
                assert r['groups'] == min(S, 4096 // H, int(budget // least)) >= 1
                assert r['groups'] * H <= 4096 and r['bytes'] == r['groups'] * least <= budget
                assert (r['batches'] - 1) * r['groups'] < S <= r['batches'] * r['groups']


def test_group_plan_cap_and_refusals(group_program):
    T, n = 110, 200
    # the caller's cap (option max_batch) in chains: 2 + 2 + 1 groups of 3 under a cap of 6, 7 or 8
    for cap in (6, 7, 8):
        r = group_program(T, n, 3, 5, cap=cap)
        assert (r['rc'], r['groups'], r['batches']) == (0, 2, 3)
    assert group_program(T, n, 3, 5, cap=100000)['groups'] == 5            # (never beyond the library's own cap)
    assert group_program(T, n, 3, 5000, cap=100000)['groups'] == 4096 // 3
    # a group beyond the cap or the budget: refused with the reason, the smallest budget still reported
    r = group_program(T, n, 3, 5, cap=2)
    assert r['rc'] == 1 and r['groups'] == 0 and r['least'] == group_bytes(T, n, 3, False) and 'beyond the batch cap of 2 chains' in r['why']
    r = group_program(T, n, 3, 5, budget=group_bytes(T, n, 3, False) - 1)
    assert r['rc'] == 1 and r['groups'] == 0 and r['least'] == group_bytes(T, n, 3, False) and 'below one group of 3 chains' in r['why']
    r = group_program(T, n, 4097, 5)
    assert r['check'] == 1 and r['rc'] == -1 and 'groups of 4097 chains' in r['why']
    r = group_program(10, 20, 3, 5, ndim=2)
    assert r['check'] == 1 and r['rc'] == -1 and 'one-parameter grids' in r['why']


@pytest.mark.parametrize('evidence_only', [False, True], ids=['full', 'evidenceOnly'])
def test_groups_of_one_are_the_series_plan(group_program, evidence_only):
    T, n = 110, 200
    for S in (1, 7, 4096, 10000):
        for budget in (chain_bytes(T, n, evidence_only), 64 * chain_bytes(T, n, evidence_only) + 3, 1e13):
            r = group_program(T, n, 1, S, evidence_only, budget)
            assert r['check'] == 0 and r['series_plan'][0] == 0
            assert [r['rc'], r['groups'], r['batches'], r['bytes'], r['least']] == r['series_plan']
    r = group_program(T, n, 1, 5, evidence_only, chain_bytes(T, n, evidence_only) - 1)
    assert r['rc'] == 1 == r['series_plan'][0] and r['least'] == chain_bytes(T, n, evidence_only)


# ---- the same two functions as the library exports them ------------------------------------------------------------------------------------------
def group_check(p, S, H, flags=0):
    err = C.create_string_buffer(400)
    rc = _abi.load().blhip_host_series_group_check(C.byref(p), S, H, flags, err, 400)
    return rc, err.value.decode()


def group_plan(p, S, H, flags, budget, cap=0):
    out, err = (C.c_int64 * 4)(), C.create_string_buffer(400)
    rc = _abi.load().blhip_host_series_group_plan(C.byref(p), S, H, flags, float(budget), cap, out, err, 400)
    return rc, [int(v) for v in out], err.value.decode()


def test_exported_check_and_plan():
    T, n = 110, 200
    p, keep = problem(T=T, n=(n,))
    fold = _abi.KEEP_POSTERIOR | _abi.ACCUMULATE
    assert group_check(p, 8, 3, fold) == (0, '') and group_check(p, 8, 3, fold | _abi.FORWARD_ONLY) == (0, '')
    assert group_check(p, 8, 3, _abi.EVIDENCE_ONLY | _abi.SERIES_RAGGED) == (0, '')
    # groups of one are blhip_set_series: its rules and messages, the refusal of the flag included
    rc, why = group_check(p, 8, 1, fold)
    assert rc == 1 and 'BLHIP_ACCUMULATE' in why
    assert group_check(p, 8, 1, 0) == (0, '')
    for flags, word in ((fold | _abi.RESUME, 'BLHIP_RESUME'), (_abi.CARRY | _abi.EVIDENCE_ONLY, 'BLHIP_CARRY')):
        rc, why = group_check(p, 8, 3, flags)
        assert rc == 1 and word in why
    assert group_check(p, 8, 0, 0)[0] == 1
    p2, keep2 = problem(ops=((_abi.OP_GRW, 0), (_abi.OP_CHANGEPOINT, 0)))
    assert group_check(p2, 8, 3, fold)[0] == 0
    rc, why = group_check(p2, 8, 3, fold | _abi.SERIES_RAGGED)
    assert rc == 1 and 'depends on the time stamp' in why
    p3, keep3 = problem(n=(128, 16), om=_abi.OM_GAUSSIAN)
    assert group_check(p3, 8, 3, fold)[0] == 1 and group_check(p3, 8, 1, 0)[0] == 0        # (two-parameter grids: single chains only)
    rc, out, why = group_plan(p, 512, 20, fold, 1e13)
    assert rc == 0 and out == [204, 3, 204 * group_bytes(T, n, 20, False), group_bytes(T, n, 20, False)] and why == ''
    rc, out, why = group_plan(p, 5, 3, fold, 1e13, cap=2)
    assert rc == 1 and out[0] == 0 and 'cap of 2' in why
    for S in (5, 5000):
        assert group_plan(p, S, 1, 0, 1e13)[:2] == plan(p, S, 0, 1e13)
    assert group_plan(p3, 5, 3, fold, 1e13)[0] == -1


# ---- fitMany: the loop on the oracle-backed engine, and a double of the grouped device path -----------------------------------------------------
class GroupedOracle(OracleEngine):
    """OracleEngine + the three methods HyperStudy.fitMany asks a device engine for.  fit_series_groups: per series one oracle fit of its
    H chains folded into the oracle's accumulator, finalised -- what the grouped fold leaves on the device."""
    series_group_fits = True

    def __init__(self):
        super(GroupedOracle, self).__init__()
        self.options, self.calls, self._avg = {}, [], None

    def series_group_check(self, problem, n_series, n_group, flags=0):
        self.calls.append(('check', n_series, n_group, flags))
        return None

    def series_group_plan(self, problem, n_series, n_group, evidence_only=False):
        cap = int(self.options.get('max_batch', 4096))
        if n_group > cap:
            return 0, 'a group of %d chains is beyond the batch cap of %d chains (option max_batch)' % (n_group, cap)
        return min(n_series, cap // n_group), None

    def fit_series_groups(self, problem, series, n_group, op_values, forward_only=False, evidence_only=False, keep_posterior=False,
                          accumulate=False, log_chain_weight=None, owner=None):
        if self._posterior_owner is not None and self._posterior_owner is not owner:
            prev, self._posterior_owner = self._posterior_owner, None
            prev._materialize_posterior()
        S, H, T, G = len(series), n_group, problem.T, problem.G
        if self.options.get('refuse_memory') and keep_posterior:         # (the library's words: chains_per_batch, blhip_batch.hpp)
            raise bl.BackendError('BLHIP_KEEP_POSTERIOR: %d chains do not fit in device memory at once' % (S * H))
        assert len(op_values) == S * H and (evidence_only or (accumulate and keep_posterior and len(log_chain_weight) == S * H))
        self.calls.append(('fit', S, H))
        logE, local, astep, aphase = [], [], [], []
        means, self._avg = np.full((S, len(problem.marginal), T), np.nan), np.full((S, T, G), np.nan)
        for s in range(S):
            p = dataclasses.replace(problem, data=np.asarray(series[s], dtype=float).reshape(np.shape(problem.data)))
            self.acc_log, self.acc_lin, self.acc_shape = np.zeros((T, G)) - np.inf, None, (T, G)
            r = OracleEngine.fit(self, p, op_values[s * H:(s + 1) * H], forward_only=forward_only, evidence_only=evidence_only,
                                 accumulate=not evidence_only, log_chain_weight=None if evidence_only else log_chain_weight[s * H:(s + 1) * H])
            logE.append(r.log_evidence), local.append(r.local_evidence), astep.append(r.abort_step), aphase.append(r.abort_phase)
            if not evidence_only and np.isfinite(np.amax(self.acc_log)):
                means[s] = self.accum_finalize(p)
                self._avg[s] = self.acc_final
        if keep_posterior and not evidence_only:
            self._posterior_owner = owner
        return FitResult(np.concatenate(logE), np.concatenate(local), None if evidence_only else means, np.concatenate(astep),
                         np.concatenate(aphase), {})

    def posterior(self, chain, T, grid_size, t0=0, t1=None):
        if self._avg is not None:
            return self._avg[chain].reshape([T] + list(grid_size))[t0:t1]
        return super(GroupedOracle, self).posterior(chain, T, grid_size, t0, t1)

    def marginal(self, source, chain, keep_axis, T, n_keep):
        if self._avg is not None and source == 0:
            post = self._avg[chain].reshape([T] + self._gs)
            axes = tuple(a + 1 for a in range(len(self._gs)) if a != keep_axis)
            return post.sum(axis=axes) if axes else post.copy()
        return super(GroupedOracle, self).marginal(source, chain, keep_axis, T, n_keep)

    def fit(self, *args, **kw):
        if self._posterior_owner is not None and self._posterior_owner is not kw.get('owner'):
            prev, self._posterior_owner = self._posterior_owner, None
            prev._materialize_posterior()              # (the averages of a grouped fit: read before they go)
        self._avg = None
        return super(GroupedOracle, self).fit(*args, **kw)


@pytest.fixture(params=['loop', 'grouped'])
def engine(request):
    eng = OracleEngine() if request.param == 'loop' else GroupedOracle()
    prev = bl.set_engine(eng)
    Study._series_loop_announced = frozenset()
    yield eng
    bl.set_engine(prev)


def walk_study():
    S = bl.HyperStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)), bl.tm.GaussianRandomWalk('sigma', bl.cint(0, 0.6, 4), target='rate'), silent=True)
    return S


def two_hyper_study():
    S = bl.HyperStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)),
          bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('sigma', [0.1, 0.2, 0.4], target='rate', prior=[1., 2., 1.]),
                                        bl.tm.RegimeSwitch('log10pMin', [-7, -3])), silent=True)
    return S


def all_changepoints():
    S = bl.ChangepointStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)), bl.tm.ChangePoint('tc', 'all'), silent=True)
    return S


def two_changepoints():
    S = bl.ChangepointStudy(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)),
          bl.tm.CombinedTransitionModel(bl.tm.ChangePoint('t1', [2, 4, 6], prior=[1., 2., 3.]), bl.tm.ChangePoint('t2', [2, 4, 6])), silent=True)
    return S


def certain_study():
    S = bl.HyperStudy(silent=True)
    S.set(bl.om.Bernoulli('p', np.linspace(0.0, 1.0, 5), prior=np.array([1.0, 0.0, 0.0, 0.0, 1.0])),
          bl.tm.GaussianRandomWalk('sigma', [0., 0.3], target='p', prior=[1., 0.]), silent=True)
    return S


RNG = np.random.RandomState(7)
EQUAL = [RNG.poisson(2.0 + s, size=8).astype(float) for s in range(5)]
RAGGED = [RNG.poisson(2.0 + s, size=k).astype(float) for s, k in enumerate((7, 5, 6))]
RAGGED[0][2] = np.nan
CERTAIN = [np.array([1.0, 1.0, 1.0]), np.array([1.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0])]
GRID_ATTRS = ('hyperGridValues', 'hyperGridConstant', 'flatHyperPriorValues', 'allHyperGridValues', 'allHyperPriorValues', 'mask')


def loop(make, series, stamps=None, **kw):
    """what the user's loop leaves on a fresh hyper-study, series by series"""
    out = []
    for s, d in enumerate(series):
        S = make()
        S.loadData(d, timestamps=None if stamps is None else stamps[s], silent=True)
        with np.errstate(all='ignore'):
            S.fit(silent=True, **kw)
        out.append(S)
    return out


def same(R, want, exact):
    """exact: the loop itself ran (every entry bit for bit); else the double of the device path -- the same oracle chains, folded by the
    same oracle function, the books kept by HyperSeriesFits: a few ulps where they were summed in another order"""
    eq = (lambda a, b: np.array_equal(a, b, equal_nan=True)) if exact else (lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-300, equal_nan=True))
    assert isinstance(R, bl.HyperSeriesFits) and len(R) == len(want)
    for s, W in enumerate(want):
        assert eq(R.logEvidence[s], W.logEvidence) and eq(R.localEvidence[s], W.localEvidence)
        assert np.array_equal(R.logEvidenceList[s], np.array(W.logEvidenceList, dtype=float))
        assert (R.hyperParameterDistribution[s] is None) == (W.hyperParameterDistribution is None)
        if W.hyperParameterDistribution is not None:
            assert np.shape(R.hyperParameterDistribution[s]) == np.shape(W.hyperParameterDistribution)
            assert eq(R.hyperParameterDistribution[s], W.hyperParameterDistribution)
        assert np.array_equal(R.formattedTimestamps[s], W.formattedTimestamps)
        if not R.evidenceOnly:
            post = R.averagePosteriorSequence(s)
            assert np.shape(post) == np.shape(W.posteriorSequence) and eq(post, W.posteriorSequence)
            assert eq(R.posteriorMeanValues[s], W.posteriorMeanValues)
        T1 = R.study(s)
        assert type(T1) is type(W) and np.array_equal(T1.rawData, W.rawData, equal_nan=True)
        for a in GRID_ATTRS:
            if hasattr(W, a):
                assert eq(np.asarray(getattr(T1, a), dtype=float), np.asarray(getattr(W, a), dtype=float)), a


@pytest.mark.parametrize('kw', [{}, dict(forwardOnly=True), dict(evidenceOnly=True)], ids=['full', 'forwardOnly', 'evidenceOnly'])
@pytest.mark.parametrize('make, series', [(walk_study, EQUAL), (walk_study, RAGGED), (two_hyper_study, EQUAL), (all_changepoints, EQUAL),
                                          (two_changepoints, EQUAL), (certain_study, CERTAIN)],
                         ids=['walk', 'walk_ragged', 'two_hyper', 'tc_all', 'two_cp', 'certain'])
def test_fitmany_equals_the_loop(engine, make, series, kw):
    S = make()
    S.loadData(series[-1], silent=True)
    before = [np.array(v) for v in S._unpackAllHyperParameters()]
    R = S.fitMany(series, silent=True, **kw)
    want = loop(make, series, **kw)
    same(R, want, exact=isinstance(engine, OracleEngine) and not isinstance(engine, GroupedOracle))
    if isinstance(engine, GroupedOracle):
        assert [c for c in engine.calls if c[0] == 'fit'] == [('fit', len(series), len(want[0].hyperGridValues))]      # ONE call
    # the study is left as it was
    assert np.array_equal(S.rawData, series[-1], equal_nan=True) and S.hyperParameterDistribution is None and S.logEvidenceList == []
    assert all(np.array_equal(a, b) for a, b in zip(before, S._unpackAllHyperParameters()))
    if make is two_hyper_study:
        x, y, joint = R.getJointHyperParameterDistribution(1, ['sigma', 'log10pMin'])
        x0, y0, joint0 = want[1].getJointHyperParameterDistribution(['sigma', 'log10pMin'])
        assert np.array_equal(x, x0) and np.array_equal(y, y0) and np.allclose(joint, joint0, rtol=1e-12, atol=0)
    if make is two_changepoints:
        assert len(R.hyperParameterDistribution[0]) == 9 and int(np.sum(R.study(0).mask)) == 3 and len(R.logEvidenceList[0]) == 3
        d1, p1 = R.study(2).getDurationDistribution(['t1', 't2'])
        d0, p0 = want[2].getDurationDistribution(['t1', 't2'])
        assert np.array_equal(d1, d0) and np.allclose(p1, p0, rtol=1e-12, atol=0)
    if make is walk_study:
        v, d = R.getHyperParameterDistribution(0, 'sigma')
        v0, d0 = want[0].getHyperParameterDistribution('sigma')
        assert np.array_equal(v, v0) and np.allclose(d, d0, rtol=1e-12, atol=0)
    if make is certain_study:
        assert R.logEvidence[1] == -np.inf and np.all(np.isnan(R.hyperParameterDistribution[1]))
        if not kw.get('evidenceOnly'):
            assert np.all(np.isnan(R.averagePosteriorSequence(1)))


def test_batches_of_whole_groups_and_pickling():
    eng = GroupedOracle()
    prev = bl.set_engine(eng)
    try:
        eng.options['max_batch'] = 9                      # H = 4: two groups per batch
        S = walk_study()
        R = S.fitMany(EQUAL, silent=True)
        assert [c for c in eng.calls if c[0] == 'fit'] == [('fit', 2, 4), ('fit', 2, 4), ('fit', 1, 4)]
        assert R._device is not None and R._device[1:3] == (4, 1)
        want = loop(walk_study, EQUAL)
        same(R, want, exact=False)
        values, dist = R.getParameterDistributions(4, 'rate')                # (while on the device; series 1 was copied out before)
        assert np.allclose(dist * S.latticeConstant[0], want[4].posteriorSequence, rtol=1e-12)
        R2 = pickle.loads(pickle.dumps(R))
        assert R._device is None and R2._device is None
        same(R2, want, exact=False)
        v2, d2 = R2.getParameterDistributions(4, 'rate')
        assert np.array_equal(values, v2) and np.allclose(dist, d2, rtol=1e-13)
    finally:
        bl.set_engine(prev)


def test_calls_that_take_the_loop_say_why_once(capsys):
    eng = GroupedOracle()
    prev = bl.set_engine(eng)
    try:
        for setup, word in ((lambda: eng.options.update(series_fit=0), 'option series_fit is 0'),
                            (lambda: eng.options.update(series_fit=1, max_batch=3), 'a group of 4 chains is beyond the batch cap of 3'),
                            (lambda: eng.options.update(max_batch=4096), None)):
            setup()
            Study._series_loop_announced = frozenset()
            capsys.readouterr()
            R = walk_study().fitMany(EQUAL, silent=True)
            R = walk_study().fitMany(EQUAL[:3], silent=True)
            err = capsys.readouterr().err
            if word is None:
                assert err == ''
            else:
                assert err.count('fitMany runs the loop over HyperStudy.fit') == 1 and word in err, err
            same(R, loop(walk_study, EQUAL[:3]), exact=word is not None)
        Study._series_loop_announced = frozenset()
        walk_study().fitMany(EQUAL[:1], silent=True)
        assert 'fewer than 2 series' in capsys.readouterr().err
    finally:
        bl.set_engine(prev)


def test_one_hyper_grid_point_and_plain_studies_keep_their_calls():
    """at most one hyper-grid point: Study.fitMany's path with that point's values.  Study.fitMany of a plain Study: a SeriesFits, and the
    same calls into the engine as before -- one fit per series on an engine without series fits."""
    def one_point():
        S = bl.HyperStudy(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)), bl.tm.GaussianRandomWalk('sigma', [0.3], target='rate'), silent=True)
        return S

    def plain():
        S = bl.Study(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)), bl.tm.GaussianRandomWalk('sigma', 0.3, target='rate'), silent=True)
        return S
    eng = RecordingEngine(OracleEngine())
    prev = bl.set_engine(eng)
    try:
        St = one_point()
        R = St.fitMany(EQUAL[:3], silent=True)
        assert isinstance(R, bl.HyperSeriesFits) and R.hyperParameterDistribution == [None] * 3
        assert St.transitionModel.hyperParameterValues[0] == [0.3]
        hyper_calls = [line.split('(')[0] for line in eng.trace]
        same(R, loop(one_point, EQUAL[:3]), exact=True)
        del eng.trace[:]
        P = plain().fitMany(EQUAL[:3], silent=True)
        assert type(P) is bl.SeriesFits
        plain_calls = [line.split('(')[0] for line in eng.trace]
        assert plain_calls.count('fit') == 3 and not [c for c in plain_calls if 'series' in c or 'accum' in c], plain_calls
        assert [c for c in hyper_calls if c == 'fit'] == ['fit'] * 3 and not [c for c in hyper_calls if 'accum' in c], hyper_calls
        for s in range(3):
            assert P.logEvidence[s] == R.logEvidence[s] and np.array_equal(P.posteriorSequence(s), R.posteriorSequence(s))
    finally:
        bl.set_engine(prev)


def test_a_batch_the_fit_itself_finds_too_large_takes_the_loop(group_program, capsys):
    """The group plan shares a series' likelihood table among its H chains; the memory plan of the fit itself (chains_per_batch) counts
    every chain with a table of its own.  With a budget between the two figures the plan admits a group the fit refuses with
    'BLHIP_KEEP_POSTERIOR: ... do not fit in device memory at once': fitMany runs the loop and says so."""
    T, n, H = 110, 200, 20
    plan_needs, fit_needs = group_bytes(T, n, H, False), H * chain_bytes(T, n, False)
    assert plan_needs < fit_needs
    r = group_program(T, n, H, 5, budget=(plan_needs + fit_needs) // 2)
    assert r['rc'] == 0 and r['groups'] == 1                      # (admitted by the plan, one group per batch)
    eng = GroupedOracle()
    eng.options['refuse_memory'] = 1
    prev = bl.set_engine(eng)
    try:
        Study._series_loop_announced = frozenset()
        capsys.readouterr()
        R = walk_study().fitMany(EQUAL[:3], silent=True)
        err = capsys.readouterr().err
        assert err.count('fitMany runs the loop over HyperStudy.fit') == 1 and 'do not fit in device memory at once' in err, err
        same(R, loop(walk_study, EQUAL[:3]), exact=True)
        E = walk_study().fitMany(EQUAL[:3], evidenceOnly=True, silent=True)       # (keeps nothing: the library cuts its own batches)
        assert [c for c in eng.calls if c[0] == 'fit'] == [('fit', 3, 4)]
        same(E, loop(walk_study, EQUAL[:3], evidenceOnly=True), exact=False)
    finally:
        bl.set_engine(prev)


@pytest.mark.parametrize('which', ['loop', 'grouped'])
def test_one_combination_of_change_points_leaves_the_scattered_prior(which):
    """two change-points over [2, 4]^2: the mask keeps ONE of 4 combinations, so fit switches to Study.fit -- and still leaves
    flatHyperPriorValues scattered to the full grid; study(s) of fitMany holds the same"""
    def make():
        S = bl.ChangepointStudy(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, 20)),
              bl.tm.CombinedTransitionModel(bl.tm.ChangePoint('t1', [2, 4]), bl.tm.ChangePoint('t2', [2, 4])), silent=True)
        return S
    eng = OracleEngine() if which == 'loop' else GroupedOracle()
    prev = bl.set_engine(eng)
    try:
        R = make().fitMany(EQUAL[:3], silent=True)
        want = loop(make, EQUAL[:3])
        assert len(want[0].hyperGridValues) == 1 and len(want[0].flatHyperPriorValues) == 4 and want[0].hyperParameterDistribution is None
        same(R, want, exact=True)
        for s in range(3):
            assert np.array_equal(R.study(s).flatHyperPriorValues, want[s].flatHyperPriorValues)
    finally:
        bl.set_engine(prev)
