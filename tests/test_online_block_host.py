"""OnlineStudy.stepMany without a GPU: the host side of a block (raw-series bookkeeping, block programs, the evidence bookkeeping vectorised
over time, time chunks, the repeat of a chunk with a dead chain) over the block test double (tests/online_block_engine.py), and the
time-chunk planner through the C-ABI and a stand-alone program."""
import contextlib
import io
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import cases
import oracle_adapter as oa
import bayesloop_amd as bl
from bayesloop_amd.engine import HipEngine
from online_block_engine import BlockOracleEngine
from test_online import ATOL, check_online, reference_accessor_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOK = ('logEvidenceList', 'hyperLogEvidenceList', 'hyperParameterDistribution', 'transitionModelDistribution',
        'localTransitionModelDistribution', 'logEvidence', 'hyperParameterSequence', 'transitionModelSequence', 'localTransitionModelSequence')


@contextlib.contextmanager
def block_engine(**kw):
    prev = bl.engine._engine
    eng = BlockOracleEngine(**kw)
    bl.set_engine(eng)
    try:
        yield eng
    finally:
        bl.set_engine(prev)


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        fn(*a)
    return out.getvalue()


def feed_loop(S, data):
    for d in data:
        S.step(d)


def results(S):
    return dict(logEvidence=S.logEvidence, posteriorSequence=S.posteriorSequence, posteriorMeanValues=S.posteriorMeanValues,
                transitionModelSequence=S.transitionModelSequence, localTransitionModelSequence=S.localTransitionModelSequence,
                hyperParameterSequence=S.hyperParameterSequence, parameterPosterior=S.parameterPosterior, logEvidenceList=S.logEvidenceList)


def flat(v):
    if isinstance(v, (list, tuple)):
        return np.concatenate([flat(x) for x in v]) if len(v) else np.zeros(0)
    return np.asarray(v, dtype=float).ravel()


def assert_same_bookkeeping(S, W):
    """bit for bit: the bookkeeping is host arithmetic on the local evidences, and those are the same numbers in both runs"""
    for key in BOOK:
        assert np.array_equal(flat(getattr(S, key)), flat(getattr(W, key)), equal_nan=True), key
    assert np.array_equal(np.asarray(S.rawData), np.asarray(W.rawData), equal_nan=True) and np.asarray(S.rawData).dtype == np.asarray(W.rawData).dtype
    assert np.array_equal(S.rawTimestamps, W.rawTimestamps) and list(S.formattedTimestamps) == list(W.formattedTimestamps)
    assert S.firstStep == W.firstStep


def assert_same_state(S, W, rtol=1e-12):
    assert_same_bookkeeping(S, W)
    np.testing.assert_allclose(S.marginalizedPosterior, W.marginalizedPosterior, rtol=rtol, atol=1e-300)
    for a, b in zip(S.parameterPosterior, W.parameterPosterior):
        np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-300)
    np.testing.assert_allclose(flat(S.posteriorSequence), flat(W.posteriorSequence), rtol=rtol, atol=1e-300)
    # (means are signed sums that can cancel to ~0 on a symmetric grid: test_online.py's absolute bar)
    np.testing.assert_allclose(flat(S.posteriorMeanValues), flat(W.posteriorMeanValues), rtol=rtol, atol=ATOL)
    assert len(S.posteriorSequence) == len(W.posteriorSequence) == len(S.hyperParameterSequence)


def feed_all(S, data):
    S.stepMany(np.array(data))


def feed_split(S, data):
    k = max(1, len(data) // 3)
    S.stepMany(np.array(data[:k]))
    S.step(data[k])
    S.stepMany(np.array(data[k + 1:]))


@pytest.mark.parametrize('feeding', ['all', 'split', 'chunks_of_2'])
@pytest.mark.parametrize('case', list(cases.ONLINE_CASES))
def test_step_many_over_the_block_double_matches_golden_and_loop(case, feeding):
    data = cases.online_data(cases.ONLINE_CASES[case])
    with block_engine(chunk_steps=2 if feeding == 'chunks_of_2' else None) as eng:
        W = cases.build_online(bl, case)
        quiet(feed_loop, W, data)
        S = cases.build_online(bl, case)
        S.BLOCK_MIN_POINTS = 1                  # (blocks of any length, also the one- and two-point pieces of the split feeding)
        quiet(feed_split if feeding == 'split' else feed_all, S, data)
        if feeding == 'chunks_of_2':
            assert max(f[0] for f in eng.block_fits) == 2
        gold = oa.load_golden(case)
        check_online(results(S), gold, int(gold['n_models']))
        reference_accessor_checks(S, case)
        assert_same_state(S, W)


def drift(t, slope=0.3):
    return slope * t


def cp_drift_study(history=True):
    S = bl.OnlineStudy(storeHistory=history, silent=True)
    S.setOM(bl.om.Poisson('rate', bl.oint(0, 8, 90)), silent=True)
    S.addTransitionModel('cp', bl.tm.ChangePoint('tc', [1, 3]))
    S.addTransitionModel('drift', bl.tm.Deterministic(drift, target='rate'))
    return S


@pytest.mark.parametrize('history', [True, False])
def test_block_evaluates_every_transition_at_time_stamp_minus_one(history):
    """A ChangePoint at 1 and 3 -- inside the block's index range -- must not restart anything, a Deterministic drift must shift by the same
    amount at every step: a block that used the real time stamps differs from the loop here."""
    data = np.array([2, 3, 1, 4, 6, 5])
    with block_engine():
        with contextlib.redirect_stdout(io.StringIO()):
            W, S = cp_drift_study(history), cp_drift_study(history)
            feed_loop(W, data)
            S.stepMany(data)
        assert_same_state(S, W)


def test_option_online_block_0_is_the_loop():
    data = cases.online_data(cases.ONLINE_CASES['online_kat_2tm'])
    with block_engine() as eng:
        eng.set_option('online_block', 0)
        S = cases.build_online(bl, 'online_kat_2tm')
        quiet(S.stepMany, np.array(data))
        assert [f[0] for f in eng.block_fits] == [1] * (2 * len(data))          # one-step fits only: step's
        W = cases.build_online(bl, 'online_kat_2tm')
        quiet(feed_loop, W, data)
        assert_same_state(S, W, rtol=0)
        # ... and so is a call with fewer points to filter than a block is worth (OnlineStudy.BLOCK_MIN_POINTS), whatever the option says
        eng.set_option('online_block', 1)
        del eng.block_fits[:]
        S = cases.build_online(bl, 'online_kat_2tm')
        quiet(S.stepMany, np.array(data[:3]))
        assert [f[0] for f in eng.block_fits] == [1] * 6
        quiet(S.stepMany, np.array(data[3:] + data))
        assert [f[0] for f in eng.block_fits[6:]] == [7, 7]


def test_empty_block_is_a_no_op_and_messages_come_once():
    with block_engine():
        S = cases.build_online(bl, 'online_ar1_wait')
        assert quiet(S.stepMany, np.array([])) == '' and len(S.rawData) == 0 and S.firstStep
        out = quiet(S.stepMany, np.array([1]))                                  # one point in front of a full segment: it waits
        assert out.count('Will wait for more data') == 1 and S.firstStep and len(S.rawData) == 1
        out = quiet(S.stepMany, np.array([0, 1, 0, 0, 1]))
        assert 'Will wait' not in out and out.count('flat transition model prior') == 1 and not S.firstStep
        quiet(S.stepMany, np.array([]))
        assert len(S.posteriorSequence) == 5
        S2 = cases.build_online(bl, 'online_ar1_wait')
        out = quiet(S2.stepMany, np.array([1, 0, 1, 0, 0, 1]))                  # waiting and filtering in ONE call
        assert out.count('Will wait for more data') == 1 and out.count('Start model fit') == 1
        assert_same_state(S2, S)


def test_multi_dimensional_data_block():
    rng = np.random.default_rng(3)
    data = rng.normal(0.5, 1.0, (6, 2))

    def make():
        S = bl.OnlineStudy(storeHistory=True, silent=True)
        S.setOM(bl.om.Gaussian('mean', bl.cint(-3, 3, 24), 'std', bl.oint(0, 3, 20)), silent=True)
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', [0.1, 0.3], target='mean'))
        return S
    with block_engine(), contextlib.redirect_stdout(io.StringIO()):
        W, S = make(), make()
        feed_loop(W, data)
        S.stepMany(data[:4])
        S.stepMany(data[4:])
        assert S.rawData.shape == (6, 2)
        assert_same_state(S, W)


def test_user_defined_transition_model_is_refused_as_in_step():
    import plugin_models
    models = plugin_models.make(bl.tm)

    def make(cls):
        S = bl.OnlineStudy(silent=True)
        S.setOM(bl.om.Poisson('rate', bl.oint(0, 6, 50)), silent=True)
        S.addTransitionModel('user', cls('s', [0.1, 0.2], target='rate') if cls is models['CappedRandomWalk']
                             else cls('a', 0.2, 'b', 0.1, target='rate'))
        return S
    with block_engine() as eng, contextlib.redirect_stdout(io.StringIO()):
        for cls in models.values():
            with pytest.raises(bl.exceptions.ConfigurationError) as e_step:
                make(cls).step(2)
            with pytest.raises(bl.exceptions.ConfigurationError) as e_many:
                make(cls).stepMany(np.array([2, 3, 1]))
            assert str(e_step.value) == str(e_many.value)
        assert eng.block_fits == []


def test_pickle_round_trip_after_step_many_then_one_more_step():
    data = cases.online_data(cases.ONLINE_CASES['online_poisson_3tm'])
    with block_engine():
        W = cases.build_online(bl, 'online_poisson_3tm')
        quiet(feed_loop, W, data)
        S = cases.build_online(bl, 'online_poisson_3tm')
        quiet(S.stepMany, np.array(data[:-1]))
        S2 = pickle.loads(pickle.dumps(S))
        assert S2._backupSlots == [] and set(S2._slots).isdisjoint(S._slots)
        quiet(S2.step, data[-1])
        assert_same_state(S2, W)


def test_a_chunk_with_a_dead_chain_is_repeated_through_step():
    """A prior without mass where the likelihood of the third datum survives (Static model): that chain's normaliser is zero.  The chunk is
    repeated point by point from the states carried into it: NaN pattern and all, the study ends where the loop ends."""
    data = np.array([1, 1, 0, 1, 1, 0])

    def study():
        S = bl.OnlineStudy(storeHistory=True, silent=True)
        p = np.zeros(11)
        p[0], p[10] = 0.5, 0.5               # mass on p = 0 and p = 1 only: a 1 kills the first, a 0 after it the second
        S.setOM(bl.om.Bernoulli('p', bl.cint(0.0, 1.0, 11), prior=p), silent=True)
        S.addTransitionModel('static', bl.tm.Static())
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', [0.05, 0.2], target='p'))
        return S
    with block_engine(chunk_steps=2) as eng, contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        W, S = study(), study()
        feed_loop(W, data)
        n_loop = len(eng.block_fits)
        S.stepMany(data)
        fits = eng.block_fits[n_loop:]
        assert any(f[0] == 2 for f in fits) and any(f[0] == 1 for f in fits)       # blocks, and the repeat through step
        assert not np.all(np.isfinite(flat(W.logEvidenceList)))                    # (the construction does kill a chain)
        assert_same_state(S, W)


@pytest.mark.parametrize('C', [1, 2, 7, 64, 200])
def test_vectorised_bookkeeping_is_bit_identical_for_identical_local_evidences(C):
    """The bookkeeping of a block from (chains, N) local evidences against step's, which sees them one column at a time."""
    rng = np.random.default_rng(C)
    N = 9
    local = [np.exp(rng.normal(-2, 3, (c, N))) for c in (C, 3)]
    local[1][1, 4:] = 0.0                    # a dead chain among live ones: -inf evidences from there on

    class Scripted(BlockOracleEngine):
        def fit(self, problem, op_values, **kw):
            res = super().fit(problem, op_values, **kw)
            i = 0 if len(op_values) == C and self._calls % 2 == 0 else 1
            self._calls += 1
            t0 = self._t[i]
            self._t[i] += problem.T
            res.local_evidence[:] = local[i][:, t0:t0 + problem.T]
            res.abort_step[:] = -1
            return res

    def study():
        S = bl.OnlineStudy(storeHistory=True, silent=True)
        S.setOM(bl.om.Poisson('rate', bl.oint(0, 6, 12)), silent=True)
        S.addTransitionModel('a', bl.tm.GaussianRandomWalk('s', np.linspace(0.05, 0.5, C).tolist() if C > 1 else 0.1, target='rate'))
        S.addTransitionModel('b', bl.tm.GaussianRandomWalk('q', [0.1, 0.2, 0.3], target='rate'))
        return S
    out = []
    for block in (False, True):
        eng = Scripted()
        eng._calls, eng._t = 0, [0, 0]
        prev = bl.engine._engine
        bl.set_engine(eng)
        try:
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
                S = study()
                if block:
                    S.stepMany(np.arange(N) % 4)
                else:
                    feed_loop(S, np.arange(N) % 4)
            out.append(S)
        finally:
            bl.set_engine(prev)
    assert_same_bookkeeping(out[1], out[0])


# ---- the time-chunk planner ---------------------------------------------------------------------------------------------------------
def plan(grid, chains, planes, N, budget):
    return HipEngine.online_block_plan(grid, chains, planes, N, budget)


@pytest.mark.parametrize('grid,chains,planes', [([1000], 64, 3), ([256, 256], 32, 1), ([5, 18, 14], 16, 4), ([200], 4, 0)])
def test_block_planner_through_the_abi(grid, chains, planes):
    N = 1000
    one = plan(grid, chains, planes, N, 1e30)
    assert one['steps'] == N and one['n_chunks'] == 1
    floor = one['min_budget_bytes']
    assert plan(grid, chains, planes, N, floor - 1) is None                       # below one step: an error
    last = 0
    for budget in np.linspace(floor, one['chunk_bytes'] * 1.01, 23):
        p = plan(grid, chains, planes, N, float(budget))
        assert p is not None and 1 <= p['steps'] <= N and p['steps'] >= last      # monotone in the budget
        assert p['chunk_bytes'] <= budget                                         # the chunk fits
        if p['steps'] < N:
            more = plan(grid, chains, planes, p['steps'] + 1, 1e30)
            assert more['chunk_bytes'] > budget                                   # one more step does not
        assert p['n_chunks'] == -(-N // p['steps'])
        last = p['steps']
    assert last == N
    with pytest.raises(bl.exceptions.BackendError):
        plan(grid, 0, planes, N, 1e9)


@pytest.mark.parametrize('sanitize', [False, True])
def test_block_planner_stand_alone_program(tmp_path, sanitize):
    """tests/host/online_block_plan_main.cpp includes the planner's header and checks the same properties in C++; built plain and with
    the address / undefined-behaviour sanitizers (a stand-alone host program)."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    exe = str(tmp_path / 'online_block_plan')
    cmd = [hipcc, '-std=c++17', '--offload-arch=gfx950', os.path.join(ROOT, 'tests', 'host', 'online_block_plan_main.cpp'), '-o', exe]
    if sanitize:
        cmd += ['-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined', '-fsanitize=address,undefined']
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert run.returncode == 0 and 'online block plan: ok' in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    assert 'runtime error' not in run.stderr and 'AddressSanitizer' not in run.stderr
