"""
bayesloop_amd/core.py with its problem builder (Study._likelihoodSource / _problem), the evidence book of a block as methods of the
online study (_bookModel / _bookAcross / _commitBooks) and the other shared helpers asks the engine for the work, and leaves every study
in the state, of the commit before them -- bit for bit.

Not-gpu half: every case runs over the CPU doubles (tests/oracle_engine.py, tests/online_block_engine.py) behind
tests/recording_engine.py.  Held against tests/golden/core_dedup_parent.npz, which tests/golden/gen_core_dedup_parent.py recorded with
the parent commit's package: the full trace of calls into the engine (one line per call: the method and a digest of the line with every
argument in it; the arrays of a FitProblem hashed field by field), everything the study printed, and the study's state -- the evidence
book of the online study (BOOK of tests/test_online_block_host.py), logEvidence, localEvidence, posteriorMeanValues,
hyperParameterDistribution, the raw series and both sets of time stamps in full, the grid-sized results (DIGESTED) by shape and SHA-256.
Numbers are held by their bytes: the sign of a zero and the sign and payload of a NaN included.

gpu half: the state comparison alone, on the device, against tests/golden/core_dedup_parent_gpu.npz (the parent's core.py over the same
library on an MI355X).  The library is the same build and the trace is held above: a difference there is a changed call, not arithmetic.

LEFT_OUT: cases on which the parent commit differs from itself between two recordings in two processes (none did).
"""
import contextlib
import dataclasses
import gc
import hashlib
import io
import json
import os
import pickle

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import likprogram_studies as ls
import plugin_models
from bayesloop_amd import _abi
from online_block_engine import BlockOracleEngine
from oracle_engine import OracleEngine
from recording_engine import RecordingEngine
from test_online_block_host import BOOK

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'core_dedup_parent.npz')
GOLDEN_GPU = os.path.join(HERE, 'golden', 'core_dedup_parent_gpu.npz')

STATE = BOOK + ('localEvidence', 'posteriorMeanValues', 'rawData', 'rawTimestamps', 'formattedTimestamps', 'firstStep', 'logEvidenceList',
                'fitWarningCounter')
DIGESTED = ('posteriorSequence', 'averagePosteriorSequence', 'marginalizedPosterior', 'parameterPosterior', 'transitionModelPosterior')
LEFT_OUT = ()


# ---- what is kept of a run ------------------------------------------------------------------------------------------------------------
def flat(v):
    if v is None:
        return np.zeros(0)
    if isinstance(v, (list, tuple)):
        return np.concatenate([flat(x) for x in v]) if len(v) else np.zeros(0)
    return np.asarray(v, dtype=np.float64).ravel()


def structure(v):
    if v is None:
        return 'None'
    if isinstance(v, (list, tuple)):
        return '[%s]' % ','.join(structure(x) for x in v)
    a = np.asarray(v)
    return '%s%s' % (a.dtype.str, 'x'.join(map(str, a.shape)))


def line_digest(line):
    return '%s %s' % (line.split('(', 1)[0], hashlib.sha256(line.encode()).hexdigest()[:12])


def snapshot(S, record):
    """Adds everything held of study S to the record: per attribute its structure and, in ``record['values']``, its numbers (DIGESTED: their
    SHA-256 in place of the numbers)"""
    held, values = [], []
    for key in STATE + DIGESTED:
        try:
            v = getattr(S, key)
        except AttributeError:
            continue
        f = np.ascontiguousarray(flat(v))
        if key in DIGESTED:
            held.append([key, structure(v), hashlib.sha256(f.tobytes()).hexdigest()])
        else:
            held.append([key, structure(v), len(f)])
            values.append(f)
    record['state'] = held
    record['values'] = np.concatenate(values) if values else np.zeros(0)
    return record


def packed(case, record):
    """-> the two arrays a case takes in the golden file: its numbers, and everything else as one JSON text"""
    values = record.pop('values')
    return {case + '/values': values, case + '/text': np.array(json.dumps(record, sort_keys=True))}


# ---- engines --------------------------------------------------------------------------------------------------------------------------
class ProgramDouble(OracleEngine):
    """Takes a likelihood program the way the HipEngine does; its arithmetic reads the table the model's own pdf gives instead."""
    lik_programs = True

    def fit(self, problem, op_values, **kw):
        if problem.lik_program is not None:
            problem = dataclasses.replace(problem, obs_model=_abi.OM_TABLE, lik=self.table, lik_program=None)
        return super().fit(problem, op_values, **kw)


class ScriptedAbort(OracleEngine):
    """Reports a zero normaliser in the given phase: at step 2 of a whole fit (Study.fit), at the first one-step fit of the backward pass or
    the third of the forward pass (Study._fitHostTransition)."""

    def __init__(self, phase):
        super().__init__()
        self.phase, self.n = phase, 0

    def fit(self, problem, op_values, **kw):
        res = super().fit(problem, op_values, **kw)
        self.n += 1
        whole = problem.T > 1
        backward = getattr(problem, 'backward_init', None) is not None
        if whole or (backward if self.phase == 1 else self.n == 3):
            res.abort_step[0], res.abort_phase[0] = (2 if whole else 0), self.phase
        return res


# ---- cases: name -> (engine factory, function that runs the case and returns its study) -----------------------------------------------
def feed_step(S, data):
    for d in data:
        S.step(d)


def feed_many(S, data):
    S.stepMany(np.array(data))


def feed_split(S, data):
    S.BLOCK_MIN_POINTS = 1                  # (blocks of any length, also the one- and two-point pieces)
    k = max(1, len(data) // 3)
    S.stepMany(np.array(data[:k]))
    S.step(data[k])
    S.stepMany(np.array(data[k + 1:]))


def feed_chunks(S, data):
    S.BLOCK_MIN_POINTS = 1
    S.stepMany(np.array(data))


def feed_pickled(S, data):
    """a pickle round trip in mid-stream: block, pickle, step, pickle, block"""
    k = len(data) // 2
    S.stepMany(np.array(data[:k]))
    S = pickle.loads(pickle.dumps(S))
    S.step(data[k])
    S = pickle.loads(pickle.dumps(S))
    S.stepMany(np.array(data[k + 1:]))
    return S


FEEDS = dict(step=feed_step, many=feed_many, split=feed_split, chunks2=feed_chunks, pickled=feed_pickled)


def online(case, feeding, history):
    def run():
        S = cases.build_online(bl, case, storeHistory=history)
        return FEEDS[feeding](S, cases.online_data(cases.ONLINE_CASES[case])) or S
    return run


def dead_chain(feeding):
    """the study of test_a_chunk_with_a_dead_chain_is_repeated_through_step"""
    def run():
        S = bl.OnlineStudy(storeHistory=True, silent=True)
        p = np.zeros(11)
        p[0], p[10] = 0.5, 0.5
        S.setOM(bl.om.Bernoulli('p', bl.cint(0.0, 1.0, 11), prior=p), silent=True)
        S.addTransitionModel('static', bl.tm.Static())
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', [0.05, 0.2], target='p'))
        FEEDS[feeding](S, np.array([1, 1, 0, 1, 1, 0]))
        return S
    return run


def waiting():
    """test_empty_block_is_a_no_op_and_messages_come_once: a point that waits in a call of its own, then a block"""
    S = cases.build_online(bl, 'online_ar1_wait')
    S.stepMany(np.array([]))
    S.stepMany(np.array([1]))
    S.stepMany(np.array([0, 1, 0, 0, 1]))
    S.stepMany(np.array([]))
    return S


def list_fed(history):
    """step takes a point as a list too: every entry joins the raw series, the call takes ONE time stamp (reference core.py:2095-2096)"""
    def run():
        S = bl.OnlineStudy(storeHistory=history, silent=True)
        S.setOM(bl.om.Poisson('rate', bl.oint(0, 6, 40)), silent=True)
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', [0.1, 0.3], target='rate'))
        for point in ([1, 2], [3, 4], [2, 2], [3], 1):
            S.step(point)
        return S
    return run


def multi_dimensional(feeding):
    """the study of test_multi_dimensional_data_block: a data point is a 1-D array"""
    def run():
        S = bl.OnlineStudy(storeHistory=True, silent=True)
        S.setOM(bl.om.Gaussian('mean', bl.cint(-3, 3, 24), 'std', bl.oint(0, 3, 20)), silent=True)
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', [0.1, 0.3], target='mean'))
        FEEDS[feeding](S, np.random.default_rng(3).normal(0.5, 1.0, (6, 2)))
        return S
    return run


def cp_drift(feeding, history):
    """the change-point + Deterministic study of tests/test_online_block_host.py"""
    def run():
        from test_online_block_host import cp_drift_study
        S = cp_drift_study(history)
        FEEDS[feeding](S, np.array([2, 3, 1, 4, 6, 5]))
        return S
    return run


def _numpy_likelihood(data, mu, s):
    return np.exp(-np.abs(data - mu) / s) / (2. * s) + 1e-3 * (mu > 5.)


def fit_study(which, **kw):
    def run():
        if which == 'table':
            S = bl.Study()
            S.loadData(cases.series(31, 9))
            S.set(bl.om.NumPy(_numpy_likelihood, 'mu', bl.cint(-4, 4, 17), 's', bl.oint(0, 3, 9)), bl.tm.GaussianRandomWalk('w', 0.3, target='mu'))
        elif which == 'program':
            S = ls.normal_study(bl, sizes=(12, 5), T=6)
            S._formatData()
            bl.get_engine().table = np.array([S.observationModel.processedPdf(S.grid, seg) for seg in S.formattedData])
        else:
            S = cases.build(bl, which)
        S.fit(**kw)
        if kw.get('evidenceOnly'):
            S.fit()                        # ... and a pending posterior that an evidence-only fit has to bring to the host first
            S.fit(**kw)
        return S
    return run


def hyper_fit(case):
    def run():
        S = cases.build(bl, case)
        S.fit(**dict(cases.CASES[case].get('fit', {})))
        return S
    return run


def plugin(name):
    def run():
        S, kw = plugin_models.studies(bl, plugin_models.make(bl.tm))[name]
        S.fit(**kw)
        return S
    return run


def plugin_abort():
    S, kw = plugin_models.studies(bl, plugin_models.make(bl.tm))['leaky_poisson_full']
    S.loadData(plugin_models.COAL[:8], silent=True)
    S.fit()
    return S


def plugin_no_chain():
    """a hyper-study over a user-defined walk to which no chain contributes (tests/test_fold_recovery.py)"""
    S = cases.build(bl, dict(study='HyperStudy', data=np.array([0.2, 0.1, 500.0, 0.3, -0.1]),
                             om=('Gaussian', [('mean', ('cint', -2, 2, 32)), ('std', ('oint', 0, 0.5, 32))], 'default'),
                             tm=('GRW', 'sigma', [0.05, 0.1, 0.2], 'mean', None)))
    S.set(plugin_models.make(bl.tm)['LeakyRandomWalk']('sigma', [0.05, 0.1, 0.2], 'leak', 0.0, target='mean'))
    S.fit()
    return S


MODES = dict(full={}, forward=dict(forwardOnly=True), evidence=dict(evidenceOnly=True))
PLUGINS = ('leaky_poisson_full', 'leaky_poisson_fwdonly', 'leaky_poisson_evid', 'cooling_poisson_full', 'combined_gauss_full',
           'capped_gauss_full', 'serial_poisson_full', 'leaky_hyper_evid', 'leaky_hyper_full', 'leaky_hyper_fwdonly', 'combined_gauss_hyper_full')

CASES = {}
for _c in cases.ONLINE_CASES:
    for _h in (True, False):
        for _f in ('step', 'many', 'split'):
            CASES['%s-%s-%s' % (_c, _f, 'history' if _h else 'current')] = (BlockOracleEngine, online(_c, _f, _h))
    CASES['%s-chunks2-history' % _c] = (lambda: BlockOracleEngine(chunk_steps=2), online(_c, 'chunks2', True))
CASES['online_poisson_3tm-chunks2-current'] = (lambda: BlockOracleEngine(chunk_steps=2), online('online_poisson_3tm', 'chunks2', False))
for _c in ('online_poisson_3tm', 'online_gauss2d'):
    for _h in (True, False):
        CASES['%s-pickled-%s' % (_c, 'history' if _h else 'current')] = (BlockOracleEngine, online(_c, 'pickled', _h))
CASES['dead_chain-step'] = (BlockOracleEngine, dead_chain('step'))
CASES['dead_chain-chunks2'] = (lambda: BlockOracleEngine(chunk_steps=2), dead_chain('chunks2'))
CASES['waiting'] = (BlockOracleEngine, waiting)
CASES['list_fed-history'] = (BlockOracleEngine, list_fed(True))
CASES['list_fed-current'] = (BlockOracleEngine, list_fed(False))
CASES['multi_dimensional-step'] = (BlockOracleEngine, multi_dimensional('step'))
CASES['multi_dimensional-split'] = (BlockOracleEngine, multi_dimensional('split'))
for _h in (True, False):
    for _f in ('step', 'many'):
        CASES['cp_drift-%s-%s' % (_f, 'history' if _h else 'current')] = (BlockOracleEngine, cp_drift(_f, _h))
for _m, _kw in MODES.items():
    CASES['fit-builtin-' + _m] = (OracleEngine, fit_study('kat_changepoint', **_kw))
    CASES['fit-table-' + _m] = (OracleEngine, fit_study('table', **_kw))
    CASES['fit-program-' + _m] = (ProgramDouble, fit_study('program', **_kw))
CASES['fit-independent-full'] = (OracleEngine, fit_study('kat_independent'))
CASES['fit-abort-forward'] = (OracleEngine, fit_study('abort_forward'))
for _p in (0, 1):
    CASES['fit-abort-scripted-phase%d' % _p] = (lambda p=_p: ScriptedAbort(p), fit_study('kat_grw'))
    CASES['fit-abort-scripted-phase%d-evidence' % _p] = (lambda p=_p: ScriptedAbort(p), fit_study('kat_grw', evidenceOnly=True))
    CASES['plugin-abort-phase%d' % _p] = (lambda p=_p: ScriptedAbort(p), plugin_abort)
for _c in ('kat_hyper_0hp', 'kat_hyper_1hp', 'kat_changepointstudy'):
    CASES['hyper-' + _c] = (OracleEngine, hyper_fit(_c))
for _n in PLUGINS:
    CASES['plugin-' + _n] = (OracleEngine, plugin(_n))
CASES['plugin-no_chain'] = (OracleEngine, plugin_no_chain)

GPU_CASES = {}
for _c in ('online_kat_2tm', 'online_poisson_3tm'):
    for _h in (True, False):
        for _f in ('step', 'many'):
            GPU_CASES['%s-%s-%s' % (_c, _f, 'history' if _h else 'current')] = online(_c, _f, _h)
GPU_CASES['plugin-cooling_poisson_full'] = plugin('cooling_poisson_full')
GPU_CASES['hyper-kat_hyper_1hp'] = hyper_fit('kat_hyper_1hp')


def collect(case):
    """Runs a not-gpu case behind a recording engine -> ({'<case>/<key>': array}, the trace's full lines)"""
    make_engine, run = CASES[case]
    # An online study gives its carry slots back when it is collected (OnlineStudy.__del__), through whatever engine is installed then, and
    # a study and its transition model refer to each other: the collector decides when.  Studies of earlier tests go now, none goes
    # while the case runs, and the case's own go before its engine does.
    gc.collect()
    gc.disable()
    counted = bl.OnlineStudy._slot_counter[0]
    bl.OnlineStudy._slot_counter[0] = 0              # (carry slots are part of the calls: count them from the same start in every case)
    rec = RecordingEngine(make_engine())
    prev = bl.set_engine(rec)
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text), np.errstate(all='ignore'):
            S = run()
        lines = list(rec.trace)
        out = dict(trace=[line_digest(x) for x in lines], stdout=text.getvalue())
        with np.errstate(all='ignore'):
            snapshot(S, out)
        del S
        gc.collect()
    finally:
        gc.enable()
        bl.set_engine(prev)
        bl.OnlineStudy._slot_counter[0] = max(counted, bl.OnlineStudy._slot_counter[0])
    return packed(case, out), lines


def collect_gpu(case):
    """Runs a gpu case on the engine in place -> {'<case>/<key>': array}"""
    text = io.StringIO()
    with contextlib.redirect_stdout(text), np.errstate(all='ignore'):
        S = GPU_CASES[case]()
        out = snapshot(S, dict(stdout=text.getvalue()))
    return packed(case, out)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def hold(got, golden, case, lines=None):
    assert case + '/text' in golden.files, 'no recording of %s' % case
    g, w = json.loads(str(got[case + '/text'])), json.loads(str(golden[case + '/text']))
    gt, wt = g.pop('trace', []), w.pop('trace', [])
    if gt != wt:
        n = next((i for i, (x, y) in enumerate(zip(gt, wt)) if x != y), min(len(gt), len(wt)))
        pytest.fail('%s: %d calls into the engine (the parent: %d); the first that differs is call %d: the parent made "%s", this is\n%s'
                    % (case, len(gt), len(wt), n, wt[n] if n < len(wt) else '(none)', lines[n] if n < len(lines) else '(none)'))
    assert g['stdout'] == w['stdout']
    assert g['state'] == w['state']                     # (which attributes, their structure, the digests of the grid-sized ones)
    gv, wv, at = got[case + '/values'], golden[case + '/values'], 0
    for key, _, n in g['state']:
        if isinstance(n, int):
            assert same(gv[at:at + n], wv[at:at + n]), '%s of %s: %r != %r' % (key, case, gv[at:at + n], wv[at:at + n])
            at += n
    assert at == len(gv) == len(wv)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('case', [c for c in CASES if c not in LEFT_OUT])
def test_calls_and_state_are_the_parents(case, golden):
    got, lines = collect(case)
    hold(got, golden, case, lines)


def test_every_recorded_case_is_held(golden):
    assert sorted(set(k.split('/')[0] for k in golden.files)) == sorted(CASES) and len(LEFT_OUT) <= 1


@pytest.mark.parametrize('case', list(cases.ONLINE_CASES) + ['cp_drift'])
def test_one_step_op_values_do_not_depend_on_the_time_stamp(case):
    """step's programs used to be compiled at time stamp 0 and a block's at -1; both come from OnlineStudy._compileModel at -1 now.  With
    one step and the transition into it evaluated at ``resume_time``, no op value reads the stamp: the values at 0 are those at -1."""
    from test_online_block_host import cp_drift_study
    with contextlib.redirect_stdout(io.StringIO()):
        S = cp_drift_study(True) if case == 'cp_drift' else cases.build_online(bl, case)
        if S.tmCount is None:
            S.addTransitionModel('transition model', S.transitionModel)
    for tm, hpv in zip(S.transitionModels, S.hyperParameterValues):
        S.setTransitionModel(tm, silent=True)
        program, _, values = S._compileModel(tm, hpv, 1)
        at_zero = S._opValueMatrix(program, np.asarray(hpv, dtype=float) if len(hpv) > 0 else np.zeros((1, 0)), timestamps=[0.0], resume_time=-1.0)
        assert same(values, at_zero)


@pytest.fixture(scope='module')
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(GPU_CASES))
def test_state_on_the_device_is_the_parents(case, hip_engine):
    golden = np.load(GOLDEN_GPU)
    assert sorted(set(k.split('/')[0] for k in golden.files)) == sorted(GPU_CASES)
    hold(collect_gpu(case), golden, case)
