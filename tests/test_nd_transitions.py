"""
NotEqual, Independent, Serial and Deterministic transition models on grids with three and four parameters, on the GPU: the plain N-D
path (bayesloop_amd/csrc/blhip_nd.hpp) with the renormalising stages of blhip_nd_stages.hpp -- bln::ne_max_kernel, ne_invert_kernel,
ne_clamp_kernel, shift_axis_kernel.  Cases: tests/nd_transition_cases.py.

Every comparison is compare.check at compare.GPU_TOL (log-evidence 1e-9 relative, posteriors |dp| <= 1e-12 + 1e-9 p); the cases with
a Deterministic model carry the registered FFT_FLOOR (tolerances.FFT_TOL: 1e-15 absolute, inside the bar).  Plain studies keep their
posteriors on the device (BLHIP_KEEP_POSTERIOR), hyper-studies fold them (BLHIP_ACCUMULATE), OnlineStudy and the plug-in calls resume
and carry (BLHIP_RESUME | BLHIP_CARRY); forwardOnly / evidenceOnly variants are among the cases.
"""
import contextlib
import io
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import nd_transition_cases as ndc
import oracle_adapter as oa
from oracle import bl_oracle as orc

pytest.importorskip('scipy.stats')
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def result_of(S, c):
    res = dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence)
    if not c.get('fit', {}).get('evidenceOnly', False) and np.isfinite(S.logEvidence):
        res['posteriorSequence'] = S.posteriorSequence
        res['posteriorMeanValues'] = S.posteriorMeanValues
    for key in ('logEvidenceList', 'hyperParameterDistribution', 'hyperGridValues', 'mask'):
        if hasattr(S, key) and getattr(S, key) is not None and len(np.atleast_1d(getattr(S, key))) > 0:
            res[key] = np.asarray(getattr(S, key))
    return res


def gold_of(want, got):
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution', 'mask'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    return gold


def fit_case(c):
    S = cases.build(bl, c)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
    assert S.lastTiming['fwd_kernel_variant'] == 7, S.lastTiming
    return S


_ORACLE = {}


def oracle_of(case):
    """the oracle's result of a case, computed once per session"""
    if case not in _ORACLE:
        with np.errstate(all='ignore'):
            _ORACLE[case] = oa.run(ndc.ND[case])
    return _ORACLE[case]


def check_marginals(S, post):
    """marginal distributions of every parameter against the (average) posterior sequence `post`"""
    post = np.asarray(post)
    for k, name in enumerate(S.observationModel.parameterNames):
        axes = tuple(a + 1 for a in range(post.ndim - 1) if a != k)
        np.testing.assert_allclose(S.getParameterDistributions(name, density=False)[1], post.sum(axis=axes), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('case', sorted(ndc.ND))
def test_case_matches_the_oracle(case):
    c = ndc.ND[case]
    S = fit_case(c)
    want = oracle_of(case)
    got = result_of(S, c)
    gold = gold_of(want, got)
    compare.check(got, gold, compare.GPU_TOL, case_tol=c.get('tol'))
    if 'posteriorSequence' in gold:
        check_marginals(S, want['posteriorSequence'])


@pytest.mark.parametrize('case', ndc.GOLDEN)
def test_case_matches_the_references_fixture(case):
    c = ndc.ND[case]
    S = fit_case(c)
    compare.check(result_of(S, c), oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


def run_online(c):
    S = cases.build_online(bl, c)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        for d in cases.online_data(c):
            S.step(d)
    return S


def check_online(S, want):
    """want: oracle_adapter.run_online's dict, or a fixture of gen_golden.run_online (per-model arrays under numbered keys)."""
    tol = compare.GPU_TOL
    rt, at = tol['post_rtol'], tol['post_atol']
    gl = float(want['logEvidence'])
    assert abs(S.logEvidence - gl) <= tol['logE_rtol'] * abs(gl), (S.logEvidence, gl)
    for key in ('posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence'):
        np.testing.assert_allclose(np.asarray(getattr(S, key)), np.asarray(want[key]), rtol=rt, atol=at, err_msg=key)
    for i in range(len(S.transitionModels)):
        if 'hyperParameterSequence' in want:
            hs, pp, le = [h[i] for h in want['hyperParameterSequence']], want['parameterPosterior'][i], want['logEvidenceList'][i]
        else:
            hs, pp, le = want['hyperParameterSequence%d' % i], want['parameterPosterior%d' % i], want['logEvidenceList%d' % i]
        np.testing.assert_allclose(np.asarray([h[i] for h in S.hyperParameterSequence]), np.asarray(hs), rtol=rt, atol=at)
        np.testing.assert_allclose(np.asarray(S.parameterPosterior[i]), np.asarray(pp), rtol=rt, atol=at, err_msg='parameterPosterior %d' % i)
        np.testing.assert_allclose(np.asarray(S.logEvidenceList[i]), np.asarray(le), rtol=tol['logE_rtol'])


@pytest.mark.parametrize('case', sorted(ndc.ONLINE))
def test_online_study_step_by_step(case):
    c = ndc.ONLINE[case]
    with np.errstate(all='ignore'):
        want = oa.run_online(c)
    S = run_online(c)
    check_online(S, want)                       # (the sequences hold every step's result)
    if case in ndc.GOLDEN_ONLINE:
        check_online(S, oa.load_golden(case))


# ---- one step of every admitted model through the plug-in calls (transitionModels.py:49-63) -----------------------------------------

def _up(t, slope=0.25):
    return slope * t


def _down(t, slope=-0.4):
    return slope * t


def _flat(t, slope=0.0):
    return slope * t


def _det(fn, target):
    """(model factory, oracle ops, oracle values) of a Deterministic model with the scalar default `slope` of fn"""
    import inspect
    slope = inspect.getfullargspec(fn).defaults[0]
    names = ['df', 'loc', 'scale']
    return (lambda: bl.tm.Deterministic(fn, target=target)), [('deterministic', names.index(target), -1, 0, fn, ['slope'])], [slope]


def _spec(spec):
    ops, vals, _ = oa.flatten_tm(spec, ['df', 'loc', 'scale'])
    return (lambda: cases.make_tm(bl, spec)), ops, orc.align_values(ops, vals)


ONE_STEP = {
    'notequal': _spec(('NE', 'p', -2.5, None)),
    'notequal_low_limit': _spec(('NE', 'p', -6., None)),
    'independent': _spec(('Independent',)),
    'walk': _spec(('GRW', 's', 0.5, 'loc', None)),
    'changepoint': _spec(('ChangePoint', 'tc', 2, None)),
    'combined': _spec(('Combined', [('GRW', 's', 0.3, 'scale', None), ('NE', 'p', -3., None)])),
    'serial': _spec(('Serial', [('GRW', 's', 0.3, 'loc', None), ('BreakPoint', 'tb', 3, None), ('NE', 'p', -3., None)])),
    'shift_positive_first_axis': _det(_up, 'df'),
    'shift_negative_middle_axis': _det(_down, 'loc'),
    'shift_positive_last_axis': _det(_up, 'scale'),
    'shift_zero': _det(_flat, 'loc'),
}


def _inputs(shape):
    rng = np.random.default_rng(7)
    x = rng.uniform(0.1, 1.0, shape)                      # positive, sum != 1
    z = rng.uniform(0.1, 1.0, shape)
    z[rng.uniform(size=shape) < 0.3] = 0.0                 # exact zeros
    twice = rng.uniform(0.1, 1.0, shape)
    twice.flat[17] = twice.flat[1003] = 2.0                # the maximum is attained twice (in two different blocks)
    return dict(positive=x, zeros=z, maximum_twice=twice)


@pytest.mark.parametrize('name', sorted(ONE_STEP))
def test_one_step_of_a_model_through_the_plug_in_calls(name):
    make, ops, values = ONE_STEP[name]
    S = bl.Study(silent=True)
    S.loadData(cases.make_data(('series', 130, 6)), silent=True)
    model = make()
    S.set(cases.make_om(bl, ndc.t3()), model, silent=True)
    g = orc.Grid([np.asarray(m) for m in S.marginalGrid])
    reset = orc.changepoint_prior(g, None)
    indep = reset / np.prod(g.lattice)
    for kind, x in _inputs(tuple(S.gridSize)).items():
        for t in (2, 3):                                   # (a restart / the break-point lie at these time stamps)
            with np.errstate(all='ignore'):
                want_f = orc.transition_forward(ops, values, x.copy(), t, g, reset, indep)
                want_b = orc.transition_backward(ops, values, x.copy(), t, g, reset, indep)
            got_f = np.asarray(model.computeForwardPrior(x.copy(), t), dtype=float)
            got_b = np.asarray(model.computeBackwardPrior(x.copy(), t), dtype=float)
            for got, want, what in ((got_f, want_f, 'forward'), (got_b, want_b, 'backward')):
                assert got.shape == want.shape
                err = np.abs(got - want) - (compare.GPU_TOL['post_atol'] + compare.GPU_TOL['post_rtol'] * np.abs(want))
                assert err.max() <= 0, (name, kind, t, what, float(np.abs(got - want).max()))


def test_regimeswitch_keeps_refusing_the_plug_in_call():
    S = cases.build(bl, dict(study='Study', data=('series', 130, 6), om=ndc.t3(), tm=('Static',)))
    model = bl.tm.RegimeSwitch('p', -3)
    model.study = S
    with pytest.raises(NotImplementedError):
        model.computeForwardPrior(np.ones(S.gridSize), 2)


# ---- batches ------------------------------------------------------------------------------------------------------------------

def test_a_split_batch_gives_the_results_of_one_batch():
    """The 8 chains of the break-point study in batches of 3 + 3 + 2: per chain nothing depends on its neighbours in the batch
    (identical log-evidences); the folded results keep the bar against the oracle."""
    c = ndc.ND['ndt_breakpoints']
    one = fit_case(c)
    assert one.lastTiming['batches'] == 1, one.lastTiming
    eng = bl.get_engine()
    eng.set_option('max_batch', 3)
    try:
        split = fit_case(c)
        assert split.lastTiming['batches'] == 3, split.lastTiming
    finally:
        eng.set_option('max_batch', 1024)
    assert np.array_equal(np.asarray(split.logEvidenceList), np.asarray(one.logEvidenceList))
    got = result_of(split, c)
    compare.check(got, gold_of(oracle_of('ndt_breakpoints'), got), compare.GPU_TOL)
    np.testing.assert_allclose(np.asarray(split.posteriorSequence), np.asarray(one.posteriorSequence), rtol=1e-12, atol=1e-15)


def _steep(t, slope=6.0):
    return slope * t


def test_a_shift_of_more_than_12_cells_is_refused_and_the_engine_goes_on():
    """slope 6 per step on the loc axis (lattice 6 / 17): 17 cells per step.  The library refuses before any launch; the next fit on
    the same engine succeeds."""
    S = bl.Study(silent=True)
    S.loadData(cases.make_data(('series', 131, 6)), silent=True)
    S.set(cases.make_om(bl, ndc.t3()), bl.tm.Deterministic(_steep, target='loc'), silent=True)
    with pytest.raises(bl.exceptions.BackendError, match='shifts by .* grid cells'):
        S.fit(silent=True)
    c = ndc.ND['ndt_shift_last']
    T = fit_case(c)
    got = result_of(T, c)
    compare.check(got, gold_of(oracle_of('ndt_shift_last'), got), compare.GPU_TOL, case_tol=c.get('tol'))


# ---- the existing N-D cases are unchanged ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['nd3_changepoint_then_walk', 'nd3_hyper_two'])
def test_existing_cases_are_bit_identical_to_the_parent_commit(case):
    """tests/golden/nd_parent_results.npz: the results of these two cases from a build of the commit before the stages existed, on the
    same hardware.  A batch without the new ops launches the kernels it launched then, with the same arguments."""
    from test_gpu_parity import ND_CASES
    parent = np.load(os.path.join(HERE, 'golden', 'nd_parent_results.npz'))
    S = fit_case(ND_CASES[case])
    for key in ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        assert np.array_equal(np.asarray(getattr(S, key), dtype=float), parent['%s/%s' % (case, key)]), key
