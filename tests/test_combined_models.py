"""
Composed CombinedTransitionModel programs on the MI355X: transitions that do not fit into one step of the generic kernel run as stage
lists -- blk::step_kernel in its stage modes in front of the fused step kernel (DESIGN.md "Composed transitions").  The fixtures of
tests/combined_cases.py through the HIP library, at the bars of tests/test_combined_models_oracle.py (compare.GPU_TOL; FFT_FLOOR for the
Deterministic / AlphaStable cases); each composed case asserts through the kernel census that the stage kernel ran, the single-stage
control that it did not.  (Without stage lists every composed case is refused at fit time with a BackendError.)
"""
import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import combined_cases as cc
import compare
import oracle_adapter as oa
from conftest import kernel_census
from test_combined_models_oracle import result_of, fit_case, run_online, check_online

pytestmark = pytest.mark.gpu

STAGE_FWD, STAGE_BWD = 'blk::step_kernel<100, 2, false>', 'blk::step_kernel<100, 3, false>'


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def _counts():
    return {name: c for c, name in kernel_census()}


def _ran(before, after):
    return {k for k in after if after[k] > before.get(k, 0)}


def expected_stages(c):
    fit = c.get('fit', {})
    return [STAGE_FWD] if (fit.get('evidenceOnly') or fit.get('forwardOnly')) else [STAGE_FWD, STAGE_BWD]


@pytest.mark.parametrize('case', sorted(cc.COMBINED))
def test_composed_program_matches_reference(case):
    c = cc.COMBINED[case]
    before = _counts()
    S = fit_case(c)
    got = result_of(S, c)
    ran = _ran(before, _counts())
    if c.get('single_stage'):
        assert STAGE_FWD not in ran and STAGE_BWD not in ran, sorted(ran)
    else:
        missing = [k for k in expected_stages(c) if k not in ran]
        assert not missing, 'stage kernel(s) not launched: %s; launched: %s' % (missing, sorted(ran))
    compare.check(got, oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', sorted(cc.SINGLE_STAGE))
def test_single_stage_program_launches_no_stage_kernel(case):
    c = cc.SINGLE_STAGE[case]
    before = _counts()
    S = fit_case(c)
    got = result_of(S, c)
    ran = _ran(before, _counts())
    assert STAGE_FWD not in ran and STAGE_BWD not in ran, sorted(ran)
    compare.check(got, oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('k', range(len(cc.TUTORIAL_LOG10)))
def test_tutorial_evidence_matches_the_published_values(k):
    """docs/source/tutorials/hyperparameteroptimization.ipynb: S.optimize(['slope_2']) prints these log10-evidences."""
    v, log10 = cc.TUTORIAL_LOG10[k]
    case = 'comb_tutorial_evidence_%d' % k
    c = cc.COMBINED[case]
    S = fit_case(c)
    gold = oa.load_golden(case)
    assert abs(S.logEvidence - float(gold['logEvidence'])) <= compare.GPU_TOL['logE_rtol'] * abs(float(gold['logEvidence']))
    np.testing.assert_almost_equal(S.logEvidence / np.log(10), log10, decimal=5)


def test_tutorial_model_through_the_user_interface():
    """The tutorial's second model as a user writes it (loadExampleData, lambdas), evidence-only at slope_2 = -0.046875."""
    S = bl.Study(silent=True)
    S.loadExampleData(silent=True)
    S.set(bl.om.Poisson('accident_rate', bl.oint(0, 6, 1000)), silent=True)
    T = bl.tm.SerialTransitionModel(
        bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('early_sigma', 0.05, target='accident_rate'), bl.tm.RegimeSwitch('pmin', -7)),
        bl.tm.BreakPoint('first_break', 1885),
        bl.tm.Deterministic(lambda t, slope_1=-0.2: slope_1 * t, target='accident_rate'),
        bl.tm.BreakPoint('second_break', 1895),
        bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('late_sigma', 0.25, target='accident_rate'),
                                      bl.tm.Deterministic(lambda t, slope_2=-0.046875: slope_2 * t, target='accident_rate')))
    S.set(T, silent=True)
    S.fit(evidenceOnly=True, silent=True)
    gold = float(oa.load_golden('comb_tutorial_evidence_6')['logEvidence'])
    assert abs(S.logEvidence - gold) <= compare.GPU_TOL['logE_rtol'] * abs(gold)


@pytest.mark.parametrize('case', sorted(cc.ONLINE))
def test_composed_model_in_online_study(case):
    before = _counts()
    S = run_online(cc.ONLINE[case])
    ran = _ran(before, _counts())
    assert STAGE_FWD in ran, sorted(ran)
    gold = oa.load_golden(case)
    check_online(S, gold, int(gold['n_models']))
