"""
The fixtures of composed CombinedTransitionModel programs (tests/combined_cases.py, tests/golden/gen_combined_golden.py) against the
CPU oracle, through the product's host logic with the oracle test double as its engine (tests/oracle_engine.py).  These pass without
the device path too: they show that the fixtures are the reference's.  Bar: compare.GPU_TOL; the Deterministic / AlphaStable cases
also take the registered FFT_FLOOR (tests/tolerances.py).
"""
import contextlib
import io

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import combined_cases as cc
import compare
import oracle_adapter as oa
from oracle_engine import OracleEngine

ALL = dict(cc.COMBINED, **cc.SINGLE_STAGE)


@pytest.fixture(scope='module', autouse=True)
def oracle_engine():
    prev = bl.set_engine(OracleEngine())
    yield
    bl.set_engine(prev)


def result_of(S, c):
    res = dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence)
    if not c.get('fit', {}).get('evidenceOnly', False) and np.isfinite(S.logEvidence):
        res['posteriorSequence'] = S.posteriorSequence
        res['posteriorMeanValues'] = S.posteriorMeanValues
    for key in ('logEvidenceList', 'hyperParameterDistribution', 'hyperGridValues', 'mask'):
        if hasattr(S, key) and getattr(S, key) is not None and len(np.atleast_1d(getattr(S, key))) > 0:
            res[key] = np.asarray(getattr(S, key))
    return res


def fit_case(c):
    S = cases.build(bl, c)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
    return S


def run_online(c):
    S = cases.build_online(bl, c)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        for d in cases.online_data(c):
            S.step(d)
    return S


def check_online(S, gold, n_models, rtol=compare.GPU_TOL['post_rtol'], atol=compare.GPU_TOL['post_atol']):
    gl = float(gold['logEvidence'])
    assert abs(S.logEvidence - gl) <= compare.GPU_TOL['logE_rtol'] * abs(gl), (S.logEvidence, gl)
    for key in ('posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence'):
        np.testing.assert_allclose(np.asarray(getattr(S, key)), gold[key], rtol=rtol, atol=atol, err_msg=key)
    for i in range(n_models):
        np.testing.assert_allclose(np.asarray([h[i] for h in S.hyperParameterSequence]), gold['hyperParameterSequence%d' % i],
                                   rtol=rtol, atol=atol)
        np.testing.assert_allclose(np.asarray(S.parameterPosterior[i]), gold['parameterPosterior%d' % i], rtol=rtol, atol=atol)
        np.testing.assert_allclose(np.asarray(S.logEvidenceList[i]), gold['logEvidenceList%d' % i], rtol=compare.GPU_TOL['logE_rtol'])


@pytest.mark.parametrize('case', sorted(ALL))
def test_oracle_matches_combined_fixture(case):
    c = ALL[case]
    S = fit_case(c)
    compare.check(result_of(S, c), oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', sorted(cc.ONLINE))
def test_oracle_matches_combined_online_fixture(case):
    gold = oa.load_golden(case)
    check_online(run_online(cc.ONLINE[case]), gold, int(gold['n_models']))


def test_tutorial_fixtures_hold_the_published_evidences():
    """The fixtures of the tutorial's seven slope_2 values are the notebook's printed log10-evidences (5 decimals)."""
    for k, (v, log10) in enumerate(cc.TUTORIAL_LOG10):
        gold = oa.load_golden('comb_tutorial_evidence_%d' % k)
        assert round(float(gold['logEvidence']) / np.log(10), 5) == pytest.approx(log10, abs=1e-9), (v, gold['logEvidence'])
