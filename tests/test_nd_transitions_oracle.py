"""
NotEqual, Independent, Serial and Deterministic models on grids with three and four parameters (tests/nd_transition_cases.py) through
the product's host logic with the oracle test double as its engine (tests/oracle_engine.py): programs, expanded programs, op value
matrices, change-point masks and shift tables of these studies are what the CPU oracle fits; the fixtures the reference wrote
(tests/golden/gen_nd_transition_golden.py) agree with the oracle; the inputs of the NotEqual hyper-study reach all three clamp regimes;
the three models that stay refused on such grids are refused before any device work.
"""
import contextlib
import io

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import nd_transition_cases as ndc
import oracle_adapter as oa
from oracle_engine import OracleEngine

pytest.importorskip('scipy.stats')


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
    return S


def run_online(c):
    S = cases.build_online(bl, c)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        for d in cases.online_data(c):
            S.step(d)
    return S


def check_online(S, want, tol):
    """want: oracle_adapter.run_online's dict, or a fixture of gen_golden.run_online (per-model arrays under numbered keys)."""
    rt, at = tol['post_rtol'], tol['post_atol']
    gl = float(want['logEvidence'])
    assert abs(S.logEvidence - gl) <= tol['logE_rtol'] * abs(gl), (S.logEvidence, gl)
    for key in ('posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence'):
        np.testing.assert_allclose(np.asarray(getattr(S, key)), np.asarray(want[key]), rtol=rt, atol=at, err_msg=key)
    n = len(S.transitionModels)
    for i in range(n):
        if 'hyperParameterSequence' in want:
            hs, pp, le = [h[i] for h in want['hyperParameterSequence']], want['parameterPosterior'][i], want['logEvidenceList'][i]
        else:
            hs, pp, le = want['hyperParameterSequence%d' % i], want['parameterPosterior%d' % i], want['logEvidenceList%d' % i]
        np.testing.assert_allclose(np.asarray([h[i] for h in S.hyperParameterSequence]), np.asarray(hs), rtol=rt, atol=at)
        np.testing.assert_allclose(np.asarray(S.parameterPosterior[i]), np.asarray(pp), rtol=rt, atol=at)
        np.testing.assert_allclose(np.asarray(S.logEvidenceList[i]), np.asarray(le), rtol=tol['logE_rtol'])


@pytest.mark.parametrize('case', sorted(ndc.ND))
def test_host_logic_reproduces_the_oracle(case):
    c = ndc.ND[case]
    S = fit_case(c)
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    compare.check(got, gold_of(want, got), compare.ORACLE_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', sorted(ndc.ONLINE))
def test_online_host_logic_reproduces_the_oracle(case):
    c = ndc.ONLINE[case]
    with np.errstate(all='ignore'):
        want = oa.run_online(c)
    check_online(run_online(c), want, compare.ORACLE_TOL)


@pytest.mark.parametrize('case', ndc.GOLDEN)
def test_oracle_matches_the_references_fixture(case):
    c = ndc.ND[case]
    compare.check(result_of(fit_case(c), c), oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', ndc.GOLDEN_ONLINE)
def test_oracle_matches_the_references_online_fixture(case):
    check_online(run_online(ndc.ONLINE[case]), oa.load_golden(case), compare.GPU_TOL)


def test_notequal_hyper_study_reaches_all_three_clamp_regimes():
    """A condition on the INPUTS: per hyper-value, the share of cells NotEqual sets to its limit, from the oracle's own posteriors
    (transitionModels.py:465-469: out = max - p; out /= sum; out < 10**v dV).  One cell (the maximum only), part of the grid, all of it."""
    c = ndc.ND['ndt_notequal_hyper']
    S = cases.build(bl, c)
    dV = float(np.prod(S.latticeConstant))
    shares = []
    for v in ndc.NE_VALUES:
        single = dict(c, study='Study', tm=('NE', 'p_min', v, None))
        with np.errstate(all='ignore'):
            post = np.asarray(oa.run(single)['posteriorSequence'])
        clamped = total = 0
        for p in post[:-1]:                      # the forward transitions into steps 1 .. T-1 act on normalised posteriors
            out = np.amax(p) - p
            out /= np.sum(out)
            clamped += int((out < 10. ** v * dV).sum())
            total += out.size
        shares.append((clamped, total, len(post) - 1))
    (c0, n0, steps), (c1, n1, _), (c2, n2, _) = shares
    assert c0 == steps, shares                   # exactly one cell per step: the maximum
    assert 0.05 < c1 / n1 < 0.95, shares
    assert c2 == n2, shares


@pytest.mark.parametrize('model', sorted(ndc.REFUSED))
def test_models_that_stay_refused_on_three_parameter_grids(model):
    c = dict(study='Study', data=('series', 82, 6), om=ndc.t3(), tm=ndc.REFUSED[model])
    S = cases.build(bl, c)
    with pytest.raises(bl.exceptions.ConfigurationError):
        S.fit(silent=True)
    O = cases.build_online(bl, dict(om=ndc.t3(4, 8, 6), models=[('static', ('Static',)), ('refused', ndc.REFUSED[model])], data=[0.1]))
    with pytest.raises(bl.exceptions.ConfigurationError):
        with contextlib.redirect_stdout(io.StringIO()):
            O.step(0.1)
