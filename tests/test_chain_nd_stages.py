"""
The stage flavour of the chain-resident kernel on grids with three and four parameters (bayesloop_amd/csrc/blhip_chain_nd.hpp:
bln::chain_nd_stage_kernel<BWD, 256 | 1024>), on the GPU: batches with NotEqual and Deterministic models, resumed and carried fits
(OnlineStudy.stepMany).  Cases: tests/chain_nd_stage_cases.py.

Every comparison is compare.check at compare.GPU_TOL (log-evidence 1e-9 relative, posteriors |dp| <= 1e-12 + 1e-9 p, the NaN pattern of
localEvidence included; Deterministic cases carry the registered FFT_TOL) against the oracle.  Under chain_nd = 2 such a batch reports
fwd_ / bwd_kernel_variant 10 and ONE launch per pass; under chain_nd_stages = 0 it reports 7 and the plain path's launch per step.
"""
import contextlib
import io

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import chain_nd_stage_cases as cs
import compare
import oracle_adapter as oa
from test_chain_nd import check_marginals, gold_of, result_of
from test_online_block import assert_meets, quiet

pytest.importorskip('scipy.stats')
pytestmark = pytest.mark.gpu

_ORACLE = {}
DEFAULTS = dict(chain_nd=1, chain_nd_stages=1, max_batch=1024)


def oracle_of(case):
    """the oracle's result of a case, computed once per session"""
    if case not in _ORACLE:
        with np.errstate(all='ignore'):
            _ORACLE[case] = oa.run(cs.ALL[case])
    return _ORACLE[case]


@contextlib.contextmanager
def options(**kw):
    eng = bl.get_engine()
    try:
        for k, v in kw.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in kw:
            eng.set_option(k, DEFAULTS[k])


def fit(c, **opts):
    S = cases.build(bl, c)
    with options(**opts), contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
    return S


def check_route(S, c, variant, batches=1):
    lt = S.lastTiming
    fit_kw = c.get('fit', {})
    full = not (fit_kw.get('forwardOnly', False) or fit_kw.get('evidenceOnly', False))
    assert lt['batches'] == batches, lt
    assert lt['fwd_kernel_variant'] == variant and lt['bwd_kernel_variant'] == variant, lt
    T = len(cases.make_data(c['data']))
    per_pass = batches * (1 if variant == cs.VARIANT else T)
    assert lt['forward_launches'] == per_pass, lt
    assert lt['backward_launches'] == (per_pass if full else 0), lt


def check_oracle(S, case, c):
    got = result_of(S, c)
    want = oracle_of(case)
    gold = gold_of(want, got)
    compare.check(got, gold, compare.GPU_TOL, case_tol=c.get('tol'))
    return want, gold


@pytest.mark.parametrize('case', sorted(cs.ND))
def test_batch_of_sixteen_chains_with_stages_matches_the_oracle(case):
    """16 chains under chain_nd = 2: the kernel, one launch per pass, at the bar"""
    c = cs.ND[case]
    S = fit(c, chain_nd=2)
    assert len(S.logEvidenceList) == cs.CHAINS
    check_route(S, c, cs.VARIANT)
    want, gold = check_oracle(S, case, c)
    if 'posteriorSequence' in gold and c.get('store') != 'sparse':
        check_marginals(S, want['posteriorSequence'])


@pytest.mark.parametrize('case', sorted(cs.ND))
def test_option_chain_nd_stages_0_keeps_the_plain_path(case):
    """the same cases under chain_nd = 2, chain_nd_stages = 0: variant 7, one fused launch per step and pass, at the bar"""
    c = cs.ND[case]
    S = fit(c, chain_nd=2, chain_nd_stages=0)
    check_route(S, c, cs.PLAIN)
    check_oracle(S, case, c)


@pytest.mark.parametrize('case', sorted(cs.FORCED))
def test_single_study_with_stages_under_chain_nd_2(case):
    c = cs.FORCED[case]
    check_route(fit(c), c, cs.PLAIN)
    S = fit(c, chain_nd=2)
    check_route(S, c, cs.VARIANT)
    want, _ = check_oracle(S, case, c)
    check_marginals(S, want['posteriorSequence'])


def test_option_chain_nd_stages_is_known():
    eng = bl.get_engine()
    with options(chain_nd_stages=0):
        pass
    with pytest.raises(bl.exceptions.BackendError, match='unknown option'):
        eng.set_option('chain_nd_stage', 1)


def test_split_batches_with_stages():
    """35 chains, max_batch = 16: 16 + 16 + 3 chains in three resident batches give the results of one batch -- a chain's block depends on
    nothing but the chain: the log-evidences bit for bit"""
    c = cs.SPLIT
    one = fit(c, chain_nd=2)
    check_route(one, c, cs.VARIANT)
    assert len(one.logEvidenceList) == 35
    split = fit(c, chain_nd=2, max_batch=16)
    check_route(split, c, cs.VARIANT, batches=3)
    assert np.array_equal(np.asarray(split.logEvidenceList), np.asarray(one.logEvidenceList))
    check_oracle(one, 'cns_split', c)
    check_oracle(split, 'cns_split', c)


@pytest.mark.parametrize('history', [True, False])
def test_step_many_on_three_parameters_meets_the_loop(history):
    """a walk over 16 widths and NotEqual over 16 values: stepMany on 7 points leaves the study where the loop over step leaves it
    (tests/test_online_block.py's comparison and bar); the block's fits -- the first carried, the others of a second block resumed and
    carried -- take the kernel"""
    c = cs.ONLINE
    data = cases.online_data(c)
    eng = bl.get_engine()
    seen = []
    fit_fn = eng.fit

    def spy(*a, **kw):
        r = fit_fn(*a, **kw)
        seen.append((kw.get('resume', False), kw.get('carry', False), dict(r.timing)))
        return r

    S = cases.build_online(bl, c, storeHistory=history)
    S.BLOCK_MIN_POINTS = 1
    with options(chain_nd=2):
        eng.fit = spy
        try:
            quiet(S.stepMany, np.array(data[:3]))
            quiet(S.stepMany, np.array(data[3:]))
        finally:
            del eng.fit
    assert len(seen) == 4 and [s[:2] for s in seen] == [(False, True), (False, True), (True, True), (True, True)], [s[:2] for s in seen]
    for _, _, lt in seen:
        assert lt['fwd_kernel_variant'] == cs.VARIANT and lt['forward_launches'] == 1 and lt['batches'] == 1, lt
    W = cases.build_online(bl, c, storeHistory=history)
    with options(chain_nd_stages=0):
        for d in data:
            quiet(W.step, d)
    assert_meets(S, W)
