"""
The chain-resident kernel for chain batches on grids with three and four parameters (bayesloop_amd/csrc/blhip_chain_nd.hpp:
bln::chain_nd_kernel<BWD, 256 | 1024>), on the GPU.  Cases: tests/chain_nd_cases.py.

Every comparison is compare.check at compare.GPU_TOL (log-evidence 1e-9 relative, posteriors |dp| <= 1e-12 + 1e-9 p, the NaN pattern
of localEvidence included) against the oracle.  A batch the kernel must take reports fwd_ / bwd_kernel_variant 10 and ONE launch per
pass; one it must not take reports 7 (the plain N-D path).  Option chain_nd: 0 never, 1 (default) from 16 chains on, 2 wherever the
LDS envelope admits the batch.
"""
import contextlib
import io

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import chain_nd_cases as cn
import compare
import oracle_adapter as oa

pytest.importorskip('scipy.stats')
pytestmark = pytest.mark.gpu


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


def check_marginals(S, post):
    """marginal distributions of every parameter against the (average) posterior sequence `post`"""
    post = np.asarray(post)
    for k, name in enumerate(S.observationModel.parameterNames):
        axes = tuple(a + 1 for a in range(post.ndim - 1) if a != k)
        np.testing.assert_allclose(S.getParameterDistributions(name, density=False)[1], post.sum(axis=axes), rtol=1e-9, atol=1e-12)


ALL = dict(cn.ND, **cn.BELOW, **cn.FORCED, cnd_split=cn.SPLIT)
_ORACLE = {}


def oracle_of(case):
    """the oracle's result of a case, computed once per session"""
    if case not in _ORACLE:
        with np.errstate(all='ignore'):
            _ORACLE[case] = oa.run(ALL[case])
    return _ORACLE[case]


@contextlib.contextmanager
def options(**kw):
    eng = bl.get_engine()
    defaults = dict(chain_nd=1, max_batch=1024)
    try:
        for k, v in kw.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in kw:
            eng.set_option(k, defaults[k])


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
    per_pass = batches * (1 if variant == cn.VARIANT else T)
    assert lt['forward_launches'] == per_pass, lt
    assert lt['backward_launches'] == (per_pass if full else 0), lt


def check_oracle(S, case, c):
    got = result_of(S, c)
    want = oracle_of(case)
    gold = gold_of(want, got)
    compare.check(got, gold, compare.GPU_TOL, case_tol=c.get('tol'))
    return want, gold


@pytest.mark.parametrize('case', sorted(cn.ND))
def test_batch_of_sixteen_chains_matches_the_oracle(case):
    """16 chains take the kernel where the cost model gives it the batch (the largest grids: under chain_nd = 2), the plain path where the
    envelope refuses the grid, whatever the option"""
    c = cn.ND[case]
    S = fit(c, **c.get('opts', {}))
    assert len(S.logEvidenceList) == cn.MIN_CHAINS
    check_route(S, c, c.get('variant', cn.VARIANT))
    want, gold = check_oracle(S, case, c)
    if 'posteriorSequence' in gold:
        check_marginals(S, want['posteriorSequence'])


def test_a_dead_chain_leaves_its_neighbours_alone():
    """sigma = 0: the normaliser of step 2 is 0, the chain's evidence -inf and its local evidence NaN from there on, as the oracle's; the
    15 other chains of the batch keep the bar"""
    c = cn.ND['cnd_dead_chain']
    S = fit(c, **c['opts'])
    check_route(S, c, cn.VARIANT)
    want = oracle_of('cnd_dead_chain')
    le, wl = np.asarray(S.logEvidenceList, dtype=float), np.asarray(want['logEvidenceList'], dtype=float)
    assert np.isneginf(wl[0]) and np.all(np.isfinite(wl[1:]))
    assert le[0] == wl[0]
    np.testing.assert_allclose(le[1:], wl[1:], rtol=compare.GPU_TOL['logE_rtol'], atol=0)
    assert np.array_equal(np.isnan(np.asarray(S.localEvidence, dtype=float)), np.isnan(np.asarray(want['localEvidence'], dtype=float)))
    assert np.isnan(np.asarray(want['localEvidence'], dtype=float)).sum() == 1


@pytest.mark.parametrize('case', cn.GOLDEN)
def test_case_matches_the_references_fixture(case):
    c = cn.ND[case]
    S = fit(c, **c.get('opts', {}))
    check_route(S, c, cn.VARIANT)
    compare.check(result_of(S, c), oa.load_golden(case), compare.GPU_TOL)


def test_one_chain_below_the_floor():
    """15 chains: the plain path by default, the kernel under chain_nd = 2; both at the bar"""
    c = cn.BELOW['cnd_fifteen_chains']
    S = fit(c)
    assert len(S.logEvidenceList) == cn.MIN_CHAINS - 1
    check_route(S, c, cn.PLAIN)
    check_oracle(S, 'cnd_fifteen_chains', c)
    R = fit(c, chain_nd=2)
    check_route(R, c, cn.VARIANT)
    check_oracle(R, 'cnd_fifteen_chains', c)


@pytest.mark.parametrize('case', sorted(cn.FORCED))
def test_single_chain_study_under_chain_nd_2(case):
    """a plain Study keeps its posteriors on the device and hands them out: by default the plain path, forced into the kernel"""
    c = cn.FORCED[case]
    check_route(fit(c), c, cn.PLAIN)
    S = fit(c, chain_nd=2)
    check_route(S, c, cn.VARIANT)
    want, _ = check_oracle(S, case, c)
    check_marginals(S, want['posteriorSequence'])


@pytest.mark.parametrize('case', ['cnd_hyper_first_last', 'cnd_three_walks', 'cnd_serial_segments', 'cnd_largest'])
def test_kernel_against_the_plain_path(case):
    """the same study under chain_nd = 2 and chain_nd = 0: both at the bar against the oracle (the deviation between the two is printed;
    profiles/chain_nd_notes.md records it)"""
    c = cn.ND[case]
    K, P = fit(c, chain_nd=2), fit(c, chain_nd=0)
    assert c.get('variant', cn.VARIANT) == cn.VARIANT
    check_route(K, c, cn.VARIANT)
    check_route(P, c, cn.PLAIN)
    check_oracle(K, case, c)
    check_oracle(P, case, c)
    pk, pp = np.asarray(K.posteriorSequence), np.asarray(P.posteriorSequence)
    lk, lp = np.asarray(K.logEvidenceList), np.asarray(P.logEvidenceList)
    with np.errstate(all='ignore'):
        rel = np.nanmax(np.where(pp > 1e-12, np.abs(pk - pp) / pp, 0.0))
    print('%s: kernel vs plain: posterior max rel %.3e (cells > 1e-12), max abs %.3e; log-evidence max rel %.3e'
          % (case, rel, np.abs(pk - pp).max(), np.max(np.abs(lk - lp) / np.abs(lp))))


def test_option_chain_nd_is_known_and_others_are_not():
    eng = bl.get_engine()
    with options(chain_nd=0):
        pass
    with pytest.raises(bl.exceptions.BackendError, match='unknown option'):
        eng.set_option('chain_nd_', 1)


def test_split_batches():
    """35 chains, max_batch = 16: two resident batches and a remainder of 3 on the plain path.  The chains of the resident batches have
    the log-evidences of the unsplit run bit for bit (a chain's block depends on nothing but the chain); the call's results stay at the
    bar across the seam."""
    c = cn.SPLIT
    one = fit(c)
    check_route(one, c, cn.VARIANT)
    assert len(one.logEvidenceList) == 35
    T = len(cases.make_data(c['data']))
    split = fit(c, max_batch=16)
    lt = split.lastTiming
    assert lt['batches'] == 3 and lt['fwd_kernel_variant'] == cn.PLAIN, lt          # (the last batch's id)
    assert lt['forward_launches'] == 2 + T and lt['backward_launches'] == 2 + T, lt
    assert np.array_equal(np.asarray(split.logEvidenceList)[:32], np.asarray(one.logEvidenceList)[:32])
    check_oracle(one, 'cnd_split', c)
    check_oracle(split, 'cnd_split', c)
    # two resident batches and nothing else
    two = fit(dict(c, tm=cn._two_walks(cn.T3, 'df', 'loc', (0, 1, 2, 3), (1, 2, 3, 4, 6, 8, 12, 5))), max_batch=16)
    check_route(two, c, cn.VARIANT, batches=2)
    ref = fit(dict(c, tm=cn._two_walks(cn.T3, 'df', 'loc', (0, 1, 2, 3), (1, 2, 3, 4, 6, 8, 12, 5))))
    check_route(ref, c, cn.VARIANT)
    assert np.array_equal(np.asarray(two.logEvidenceList), np.asarray(ref.logEvidenceList))
    np.testing.assert_allclose(np.asarray(two.posteriorSequence), np.asarray(ref.posteriorSequence), rtol=compare.GPU_TOL['post_rtol'],
                               atol=compare.GPU_TOL['post_atol'])
