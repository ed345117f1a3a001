"""
Batches the chain-resident route of two-parameter grids plans and then declines (ChainRun::setup, blhip_fit_paths.hpp: chain_fold_settle and
chain_padding_rule answer keep = 0 after the fold plan is made) run on the launch-per-step kernels, which store [t][row][column]; their
separate fold must read exactly that, whatever the declined plan said about the layout (chain_fold_source, blhip_chain_plan.hpp).  Every
case of tests/declined_cases.py is a whole study against the float64 oracle at the suite's bar (compare.GPU_TOL, as
test_fold_recovery.assert_oracle applies it), with the route asserted: no chain kernel (variant 6), no fall-back -- a decline is none --,
and every chain folded once.  tests/test_chain_plan_host.py holds the host planner to `keep 0` on the same facts.

The C case is the other side: the chain kernels run, the fused fold is off, and accumulate2_kernel reads two strips of 1024 rows in the
strip-major layout -- the smallest shape on which that layout is not the row-major one.

test_the_data_show_a_strip_major_misread needs no GPU: it applies the misread to the oracle's average posterior and asserts that the bar
rejects it, so the studies are not symmetric enough to hide the permutation.

See tests/DECLINED_BATCHES.md.
"""
import functools

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import declined_cases as dc
import oracle_adapter as oa

gpu = pytest.mark.gpu
KEYS = ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'hyperParameterDistribution', 'logEvidenceList')
ALL = dict(dc.DECLINED, **dc.C_CASES)


@pytest.fixture(scope='module')
def eng():
    prev = bl.set_engine(None)
    e = bl.get_engine()                      # raises BackendError if libblhip.so or the GPU is missing
    assert type(e).__name__ == 'HipEngine'
    yield e
    bl.set_engine(prev)


@functools.lru_cache(maxsize=None)
def oracle(name):
    with np.errstate(all='ignore'):
        return oa.run(ALL[name]['case'])


def fit(eng, name):
    """-> (study, folded count of the accumulator); the case's options are reset afterwards"""
    d = ALL[name]
    try:
        for k, v in d['opts'].items():
            eng.set_option(k, v)
        S = cases.build(bl, d['case'])
        S.fit(**cases.fit_kwargs(d['case']))
        folded = eng.accum_log_ref()[1] if d['hyper'] else None
    finally:
        for k in d['opts']:
            eng.set_option(k, dc.OPTION_DEFAULTS[k])
    return S, folded


def assert_oracle(S, name):
    want = oracle(name)
    gold = {k: want[k] for k in KEYS if k in want}
    got = {k: (np.asarray(getattr(S, k)) if k in ('hyperParameterDistribution', 'logEvidenceList') else getattr(S, k)) for k in gold}
    pw, pg = np.asarray(want['posteriorSequence'], dtype=float), np.asarray(got['posteriorSequence'], dtype=float)
    print('%s: logEvidence %.15g (oracle %.15g), largest relative posterior error %.3g' % (
        name, S.logEvidence, want['logEvidence'], float(np.max(np.abs(pg - pw) / np.maximum(np.abs(pw), 1e-300)))))
    compare.check(got, gold, compare.GPU_TOL)


def assert_every_chain_folded_once(S, folded):
    prior = np.asarray(S.flatHyperPriorValues, dtype=float)
    n = int(np.sum(np.isfinite(np.asarray(S.logEvidenceList, dtype=float)) & (prior > 0)))
    assert folded == n == len(prior), (folded, n, len(prior))


@gpu
@pytest.mark.parametrize('name', list(dc.DECLINED))
def test_a_declined_batch_matches_the_oracle(eng, name):
    S, folded = fit(eng, name)
    t = S.lastTiming
    print(name, {k: t[k] for k in ('fwd_kernel_variant', 'bwd_kernel_variant', 'resident_fallbacks', 'batches', 'accumulate_launches')})
    assert t['fwd_kernel_variant'] != 6 and t['bwd_kernel_variant'] != 6 and t['resident_fallbacks'] == 0, t
    if ALL[name]['hyper']:
        assert_every_chain_folded_once(S, folded)
    assert_oracle(S, name)


@gpu
def test_the_separate_fold_of_two_strips(eng):
    """the chain kernels store strip-major, accumulate2_kernel folds from it (the planner's answer for this batch: test_chain_plan_host.py)"""
    from test_postfit_kernels import Launched, only_fold
    name = 'C1_walks_unfused_1024x32'
    with Launched() as k:
        S, folded = fit(eng, name)
    t = S.lastTiming
    assert t['fwd_kernel_variant'] == 6 and t['bwd_kernel_variant'] == 6 and t['resident_fallbacks'] == 0 and t['batches'] == 1, t
    k.require('chain_kernel')
    only_fold(k, 'accumulate2_kernel')
    k.forbid('depad_kernel')
    assert k.count['accumulate2_kernel'] == 1, k.count
    assert_every_chain_folded_once(S, folded)
    assert_oracle(S, name)


def _misread_cases():
    # (ragged columns / an odd number of cells: the misread leaves the step -- nothing the bar could be asked about)
    out = [(n, ALL[n]['case'], ALL[n]['grid']) for n in list(dc.A_CASES) + list(dc.C_CASES) if ALL[n]['grid'][1] % 16 == 0]
    return out + [('fold_recovery_single_chain_2strips', None, (1024, 32))]


@pytest.mark.parametrize('name,case,grid', _misread_cases(), ids=[c[0] for c in _misread_cases()])
def test_the_data_show_a_strip_major_misread(name, case, grid):
    if case is None:
        import test_fold_recovery as fr
        case = fr.FLAVOURS['single_chain_2strips']['plain']
        with np.errstate(all='ignore'):
            want = oa.run(case)
    else:
        want = oracle(name)
    gold = {k: want[k] for k in KEYS if k in want}
    wrong = dc.strip_major_misread(want['posteriorSequence'], *grid)
    assert wrong is not None and wrong.shape == np.asarray(want['posteriorSequence']).shape
    compare.check(dict(gold), gold, compare.GPU_TOL)                     # (the bar accepts the oracle itself ...)
    with pytest.raises(AssertionError, match='posteriorSequence'):       # (... and rejects it misread, by the posteriors alone)
        compare.check(dict(gold, posteriorSequence=wrong), gold, compare.GPU_TOL)
