"""
The average posterior of a hyper-study is built two ways inside ONE call of the library (blhip.hip, do_fit):
  * fused batches: the chain-resident backward kernel adds the batch to the carried partial accumulators, which go into the
    average once per call (DESIGN 4.5 e);
  * direct batches: every other batch is folded straight into the accumulator -- a batch with a walk wider than the chain-resident
    kernels' band, or one whose resident forward check failed and that was repeated in place.
A fused batch whose check fails after its backward pass has written slots that carry earlier batches makes the call repeat the
batches since the first carried one on the launch-per-step kernels.  A direct batch inside that range must not be folded twice.

The failures are forced on the host (options fold_force_fail_batch, chain_force_fail_batch / chain_force_fail_stage); every forced
run must give the unforced run's results, and the accumulator's folded count (accum_log_ref()[1]) must equal the number of hyper
points with a finite evidence and a positive hyper-prior value -- a double fold shows in that count whatever the weights.
"""
import functools

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import oracle_adapter as oa

pytestmark = pytest.mark.gpu

NB = 16                                   # chains per batch (option max_batch)
RANGE, PREDICTION, FORCED = 2, 3, 4       # BLHIP_FALLBACK_*
DEFAULTS = dict(max_batch=1024, fold_force_fail_batch=-1, chain_force_fail_batch=-1, chain_force_fail_stage=0, fold2=1, fold2_cp=1,
                fuse_accumulate=1, chain_ax1=1)


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()                    # raises BackendError if libblhip.so or the GPU is missing
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def _g2(n0, n1):
    return ('Gaussian', [('mean', ('cint', -8, 8, n0)), ('std', ('oint', 0, 4, n1))], 'default')


def _values(lo, hi, nbatch=3, wide=None, wide_batch=1):
    """nbatch batches of NB random-walk widths, each spanning [lo, hi] (every batch carries a similar share of the hyper-parameter
    distribution); `wide` replaces a width in the MIDDLE of batch `wide_batch`: narrow widths after it keep split_wide_axis0 from
    cutting it out, so that batch runs on the launch-per-step kernels and is folded directly."""
    base = np.linspace(lo, hi, NB)
    v = np.concatenate([base + 0.002 * b for b in range(nbatch)])
    if wide is not None:
        v[wide_batch * NB + NB // 2] = wide
    return [float(x) for x in v]


def _hyper(n0, n1, seed, T, values, prior=None):
    return dict(study='HyperStudy', data=('series', seed, T), om=_g2(n0, n1), tm=('GRW', 'sigma', values, 'mean', prior))


def _both_axes(values):
    return dict(study='HyperStudy', data=('series', 95, 6), om=_g2(128, 128),
                tm=('Combined', [('GRW', 's1', values, 'mean', None), ('GRW', 's2', 0.05, 'std', None)]))


# fused-fold flavours: the case with a wide walk in the middle batch (None: the flavour has none), the case without, and the option that
# turns the flavour's fused fold off (-> every batch is stored and folded on its own)
FLAVOURS = {
    # the two-chain fold kernel (128 rows; radius 95 > CHAIN_R0_MAX for the wide walk)
    'two_chain': dict(wide=_hyper(128, 64, 93, 8, _values(0.0, 0.5, wide=3.0)), plain=_hyper(128, 64, 93, 8, _values(0.0, 0.5)),
                      off=dict(fold2=0), opts={}),
    # the single-chain fold (1024 rows: the two-chain kernel stops at 512; the wide walk: radius 115 > 80)
    'single_chain': dict(wide=_hyper(1024, 16, 94, 6, _values(0.01, 0.15, wide=0.45)), plain=_hyper(1024, 16, 94, 6, _values(0.01, 0.15)),
                         off=dict(fuse_accumulate=0), opts=dict(fold2=0)),
    # ... on two strips (one strip of 16 columns stores strip-major exactly as row-major: a repeated batch's layout cannot go wrong there)
    'single_chain_2strips': dict(wide=_hyper(1024, 32, 98, 6, _values(0.01, 0.15, wide=0.45)), plain=_hyper(1024, 32, 98, 6, _values(0.01, 0.15)),
                                 off=dict(fuse_accumulate=0), opts=dict(fold2=0)),
    # change points: the two-chain fold with its restart rule
    'changepoint': dict(wide=None, plain=dict(study='ChangepointStudy', data=('series_jump', 96, 52, 26, 0.0), om=_g2(256, 32),
                                              tm=('ChangePoint', 'tChange', [int(x) for x in np.arange(2, 50)], None)),
                        off=dict(fold2_cp=0), opts={}),
    # walks on both parameters: the transposing kernels' fold (radius 79 > 40 for the wide walk)
    'both_axes': dict(wide=_both_axes(_values(0.0, 0.3, wide=2.5)), plain=_both_axes(_values(0.0, 0.3)), off=dict(chain_ax1=0), opts={}),
}


def _key(c):
    return repr(sorted(c.items()))


@functools.lru_cache(maxsize=None)
def _oracle(key):
    c = _CASES[key]
    with np.errstate(all='ignore'):
        return oa.run(c)


_CASES = {}


def oracle(c):
    k = _key(c)
    _CASES[k] = c
    return _oracle(k)


def fit(c, **opts):
    """One fit with max_batch = NB and the given options (every option is reset afterwards); -> (study, folded count of the accumulator)."""
    eng = bl.get_engine()
    opts = dict(dict(max_batch=NB), **opts)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        S = cases.build(bl, c)
        S.fit(**cases.fit_kwargs(c))
        folded = eng.accum_log_ref()[1]        # (the accumulator stays open after a single-rank HyperStudy.fit: the average lives there)
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])
    return S, folded


def expected_folded(S):
    prior = np.asarray(S.flatHyperPriorValues, dtype=float)
    return int(np.sum(np.isfinite(np.asarray(S.logEvidenceList, dtype=float)) & (prior > 0)))


def assert_same(R, A):
    """The bars of the carried-partials test (test_gpu_parity.py): the forced run against the unforced one."""
    assert abs(A.logEvidence - R.logEvidence) <= 1e-12 * abs(A.logEvidence), (R.logEvidence, A.logEvidence)
    np.testing.assert_allclose(np.array(R.posteriorSequence), np.array(A.posteriorSequence), rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(R.posteriorMeanValues, A.posteriorMeanValues, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(R.hyperParameterDistribution, A.hyperParameterDistribution, rtol=1e-11)


def assert_oracle(S, c, nbatch, weighted=True):
    """The unforced run against the oracle; and every batch carries >= 5 % of the hyper-parameter distribution, so that a batch folded
    twice moves the average posterior far outside the bars of assert_same (not only the folded count)."""
    want = oracle(c)
    got = dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence, posteriorSequence=S.posteriorSequence,
               posteriorMeanValues=S.posteriorMeanValues, hyperParameterDistribution=np.asarray(S.hyperParameterDistribution))
    gold = {k: want[k] for k in ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'hyperParameterDistribution')}
    compare.check(got, gold, compare.GPU_TOL)
    if weighted:
        h = np.asarray(want['hyperParameterDistribution'])
        assert len(h) == nbatch * NB
        shares = [float(h[b * NB:(b + 1) * NB].sum() / h.sum()) for b in range(nbatch)]
        assert min(shares) >= 0.05, shares


def assert_recovered(R, A, folded, n_forced, reason):
    t = R.lastTiming
    assert t['resident_fallbacks'] >= n_forced and t['resident_fallback_reason'] == reason, t
    pa, pr = np.array(A.posteriorSequence), np.array(R.posteriorSequence)
    err = float(np.max(np.abs(pr - pa) / np.maximum(np.abs(pa), 1e-300)))
    assert folded == expected_folded(R), 'folded %d, expected %d (largest relative posterior error %.3g)' % (folded, expected_folded(R), err)
    assert_same(R, A)


# (option sets that poison the carried slots of batch `b` after its backward pass: the prediction check, the range check, a give-up)
def poison(kind, b):
    return {'fold': (dict(fold_force_fail_batch=b), PREDICTION),
            'stage2': (dict(chain_force_fail_batch=b, chain_force_fail_stage=2), RANGE),
            'stage3': (dict(chain_force_fail_batch=b, chain_force_fail_stage=3), FORCED)}[kind]


def _rearm():
    bl.get_engine().set_option('resident_ok', 1)


@pytest.mark.parametrize('flavour', list(FLAVOURS))
def test_every_fused_fold_flavour_carries_its_slots_through_the_call(flavour):
    """The unforced plan the other tests rely on: three chain-resident batches, ONE fold of the carried slots (accumulate_launches 1);
    with the flavour's fused fold off every batch folds on its own (3) and the results agree."""
    F = FLAVOURS[flavour]
    c = F['plain']
    A, folded = fit(c, **F['opts'])
    t = A.lastTiming
    assert t['batches'] == 3 and t['bwd_kernel_variant'] == 6 and t['accumulate_launches'] == 1 and t['resident_fallbacks'] == 0, t
    assert folded == expected_folded(A) == 3 * NB
    assert_oracle(A, c, 3)
    B, folded = fit(c, **dict(F['opts'], **F['off']))
    assert B.lastTiming['accumulate_launches'] == 3, B.lastTiming
    assert folded == 3 * NB
    assert_same(B, A)


@pytest.mark.parametrize('poison_kind', ['fold', 'stage2', 'stage3'])
@pytest.mark.parametrize('flavour', ['two_chain', 'single_chain', 'single_chain_2strips', 'both_axes'])
def test_wide_batch_between_fused_batches_is_folded_once(flavour, poison_kind):
    """fused, direct (a wide walk), fused -- the last batch poisons the slots that carry the first: the repeat re-runs batches 0 .. 2,
    the direct batch 1 must not reach the accumulator a second time."""
    F = FLAVOURS[flavour]
    c = F['wide']
    A, folded = fit(c, **F['opts'])
    t = A.lastTiming
    assert t['batches'] == 3 and t['bwd_kernel_variant'] == 6 and t['resident_fallbacks'] == 0, t
    assert t['accumulate_launches'] == 2, t                     # the direct fold of batch 1 + ONE fold of the carried slots
    assert folded == expected_folded(A) == 3 * NB
    assert_oracle(A, c, 3)
    opts, reason = poison(poison_kind, 2)
    try:
        R, folded = fit(c, **dict(F['opts'], **opts))
    finally:
        _rearm()
    assert_recovered(R, A, folded, 1, reason)


@pytest.mark.parametrize('flavour', list(FLAVOURS))
def test_batch_repeated_in_place_then_poisoned_slots(flavour):
    """Two failures in one call: batch 1's forward check fails (chain_force_fail_stage 1: repeated in place, folded directly), then
    batch 2's prediction check fails after its backward pass has added to the slots that carry batch 0."""
    F = FLAVOURS[flavour]
    c = F['plain']
    A, _ = fit(c, **F['opts'])
    assert A.lastTiming['accumulate_launches'] == 1 and A.lastTiming['bwd_kernel_variant'] == 6, A.lastTiming
    assert_oracle(A, c, 3)
    B, folded = fit(c, **dict(F['opts'], chain_force_fail_batch=1, chain_force_fail_stage=1))
    assert B.lastTiming['accumulate_launches'] == 2, B.lastTiming        # (batch 1 became direct)
    assert_recovered(B, A, folded, 1, RANGE)
    R, folded = fit(c, **dict(F['opts'], chain_force_fail_batch=1, chain_force_fail_stage=1, fold_force_fail_batch=2))
    assert_recovered(R, A, folded, 2, PREDICTION)


@pytest.mark.parametrize('poison_kind', ['fold', 'stage2', 'stage3'])
def test_failure_in_the_second_batch(poison_kind):
    """fused, fused, direct: batch 1 poisons the slots that carry batch 0 -- the repeat covers batches 0 and 1, the direct batch 2
    follows it (after a give-up on the launch-per-step kernels as well)."""
    F = FLAVOURS['two_chain']
    c = _hyper(128, 64, 93, 8, _values(0.0, 0.5, wide=3.0, wide_batch=2))
    A, folded = fit(c)
    t = A.lastTiming                                            # (bwd_kernel_variant: the last batch's, the direct one here)
    assert t['batches'] == 3 and t['accumulate_launches'] == 2 and t['resident_fallbacks'] == 0, t
    assert folded == 3 * NB
    assert_oracle(A, c, 3)
    opts, reason = poison(poison_kind, 1)
    try:
        R, folded = fit(c, **dict(F['opts'], **opts))
    finally:
        _rearm()
    assert_recovered(R, A, folded, 1, reason)


@pytest.mark.parametrize('poison_kind', ['fold', 'stage2', 'stage3'])
def test_failure_after_a_flush_of_the_carried_slots(poison_kind):
    """Four batches; the hyper-prior lifts batches 1 .. 3 by 552 e-folds above batch 0, so batch 1 flushes the slots that carry batch 0
    (prepare_fold) and starts them afresh; batch 2 is direct (a wide walk), batch 3 poisons the slots -- the repeat covers batches 1 .. 3
    only.  (Batch 0 carries no weight here: the folded count is the detector for it.)"""
    v = _values(0.0, 0.5, nbatch=4, wide=3.0, wide_batch=2)
    prior = [1e-240] * NB + [1.0] * (3 * NB)
    c = _hyper(128, 64, 97, 8, v, prior=('array', prior))
    A, folded = fit(c)
    t = A.lastTiming
    assert t['batches'] == 4 and t['bwd_kernel_variant'] == 6 and t['resident_fallbacks'] == 0, t
    assert t['accumulate_launches'] == 3, t                     # the flush of batch 0, the direct fold of batch 2, the final flush
    assert folded == expected_folded(A) == 4 * NB
    assert_oracle(A, c, 4, weighted=False)
    h = np.asarray(oracle(c)['hyperParameterDistribution'])
    assert min(float(h[b * NB:(b + 1) * NB].sum() / h.sum()) for b in (1, 2, 3)) >= 0.05
    opts, reason = poison(poison_kind, 3)
    try:
        R, folded = fit(c, **opts)
    finally:
        _rearm()
    assert_recovered(R, A, folded, 1, reason)


# ---- a hyper-study to which no chain contributes: the reference's average is all NaN (core.py:1375-1382) --------------------------

def _no_chain_case(study='HyperStudy'):
    # a zero normaliser at step 2 in every chain (the 500 lies ~1000 standard deviations off the grid): every logEvidence is -inf
    return dict(study=study, data=np.array([0.2, 0.1, 500.0, 0.3, -0.1]), om=('Gaussian', [('mean', ('cint', -2, 2, 32)), ('std', ('oint', 0, 0.5, 32))],
                                                                             'default'),
                tm=('GRW', 'sigma', [0.05, 0.1, 0.2], 'mean', None))


@pytest.mark.parametrize('host_transition', [False, True])
def test_no_chain_contributes(host_transition):
    """The device path (dist.sharded_hyper_fit: the library's accumulator) and the host-transition path (a user-defined walk:
    HyperStudy._fitHostTransitionHyper) give the reference's NaN average, NaN means, NaN hyper-parameter distribution and -inf evidence."""
    import plugin_models
    c = _no_chain_case()
    with np.errstate(all='ignore'):
        want = oa.run(c)
    S = cases.build(bl, c)
    if host_transition:
        S.set(plugin_models.make(bl.tm)['LeakyRandomWalk']('sigma', [0.05, 0.1, 0.2], 'leak', 0.0, target='mean'), silent=True)
    with np.errstate(all='ignore'):
        S.fit(silent=True)
    assert S.logEvidence == want['logEvidence'] == -np.inf
    wp = np.asarray(want['posteriorSequence'])
    assert np.all(np.isnan(wp)) and np.all(np.isnan(want['posteriorMeanValues']))
    for post in (np.asarray(S.posteriorSequence), np.asarray(S.averagePosteriorSequence)):
        assert post.shape == wp.shape and np.all(np.isnan(post))
    means = np.asarray(S.posteriorMeanValues, dtype=float)
    assert means.shape == np.asarray(want['posteriorMeanValues']).shape and np.all(np.isnan(means))
    np.testing.assert_array_equal(np.isnan(S.hyperParameterDistribution), np.isnan(want['hyperParameterDistribution']))
    assert bl.get_engine()._accum_owner is None             # (the accumulator was closed: nobody owns it)
