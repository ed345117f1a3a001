"""
Study.fitMany on two-parameter grids on a real MI355X: many data series as ONE device call per batch of series -- a chain of the
chain-resident kernels (blc::chain_kernel, blc::chainax_kernel) per series, every chain reading its own records, anchors or likelihood
table (ChainParams::rec_chain / anch_chain / lik_chain).

Every case compares, per series, logEvidence, localEvidence, the posterior means and the whole posterior sequence with the CPU oracle's
fit of that series ALONE at the project's parity bar (compare.GPU_TOL), asserts with the kernel census that the expected family ran and
no launch-per-step kernel did, and that stderr carries no loop notice.  Series within a case differ (mean 0.3 s, width 1 + 0.3 s), so a
wrong per-chain offset shows.  The shapes are the smallest that reach each code path: T = 3 .. 6, three series unless stated.
"""
import numpy as np
import pytest

import bayesloop_amd as bl
import compare
from test_series_fit import Launched, at_the_bar, entry, golds_of, oracle_alone

pytestmark = pytest.mark.gpu

CHAIN, CHAINAX = 'blc::chain_kernel', 'blc::chainax_kernel'
PER_STEP_PREFIXES = ('blk::step_kernel', 'step_kernel', 'blf::', 'blm::', 'blr::')
NOTICE = 'fitMany runs the loop'


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    """an engine of the module's own: the options the tests set go with it"""
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def launches(k, kernel):
    """launches of a kernel family, whichever namespace the census names it in"""
    return sum(c for f, c in k.count.items() if f == kernel or f.endswith('::' + kernel))


def values(S, T, seed=0, dim=None, wrap=None):
    """series s: mean 0.3 s, width 1 + 0.3 s.  wrap (hundreds of series): s counts modulo wrap -- series 100 would lie 30 grid widths outside
    the grid, its likelihood underflows everywhere, and a chain-resident pass that meets such a chain hands the whole call to the loop"""
    rng = np.random.RandomState(100 + seed)
    return [rng.normal(0.3 * (s % (wrap or S)), 1 + 0.3 * (s % (wrap or S)), size=T if dim is None else (T, dim)) for s in range(S)]


def gaussian(n0, n1, tm):
    def make():
        S = bl.Study(silent=True)
        S.set(bl.om.Gaussian('mean', bl.cint(-2, 2, n0), 'std', bl.oint(0, 3, n1)), tm(), silent=True)
        return S
    return make


def walk_mean(sigma=0.1):
    return lambda: bl.tm.GaussianRandomWalk('sigma', sigma, target='mean')


def walk_both(s0=0.2, s1=0.1):
    return lambda: bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s0', s0, target='mean'), bl.tm.GaussianRandomWalk('s1', s1, target='std'))


def on_chain_kernels(k, family, err):
    """the family expected ran, no launch-per-step kernel and not the other chain family, no loop notice"""
    assert k.count.get(family, 0) >= 1, k.count
    other = CHAINAX if family == CHAIN else CHAIN
    assert k.count.get(other, 0) == 0 and k.count.get('blc::chain_clamp_kernel', 0) == 0, k.count
    # (blr::residency_probe_kernel is no fit kernel: the one-block-per-CU probe in front of any fit that may take a resident path)
    assert not [f for f in k.count if f.startswith(PER_STEP_PREFIXES) and f != 'blr::residency_probe_kernel'], k.count
    assert NOTICE not in err, err


def fit_many(make, series, capfd, **kw):
    bl.Study._series_loop_announced = frozenset()
    capfd.readouterr()
    with Launched() as k:
        R = make().fitMany(series, silent=True, **kw)
    return R, k, capfd.readouterr().err


KW = [{}, dict(forwardOnly=True), dict(evidenceOnly=True)]
KW_IDS = ['full', 'forwardOnly', 'evidenceOnly']


# ---- Gaussian, walk on the mean: the filtering flavours, anchors per chain ------------------------------------------------------------------
@pytest.mark.parametrize('kw', KW, ids=KW_IDS)
@pytest.mark.parametrize('n0, n1', [(128, 16), (128, 32), (33, 32)], ids=['exact_one_strip', 'two_strips', 'padded'])
def test_gaussian_walk_on_the_mean(n0, n1, kw, capfd):
    make, series = gaussian(n0, n1, walk_mean(0.1 if n0 == 128 else 0.2)), values(3, 5, seed=n0 + n1)
    R, k, err = fit_many(make, series, capfd, **kw)
    on_chain_kernels(k, CHAIN, err)
    assert launches(k, 'anchor_table_kernel') >= 1, k.count
    assert R.lastTiming['fwd_kernel_variant'] == 6 and (kw or R.lastTiming['bwd_kernel_variant'] == 6)
    if (n0, n1) == (33, 32) and not kw.get('evidenceOnly'):
        assert launches(k, 'depad_kernel') >= 1, k.count           # (the kernels' sequence lives on 128 x 32: copied out)
    at_the_bar(R, golds_of(('2d walk', n0, n1), make, series, **kw))
    if not kw:                                                         # the accessors: (T, n0, n1) sequences, two rows of means, marginals
        post = R.posteriorSequence(1)
        assert post.shape == (5, n0, n1) and R.posteriorMeanValues[1].shape == (2, 5)
        St = make()
        for a, name in enumerate(('mean', 'std')):
            grid, dist = R.getParameterDistributions(1, name)
            assert dist.shape == (5, (n0, n1)[a]) and np.array_equal(grid, St.marginalGrid[a])
            assert np.allclose(dist * St.latticeConstant[a], post.sum(axis=2 - a), rtol=1e-12, atol=0)
            assert np.array_equal(R.getParameterMeanValues(1, name), R.posteriorMeanValues[1][a])
        T1 = R.study(2)
        assert np.array_equal(T1.posteriorSequence, R.posteriorSequence(2)) and T1.logEvidence == R.logEvidence[2]


def test_a_nan_inside_one_series(capfd):
    """two data dimensions, one value of ONE series missing: the number of valid dimensions at that step differs between the chains"""
    make = gaussian(128, 16, walk_mean())
    series = values(3, 5, seed=7, dim=2)
    series[1][2, 0] = np.nan
    series[2][3, :] = np.nan
    R, k, err = fit_many(make, series, capfd)
    on_chain_kernels(k, CHAIN, err)
    at_the_bar(R, golds_of('2d nan', make, series))


def test_series_results_pickle(capfd):
    import pickle
    make, series = gaussian(128, 16, walk_mean()), values(3, 4, seed=3)
    R, k, err = fit_many(make, series, capfd)
    R2 = pickle.loads(pickle.dumps(R))
    assert R2._device is None
    at_the_bar(R2, golds_of('2d pickle', make, series))
    assert np.array_equal(R2.posteriorSequence(1), R.posteriorSequence(1))


# ---- the no-stencil flavour: records read in the kernel -------------------------------------------------------------------------------------
def test_gaussian_static(capfd):
    make, series = gaussian(128, 16, lambda: bl.tm.Static()), values(3, 5, seed=11)
    R, k, err = fit_many(make, series, capfd)
    on_chain_kernels(k, CHAIN, err)
    assert any('chain_kernel<4,' in nm for nm in k.names), k.names
    assert launches(k, 'anchor_table_kernel') == 0, k.count
    at_the_bar(R, golds_of('2d static', make, series))


@pytest.mark.parametrize('kw', [{}, dict(evidenceOnly=True)], ids=['full', 'evidenceOnly'])
def test_gaussian_changepoint_shares_no_prefix(kw, capfd):
    """ChangePoint at stamp 3 of 6: in a hyper-study the chains of such a batch are identical up to their restart and all but one skip
    that prefix (also evidence-only); series are not -- every chain runs its own steps 0 .. 2"""
    make, series = gaussian(128, 16, lambda: bl.tm.ChangePoint('tChange', 3)), values(3, 6, seed=13)
    R, k, err = fit_many(make, series, capfd, **kw)
    on_chain_kernels(k, CHAIN, err)
    assert any('chain_kernel<4,' in nm for nm in k.names), k.names
    at_the_bar(R, golds_of('2d changepoint', make, series, **kw))


# ---- walks on both parameters: blc::chainax_kernel, padded inside 128 x 128 -----------------------------------------------------------------
@pytest.mark.parametrize('S', [3, 2], ids=['three', 'two'])
def test_gaussian_walks_on_both_parameters(S, capfd):
    """S = 2: single fits and batches of two tabulate the even steps' likelihood once per batch (chainax_lik_table) -- off for series"""
    make, series = gaussian(40, 36, walk_both()), values(S, 4, seed=17)
    R, k, err = fit_many(make, series, capfd)
    on_chain_kernels(k, CHAINAX, err)
    assert launches(k, 'ax_lik_table_kernel') == 0, k.count
    at_the_bar(R, golds_of(('2d both', S), make, series))


# ---- table models: a (T, G) table per chain ---------------------------------------------------------------------------------------------------
def scaled_ar1(tm):
    def make():
        S = bl.Study(silent=True)
        S.set(bl.om.ScaledAR1('rho', bl.oint(-1, 1, 128), 'sigma', bl.oint(0, 3, 16)), tm(), silent=True)
        return S
    return make


def laplace():
    S = bl.Study(silent=True)
    S.set(bl.om.Laplace('mean', bl.cint(-2, 2, 100), 'scale', bl.oint(0, 3, 37)), bl.tm.GaussianRandomWalk('sigma', 0.1, target='mean'), silent=True)
    return S


def test_scaled_ar1_segments_of_two(capfd):
    make = scaled_ar1(lambda: bl.tm.GaussianRandomWalk('sigma', 0.05, target='rho'))
    series = values(3, 6, seed=19)                                     # (T + 1 points: 5 segments of two)
    R, k, err = fit_many(make, series, capfd)
    on_chain_kernels(k, CHAIN, err)
    assert any(nm.startswith(CHAIN) and nm.rstrip('>').endswith('true') for nm in k.names), k.names      # (the TAB flavour)
    assert launches(k, 'lik_table_kernel') >= 2, k.count            # (series 0's, as any fit, and the batch's)
    assert len(R.localEvidence[0]) == 5
    at_the_bar(R, golds_of('2d scaled ar1', make, series))


def test_laplace_padded_table(capfd):
    series = values(3, 4, seed=23)
    R, k, err = fit_many(laplace, series, capfd)
    on_chain_kernels(k, CHAIN, err)
    assert any(nm.startswith(CHAIN) and nm.rstrip('>').endswith('true, true') for nm in k.names), k.names      # (PAD, TAB)
    at_the_bar(R, golds_of('2d laplace', laplace, series))


# ---- batches and rounds ------------------------------------------------------------------------------------------------------------------------
def same_bits(A, B, n, sequences=True):
    assert np.array_equal(A.logEvidence, B.logEvidence)
    for s in range(n):
        assert np.array_equal(A.localEvidence[s], B.localEvidence[s], equal_nan=True), s       # (NaN: 0 / 0 in the reference, on both sides)
        if sequences:
            assert np.array_equal(A.posteriorMeanValues[s], B.posteriorMeanValues[s], equal_nan=True), s
            assert np.array_equal(A.posteriorSequence(s), B.posteriorSequence(s), equal_nan=True), s


def test_batches_of_three(hip_engine, capfd):
    """7 series in batches of 3 + 3 + 1: the batch's first chain enters the series index, a batch of ONE chain stays on the chain kernel, and
    the results do not depend on the batch size, bit for bit"""
    make, series = gaussian(128, 16, walk_mean()), values(7, 5, seed=29)
    whole = make().fitMany(series, silent=True)
    whole_e = make().fitMany(series, evidenceOnly=True, silent=True)
    hip_engine.set_option('max_batch', 3)
    try:
        R, k, err = fit_many(make, series, capfd)
        on_chain_kernels(k, CHAIN, err)
        assert k.count[CHAIN] == 6 and launches(k, 'anchor_table_kernel') == 3, k.count      # (three device calls of two passes)
        E, k, err = fit_many(make, series, capfd, evidenceOnly=True)
        on_chain_kernels(k, CHAIN, err)
        assert k.count[CHAIN] == 3 and E.lastTiming['batches'] == 3, (k.count, E.lastTiming['batches'])
    finally:
        hip_engine.set_option('max_batch', 1024)
    golds = golds_of('2d batches', make, series)
    at_the_bar(R, golds)
    at_the_bar(E, golds_of('2d batches', make, series, evidenceOnly=True))
    at_the_bar(whole, golds)
    same_bits(R, whole, 7)
    same_bits(E, whole_e, 7, sequences=False)


@pytest.mark.parametrize('tm', [lambda: bl.tm.Static(), walk_mean(0.05)], ids=['static', 'radius_6'])
def test_a_last_call_of_one_series_stays_on_the_chain_kernel(hip_engine, tm, capfd):
    """3 + 3 + 1 with a model whose SINGLE fit takes the time-resident kernel (no stencil, or a radius of at most 8): the last device call
    holds one series and must not take that kernel, which reads the shared tables -- it stays on blc::chain_kernel, nothing goes to the loop"""
    make, series = gaussian(128, 16, tm), values(7, 4, seed=59)
    hip_engine.set_option('max_batch', 3)
    try:
        R, k, err = fit_many(make, series, capfd)
    finally:
        hip_engine.set_option('max_batch', 1024)
    on_chain_kernels(k, CHAIN, err)
    assert k.count[CHAIN] == 6, k.count                                # (three device calls of two passes, the last with one chain)
    at_the_bar(R, golds_of(('2d last of one', type(make().transitionModel).__name__), make, series))


def test_more_series_than_a_launch_round(hip_engine, capfd):
    """One strip per chain: a launch round holds as many chains as the chip has compute units (at most 256).  The round size is read off
    the plan: the number of series is doubled until ONE evidence-only pass takes two launches.  Every series is then held bit for bit to a
    call in batches of 32 (one round each), and a sample -- first, last, around every power of two -- to the oracle."""
    make, T = gaussian(128, 16, walk_mean()), 3
    S, E = 32, None
    while S <= 1024:
        series = values(S, T, seed=31, wrap=5)
        E, k, err = fit_many(make, series, capfd, evidenceOnly=True)
        on_chain_kernels(k, CHAIN, err)
        assert E.lastTiming['batches'] == 1
        if k.count[CHAIN] >= 2:
            break
        S *= 2
    assert S <= 1024, 'no call of up to 1024 series took a second launch round'
    R, k, err = fit_many(make, series, capfd)
    on_chain_kernels(k, CHAIN, err)
    assert k.count[CHAIN] >= 4, k.count
    hip_engine.set_option('max_batch', 32)
    try:
        small = make().fitMany(series, silent=True)
        small_e = make().fitMany(series, evidenceOnly=True, silent=True)
    finally:
        hip_engine.set_option('max_batch', 1024)
    same_bits(R, small, S)
    same_bits(E, small_e, S, sequences=False)
    sample = sorted({0, 1, S - 1} | {p + d for p in (32, 64, 128, 256, 512) for d in (-1, 0) if p + d < S})
    for s in sample:
        compare.check(entry(R, s), oracle_alone(make, series[s]), compare.GPU_TOL)


# ---- the same kernel on the same anchors: bit for bit with single fits ----------------------------------------------------------------------
def test_bit_for_bit_with_single_fits(hip_engine):
    """option resident = 0 keeps a single fit off the time-resident kernel: it runs blc::chain_kernel as a batch of one (kernel variant 6 in
    both passes), on anchors tabulated by the same kernel from the same records -- entry s of fitMany equals it bit for bit"""
    make, series = gaussian(128, 16, walk_mean()), values(3, 5, seed=37)
    R = make().fitMany(series, silent=True)
    hip_engine.set_option('resident', 0)
    try:
        for s, d in enumerate(series):
            S = make()
            S.loadData(d, silent=True)
            S.fit(silent=True)
            assert S.lastTiming['fwd_kernel_variant'] == 6 and S.lastTiming['bwd_kernel_variant'] == 6, S.lastTiming
            assert R.logEvidence[s] == S.logEvidence
            assert np.array_equal(R.localEvidence[s], S.localEvidence)
            assert np.array_equal(R.posteriorMeanValues[s], S.posteriorMeanValues)
            assert np.array_equal(R.posteriorSequence(s), S.posteriorSequence)
    finally:
        hip_engine.set_option('resident', 1)


# ---- fallbacks: a chain-resident pass that fails its check ends the call in the loop -----------------------------------------------------------
@pytest.mark.parametrize('stage', [1, 2], ids=['forward_check', 'backward_check'])
def test_a_failed_check_ends_in_the_loop(hip_engine, stage, capfd):
    make, series = gaussian(128, 16, walk_mean()), values(3, 5, seed=41)
    hip_engine.set_option('chain_force_fail_batch', 0)
    hip_engine.set_option('chain_force_fail_stage', stage)
    try:
        R, k, err = fit_many(make, series, capfd)
    finally:
        hip_engine.set_option('chain_force_fail_batch', -1)
        hip_engine.set_option('chain_force_fail_stage', 0)
    assert err.count(NOTICE) == 1 and 'series fit:' in err and 'grid of 2 parameters' in err, err
    at_the_bar(R, golds_of('2d fallback', make, series))


def test_a_give_up_ends_in_the_loop(capfd):
    """stage 3: a give-up seen after the backward pass.  It parks the context's resident paths for the fits that follow, as a real one does
    (the loop's single fits run on the launch-per-step kernels): an engine of the test's own, so that no later test inherits that state"""
    make, series = gaussian(128, 16, walk_mean()), values(3, 5, seed=41)
    prev = bl.set_engine(None)
    try:
        eng = bl.get_engine()
        eng.set_option('chain_force_fail_batch', 0)
        eng.set_option('chain_force_fail_stage', 3)
        R, k, err = fit_many(make, series, capfd)
        assert err.count(NOTICE) == 1 and 'series fit:' in err and 'gave up' in err and 'grid of 2 parameters' in err, err
        at_the_bar(R, golds_of('2d fallback', make, series))
    finally:
        bl.set_engine(prev)


def test_option_series_fit_off_is_the_loop(hip_engine, capfd):
    make, series = gaussian(128, 16, walk_mean()), values(3, 5, seed=41)
    hip_engine.set_option('series_fit', 0)
    try:
        R, k, err = fit_many(make, series, capfd)
    finally:
        hip_engine.set_option('series_fit', 1)
    assert err.count(NOTICE) == 1 and 'series_fit' in err, err
    assert k.count.get(CHAIN, 0) == 2 * len(series), k.count          # (the loop: single fits of this shape run the chain kernel themselves, a launch per series and pass)
    at_the_bar(R, golds_of('2d fallback', make, series))


# ---- outside the envelope: the loop, with the reason, results at the bar ---------------------------------------------------------------------
def regime():
    return bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('sigma', 0.2, target='mean'), bl.tm.RegimeSwitch('log10pMin', -7))


@pytest.mark.parametrize('name, make, series, word', [
    ('regime switch', gaussian(33, 32, regime), values(3, 4, seed=43), 'RegimeSwitch'),
    ('scaled ar1 both', scaled_ar1(lambda: bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s0', 0.05, target='rho'),
                                                                           bl.tm.GaussianRandomWalk('s1', 0.1, target='sigma'))),
     values(3, 5, seed=47), 'walks on both parameters'),
    ('ragged', gaussian(128, 16, walk_mean()), [v[:n] for v, n in zip(values(3, 5, seed=53), (5, 3, 4))], 'different lengths'),
], ids=['regime_switch', 'scaled_ar1_both_axes', 'ragged'])
def test_calls_outside_the_envelope_take_the_loop(name, make, series, word, capfd):
    R, k, err = fit_many(make, series, capfd)
    assert err.count(NOTICE) == 1 and 'grid of 2 parameters' in err and word in err, err
    assert str(make().observationModel) in err
    assert launches(k, 'anchor_table_kernel') <= len(series), k.count      # (at most the loop's own single fits)
    at_the_bar(R, golds_of(('2d loop', name), make, series))
