"""
The kernels that carry a lazily scaled state ALONG TIME on the MI355X, over 14 and 26 steps, cell by cell against tests/highprec.py: the lagged
normalisers of the chain-resident family (blc::chain_kernel, chainax_kernel: the scale wave, the ring of NSLOT = 8 slots behind its wrap, restarts)
and of blr::resident_kernel (the lagged SUM, marginally stable), the launch boundaries of bl1f::fused1d_kernel and bl1p::persist1d_kernel, the
forward sums bl1c::chain1d_kernel / chain1d_long_kernel read at every backward step, with blk::step_kernel as the control.  The likelihood of step t
is 2^(e_t) y_t: the schedule e_t moves the normalisers -- to either side of the hosts' guards, on purpose -- and leaves the reference's posteriors
alone.  Every comparison is worst(got, want, SLACK * bound) <= 1 over ALL cells with the bound of tests/highprec.py under the family's own scale
rule (tests/scale_rules.py); the weights are the restated ones rounded to float64.  Whether a guard fires is PREDICTED from the reference's
normalisers (tests/long_series_cases.py) and asserted through resident_fallbacks / resident_fallback_reason, the launch counts and the census.
Problems, schedules and predictions: tests/long_series_cases.py, which tests/test_highprec.py runs through the float64 oracle at the same bounds.
What is covered, what the card showed: tests/LONG_SERIES.md.  BLHIP_LONG_REPORT=<file> appends, per test, the instantiations that ran and the
worst error / bound.
"""
import os
import re

import pytest

import bayesloop_amd as bl
import highprec as hp
import long_series_cases as ls
import step_transition_cases as sc
from conftest import kernel_census
from test_step_transitions import WATCH, Options

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)]

WORST = {}
LAG_DEFAULTS = dict(chain_resident_lag=4, resident_lag=2)
FALLBACK_RANGE = 2                                                  # BLHIP_FALLBACK_RANGE (include/blhip.h)
# where a range fallback lands: the launch-per-step kernels of a table-likelihood fit
LAUNCH_PER_STEP = re.compile(r'^(blk::step_kernel<100,|blf::fast_step_kernel<100,|blm::mfma_step_kernel<100,|blh::hwide_kernel|blh::vwide_kernel)')
RESIDENT_RULES = ('norm_lag', 'sum_lag')


@pytest.fixture(scope='module')
def eng():
    prev = bl.set_engine(None)
    e = bl.get_engine()
    assert type(e).__name__ == 'HipEngine'
    yield e
    bl.set_engine(prev)
    for k in sorted(WORST):
        print('worst error / bound, %s: %.3f' % (k, WORST[k]))
        _report('worst', '%s %.4f' % (k, WORST[k]))


def _report(what, text):
    path = os.environ.get('BLHIP_LONG_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write('%s\t%s\t%s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, text))


def _counts():
    return {name: c for c, name in kernel_census()}


def _run(eng, fam, schedule, full=True, rule=None):
    R = ls.reference(fam, schedule, full=full, rule=rule)
    assert R['verdict'] != 'refused', (fam, schedule, R['fwd'], R['bwd'])            # (long_series_cases.REFUSED names them; none is run)
    assert len(R['keep']) >= len(R['refs']) - 1
    T = ls.steps_of(schedule)
    chk = sc.Check('%s %s' % (fam, schedule))
    what = '%s %s %s' % (fam, schedule, 'full' if full else 'forward')
    with Options(eng, sc.CASES[ls.FAMILIES[fam]['case']]['opts']):
        before = _counts()
        got = ls.run_problem(eng, fam, schedule, R['keep'], full=full)
        after = _counts()
    delta = {k: after[k] - before.get(k, 0) for k in after if after[k] > before.get(k, 0)}
    ran = {k for k in delta if WATCH.match(k)}
    _report('ran ' + what, ', '.join(sorted(ran)))
    expect = ls.expected(fam, full)
    tm = got['timing'][0]
    kind = R['rule'][0]
    if R['verdict'] == 'range':
        # the rule of tests/test_likelihood_kernels.py for a fit that leaves a resident path half way: something watched ran, then the launch-per-step flavours
        if not (ran & expect and ran - expect and all(LAUNCH_PER_STEP.match(k) for k in ran - expect)):
            chk.bad.append('%s: predicted a range fallback from %s to the launch-per-step kernels, ran %s' % (what, sorted(expect), sorted(ran)))
        if not (tm['resident_fallbacks'] >= 1 and tm['resident_fallback_reason'] == FALLBACK_RANGE):
            chk.bad.append('%s: predicted BLHIP_FALLBACK_RANGE (sums %r), timing says fallbacks %r reason %r' %
                           (what, R['fwd'], tm['resident_fallbacks'], tm['resident_fallback_reason']))
    else:
        if ran != expect:
            chk.bad.append('%s: expected %s, ran %s' % (what, sorted(expect), sorted(ran)))
        if kind in RESIDENT_RULES and tm['resident_fallbacks'] != 0:
            chk.bad.append('%s: predicted no fallback (sums %r / %r), timing says fallbacks %r reason %r' %
                           (what, R['fwd'], R['bwd'], tm['resident_fallbacks'], tm['resident_fallback_reason']))
    if kind == 'launch':
        fwd_kernel = next(k for k in expect if k.endswith('false>'))
        if delta.get(fwd_kernel, 0) != ls.forward_launches(fam, T, R['verdict']):
            chk.bad.append('%s: %d launches of %s, predicted %d (%s)' % (what, delta.get(fwd_kernel, 0), fwd_kernel, ls.forward_launches(fam, T, R['verdict']),
                                                                       'repeated with one step per launch' if R['verdict'] == 'repeat' else 'no repeat'))
    ls.compare(chk, fam, schedule, R['keep'], got, R['refs'], full=full)
    key = '%s %s%s' % (fam, schedule, '' if full else ' forward')
    WORST[key] = max(WORST.get(key, 0.0), chk.top)
    _report('worst ' + key, '%.4f %s' % (chk.top, R['verdict']))
    print('%s (%s): worst error / bound %.3f' % (what, R['verdict'], chk.top))
    assert not chk.bad, '\n'.join(chk.bad[:30])


FULL, FORWARD, LAGS = ls.combinations(), ls.forward_combinations(), ls.lag_combinations()


def test_every_family_and_schedule_is_run_or_named():
    assert set(ls.FAMILIES) == {'resident', 'chain', 'chain_sources', 'chainax', 'chain1d_walks', 'chain1d_shifts', 'chain1d_long', 'fused1d', 'persist1d', 'generic'}
    assert set(ls.SCHEDULES) == {'flat', 'ramp', 'ramp_80', 'burst_in', 'burst_out', 'burst_mild', 'alternate', 'resonant_in', 'resonant_out'}
    assert sorted(set(ls.combinations(refused=True)) - set(FULL)) == sorted(ls.REFUSED)


@pytest.mark.parametrize('fam,schedule', FULL, ids=['%s-%s' % x for x in FULL])
def test_long_series_cell_by_cell(eng, fam, schedule):
    """a full fit: all posteriors, logEvidence, local_evidence and the means against the longdouble pass under the family's scale rule; the
    predicted fallback or repeat; the exact set of watched instantiations that ran"""
    _run(eng, fam, schedule)


@pytest.mark.parametrize('fam,schedule', FORWARD, ids=['%s-%s' % x for x in FORWARD])
def test_long_series_forward_only(eng, fam, schedule):
    """the forward-only fit (the time-resident kernel normalises its rows `lag` steps behind and leaves the last `lag` to the host)"""
    _run(eng, fam, schedule, full=False)


@pytest.mark.parametrize('fam,schedule,rule', LAGS, ids=['%s-%s-lag%d' % (f, s, r[1]) for f, s, r in LAGS])
def test_long_series_lag_sweep(eng, fam, schedule, rule):
    """the same fits at the other lags the kernels take, each against the bound and the prediction of ITS rule"""
    opt = ls.LAG_OPTION[rule[0]]
    eng.set_option(opt, rule[1])
    try:
        _run(eng, fam, schedule, rule=rule)
    finally:
        eng.set_option(opt, LAG_DEFAULTS[opt])


# ---- the Gaussian families: the problems of tests/test_likelihood_kernels.py over long series -----------------------------------------------------------

GAUSS = [c for c in ls.gaussian_combinations() if c[0] != 'chain_clamp']
CLAMPED = [c for c in ls.gaussian_combinations() if c[0] == 'chain_clamp']


@pytest.mark.parametrize('fam,name', GAUSS, ids=['%s-%s' % x for x in GAUSS])
def test_gaussian_long_series(eng, monkeypatch, fam, name):
    """every kind of fit the family has (full and forward-only or evidence-only; chain_fold2: the folded batch), through the driver, the
    comparisons and the census of tests/test_likelihood_kernels.py, with the long series and the reference under the family's scale rule in the
    place of its three records.  No series leaves a guard (asserted on the CPU), so the census is the exact set of the family's own kernels."""
    import test_likelihood_kernels as tl
    monkeypatch.setattr(tl, 'setup', lambda f, case, steps, full, cap: ls.gaussian_setup(f, case, full))
    T = ls.SERIES[name][0]
    chk = tl.Check('long ' + fam)
    for kind in tl.FAMILIES[fam]['kinds']:
        tl.run_kind(eng, fam, name, tuple(range(T)), kind, chk)
    key = 'gaussian %s %s' % (fam, name)
    WORST[key] = chk.top
    _report('worst ' + key, '%.4f none' % chk.top)
    assert not chk.bad, '\n'.join(chk.bad[:30])


@pytest.mark.parametrize('fam,name', CLAMPED, ids=['%s-%s' % x for x in CLAMPED])
def test_gaussian_long_series_clamped(eng, fam, name):
    """blc::chain_clamp_kernel as tests/test_chain_clamp_bounds.py runs it (chain_clamp = 2; a full fit and an evidence-only one), over the long
    series: every step behind the first waits for the sum before it and runs at the exact scale, which the lagged rule of the steps behind reads"""
    import chain_clamp_cases as cc
    import test_likelihood_kernels as tl
    T = ls.SERIES[name][0]
    shape = ls.CLAMP_SHAPE
    chk = tl.Check('long ' + fam)
    for kind in ('full', 'evidence'):
        full = kind == 'full'
        problem, values, refs, liks, rec_ok = ls.gaussian_setup(fam, name, full)
        ref = refs[0]
        assert rec_ok and tl.aborted_at(ref) is None
        before = _counts()
        eng.set_option('chain_clamp', 2)
        try:
            res = eng.fit(problem, values, keep_posterior=True) if full else eng.fit(problem, values, evidence_only=True)
            post = eng.posterior(0, T, list(shape)) if full else None
        finally:
            eng.set_option('chain_clamp', 1)
        after = _counts()
        ran = {k for k in after if after[k] > before.get(k, 0)}
        _report('ran %s %s %s' % (fam, name, kind), ', '.join(sorted(ran)))
        missing = [k for k in cc.kernels_of(8, cc.ntw_of(shape[0]), kind) if k not in ran]
        if missing or any(k.startswith('blk::step_kernel<') for k in ran) or res.timing['resident_fallbacks'] != 0:
            chk.bad.append('%s %s: expected %s and no fallback, ran %s (fallbacks %r)' % (name, kind, missing, sorted(ran), res.timing['resident_fallbacks']))
        w = '%s %s' % (name, kind)
        assert res.abort_step[0] < 0, res.abort_step
        chk.within([res.log_evidence[0]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
        for t in range(T):
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            chk.local(res.local_evidence[0, t], loc[0], loc[1], w + ' localEvidence[%d]' % t)
            if full:
                chk.within(post[t], ref['post'][t][0], ref['post'][t][1], w + ' posterior[%d]' % t)
                if res.posterior_mean is not None:
                    chk.within(res.posterior_mean[0, :, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)
    key = 'gaussian %s %s' % (fam, name)
    WORST[key] = chk.top
    _report('worst ' + key, '%.4f none' % chk.top)
    assert not chk.bad, '\n'.join(chk.bad[:30])
