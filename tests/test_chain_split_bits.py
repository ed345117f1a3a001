"""
The chain-resident path of two-parameter grids after the split of ChainRun::setup into a host-only route planner
(bayesloop_amd/csrc/blhip_chain_plan.hpp) and device steps (blhip_fit_paths.hpp) computes the bits, launches the kernels and accounts the
traffic of the commit before the split.  tests/golden/chain_split_parent.npz holds, per case, the results of a library built from that
commit on the same hardware (tests/golden/gen_chain_split_parent.py wrote it), the deterministic part of the fit's timing -- launches,
batches, kernel variants, fall-backs and the by-construction HBM bytes and flops, sums that fingerprint the route: the rounds, what
folds, what is shared -- and the kernels the fit launched with their counts (blhip_kernel_census before and after; the co-residency
probe, which runs by the clock, left out).  Every array must be np.array_equal (the posterior sequences: bit-equal by their SHA-256, see
DIGESTED), every figure and the census equal.

The cases cross the branches of the route: the two-chain fold, evidence-only and storing passes on an exact grid; a padded grid copied
out (depad) and folded; the table kernels exact (folding) and padded (stored, folded by accumulate_pad_kernel); 1024 rows; both axes with
the table of the even steps and with a transposed table; RegimeSwitch on an exact and on a 384-row grid; change points with the shared
and skipped prefix, evidence-only, and inside a filtering chain; carried partial accumulators over batches, and a batch repeated.

ORACLE_HELD: cases on which the parent commit's library does not agree with itself from process to process keep the exact route
fingerprint; their arrays are held to the float64 oracle at the suite's bar instead.
"""
import contextlib
import hashlib
import io
import json
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import chain_clamp_cases as cc
import compare
import context_history_cases as ch
import oracle_adapter as oa
from test_gpu_parity import _g2, _om2, _ill_tol, result_of
from test_kernel_sweep import _chain_sigmas

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'chain_split_parent.npz')

ARRAYS = ('logEvidence', 'localEvidence', 'logEvidenceList', 'posteriorMeanValues', 'hyperParameterDistribution', 'posteriorSequence')
COUNTS = ('forward_launches', 'backward_launches', 'batches', 'fwd_kernel_variant', 'bwd_kernel_variant', 'resident_fallbacks', 'resident_fallback_reason')
SUMS = ('fwd_hbm_bytes', 'bwd_hbm_bytes', 'fwd_flops', 'bwd_flops')
DEFAULTS = dict(max_batch=1024, fold_force_fail_batch=-1)
ORACLE_HELD = ()
# the posterior sequences of the 15 full fits are 3 MB together, more than a committed file may hold: the file keeps their shape and the
# SHA-256 of their bytes -- equal digests are equal bits, which np.array_equal follows from (every other array is kept in full)
DIGESTED = ('posteriorSequence',)


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.asarray('%s %s' % ('x'.join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest()))


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def _laplace(n0, n1):
    return _om2('Laplace', ('mu', ('cint', -5, 5, n0)), ('b', ('oint', 0, 3, n1)))


def _hyper(om, n0, lo, hi, target, seed, T=6, nk=6, **kw):
    return dict(study='HyperStudy', data=('series', seed, T), om=om, tm=('GRW', 'sigma', _chain_sigmas(nk, n0, lo, hi), target, None), **kw)


def _gauss(n0, n1, seed, **kw):
    return _hyper(_g2(n0, n1), n0, -8.0, 8.0, 'mean', seed, **kw)


def _study(n0, n1, seed):
    return dict(study='Study', data=('series', seed, 6), om=_g2(n0, n1), tm=('GRW', 'sigma', _chain_sigmas(6, n0, -8.0, 8.0)[0], 'mean', None))


def _both_axes(n0=100, n1=90, nk=8, T=4):
    """tests/test_kernel_sweep.py: AX_SWEEP's hyper-study -- two widths on the first parameter, one on the second"""
    r0 = 2 * nk - 8
    lat0, lat1 = 16.0 / (n0 - 1.0), 4.0 / (n1 + 1.0)
    return dict(study='HyperStudy', data=('series', 8000 + 13 * nk + 1 + 7, T), om=_g2(n0, n1),
                tm=('Combined', [('GRW', 's1', [(r0 - 1 - k) / 4.0 * lat0 for k in range(2)], 'mean', None), ('GRW', 's2', (r0 - 3) / 4.0 * lat1, 'std', None)]))


def _clamp(grid):
    return cc.study(grid, cc.model('walk_then_switch', cc.chain_sigmas(8, grid[0])[0], -7), cc.seed_of(grid, 8))


def _changepoints(tm, **kw):
    return dict(study='ChangepointStudy', data=('series_jump', 61, 8, 4, 2.0), om=_g2(128, 16), tm=tm, **kw)


FIVE = _hyper(_g2(128, 16), 128, -8.0, 8.0, 'mean', 7105)
FIVE['tm'] = ('GRW', 'sigma', [float(x) for x in np.linspace(0.05, 0.45, 5)], 'mean', None)

# case -> (definition, engine options of the fit)
CASES = {
    'gauss_128x16_hyper_fold2': (_gauss(128, 16, 7101), {}),
    'gauss_128x16_hyper_evidence': (_gauss(128, 16, 7101, fit=dict(evidenceOnly=True)), {}),
    'gauss_128x16_study': (_study(128, 16, 7102), {}),
    'pad_100x20_study_depad': (_study(100, 20, 7103), {}),
    'pad_100x20_hyper_fold2': (_gauss(100, 20, 7104), {}),
    'laplace_128x16_hyper': (_hyper(_laplace(128, 16), 128, -5.0, 5.0, 'mu', 7106), {}),
    'laplace_100x20_hyper': (_hyper(_laplace(100, 20), 100, -5.0, 5.0, 'mu', 7107), {}),
    'tall_1024x16_hyper': (_gauss(1024, 16, 7108), {}),
    'both_axes_100x90_hyper': (_both_axes(), {}),
    'both_axes_laplace_60x44': (dict(cases.CASES['laplace_grw_2d'], data=('series', 71, 8)), {}),
    'clamp_128x32': (_clamp(cc.EXACT[0]), {}),
    'clamp_rows384': (_clamp(cc.ROWS_384), {}),
    'changepoints_full': (_changepoints(('ChangePoint', 'tChange', [2, 3, 5, 6], None)), {}),
    'changepoints_evidence': (_changepoints(('ChangePoint', 'tChange', [2, 3, 5, 6], None), fit=dict(evidenceOnly=True)), {}),
    'changepoints_in_a_walk': (_changepoints(('Combined', [('GRW', 'sigma', 0.3, 'mean', None), ('ChangePoint', 'tChange', [2, 4, 6], None)])), {}),
    'hyper5_batches_of_2': (FIVE, dict(max_batch=2)),
    'hyper5_batch_repeated': (FIVE, dict(max_batch=2, fold_force_fail_batch=1)),
}


def collect(case):
    """fits the case on the library the engine has loaded -> {'<case>/<array>': values, '<case>/counts': COUNTS, '<case>/sums': SUMS,
    '<case>/census': the fit's kernels and launch counts as JSON}"""
    c, opts = CASES[case]
    eng = bl.get_engine()
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
            S = cases.build(bl, c)
            before = ch.census()
            S.fit(**cases.fit_kwargs(c))
            launched = ch.census_delta(before, ch.census())          # (before the posteriors are read: that launches the normalisation)
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])
    out = {}
    for key in ARRAYS:
        value = getattr(S, key, None)
        if value is None or (key.startswith('posterior') and c.get('fit', {}).get('evidenceOnly')):
            continue
        a = np.asarray(value, dtype=float)
        if a.size and key in DIGESTED:
            out['%s/%s.sha256' % (case, key)] = digest(a)
        elif a.size:
            out['%s/%s' % (case, key)] = a
    timing = S.lastTiming
    out['%s/counts' % case] = np.asarray([timing[k] for k in COUNTS], dtype=np.int64)
    out['%s/sums' % case] = np.asarray([timing[k] for k in SUMS], dtype=np.float64)
    out['%s/census' % case] = np.asarray(json.dumps(sorted(launched.items())))
    return out, S


def route_of(rec, case):
    return dict(zip(COUNTS, (int(x) for x in rec['%s/counts' % case]))), dict(zip(SUMS, (float(x) for x in rec['%s/sums' % case]))), \
        json.loads(str(rec['%s/census' % case]))


@pytest.mark.parametrize('case', sorted(CASES))
def test_results_launches_and_traffic_are_the_parent_commits(case):
    parent = np.load(GOLDEN)
    got, S = collect(case)
    want = {k: parent[k] for k in parent.files if k.startswith(case + '/')}
    assert sorted(got) == sorted(want)
    assert '%s/logEvidence' % case in want and '%s/localEvidence' % case in want
    got_route, want_route = route_of(got, case), route_of(want, case)
    print(case, got_route)
    assert got_route[0] == want_route[0]
    assert got_route[1] == want_route[1]                      # (deterministic sums of doubles: equal, not close)
    assert [tuple(x) for x in got_route[2]] == [tuple(x) for x in want_route[2]]
    arrays = sorted(k for k in want if k.rsplit('/', 1)[1] in ARRAYS)
    if case in ORACLE_HELD:
        c = CASES[case][0]
        with np.errstate(all='ignore'):
            ref = oa.run(c)
        res = result_of(S, c)
        gold = {k: np.asarray(ref[k]) for k in ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'logEvidenceList',
                                                'hyperParameterDistribution') if ref.get(k) is not None and k in res and len(np.atleast_1d(ref[k]))}
        compare.check(res, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
        return
    for k in arrays:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
    for k in sorted(k for k in want if k.endswith('.sha256')):
        assert str(got[k]) == str(want[k]), '%s: shape and SHA-256 of the bytes, got %s, want %s' % (k, got[k], want[k])
