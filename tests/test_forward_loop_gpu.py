"""
The step loop of the forward chain-resident kernel (blc::chain_kernel<NK, NTW, false, STORE, ...>, bayesloop_amd/csrc/blhip_chainres.hpp)
after its integer, address and control code changed -- the exponential of the recurrence's second difference behind a real branch, the
stores of a step addressed from ONE per-lane offset and a scalar base that walks from cell to cell, the unfiltered copy of a restart inside
its arm -- computes the bits of the commit before: no floating-point operation was touched.  tests/golden/forward_loop_parent.json holds,
per case, the SHA-256 of logEvidence, logEvidenceList, the posterior means and the (average) posterior sequence a library built from that
commit gave on the same hardware (tests/golden/gen_forward_loop_parent.py wrote it).  Every case also asserts the chain-resident route
(forward kernel variant 6, no fall-back) and holds the fit to the float64 oracle at compare.GPU_TOL.

All series have T = 8 with a missing observation in the middle and one at the end: the number of valid data dimensions changes three times
after the first step, so the branch around the exponential is TAKEN in mid-series, not only skipped.

The cases are the smallest shapes that reach each path of the loop:
  * geometries 128 x 16, 256 x 16, 512 x 32 (exact: one, two, four tiles per wave; two strips at 512 x 32) and 500 x 30 (padded: reflect1
    and the bounded reads);
  * ring lengths 6, 12 and 24 in ONE batch (band radii 3, 15, 39: first and last waves reflect; 24 is the widest band kept in registers;
    on 128 rows a radius above 16 leaves the wave's own rows in LDS);
  * the storing forward kernel in all three layouts -- 33 chains (layout 2: 8 pairs for the four-chain fold + an odd chain), 8 chains
    (layout 1: the two-chain fold), a plain Study that hands its posteriors out (layout 0, + the storing backward kernel);
  * the evidence-only forward kernel (it stores nothing);
  * a walk followed by a change point in one model: the only live use of the unfiltered arm and of a restart inside a filtering chain.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import oracle_adapter as oa
from test_gpu_parity import _g2, _ill_tol, result_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'forward_loop_parent.json')

T = 8
NAN_AT = [4, 7]                      # one missing observation in the middle, one at the end
LO, HI = -8.0, 8.0                   # the mean axis of _g2
OPTION_DEFAULTS = dict(resident=1)   # the library's defaults of the options a case sets
KEYS = ('logEvidence', 'logEvidenceList', 'posteriorMeanValues', 'posteriorSequence')


def _sigmas(n0, nks, per_ring):
    """per_ring walk widths for each ring length nk of `nks`, all with the SciPy radius int(4 sigma / lattice + 0.5) = 2 nk - 9 (one below the
    band radius 2 nk - 8 the kernel's ring of nk entries holds), interleaved so that every ring length appears in every part of the batch"""
    lattice = (HI - LO) / (n0 - 1.0)
    rows = [[(2 * nk - 9 + 0.01 * j) / 4.0 * lattice for nk in nks] for j in range(per_ring)]
    return [float(s) for row in rows for s in row]


def _hyper(n0, n1, seed, nchains, fit=None):
    sig = _sigmas(n0, (6, 12, 24), (nchains + 2) // 3)[:nchains]
    c = dict(study='HyperStudy', data=('series_nan', seed, T, NAN_AT), om=_g2(n0, n1), tm=('GRW', 'sigma', sig, 'mean', None))
    if fit:
        c['fit'] = dict(fit)
    return c


def _study(n0, n1, seed, nk):
    return dict(study='Study', data=('series_nan', seed, T, NAN_AT), om=_g2(n0, n1), tm=('GRW', 'sigma', _sigmas(n0, (nk,), 1)[0], 'mean', None))


CASES = {
    # storing forward kernel, layout 2 (>= 32 chains: the four-chain fold), every geometry
    'hyper33-128x16': _hyper(128, 16, 9101, 33),
    'hyper33-256x16': _hyper(256, 16, 9102, 33),
    'hyper33-512x32': _hyper(512, 32, 9103, 33),
    'hyper33-500x30-padded': _hyper(500, 30, 9104, 33),
    # ... layout 1 (8 chains: the two-chain fold)
    'hyper8-256x16': _hyper(256, 16, 9105, 8),
    'hyper8-500x30-padded': _hyper(500, 30, 9106, 8),
    # ... layout 0 (a plain Study: posteriors handed out, the storing backward kernel reads what the forward kernel stored)
    'study-128x16-ring24': _study(128, 16, 9107, 24),
    'study-256x16-ring12': _study(256, 16, 9108, 12),
    # (a single chain of radius <= 8 takes the time-resident kernel where its tiles fit the grid: that path is switched off for this case)
    'study-512x32-ring6': dict(_study(512, 32, 9109, 6), opts=dict(resident=0)),
    'study-500x30-padded-ring12': _study(500, 30, 9110, 12),
    # the forward kernel that stores nothing
    'evidence33-128x16': _hyper(128, 16, 9111, 33, fit=dict(evidenceOnly=True)),
    'evidence33-512x32': _hyper(512, 32, 9112, 33, fit=dict(evidenceOnly=True)),
    'evidence33-500x30-padded': _hyper(500, 30, 9113, 33, fit=dict(evidenceOnly=True)),
    # a restart inside a filtering chain: the change point comes after the walk in the model's list, its step takes the source unfiltered
    'walk-changepoint-256x16': dict(study='ChangepointStudy', data=('series_nan', 9114, T, NAN_AT), om=_g2(256, 16),
                                    tm=('Combined', [('GRW', 'sigma', _sigmas(256, (12,), 1)[0], 'mean', None),
                                                     ('ChangePoint', 'tChange', [2, 5, 6], None)])),
    'walk-changepoint-128x16-ring24': dict(study='ChangepointStudy', data=('series_nan', 9115, T, NAN_AT), om=_g2(128, 16),
                                           tm=('Combined', [('GRW', 'sigma', _sigmas(128, (24,), 1)[0], 'mean', None),
                                                            ('ChangePoint', 'tChange', [1, 4, 6], None)])),
}


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return '%s %s' % ('x'.join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest())


def collect(case):
    """fits the case on the library the engine has loaded -> ({key: shape and SHA-256 of the bytes}, the fit's timing, the study)"""
    c = CASES[case]
    eng = bl.get_engine()
    opts = c.get('opts', {})
    S = cases.build(bl, c)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        with np.errstate(all='ignore'):
            S.fit(**cases.fit_kwargs(c))
    finally:
        for k in opts:
            eng.set_option(k, OPTION_DEFAULTS[k])
    timing = dict(S.lastTiming)
    evid = c.get('fit', {}).get('evidenceOnly', False)
    out = {}
    for key in KEYS:
        value = getattr(S, key, None)
        if value is None or (evid and key.startswith('posterior')) or not np.size(value):
            continue
        out[key] = digest(np.asarray(value, dtype=float))
    return out, timing, S


def test_the_cases_are_the_ones_listed():
    assert len(CASES) == 15
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(CASES)


@pytest.mark.parametrize('case', sorted(CASES))
def test_route_oracle_and_the_parent_commits_bits(case):
    c = CASES[case]
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got, t, S = collect(case)
    print(case, {k: t[k] for k in ('fwd_kernel_variant', 'bwd_kernel_variant', 'resident_fallbacks', 'batches')}, got)
    assert t['fwd_kernel_variant'] == 6 and t['resident_fallbacks'] == 0, t
    with np.errstate(all='ignore'):
        ref = oa.run(c)
    res = result_of(S, c)
    gold = {k: np.asarray(ref[k]) for k in ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'logEvidenceList',
                                            'hyperParameterDistribution') if ref.get(k) is not None and k in res and len(np.atleast_1d(ref[k]))}
    compare.check(res, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    assert sorted(got) == sorted(want)
    assert 'logEvidence' in want and (c.get('fit', {}).get('evidenceOnly') or 'posteriorSequence' in want)
    for k in sorted(want):
        assert got[k] == want[k], '%s/%s: shape and SHA-256 of the bytes, got %s, want %s' % (case, k, got[k], want[k])
