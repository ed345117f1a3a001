"""The folding backward pass with FOUR chains per accumulator cell (blc::chain_fold2_kernel<NK, NTW, false, true>, blhip_chainres.hpp), on the GPU.

A block owns a strip of 8 grid columns of four chains; the stored states and the partial accumulators live in [t][strip of 8][row][8]; the
plan (blhip_chain_plan.hpp: chain_fold_plan) takes batches of at least fold4_min_chains chains (32; lowered here).  Held:
* parity with the oracle at the suite's bar and with the same fit on the two-chain kernel (fold4 = 0; not bit for bit: the order of the
  sums differs) for a full quad and every kind of odd end (4, 5, 6, 7, 9 chains), all chains with different bands; one case with a missing
  data point and a two-column record with one entry missing (the number of valid data dimensions changes along the series);
* every instantiation (ring lengths 6 .. 24 x 1 - 4 tiles per wave) launched once and compared with the oracle;
* a long series (26 steps, lag 4) against the longdouble reference through the driver of tests/test_likelihood_kernels.py, as
  tests/test_long_series.py runs the two-chain kernel;
* a call of three batches, two of them on this kernel and a last one too small for it: the carried partial accumulators are flushed between
  the layouts; the same call with a forced failure of the second batch's prediction check repeats on the launch-per-step kernels;
* identical bits from fit to fit in one process and in a fresh one.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import oracle_adapter as oa
from test_gpu_parity import result_of, _g2
from test_kernel_sweep import run, _counts, _chain_sigmas

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = dict(fold4=1, fold4_min_chains=32, max_batch=1024, fold_force_fail_batch=-1)


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


class options:
    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        for k, v in self.opts.items():
            bl.get_engine().set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            bl.get_engine().set_option(k, DEFAULT[k])


def quad(nk, ntw):
    return 'blc::chain_fold2_kernel<%d, %d, false, true>' % (nk, ntw)


def sigmas(radii, n0=128, lo=-8.0, hi=8.0):
    """walk widths whose SciPy radius int(4 sigma / lattice + 0.5) (transitionModels.py:108-111) is the given one"""
    lattice = (hi - lo) / (n0 - 1.0)
    return [r / 4.0 * lattice for r in radii]


RADII = [2, 5, 9, 14, 3, 7, 11, 19, 6]          # all different: both halves of a block and both of its pairs carry different bands
T_PARITY = 12


def parity_case(n, data=None):
    return dict(study='HyperStudy', data=('series', 4100 + n, T_PARITY) if data is None else data, om=_g2(128, 16),
                tm=('GRW', 'sigma', sigmas(RADII[:n]), 'mean', None))


def missing_data():
    x = cases.make_data(('series2d', 4177, T_PARITY)).copy()          # (two columns, entry [3, 1] missing)
    x[7, :] = np.nan                                                   # a missing data point
    return x


def ring(radius):
    return (16 + 2 * max(4, (radius + 3) // 4 * 4)) // 4


def fit(c):
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    return S, result_of(S, c)


def close_to_two_chain(got, c):
    with options(fold4=0):
        before = _counts()
        _, two = fit(c)
        after = _counts()
    ran = [k for k in after if after[k] > before.get(k, 0) and k.startswith('blc::chain_fold2_kernel<')]
    assert ran and not any(k.endswith(', true>') and k.count(',') == 3 for k in ran), ran
    assert abs(got['logEvidence'] - two['logEvidence']) <= 1e-12 * abs(two['logEvidence'])
    np.testing.assert_allclose(np.asarray(got['posteriorSequence']), np.asarray(two['posteriorSequence']), rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(got['posteriorMeanValues'], two['posteriorMeanValues'], rtol=1e-10)
    np.testing.assert_allclose(got['hyperParameterDistribution'], two['hyperParameterDistribution'], rtol=1e-11)
    np.testing.assert_allclose(np.asarray(got['logEvidenceList'], dtype=float), np.asarray(two['logEvidenceList'], dtype=float), rtol=1e-12)


@pytest.mark.parametrize('n', [4, 5, 6, 7, 9])
def test_parity_with_the_oracle_and_the_two_chain_kernel(n):
    c = parity_case(n)
    with options(fold4_min_chains=1):
        S = run(c, ['blc::chain_kernel<%d, 1, false, true, false, false>' % ring(max(RADII[:n])), quad(ring(max(RADII[:n])), 1)])
        got = result_of(S, c)
    close_to_two_chain(got, c)


def test_parity_with_missing_data():
    c = parity_case(6, missing_data())
    with options(fold4_min_chains=1):
        S = run(c, [quad(ring(max(RADII[:6])), 1)])
        got = result_of(S, c)
    close_to_two_chain(got, c)


def test_the_default_threshold_keeps_small_batches_on_the_two_chain_kernel():
    c = parity_case(5)
    before = _counts()
    fit(c)
    after = _counts()
    ran = sorted(k for k in after if after[k] > before.get(k, 0) and k.startswith('blc::chain_fold2_kernel<'))
    assert ran == ['blc::chain_fold2_kernel<%d, 1, false>' % ring(max(RADII[:5]))], ran


SWEEP = [(ntw, nk) for ntw in (1, 2, 3, 4) for nk in range(6, 26, 2)]


@pytest.mark.parametrize('ntw,nk', SWEEP, ids=['ntw%d-nk%d' % x for x in SWEEP])
def test_every_instantiation(ntw, nk):
    """grids of 128 ntw x 16, five chains (a quad and a single chain), six steps; the widest walk needs exactly the ring"""
    n0 = 128 * ntw
    r0 = 2 * nk - 8
    lattice = 16.0 / (n0 - 1.0)
    sig = [(r0 - 1 - k) / 4.0 * lattice for k in range(5)]
    assert sig[:3] == _chain_sigmas(nk, n0, -8.0, 8.0)
    c = dict(study='HyperStudy', data=('series', 7600 + 97 * nk + 11 * ntw, 6), om=_g2(n0, 16), tm=('GRW', 'sigma', sig, 'mean', None))
    with options(fold4_min_chains=1):
        run(c, ['blc::chain_kernel<%d, %d, false, true, false, false>' % (nk, ntw), quad(nk, ntw)])


def test_long_series_against_the_longdouble_reference(monkeypatch):
    """26 steps under a drive of period 6, lag 4 (the default): the scal[] ring wraps three times, every chain's scale is prepared by the scale
    wave two per pair-step; five chains = a quad and a single chain; bounds counted in tests/highprec.py, as for `chain_fold2`"""
    import long_series_cases as ls
    import test_likelihood_kernels as tl
    eng = bl.get_engine()

    def ran(rec, T, kind):
        assert rec and kind == 'fold'
        return {'blc::chain_kernel<8, 1, false, true, false, false>', quad(8, 1), 'blc::anchor_table_kernel'}
    fam = dict(tl.FAMILIES['chain_fold2'], opts={'fold4_min_chains': 1}, chains=[[(0, 7)], [(0, 6)], [(0, 5)], [(0, 3)], [(0, 2)]], ran=ran)
    monkeypatch.setitem(tl.FAMILIES, 'chain_fold4', fam)
    monkeypatch.setitem(tl.DEFAULTS, 'fold4_min_chains', 32)
    monkeypatch.setitem(ls.GAUSSIAN, 'chain_fold4', ls.GAUSSIAN['chain_fold2'])          # (the same scale rule: norm_lag(4))
    monkeypatch.setattr(tl, 'setup', lambda f, case, steps, full, cap: ls.gaussian_setup(f, case, full))
    name = 'jumping_period6'
    T = ls.SERIES[name][0]
    assert T == 26
    chk = tl.Check('long chain_fold4')
    tl.run_kind(eng, 'chain_fold4', name, tuple(range(T)), 'fold', chk)
    assert not chk.bad, '\n'.join(chk.bad[:30])


def carry_case():
    # 68 chains, at most 32 per batch: the library cuts even batches of a multiple of 8 chains -- 24, 24 and 20; with fold4_min_chains = 24 the
    # first two take the four-chain kernel and the last one, below the threshold, the two-chain kernel
    return dict(study='HyperStudy', data=('series', 4193, 8), om=_g2(128, 16), tm=('GRW', 'sigma', ('cint', 0.02, 0.9, 68), 'mean', None))


def test_batches_of_both_layouts_in_one_call_and_recovery():
    c = carry_case()
    with np.errstate(all='ignore'):
        want = oa.run(c)
    gold = {k: want[k] for k in ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues')}
    with options(max_batch=32, fold4_min_chains=24):
        before = _counts()
        A, got = fit(c)
        after = _counts()
        ran = {k for k in after if after[k] > before.get(k, 0) and k.startswith('blc::chain_fold2_kernel<')}
        assert any(k.count(',') == 3 for k in ran) and any(k.count(',') == 2 for k in ran), ran
        # the slots are flushed where the layout changes, and once more after the last batch
        assert A.lastTiming['batches'] == 3 and A.lastTiming['accumulate_launches'] == 2 and A.lastTiming['resident_fallbacks'] == 0, A.lastTiming
        compare.check({k: got[k] for k in gold}, gold, compare.GPU_TOL)
        with options(fold_force_fail_batch=1):
            B, gotB = fit(c)
            assert B.lastTiming['resident_fallbacks'] >= 1 and B.lastTiming['resident_fallback_reason'] == 3, B.lastTiming      # BLHIP_FALLBACK_PREDICTION
        compare.check({k: gotB[k] for k in gold}, gold, compare.GPU_TOL)
    assert abs(got['logEvidence'] - gotB['logEvidence']) <= 1e-12 * abs(got['logEvidence'])
    np.testing.assert_allclose(np.asarray(gotB['posteriorSequence']), np.asarray(got['posteriorSequence']), rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(gotB['hyperParameterDistribution'], got['hyperParameterDistribution'], rtol=1e-11)


def _bits(res):
    import hashlib
    h = hashlib.sha256()
    for k in ('posteriorSequence', 'localEvidence', 'posteriorMeanValues', 'hyperParameterDistribution', 'logEvidenceList'):
        h.update(np.ascontiguousarray(np.asarray(res[k], dtype=np.float64)).tobytes())
    h.update(np.float64(res['logEvidence']).tobytes())
    return h.hexdigest()


FRESH = '''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bayesloop_amd as bl
bl.set_engine(None)
import test_fold4_gpu as t
with t.options(fold4_min_chains=1):
    print('BITS', t._bits(t.fit(t.parity_case(7))[1]))
'''


def test_identical_bits_from_fit_to_fit_and_in_a_fresh_process():
    c = parity_case(7)
    with options(fold4_min_chains=1):
        first = _bits(fit(c)[1])
        fit(parity_case(9))                       # (another batch between the two: granules, slots and tables of the context are reused)
        second = _bits(fit(c)[1])
    assert first == second
    out = subprocess.run([sys.executable, '-c', FRESH % (ROOT, os.path.join(ROOT, 'tests'))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = [l.split()[1] for l in out.stdout.splitlines() if l.startswith('BITS')]
    assert fresh == [first], (fresh, first)
