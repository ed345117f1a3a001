"""
Deterministic shifts beyond 12 grid cells per time step on 2-D grids, on the MI355X: such a shift runs as a stage of its own,
blk::bigshift_kernel<AXIS, BWD> (DESIGN.md "Large shifts on 2-D grids"), in front of the other stages and the fused step kernel.  The
fixtures of tests/bigshift_cases.py through the HIP library, at the bars of tests/test_bigshift_oracle.py (compare.GPU_TOL with the
registered FFT_FLOOR); every case asserts through the kernel census that the expected instantiations of the kernel ran -- forward, and
backward for full fits, per shifted axis -- and the control (8 cells per step) that none did and that it ran as a single-stage program.
(Without the kernel every non-control case is refused at fit time with a BackendError.)
"""
import numpy as np
import pytest

import bayesloop_amd as bl
import bigshift_cases as bc
import compare
import oracle_adapter as oa
from conftest import kernel_census
from test_bigshift_oracle import check_direct
from test_combined_models_oracle import result_of, fit_case, run_online, check_online

pytestmark = pytest.mark.gpu

BIG = {(ax, bwd): 'blk::bigshift_kernel<%d, %s>' % (ax, 'true' if bwd else 'false') for ax in (0, 1) for bwd in (False, True)}
STAGE_FWD, STAGE_BWD = 'blk::step_kernel<100, 2, false>', 'blk::step_kernel<100, 3, false>'


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def _counts():
    return {name: c for c, name in kernel_census()}


def _ran(before, after):
    return {k for k in after if after[k] > before.get(k, 0)}


def expected_kernels(c):
    fit = c.get('fit', {})
    full = not (fit.get('evidenceOnly') or fit.get('forwardOnly'))
    return [BIG[(ax, bwd)] for ax in c['axes'] for bwd in ((False, True) if full else (False,))]


@pytest.mark.parametrize('case', sorted(bc.BIGSHIFT))
def test_large_shift_matches_reference(case):
    c = bc.BIGSHIFT[case]
    before = _counts()
    S = fit_case(c)
    got = result_of(S, c)
    ran = _ran(before, _counts())
    missing = [k for k in expected_kernels(c) if k not in ran]
    assert not missing, 'large-shift kernel(s) not launched: %s; launched: %s' % (missing, sorted(ran))
    unexpected = [k for k in BIG.values() if k in ran and k not in expected_kernels(c)]
    assert not unexpected, 'large-shift kernel(s) launched for an axis / direction the case does not have: %s' % unexpected
    compare.check(got, oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', sorted(bc.CONTROL))
def test_small_shift_launches_no_large_shift_kernel(case):
    """8 cells per step: the single-stage program of the generic step kernel (its small-shift stencil), as before"""
    c = bc.CONTROL[case]
    before = _counts()
    S = fit_case(c)
    got = result_of(S, c)
    ran = _ran(before, _counts())
    assert not [k for k in BIG.values() if k in ran], sorted(ran)
    assert STAGE_FWD not in ran and STAGE_BWD not in ran, sorted(ran)
    assert 'blk::step_kernel<2, 0, false>' in ran and 'blk::step_kernel<2, 1, true>' in ran, sorted(ran)
    compare.check(got, oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', sorted(bc.ONLINE))
def test_large_shift_in_online_study(case):
    """resumed one-step problems with carried states (OnlineStudy.step): forward only"""
    before = _counts()
    S = run_online(bc.ONLINE[case])
    ran = _ran(before, _counts())
    assert BIG[(0, False)] in ran, sorted(ran)
    gold = oa.load_golden(case)
    check_online(S, gold, int(gold['n_models']))


@pytest.mark.parametrize('name', sorted(bc.direct_calls(bl)))
def test_large_shift_direct_calls(name):
    """the built-in model's own computeForwardPrior / computeBackwardPrior (one-step device programs)"""
    before = _counts()
    check_direct(name)
    ran = _ran(before, _counts())
    ax = 0 if name.endswith('axis0') else 1
    assert BIG[(ax, False)] in ran, sorted(ran)


def test_shift_beyond_the_line_limit_is_refused_with_the_limit():
    """an axis longer than one block's LDS holds: the refusal names the limit (16 384 points)"""
    om = ('Gaussian', [('mean', ('cint', -3, 3, 4)), ('std', ('oint', 0.1, 3, 16385))], 'default')
    c = dict(study='Study', data=('series', 215, 3), om=om, tm=('Deterministic', 'bs_std_long', 'std'), fit=dict(evidenceOnly=True))
    with pytest.raises(bl.BackendError, match='16384'):
        fit_case(c)
