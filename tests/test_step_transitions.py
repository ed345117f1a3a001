"""
The TRANSITION half of the fused step kernels on the MI355X -- the stencil, the clamp or the dense kernel that turns the previous state into
the prior of a step, and the bookkeeping sums that go with it -- cell by cell against tests/highprec.py: blk::step_kernel<100, 0 / 1, *> (walks,
clamp modes 1, 2, 3, the dense BivariateRandomWalk kernel, the AlphaStable stencil, the small spline shift, every source kind),
bl1c::chain1d_kernel (CL = 0, 1, 2; one and two cells per thread), bl1f::fused1d_kernel, bl1p::persist1d_kernel, blf::fast_step_kernel and
blm::mfma_step_kernel in every radius bucket from both sides, blh::hwide_kernel / vwide_kernel, the resident families with a table likelihood,
the plain path on grids with three and four parameters (bln::filter_axis_kernel, bln::step_kernel<BWD>, the stages ne_max / ne_invert / ne_clamp /
shift_axis_kernel), bln::chain_nd_kernel<BWD, 256 | 1024> and bl1c::chain1d_long_kernel<BWD, M, CL> in its four (M, CL) flavours.
Every comparison is worst(got, want, SLACK * bound) <= 1 over ALL cells with a bound COUNTED in tests/highprec.py (no literal tolerance); the
weights are the restated ones rounded to float64 (tests/test_host_logic.py holds the library's to them), never the library's own.  Problems,
drivers and references: tests/step_transition_cases.py, which tests/test_highprec.py runs through the float64 oracle at the same bounds.  What
is covered, what the card showed and which in-bounds changes these tests catch: tests/STEP_TRANSITIONS.md.
BLHIP_STEP_REPORT=<file> appends, per test, the instantiations that ran and the worst error / bound.
"""
import os
import re

import numpy as np
import pytest

import bayesloop_amd as bl
import highprec as hp
import step_transition_cases as sc
from conftest import kernel_census

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)]

WORST = {}
DEFAULTS = dict(chain_resident=1, resident=1, mfma=1, fast=1, chain1d=1, persist1d=1, fuse1d=8, chain_nd=1, chain1d_long=1)
# the instantiations that apply a transition to a table-likelihood fit, and the large-shift / stage kernels none of these problems may reach
WATCH = re.compile(r'^(blk::step_kernel<100,|blk::bigshift_kernel<|bl1c::chain1d_kernel<100,|bl1f::fused1d_kernel<100,|bl1p::persist1d_kernel<100,|'
                   r'blf::fast_step_kernel<100,|blm::mfma_step_kernel<100,|blh::hwide_kernel|blh::vwide_kernel|blr::resident_kernel<.*, true>$|'
                   r'blc::chain_kernel<.*, true>$|blc::chain_fold2_kernel<|blc::chainax_kernel<|bln::|bl1c::chain1d_long_kernel<)')


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
    path = os.environ.get('BLHIP_STEP_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write('%s\t%s\t%s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, text))


def _counts():
    return {name: c for c, name in kernel_census()}


class Options:
    def __init__(self, e, opts):
        self.e, self.opts = e, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.e.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.e.set_option(k, DEFAULTS[k])


COMBOS = [(name, kind) for name, c in sc.CASES.items() for kind in c['inputs']]


def test_every_watched_family_is_in_the_table():
    fams = {c['family'] for c in sc.CASES.values()}
    assert fams == {'generic', 'chain1d', 'fused1d', 'persist1d', 'fast', 'mfma', 'hwide', 'vwide', 'resident', 'chain', 'chainax', 'nd', 'chain_nd',
                    'chain1d_long'}
    for name, c in sc.CASES.items():
        assert set(sc.EXPECT[name]) == set(c['drivers']), name


@pytest.mark.parametrize('name,kind', COMBOS, ids=['%s-%s' % x for x in COMBOS])
def test_transitions_cell_by_cell(eng, name, kind):
    """every driver of the case: all posteriors, logEvidence, local_evidence and the means against the longdouble pass; the exact set of watched
    instantiations that ran"""
    case = sc.CASES[name]
    chk = sc.Check(name)
    for driver in case['drivers']:
        refs, ok = sc.reference(name, kind, driver)
        keep = [b for b, o in enumerate(ok) if o]
        assert len(keep) >= len(ok) - 1
        with Options(eng, case['opts']):
            before = _counts()
            got = sc.run_problem(eng, name, kind, driver, keep)
            after = _counts()
        ran = {k for k in after if after[k] > before.get(k, 0) and WATCH.match(k)}
        _report('ran %s' % driver, ', '.join(sorted(ran)))
        if ran != set(sc.EXPECT[name][driver]):
            chk.bad.append('%s %s %s: expected %s, ran %s' % (name, kind, driver, sorted(sc.EXPECT[name][driver]), sorted(ran)))
        sc.compare(chk, name, kind, driver, keep, got, refs)
    fam = case['family']
    WORST[fam] = max(WORST.get(fam, 0.0), chk.top)
    _report('worst ' + fam, '%.4f' % chk.top)
    print('%s %s: worst error / bound %.3f' % (name, kind, chk.top))
    assert not chk.bad, '\n'.join(chk.bad)
