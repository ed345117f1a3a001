"""
Rounding bounds of blc::chain_clamp_kernel (bayesloop_amd/csrc/blhip_chainclamp.hpp): one clamped fit per geometry -- 128 / 256 / 512 rows,
exact and padded -- held to the longdouble restatement with running bounds of tests/highprec.py, hp.gaussian_fit(..., clamp=...), exactly as
the `generic` family of tests/test_likelihood_kernels.py holds blk::step_kernel to it: that file's problem construction (setup), its
comparisons (Check) and its slack (hp.SLACK), nothing looser.  A walk of radius 7 on the first parameter followed by a RegimeSwitch at
log10pMin = -7 (clamp mode 2), T = 3, as a full fit and evidence-only.  The recurrence's bound is stated for the kernel's own anchors: one
per wave and step, 4 NTW - 1 steps of 4 rows behind it.  See tests/CHAIN_CLAMP.md.
"""
import numpy as np
import pytest

import bayesloop_amd as bl
import chain_clamp_cases as cc
import highprec as hp
import test_likelihood_kernels as tlk
from conftest import kernel_census

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)]

GEOMETRIES = [(128, 32), (256, 32), (512, 32), (100, 40), (200, 40), (400, 40)]
RADIUS, PMIN, STEPS = 7, -7.0, (0, 1, 2)


@pytest.fixture(scope='module')
def eng():
    prev = bl.set_engine(None)
    e = bl.get_engine()
    assert type(e).__name__ == 'HipEngine'
    yield e
    e.set_option('chain_clamp', 1)
    bl.set_engine(prev)


def _counts():
    return {name: c for c, name in kernel_census()}


@pytest.mark.parametrize('case', ['inside_wide_1', 'inside_1'])
@pytest.mark.parametrize('shape', GEOMETRIES, ids=['%dx%d' % g for g in GEOMETRIES])
def test_clamped_fits_stay_inside_the_rounding_bounds(eng, monkeypatch, shape, case):
    ntw = cc.ntw_of(shape[0])
    fam = 'chain_clamp_%dx%d' % shape
    monkeypatch.setitem(tlk.FAMILIES, fam, dict(shape=shape, opts={}, chains=[[(0, RADIUS)]], clamp=PMIN, rec=(4, 4 * ntw - 1, (1,)), ran=None,
                                                kinds=('full', 'evidence')))
    T = len(STEPS)
    chk = tlk.Check(fam)
    for kind in ('full', 'evidence'):
        full = kind == 'full'
        problem, values, refs, liks, rec_ok = tlk.setup(fam, case, STEPS, full, 1e150)
        assert rec_ok, 'the case lies outside the recurrence: the resident kernels would not take it'
        ref = refs[0]
        assert tlk.aborted_at(ref) is None
        before = _counts()
        eng.set_option('chain_clamp', 2)
        try:
            res = eng.fit(problem, values, keep_posterior=True) if full else eng.fit(problem, values, evidence_only=True)
            post = eng.posterior(0, T, list(shape)) if full else None
        finally:
            eng.set_option('chain_clamp', 1)
        after = _counts()
        ran = {k for k in after if after[k] > before.get(k, 0)}
        missing = [k for k in cc.kernels_of(8, ntw, kind) if k not in ran]
        assert not missing, 'expected kernel(s) not launched: %s (launched: %s)' % (missing, sorted(ran))
        assert not any(k.startswith('blk::step_kernel<') for k in ran), sorted(ran)
        w = '%s %s' % (case, kind)
        assert res.abort_step[0] < 0, res.abort_step
        chk.within([res.log_evidence[0]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
        for t in range(T):
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            chk.local(res.local_evidence[0, t], loc[0], loc[1], w + ' localEvidence[%d]' % t)
            if full:
                chk.within(post[t], ref['post'][t][0], ref['post'][t][1], w + ' posterior[%d]' % t)
                if res.posterior_mean is not None:
                    chk.within(res.posterior_mean[0, :, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)
    chk.done()
