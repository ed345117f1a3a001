"""
The Gaussian likelihood inside the fused step kernels on the MI355X, cell by cell against tests/highprec.py: the multiplicative recurrence
(mantissa * 2^exponent, re-anchored with blmath::exp_mn; the reciprocal recurrence for p / L) of blf::fast_step_kernel,
blm::mfma_step_kernel, blr::resident_kernel, blc::chain_kernel (in-kernel anchors and blc::anchor_table_kernel), blc::chain_fold2_kernel and
blc::chainax_kernel, and the per-cell exponential of their REC = false flavours, of blk::step_kernel<2, ..> and of the GaussianMean model of
the 1-D kernels.  Every comparison is worst(got, want, bound) <= 1 with a bound COUNTED in tests/highprec.py (no literal tolerance); what is
covered, what the card showed and which in-bounds changes of the kernels these tests catch: tests/LIKELIHOOD_KERNELS.md.

Small fits at engine level (FitProblem), T = 1, 2, 3.  The prior is the reciprocal of the true likelihood of step 0 (clipped to the float64
range, 1 where the likelihood rounds to 0): prior * L is O(1) wherever L is a normal number, so every cell of the T = 1 forward-only
posterior shows the relative error of its own L, and where every value inside the bound rounds to 0 the output must be exactly 0.  The
T = 2 and 3 fits check the backward side: posteriors, sum p / L through localEvidence (NaN exactly where the reference divides 0 by 0), the
means.  A step whose reference normaliser is 0 must abort there (core.py:390-400) -- not produce inf or NaN.  Inputs: tests/likelihood_cases.py.
Every engine call takes census deltas and asserts which of the watched instantiations ran.  BLHIP_LIKELIHOOD_REPORT=<file> appends, per test,
the instantiations that ran and the worst error / bound.
"""
import os
import re

import numpy as np
import pytest

import bayesloop_amd as bl
import highprec as hp
import likelihood_cases as lc
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem
from conftest import kernel_census
from oracle import bl_oracle as bo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)]

WORST = {}
DEFAULTS = dict(chain_resident=1, resident=1, mfma=1, chain1d=1, persist1d=1, fuse1d=8)
# the instantiations that evaluate a Gaussian likelihood (the tabulated flavours -- last template argument true -- read a table instead)
WATCH = re.compile(r'^(blf::fast_step_kernel<2,|blm::mfma_step_kernel<2,|blr::resident_kernel<.*, false>$|blc::chain_kernel<.*, false>$|'
                   r'blc::chain_fold2_kernel<|blc::chainax_kernel<|blc::anchor_table_kernel|blc::ax_lik_table_kernel|blk::step_kernel<2,|'
                   r'bl1c::chain1d_kernel<3,|bl1c::lik1d_table_kernel<3>|bl1f::\w+<3,|bl1p::\w+<3,)')


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
    path = os.environ.get('BLHIP_LIKELIHOOD_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write('%s\t%s\t%s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, text))


def _counts():
    return {name: c for c, name in kernel_census()}


def recurrence_flavour(name):
    """True / False: the instantiation evaluates the likelihood by the recurrence / by one exponential per cell; None: neither (a table builder)"""
    args = [a.strip() for a in name[name.index('<') + 1:-1].split(',')] if '<' in name else []
    if name.startswith('blf::fast_step_kernel'):
        return args[4] == 'true'
    if name.startswith('blm::mfma_step_kernel'):
        return args[3] == 'true'
    if name.startswith(('blk::step_kernel', 'bl1')):
        return False
    if name.startswith('blc::ax_lik_table_kernel'):
        return None
    return True


class Census:
    """with Census(expect): ...  -- asserts on exit that exactly the `expect`ed ones of the watched instantiations ran.  flavour = True / False
    instead (a fit that stops at a zero normaliser leaves a resident path half way and repeats on the launch-per-step kernels, so the set
    depends on where it stops): something watched ran, and everything that ran has this recurrence flavour -- the routing that matters"""

    def __init__(self, expect, what='', chk=None, flavour=None):
        self.expect, self.what, self.chk, self.flavour = set(expect), what, chk, flavour

    def __enter__(self):
        self.before = _counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        after = _counts()
        ran = {k for k in after if after[k] > self.before.get(k, 0)}
        watched = {k for k in ran if WATCH.match(k)}
        _report('ran ' + self.what, ', '.join(sorted(watched)))
        msg = '%s: expected %s, ran %s (all launches: %s)' % (self.what, sorted(self.expect), sorted(watched), sorted(ran))
        if self.flavour is not None:
            wrong = sorted(k for k in watched if recurrence_flavour(k) not in (None, self.flavour))
            ok = bool(watched) and not wrong
            msg = '%s: expected kernels with REC = %s only, ran %s' % (self.what, self.flavour, sorted(watched))
        else:
            ok = watched == self.expect
        if self.chk is not None and not ok:
            self.chk.bad.append(msg)                     # (collected: the comparisons of the call are still made)
            return False
        assert ok, msg
        return False


class Options:
    def __init__(self, e, opts):
        self.e, self.opts = e, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.e.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.e.set_option(k, DEFAULTS[k])


def b(v):
    return 'true' if v else 'false'


# ---- the families: the smallest problem that selects each (options and geometries of tests/test_kernel_sweep.py) ---------------------------
# shape; uneven mean grid; engine options; per chain the walks [(axis, radius in cells: sigma = (radius - 1/4) / 4 lattice)]; the recurrence's
# (stride, steps between anchors - 1, directions) for the bound; what runs per kind of fit and flavour (rec: the recurrence was accepted).

# The rules behind the expected sets: in the launch-per-step families the steps WITHOUT
# a stencil -- step 0 forward, the last step backward -- go to the streaming kernel (radius bucket 0), the steps between to the family's
# kernel; a resident family beyond the recurrence's envelope falls to the launch-per-step kernels; a chain-resident geometry takes the ring
# length of the widest band its steps need (T = 1 has none).

def lps(rec, T, kind, mf=None):
    """the launch-per-step kernels of a fit: blf::fast_step_kernel for the steps without a stencil, `mf` (a pattern with the pass) for the others"""
    f = 'blf::fast_step_kernel<2, %%d, 0, false, %s>' % b(rec)
    out = {f % 0}
    if T > 1:
        out.add((mf or f) % 0)
    if kind in ('full', 'fold'):
        out.add(f % 1)
        if T > 1:
            out.add((mf or f) % 1)
    return out


def _fast(rec, T, kind):
    return lps(rec, T, kind)


def _mfma(lean, h=False):
    def f(rec, T, kind):
        return lps(rec, T, kind, 'blm::mfma_step_kernel<2, %%d, 8, %s, %s, %s>' % (b(rec), b(h), b(lean)))
    return f


def _resident(tr, tc, pad):
    def f(rec, T, kind):
        if not rec:
            return _mfma(False, True)(False, T, kind)
        k = 'blr::resident_kernel<%d, %d, 8, 8, %%s, %%d, %s, false>' % (tr, tc, b(pad))
        return {k % ('false', 0 if pad else 3)} if kind == 'forward' else {k % ('false', 0 if pad else 2), k % ('true', 0)}
    return f


def _chain(radius, pad):
    def f(rec, T, kind):
        if not rec:
            return lps(False, T, kind, ('blm::mfma_step_kernel<2, %%d, 8, false, false, %s>' % b(not pad)) if radius else None)
        nk = 4 if radius == 0 else (8 if T > 1 else 6)
        k = 'blc::chain_kernel<%d, 1, %%s, %%s, %s, false>' % (nk, b(pad))
        tab = {'blc::anchor_table_kernel'} if radius else set()
        if kind == 'evidence':
            return {k % ('false', 'false')} | tab
        if kind == 'full':
            return {k % ('false', 'true'), k % ('true', 'true')} | tab
        return {k % ('false', 'true'), 'blc::chain_fold2_kernel<%d, 1, %s>' % (nk, b(pad))} | tab
    return f


def _chainax(rec, T, kind):
    if not rec or T == 1:                # (T = 1: no transition, nothing for the transposing kernels to do)
        return lps(rec, T, kind, 'blm::mfma_step_kernel<2, %d, 8, false, true, false>')
    k = 'blc::chainax_kernel<8, 1, %s, %s, true>'
    tab = {'blc::ax_lik_table_kernel'}
    return ({k % ('false', 'false')} if kind == 'evidence' else {k % ('false', 'true'), k % ('true', 'true')}) | tab


def _generic(rec, T, kind):
    k = 'blk::step_kernel<2, %d, %s>'
    return {k % (0, 'true')} if kind == 'forward' else {k % (0, 'false'), k % (1, 'true')}


OFF = dict(chain_resident=0, resident=0)
ONE = ('forward', 'full')
FAMILIES = {
    'fast_rec': dict(shape=(140, 90), opts=dict(OFF, mfma=0), chains=[[]], rec=(1, 15, (1,)), ran=_fast, kinds=ONE),
    'fast_exp': dict(shape=(140, 90), uneven=True, opts=dict(OFF, mfma=0), chains=[[]], rec=None, ran=_fast, kinds=ONE),
    'mfma_rec': dict(rec_also=(1, 15, (1,)), shape=(140, 90), opts=OFF, chains=[[(0, 7)]], rec=(4, 15, (1,)), ran=_mfma(False), kinds=ONE),
    'mfma_exp': dict(shape=(140, 90), uneven=True, opts=OFF, chains=[[(0, 7)]], rec=None, ran=_mfma(False), kinds=ONE),
    'mfma_lean_rec': dict(rec_also=(1, 15, (1,)), shape=(128, 64), opts=OFF, chains=[[(0, 7)]], rec=(4, 15, (1,)), ran=_mfma(True), kinds=ONE),
    'mfma_lean_exp': dict(shape=(128, 64), uneven=True, opts=OFF, chains=[[(0, 7)]], rec=None, ran=_mfma(True), kinds=ONE),
    'resident_exact': dict(shape=(32, 32), opts={}, chains=[[(0, 7), (1, 5)]], rec=(1, 31, (1, -1)), ran=_resident(32, 32, False), kinds=ONE),
    'resident_padded': dict(shape=(48, 40), opts={}, chains=[[(0, 7), (1, 5)]], rec=(1, 31, (1, -1)), ran=_resident(32, 32, True), kinds=ONE),
    'chain_exact': dict(shape=(128, 16), opts={}, chains=[[(0, 7)], [(0, 6)], [(0, 5)]], rec=(4, 3, (1,)), ran=_chain(7, False), kinds=('full', 'evidence')),
    'chain_padded': dict(shape=(100, 20), opts={}, chains=[[(0, 7)], [(0, 6)], [(0, 5)]], rec=(4, 3, (1,)), ran=_chain(7, True), kinds=('full', 'evidence')),
    'chain_in_kernel_anchors': dict(shape=(128, 16), opts={}, chains=[[(0, 0)], [(0, 0)], [(0, 0)]], rec=(4, 3, (1,)), ran=_chain(0, False),
                                    kinds=('evidence',)),
    'chain_fold2': dict(shape=(128, 16), opts={}, chains=[[(0, 7)], [(0, 6)], [(0, 5)]], rec=(4, 3, (1,)), ran=_chain(7, False), kinds=('fold',)),
    'chainax': dict(rec_also=(1, 15, (1,)), shape=(100, 90), opts={}, chains=[[(0, 7), (1, 5)], [(0, 6), (1, 5)]], rec=(4, 3, (1,)), both=True, ran=_chainax, kinds=('full', 'evidence')),
    'generic': dict(shape=(24, 20), opts={}, chains=[[(0, 3)]], clamp=-7.0, rec=None, ran=_generic, kinds=ONE),
}


def _sigma(radius, lattice):
    """a walk width whose SciPy radius int(4 sigma / lattice + 0.5) is `radius` (transitionModels.py:108-111)"""
    return 0.0 if radius == 0 else (radius - 0.25) / 4.0 * lattice


_REF = {}


def setup(fam, case, steps, full, prior_cap):
    """-> (problem, op values, per chain the longdouble reference with its bounds, likelihoods, whether the recurrence is accepted) for the
    records `steps` of the case; computed once per key and left unchanged"""
    key = (fam, case, steps, full, prior_cap)
    if key in _REF:
        return _REF[key]
    if len(_REF) > 64:
        _REF.clear()
    F = FAMILIES[fam]
    n0, n1 = F['shape']
    T = len(steps)
    mean, std = lc.mean_grid(n0, F.get('uneven', False)), lc.std_of(case, n1, n0)
    recs = lc.records(case, n0)[list(steps)]
    g = bo.Grid([mean, std])
    rec_ok = F['rec'] is not None and lc.recurrence_accepted(mean, std, recs)
    liks = []
    for r in recs:
        L = hp.gaussian_likelihood(mean, std, r)
        if rec_ok:
            e, z = hp.likelihood_bound_rec(mean, std, r, *F['rec'], split=True)
            if 'rec_also' in F:      # (the steps without a stencil run the streaming kernel: its anchors, 16 rows apart, as well)
                e1, z1 = hp.likelihood_bound_rec(mean, std, r, *F['rec_also'], split=True)
                e, z = np.maximum(e, e1), np.maximum(z, z1)
            if F.get('both'):        # (blc::chainax_kernel: the steps in the transposed layout take one exponential per cell)
                e2, z2 = hp.likelihood_bound_exp(mean, std, r, split=True, extra=hp.C_EXPMN)
                e, z = np.maximum(e, e2), np.maximum(z, z2)
        else:
            e, z = hp.likelihood_bound_exp(mean, std, r, split=True)
        liks.append((L, e + z, e))
    prior = lc.reciprocal_prior(liks[0][0])
    if prior_cap:
        prior = np.minimum(prior, prior_cap)
    refs, ops, values = [], [], []
    for walks in F['chains']:
        taps = [(ax, bo.gaussian_kernel1d(_sigma(rad, g.lattice[ax]) / g.lattice[ax])[1] if rad else np.ones(1)) for ax, rad in walks]
        refs.append(hp.gaussian_fit(prior, [(L, e) for L, e, _ in liks], taps, [mean, std], g.lattice, nblk=n0 * n1 // 64 + 1, full=full, clamp=F.get('clamp')))
        values.append([_sigma(rad, g.lattice[ax]) for ax, rad in walks] + ([F['clamp']] if 'clamp' in F else []))
    ops = [(_abi.OP_GRW, ax, -1, 0) for ax, _ in F['chains'][0]] + ([(_abi.OP_REGIMESWITCH, 0, -1, 0)] if 'clamp' in F else [])
    if not ops:
        ops, values = [(_abi.OP_STATIC, 0, -1, 0)], [[np.nan]] * len(F['chains'])
    problem = FitProblem(obs_model=_abi.OM_GAUSSIAN, marginal=[mean, std], lattice=list(g.lattice), data=recs.reshape(T, 1, -1),
                         timestamps=np.arange(T, dtype=np.float64), prior=prior, ops=ops)
    _REF[key] = (problem, np.asarray(values, dtype=np.float64), refs, liks, rec_ok)
    return _REF[key]


class Check:
    """collects every miss of a test before failing; keeps the worst error / bound per family"""

    def __init__(self, fam):
        self.fam, self.bad, self.top = fam, [], 0.0

    def within(self, got, want, bound, what):
        got = np.asarray(got, dtype=np.float64)
        want, bound = np.broadcast_to(np.asarray(want), got.shape), np.broadcast_to(np.asarray(bound), got.shape)
        nan = np.isnan(np.asarray(want, dtype=np.float64))
        if not np.array_equal(np.isnan(got), nan):
            self.bad.append('%s: NaN in %d cells, the reference has it in %d' % (what, int(np.isnan(got).sum()), int(nan.sum())))
            return
        if nan.all():
            return
        q = hp.worst(got[~nan], want[~nan], hp.SLACK * bound[~nan])
        print('%s %s: error / bound %.3f' % (self.fam, what, q))
        self.top = max(self.top, q)
        if not q <= 1.0:
            i, g, w, bd = hp.worst_at(got[~nan], want[~nan], hp.SLACK * bound[~nan])
            self.bad.append('%s: error / bound %.3g at %d of %s (got %r, want %r, bound %.3g)' % (what, q, i, got.shape, g, float(w), float(bd)))

    def local(self, got, want, bound, what):
        """a localEvidence entry; where the bound is infinite (a cell whose likelihood is not above its own bound: subnormal) the comparison
        says nothing, and the entry is held to being finite and positive"""
        if np.isfinite(float(bound)) or np.isnan(float(want)):
            return self.within([got], [want], [bound], what)
        if not (np.isfinite(got) and got > 0.0):
            self.bad.append('%s: %r is not finite and positive (reference %r, no finite bound)' % (what, got, float(want)))

    def exact_zeros(self, got, L, e_rel, what):
        """where every value inside the likelihood's bound rounds to 0 in float64 (L + SLACK e < TINY / 2) the output is exactly 0"""
        zero = (hp._ld(L) + hp.SLACK * hp._ld(e_rel)) < hp.LD(hp.TINY) / 2
        wrong = zero & ~(np.asarray(got) == 0.0)
        if wrong.any():
            i = int(np.argmax(wrong.reshape(-1)))
            self.bad.append('%s: %d of %d cells whose likelihood rounds to 0 are not exactly 0 (first: cell %d holds %r)' %
                            (what, int(wrong.sum()), int(zero.sum()), i, np.asarray(got).reshape(-1)[i]))

    def done(self):
        WORST[self.fam] = max(WORST.get(self.fam, 0.0), self.top)
        _report('worst ' + self.fam, '%.4f' % self.top)
        assert not self.bad, '\n'.join(self.bad)


def aborted_at(ref):
    """the first step whose normaliser is 0 in float64 (core.py:390-400), or None"""
    for t, (N, _) in enumerate(ref['norm']):
        if not float(N) > 0.0:
            return t
    return None


def run_kind(e, fam, case, steps, kind, chk):
    F = FAMILIES[fam]
    T = len(steps)
    # (T > 1: the prior stays below 1e150, so that the sums of p / L stay inside the float64 range)
    problem, values, refs, liks, rec_ok = setup(fam, case, tuple(steps), kind in ('full', 'fold'), None if T == 1 else 1e150)
    shape, G = list(F['shape']), int(np.prod(F['shape']))
    expect = F['ran'](rec_ok, T, kind)
    stops = any(aborted_at(r) is not None for r in refs)
    what = '%s records %s %s' % (case, list(steps), kind)
    acc = None
    with Options(e, F['opts']):
        if kind == 'fold':
            e.accum_begin(T, G)
        try:
            with Census(expect, what, chk, flavour=rec_ok if stops else None):
                if kind == 'forward':
                    res = e.fit(problem, values, forward_only=True, keep_posterior=True)
                elif kind == 'full':
                    res = e.fit(problem, values, keep_posterior=True)
                elif kind == 'evidence':
                    res = e.fit(problem, values, evidence_only=True)
                else:
                    res = e.fit(problem, values, accumulate=True, log_chain_weight=np.zeros(len(values)))
                posts = None
                if kind in ('forward', 'full') and all(aborted_at(r) is None for r in refs):
                    posts = [e.posterior(c, T, shape) for c in range(len(values))]
            if kind == 'fold' and all(aborted_at(r) is None for r in refs):
                acc = e.accum_read(T, [G]).reshape([T] + shape)
        finally:
            if kind == 'fold':
                e.accum_end()
    dV = float(np.prod(problem.lattice))
    for c, ref in enumerate(refs):
        w = '%s chain %d' % (what, c)
        stop = aborted_at(ref)
        if stop is not None:
            if not (res.abort_step[c] == stop and res.abort_phase[c] == 0):
                chk.bad.append('%s: the normaliser of step %d is 0, the fit reports abort step %d phase %d, logE %r' %
                               (w, stop, res.abort_step[c], res.abort_phase[c], res.log_evidence[c]))
            continue
        if res.abort_step[c] >= 0:
            chk.bad.append('%s: aborted at step %d phase %d' % (w, res.abort_step[c], res.abort_phase[c]))
            continue
        chk.within([res.log_evidence[c]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
        full = kind in ('full', 'fold')
        for t in range(T):
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            chk.local(res.local_evidence[c, t], loc[0], loc[1], w + ' localEvidence[%d]' % t)
            if posts is not None:
                want = ref['post'][t] if full else ref['alpha'][t]
                chk.within(posts[c][t], want[0], want[1], w + ' posterior[%d]' % t)
                if t == 0:
                    chk.exact_zeros(posts[c][0], liks[0][0], liks[0][2], w + ' posterior[0]')
                if res.posterior_mean is not None:
                    chk.within(res.posterior_mean[c, :, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)
    if acc is not None:
        # the evidence-weighted average (include/blhip.h): sum_h exp(logE_h - ref) max(post_h, 1e-300), with the library's own float64 log-weights as data
        lw = res.log_evidence
        refw = float(np.max(lw))
        A = sum(np.exp(hp.LD(lw[c]) - hp.LD(refw)) * np.maximum(np.stack([p for p, _ in refs[c]['post']]), hp.LD(hp.CLAMP)) for c in range(len(refs)))
        eA = sum(np.exp(hp.LD(lw[c]) - hp.LD(refw)) * np.stack([ep for _, ep in refs[c]['post']]) for c in range(len(refs)))
        bound = eA + hp.fold_bound(A, len(refs), 0, hp.fold_span(lw, refw)) / hp.SLACK
        chk.within(acc, A, bound, what + ' accumulator')


FAM_CASES = [(f, c) for f in FAMILIES for c in lc.CASES]


@pytest.mark.parametrize('fam,case', FAM_CASES, ids=['%s-%s' % fc for fc in FAM_CASES])
def test_every_cell_of_the_likelihood(eng, fam, case):
    """T = 1, each of the case's three records in turn: the forward-only posterior cell by cell (evidence-only families: the normaliser)"""
    chk = Check(fam)
    kind = FAMILIES[fam]['kinds'][0]
    for k in range(3):
        run_kind(eng, fam, case, (k,), kind, chk)
    chk.done()


BWD_CASES = [(f, c, T) for f in FAMILIES for c in lc.BACKWARD_CASES for T in (2, 3)]


@pytest.mark.parametrize('fam,case,T', BWD_CASES, ids=['%s-%s-T%d' % x for x in BWD_CASES])
def test_backward_side(eng, fam, case, T):
    """T = 2 and 3, every kind of fit of the family: the likelihoods of the steps behind a transition cell by cell in the forward-only
    posteriors; full fits: posteriors, localEvidence = 1 / (sum p / L dV) (NaN exactly where the reference divides 0 by 0), means, logE"""
    chk = Check(fam)
    for kind in FAMILIES[fam]['kinds']:
        run_kind(eng, fam, case, tuple(range(T)), kind, chk)
    chk.done()


# ---- GaussianMean on 1-D grids (observationModels.py:705-706): one exponential per cell in bl1c:: / bl1f:: / bl1p:: ------------------------------
# a row of 300 means; the datum of a step is (x, s).  chain1d = 2 forces the chain-resident 1-D kernel, chain1d = 0 leaves the K-steps-per-launch
# kernel (persist1d = 0) or the persistent one (K = fuse1d = 2 < T).

GM_N = 300
GM_FAMILIES = {
    'chain1d': (dict(chain1d=2), r'bl1c::chain1d_kernel<3, (false|true), \d, 0>'),
    'fused1d': (dict(chain1d=0, persist1d=0), r'bl1f::fused1d_kernel<3, (false|true)>'),
    'persist1d': (dict(chain1d=0, fuse1d=2), r'bl1p::persist1d_kernel<3, (false|true)>'),
}
GM_CASES = {
    'inside': [('node', 0.5), ('between', 0.032), ('lo', 4.0)],
    'narrow': [('between', 1.6e-4), ('node', 1.6e-4), ('hi', 1e-3)],
    'outside': [('lo-1', 4.0), ('hi+1', 4.0), ('lo-10', 4.0)],
    'missing': [('nan', 1.0), ('node', lc.NAN), ('node2', 0.25)],
}
GM_BACKWARD = ['inside', 'missing', 'outside']


def gm_setup(case, steps, full):
    key = ('gm', case, steps, full)
    if key in _REF:
        return _REF[key]
    mean = lc.mean_grid(GM_N)
    g = bo.Grid([mean])
    data = np.array([[lc.position(p, GM_N), s] for p, s in GM_CASES[case]], dtype=np.float64)[list(steps)]
    liks = []
    for x, s in data:
        L = hp.gaussian_mean_likelihood(mean, x, s).reshape(-1, 1)
        ok = x == x and s == s
        e, z = hp.likelihood_bound_exp(mean, [s if ok else 1.0], [x if ok else lc.NAN], split=True)
        liks.append((L, e + z, e))
    T = len(steps)
    prior = lc.reciprocal_prior(liks[0][0])
    if T > 1:
        prior = np.minimum(prior, 1e150)
    sigma = _sigma(5, g.lattice[0])
    taps = [(0, bo.gaussian_kernel1d(sigma / g.lattice[0])[1])]
    ref = hp.gaussian_fit(prior, [(L, e) for L, e, _ in liks], taps, [mean, np.zeros(1)], [g.lattice[0], 1.0], nblk=GM_N // 64 + 1, full=full)
    problem = FitProblem(obs_model=_abi.OM_GAUSSIAN_MEAN, marginal=[mean], lattice=[g.lattice[0]], data=data.reshape(T, 1, 2),
                         timestamps=np.arange(T, dtype=np.float64), prior=prior[:, 0], ops=[(_abi.OP_GRW, 0, -1, 0)])
    _REF[key] = (problem, np.array([[sigma]]), ref, liks)
    return _REF[key]


def gm_run(e, fam, case, steps, full, chk):
    opts, pattern = GM_FAMILIES[fam]
    problem, values, ref, liks = gm_setup(case, tuple(steps), full)
    T = len(steps)
    what = '%s records %s %s' % (case, list(steps), 'full' if full else 'forward')
    stop = aborted_at(ref)
    with Options(e, opts):
        before = _counts()
        res = e.fit(problem, values, forward_only=not full, keep_posterior=True)
        posts = e.posterior(0, T, [GM_N]) if stop is None else None
        after = _counts()
    watched = {k for k in after if after[k] > before.get(k, 0) and WATCH.match(k)}
    _report('ran ' + what, ', '.join(sorted(watched)))
    if fam == 'persist1d' and T <= 2:                     # (the persistent kernel needs more steps than one launch of the fused one takes, K = 2: shorter fits run that one)
        pattern = GM_FAMILIES['fused1d'][1]
    passes = {re.fullmatch(pattern, k).group(1) for k in watched if re.fullmatch(pattern, k)}
    if not (watched and all(re.fullmatch(pattern, k) for k in watched) and (passes == ({'false', 'true'} if full else {'false'}) or stop is not None)):
        chk.bad.append('%s: expected the %s of %s, ran %s' % (what, 'two passes' if full else 'forward pass', pattern, sorted(watched)))
    if stop is not None:
        if not (res.abort_step[0] == stop and res.abort_phase[0] == 0):
            chk.bad.append('%s: the normaliser of step %d is 0, the fit reports abort step %d phase %d' % (what, stop, res.abort_step[0], res.abort_phase[0]))
        return
    if res.abort_step[0] >= 0:
        chk.bad.append('%s: aborted at step %d phase %d' % (what, res.abort_step[0], res.abort_phase[0]))
        return
    chk.within([res.log_evidence[0]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], what + ' logE')
    for t in range(T):
        loc = ref['local'][t] if full else ref['local_fwd'][t]
        chk.local(res.local_evidence[0, t], loc[0], loc[1], what + ' localEvidence[%d]' % t)
        want = ref['post'][t] if full else ref['alpha'][t]
        chk.within(posts[t], want[0][:, 0], want[1][:, 0], what + ' posterior[%d]' % t)
        if t == 0:
            chk.exact_zeros(posts[0], liks[0][0][:, 0], liks[0][2][:, 0], what + ' posterior[0]')
        chk.within(res.posterior_mean[0, :1, t], ref['means'][t][0][:1], ref['means'][t][1][:1], what + ' mean[%d]' % t)


GM_ALL = [(f, c) for f in GM_FAMILIES for c in GM_CASES]


@pytest.mark.parametrize('fam,case', GM_ALL, ids=['%s-%s' % x for x in GM_ALL])
def test_gaussian_mean_on_a_row_of_300_cells(eng, fam, case):
    """every datum alone (T = 1, forward-only: cell by cell), then T = 2 and 3, forward-only and full"""
    chk = Check('gaussian_mean_' + fam)
    for k in range(3):
        gm_run(eng, fam, case, (k,), False, chk)
    if case in GM_BACKWARD:
        for T in (2, 3):
            for full in (False, True):
                gm_run(eng, fam, case, tuple(range(T)), full, chk)
    chk.done()
