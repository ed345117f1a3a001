"""
The Poisson likelihood inside the step kernels and the likelihood table of the Bernoulli, Laplace, WhiteNoise, AR1 and ScaledAR1 models on the
MI355X, cell by cell against tests/highprec.py: blk::likelihood<OM_POISSON> -- the direct route pow(lambda, k) exp(-lambda) / k! and the
log-space route exp(k log(lambda) - lambda - ln k!) that the host selects per record (blhip_host_poisson_direct) -- in blk::step_kernel<1, ..>,
bl1c::chain1d_kernel<1, ..>, bl1c::lik1d_table_kernel<1>, bl1f::fused1d_kernel<1, ..> and bl1p::persist1d_kernel<1, ..>, and blk::lik_table_kernel
with the <100, ..> kernels that consume its table.  Every comparison is worst(got, want, SLACK * bound) <= 1 with a bound COUNTED in
tests/highprec.py; what is covered, what the card showed and which in-bounds changes of the kernels these tests catch: tests/OBSERVATION_KERNELS.md.

Small fits at engine level, T = 1, 2, 3, as tests/test_likelihood_kernels.py runs them: the prior is the reciprocal of the true likelihood of
step 0, so every cell of the T = 1 forward-only posterior shows the relative error of its own L, and where every value inside the bound rounds
to 0 the output must be exactly 0.  A step whose reference normaliser is 0 must abort there.  Inputs: tests/observation_cases.py.  Every engine
call takes census deltas and asserts which of the watched instantiations ran.  BLHIP_OBSERVATION_REPORT=<file> appends, per test, the
instantiations that ran and the worst error / bound.

compare() and the two setup functions are engine-agnostic: tests/test_highprec.py runs them on the float64 oracle at the same bounds.
"""
import os
import re

import numpy as np
import pytest

import bayesloop_amd as bl
import highprec as hp
import likelihood_cases as lc
import observation_cases as oc
import test_likelihood_kernels as lk
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem
from oracle import bl_oracle as bo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)]

WORST = {}
DEFAULTS = dict(chain_resident=1, resident=1, mfma=1, fast=1, chain1d=1, persist1d=1, fuse1d=8)
# the instantiations that evaluate a Poisson likelihood, the two table builders, and every consumer of a likelihood table
WATCH = re.compile(r'^(blk::step_kernel<1,|bl1c::chain1d_kernel<1,|bl1c::lik1d_table_kernel<1>|bl1f::\w+<1,|bl1p::\w+<1,|blk::lik_table_kernel|\w+::\w+<100,)')


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
    path = os.environ.get('BLHIP_OBSERVATION_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write('%s\t%s\t%s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, text))


_counts, aborted_at, _sigma = lk._counts, lk.aborted_at, lk._sigma


class Options:
    def __init__(self, e, opts):
        self.e, self.opts = e, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.e.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.e.set_option(k, DEFAULTS[k])


class Check(lk.Check):
    """the comparisons of tests/test_likelihood_kernels.py; the worst error / bound per family goes to this file's table (or the caller's) and report"""

    def __init__(self, fam, worst=WORST):
        lk.Check.__init__(self, fam)
        self.worst = worst

    def done(self):
        self.worst[self.fam] = max(self.worst.get(self.fam, 0.0), self.top)
        _report('worst ' + self.fam, '%.4f' % self.top)
        assert not self.bad, '\n'.join(self.bad)


_REF = {}


def _fit_reference(prior, liks, grids, lattice, radii, full):
    """hp.transition_fit per chain: a walk of the chain's radius along axis 0 between the steps (radius 0: Static)"""
    refs = []
    for rad in radii:
        stages = [('walk', 0, bo.gaussian_kernel1d(_sigma(rad, lattice[0]) / lattice[0])[1])] if rad else []
        steps = [dict(fwd=('prev', stages), bwd=('prev', stages)) for _ in liks]
        refs.append(hp.transition_fit(prior, [(L, e) for L, e, _ in liks], steps, grids, lattice, nblk=int(np.size(prior)) // 64 + 1, full=full))
    return refs


def _finish(key, om, grids, data, liks, radii, full, seg_len=1):
    T = len(liks)
    g = bo.Grid(grids)
    prior = lc.reciprocal_prior(liks[0][0])
    if T > 1:                                  # (the sums of p / L stay inside the float64 range)
        prior = np.minimum(prior, 1e150)
    refs = _fit_reference(prior, liks, grids, list(g.lattice), radii, full)
    walk = any(radii)
    ops = [(_abi.OP_GRW, 0, -1, 0)] if walk else [(_abi.OP_STATIC, 0, -1, 0)]
    values = np.array([[_sigma(r, g.lattice[0]) if walk else np.nan] for r in radii], dtype=np.float64)
    problem = FitProblem(obs_model=om, marginal=grids, lattice=list(g.lattice), data=data, timestamps=np.arange(T, dtype=np.float64), prior=prior,
                         ops=ops, seg_len=seg_len)
    _REF[key] = (problem, values, refs, liks)
    return _REF[key]


def poisson_setup(case, n, steps, full, radii=(5,)):
    """-> (problem, op values, per chain the longdouble reference with its bounds, per step (L, bound, relative part)); memoised, left unchanged"""
    key = ('poisson', case, n, steps, full, radii)
    if key in _REF:
        return _REF[key]
    rates, recs = oc.poisson_rates(case, n), oc.poisson_records(case)[list(steps)]
    liks = []
    for r in recs:
        e, z = hp.poisson_bound(rates, r, oc.direct_domain(rates, r))
        liks.append((hp.poisson_likelihood(rates, r), e + z, e))
    return _finish(key, _abi.OM_POISSON, [rates], recs.reshape(len(steps), 1, -1), liks, radii, full)


TABLE_OM = dict(bernoulli=_abi.OM_BERNOULLI, laplace=_abi.OM_LAPLACE, white_noise=_abi.OM_WHITE_NOISE, ar1=_abi.OM_AR1, scaled_ar1=_abi.OM_SCALED_AR1)


def table_setup(model, shape, case, steps, full):
    key = (model, shape, case, steps, full)
    if key in _REF:
        return _REF[key]
    grids, segs = oc.table_grids(model, shape), oc.table_segments(model, case, shape)[list(steps)]
    liks = []
    for s in segs:
        L, e, z = hp.TABLE_LIKELIHOODS[model](*grids, s, bound=True)
        liks.append((L, e + z, e))
    return _finish(key, TABLE_OM[model], grids, segs, liks, (0,), full, seg_len=oc.SEG_LEN[model])


def compare(e, setup, full, chk, what, chains=None):
    """runs the fit on the engine `e` (the HIP engine, or tests/oracle_engine.py's float64 one) and holds it to the reference: the abort step
    where a normaliser is 0, else logE, localEvidence, the posteriors cell by cell (exact zeros in step 0), the means"""
    problem, values, refs, liks = setup
    T, shape = problem.T, problem.grid_size
    stops = [aborted_at(r) for r in refs]
    res = e.fit(problem, values, forward_only=not full, keep_posterior=True)
    posts = [e.posterior(c, T, shape) for c in range(len(refs))] if all(s is None for s in stops) else None
    for c, ref in enumerate(refs):
        w = '%s chain %d' % (what, c) if len(refs) > 1 else what
        if stops[c] is not None:
            if not (res.abort_step[c] == stops[c] and res.abort_phase[c] == 0):
                chk.bad.append('%s: the normaliser of step %d is 0, the fit reports abort step %d phase %d, logE %r' %
                               (w, stops[c], res.abort_step[c], res.abort_phase[c], res.log_evidence[c]))
            continue
        if res.abort_step[c] >= 0:
            chk.bad.append('%s: aborted at step %d phase %d' % (w, res.abort_step[c], res.abort_phase[c]))
            continue
        chk.within([res.log_evidence[c]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
        for t in range(T):
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            chk.local(res.local_evidence[c, t], loc[0], loc[1], w + ' localEvidence[%d]' % t)
            if posts is not None:
                want = ref['post'][t] if full else ref['alpha'][t]
                chk.within(posts[c][t], want[0], want[1], w + ' posterior[%d]' % t)
                if t == 0:
                    chk.exact_zeros(posts[c][0], liks[0][0], liks[0][2], w + ' posterior[0]')
            chk.within(res.posterior_mean[c, :, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)
    return any(s is not None for s in stops)


def run(e, opts, expect, setup, full, chk, what):
    """compare() under the engine options `opts`, with the census: exactly the `expect`ed ones of the watched instantiations ran (a fit that
    stops at a zero normaliser leaves its path half way: then a subset of them, and at least one)"""
    with Options(e, opts):
        before = _counts()
        stopped = compare(e, setup, full, chk, what)
        after = _counts()
    watched = {k for k in after if after[k] > before.get(k, 0) and WATCH.match(k)}
    _report('ran ' + what, ', '.join(sorted(watched)))
    if not (watched == set(expect) or (stopped and watched and watched <= set(expect))):
        chk.bad.append('%s: expected %s, ran %s' % (what, sorted(expect), sorted(watched)))


# ---- Poisson: a row of 300 (600) rates; the options of GM_FAMILIES in tests/test_likelihood_kernels.py select the family ---------------------------
# chain1d = 2 forces the chain-resident 1-D kernel (M = 1 up to 512 cells, M = 2 beyond), chain1d = 0 leaves the K-steps-per-launch kernel
# (persist1d = 0), the persistent one (K = fuse1d = 2 < T; shorter fits run the fused one) or, with fuse1d = 0, the generic step kernel.
# A batch of four chains shares ONE (T, n) table that bl1c::lik1d_table_kernel<1> builds; the chain kernel then reads it (<100, ..>).

def _passes(pattern, full):
    return {pattern % 'false'} | ({pattern % 'true'} if full else set())


def _chain1d(M):
    def f(T, full, repeated=False):
        return _passes('bl1c::chain1d_kernel<1, %%s, %d, 0>' % M, full)
    return f


def _fused1d(T, full, repeated=False):
    return _passes('bl1f::fused1d_kernel<1, %s>', full)


def _persist1d(T, full, repeated=False):
    """a pass of a single launch (T <= K = 2) has no launch boundary to save and runs the fused kernel; where a raw sum of that launch comes
    near the bottom of the float64 range the host repeats the fit with K = 1 (forward_bookkeeping, blhip_book.hpp), and a fit of T = 2 > K is
    then the persistent kernel's: the fused kernel's forward pass AND both passes of the persistent one have run"""
    if T == 1:
        return _fused1d(T, full)
    if T == 2:
        return _fused1d(T, False) | _passes('bl1p::persist1d_kernel<1, %s>', full) if repeated else _fused1d(T, full)
    return _passes('bl1p::persist1d_kernel<1, %s>', full)


RAW_SUM_FLOOR = 1e-200     # blhip_book.hpp: a raw sum of a K-steps-per-launch pass at or below it sends the fit to K = 1


def repeated_with_one_step_per_launch(setup, K):
    """whether the host repeats the fit with K = 1: a launch of K steps normalises lazily, so the raw sum of its step t is the product of the
    reference's normalisers since the launch's first step (the backward pass's sums carry the same product over 1 / G).  Taken from the
    longdouble reference; a case whose product lies within 1e6 of the floor would make the expectation a matter of rounding and is refused."""
    _, _, refs, _ = setup
    low = False
    for ref in refs:
        G = int(np.size(ref['alpha'][0][0]))
        for t0 in range(0, len(ref['norm']), K):
            raw = hp.LD(1)
            for N, _ in ref['norm'][t0:t0 + K]:
                raw = raw * N
                if not float(N) > 0.0:
                    break
                assert not 1e-6 * RAW_SUM_FLOOR * G < float(raw) < 1e6 * RAW_SUM_FLOOR * G, 'a raw sum of %r: too near the floor' % float(raw)
                low = low or float(raw) < RAW_SUM_FLOOR
    return low


def _generic(T, full, repeated=False):
    return {'blk::step_kernel<1, 0, true>'} if not full else {'blk::step_kernel<1, 0, false>', 'blk::step_kernel<1, 1, true>'}


def _batch(T, full, repeated=False):
    return {'bl1c::lik1d_table_kernel<1>'} | _passes('bl1c::chain1d_kernel<100, %s, 1, 0>', full)


POISSON_FAMILIES = {
    'chain1d': dict(n=300, opts=dict(chain1d=2), ran=_chain1d(1)),
    'chain1d_600': dict(n=600, opts=dict(chain1d=2), ran=_chain1d(2)),
    'fused1d': dict(n=300, opts=dict(chain1d=0, persist1d=0), ran=_fused1d),
    'persist1d': dict(n=300, opts=dict(chain1d=0, fuse1d=2), ran=_persist1d),
    'generic': dict(n=300, opts=dict(chain1d=0, fuse1d=0), ran=_generic),
    'batch_table': dict(n=300, opts=dict(chain1d=2), ran=_batch, radii=(5, 4, 3, 2)),
}
POISSON_ALL = [(f, c) for f in POISSON_FAMILIES for c in oc.POISSON_CASES]


def poisson_problems(case):
    """(steps, full) of a case: every record alone, forward-only; the BACKWARD cases also T = 2 and 3, forward-only and full"""
    out = [((k,), False) for k in range(3)]
    if case in oc.POISSON_BACKWARD:
        out += [(tuple(range(T)), full) for T in (2, 3) for full in (False, True)]
    return out


@pytest.mark.parametrize('fam,case', POISSON_ALL, ids=['%s-%s' % x for x in POISSON_ALL])
def test_poisson_on_a_row_of_rates(eng, fam, case):
    F = POISSON_FAMILIES[fam]
    chk = Check('poisson_' + fam)
    for steps, full in poisson_problems(case):
        what = '%s records %s %s' % (case, list(steps), 'full' if full else 'forward')
        setup = poisson_setup(case, F['n'], steps, full, F.get('radii', (5,)))
        repeated = repeated_with_one_step_per_launch(setup, F['opts'].get('fuse1d', DEFAULTS['fuse1d']) or 1)
        run(eng, F['opts'], F['ran'](len(steps), full, repeated), setup, full, chk, what)
    chk.done()


# ---- the table models: blk::lik_table_kernel builds the (T, G) table, a <100, ..> kernel consumes it (Static transition) ---------------------------
# the consumers are pinned by options, as tests/step_transition_cases.py pins them: the chain-resident 1-D kernel on a row, the generic step kernel
# on the two-parameter grids

TABLE_OPTS_1D = dict(chain1d=2)
TABLE_OPTS_2D = dict(chain_resident=0, resident=0, fast=0, mfma=0)

def _table_1d(T, full):
    return {'blk::lik_table_kernel'} | _passes('bl1c::chain1d_kernel<100, %s, 1, 0>', full)


def _table_2d(T, full):
    return {'blk::lik_table_kernel'} | ({'blk::step_kernel<100, 0, true>'} if not full else {'blk::step_kernel<100, 0, false>', 'blk::step_kernel<100, 1, true>'})


TABLE_ALL = [(m, s, c) for m in oc.TABLE_CASES for s in oc.TABLE_SHAPES[m] for c in oc.TABLE_CASES[m]]


def table_problems(model, case):
    out = [((k,), False) for k in range(3)]
    if case in oc.TABLE_BACKWARD[model]:
        out += [(tuple(range(T)), full) for T in (2, 3) for full in (False, True)]
    return out


@pytest.mark.parametrize('model,shape,case', TABLE_ALL, ids=['%s-%s-%s' % (m, 'x'.join(map(str, s)), c) for m, s, c in TABLE_ALL])
def test_table_models_cell_by_cell(eng, model, shape, case):
    chk = Check('table_' + model)
    for steps, full in table_problems(model, case):
        what = '%s records %s %s' % (case, list(steps), 'full' if full else 'forward')
        expect = (_table_1d if len(shape) == 1 else _table_2d)(len(steps), full)
        run(eng, TABLE_OPTS_1D if len(shape) == 1 else TABLE_OPTS_2D, expect, table_setup(model, shape, case, steps, full), full, chk, what)
    chk.done()
