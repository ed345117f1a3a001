"""
The posterior predictive on the device (bayesloop_amd/csrc/blhip_predictive.hpp, blhip_posterior_predictive): Study.simulate for one time
stamp, the time average and -- new -- every time stamp at once.

The contraction alone.  The inputs come from the device itself -- the kept posteriors of a small hyper-fit and its finalised average
posterior, read back bit for bit -- and the likelihood rows from the caller, so neither the fit nor a likelihood is under test; the
expected value is a longdouble sum of the same products.  The posteriors hold exact zeros (a narrow likelihood far from most of the grid),
the average posterior the 1e-300 floors of the fold; the rows span 300 decades.  Bound per entry: a sum of G non-negative products in ANY
order is off by at most (G - 1 + 1) roundings per term, the averaged operand carries two more (a compensated sum and a division), and a
product below the normal range is off by at most the subnormal step:  ((G + 2) u sum|terms| + G TINY) x SLACK, u = 2 ** -53.
Shapes: T of 1, 15, 16, 17, 33 rows (ranges of a 33-step sequence: strictly inside it but for the last), X of 1, 16, 17, 40 values, G of
2, 105, 1260 and two slabs + 5 cells of the plan.  The model of the call describes the grid with as many parameters as its name says; the
sequence itself is the one a 1-D fit of as many cells left (the contraction runs over cells, whatever their arrangement).

Rows built on the device: simulate(x, t='all'), simulate(x, t) and simulate(x) with density False and True against the host formula on
S.posteriorSequence with om.pdf, at rtol 1e-9 (all terms are non-negative; a term is off by about 1500 u = 1.7e-13 at the most, the sums
of G <= 2 ** 20 terms by 2 gamma_G <= 2.4e-10).

Which kernels ran is read from the library's registry and asserted.
"""
import ctypes as C
import re

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import HipEngine, extra_engine
import cases
import highprec as hp
import oracle_adapter as oa
import predictive_cases as pc
from conftest import kernel_census

pytestmark = pytest.mark.gpu

ROW_KERNELS = ('tabulate_rows_kernel', 'lik_table_kernel', 'lik_program_kernel')


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    try:
        eng.accum_end()
        eng.release_posterior()
    finally:
        bl.set_engine(prev)


@pytest.fixture
def eng(hip_engine):
    return hip_engine


def _counts():
    out = {}
    for c, name in kernel_census():
        fam = re.sub(r'[<(].*', '', name).split('::')[-1].strip()
        out[fam] = out.get(fam, 0) + c
    return out


class Launched:
    """with Launched() as k: ... ; k.count[family] = launches inside"""

    def __enter__(self):
        self.before = _counts()
        self.count = {}
        return self

    def __exit__(self, *exc):
        after = _counts()
        self.count = {k: after[k] - self.before.get(k, 0) for k in after if after[k] > self.before.get(k, 0)}

    def require(self, *kernels):
        missing = [k for k in kernels if k not in self.count]
        assert not missing, 'expected kernel(s) not launched: %s; launched: %s' % (missing, sorted(self.count))

    def forbid(self, *kernels):
        hit = [k for k in kernels if k in self.count]
        assert not hit, 'kernel(s) launched that this case must not take: %s' % hit


def within(got, want, bound, what):
    q = hp.worst(got, want, bound)
    print('%s: worst |error| / bound = %.3g' % (what, q))
    assert q <= 1.0, '%s: worst |error| / bound = %.3g at (index, got, want, bound) = %r' % (what, q, hp.worst_at(got, want, bound))


# ---- the contraction alone -----------------------------------------------------------------------------------------------------------------

T_SEQ, CHAINS = 33, 3
GRIDS = pc.contract_grids(lambda G, T, X: HipEngine.predictive_plan(G, T, X))
_PROBLEMS = {}


def sequences(eng, G):
    """A kept, accumulating fit of CHAINS chains on a 1-D grid of G cells with a narrow likelihood, then the finalised average: -> the
    chains' posteriors (CHAINS, T, G) and the average posterior (T, G) as the device holds them."""
    if G not in _PROBLEMS:
        data = cases.gm_data(5, T_SEQ)
        data[:, 1] = 0.2 if G > 2 else 4.0              # (two cells, at -8 and 8: a narrow likelihood would leave nothing to normalise)
        S = cases.build(bl, dict(study='Study', data=data, om=('GaussianMean', [('mean', ('cint', -8, 8, G))], 'default'), tm=('GRW', 'sigma', 0.1, 'mean', None)))
        S._checkConsistency()
        S._formatData()
        _PROBLEMS[G] = S._compile(silent=True)[0]
    problem = _PROBLEMS[G]
    ov = (np.linspace(0.15, 0.9, CHAINS) * 0.3).reshape(CHAINS, 1)
    eng.accum_begin(T_SEQ, G)
    res = eng.fit(problem, ov, keep_posterior=True, accumulate=True, log_chain_weight=np.linspace(0.0, -3.0, CHAINS))
    assert np.all(res.abort_step < 0) and np.all(np.isfinite(res.log_evidence))
    eng.accum_finalize(problem)
    posts = np.stack([eng.posterior(b, T_SEQ, [G]) for b in range(CHAINS)])
    acc = eng.accum_read(T_SEQ, [G])
    return posts, acc


def reference(seq, rows, average):
    """-> (longdouble sums (T or 1, X), bounds)"""
    p = np.asarray(seq, dtype=np.longdouble)
    if average:
        p = (p.sum(axis=0) / np.longdouble(len(seq)))[None]
    terms = p[:, None, :] * np.asarray(rows, dtype=np.longdouble)[None, :, :]                 # (T, X, G), all >= 0
    G = seq.shape[1]
    want = terms.sum(axis=2)
    bound = hp.SLACK * ((G + 2) * hp.U * want + G * hp.TINY)
    return want, np.asarray(bound, dtype=np.longdouble)


def model_of(grid):
    return [np.linspace(0.5, 1.5, n) for n in grid]


@pytest.mark.parametrize('X', pc.CONTRACT_X)
@pytest.mark.parametrize('grid', sorted(GRIDS), ids=sorted(GRIDS))
def test_contraction_against_longdouble_sums(eng, grid, X):
    shape = GRIDS[grid]
    G = int(np.prod(shape))
    posts, acc = sequences(eng, G)
    if G > 2:
        assert (posts == 0.0).any(), 'the kept posteriors hold no exact zero'
        assert (acc < 1e-299).any() and (acc > 0.0).all(), 'the average posterior holds no floor'
    spread = pc.likelihood_rows(X, G, 100 + G + X)
    assert spread.max() / spread[spread > 0].min() > 1e290
    marg, x = model_of(shape), np.zeros(X)
    for T in pc.CONTRACT_T:
        t0 = (T_SEQ - T) // 2
        assert T == T_SEQ or 0 < t0 < t0 + T < T_SEQ
        for source, chain, seq in ((0, CHAINS - 1, posts[CHAINS - 1]), (1, 0, acc)):
            # (the spread rows with the range's rows, the balanced ones -- every cell counts -- with its average and, at full length, its rows)
            for average, rows in ((False, spread), (True, spread), (True, pc.balanced_rows(seq[t0:t0 + T], X, G + T)),
                                  (False, pc.balanced_rows(seq, X, G + T + 1))):
                with Launched() as k:
                    got = eng.predictive(source, chain, marg, _abi.OM_TABLE, x, t0, t0 + T, average, host_rows=rows)
                k.require('contract_kernel', 'combine_kernel')
                k.forbid(*ROW_KERNELS)
                assert ('average_rows_kernel' in k.count) == average
                assert k.count['contract_kernel'] == 1 and k.count['combine_kernel'] == 1
                assert got.shape == (1 if average else T, X)
                want, bound = reference(seq[t0:t0 + T], rows, average)
                within(got, want, bound, 'source %d, T = %d%s' % (source, T, ', average' if average else ''))
                again = eng.predictive(source, chain, marg, _abi.OM_TABLE, x, t0, t0 + T, average, host_rows=rows)
                assert np.array_equal(got, again, equal_nan=True), 'two calls on the same inputs differ'
    eng.accum_end()


def test_three_chunks_with_a_ragged_last_one():
    """The budget leaves room for 16 likelihood rows of the 40: chunks of 16, 16 and 8 values, each contracted and combined on its own,
    land in their columns of the result.  (A context of its own: the option dies with it.)"""
    shape = GRIDS['two-slabs+5']
    G, X = shape[0], 40
    e = extra_engine(bl.get_engine().device)
    try:
        posts, acc = sequences(e, G)
        rows = pc.likelihood_rows(X, G, 7)
        for average, T in ((False, T_SEQ), (True, 1)):
            budget = HipEngine.predictive_plan(G, T, X, average)['min_budget_bytes']
            while HipEngine.predictive_plan(G, T, X, average, budget)['rows_per_chunk'] < 16:
                budget += 256
            p = HipEngine.predictive_plan(G, T, X, average, budget)
            assert (p['rows_per_chunk'], p['n_chunks'], p['n_slabs']) == (16, 3, 3)
            e.set_option('mem_budget_bytes', budget / 0.9 + 64)          # (the library plans within 0.9 of the option)
            with Launched() as k:
                got = e.predictive(0, 1, model_of(shape), _abi.OM_TABLE, np.zeros(X), 0, T_SEQ, average, host_rows=rows)
            assert k.count['contract_kernel'] == 3 and k.count['combine_kernel'] == 3
            want, bound = reference(posts[1], rows, average)
            within(got, want, bound, 'three chunks%s' % (', average' if average else ''))
            e.set_option('mem_budget_bytes', 1e15)
            with Launched() as k:
                whole = e.predictive(0, 1, model_of(shape), _abi.OM_TABLE, np.zeros(X), 0, T_SEQ, average, host_rows=rows)
            assert k.count['contract_kernel'] == 1
            assert np.array_equal(got, whole), 'the chunks are no columns of the unchunked result'
        e.set_option('mem_budget_bytes', 64.0)
        rc = e.lib.blhip_posterior_predictive(e.ctx, 0, 1, 0, T_SEQ, 0, C.byref(_model(shape)[0]), _abi.dptr(np.zeros(X)), X, None, _abi.dptr(rows),
                                              _abi.dptr(np.empty(T_SEQ * X)))
        assert rc != 0 and 'budget' in e.lib.blhip_last_error(e.ctx).decode()
    finally:
        e.accum_end()
        del e


# ---- rows built on the device --------------------------------------------------------------------------------------------------------------

def simulate_everything(S, x):
    """every kind of call while the posterior is on the device -> {(index, density): result}, the kernels launched"""
    T = len(S.formattedTimestamps)
    out = {}
    with Launched() as k:
        for density in (False, True):
            out[('all', density)] = S.simulate(x, t='all', density=density)
            out[(T // 2, density)] = S.simulate(x, t=S.formattedTimestamps[T // 2], density=density)
            out[(None, density)] = S.simulate(x, density=density)
    assert S._posterior_pending is not None, 'the posterior sequence was copied to the host'
    return out, k


def check_against_host(S, x, out):
    T = len(S.formattedTimestamps)
    for (index, density), got in out.items():
        with np.errstate(all='ignore'):
            want = pc.host_simulate(S, x, index, density)
        assert got.shape == want.shape == ((T, len(x)) if index == 'all' else (len(x),))
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-300, err_msg='index %r, density %r' % (index, density))


@pytest.mark.parametrize('name', sorted(pc.MODELS))
def test_simulate_with_rows_built_on_the_device(eng, name):
    S = pc.build_model(bl, name)
    x, where = pc.MODELS[name][1], pc.MODELS[name][2]
    with np.errstate(all='ignore'):
        S.fit(silent=True)
    if name in ('scipy_t_5x18x14', 'johnsonsu_3x3x7x6'):
        assert list(S.gridSize) == [int(v) for v in name.split('_')[-1].split('x')]
    out, k = simulate_everything(S, x)
    k.require('contract_kernel', 'combine_kernel', 'average_rows_kernel')
    rows_kernel = dict(formula='tabulate_rows_kernel', table='lik_table_kernel', program='lik_program_kernel', host=None)[where]
    if rows_kernel:
        k.require(rows_kernel)
    k.forbid(*[r for r in ROW_KERNELS if r != rows_kernel])
    check_against_host(S, x, out)


def test_models_whose_rows_come_from_the_host(eng):
    """bl.om.NumPy has no density the library can see; a subclass that overrides pdf is taken at its word."""
    def likelihood(data, mu, s):
        return np.exp(-np.abs(data - mu) / s) / (2. * s) + 1e-3 * (mu > 5.)

    S = bl.Study(silent=True)
    S.loadData(cases.series(31, 9), silent=True)
    S.set(bl.om.NumPy(likelihood, 'mu', bl.cint(-4, 4, 33), 's', bl.oint(0, 3, 13)), bl.tm.GaussianRandomWalk('w', 0.3, target='mu'), silent=True)
    S.fit(silent=True)
    x = np.linspace(-4.0, 4.0, 18)
    out, k = simulate_everything(S, x)
    k.require('contract_kernel')
    k.forbid(*ROW_KERNELS)
    check_against_host(S, x, out)

    class Twice(bl.om.Poisson):
        def pdf(self, grid, dataSegment):
            return 2.0 * bl.om.Poisson.pdf(self, grid, dataSegment)

    S = bl.Study(silent=True)
    S.loadData(cases.COAL[:12], silent=True)
    S.set(Twice('rate', bl.oint(0, 6, 70)), bl.tm.GaussianRandomWalk('w', 0.2, target='rate'), silent=True)
    S.fit(silent=True)
    x = np.arange(0.0, 9.0)
    out, k = simulate_everything(S, x)
    k.require('contract_kernel')
    k.forbid(*ROW_KERNELS)
    check_against_host(S, x, out)


def test_poisson_values_outside_the_direct_formula(eng):
    """A count the host formula truncates (2.5: factorial(int(k)) with rate ** 2.5) takes a host row beside the device rows of the
    others; a count above 170 raises on the device path what it raises on the host path (171! is no double)."""
    S = pc.build_model(bl, 'poisson1d')
    S.fit(silent=True)
    x = np.array([0.0, 3.0, 2.5, 170.0, 1.0, 60.0, 7.0, 12.0])
    out, k = simulate_everything(S, x)
    k.require('contract_kernel', 'tabulate_rows_kernel')
    assert k.count['tabulate_rows_kernel'] == k.count['contract_kernel'] // 2           # one of the two calls behind each simulate has host rows
    for bad in (171.0, 500.0):
        with pytest.raises(OverflowError):
            S.simulate(np.array([1.0, bad, 2.0]), t='all')
    assert S._posterior_pending is not None
    check_against_host(S, x, out)
    for bad in (171.0, 500.0):
        with pytest.raises(OverflowError):
            S.simulate(np.array([1.0, bad, 2.0]))                      # (the host path: the posterior is on the host now)


# ---- golden, options, the average posterior ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', sorted(pc.GOLDEN_X))
def test_fixture_on_the_device_path(eng, case):
    gold = oa.load_golden('predictive')
    S = cases.build(bl, case)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(case))
    assert S._posterior_pending.source == (0 if cases.CASES[case]['study'] == 'Study' else 1)
    x = gold[case + '_x']
    with Launched() as k:
        prob = S.simulate(x, t='all')
        dens = S.simulate(x, t='all', density=True)
    k.require('contract_kernel')
    assert S._posterior_pending is not None
    np.testing.assert_allclose(prob, gold[case + '_prob'], rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(dens, gold[case + '_density'], rtol=1e-9, atol=1e-300)
    sim = oa.load_golden('simulate')
    if case + '_avg' in sim:
        np.testing.assert_allclose(S.simulate(x), sim[case + '_avg'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(S.simulate(x, t=float(sim[case + '_t'])), sim[case + '_at'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(S.simulate(x, density=True), sim[case + '_avg_density'], rtol=1e-9, atol=1e-300)
        assert S._posterior_pending is not None


def test_changepoint_study_on_the_average_posterior(eng):
    S = cases.build(bl, 'c1_coal_changepoint')
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs('c1_coal_changepoint'))
    assert S._posterior_pending.source == 1
    x = np.arange(0.0, 9.0)
    out, k = simulate_everything(S, x)
    k.require('contract_kernel', 'tabulate_rows_kernel')
    check_against_host(S, x, out)


def test_option_predictive_0_and_non_finite_values_take_the_host_path(eng):
    """Option predictive = 0: the parent's host code -- a row or the time average leaves the device, the sums are numpy's -- and t='all'
    copies the sequence to the host first.  A non-finite value sends the whole call the same way."""
    S = pc.build_model(bl, 'gaussian2d')
    x = pc.MODELS['gaussian2d'][1]
    T = 19
    S.fit(silent=True)
    eng.set_option('predictive', 0)
    try:
        with Launched() as k:
            host = {(T // 2, d): S.simulate(x, t=S.formattedTimestamps[T // 2], density=d) for d in (False, True)}
            host.update({(None, d): S.simulate(x, density=d) for d in (False, True)})
            assert S._posterior_pending is not None
            host.update({('all', d): S.simulate(x, t='all', density=d) for d in (False, True)})
    finally:
        eng.set_option('predictive', 1)
    k.forbid('contract_kernel', 'tabulate_rows_kernel', 'combine_kernel')
    S.fit(silent=True)
    xn = np.array([0.5, np.nan, 1.0])
    with Launched() as kn, np.errstate(all='ignore'):
        got_nan = S.simulate(xn, t=S.formattedTimestamps[3], density=True)
    kn.forbid('contract_kernel', 'tabulate_rows_kernel', 'combine_kernel')
    dev, k = simulate_everything(S, x)
    k.require('contract_kernel', 'tabulate_rows_kernel')
    for (index, density), got in host.items():
        with np.errstate(all='ignore'):
            want = pc.host_simulate(S, x, index, density)
        if index is None:                                            # (the time average came from the device's own reduction)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(got, want), (index, density)
    check_against_host(S, x, dev)
    with np.errstate(all='ignore'):
        assert np.array_equal(got_nan, pc.host_simulate(S, xn, 3, True), equal_nan=True)


def test_small_single_calls_stay_on_the_host(eng):
    """Fewer than 8 values and fewer than 16 384 cells x values, one row: the host path (the measured threshold of
    profiles/predictive_notes.md); the band over all time stamps goes to the device at any size, and so does a larger single call."""
    S = pc.build_model(bl, 'bernoulli')
    S.fit(silent=True)
    assert bl.Study.PREDICTIVE_MIN_VALUES == 8 and bl.Study.PREDICTIVE_MIN_WORK == 16384
    x = np.array([0.0, 1.0])
    with Launched() as k:
        one, avg = S.simulate(x, t=S.formattedTimestamps[4], density=True), S.simulate(x, density=True)
    k.forbid('contract_kernel', 'lik_table_kernel')
    with Launched() as k:
        band = S.simulate(x, t='all', density=True)
    k.require('contract_kernel', 'lik_table_kernel')
    with Launched() as k:
        more = S.simulate(np.tile(x, 4), t=S.formattedTimestamps[4], density=True)
    k.require('contract_kernel')
    assert S._posterior_pending is not None
    np.testing.assert_allclose(band[4], one, rtol=1e-12)
    np.testing.assert_allclose(more, np.tile(one, 4), rtol=1e-12)
    np.testing.assert_allclose(avg, pc.host_simulate(S, x, None, True), rtol=1e-12)
    S2 = pc.build_model(bl, 'gaussian2d')                        # 4 values x 407 cells: host; 4 x 16 384 cells: device
    S2.fit(silent=True)
    with Launched() as k:
        S2.simulate(np.linspace(-1.0, 1.0, 4))
    k.forbid('contract_kernel')
    S3 = cases.build(bl, 'c3_small')
    S3.fit(silent=True)
    with Launched() as k:
        S3.simulate(np.linspace(-1.0, 1.0, 4))
    k.require('contract_kernel')


# ---- error paths ---------------------------------------------------------------------------------------------------------------------------

def _model(grid, om=_abi.OM_TABLE):
    ms = model_of(grid)
    cp = _abi.Problem()
    cp.ndim, cp.obs_model = len(ms), om
    for k, m in enumerate(ms):
        cp.n[k] = len(m)
        cp.marginal[k] = _abi.dptr(m)
    return cp, ms


def refused(e, *args):
    rc = e.lib.blhip_posterior_predictive(e.ctx, *args)
    msg = (e.lib.blhip_last_error(e.ctx) or b'').decode()
    assert rc != 0 and msg.strip(), 'rc = %d, message %r' % (rc, msg)
    return msg


def test_error_paths(eng):
    G, X = 105, 5
    cp, keep = _model((3, 7, 5))
    rows, x, out = pc.likelihood_rows(X, G, 1), np.zeros(X), np.empty(T_SEQ * X)
    R, Xp, O = _abi.dptr(rows), _abi.dptr(x), _abi.dptr(out)
    fresh = extra_engine(eng.device)
    assert 'no posterior kept' in refused(fresh, 0, 0, 0, 1, 0, C.byref(cp), Xp, X, None, R, O)
    assert 'not finalised' in refused(fresh, 1, 0, 0, 1, 0, C.byref(cp), Xp, X, None, R, O)
    del fresh
    eng.accum_begin(T_SEQ, G)
    assert 'not finalised' in refused(eng, 1, 0, 0, 1, 0, C.byref(cp), Xp, X, None, R, O)
    posts, acc = sequences(eng, G)
    good = lambda: eng.predictive(0, 1, keep, _abi.OM_TABLE, x, 2, 9, False, host_rows=rows)
    first = good()
    for t0, t1 in ((-1, 3), (0, T_SEQ + 1), (4, 4), (5, 4), (T_SEQ, T_SEQ + 1)):
        for average in (0, 1):
            assert 'range' in refused(eng, 0, 0, t0, t1, average, C.byref(cp), Xp, X, None, R, O)
            assert 'range' in refused(eng, 1, 0, t0, t1, average, C.byref(cp), Xp, X, None, R, O)
    for chain in (-1, CHAINS):
        assert 'chain' in refused(eng, 0, chain, 0, 1, 0, C.byref(cp), Xp, X, None, R, O)
    assert 'source' in refused(eng, 2, 0, 0, 1, 0, C.byref(cp), Xp, X, None, R, O)
    other, keep2 = _model((3, 7, 6))
    assert 'does not match' in refused(eng, 0, 0, 0, 1, 0, C.byref(other), Xp, X, None, R, O)
    assert 'NULL' in refused(eng, 0, 0, 0, 1, 0, None, Xp, X, None, R, O)
    assert 'NULL' in refused(eng, 0, 0, 0, 1, 0, C.byref(cp), Xp, X, None, R, None)
    assert 'NULL' in refused(eng, 0, 0, 0, 1, 0, C.byref(cp), None, X, None, None, O)
    refused(eng, 0, 0, 0, 1, 0, C.byref(cp), Xp, 0, None, R, O)
    # a model without rows on the device and none from the caller; a Poisson value outside the direct formula; a non-finite value
    assert 'host_rows' in refused(eng, 0, 0, 0, 1, 0, C.byref(cp), Xp, X, None, None, O)
    gm, keep3 = _model((105,), _abi.OM_GAUSSIAN_MEAN)
    assert 'host_rows' in refused(eng, 0, 0, 0, 1, 0, C.byref(gm), Xp, X, None, None, O)
    po, keep4 = _model((105,), _abi.OM_POISSON)
    kf = np.ones(X)
    assert 'x_step' in refused(eng, 0, 0, 0, 1, 0, C.byref(po), Xp, X, None, None, O)
    xb = np.array([0.0, 1.0, 2.5, 3.0, 4.0])
    assert 'direct formula' in refused(eng, 0, 0, 0, 1, 0, C.byref(po), _abi.dptr(xb), X, _abi.dptr(kf), None, O)
    xb[2] = np.inf
    assert 'finite' in refused(eng, 0, 0, 0, 1, 0, C.byref(po), _abi.dptr(xb), X, _abi.dptr(kf), None, O)
    ga, keep5 = _model((105,), _abi.OM_GAUSSIAN)
    assert 'parameter' in refused(eng, 0, 0, 0, 1, 0, C.byref(ga), Xp, X, None, None, O)
    # ... and the next good call gives what the first one gave
    assert np.array_equal(good(), first)
    want, bound = reference(posts[1][2:9], rows, False)
    within(first, want, bound, 'after the refusals')
    eng.accum_end()
