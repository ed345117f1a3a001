"""
Probability queries of the parser at many time steps on the device (bayesloop_amd/csrc/blhip_query.hpp, blhip_posterior_query):
``P(query, t='all')`` / ``Study.eval`` with a vector of time stamps.

The kernels alone.  The sequence is what a kept small 1-D fit and its finalised average left on the device, read back bit for bit; the
program, its tables and B's columns and probabilities are handed to blhip_posterior_query directly, so neither a fit nor the parser is
under test.  The indicator of every cell (pair) is computed in NumPy float64 by the same sequence of operations (query_program_ref.py),
the expected value is a longdouble sum of the same terms.  Bounds per entry:

* one space: the result is a sum of at most G non-negative terms in SOME order (lanes, waves, slabs): every term passes at most G - 1
  additions, each off by at most u = 2 ** -53 of the partial sum, which never exceeds the total:  (G + 1) u sum(terms) x SLACK
  (tests/highprec.py; additions are exact below the normal range, so no absolute term).
* pairs: a term pA[i] pB[j] passes at most G_b - 1 additions before and G_a - 1 after its one multiplication, which is off by u of the
  product or, below the normal range, by the subnormal step; the normaliser (sum pA)(sum pB) carries fewer roundings than that, the
  final division one more:  (G_a G_b + 2) u sum(terms) + G_a G_b TINY, terms = pA[i] pB[j] / normaliser where the indicator holds.

Programs made of + - * / sqrt abs, comparisons, tables and constants round exactly as NumPy does: their grids are multiples of 1/2 and
1/4, so every comparison meets exact ties (== and <= at grid values), and they produce NaN and +-inf (0 / 0, x / 0), which compare false
as in NumPy.  Programs that call exp / log / pow / sin / cos may differ from NumPy's by ulps; each such case asserts first, on the host,
that min |lhs - rhs| over all finite cells and steps is at least 1e-6 max(1, |lhs|, |rhs|) -- so no indicator can flip -- and still
compares every cell of every step.  (log of a non-positive number gives NaN / -inf on both sides.)

Shapes: G of 2, 105 (3 x 5 x 7), 1260 (36 x 35) and two slabs + 5 cells of the plan (2053; pairs: 517); 1, 15, 16, 17, 33 steps as a
shuffled list of rows with repeats; G_b of 1, 5, 257, constant and per step; with and without series values; the five relations; a
budget that forces two step chunks.  Which kernels ran is read from the library's registry and asserted.

End to end: the cases of tests/golden/parser_series.npz through ``P(query, t='all')`` on the HipEngine at the bar of tests/test_parser.py,
1e-9 + 1e-9 |want|, with the kernel each plan takes -- or none, for the plans that stay on the loop.
"""
import ctypes as C
import os

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import HipEngine, extra_engine
from bayesloop_amd.exceptions import BackendError
import cases
import highprec as hp
import parser_series_cases as psc
import query_program_ref as qref
from conftest import kernel_census

pytestmark = pytest.mark.gpu

L = _abi
ROWS = {False: 'blq::query_rows_kernel<false>', True: 'blq::query_rows_kernel<true>'}
PAIRS = {False: 'blq::query_pairs_kernel<false>', True: 'blq::query_pairs_kernel<true>'}
COMBINE = 'blq::combine_kernel'
QUERY_KERNELS = tuple(ROWS.values()) + tuple(PAIRS.values()) + (COMBINE,)
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'parser_series.npz'))


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
    return {name: c for c, name in kernel_census() if name in QUERY_KERNELS}


class Launched:
    """with Launched() as k: ... ; k.count[kernel] = launches inside (the query kernels only, by their full names)"""

    def __enter__(self):
        self.before = _counts()
        assert sorted(self.before) == sorted(QUERY_KERNELS), sorted(self.before)
        self.count = {}
        return self

    def __exit__(self, *exc):
        after = _counts()
        self.count = {k: after[k] - self.before[k] for k in after if after[k] > self.before[k]}

    def only(self, kernel, times=1):
        assert self.count == {kernel: times, COMBINE: times}, self.count


def within(got, want, bound, what):
    q = hp.worst(got, want, bound)
    print('%s: worst |error| / bound = %.3g' % (what, q))
    assert q <= 1.0, '%s: worst |error| / bound = %.3g at (index, got, want, bound) = %r' % (what, q, hp.worst_at(got, want, bound))


# ---- the kernels alone -----------------------------------------------------------------------------------------------------------------
T_SEQ, CHAINS = 33, 3
N_STEPS = (1, 15, 16, 17, 33)
GRIDS_ROWS = {'2': (2,), '3x5x7': (3, 5, 7), '36x35': (36, 35), 'two-slabs+5': (2053,)}
GRIDS_PAIRS = {'2': (2,), '3x5x7': (3, 5, 7), '36x35': (36, 35), 'two-slabs+5': (517,)}
_PROBLEMS, _SEQUENCES = {}, {}


def sequences(eng, G):
    """A kept, accumulating fit of CHAINS chains on a 1-D grid of G cells, then the finalised average: -> (source, chain, rows (T, G) as the
    device holds them) of the last chain's posterior and of the average posterior.  The device keeps what the LAST call left."""
    if G not in _PROBLEMS:
        data = cases.gm_data(5, T_SEQ)
        data[:, 1] = 0.2 if G > 2 else 4.0
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
    return ((0, CHAINS - 1, eng.posterior(CHAINS - 1, T_SEQ, [G])), (1, 0, eng.accum_read(T_SEQ, [G])))


def marginals(shape):
    """multiples of 1/2 around zero: products, cubes and quotients by 1 and 2 of them are exact, ties abound"""
    return [(np.arange(n) - n // 3) * 0.5 for n in shape]


def step_list(n, seed):
    steps = np.random.RandomState(seed).randint(0, T_SEQ, size=n)
    if n > 1:
        steps[-1] = steps[0]                      # (a repeat)
    return steps.astype(np.int64)


def exact_programs(shape):
    """name -> (ops, consts, series or None): + - * / sqrt abs, comparisons, a table, constants"""
    last, n_last = len(shape) - 1, shape[-1]
    table = (np.arange(n_last) % 7) * 0.5
    thr = 2.0
    out = {}
    # m0 ** 3 + table[last] + (m_last - 1) / (m_last - 1) - thr: 0 / 0 where m_last = 1
    out['cube+table+0/0'] = ([(L.LP_PARAM, 0), (L.LP_POWI, 3), (L.LP_AXIS, last | (2 << 2)), (L.LP_ADD, 0),
                              (L.LP_PARAM, last), (L.LP_CONST, 0), (L.LP_NEG, 0), (L.LP_ADD, 0), (L.LP_PARAM, last), (L.LP_CONST, 0), (L.LP_NEG, 0), (L.LP_ADD, 0),
                              (L.LP_DIV, 0), (L.LP_ADD, 0), (L.LP_CONST, 1), (L.LP_NEG, 0), (L.LP_ADD, 0)], [1.0, thr] + table.tolist(), None)
    # (m0 < m_last) + (m0 <= m_last) + (m0 == m_last) + |m0| - sqrt(m_last ** 2) + m0 / (m_last - 1) - 1.5: x / 0 where m_last = 1
    out['comparisons+x/0'] = ([(L.LP_PARAM, 0), (L.LP_PARAM, last), (L.LP_LT, 0), (L.LP_PARAM, 0), (L.LP_PARAM, last), (L.LP_LE, 0), (L.LP_ADD, 0),
                               (L.LP_PARAM, 0), (L.LP_PARAM, last), (L.LP_EQ, 0), (L.LP_ADD, 0), (L.LP_PARAM, 0), (L.LP_ABS, 0), (L.LP_ADD, 0),
                               (L.LP_PARAM, last), (L.LP_POWI, 2), (L.LP_SQRT, 0), (L.LP_NEG, 0), (L.LP_ADD, 0),
                               (L.LP_PARAM, 0), (L.LP_PARAM, last), (L.LP_CONST, 0), (L.LP_NEG, 0), (L.LP_ADD, 0), (L.LP_DIV, 0), (L.LP_ADD, 0),
                               (L.LP_CONST, 1), (L.LP_NEG, 0), (L.LP_ADD, 0)], [1.0, 1.5], None)
    # (m0 - c_s) * 2 + m_last / 2 - d_s
    n = max(N_STEPS)
    series = np.stack([(np.arange(n) % 5) * 0.25 - 0.5, (np.arange(n) % 3) * 0.5], axis=1)
    out['series'] = ([(L.LP_PARAM, 0), (L.LP_STEP, 0), (L.LP_NEG, 0), (L.LP_ADD, 0), (L.LP_CONST, 0), (L.LP_MUL, 0), (L.LP_PARAM, last), (L.LP_CONST, 1), (L.LP_MUL, 0),
                      (L.LP_ADD, 0), (L.LP_STEP, 1), (L.LP_NEG, 0), (L.LP_ADD, 0)], [2.0, 0.5], series)
    return out


def libm_programs(shape):
    """name -> (ops of lhs, consts, series or None, rhs per step or a number): exp log pow sin cos; f = lhs - rhs"""
    last = len(shape) - 1
    # exp(0.3 m0) + log(m_last) + sin(m0) cos(m_last) + (|m0| + 0.5) ** (m_last / 4)
    lhs = [(L.LP_CONST, 0), (L.LP_PARAM, 0), (L.LP_MUL, 0), (L.LP_EXP, 0), (L.LP_PARAM, last), (L.LP_LOG, 0), (L.LP_ADD, 0),
           (L.LP_PARAM, 0), (L.LP_SIN, 0), (L.LP_PARAM, last), (L.LP_COS, 0), (L.LP_MUL, 0), (L.LP_ADD, 0),
           (L.LP_PARAM, 0), (L.LP_ABS, 0), (L.LP_CONST, 1), (L.LP_ADD, 0), (L.LP_PARAM, last), (L.LP_CONST, 2), (L.LP_MUL, 0), (L.LP_POW, 0), (L.LP_ADD, 0)]
    consts = [0.3, 0.5, 0.25, 1.7345678]
    n = max(N_STEPS)
    return {'libm': (lhs, consts, None, 1.7345678), 'libm+series': (lhs, consts, (1.2345678 + 0.137 * np.arange(n)).reshape(n, 1), None)}


def minus_rhs(lhs, series):
    """lhs -> lhs - rhs with rhs the constant 3 or the series value 0"""
    return list(lhs) + [((L.LP_STEP, 0) if series is not None else (L.LP_CONST, 3)), (L.LP_NEG, 0), (L.LP_ADD, 0)]


def assert_margin(lhs_ops, consts, marg, rhs, b_values=None):
    """no finite cell (pair) within 1e-6, relatively, of any of the thresholds rhs"""
    lhs = qref.interpret(lhs_ops, consts, marg, None, b_values)
    fin = np.isfinite(lhs)
    for r in np.atleast_1d(rhs):
        gap = np.abs(lhs[fin] - r) / np.maximum(1.0, np.maximum(np.abs(lhs[fin]), abs(r)))
        assert gap.size == 0 or gap.min() >= 1e-6, (r, gap.min())
    return int(fin.sum()), int((~fin).sum())


def rows_reference(seq, steps, ops, consts, relation, marg, series):
    G = seq.shape[1]
    want = np.zeros(len(steps), dtype=np.longdouble)
    ind = None
    for s, row in enumerate(steps):
        if ind is None or series is not None:
            ind = qref.indicator(relation, qref.interpret(ops, consts, marg, None if series is None else series[s]))
        want[s] = np.asarray(seq[row], dtype=np.longdouble)[ind].sum()
    return want, np.asarray(hp.SLACK * (G + 1) * hp.U * want, dtype=np.longdouble)


@pytest.mark.parametrize('grid', sorted(GRIDS_ROWS), ids=sorted(GRIDS_ROWS))
def test_one_space_against_longdouble_sums(eng, grid):
    shape = GRIDS_ROWS[grid]
    G = int(np.prod(shape))
    if grid == 'two-slabs+5':
        plan = HipEngine.query_plan(G, max(N_STEPS))
        assert (plan['slab'], plan['n_slabs']) == ((G - 5) // 2, 3)
    marg = marginals(shape)
    programs, ties = [], set()
    for name, (ops, consts, series) in exact_programs(shape).items():
        f = np.stack([qref.interpret(ops, consts, marg, sv) for sv in ([None] if series is None else series)])
        if G > 2:
            assert (f > 0).any() and (f < 0).any(), name                                      # both sides of the threshold
        if (f == 0.0).any():
            ties.add(name)                                                                    # exact ties
        if 'x/0' in name and G > 2:
            assert np.isinf(f).any(), name
        if '0/0' in name and G > 2:
            assert np.isnan(f).any(), name
        programs += [(name, ops, consts, series, rel) for rel in (L.QR_LT, L.QR_LE, L.QR_EQ, L.QR_GT, L.QR_GE)]
    assert 'series' in ties and (len(shape) == 1 or len(ties) == 3), ties
    for name, (lhs, consts, series, rhs) in libm_programs(shape).items():
        fin, odd = assert_margin(lhs, consts, marg, rhs if series is None else series[:, 0])
        assert fin > 0 and (odd > 0 or G == 2)                                                # (log of a non-positive grid value)
        programs += [(name, minus_rhs(lhs, series), consts, series, rel) for rel in (L.QR_LT, L.QR_GE)]
    seqs = sequences(eng, G)
    launched = set()
    for n_i, n in enumerate(N_STEPS):
        steps = step_list(n, 100 + n)
        for source, chain, seq in seqs:
            for p_i, (name, ops, consts, series, rel) in enumerate(programs):
                if (p_i + n_i + source) % 2 and n not in (17, 33):
                    continue                                                                   # (every program at 17 and 33 steps, half of them elsewhere)
                sv = None if series is None else series[:n]
                with Launched() as k:
                    got = eng.posterior_query(source, chain, steps, ops, consts, rel, marg, series=sv)
                k.only(ROWS[series is not None])
                launched.add(series is not None)
                want, bound = rows_reference(seq, steps, ops, consts, rel, marg, sv)
                within(got, want, bound, '%s, relation %d, %d steps, source %d' % (name, rel, n, source))
                if n == 17:
                    assert np.array_equal(got, eng.posterior_query(source, chain, steps, ops, consts, rel, marg, series=sv)), 'two calls on the same inputs differ'
    assert launched == {False, True}
    eng.accum_end()


def b_space(G_b, n, seed):
    rng = np.random.RandomState(seed)
    b_values = np.stack([(np.arange(G_b) - G_b // 2) * 0.5, (np.arange(G_b) % 3) * 1.0])        # multiples of 1/2 with a zero; 0, 1, 2
    if G_b == 1:
        per_step = np.full((n, 1), 0.5)                     # (not normalised, and a power of two: the products stay exact)
    else:
        per_step = rng.random_sample((n, G_b)) * 10.0 ** rng.randint(-3, 1, size=(n, G_b))
        per_step[:, 1] = 0.0                                # exact zeros among the probabilities
    return b_values, per_step


def pair_programs(shape):
    last, n_last = len(shape) - 1, shape[-1]
    table = (np.arange(n_last) % 7) * 0.5
    n = max(N_STEPS)
    out = {}
    # m0 * b0 + table[last] + m_last / b1 - 1: x / 0 and 0 / 0 where b1 = 0
    out['product+table+x/0'] = ([(L.LP_PARAM, 0), (L.QP_BCOL, 0), (L.LP_MUL, 0), (L.LP_AXIS, last | (1 << 2)), (L.LP_ADD, 0), (L.LP_PARAM, last), (L.QP_BCOL, 1), (L.LP_DIV, 0),
                                 (L.LP_ADD, 0), (L.LP_CONST, 0), (L.LP_NEG, 0), (L.LP_ADD, 0)], [1.0] + table.tolist(), None)
    # m0 * b0 - c_s + m_last / 2
    out['series'] = ([(L.LP_PARAM, 0), (L.QP_BCOL, 0), (L.LP_MUL, 0), (L.LP_STEP, 0), (L.LP_NEG, 0), (L.LP_ADD, 0), (L.LP_PARAM, last), (L.LP_CONST, 0), (L.LP_MUL, 0),
                      (L.LP_ADD, 0)], [0.5], ((np.arange(n) % 5) * 0.25 - 0.5).reshape(n, 1))
    return out


def pair_libm_program(shape):
    last = len(shape) - 1
    # exp(0.01 m0) * b0 + log(|b0| + m_last)
    lhs = [(L.LP_CONST, 0), (L.LP_PARAM, 0), (L.LP_MUL, 0), (L.LP_EXP, 0), (L.QP_BCOL, 0), (L.LP_MUL, 0), (L.QP_BCOL, 0), (L.LP_ABS, 0), (L.LP_PARAM, last), (L.LP_ADD, 0),
           (L.LP_LOG, 0), (L.LP_ADD, 0)]
    return lhs, [0.01, 0.25, 0.5, 0.7345678]


def pairs_reference(seq, steps, ops, consts, relation, marg, series, b_values, b_prob, b_const):
    G_a, G_b = seq.shape[1], b_values.shape[1]
    want = np.zeros(len(steps), dtype=np.longdouble)
    ind = None
    for s, row in enumerate(steps):
        if ind is None or series is not None:
            ind = qref.indicator(relation, qref.interpret(ops, consts, marg, None if series is None else series[s], b_values)).astype(np.longdouble)
        pa, pb = np.asarray(seq[row], dtype=np.longdouble), np.asarray(b_prob[0 if b_const else s], dtype=np.longdouble)
        want[s] = (pa * (ind @ pb)).sum() / (pa.sum() * pb.sum())
    return want, np.asarray((G_a * G_b + 2) * hp.U * want + G_a * G_b * hp.TINY, dtype=np.longdouble)


@pytest.mark.parametrize('G_b', (1, 5, 257))
@pytest.mark.parametrize('grid', sorted(GRIDS_PAIRS), ids=sorted(GRIDS_PAIRS))
def test_pairs_against_longdouble_sums(eng, grid, G_b):
    shape = GRIDS_PAIRS[grid]
    G = int(np.prod(shape))
    if grid == 'two-slabs+5':
        plan = HipEngine.query_plan(G, max(N_STEPS), n_b=G_b)
        assert (plan['slab'], plan['n_slabs']) == ((G - 5) // 2, 3)
    marg = marginals(shape)
    b_values, b_rows = b_space(G_b, max(N_STEPS), 7 * G + G_b)
    programs = []
    for name, (ops, consts, series) in pair_programs(shape).items():
        f = np.stack([qref.interpret(ops, consts, marg, sv, b_values) for sv in ([None] if series is None else series[:5])])
        if G > 2 and G_b > 1:
            assert (f == 0.0).any() and (f > 0).any() and (f < 0).any(), name                 # exact ties, both sides of the threshold
        if 'x/0' in name:
            assert np.isinf(f).any() or G_b == 1 and G == 2, name
            assert np.isnan(f).any() or G == 2, name
        programs += [(name, ops, consts, series, rel) for rel in (L.QR_LT, L.QR_LE, L.QR_EQ, L.QR_GT, L.QR_GE)]
    lhs, consts = pair_libm_program(shape)
    fin, odd = assert_margin(lhs, consts, marg, consts[3], b_values)
    assert fin > 0
    programs += [('libm', list(lhs) + [(L.LP_CONST, 3), (L.LP_NEG, 0), (L.LP_ADD, 0)], consts, None, rel) for rel in (L.QR_LT, L.QR_GE)]
    seqs = sequences(eng, G)
    launched, case = set(), 0
    for n in N_STEPS:
        steps = step_list(n, 200 + n)
        for source, chain, seq in seqs:
            for name, ops, consts, series, rel in programs:
                case += 1
                b_const = bool(case % 2)
                if (case // 2 + source) % 2 and n not in (17, 33):
                    continue
                sv = None if series is None else series[:n]
                b_prob = b_rows[n % 7:n % 7 + 1] if b_const else b_rows[:n]
                with Launched() as k:
                    got = eng.posterior_query(source, chain, steps, ops, consts, rel, marg, series=sv, b_values=b_values, b_prob=b_prob, b_const=b_const)
                k.only(PAIRS[series is not None])
                launched.add((series is not None, b_const))
                want, bound = pairs_reference(seq, steps, ops, consts, rel, marg, sv, b_values, b_prob, b_const)
                within(got, want, bound, '%s, relation %d, %d steps, source %d, G_b %d%s' % (name, rel, n, source, G_b, ', constant' if b_const else ''))
                if n == 17:
                    again = eng.posterior_query(source, chain, steps, ops, consts, rel, marg, series=sv, b_values=b_values, b_prob=b_prob, b_const=b_const)
                    assert np.array_equal(got, again), 'two calls on the same inputs differ'
    assert launched == {(False, False), (False, True), (True, False), (True, True)}
    eng.accum_end()


def fixed_bytes(ops, consts, marg, b_values=None, b_prob=None, b_const=False):
    """the uploads of a call that do not depend on the step as blhip_posterior_query places them: the program, the constants, B's columns, a
    constant b_prob and the marginal grids, each rounded up to 256 bytes (an absent one takes one 256-byte place)"""
    up = lambda nbytes: (nbytes + 255) // 256 * 256
    return (up(8 * len(ops)) + up(8 * max(1, len(consts))) + up(8 * max(1, 0 if b_values is None else b_values.size))
            + up(8 * (b_prob.shape[1] if b_const else 1)) + sum(up(8 * len(m)) for m in marg))


def test_two_step_chunks_and_refusals():
    """A budget with room for 32 of the 33 steps: two chunks, each combined on its own, land in their places of the result -- for both
    kernels.  Then every refusal of the entry point, each followed by a call that works.  (A context of its own: the options die with it.)"""
    shape = GRIDS_PAIRS['36x35']
    G, n = 1260, 33
    marg = marginals(shape)
    steps = step_list(n, 5)
    e = extra_engine(bl.get_engine().device)
    try:
        ops_one, consts_one, series_one = exact_programs(shape)['series']
        with pytest.raises(BackendError, match='no posterior kept'):
            e.posterior_query(0, 0, steps, ops_one, consts_one, L.QR_GT, marg, series=series_one)
        with pytest.raises(BackendError, match='not finalised'):
            e.posterior_query(1, 0, steps, ops_one, consts_one, L.QR_GT, marg, series=series_one)
        (source, chain, seq), _ = sequences(e, G)
        ops_two, consts_two, series_two = pair_programs(shape)['series']
        b_values, b_rows = b_space(257, n, 3)
        calls = ((ROWS[True], dict(ops=ops_one, consts=consts_one, series=series_one), dict()),
                 (PAIRS[True], dict(ops=ops_two, consts=consts_two, series=series_two, b_values=b_values, b_prob=b_rows), dict(n_b=257)))
        for kernel, kw, plan_kw in calls:
            fixed = fixed_bytes(kw['ops'], kw['consts'], marg, kw.get('b_values'), kw.get('b_prob'))
            ask = lambda budget: HipEngine.query_plan(G, n, kw['series'].shape[1], fixed_bytes=fixed, budget=budget, **plan_kw)
            budget = ask(float(1 << 62))['min_budget_bytes']
            while ask(budget)['steps_per_chunk'] < 32:
                budget += 256
            assert (ask(budget)['steps_per_chunk'], ask(budget)['n_chunks']) == (32, 2)
            e.set_option('mem_budget_bytes', budget / 0.9 + 64)          # (the library plans within 0.9 of the option)
            with Launched() as k:
                got = e.posterior_query(source, chain, steps, relation=L.QR_GT, marginal=marg, **kw)
            k.only(kernel, 2)
            e.set_option('mem_budget_bytes', 1e15)
            with Launched() as k:
                whole = e.posterior_query(source, chain, steps, relation=L.QR_GT, marginal=marg, **kw)
            k.only(kernel, 1)
            assert np.array_equal(got, whole), 'the chunks are no pieces of the unchunked result'
            if 'b_prob' in kw:
                want, bound = pairs_reference(seq, steps, kw['ops'], kw['consts'], L.QR_GT, marg, kw['series'], b_values, b_rows, False)
            else:
                want, bound = rows_reference(seq, steps, kw['ops'], kw['consts'], L.QR_GT, marg, kw['series'])
            within(got, want, bound, 'two chunks, %s' % kernel)
        # ---- refusals: nothing is launched, the message says why, the next call works
        good = dict(ops=ops_one, consts=consts_one, series=series_one, relation=L.QR_GT, marginal=marg)
        refusals = (('outside the 33 rows', dict(steps=np.array([0, T_SEQ] + [1] * 31))), ('outside the 33 rows', dict(steps=np.array([-1] + [1] * 32))),
                    ('does not match the sequence', dict(marginal=marginals((36, 34)))), ('stack underflow', dict(ops=ops_one[1:])),
                    ('leaves 2 values', dict(ops=list(ops_one) + [(L.LP_PARAM, 0)])), ('AXIS', dict(ops=[(L.LP_AXIS, 1 | (1 << 2))], consts=np.ones(35))),
                    ('STEP 2 out of range', dict(ops=[(L.LP_STEP, 2)])), ('not finite', dict(series=np.where(np.arange(33)[:, None] == 4, np.inf, series_one))),
                    ('relation', dict(relation=7)), ('chain', dict(chain=CHAINS)))
        served = e.posterior_query(source, chain, steps, **good)
        for message, change in refusals:
            args = dict(good, source=source, chain=chain, steps=steps)
            args.update(change)
            with Launched() as k:
                with pytest.raises(BackendError, match=message):
                    e.posterior_query(**args)
            assert k.count == {}, (message, k.count)
            assert np.array_equal(e.posterior_query(source, chain, steps, **good), served)
        q = _abi.Query()
        rc = e.lib.blhip_posterior_query(e.ctx, 0, chain, steps.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(q), None)
        assert rc == -1 and 'host_out is NULL' in e.lib.blhip_last_error(e.ctx).decode()
        out = np.empty(n)
        rc = e.lib.blhip_posterior_query(e.ctx, 0, chain, None, n, C.byref(q), _abi.dptr(out))
        assert rc == -1 and 'steps is NULL' in e.lib.blhip_last_error(e.ctx).decode()
        rc = e.lib.blhip_posterior_query(e.ctx, 0, chain, steps.ctypes.data_as(C.POINTER(C.c_int64)), n, None, _abi.dptr(out))
        assert rc == -1 and 'query is NULL' in e.lib.blhip_last_error(e.ctx).decode()
        e.set_option('mem_budget_bytes', 64.0)
        with pytest.raises(BackendError, match='budget'):
            e.posterior_query(source, chain, steps, **good)
        e.set_option('mem_budget_bytes', 1e15)
        want, bound = rows_reference(seq, steps, ops_one, consts_one, L.QR_GT, marg, series_one)
        within(e.posterior_query(source, chain, steps, **good), want, bound, 'after the refusals')
    finally:
        e.accum_end()
        del e


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def close(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.abs(got - want) > 1e-9 + 1e-9 * np.abs(want)
    assert not bad.any(), (got[bad], want[bad])


# case -> (builder on the GPU engine, t, the kernel of its plan)
END_TO_END = {
    'coal_lt': ('coal', 'all', ROWS[False]), 'gauss_ratio': ('gauss', 'all', ROWS[False]), 'gauss_series': ('gauss', 'all', ROWS[True]),
    'gauss_sincos': ('gauss', 'all', ROWS[False]), 'gauss_exp': ('gauss', 'all', ROWS[False]), 'gauss_pow': ('gauss', 'all', ROWS[False]),
    'two_product': ('two', 'all', PAIRS[False]), 'two_difference': ('two', 'all', PAIRS[False]),
    'hyper_product': ('hyper_alone', 'all', PAIRS[False]), 'changepoint': ('changepoint_alone', [0, 1, 2, 3, 4], PAIRS[False]),
    'online': ('hyper', 'all', None),
}


@pytest.mark.parametrize('builder', sorted(set(v[0] for v in END_TO_END.values())))
def test_goldens_through_the_parser_on_the_device(eng, builder):
    S = psc.BUILDERS[builder](bl)
    with psc._quiet():
        P = bl.Parser(*S)
    for case, (b, t, kernel) in sorted(END_TO_END.items()):
        if b != builder:
            continue
        _, query, series, _, _ = psc.CASES[case]
        with Launched() as k:
            got = P(query, t=t, silent=True, series=series)
        if kernel is None:
            assert k.count == {}, (case, k.count)
        else:
            k.only(kernel)
        close(got, GOLDEN[case])
        assert np.array_equal(got, P(query, t=t, silent=True, series=series)), 'two calls on the same inputs differ'
        # the loop over the scalar call is the definition
        stamps = P._stamps(t)
        loop = np.array([P(psc.textual(query, series, i), t=ts, silent=True) for i, ts in enumerate(stamps)])
        close(got, loop)
    # the studies stay usable
    first = S[0]
    name = first.observationModel.parameterNames[0]
    if hasattr(first, 'getParameterDistributions') and builder != 'hyper':
        x, p = first.getParameterDistributions(name, plot=False)
        assert np.all(np.isfinite(p)) and len(p) == len(first.formattedTimestamps)
        before = first.eval(name + ' > 1', t=first.formattedTimestamps[1], silent=True)
        with psc._quiet():
            first.fit()
        assert abs(first.eval(name + ' > 1', t=first.formattedTimestamps[1], silent=True) - before) <= 1e-12


def test_plans_that_stay_on_the_loop(eng):
    S = psc.BUILDERS['two'](bl)
    with psc._quiet():
        P = bl.Parser(*S)
    want = np.array([P('(rate*rate2) + rate > 3', t=t, silent=True) for t in range(5)])
    with Launched() as k:
        got = P('(rate*rate2) + rate > 3', t='all', silent=True)                    # three spaces
    assert k.count == {} and np.array_equal(got, want)
    for option, value, back in (('parser_device', 0.0, 1.0), ('parser_pair_max', 2499.0, 6.4e7)):
        eng.set_option(option, value)
        try:
            with Launched() as k:
                got = P('rate*rate2 >= 4', t='all', silent=True)
                one = P('rate2 > 2', t='all', silent=True)
            close(got, GOLDEN['two_product'])
            if option == 'parser_device':
                assert k.count == {}, k.count
            else:
                k.only(ROWS[False])                                                 # (the cap bars the pair space, not the one-space query)
            assert np.array_equal(one, np.array([P('rate2 > 2', t=t, silent=True) for t in range(5)])) or option != 'parser_device'
        finally:
            eng.set_option(option, back)
    with Launched() as k:
        close(P('rate*rate2 >= 4', t='all', silent=True), GOLDEN['two_product'])
    k.only(PAIRS[False])
