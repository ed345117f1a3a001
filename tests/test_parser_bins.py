"""
Distribution queries of the parser at many time steps on the device (bayesloop_amd/csrc/blhip_bins.hpp, blhip_posterior_bins):
``P(query, t='all')`` / ``Study.eval`` for a query without a relation.

The kernels alone.  The sequences are what the device holds, read back bit for bit: the kept posteriors of a small 1-D fit with a narrow
likelihood (source 0, the last of three chains: exact zeros and values far below 1e-300) and a finalised average posterior folded from
rows the test makes (source 1: integer multiples of a power of two whose row sums are powers of two, so the normalisation is exact and so
is every sum of them in any order).  The maps are those of tests/parser_bins_cases.py for the slab length blhip_host_bins_plan reports.
Every entry is held

* to the longdouble sum of its cells within hp.marginal_bound(want, cells of the bin): n terms of one sign in any order,
  (n + 1) u |sum| x SLACK (tests/highprec.py);
* to the NumPy restatement of the kernels' order of additions (parser_bins_cases.kernel_order_sums) bit for bit;
* on the exact rows to np.bincount bit for bit: what differs there is mis-binned, not rounded.

End to end: the queries of parser_bins_cases.QUERIES through the parser on the HipEngine -- the kernels run (read from the library's
registry), the labels are the scalar call's, the probabilities are the loop's and the reference's within compare.GPU_TOL; what stays on
the loop launches nothing.
"""
import ctypes as C
import os

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem, HipEngine, extra_engine
from bayesloop_amd.exceptions import BackendError
import cases
import compare
import highprec as hp
import parser_bins_cases as pbc
from conftest import kernel_census

pytestmark = pytest.mark.gpu

psc = pbc.psc
BINS, COMBINE = 'blb::bins_kernel', 'blb::bins_combine_kernel'
REFERENCE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'parser_bins_reference.npz'))


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
    return {name: c for c, name in kernel_census() if name in (BINS, COMBINE)}


class Launched:
    """with Launched() as k: ... ; k.count[kernel] = launches inside (the two kernels of this file)"""

    def __enter__(self):
        self.before = _counts()
        assert sorted(self.before) == [COMBINE, BINS], sorted(self.before)
        self.count = {}
        return self

    def __exit__(self, *exc):
        after = _counts()
        self.count = {k: after[k] - self.before[k] for k in after if after[k] > self.before[k]}

    def both(self, times=1):
        assert self.count == {BINS: times, COMBINE: times}, self.count


def within(got, want, bound, what):
    q = hp.worst(got, want, bound)
    print('%s: worst |error| / bound = %.3g' % (what, q))
    assert q <= 1.0, '%s: worst |error| / bound = %.3g at (index, got, want, bound) = %r' % (what, q, hp.worst_at(got, want, bound))


# ---- the kernels alone -------------------------------------------------------------------------------------------------------------------
CHAINS = 3
SHAPE = HipEngine.bins_plan(1000, 7, 50)             # (host-only: the slab length and the steps of a block)
SLAB, SB = SHAPE['slab'], SHAPE['sb']
T_SEQ = 2 * SB + 3
MAPS = pbc.maps(SLAB)
_PROBLEMS = {}


def step_lists():
    rs = np.random.RandomState(3)
    out = [np.array([T_SEQ - 2])] + [np.arange(n) for n in (SB - 1, SB, SB + 1)]
    mixed = rs.randint(0, T_SEQ, size=2 * SB + 5)
    mixed[-1] = mixed[0]                              # unordered, with repeats
    return [s.astype(np.int64) for s in out + [mixed]]


def kept_sequence(eng, G):
    """source 0: a kept fit of CHAINS chains on a 1-D grid of G cells under a narrow likelihood -> (0, last chain, its rows as the device holds them)"""
    if G not in _PROBLEMS:
        data = cases.gm_data(5, T_SEQ)
        data[:, 1] = 0.2
        S = cases.build(bl, dict(study='Study', data=data, om=('GaussianMean', [('mean', ('cint', -8, 8, G))], 'default'), tm=('GRW', 'sigma', 0.1, 'mean', None)))
        S._checkConsistency()
        S._formatData()
        _PROBLEMS[G] = S._compile(silent=True)[0]
    res = eng.fit(_PROBLEMS[G], (np.linspace(0.15, 0.9, CHAINS) * 0.3).reshape(CHAINS, 1), keep_posterior=True)
    assert np.all(res.abort_step < 0)
    seq = eng.posterior(CHAINS - 1, T_SEQ, [G])
    if G >= 255:
        assert (seq == 0.0).any() and ((seq > 0.0) & (seq < 1e-300)).any(), 'the rows do not reach zeros and values below 1e-300'
    return 0, CHAINS - 1, seq


def exact_rows(G, seed):
    """(T_SEQ, G) integers >= 1 whose row sums are powers of two, times 2^-30"""
    rs = np.random.RandomState(seed)
    m = rs.randint(1, 2 ** 20, size=(T_SEQ, G)).astype(np.int64)
    total = m.sum(axis=1)
    m[:, -1] += (2 ** np.ceil(np.log2(total + 1)).astype(np.int64)) - total
    assert np.all(np.log2(m.sum(axis=1)) % 1 == 0) and m.max() < 2 ** 40
    return m.astype(np.float64) * 2.0 ** -30


def average_sequence(eng, G):
    """source 1: the finalised average posterior of ONE folded caller's sequence of exact rows -> (1, 0, its rows as the device holds them)"""
    rows = exact_rows(G, G)
    problem = FitProblem(obs_model=_abi.OM_TABLE, marginal=[np.arange(G, dtype=float)], lattice=[1.0], data=np.zeros(T_SEQ),
                         timestamps=np.arange(T_SEQ, dtype=float), prior=np.full(G, 1.0 / G), ops=[(_abi.OP_STATIC, 0)])
    eng.accum_begin(T_SEQ, G)
    eng.accum_fold_host(rows, 0.0)
    eng.accum_finalize(problem)
    seq = eng.accum_read(T_SEQ, [G])
    # the normalisation divided by a power of two: the device holds multiples of 2^-70 below 1, at most 41 bits wide -- sums of G <= 2^11 of them are exact
    scaled = seq * 2.0 ** 70
    assert np.array_equal(scaled, np.round(scaled)) and np.array_equal(seq.sum(axis=1), np.ones(T_SEQ))
    assert np.array_equal(seq * rows.sum(axis=1, keepdims=True), rows), 'the device does not hold the rows, exactly normalised'
    return 1, 0, seq


def reference(seq, steps, m, n_bins):
    """-> (longdouble sums (len(steps), n_bins), cells per bin)"""
    rows = seq[steps]
    want = np.zeros((len(steps), n_bins), dtype=hp.LD)
    counts = np.bincount(m[m >= 0], minlength=n_bins)
    order = np.argsort(m, kind='stable')
    order = order[m[order] >= 0]
    at = 0
    for b in np.nonzero(counts)[0]:
        want[:, b] = hp._sum(rows[:, order[at:at + counts[b]]], 1)
        at += counts[b]
    return want, counts


def check_call(eng, source, chain, seq, steps, name, exact):
    G, n_bins, m = MAPS[name]
    with Launched() as k:
        got = eng.posterior_bins(source, chain, steps, m, n_bins)
    if (m >= 0).any():
        k.both()
    else:
        assert k.count == {COMBINE: 1}, k.count
        assert not got.any(), 'a map that leaves every cell out gives exactly 0'
    assert got.shape == (len(steps), n_bins)
    want, counts = reference(seq, steps, m, n_bins)
    within(got, want, hp.marginal_bound(want, counts[None, :]), '%s, source %d, %d steps' % (name, source, len(steps)))
    gw = pbc.group_width(m, SLAB, 8)
    assert np.array_equal(got, pbc.kernel_order_sums(seq[steps], m, n_bins, SLAB, gw)), '%s: not the order of additions the header states' % name
    if exact:
        inside = m >= 0
        for i, s in enumerate(steps):
            assert np.array_equal(got[i], np.bincount(m[inside], weights=seq[s][inside], minlength=n_bins)), '%s: a cell landed in another bin' % name
    assert np.array_equal(got, eng.posterior_bins(source, chain, steps, m, n_bins)), 'two calls on the same inputs differ'


@pytest.mark.parametrize('G', sorted(set(v[0] for v in MAPS.values())))
def test_bins_against_longdouble_sums(eng, G):
    names = sorted(n for n, v in MAPS.items() if v[0] == G)
    assert HipEngine.bins_plan(G, 1, 5)['n_slabs'] == -(-G // SLAB)
    lists = step_lists()
    for make, exact in ((kept_sequence, False), (average_sequence, True)):
        if G == 1 and not exact:
            continue                                  # (a one-cell grid has no lattice to fit on; the average posterior covers G = 1)
        source, chain, seq = make(eng, G)
        for name in names:
            for steps in (lists if name in ('skewed', 'seam', 'G257-2bins', 'one-cell', '64bins') else lists[-1:]):
                check_call(eng, source, chain, seq, steps, name, exact)
    eng.accum_end()


def test_two_step_chunks_options_and_refusals():
    """A budget that forces two chunks gives the bits of one chunk; other slab lengths, steps per block and group widths (the options the
    probe measures with) give their own fixed order, with more than 64 KiB of LDS per block among them; then every refusal of the entry
    point, each followed by a call that works.  (A context of its own: the options die with it.)"""
    G, n_bins, m = MAPS['skewed']
    e = extra_engine(bl.get_engine().device)
    try:
        steps = step_lists()[-1]
        n = len(steps)
        with pytest.raises(BackendError, match='no posterior kept'):
            e.posterior_bins(0, 0, steps, m, n_bins)
        with pytest.raises(BackendError, match='not finalised'):
            e.posterior_bins(1, 0, steps, m, n_bins)
        source, chain, seq = kept_sequence(e, G)
        want, counts = reference(seq, steps, m, n_bins)
        bound = hp.marginal_bound(want, counts[None, :])
        whole = e.posterior_bins(source, chain, steps, m, n_bins)
        within(whole, want, bound, 'one chunk')
        ask = lambda budget: HipEngine.bins_plan(G, n_bins, n, m, budget=budget)
        budget = ask(float(1 << 62))['min_budget_bytes']
        while ask(budget)['steps_per_chunk'] < 2 * SB:
            budget += 256
        assert (ask(budget)['steps_per_chunk'], ask(budget)['n_chunks']) == (2 * SB, 2)
        try:
            e.set_option('mem_budget_bytes', budget / 0.9 + 64)          # (the library plans within 0.9 of the option)
            with Launched() as k:
                got = e.posterior_bins(source, chain, steps, m, n_bins)
            k.both(2)
        finally:
            e.set_option('mem_budget_bytes', 1e15)
        assert np.array_equal(got, whole), 'the chunks are no pieces of the unchunked result'
        # ---- the shape options
        for slab, sb, gw in ((256, 16, 4), (1024, 4, 16), (1024, 16, 2)):
            try:
                for key, v in (('bins_slab', slab), ('bins_sb', sb), ('bins_gw', gw)):
                    e.set_option(key, v)
                with Launched() as k:
                    got = e.posterior_bins(source, chain, steps, m, n_bins)
                k.both()
            finally:
                for key, v in (('bins_slab', SLAB), ('bins_sb', SB), ('bins_gw', 8)):
                    e.set_option(key, v)
            used = slab if 8 * sb * (2 * slab + 2) <= 160 * 1024 else 512          # (blb::shape halves a slab whose worst map would not fit the LDS)
            within(got, want, bound, 'slab %d, sb %d, gw %d' % (slab, sb, gw))
            assert np.array_equal(got, pbc.kernel_order_sums(seq[steps], m, n_bins, used, pbc.group_width(m, used, gw)))
        # ---- refusals: nothing is launched, the message says why, the next call works
        good = dict(source=source, chain=chain, steps=steps, bin=m, n_bins=n_bins)
        low = m.copy()
        low[7] = -2
        refusals = (('outside the %d rows' % T_SEQ, dict(steps=np.array([0, T_SEQ]))), ('outside the %d rows' % T_SEQ, dict(steps=np.array([-1, 1]))),
                    ('does not match the sequence', dict(bin=m[:-1])), (r'bin\[\d+\] = \d+ is outside', dict(n_bins=n_bins - 1)),
                    (r'bin\[7\] = -2 is outside', dict(bin=low)), ('n_bins = 0', dict(n_bins=0)), ('chain', dict(chain=CHAINS)), ('bad source', dict(source=2)),
                    ('not finalised', dict(source=1)))
        for message, change in refusals:
            with Launched() as k:
                with pytest.raises(BackendError, match=message):
                    e.posterior_bins(**dict(good, **change))
            assert k.count == {}, (message, k.count)
            assert np.array_equal(e.posterior_bins(**good), whole)
        sp, mp, out = steps.ctypes.data_as(C.POINTER(C.c_int64)), m.ctypes.data_as(C.POINTER(C.c_int32)), np.empty((n, n_bins))
        for args, word in (((sp, n, mp, G, n_bins, None), 'host_out is NULL'), ((None, n, mp, G, n_bins, _abi.dptr(out)), 'steps is NULL'),
                           ((sp, n, None, G, n_bins, _abi.dptr(out)), 'bin is NULL'), ((sp, 0, mp, G, n_bins, _abi.dptr(out)), 'n_steps = 0')):
            assert e.lib.blhip_posterior_bins(e.ctx, 0, chain, *args) == -1 and word in e.lib.blhip_last_error(e.ctx).decode(), word
        try:
            e.set_option('mem_budget_bytes', 64.0)
            with pytest.raises(BackendError, match='budget'):
                e.posterior_bins(**good)
        finally:
            e.set_option('mem_budget_bytes', 1e15)
        assert np.array_equal(e.posterior_bins(**good), whole)
    finally:
        e.accum_end()
        del e


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def close(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.abs(got - want) > compare.GPU_TOL['post_atol'] + compare.GPU_TOL['post_rtol'] * np.abs(want)
    assert not bad.any(), (got[bad], want[bad])


@pytest.mark.parametrize('builder', sorted(pbc.QUERIES))
def test_queries_through_the_parser_on_the_device(eng, builder):
    S = pbc.BUILDERS[builder](bl)
    with psc._quiet():
        P = bl.Parser(*S)
    stamps = list(S[0].formattedTimestamps)
    pick = [len(stamps) - 1, 2, 0, 2, 3]
    for query in pbc.QUERIES[builder]:
        with Launched() as k:
            got = P(query, t='all', silent=True)
        k.both()
        loop = [P(query, t=ts, silent=True) for ts in stamps]
        assert isinstance(got, list) and len(got) == len(loop)
        for (x, p), (xw, pw) in zip(got, loop):
            assert np.array_equal(x, xw)
            close(p, pw)
        if (builder, query) in pbc.REFERENCE_CASES:
            close([p for _, p in got], REFERENCE[pbc.key(builder, query) + '|p'])
            assert np.allclose([x for x, _ in got], REFERENCE[pbc.key(builder, query) + '|x'], rtol=1e-12, atol=1e-12)
        for form in ([stamps[i] for i in pick], np.array([stamps[i] for i in pick])):
            with Launched() as k:
                some = P(query, t=form, silent=True)
            k.both()
            for (x, p), i in zip(some, pick):
                assert np.array_equal(x, got[i][0]) and np.array_equal(p, got[i][1])
        with Launched() as k:
            one = S[0].eval(query, t=[stamps[1]], silent=True)                 # fewer than parser.DIST_MIN_STAMPS = 3 stamps: the loop
            two = P(query, t=[stamps[1], stamps[0]], silent=True)
        assert k.count == {} and np.array_equal(one[0][1], loop[1][1]) and np.array_equal(two[1][1], loop[0][1])
    # ---- option parser_device = 0 keeps distribution queries on the loop
    query = pbc.QUERIES[builder][0]
    eng.set_option('parser_device', 0.0)
    try:
        with Launched() as k:
            got = P(query, t='all', silent=True)
    finally:
        eng.set_option('parser_device', 1.0)
    assert k.count == {}
    for (x, p), ts in zip(got, stamps):
        xw, pw = P(query, t=ts, silent=True)
        assert np.array_equal(x, xw) and np.array_equal(p, pw)
    # ---- the study stays usable
    first = S[0]
    before = P(query, t=stamps[:3], silent=True)
    with psc._quiet():
        first.fit()
        P = bl.Parser(*S)
    for (x, p), (xb, pb) in zip(P(query, t=stamps[:3], silent=True), before):
        assert np.array_equal(x, xb) and np.max(np.abs(p - pb)) <= 1e-12


def test_queries_that_stay_on_the_loop(eng):
    S = pbc.BUILDERS['coal'](bl)
    with psc._quiet():
        P = bl.Parser(*S)
    for _, query, error in pbc.RAISING:
        with Launched() as k:
            with pytest.raises(error), np.errstate(all='ignore'):
                P(query, t='all', silent=True)
        assert k.count == {}, (query, k.count)
    S2 = pbc.BUILDERS['two'](bl)
    with psc._quiet():
        P2 = bl.Parser(*S2)
    with Launched() as k:
        got = P2('rate + rate2', t='all', silent=True)
    assert k.count == {} and len(got) == 5
    for (x, p), ts in zip(got, range(5)):
        xw, pw = P2('rate + rate2', t=ts, silent=True)
        assert np.array_equal(x, xw) and np.array_equal(p, pw)
    with Launched() as k:
        P2('rate2*2', t='all', silent=True)
    k.both()
