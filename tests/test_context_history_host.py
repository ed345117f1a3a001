"""
The table of tests/context_history_cases.py held to the library's source, and the harness of tests/test_context_history.py run without a GPU:
through the float64 oracle (fresh and long-lived instances of tests/oracle_engine.OracleEngine: it must pass), and through LeakyEngine -- a
plain Python class around the oracle that keeps something of its previous call, one way at a time -- which it must catch, naming the
predecessor.  What is covered: tests/CONTEXT_HISTORY.md.
"""
import numpy as np
import pytest

import context_history_cases as ch
import step_transition_cases as sc
from bayesloop_amd.engine import HipEngine
from oracle_engine import OracleEngine

# ---- the table ----------------------------------------------------------------------------------------------------------------------------------

def test_the_table_names_every_family_of_the_two_case_files():
    tables = {sc.CASES[c]['family'] for c, _ in ch.TABLE_CASES}
    assert tables == {c['family'] for c in sc.CASES.values()}
    assert len(tables) == 14
    for need in ('chainax_100x90', 'hwide_40x300', 'vwide_140x64', 'fast_band8_sources_140x90', 'mfma_band8_sources_140x90', 'nd_shift_then_walk_5x18x14',
                 'chain1d_long_sources_4100'):
        assert 'table_' + need in ch.TARGETS, need
    for fam in sorted(tables):          # the family's *_sources_* case, where it has one
        sources = [n for n, c in sc.CASES.items() if c['family'] == fam and 'sources' in n]
        assert not sources or any('table_' + n in ch.TARGETS for n in sources), fam
    import test_likelihood_kernels as tl
    assert set(ch.GAUSS_FAMILIES) - {'chain_clamp'} <= set(tl.FAMILIES)
    # (the recurrence families; the per-cell exponential flavours and the generic kernel keep no state of their own beyond what these share)
    assert {f for f in tl.FAMILIES if tl.FAMILIES[f]['rec'] is not None} - {'chain_in_kernel_anchors', 'generic'} <= set(ch.GAUSS_FAMILIES)
    assert {t.family for t in ch.TARGETS.values()} >= {'likprogram', 'poisson', 'bigshift', 'hyper_fold', 'carried', 'history', 'readers', 'device_table'}
    assert 30 <= len(ch.TARGETS) <= 45
    assert all(t.variants >= 2 for t in ch.TARGETS.values())


def test_every_reusable_buffer_of_the_context_is_used_by_a_target():
    members = ch.devbuf_members()
    assert len(members) == len(set(members)) >= 37 and {'state', 'post', 'xch', 'probebuf', 'postinv'} <= set(members)
    assert set(ch.USES) == set(ch.TARGETS)
    declared = set().union(*ch.USES.values())
    assert declared <= set(members), sorted(declared - set(members))                          # every declared name is a DevBuf of the struct
    assert set(ch.NOT_IN_THE_TABLE) == {'commbuf', 'probebuf'}                                 # the two allowed exceptions
    assert set(members) - declared == set(ch.NOT_IN_THE_TABLE), sorted(set(members) - declared - set(ch.NOT_IN_THE_TABLE))


# ---- same_bits ----------------------------------------------------------------------------------------------------------------------------------------

def test_same_bits_sees_the_sign_of_a_zero_a_nan_payload_a_shape_and_a_dtype():
    a = dict(x=np.array([0.0, 1.0, np.nan]), n=np.array([-1, 2]))
    assert ch.same_bits(a, {k: v.copy() for k, v in a.items()}) == []
    b = {k: v.copy() for k, v in a.items()}
    b['x'][0] = -0.0
    assert a['x'][0] == b['x'][0]
    bad = ch.same_bits(b, a)
    assert len(bad) == 1 and bad[0].startswith('x: 1 of 3 values differ, first at (0,)')
    c = {k: v.copy() for k, v in a.items()}
    c['x'].view(np.uint64)[2] ^= 1                                                             # another NaN
    assert np.isnan(c['x'][2]) and len(ch.same_bits(c, a)) == 1
    assert ch.same_bits(dict(a, x=a['x'][:2]), a) and ch.same_bits(dict(a, x=a['x'].astype(np.float32)), a)
    assert ch.same_bits(dict(x=a['x']), a) and ch.same_bits(dict(n=a['n'], x=a['x']), a)       # other calls, another call order
    assert ch.same_route(dict(census={'k': 2}, fits=[(6, 0, 0, 1)]), dict(census={'k': 2}, fits=[(6, 0, 0, 1)])) == []
    assert ch.same_route(dict(census={'k': 3}, fits=[(6, 0, 0, 1)]), dict(census={'k': 2}, fits=[(6, 0, 0, 1)]))
    assert ch.same_route(dict(census={'k': 2}, fits=[(0, 1, 2, 0)]), dict(census={'k': 2}, fits=[(6, 0, 0, 1)]))


# ---- the harness on the oracle ----------------------------------------------------------------------------------------------------------------------

HOST_TARGETS = ['table_generic_walks_24x20', 'gauss_resident_exact', 'readers_reductions_40x63']


def _fresh_of(make):
    cache = {}

    def fresh(name, variant=0):
        if (name, variant) not in cache:
            cache[(name, variant)] = ch.run_target(make(), name, variant)
        return cache[(name, variant)]
    return fresh


@pytest.fixture(scope='module')
def oracle_fresh():
    return _fresh_of(OracleEngine)


@pytest.mark.parametrize('x', HOST_TARGETS)
def test_the_loop_passes_on_the_oracle(oracle_fresh, x):
    ch.after_every_predecessor(OracleEngine(), oracle_fresh, x, order=HOST_TARGETS)


# ---- the harness must be able to fail ----------------------------------------------------------------------------------------------------------------

class LeakyEngine:
    """the oracle engine with a memory -- plain Python, no library involved --, one leak at a time:
    'beyond_extent'  the posterior buffer only grows and is never cleared: a read of fewer cells than the buffer holds reads one cell past its
                     own extent, so its last value is the previous, larger call's
    'near_data'      the first chain's local_evidence is kept from the last fit of the same shapes when that fit's data were within 1e-9
    'stale_reader'   marginal / time_average answer from the kept fit BEFORE the last one"""

    def __init__(self, leak):
        self.__dict__.update(_e=OracleEngine(), leak=leak, _buf=np.zeros(0), _last={}, _kept=[])

    def __getattr__(self, name):
        return getattr(self._e, name)

    def __setattr__(self, name, value):
        setattr(self._e, name, value)

    def fit(self, problem, op_values, **kw):
        res = self._e.fit(problem, op_values, **kw)
        if self.leak == 'near_data':
            data = np.asarray(problem.data, dtype=float)
            key = (data.shape, res.local_evidence.shape)
            prev = self._last.get(key)
            self._last[key] = (data.copy(), res.local_evidence.copy())
            if prev is not None and np.allclose(prev[0], data, rtol=0.0, atol=1e-9, equal_nan=True):
                res.local_evidence[0] = prev[1][0]
        if self.leak == 'stale_reader' and kw.get('keep_posterior'):
            self.__dict__['_kept'] = (self._kept + [(self._e._post.copy(), list(self._e._gs))])[-2:]
        return res

    def posterior(self, chain, T, grid_size, t0=0, t1=None):
        out = np.array(self._e.posterior(chain, T, grid_size, t0, t1))
        if self.leak == 'beyond_extent':
            flat = out.reshape(-1)
            if flat.size < self._buf.size:
                self._buf[:flat.size] = flat
                flat[-1] = self._buf[flat.size]
            else:
                self.__dict__['_buf'] = flat.copy()
        return out

    def _stale(self, T, shape):
        if self.leak == 'stale_reader' and len(self._kept) == 2 and self._kept[0][1] == list(shape) and self._kept[0][0].size == T * int(np.prod(shape)):
            return self._kept[0][0].reshape([T] + list(shape))
        return None

    def marginal(self, source, chain, keep_axis, T, n_keep):
        post = self._stale(T, self._e._gs)
        if post is None:
            return self._e.marginal(source, chain, keep_axis, T, n_keep)
        return post.sum(axis=tuple(a + 1 for a in range(post.ndim - 1) if a != keep_axis))

    def time_average(self, source, chain, grid_size):
        post = self._stale(len(self._e._post.reshape([-1] + list(grid_size))), grid_size)
        return self._e.time_average(source, chain, grid_size) if post is None else post.mean(axis=0)


# leak -> (X, the predecessors of the loop, what the message must name): each loop fails under the leak it is aimed at and under no other
AIMED = {
    'beyond_extent': ('table_generic_walks_24x20', ['gauss_resident_exact'], ('after gauss_resident_exact[0]', 'posterior')),     # 3 x 1024 cells before 2 x 480
    'near_data': ('table_chainax_sources_32x32', ['table_chainax_sources_32x32'], ('after table_chainax_sources_32x32[1]', 'local_evidence')),
    'stale_reader': ('readers_reductions_40x63', ['readers_reductions_40x63'], ('after readers_reductions_40x63[1]', 'marginal')),
}


@pytest.mark.parametrize('aimed', sorted(AIMED))
@pytest.mark.parametrize('leak', sorted(AIMED))
def test_each_leak_fails_the_loop_aimed_at_it_and_no_other(oracle_fresh, leak, aimed):
    """the table drivers' data are zeros for every input, so X after X on other inputs is the same geometry with data within 1e-9"""
    x, order, names = AIMED[aimed]
    if leak != aimed:
        ch.after_every_predecessor(LeakyEngine(leak), oracle_fresh, x, order=order)
        return
    with pytest.raises(AssertionError) as err:
        ch.after_every_predecessor(LeakyEngine(leak), oracle_fresh, x, order=order)
    msg = str(err.value)
    assert 'other bits than on a fresh context' in msg and all(n in msg for n in names), msg


def test_a_negated_zero_in_a_result_is_caught(oracle_fresh):
    want = oracle_fresh('table_generic_walks_24x20', 1)                                           # `single`: almost all zeros
    got = ({k: v.copy() for k, v in want[0].items()}, want[1])
    key = next(k for k, v in got[0].items() if k.endswith('posterior') and (v == 0.0).any())
    i = np.unravel_index(int(np.argmax(got[0][key] == 0.0)), got[0][key].shape)
    got[0][key][i] = -0.0
    assert np.array_equal(got[0][key], want[0][key])                                               # equal as numbers
    with pytest.raises(AssertionError, match='other bits'):
        ch.compare(got, want, 'negated zero')


# ---- the memory plans: what a context's left-over buffers do to a budget (CONTEXT_HISTORY.md, "The memory plans") ------------------------------

def test_a_budget_short_of_the_left_over_workspace_plans_an_online_block_differently():
    """blhip_mem_budget adds back state, post, accpart and mixseq; a predictive workspace stays counted as used.  With M bytes on the card a
    context plans with 0.9 min(free + added back, 0.7 M): a left-over of L bytes changes the plan only where L > 0.3 M -- pinned with the two
    host-callable plans on a card of 288 GiB."""
    M = 288.0 * 2 ** 30
    grid, chains, planes, N = [512, 512], 64, 4, 400
    fresh = HipEngine.online_block_plan(grid, chains, planes, N, 0.9 * min(M, 0.7 * M))
    small = HipEngine.predictive_plan(512 * 512, 1000, 1000)['workspace_bytes']
    assert small < 0.3 * M
    assert HipEngine.online_block_plan(grid, chains, planes, N, 0.9 * min(M - small, 0.7 * M)) == fresh        # below 0.3 M: the same plan
    left = 0.85 * M                                                                               # e.g. a padded chain-resident sequence: postpad
    after = HipEngine.online_block_plan(grid, chains, planes, N, 0.9 * min(M - left, 0.7 * M))
    assert after is not None and after['steps'] < fresh['steps'] and after['n_chunks'] > fresh['n_chunks'], (fresh, after)
