"""
Every result of the library on the MI355X, held to the bits a context created a moment ago gives -- whatever the context has served before.

A blhip_ctx keeps its device buffers from call to call (DevBuf::ensure grows them and never clears them) and host state beside them; a kernel
that reads a cell its own call did not write shows the previous call's data.  No float atomics exist in the library and its summation orders are
fixed, so the property is exact: every comparison here is on the bits (NaN payloads and the sign of zero included), and on the route -- the
instantiations launched and the resident paths' fields of the timing -- which is compared first and reported with its own message.  There is no
tolerance, no retry and no registry of exceptions in this file.  The calls: tests/context_history_cases.py; what the card showed:
tests/CONTEXT_HISTORY.md.  BLHIP_HISTORY_REPORT=<file> appends, per test, the predecessors and the routes.
"""
import contextlib
import dataclasses
import io
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import context_history_cases as ch
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem, extra_engine
from bayesloop_amd.exceptions import BackendError

pytestmark = pytest.mark.gpu

_FRESH = {}


def _report(what, text):
    path = os.environ.get('BLHIP_HISTORY_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write('%s\t%s\t%s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, text))


def _route_text(route):
    return '%s | %s' % (route['fits'], ', '.join('%s x%d' % kv for kv in sorted(route['census'].items())))


@pytest.fixture(scope='module')
def device():
    e = bl.get_engine()
    assert type(e).__name__ == 'HipEngine'
    return e.device


@pytest.fixture(scope='module')
def fresh(device):
    """fresh(target, variant): the target on a context of its own, created for it and dropped behind it; cached for the module"""
    def get(name, variant=0):
        key = (name, variant)
        if key not in _FRESH:
            e = extra_engine(device)
            try:
                _FRESH[key] = ch.run_target(e, name, variant)
            finally:
                del e
            _report('fresh %s[%d]' % key, _route_text(_FRESH[key][1]))
        return _FRESH[key]
    yield get
    _FRESH.clear()


@pytest.fixture(scope='module')
def dirty(device):
    e = extra_engine(device)
    yield e
    del e


NAMES = list(ch.TARGETS)


@pytest.mark.parametrize('x', NAMES)
def test_after_every_predecessor(dirty, fresh, x):
    """on one long-lived context: every target of the table, then X -- all ordered pairs, X after itself on other data among them"""
    ch.after_every_predecessor(dirty, fresh, x, report=lambda x, p, route: _report('after ' + p, _route_text(route)))


@pytest.mark.parametrize('x', NAMES)
def test_after_a_larger_call_of_the_same_family(dirty, fresh, x):
    """buffers grown beyond X's extent, a kept batch of more chains, steps and cells than X's own"""
    for k, run in enumerate(ch.larger_runs(x)):
        ch.arm(dirty)
        with np.errstate(all='ignore'):
            run(ch.Tap(dirty), 1)
        got = ch.run_target(dirty, x, 0)
        _report('after larger call %d' % k, _route_text(got[1]))
        ch.compare(got, fresh(x, 0), '%s after larger call %d of its family' % (x, k))


# ---- calls that did not end well: product paths that leave state behind without a device fault -----------------------------------------------------

def _table_problem(shape, T=3, dead_step=1):
    G = int(np.prod(shape))
    lik = np.random.default_rng(G).uniform(0.05, 1.0, (T, G))
    lik[dead_step] = 0.0
    return FitProblem(obs_model=_abi.OM_TABLE, marginal=[np.arange(n, dtype=np.float64) for n in shape], lattice=[1.0] * len(shape),
                      data=np.zeros((T, 1)), timestamps=np.arange(T, dtype=np.float64), prior=np.full(G, 1.0 / G),
                      ops=[(_abi.OP_GRW, 0, -1, 0)], lik=lik)


def zero_likelihood(e):
    """every chain's likelihood is zero at step 1: the fits stop there (core.py:390-400) on the resident, chain-resident, 1-D and N-D paths"""
    for shape, B in (((32, 32), 1), ((128, 16), 3), ((100, 20), 3), ((300,), 2), ((5, 18, 14), 2)):
        res = e.fit(_table_problem(shape), np.linspace(1.2, 1.7, B).reshape(B, 1), keep_posterior=True)
        assert np.all(res.abort_step == 1), (shape, res.abort_step)


def refused_by_the_host(e):
    p = _table_problem((128, 16), dead_step=2)
    p.lik[2] = 1.0
    ov = np.array([[1.5]])
    with pytest.raises(BackendError):
        e.fit(dataclasses.replace(p, prior=np.ones(7)), ov)                                       # a prior of another size
    with pytest.raises(BackendError):
        e.fit(dataclasses.replace(p, carry_slot=-1), ov, forward_only=True, carry=True)           # a bad carry slot
    e.accum_begin(3, 5)
    try:
        with pytest.raises(BackendError):
            e.fit(p, ov, accumulate=True, log_chain_weight=np.zeros(1))                           # an accumulator of another shape
    finally:
        e.accum_end()


def forced_give_up(x):
    def run(e):
        e.set_option('resident_force_abort', 1)
        try:
            ch.run_target(e, x, 1)
        finally:
            e.set_option('resident_force_abort', 0)
    return run


def forced_batch_failures(e):
    """tests/test_fold_recovery.py's two-chain flavour: the range check of the last fused batch fails, then its prediction check"""
    import test_fold_recovery as tfr
    prev = bl.set_engine(e)
    try:
        for kind in ('stage2', 'fold'):
            opts, _ = tfr.poison(kind, 2)
            S, folded = tfr.fit(tfr.FLAVOURS['two_chain']['plain'], **opts)
            assert S.lastTiming['resident_fallbacks'] >= 1, S.lastTiming
            del S
    finally:
        bl.set_engine(prev)
        e.release_posterior()
        e.accum_end()


def open_accumulator(e):
    e.accum_begin(6, 128 * 16)
    e.accum_end()


NOT_WELL = ['gauss_resident_exact', 'gauss_chain_padded', 'gauss_chain_fold2', 'gauss_chainax', 'table_chain1d_sources_300', 'table_chain_nd_mixed_5x18x14',
            'hyper_fold_fused_128x16', 'carried_row_201', 'history_block_64x48']


@pytest.mark.parametrize('x', NOT_WELL)
def test_after_a_call_that_did_not_end_well(dirty, fresh, x):
    for what, run in (('a zero likelihood', zero_likelihood), ('a refused fit', refused_by_the_host), ('a forced give-up', forced_give_up(x)),
                      ('forced batch failures', forced_batch_failures), ('an accumulator never finalised', open_accumulator)):
        with np.errstate(all='ignore'):
            run(dirty)
        got = ch.run_target(dirty, x, 0)              # (run_target re-arms the resident paths: resident_ok = 1)
        _report('after ' + what, _route_text(got[1]))
        ch.compare(got, fresh(x, 0), '%s after %s' % (x, what))


# ---- readers after a call that kept nothing --------------------------------------------------------------------------------------------------------------

def test_readers_refuse_what_the_last_call_did_not_keep(dirty):
    """a kept forward-only fit of shape A, then an evidence-only fit of shape B: every reader of source 0 raises BackendError or still returns A's
    values bit for bit -- never B-shaped or mixed data"""
    import predictive_cases as pc
    import test_parser_series as tps
    import test_postfit_kernels as tp
    (n0, n1), T, B = ch.READ_SHAPE, ch.READ_T, ch.READ_B
    A = tp.problem_2d(n0, n1, T, seed=6)
    x = np.linspace(-5.0, 5.5, 18)
    ops, consts, series = tps.exact_programs((n0, n1))['series']
    steps = np.arange(17, dtype=np.int64) * 3 % T
    w = np.random.default_rng(1).uniform(0.0, 1.0, (T, B))

    def mixed():
        dirty.mix_sequence(w, plane=0, n_planes=1, source=0)
        return dirty.mix_read(T, [n0, n1])
    readers = dict(posterior=lambda: dirty.posterior(B - 1, T, [n0, n1]), marginal=lambda: dirty.marginal(0, B - 1, 0, T, n0),
                   time_average=lambda: dirty.time_average(0, B - 1, [n0, n1]),
                   predictive=lambda: dirty.predictive(0, B - 1, A.marginal, _abi.OM_GAUSSIAN, x, 0, T, False),
                   posterior_query=lambda: dirty.posterior_query(0, B - 1, steps, ops, consts, _abi.QR_GE, tps.marginals((n0, n1)), series=series[:17]),
                   mix_sequence=mixed)
    ch.arm(dirty)
    dirty.fit(A, tp.sigmas(B), forward_only=True, keep_posterior=True)
    want = {k: np.array(r()) for k, r in readers.items()}
    res = dirty.fit(tp.problem_2d(48, 80, 7, seed=7), tp.sigmas(3), evidence_only=True)
    assert np.all(res.abort_step < 0)
    bad = []
    for k, r in readers.items():
        try:
            got = np.array(r())
        except BackendError as e:
            _report('reader ' + k, 'refused: %s' % e)
            print('%s: refused (%s)' % (k, e))
            continue
        diff = ch.same_bits({k: got}, {k: want[k]})
        _report('reader ' + k, 'returned A' if not diff else 'NEITHER: ' + diff[0])
        print('%s: %s' % (k, 'returned the kept fit of shape A, bit for bit' if not diff else diff[0]))
        bad += diff
    assert not bad, 'a reader of source 0 neither refused nor returned the kept fit:\n  ' + '\n  '.join(bad)


# ---- public studies, interleaved on one context ----------------------------------------------------------------------------------------------------------

def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        return fn(*a, **kw)


STUDY = ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues')
HYPER = STUDY + ('logEvidenceList', 'hyperParameterDistribution', 'averagePosteriorSequence')


def _flat(prefix, value, out):
    """a public result as plain arrays: lists of arrays (an OnlineStudy's per-model results) one entry per item"""
    if isinstance(value, (list, tuple)) and any(isinstance(v, (list, tuple, np.ndarray)) for v in value):
        for i, v in enumerate(value):
            _flat('%s[%d]' % (prefix, i), v, out)
    elif value is None or isinstance(value, (str, bool)) or (isinstance(value, (list, tuple)) and any(not isinstance(v, (int, float, np.number)) for v in value)):
        out[prefix] = np.array(repr(value))
    else:
        out[prefix] = np.array(value)
    return out


def _results(S, keys, out, name):
    for k in keys:
        v = getattr(S, k, None)
        _flat('%s.%s' % (name, k), np.array(v) if type(v).__name__ == 'DevicePosterior' else v, out)


def _interleaved(steps):
    """the seven steps of the issue, on the engine installed now; steps: which of the studies take part (the solo runs take one each)"""
    import cases
    import test_online_block as tob
    out = {}
    A = cases.build(bl, 'c3_small') if 'A' in steps else None
    B = cases.build(bl, 'c1_coal') if 'B' in steps else None
    H = cases.build(bl, 'c4_2hp') if 'H' in steps else None
    C = cases.build(bl, 'c5_small') if 'C' in steps else None
    O1 = cases.build_online(bl, 'online_poisson_3tm') if 'O1' in steps else None
    O2 = cases.build_online(bl, 'online_gauss2d') if 'O2' in steps else None
    d1, d2 = cases.online_data(cases.ONLINE_CASES['online_poisson_3tm']), cases.online_data(cases.ONLINE_CASES['online_gauss2d'])
    if A: _quiet(A.fit, silent=True)                                                    # 1
    if B: _quiet(B.fit, silent=True)                                                    # 2
    if A: _flat('A.posteriorSequence', np.array(A.posteriorSequence), out)
    if H: _quiet(H.fit, silent=True)                                                    # 3
    if C: _quiet(C.fit, silent=True)
    if H: _flat('H.averagePosteriorSequence', np.array(H.averagePosteriorSequence), out)
    if O1: _quiet(O1.stepMany, np.array(d1[:12]))                                       # 4
    if O2: _quiet(O2.stepMany, np.array(d2[:8]))
    if O1: _quiet(O1.step, d1[12])
    if O2: _flat('O2.parameterPosterior', O2.parameterPosterior, out)
    if O1: _flat('O1.transitionModelPosterior', O1.transitionModelPosterior, out)
    if A:
        _flat('A.simulate', _quiet(A.simulate, np.linspace(-3.0, 3.0, 9), t='all'), out)   # 5
        T = len(A.formattedTimestamps)
        _flat('A.eval', _quiet(A.eval, '(mean - c)/std > 1', t='all', silent=True, series={'c': np.linspace(-0.5, 0.5, T)}), out)   # 6
    if B: _quiet(B.fit, silent=True)                                                    # 7
    for name, S, keys in (('A', A, STUDY), ('B', B, STUDY), ('H', H, HYPER), ('C', C, HYPER)):
        if S is not None:
            _results(S, keys, out, name)
    for name, S in (('O1', O1), ('O2', O2)):
        if S is not None:
            _results(S, [k for k in tob.SNAP if k != 'transitionModels'], out, name)
    return out


def test_public_studies_interleaved(device):
    """five kinds of study on ONE context, in an order that leaves results pending on the device when the next call starts: every public result
    equals, bit for bit, what the same study gives built, run and read alone on a fresh context"""
    def on_a_new_context(steps):
        e = extra_engine(device)
        ch.arm(e)
        prev = bl.set_engine(e)
        try:
            return _interleaved(steps)
        finally:
            bl.set_engine(prev)
            del e
    together = on_a_new_context(('A', 'B', 'H', 'C', 'O1', 'O2'))
    alone = {}
    for s in ('A', 'B', 'H', 'C', 'O1', 'O2'):
        alone.update(on_a_new_context((s,)))
    bad = ch.same_bits({k: together[k] for k in sorted(together)}, {k: alone[k] for k in sorted(alone)})
    assert not bad, 'interleaved studies differ from the studies alone:\n  ' + '\n  '.join(bad[:30])
