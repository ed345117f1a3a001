"""
The kernels that run AFTER the forward / backward passes, each against a high-precision reference of the same operation.

What the rest of the suite asserts about the average-posterior folds, the accumulator's rescale / normalisation / means, the marginals, the
time average, the ranged reads and the mixtures of carried states it asserts through whole studies at the parity bar (1e-9); a fold that
drops a chain carrying less than 1e-9 of the evidence passes that.  Here the INPUTS come from the device itself -- the per-chain posteriors
a fit(keep_posterior=True, accumulate=True) leaves, the log-weights the test chose, sequences the caller made -- so the fit is not under
test, and the expected value is tests/highprec.py (longdouble sums, checked against exact rational arithmetic by tests/test_highprec.py).
The bounds are the derived ones of tests/highprec.py: the number of float64 operations behind a value times u = 2 ** -53, times 2.

Which kernel ran is read from the library's registry (blhip_kernel_census) and asserted: a case that silently takes another flavour proves
nothing.  BLHIP_POSTFIT_REPORT=<file> writes, per kernel, the ids of the tests of this file that launched it.

The device limit of gridDim.y is 65 536 on gfx950 (hipDeviceProp_t::maxGridSize[1]); launches that put time steps / rows / chains x steps
there go in pieces (for_grid_y, blhip_host.hpp) -- test_fold_and_finalize_over_more_steps_than_one_launch_holds is the case beyond it.

A caller-owned accumulator (blhip_accum_begin: external_devptr) is device memory of a SECOND library context here, not a torch tensor: the
PyTorch wheel carries its own copy of the HIP runtime, and a pointer of that runtime means nothing to the one libblhip.so is linked against.
"""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import DevicePosterior, FitProblem, extra_engine
import cases
import highprec as hp
from conftest import kernel_census

pytestmark = pytest.mark.gpu

MAX_GRID_Y = 65536               # hipDeviceProp_t::maxGridSize[1] of gfx950, as read on the card
LAUNCHED_BY = {}                 # kernel family -> ids of the tests of this file that launched it


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    try:
        eng.accum_end()
        eng.carry_release(-1)
        eng.release_posterior()
    finally:
        bl.set_engine(prev)
        out = os.environ.get('BLHIP_POSTFIT_REPORT')
        if out:
            with open(out, 'w') as f:
                json.dump({k: sorted(v) for k, v in sorted(LAUNCHED_BY.items())}, f, indent=1)


@pytest.fixture
def eng(hip_engine):
    return hip_engine


def _family(name):
    return re.sub(r'[<(].*', '', name).split('::')[-1].strip()


def _counts():
    out = {}
    for c, name in kernel_census():
        out[_family(name)] = out.get(_family(name), 0) + c
    return out


class Launched:
    """with Launched() as k: ... ; k.names = the kernel families launched inside, k.count[name] = how often."""

    def __enter__(self):
        self.before = _counts()
        self.names, self.count = set(), {}
        return self

    def __exit__(self, *exc):
        after = _counts()
        self.count = {k: after[k] - self.before.get(k, 0) for k in after if after[k] > self.before.get(k, 0)}
        self.names = set(self.count)
        test = os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]
        for k in self.names:
            LAUNCHED_BY.setdefault(k, set()).add(test)

    def require(self, *kernels):
        missing = [k for k in kernels if k not in self.names]
        assert not missing, 'expected kernel(s) not launched: %s; launched: %s' % (missing, sorted(self.names))

    def forbid(self, *kernels):
        hit = [k for k in kernels if k in self.names]
        assert not hit, 'kernel(s) launched that this case must not take: %s; launched: %s' % (hit, sorted(self.names))


FOLD_KERNELS = ('accumulate_kernel', 'accumulate2_kernel', 'accumulate_small_kernel', 'accumulate_pad_kernel', 'fold_parts_kernel')


def only_fold(k, kernel):
    k.require(kernel)
    k.forbid(*[f for f in FOLD_KERNELS if f != kernel])


def within(got, want, bound, what):
    q = hp.worst(got, want, bound)
    print('%s: worst |error| / bound = %.3g' % (what, q))
    assert q <= 1.0, '%s: worst |error| / bound = %.3g at (index, got, want, bound) = %r' % (what, q, hp.worst_at(got, want, bound))


# ---- problems ------------------------------------------------------------------------------------------------------------------------

_COMPILED = {}


def compiled(om, data, target):
    """FitProblem of a plain Study with one random walk on `target`: op_values is then (n_chains, 1), the walk's width per chain."""
    key = repr((om, data if not isinstance(data, np.ndarray) else data.tobytes(), target))
    if key not in _COMPILED:
        S = cases.build(bl, dict(study='Study', data=data, om=om, tm=('GRW', 'sigma', 0.1, target, None)))
        S._checkConsistency()
        S._formatData()
        problem, program = S._compile(silent=True)
        assert len(problem.ops) == 1 and problem.ops[0][0] == _abi.OP_GRW
        _COMPILED[key] = problem
    return _COMPILED[key]


def problem_1d(G, T, seed=5, std=None):
    data = ('gm', seed, T)
    if std is not None:
        data = cases.gm_data(seed, T)
        data[:, 1] = std
    return compiled(('GaussianMean', [('mean', ('cint', -8, 8, G))], 'default'), data, 'mean')


def problem_2d(n0, n1, T, seed=6):
    return compiled(('Gaussian', [('mean', ('cint', -8, 8, n0)), ('std', ('oint', 0, 4, n1))], 'default'), ('series', seed, T), 'mean')


def sigmas(B):
    return (np.linspace(0.15, 0.9, B) if B > 1 else np.array([0.3])).reshape(B, 1)


def plain_problem(grids, T):
    """A problem that only carries a grid (what blhip_accum_finalize / _row_stats read of it); nothing is fitted with it."""
    G = int(np.prod([len(g) for g in grids]))
    return FitProblem(obs_model=_abi.OM_TABLE, marginal=[np.asarray(g, dtype=float) for g in grids], lattice=[1.0] * len(grids),
                      data=np.zeros(T), timestamps=np.arange(T, dtype=float), prior=np.full(G, 1.0 / G), ops=[(_abi.OP_STATIC, 0)])


def signed_grids(shape, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.uniform(-3.0, 2.0, n)) for n in shape]


def sequence(T, G, seed, zeros=0.1):
    """A caller-made sequence: rows normalised, some cells exactly zero."""
    rng = np.random.default_rng(seed)
    p = rng.random((T, G))
    if G > 1:
        p[rng.random((T, G)) < zeros] = 0.0
        p[:, 0] += 0.5
    return p / p.sum(axis=1, keepdims=True)


# ---- the library, below the engine where the engine has no argument for it ---------------------------------------------------------------

def rc_of(eng, fn, *args):
    """(return code, message) of a C-ABI call on the engine's context."""
    rc = getattr(eng.lib, fn)(eng.ctx, *args)
    return rc, (eng.lib.blhip_last_error(eng.ctx) or b'').decode()


def refused(eng, fn, *args):
    rc, msg = rc_of(eng, fn, *args)
    assert rc != 0 and msg.strip(), '%s%r: rc = %d, message %r' % (fn, args[:4], rc, msg)
    return msg


def accum_begin(eng, T, G, devptr=None):
    rc, msg = rc_of(eng, 'blhip_accum_begin', T, G, devptr)
    assert rc == 0, msg
    eng._acc_shape = (int(T), int(G))


def accum_devptr(eng):
    p = C.c_void_p()
    rc, msg = rc_of(eng, 'blhip_accum_state', None, C.byref(p), None)
    assert rc == 0, msg
    return p.value


def fit_kept(eng, problem, ov, target, begin=True, devptr=None):
    """One kept, accumulating fit whose chains get the log-weights `target` (B,) (-inf / nan: as given): a first fit of the same kind
    tells the evidences (fits are bit-reproducible), the second gets log_chain_weight = target - logEvidence.  Returns the chains'
    posteriors (B, T, G) as the device holds them, the float64 log-weights the library formed, and the kernels of the second fit."""
    T, G, B = problem.T, problem.G, len(ov)
    if begin or devptr is not None:
        accum_begin(eng, T, G)
        probe = eng.fit(problem, ov, keep_posterior=True, accumulate=True, log_chain_weight=np.zeros(B))
        _LOGE[(id(problem), ov.tobytes())] = probe.log_evidence.copy()
        accum_begin(eng, T, G, devptr)
    logE = _LOGE[(id(problem), ov.tobytes())]
    assert np.all(np.isfinite(logE))
    lw = np.asarray(target, dtype=float) - logE
    with Launched() as k:
        res = eng.fit(problem, ov, keep_posterior=True, accumulate=True, log_chain_weight=lw)
    assert res.timing['batches'] == 1 and np.all(res.abort_step < 0)
    assert np.array_equal(res.log_evidence, logE), 'the fit is not bit-reproducible'
    posts = np.stack([eng.posterior(b, T, [G]) for b in range(B)])
    return posts, res.log_evidence + lw, k


_LOGE = {}


def check_accumulator(eng, T, G, want, ref, n_folded, bound, what):
    log_ref, n = eng.accum_log_ref()
    assert n == n_folded, '%s: n_folded %d, expected %d' % (what, n, n_folded)
    assert log_ref == ref, '%s: reference exponent %r, expected %r' % (what, log_ref, ref)
    got = eng.accum_read(T, [G])
    within(got, want, bound, what)
    return got


# ---- folds: every chain count around the groups of four, equal weights ------------------------------------------------------------------

FOLD_SHAPES = [('accumulate2_kernel', 200, B) for B in (1, 2, 3, 4, 5, 7, 8)] + \
              [('accumulate_kernel', 201, B) for B in (1, 2, 3, 4, 5, 7, 8)] + \
              [('accumulate_small_kernel', 200, B) for B in (16, 17, 18, 19)] + [('accumulate_small_kernel', 201, 19)]


@pytest.mark.parametrize('kernel,G,B', FOLD_SHAPES, ids=['%s-G%d-B%d' % s for s in FOLD_SHAPES])
def test_fold_with_equal_weights(eng, kernel, G, B):
    """All log-weights equal: every chain is 1 / B of the result, a dropped or doubled one is an error of 1 / B against a bound of
    (B + 3) 2 ** -52."""
    T = 6
    problem = problem_1d(G, T)
    posts, log_w, k = fit_kept(eng, problem, sigmas(B), np.full(B, -3.25))
    only_fold(k, kernel)
    want, ref, n = hp.fold(posts, log_w)
    assert n == B
    check_accumulator(eng, T, G, want, ref, B, hp.fold_bound(want, B, 0, hp.fold_span(log_w, ref)), 'fold')
    eng.accum_end()


@pytest.mark.parametrize('pos', [0, 1, 2, 3])
@pytest.mark.parametrize('kind', ['zero', 'nan'])
@pytest.mark.parametrize('kernel,G,B', [('accumulate2_kernel', 200, 8), ('accumulate_kernel', 201, 8), ('accumulate_small_kernel', 200, 19)])
def test_fold_skips_a_weightless_chain(eng, kernel, G, B, kind, pos):
    """One chain with a zero hyper-prior (log-weight -inf) or a NaN log-weight at each position of a group of four: it contributes
    nothing and is not counted, its neighbours are folded in full."""
    T = 5
    problem = problem_1d(G, T)
    idx = pos + 4 * ((B - 1 - pos) // 4)             # the last chain b with b % 4 == pos
    target = np.full(B, 1.5)
    target[idx] = -math.inf if kind == 'zero' else math.nan
    posts, log_w, k = fit_kept(eng, problem, sigmas(B), target)
    only_fold(k, kernel)
    want, ref, n = hp.fold(posts, log_w)
    assert n == B - 1
    check_accumulator(eng, T, G, want, ref, B - 1, hp.fold_bound(want, B, 0, hp.fold_span(log_w, ref)), 'fold')
    without = hp.fold(np.delete(posts, idx, axis=0), np.delete(log_w, idx))[0]
    assert np.array_equal(np.asarray(want, dtype=float), np.asarray(without, dtype=float))
    eng.accum_end()


@pytest.mark.parametrize('spread', [0.0, 30.0, 700.0, 800.0])
@pytest.mark.parametrize('kernel,G,B', [('accumulate2_kernel', 200, 5), ('accumulate_kernel', 201, 6), ('accumulate_small_kernel', 200, 17)])
def test_fold_with_spread_weights(eng, kernel, G, B, spread):
    """Log-weights spread evenly over `spread` e-folds.  At 800 the last chain's weight exp(-800) is zero in float64 and the chain is
    skipped: the reference (which keeps it, 1e-348 of the result) shows that this is inside the bound; it still counts as folded."""
    T = 5
    problem = problem_1d(G, T)
    target = 2.0 - np.linspace(0.0, spread, B)
    posts, log_w, k = fit_kept(eng, problem, sigmas(B), target)
    only_fold(k, kernel)
    want, ref, n = hp.fold(posts, log_w)
    X = hp.fold_span(log_w, ref)
    assert (X <= 745.2) and (X >= min(spread, 600.0) - 1e-6)
    check_accumulator(eng, T, G, want, ref, B, hp.fold_bound(want, B, 0, X), 'fold')
    eng.accum_end()


@pytest.mark.parametrize('kernel,G,B', [('accumulate2_kernel', 200, 5), ('accumulate_kernel', 201, 5), ('accumulate_small_kernel', 200, 17)])
def test_fold_clamps_at_1e_300(eng, kernel, G, B):
    """A narrow likelihood far from most of the grid: the posteriors hold exact zeros and values below 1e-300, which the fold replaces by
    1e-300 (the reference adds log(max(p, 1e-300)) in log space, core.py:1364)."""
    T = 5
    problem = problem_1d(G, T, std=0.2)
    posts, log_w, k = fit_kept(eng, problem, sigmas(B) * 0.3, np.linspace(0.0, -3.0, B))
    only_fold(k, kernel)
    assert (posts == 0.0).any() and ((posts > 0.0) & (posts < hp.CLAMP)).any(), 'the inputs do not reach the clamp'
    want, ref, n = hp.fold(posts, log_w)
    got = check_accumulator(eng, T, G, want, ref, B, hp.fold_bound(want, B, 0, hp.fold_span(log_w, ref)), 'fold')
    wsum = np.exp(log_w - ref).sum()
    allz = (posts < hp.CLAMP).all(axis=0)
    assert allz.any() and np.allclose(got[allz], wsum * hp.CLAMP, rtol=1e-12, atol=0)
    eng.accum_end()


# ---- the running accumulator --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shifts', [(50.0, 800.0), (-50.0, -800.0), (0.0, 0.0)], ids=['above', 'below', 'equal'])
@pytest.mark.parametrize('kernel,G,B', [('accumulate2_kernel', 200, 5), ('accumulate_kernel', 201, 5), ('accumulate_small_kernel', 200, 17)])
def test_running_accumulator(eng, kernel, G, B, shifts):
    """fit, blhip_accum_fold_host of a caller-made sequence, fit, fit into ONE open accumulator; the later fits' log-weights lie 50 and
    800 above / below / at the first one's.  800 above: what was there vanishes; 800 below: nothing changes, n_folded still counts."""
    T = 5
    problem = problem_1d(G, T)
    ov = sigmas(B)
    base = -12.5
    posts, lw1, k = fit_kept(eng, problem, ov, base - np.linspace(0.0, 2.0, B))
    only_fold(k, kernel)
    A, ref, n = hp.fold(posts, lw1)
    spans, folded, earlier = hp.fold_span(lw1, ref), B, 0
    check_accumulator(eng, T, G, A, ref, folded, hp.fold_bound(A, B, earlier, spans), 'first fit')

    host = sequence(T, G, 77)
    with Launched() as kh:
        eng.accum_fold_host(host, base + 0.75)
    only_fold(kh, 'accumulate2_kernel' if G % 2 == 0 else 'accumulate_kernel')
    old = ref
    A, ref, n = hp.fold(host[None], [base + 0.75], prev=A, prev_ref=ref)
    spans, folded, earlier = spans + hp.fold_span([base + 0.75], ref, earlier=[old]), folded + 1, earlier + 1
    check_accumulator(eng, T, G, A, ref, folded, hp.fold_bound(A, 1, earlier, spans), 'host sequence')

    for shift in shifts:
        before = eng.accum_read(T, [G])
        posts, lw, k = fit_kept(eng, problem, ov, base + shift - np.linspace(0.0, 2.0, B), begin=False)
        only_fold(k, kernel)
        old = ref
        A, ref, n = hp.fold(posts, lw, prev=A, prev_ref=ref)
        spans, folded, earlier = spans + hp.fold_span(lw, ref, earlier=[old]), folded + B, earlier + 1
        got = check_accumulator(eng, T, G, A, ref, folded, hp.fold_bound(A, B, earlier, spans), 'fit at %+g' % shift)
        if shift == 800.0:
            alone = hp.fold(posts, lw)[0]
            within(got, alone, hp.fold_bound(alone, B, earlier, spans), 'what was there has vanished')
        if shift == -800.0:
            assert np.array_equal(got, before)
    eng.accum_end()


def test_rescale(eng):
    """blhip_accum_rescale before anything is folded (zeros), to +0, +30 and +700 with more folds after each, and below the current
    reference (refused, accumulator untouched)."""
    G, T, B = 200, 5, 5
    problem = problem_1d(G, T)
    ov = sigmas(B)
    accum_begin(eng, T, G)
    probe = eng.fit(problem, ov, keep_posterior=True, accumulate=True, log_chain_weight=np.zeros(B))
    _LOGE[(id(problem), ov.tobytes())] = probe.log_evidence.copy()
    accum_begin(eng, T, G)
    assert np.all(eng.accum_row_stats(problem) == 0.0)
    with Launched() as k:
        eng.accum_rescale(-40.0)
    k.require('fill_kernel')
    assert eng.accum_log_ref() == (-40.0, 0)
    assert np.all(eng.accum_read(T, [G]) == 0.0) and np.all(eng.accum_row_stats(problem) == 0.0)

    posts, lw, k = fit_kept(eng, problem, ov, -3.0 - np.linspace(0.0, 2.0, B), begin=False)
    only_fold(k, 'accumulate2_kernel')
    A, ref, n = hp.fold(posts, lw, prev=np.zeros((T, G)), prev_ref=-40.0)
    spans, folded, earlier = hp.fold_span(lw, ref), B, 1
    got = check_accumulator(eng, T, G, A, ref, folded, hp.fold_bound(A, B, earlier, spans), 'fold after the empty rescale')

    with Launched() as k:
        eng.accum_rescale(ref)                                  # + 0: nothing to do
    k.forbid('scale_all_kernel')
    assert np.array_equal(eng.accum_read(T, [G]), got) and eng.accum_log_ref() == (ref, folded)

    for shift, how in ((30.0, 'fit'), (700.0, 'host')):
        with Launched() as k:
            eng.accum_rescale(ref + shift)
        k.require('scale_all_kernel')
        A, ref = hp.rescale(A, ref, ref + shift), ref + shift
        spans, earlier = spans + shift, earlier + 1
        # (absolute part: the clamp terms of the chains folded so far, which the factor exp(-shift) takes below the normal range)
        check_accumulator(eng, T, G, A, ref, folded, hp.fold_bound(A, folded, earlier, spans), 'rescale by %g' % shift)
        old = ref
        if how == 'fit':
            posts, lw, k = fit_kept(eng, problem, ov, ref - 4.0 - np.linspace(0.0, 2.0, B), begin=False)
            only_fold(k, 'accumulate2_kernel')
            nb = B
        else:
            posts, lw, nb = sequence(T, G, 78)[None], np.array([ref + 1.25]), 1
            eng.accum_fold_host(posts[0], lw[0])
        A, ref, n = hp.fold(posts, lw, prev=A, prev_ref=ref)
        spans, folded, earlier = spans + hp.fold_span(lw, ref, earlier=[old]), folded + nb, earlier + 1
        got = check_accumulator(eng, T, G, A, ref, folded, hp.fold_bound(A, folded, earlier, spans), 'fold after the rescale by %g' % shift)

    msg = refused(eng, 'blhip_accum_rescale', ref - 1.0)
    assert 'below' in msg
    assert np.array_equal(eng.accum_read(T, [G]), got) and eng.accum_log_ref() == (ref, folded)
    eng.accum_rescale(ref + 1.0)                                 # the next valid call works
    assert eng.accum_log_ref() == (ref + 1.0, folded)
    eng.accum_end()


# ---- a caller-owned accumulator -----------------------------------------------------------------------------------------------------------

def test_caller_owned_accumulator(eng):
    """external_devptr 16-byte aligned and offset by one double, G even: launch_fold must take the two-cell kernel for the first and the
    scalar kernel for the second, and both give the library-owned accumulator bit for bit; the groups-of-chains kernel (no 16-byte
    accesses) takes either."""
    other = extra_engine(eng.device)
    try:
        for G, B, aligned_kernel, offset_kernel in ((200, 5, 'accumulate2_kernel', 'accumulate_kernel'),
                                                    (200, 17, 'accumulate_small_kernel', 'accumulate_small_kernel')):
            T = 5
            problem = problem_1d(G, T)
            target = 1.0 - np.linspace(0.0, 3.0, B)
            accum_begin(other, T, G + 2)
            base = accum_devptr(other)
            assert base % 16 == 0
            posts, lw, k = fit_kept(eng, problem, sigmas(B), target)
            only_fold(k, aligned_kernel)
            own = eng.accum_read(T, [G])
            want, ref, n = hp.fold(posts, lw)
            for off, kernel in ((0, aligned_kernel), (8, offset_kernel)):
                posts2, lw2, k = fit_kept(eng, problem, sigmas(B), target, devptr=base + off)
                only_fold(k, kernel)
                assert accum_devptr(eng) == base + off
                assert np.array_equal(posts2, posts) and np.array_equal(lw2, lw)
                got = check_accumulator(eng, T, G, want, ref, B, hp.fold_bound(want, B, 0, hp.fold_span(lw, ref)), 'offset %d' % off)
                assert np.array_equal(got, own), 'offset %d: not the library-owned result' % off
                host = sequence(T, G, 79)
                eng.accum_fold_host(host, 2.0)               # (and the B = 1 fold of a caller's sequence)
                A2, ref2, _ = hp.fold(host[None], [2.0], prev=want, prev_ref=ref)
                acc = check_accumulator(eng, T, G, A2, ref2, B + 1,
                                        hp.fold_bound(A2, 1, 1, hp.fold_span(lw, ref) + hp.fold_span([2.0], ref2, [ref])), 'host fold')
                means = eng.accum_finalize(problem)              # (row_stats_kernel / scale_rows_kernel on the same pointer)
                norm, rows, m, m_abs = hp.finalize(acc, [problem.marginal[0]])
                within(means, m, hp.mean_bound(m_abs, G), 'means')
                within(eng.accum_read(T, [G]), rows, hp.normalised_bound(rows, G), 'normalised rows')
                eng.accum_end()
            other.accum_end()
    finally:
        other.accum_end()
        del other


def test_fused_fold_and_an_unaligned_accumulator(eng):
    """The fold fused into the backward chain kernel lands in the accumulator through fold_parts_kernel, whose two-cell branch reads and
    writes the accumulator as double2.  Into a caller-owned, 16-byte aligned accumulator: the same numbers bit for bit as into the
    library's own.  Offset by one double: the host does not fuse at all (the chain kernels store, the scalar accumulate_kernel folds), and
    fold_parts_kernel would take its one-cell branch if it were ever handed such a pointer; the result is another summation order of the
    same B terms, within twice the fold's bound of the fused one."""
    n0, n1, T, B = 128, 16, 7, 9
    problem = problem_2d(n0, n1, T)
    G = n0 * n1
    ov = sigmas(B)
    lw = -np.linspace(0.0, 4.0, B)
    other = extra_engine(eng.device)
    try:
        accum_begin(other, T, G + 2)
        base = accum_devptr(other)
        results = []
        for devptr, kernel in ((None, 'fold_parts_kernel'), (base, 'fold_parts_kernel'), (base + 8, 'accumulate_kernel')):
            accum_begin(eng, T, G, devptr)
            with Launched() as k:
                res = eng.fit(problem, ov, accumulate=True, log_chain_weight=lw)
            only_fold(k, kernel)
            ref, n = eng.accum_log_ref()
            assert n == B and ref == (res.log_evidence + lw).max()
            results.append(eng.accum_read(T, [G]))
            eng.accum_end()
        assert np.all(results[0] > 0.0)
        assert np.array_equal(results[1], results[0])
        X = hp.fold_span(res.log_evidence + lw, ref)
        within(results[2], results[0], 2.0 * hp.fold_bound(results[0], B, 0, X), 'separate fold against the fused one')
    finally:
        other.accum_end()
        del other


# ---- strip-major and padded sources -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n0,n1,opts', [(128, 16, dict(fuse_accumulate=0)), (128, 16, dict(fold2=0)), (100, 16, dict(fuse_accumulate=0)),
                                        (100, 16, dict(chain_depad=0)), (100, 20, dict(fold2=0, chain_depad=0))],
                         ids=['exact-nofuse', 'exact-nofold2', 'padded-nofuse', 'padded-nodepad', 'padded-nofold2-nodepad'])
def test_fold_of_chain_resident_sequences(eng, n0, n1, opts):
    """2-D grids on the chain-resident kernels, posteriors kept.  A fit that KEEPS its posteriors hands the fold a row-major sequence: the
    strip-major source of accumulate2_kernel (sm_n0 > 0) and accumulate_pad_kernel read sequences that are private to a fit which keeps
    nothing, so there is nothing to read back and compare them with; those two flavours stay with
    test_fused_fold_matches_the_separate_fold and test_padded_grids_through_the_storing_backward_kernel (whole studies against the
    oracle).  What is asserted here: whichever separate fold a kept fit of these geometries takes under these options, it is one of the
    row-major flavours, and it meets the bound."""
    T, B = 6, 9
    problem = problem_2d(n0, n1, T)
    G = n0 * n1
    defaults = dict(fuse_accumulate=1, fold2=1, chain_depad=1)
    for key, v in opts.items():
        eng.set_option(key, v)
    try:
        posts, log_w, k = fit_kept(eng, problem, sigmas(B), -np.linspace(0.0, 6.0, B))
    finally:
        for key in opts:
            eng.set_option(key, defaults[key])
    k.require('accumulate2_kernel')
    k.forbid('accumulate_pad_kernel', 'fold_parts_kernel')
    want, ref, n = hp.fold(posts, log_w)
    check_accumulator(eng, T, G, want, ref, B, hp.fold_bound(want, B, 0, hp.fold_span(log_w, ref)), 'fold')
    eng.accum_end()


# ---- normalisation, means, per-step sums --------------------------------------------------------------------------------------------------

FINALIZE_SHAPES = [(1,), (255,), (257,), (256 * 256 + 300,), (3, 5), (300, 301), (4, 5, 6), (3, 4, 2, 5), (40, 41, 42), (9, 8, 7, 150)]


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('shape', FINALIZE_SHAPES, ids=['x'.join(map(str, s)) for s in FINALIZE_SHAPES])
def test_finalize_row_stats_and_means(eng, shape, T):
    """1- to 4-parameter grids, G of 1, 255, 257 and above 256 x 256 (row_stats_kernel's grid-stride loop), grid values of both signs.
    The accumulator is a caller-made sequence folded with weight 1 -- it must arrive bit for bit -- under a reference exponent that the
    normalisation must not see."""
    G = int(np.prod(shape))
    grids = signed_grids(shape, 300 + G % 97)
    problem = plain_problem(grids, T)
    seq = sequence(T, G, 400 + G % 89) * 3.0
    seq[0, -1] = 1e-310                                          # (below the clamp)
    accum_begin(eng, T, G)
    with Launched() as k:
        eng.accum_fold_host(seq, -77.5)
    only_fold(k, 'accumulate2_kernel' if G % 2 == 0 else 'accumulate_kernel')
    A = eng.accum_read(T, [G])
    assert np.array_equal(A, np.maximum(seq, hp.CLAMP)) and eng.accum_log_ref() == (-77.5, 1)
    with Launched() as k:
        st = eng.accum_row_stats(problem)
    k.require('row_stats_kernel', 'reduce_partials_kernel')
    want, want_abs = hp.row_stats(A, grids)
    within(st, want, hp.row_stats_bound(want_abs, G), 'row stats')
    with Launched() as k:
        means = eng.accum_finalize(problem)
    k.require('row_stats_kernel', 'reduce_partials_kernel', 'scale_rows_kernel')
    norm, rows, m, m_abs = hp.finalize(A, grids)
    within(means, m, hp.mean_bound(m_abs, G), 'means')
    within(eng.accum_read(T, [G]), rows, hp.normalised_bound(rows, G), 'normalised rows')
    eng.accum_end()


# ---- marginals, time average ---------------------------------------------------------------------------------------------------------------

def check_reductions(eng, source, chain, seq, n0, n1, one_d):
    T = seq.shape[0]
    p = seq.reshape(T, n0, n1)
    with Launched() as k:
        if one_d:
            got = eng.marginal(source, chain, 0, T, n1)
            assert np.array_equal(got, seq.reshape(T, n1))
            refused(eng, 'blhip_posterior_marginal', source, chain, 1, _abi.dptr(np.empty(T * n1)))
        else:
            m0 = eng.marginal(source, chain, 0, T, n0)
            m1 = eng.marginal(source, chain, 1, T, n1)
            within(m0, hp.marginal(p, 0), hp.marginal_bound(hp.marginal(p, 0), n1), 'marginal of parameter 0')
            within(m1, hp.marginal(p, 1), hp.marginal_bound(hp.marginal(p, 1), n0), 'marginal of parameter 1')
        ta = eng.time_average(source, chain, [n0 * n1])
    if not one_d:
        k.require('marginal_rows_kernel', 'marginal_cols_kernel')
    k.require('time_average_kernel')
    want = hp.time_average(seq)
    within(ta, want, hp.time_average_bound(want, T), 'time average')


REDUCTION_SHAPES = [(n0, n1) for n0 in (1, 2, 1024) for n1 in (1, 63, 255, 256, 257, 1000)] + [(4096 + 8, 257)]


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('n0,n1', REDUCTION_SHAPES, ids=['%dx%d' % s for s in REDUCTION_SHAPES])
def test_reductions_of_the_average_posterior(eng, n0, n1, T):
    """source = 1: marginals of both parameters and the time average of the finalised accumulator, for n1 around the block size, n0 of 1
    (a 1-D study: the copy path), 2 and 1024, and one grid above 4096 x 256 cells (time_average_kernel's grid-stride loop)."""
    one_d = n0 == 1
    G = n0 * n1
    grids = signed_grids((n1,) if one_d else (n0, n1), 500 + n1)
    problem = plain_problem(grids, T)
    accum_begin(eng, T, G)
    eng.accum_fold_host(sequence(T, G, 600 + n0 + n1), 3.0)
    out = np.empty(T * max(n0, n1))
    assert 'not finalised' in refused(eng, 'blhip_posterior_marginal', 1, 0, 0, _abi.dptr(out))
    assert 'not finalised' in refused(eng, 'blhip_posterior_time_average', 1, 0, _abi.dptr(np.empty(G)))
    eng.accum_finalize(problem)
    seq = eng.accum_read(T, [G])
    check_reductions(eng, 1, 0, seq, n0, n1, one_d)
    refused(eng, 'blhip_posterior_marginal', 1, 0, 2, _abi.dptr(out))
    refused(eng, 'blhip_posterior_marginal', 1, 0, -1, _abi.dptr(out))
    refused(eng, 'blhip_posterior_marginal', 2, 0, 0, _abi.dptr(out))
    refused(eng, 'blhip_posterior_time_average', -1, 0, _abi.dptr(np.empty(G)))
    assert np.array_equal(eng.marginal(1, 0, 0, T, n1 if one_d else n0).shape, (T, n1 if one_d else n0))      # the next valid call works
    eng.accum_end()


@pytest.mark.parametrize('n0,n1', [(1, 200), (128, 16), (100, 20), (40, 63)], ids=['1x200', '128x16', '100x20', '40x63'])
def test_reductions_of_kept_posteriors(eng, n0, n1):
    """source = 0: the first, a middle and the last chain of a kept batch; chains out of range are refused."""
    T, B = 4, 5
    one_d = n0 == 1
    problem = problem_1d(n1, T) if one_d else problem_2d(n0, n1, T)
    G = n0 * n1
    eng.fit(problem, sigmas(B), keep_posterior=True)
    for chain in (0, 2, B - 1):
        seq = eng.posterior(chain, T, [G])
        assert np.allclose(seq.sum(axis=1), 1.0, rtol=1e-12)
        check_reductions(eng, 0, chain, seq, n0, n1, one_d)
    out = np.empty(T * max(n0, n1))
    for chain in (-1, B, B + 100):
        assert 'chain' in refused(eng, 'blhip_posterior_marginal', 0, chain, 0, _abi.dptr(out))
        refused(eng, 'blhip_posterior_time_average', 0, chain, _abi.dptr(np.empty(G)))
        refused(eng, 'blhip_posterior_read', chain, 0, T, _abi.dptr(np.empty(T * G)))
    assert np.array_equal(eng.posterior(B - 1, T, [G]), seq)                    # the next valid call works
    rc, msg = rc_of(eng, 'blhip_posterior_release')
    assert rc == 0, msg
    assert 'no posterior kept' in refused(eng, 'blhip_posterior_marginal', 0, 0, 0, _abi.dptr(out))
    assert 'no posterior kept' in refused(eng, 'blhip_posterior_time_average', 0, 0, _abi.dptr(np.empty(G)))
    assert 'no posterior kept' in refused(eng, 'blhip_posterior_read', 0, 0, T, _abi.dptr(np.empty(T * G)))
    eng.fit(problem, sigmas(B), keep_posterior=True)
    assert np.array_equal(eng.posterior(B - 1, T, [G]), seq)


def test_reductions_before_any_fit():
    """A fresh context: nothing kept, no accumulator -- every reduction and read is refused with a message, and the context works after."""
    e = extra_engine(bl.get_engine().device)
    out = np.empty(64)
    for args in (('blhip_posterior_marginal', 0, 0, 0, _abi.dptr(out)), ('blhip_posterior_marginal', 1, 0, 0, _abi.dptr(out)),
                 ('blhip_posterior_time_average', 0, 0, _abi.dptr(out)), ('blhip_posterior_time_average', 1, 0, _abi.dptr(out)),
                 ('blhip_posterior_read', 0, 0, 1, _abi.dptr(out)), ('blhip_accum_read', 0, 1, _abi.dptr(out)),
                 ('blhip_accum_rescale', 0.0), ('blhip_accum_fold_host', _abi.dptr(out), 0.0), ('blhip_accum_state', None, None, None),
                 ('blhip_carry_read', 0, 0, _abi.dptr(out)), ('blhip_carry_read', 0, -1, _abi.dptr(out)),
                 ('blhip_carry_mix', 0, 1, _abi.dptr(out), 0), ('blhip_accum_begin', 0, 5, None), ('blhip_accum_begin', 5, 0, None)):
        refused(e, *args)
    accum_begin(e, 2, 8)
    p8, keep8 = e._problem(plain_problem([np.arange(8.0)], 2))
    p9, keep9 = e._problem(plain_problem([np.arange(9.0)], 2))
    refused(e, 'blhip_accum_finalize', C.byref(p8), None)                                                   # nothing accumulated
    seq = sequence(2, 8, 1)
    e.accum_fold_host(seq, 0.0)
    e.accum_fold_host(seq, math.nan)                             # contributes nothing, is no error
    e.accum_fold_host(seq, -math.inf)
    assert e.accum_log_ref() == (0.0, 1) and np.array_equal(e.accum_read(2, [8]), np.maximum(seq, hp.CLAMP))
    assert 'mismatch' in refused(e, 'blhip_accum_finalize', C.byref(p9), None)                              # another grid
    assert 'mismatch' in refused(e, 'blhip_accum_row_stats', C.byref(p9), _abi.dptr(np.empty(4)))
    e.accum_finalize(plain_problem([np.arange(8.0)], 2))
    assert 'finalised' in refused(e, 'blhip_accum_fold_host', _abi.dptr(seq), 0.0)
    assert np.allclose(e.accum_read(2, [8]).sum(axis=1), 1.0, rtol=1e-14)
    e.accum_end()
    del e


# ---- ranged reads -----------------------------------------------------------------------------------------------------------------------------

def test_ranged_reads(eng):
    """blhip_posterior_read and blhip_accum_read over EVERY [t0, t1) of a T = 5 sequence, t0 == t1 included: bit for bit the slices of the
    full read; t0 > t1, t1 > T, t0 < 0 are refused."""
    T, B, G = 5, 3, 201
    problem = problem_1d(G, T)
    posts, log_w, k = fit_kept(eng, problem, sigmas(B), np.zeros(B))
    acc = eng.accum_read(T, [G])
    for t0 in range(T + 1):
        for t1 in range(t0, T + 1):
            for chain in range(B):
                got = eng.posterior(chain, T, [G], t0=t0, t1=t1)
                assert got.shape == (t1 - t0, G) and np.array_equal(got, posts[chain, t0:t1])
            got = eng.accum_read(T, [G], t0=t0, t1=t1)
            assert got.shape == (t1 - t0, G) and np.array_equal(got, acc[t0:t1])
    out = np.empty(T * G + 8)
    for t0, t1 in ((3, 2), (0, T + 1), (-1, 2), (T + 1, T + 1)):
        assert 'range' in refused(eng, 'blhip_posterior_read', 0, t0, t1, _abi.dptr(out))
        assert 'range' in refused(eng, 'blhip_accum_read', t0, t1, _abi.dptr(out))
    refused(eng, 'blhip_posterior_read', 0, 0, T, None)
    refused(eng, 'blhip_accum_read', 0, T, None)
    assert np.array_equal(eng.posterior(1, T, [G]), posts[1]) and np.array_equal(eng.accum_read(T, [G]), acc)
    eng.accum_finalize(problem)
    fin = eng.accum_read(T, [G])
    dp = DevicePosterior(eng, 1, T, [G])
    for t in range(T):
        assert np.array_equal(dp.row(t), fin[t])
    dq = DevicePosterior(eng, 0, T, [G], chain=2)
    for t in range(T):
        assert np.array_equal(dq.row(t), posts[2, t])
    eng.accum_end()


def test_chunked_host_marginal_of_a_three_parameter_grid(eng):
    """DevicePosterior.marginal of a grid with more than two parameters reduces on the host, 2 ** 26 // G time steps per read: a sequence
    of one step more than a chunk (2 ** 26 + G doubles, 0.5 GiB), the steps on both sides of the seam against the reference."""
    shape = (64, 64, 64)
    G = int(np.prod(shape))
    step = 2 ** 26 // G
    T = step + 1
    rng = np.random.default_rng(9)
    seq = rng.random((T, G))
    problem = plain_problem(signed_grids(shape, 10), T)
    accum_begin(eng, T, G)
    eng.accum_fold_host(seq, 0.0)
    del seq
    eng.accum_finalize(problem)
    dp = DevicePosterior(eng, 1, T, list(shape))
    rows = (0, 1, step - 1, step)
    p = np.stack([dp.row(t) for t in rows])
    assert np.allclose(p.reshape(len(rows), -1).sum(axis=1), 1.0, rtol=1e-12)
    for kk in range(3):
        got = dp.marginal(kk)
        assert got.shape == (T, shape[kk])
        want = hp.marginal(p, kk)
        within(got[list(rows)], want, hp.marginal_bound(want, G // shape[kk]), 'marginal of parameter %d' % kk)
        assert np.allclose(got.sum(axis=1), 1.0, rtol=1e-12)
    eng.accum_end()


# ---- carried states --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G,n', [(1, 1), (1, 33), (255, 1), (255, 33), (257, 1), (257, 33), (8192 * 256 + 257, 3)],
                         ids=lambda v: str(v))
def test_carried_states_and_their_mixtures(eng, G, n):
    """carry_write of (n_chains, G) rows, carry_read of each chain bit-exact; carry_mix with accumulate 0, then 1, then 1 (weights with
    zeros and one negative) against the reference started from what the device held; G above 8192 x 256: carry_mix_kernel's grid-stride
    loop."""
    slot = 7
    rng = np.random.default_rng(G % 1000 + n)
    states = rng.random((n, G))
    states /= states.sum(axis=1, keepdims=True)
    eng.carry_release(-1)
    eng.carry_write(slot, states)
    for chain in sorted({0, n // 2, n - 1}):
        assert np.array_equal(eng.carry_read(slot, chain, [G]), states[chain])
    assert 'no mix' in refused(eng, 'blhip_carry_read', slot, -1, _abi.dptr(np.empty(G)))
    prev = None
    for it, accumulate in enumerate((0, 1, 1)):
        w = rng.random(n)
        w[::3] = 0.0 if n > 1 else w[0]
        if it == 2 and n > 1:
            w[1] = -0.25 * w[1]
        with Launched() as k:
            eng.carry_mix(slot, w, accumulate=bool(accumulate))
        k.require('carry_mix_kernel')
        got = eng.carry_read(slot, -1, [G])
        want, mag = hp.mix(states, w, prev=prev if accumulate else None)
        within(got, want, hp.mix_bound(mag, n), 'mix %d' % it)
        prev = got
    # error returns: wrong number of weights, a mix of another size, chains out of range, a released slot
    w = np.ones(n + 1)
    assert 'chains' in refused(eng, 'blhip_carry_mix', slot, n + 1, _abi.dptr(w), 0)
    refused(eng, 'blhip_carry_mix', slot, n, None, 0)
    refused(eng, 'blhip_carry_mix', slot + 1, n, _abi.dptr(w), 0)
    refused(eng, 'blhip_carry_read', slot, n, _abi.dptr(np.empty(G)))
    eng.carry_write(slot + 1, np.full((2, G + 1), 1.0 / (G + 1)))
    assert 'accumulating' in refused(eng, 'blhip_carry_mix', slot + 1, 2, _abi.dptr(w), 1)
    assert np.array_equal(eng.carry_read(slot, -1, [G]), prev)                   # untouched, and the next valid call works
    eng.carry_mix(slot + 1, np.array([0.5, 0.5]), accumulate=False)
    assert np.allclose(eng.carry_read(slot, -1, [G + 1]), 1.0 / (G + 1), rtol=1e-15)
    refused(eng, 'blhip_carry_write', slot, 0, G, _abi.dptr(states))
    refused(eng, 'blhip_carry_write', -1, n, G, _abi.dptr(states))
    refused(eng, 'blhip_carry_write', slot, n, G, None)
    eng.carry_release(slot)
    assert 'holds no state' in refused(eng, 'blhip_carry_read', slot, 0, _abi.dptr(np.empty(G)))
    assert 'holds no state' in refused(eng, 'blhip_carry_mix', slot, n, _abi.dptr(w), 0)
    assert np.array_equal(eng.carry_read(slot + 1, 1, [G + 1]), np.full(G + 1, 1.0 / (G + 1)))
    eng.carry_release(-1)
    refused(eng, 'blhip_carry_read', slot + 1, 0, _abi.dptr(np.empty(G + 1)))
    refused(eng, 'blhip_carry_read', slot, -1, _abi.dptr(np.empty(G + 1)))


def test_carried_states_of_a_fit(eng):
    """carry_store_kernel: the states a forward-only fit with carry=True leaves are its last filtered distributions, normalised -- the last
    row of the kept posterior of the same forward-only fit, bit for bit --, and their mixture meets the bound."""
    G, T, B = 201, 4, 5
    problem = problem_1d(G, T)
    problem.carry_slot = 3
    try:
        with Launched() as k:
            eng.fit(problem, sigmas(B), forward_only=True, keep_posterior=True, carry=True)
        k.require('carry_store_kernel')
    finally:
        problem.carry_slot = 0
    states = np.stack([eng.carry_read(3, b, [G]) for b in range(B)])
    last = np.stack([eng.posterior(b, T, [G], t0=T - 1, t1=T)[0] for b in range(B)])
    # (both are the raw last row times a rounded reciprocal of its rounded sum: 2 u each side)
    assert np.all(states > 0.0) and np.all(np.abs(states - last) <= hp.SLACK * 4 * hp.U * last)
    assert np.all(np.abs(states.sum(axis=1) - 1.0) <= hp.SLACK * (G + 2) * hp.U)
    w = np.array([0.5, 0.0, 0.25, 0.125, 0.125])
    eng.carry_mix(3, w)
    want, mag = hp.mix(states, w)
    within(eng.carry_read(3, -1, [G]), want, hp.mix_bound(mag, B), 'mix')
    eng.carry_release(-1)


# ---- more steps than one launch holds ------------------------------------------------------------------------------------------------------

def test_fold_and_finalize_over_more_steps_than_one_launch_holds(eng):
    """gridDim.y of the fold kernels, scale_rows_kernel, row_stats_kernel and the marginal kernels is a number of time steps, and the
    device takes 65 536 of them per launch: a 1-D hyper-study of 65 537 steps has to be folded, normalised and reduced in two launches
    each; the last step is the one a single launch could not reach.  (launch_fold takes accumulate_small_kernel only while
    blocks x steps < 1024: a series this long goes through accumulate2_kernel, or accumulate_kernel when G is odd.)  The marginal kernels
    get a caller-made sequence on a 2 x 4 grid."""
    T, B = MAX_GRID_Y + 1, 17
    rng = np.random.default_rng(3)
    data = np.stack([np.cumsum(rng.normal(0.0, 0.02, T)), np.ones(T)], 1)
    for G, kernel in ((8, 'accumulate2_kernel'), (9, 'accumulate_kernel')):
        problem = compiled(('GaussianMean', [('mean', ('cint', -8, 8, G))], 'default'), data, 'mean')
        ov = sigmas(B) * 4.0
        accum_begin(eng, T, G)
        with Launched() as k:
            res = eng.fit(problem, ov, keep_posterior=True, accumulate=True, log_chain_weight=np.zeros(B))
        only_fold(k, kernel)
        assert k.count[kernel] == 2 and k.count['scale_rows_kernel'] == 2 * B
        assert res.timing['batches'] == 1 and np.all(res.abort_step < 0) and np.all(np.isfinite(res.log_evidence))
        posts = np.stack([eng.posterior(b, T, [G]) for b in range(B)])
        assert np.all(np.abs(posts[:, -1].sum(axis=1) - 1.0) <= hp.SLACK * (G + 2) * hp.U), 'the last step was not normalised'
        log_w = res.log_evidence + 0.0
        want, ref, n = hp.fold(posts, log_w)
        X = hp.fold_span(log_w, ref)
        check_accumulator(eng, T, G, want, ref, B, hp.fold_bound(want, B, 0, X), 'fold')
        del posts
        host = sequence(T, G, 5)
        with Launched() as k:
            eng.accum_fold_host(host, ref - 1.0)
        only_fold(k, kernel)
        assert k.count[kernel] == 2
        A, ref2, _ = hp.fold(host[None], [ref - 1.0], prev=want, prev_ref=ref)
        acc = check_accumulator(eng, T, G, A, ref2, B + 1, hp.fold_bound(A, 1, 1, X + 1.0), 'host sequence')
        grids = [problem.marginal[0]]
        with Launched() as k:
            st = eng.accum_row_stats(problem)
            means = eng.accum_finalize(problem)
        assert k.count['row_stats_kernel'] == 4 and k.count['scale_rows_kernel'] == 2
        s, s_abs = hp.row_stats(acc, grids)
        within(st, s, hp.row_stats_bound(s_abs, G), 'row stats')
        norm, rows, m, m_abs = hp.finalize(acc, grids)
        within(means, m, hp.mean_bound(m_abs, G), 'means')
        fin = eng.accum_read(T, [G])
        within(fin, rows, hp.normalised_bound(rows, G), 'normalised rows')
        assert np.array_equal(eng.marginal(1, 0, 0, T, G), fin)
        within(eng.time_average(1, 0, [G]), hp.time_average(fin), hp.time_average_bound(hp.time_average(fin), T), 'time average')
        assert np.array_equal(eng.accum_read(T, [G], t0=T - 1, t1=T)[0], fin[-1])
        eng.accum_end()
        eng.lib.blhip_posterior_release(eng.ctx)
    n0, n1 = 2, 4
    problem = plain_problem(signed_grids((n0, n1), 12), T)
    accum_begin(eng, T, n0 * n1)
    eng.accum_fold_host(sequence(T, n0 * n1, 6), 0.0)
    eng.accum_finalize(problem)
    fin = eng.accum_read(T, [n0 * n1])
    with Launched() as k:
        m0 = eng.marginal(1, 0, 0, T, n0)
        m1 = eng.marginal(1, 0, 1, T, n1)
    assert k.count['marginal_rows_kernel'] == 2 and k.count['marginal_cols_kernel'] == 2
    p = fin.reshape(T, n0, n1)
    within(m0, hp.marginal(p, 0), hp.marginal_bound(hp.marginal(p, 0), n1), 'marginal of parameter 0')
    within(m1, hp.marginal(p, 1), hp.marginal_bound(hp.marginal(p, 1), n0), 'marginal of parameter 1')
    eng.accum_end()
