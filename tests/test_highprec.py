"""tests/highprec.py against exact rational arithmetic: the reference the post-fit kernels are compared with (tests/test_postfit_kernels.py)
must itself stay well inside the bounds it sets for them -- here: within 1/8 of each bound, on small random inputs with exact zeros, values
below the 1e-300 clamp and log-weights up to 800 e-folds apart.  exp() of the exact difference of two float64 log-weights is taken with the
decimal module at 60 digits (correctly rounded: relative error 1e-60) and turned into a Fraction."""
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

import highprec as hp

F = Fraction
SHARE = 8            # the reference may use 1 / SHARE of a bound


def _exp(x):
    """exp of a Fraction whose value is an exact difference of float64 numbers."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -999999, 999999
        d = decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)     # (a dyadic rational: exact at this precision for our inputs)
        assert F(d) == x
        return F(d.exp())


def _frac(a):
    return [F(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _assert_within(got, want_fracs, bound, what):
    got = np.asarray(got).reshape(-1)
    bound = np.asarray(bound, dtype=np.float64).reshape(-1)
    assert len(got) == len(want_fracs) == len(bound)
    for i, (g, w, b) in enumerate(zip(got, want_fracs, bound)):
        # a longdouble converts to a Fraction exactly through its two float64 halves
        hi = float(g)
        lo = float(g - hp.LD(hi))
        err = abs(F(hi) + F(lo) - w)
        assert err <= F(float(b)) / SHARE, '%s[%d]: reference %r, exact %.20e, error %.3e, bound %.3e' % (what, i, g, float(w), float(err), b)


def _posts(rng, B, T, G):
    p = rng.random((B, T, G))
    p[rng.random((B, T, G)) < 0.15] = 0.0                       # exact zeros
    tiny = rng.random((B, T, G)) < 0.15
    p[tiny] = 10.0 ** rng.uniform(-320, -299, size=int(tiny.sum()))    # below and around the clamp, denormals included
    return p


def _exact_fold(posts, log_w, prev=None, prev_ref=None):
    ok = [h for h in range(len(log_w)) if math.isfinite(log_w[h])]
    ref = max([log_w[h] for h in ok] + ([prev_ref] if prev is not None else []))
    T, G = posts.shape[1:]
    out = [F(0)] * (T * G) if prev is None else [v * _exp(F(prev_ref) - F(ref)) for v in prev]
    for h in ok:
        w = _exp(F(float(log_w[h])) - F(ref))
        ph = _frac(np.maximum(posts[h], hp.CLAMP))
        out = [o + w * v for o, v in zip(out, ph)]
    return out, ref


@pytest.mark.parametrize('spread', [0.0, 30.0, 700.0, 800.0])
@pytest.mark.parametrize('B', [1, 4, 7])
def test_fold_against_exact_arithmetic(B, spread):
    rng = np.random.default_rng(100 + B + int(spread))
    T, G = 2, 5
    posts = _posts(rng, B, T, G)
    log_w = -1234.5 - rng.uniform(0, 1, B) * spread
    if B > 1:
        log_w[0] = -1234.5
        log_w[-1] = -1234.5 - spread
    if B > 2:
        log_w[1] = -math.inf if spread else math.nan           # contributes nothing
    A, ref, n = hp.fold(posts, log_w)
    want, ref_x = _exact_fold(posts, log_w)
    assert ref == ref_x and n == int(np.isfinite(log_w).sum())
    X = hp.fold_span(log_w, ref)
    assert X <= min(spread, 745.2) + 1e-9
    _assert_within(A, want, hp.fold_bound(np.array([float(v) for v in want]), B, 0, X), 'fold')
    # the running form: onto what is there, with the reference moving up, down and staying
    for k, shift in enumerate((50.0, -50.0, 0.0, 800.0, -800.0)):
        lw2 = log_w[np.isfinite(log_w)][:1] + shift - rng.uniform(0, 1, B) * min(spread, 40.0)
        A2, ref2, n2 = hp.fold(posts[::-1], lw2, prev=A, prev_ref=ref)
        hi = np.asarray(A, dtype=np.float64)
        prev_exact = [F(float(a)) + F(float(b)) for a, b in zip(hi.reshape(-1), np.asarray(A - hp.LD(1) * hi, dtype=np.float64).reshape(-1))]
        want2, ref2_x = _exact_fold(posts[::-1], lw2, prev=prev_exact, prev_ref=ref)
        assert ref2 == ref2_x and n2 == B
        X2 = hp.fold_span(lw2, ref2, earlier=[ref])
        _assert_within(A2, want2, hp.fold_bound(np.array([float(v) for v in want2]), B, 1, X2), 'running fold %d' % k)
        if shift == 800.0:         # what was there vanishes against the bound
            only, _ = _exact_fold(posts[::-1], lw2)
            _assert_within(A2, only, hp.fold_bound(np.array([float(v) for v in only]), B, 1, X2), 'fold 800 above')
        if shift == -800.0:        # nothing changes
            assert ref2 == ref
            _assert_within(A2, prev_exact, hp.fold_bound(np.array([float(v) for v in prev_exact]), B, 1, X2), 'fold 800 below')


def test_fold_of_nothing():
    A, ref, n = hp.fold(np.ones((2, 1, 3)), [-math.inf, math.nan])
    assert A is None and ref == -math.inf and n == 0
    A, ref, n = hp.fold(np.ones((2, 1, 3)), [-math.inf, math.nan], prev=np.full((1, 3), 2.0), prev_ref=-3.0)
    assert ref == -3.0 and n == 0 and np.all(A == 2.0)


def test_rescale_against_exact_arithmetic():
    rng = np.random.default_rng(7)
    A = rng.random((2, 6))
    for d in (0.0, 30.0, 700.0):
        got = hp.rescale(A, -100.25, -100.25 + d)
        want = [v * _exp(F(-100.25) - F(-100.25 + d)) for v in _frac(A)]
        _assert_within(got, want, hp.SLACK * (2 + d) * hp.U * np.array([float(v) for v in want]), 'rescale')


@pytest.mark.parametrize('shape', [(1,), (7,), (3, 5), (2, 3, 4), (2, 3, 2, 3)])
def test_finalize_and_row_stats_against_exact_arithmetic(shape):
    rng = np.random.default_rng(11 + len(shape))
    T, G = 3, int(np.prod(shape))
    A = rng.random((T, G)) * 10.0 ** rng.uniform(-30, 3, size=(T, 1))
    A[rng.random((T, G)) < 0.2] = 0.0
    A[:, 0] += 1e-3                                               # (no all-zero row)
    grids = [np.sort(rng.uniform(-3, 2, n)) for n in shape]       # values of both signs
    st, st_abs = hp.row_stats(A, grids)
    norm, rows, means, means_abs = hp.finalize(A, grids)
    Af = [_frac(A[t]) for t in range(T)]
    idx = np.indices(shape).reshape(len(shape), -1)
    for t in range(T):
        s = sum(Af[t])
        _assert_within([st[t, 0], norm[t]], [s, s], hp.row_stats_bound([float(s)] * 2, G), 'norm')
        _assert_within(rows[t], [v / s for v in Af[t]], hp.normalised_bound([float(v / s) for v in Af[t]], G), 'rows')
        for k in range(len(shape)):
            gk = [F(float(grids[k][i])) for i in idx[k]]
            num = sum(a * g for a, g in zip(Af[t], gk))
            num_abs = sum(a * abs(g) for a, g in zip(Af[t], gk))
            _assert_within([st[t, 1 + k]], [num], hp.row_stats_bound([float(num_abs)], G), 'stats')
            _assert_within([st_abs[t, 1 + k]], [num_abs], hp.row_stats_bound([float(num_abs)], G), 'abs stats')
            _assert_within([means[k, t]], [num / s], hp.mean_bound([float(num_abs / s)], G), 'means')
            _assert_within([means_abs[k, t]], [num_abs / s], hp.mean_bound([float(num_abs / s)], G), 'abs means')


@pytest.mark.parametrize('shape', [(6,), (1, 5), (4, 3), (3, 1), (2, 3, 4)])
def test_marginal_and_time_average_against_exact_arithmetic(shape):
    rng = np.random.default_rng(23 + len(shape) + shape[0])
    T = 4
    p = rng.random((T,) + shape) * 10.0 ** rng.uniform(-200, 0, size=(T,) + shape)
    p[rng.random(p.shape) < 0.2] = 0.0
    pf = np.array(_frac(p), dtype=object).reshape(p.shape)
    for k in range(len(shape)):
        axes = tuple(a + 1 for a in range(len(shape)) if a != k)
        want = pf.sum(axis=axes) if axes else pf
        n_red = int(np.prod([shape[a - 1] for a in axes])) if axes else 1
        _assert_within(hp.marginal(p, k), list(want.reshape(-1)), hp.marginal_bound(np.array([float(v) for v in want.reshape(-1)]), n_red), 'marginal')
    want = pf.sum(axis=0) / T
    _assert_within(hp.time_average(p), list(want.reshape(-1)), hp.time_average_bound(np.array([float(v) for v in want.reshape(-1)]), T), 'time average')
    one = hp.time_average(p[:1])
    assert np.array_equal(np.asarray(one, dtype=np.float64), p[0])


@pytest.mark.parametrize('n', [1, 5, 33])
def test_mix_against_exact_arithmetic(n):
    rng = np.random.default_rng(31 + n)
    G = 9
    states = rng.random((n, G))
    states[rng.random((n, G)) < 0.2] = 0.0
    w = rng.random(n)
    w[::3] = 0.0
    sf = [_frac(s) for s in states]
    want = [sum(F(float(w[j])) * sf[j][c] for j in range(n)) for c in range(G)]
    m, mag = hp.mix(states, w)
    _assert_within(m, want, hp.mix_bound(np.array([float(v) for v in want]), n), 'mix')
    _assert_within(mag, want, hp.mix_bound(np.array([float(v) for v in want]), n), 'magnitude')
    prev = rng.random(G)
    m2, mag2 = hp.mix(states, -w, prev=prev)
    want2 = [p - v for p, v in zip(_frac(prev), want)]
    wmag = [p + v for p, v in zip(_frac(prev), want)]
    _assert_within(m2, want2, hp.mix_bound(np.array([float(v) for v in wmag]), n), 'signed mix')
    _assert_within(mag2, wmag, hp.mix_bound(np.array([float(v) for v in wmag]), n), 'signed magnitude')


def test_worst_reports_the_ratio():
    assert hp.worst([1.0, 2.0], [1.0, 2.0], [0.0, 0.0]) == 0.0
    assert hp.worst([1.0, 2.5], [1.0, 2.0], [1.0, 1.0]) == 0.5
    assert hp.worst([1.0], [2.0], [0.0]) == math.inf
    assert hp.worst([math.nan], [2.0], [1.0]) == math.inf
