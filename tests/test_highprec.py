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


# ---- the Deterministic shift and the stages around it (tests/test_transition_kernels.py holds the large-shift and stage kernels to these) --

needs_extended = pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)


def _exact_shift(line, d):
    """scipy.ndimage.shift(line, d, order = 3, mode = 'nearest') in rational arithmetic, SciPy's recursion with its float64 literal pole;
    the sampled coordinate is the float64 quantity fl(fl(i - d) + 12)."""
    n = len(line)
    N = n + 24
    z = F(hp.SPLINE_POLE)
    gain = (1 - z) * (1 - 1 / z)
    c = [F(float(line[min(max(q - 12, 0), n - 1)])) * gain for q in range(N)]
    zN = z ** N
    first = c[0]
    acc = c[0] + zN * c[N - 1]
    zi = z
    for i in range(1, N):
        acc = acc + zi * (c[i] + zN * (c[N - 1 - i] if i < N - 1 else acc))      # (ni_splines.c accumulates into c[0] in place)
        zi *= z
    c[0] = acc * (z / (1 - zN * zN)) + first
    for i in range(1, N):
        c[i] = c[i] + z * c[i - 1]
    c[N - 1] = c[N - 1] * (z / (z - 1))
    for i in range(N - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    out = []
    for i in range(n):
        pp = (float(i) - float(d)) + 12.0
        fl = math.floor(pp)
        o = F(0)
        for dk in (-1, 0, 1, 2):
            a = abs(F(pp) - (fl + dk))
            w = F(2, 3) - a * a + a * a * a / 2 if a < 1 else ((2 - a) ** 3 / 6 if a < 2 else F(0))
            o += w * c[min(max(fl + dk, 0), N - 1)]
        out.append(o)
    return out


def _small_lines(kind, n, rng):
    if kind == 'cube':
        return rng.random(n) ** 3 + 1e-3
    if kind == 'decades':
        return np.exp(-600.0 * rng.random(n))
    x = np.zeros(n)
    if kind == 'single':
        x[rng.integers(0, n)] = 1.25
    else:
        x[0], x[n - 1] = 0.75, 1.5
    return x


@needs_extended
@pytest.mark.parametrize('kind', ['cube', 'decades', 'single', 'edges'])
@pytest.mark.parametrize('n', [13, 16])
def test_spline_shift_against_exact_arithmetic(n, kind):
    """shifts inside, at and beyond the line, integer ones among them, next to 12 and beyond the device's index clamp; N = n + 24 <= 40"""
    rng = np.random.default_rng(500 + n)
    x = np.stack([_small_lines(kind, n, rng) for _ in range(2)], axis=1)            # (n, 2): two lines along axis 0
    for d in (0.0, 3.25, -7.0, 12.0, float(np.nextafter(12.0, 13.0)), 12.0000001, 13.0, -13.0, n - 0.5, float(n), n + 30.7, -(n + 5.0), 1e6, -3e9):
        got = hp.spline_shift(x, d, 0)
        bound = hp.spline_shift_bound(x, d, 0)
        for l in range(2):
            want = _exact_shift(x[:, l], d)
            _assert_within(got[:, l], want, bound[:, l], 'spline_shift(%s, n = %d, d = %r)[line %d]' % (kind, n, d, l))
        # the other axis is the same operation on the transposed array
        assert np.array_equal(hp.spline_shift(np.ascontiguousarray(x.T), d, 1), got.T)


@needs_extended
def test_stages_against_exact_arithmetic():
    """the renormalisation, RegimeSwitch, NotEqual and the reflect-boundary walk on a small grid, and that a stage carries an incoming
    bound on"""
    rng = np.random.default_rng(77)
    v = rng.random((4, 5)) ** 3
    v[1, 2] = 0.0
    vf = _frac(v)
    s = sum(vf)
    zero = np.zeros(v.shape)
    r, er, D, eD = hp.normalise_stage(v, None, nblk=2)
    _assert_within(r, [a / s for a in vf], hp.SLACK * er, 'normalise')
    _assert_within([D], [s], hp.SLACK * np.array([eD]), 'sum')
    lim = 10.0 ** -1.5
    cl = [max(a / s, F(lim)) for a in vf]
    rr, err = hp.regime_switch_stage(r, er, lim)
    _assert_within(rr, [a / sum(cl) for a in cl], hp.SLACK * err, 'regime switch')
    mx = max(vf)
    ne = [(mx - a) / (len(vf) * mx - s) for a in vf]
    ne = [max(a, F(lim)) for a in ne]
    rn, ern = hp.not_equal_stage(v, None, lim)
    _assert_within(rn, [a / sum(ne) for a in ne], hp.SLACK * ern, 'not equal')
    w = np.array([0.05, 0.25, 0.4, 0.25, 0.05])
    for axis in (0, 1):
        n = v.shape[axis]
        vm = np.moveaxis(np.array(vf, dtype=object).reshape(v.shape), axis, 0)
        want = np.zeros(vm.shape, dtype=object)
        for i in range(n):
            for j in range(5):
                k = i + j - 2
                k = -k - 1 if k < 0 else (2 * n - 1 - k if k >= n else k)
                want[i] = want[i] + F(float(w[j])) * vm[k]
        got, eg = hp.walk_stage(v, None, w, axis)
        _assert_within(got, list(np.moveaxis(want, 0, axis).reshape(-1)), hp.SLACK * eg, 'walk')
        # an incoming bound goes through the stage's magnitudes: here the weights, which sum to one
        _, eg2 = hp.walk_stage(v, zero + 1e-20, w, axis)
        assert np.all(eg2 >= eg + hp.LD(0.99e-20)) and np.all(eg2 <= eg + hp.LD(1.01e-20))
    _, e1 = hp.shift_stage(v, None, 2.5, 0)
    _, e2 = hp.shift_stage(v, zero + 1e-20, 2.5, 0)
    assert np.all(e2 > e1 + hp.LD(0.9e-20))


def _table():
    """(shape, axis, input kind, shifts): every combination tests/test_transition_kernels.py runs"""
    import transition_cases as tc
    for shape, axes in tc.GEOMETRIES:
        for ax in axes:
            for kind in tc.INPUTS:
                yield shape, ax, kind, tc.CONTROL_SHIFTS + tc.shifts(shape[ax])
    for n in tc.SWEEP_N:
        for ax in (0, 1):
            yield tc.sweep_shape(n, ax), ax, ('cube', 'single')[n % 2], tc.SWEEP_SHIFTS(n)


@needs_extended
def test_float64_recursion_stays_within_the_bound_on_the_gpu_table():
    """oracle.bl_oracle.spline_shift_nearest -- SciPy's sequential recursion in float64 -- lies within spline_shift_bound on every input,
    shift and line length of the GPU file: what the reference alone passes.  The renormalising sum is well conditioned (|D| beyond 8 times its
    own bound) on all of them but the class transition_cases.well_conditioned describes.  If inputs are ever picked that the bound cannot carry, this fails here, not on the card."""
    import transition_cases as tc
    from oracle import bl_oracle as bo
    worst = (0.0, None)
    count = 0
    left_out = []
    for shape, ax, kind, ds in _table():
        x = tc.state(kind, shape, ax)
        nblk = tc.nblk_of(shape)
        for d in ds:
            want, e = hp.shift_stage(x, None, d, ax)
            got = bo.spline_shift_nearest(x, d, ax)
            q = hp.worst(got, want, hp.SLACK * e)
            count += 1
            if q > worst[0]:
                worst = (q, (shape, ax, kind, d))
            assert q <= 1.0, (shape, ax, kind, d, q, hp.worst_at(got, want, hp.SLACK * e))
            _, _, D, eD = hp.normalise_stage(want, e, nblk)
            if not tc.well_conditioned(D, eD, hp.SLACK):
                left_out.append((shape, ax, kind, d))
    # what the GPU file leaves out: an integer shift that moves every occupied cell of a sparse input off the grid (the interpolated zeros)
    assert all(kind in ('single', 'edges') and float(d).is_integer() for _, _, kind, d in left_out), left_out
    assert len(left_out) * 10 < count, (len(left_out), count)
    print('left out as ill-conditioned: %d of %d: %s' % (len(left_out), count, sorted({(k, d) for _, _, k, d in left_out})[:12]))
    print('float64 recursion / bound: worst %.3f at %s over %d combinations' % (worst + (count,)))


@needs_extended
def test_scipy_shift_at_the_registered_floor_only():
    """scipy.ndimage.shift itself is compared at the registered FFT_FLOOR (tests/tolerances.py: 1e-15 of a normalised distribution
    absolute, 1e-9 relative), NOT at the local bound: its compiled sampling has absolute errors of ~1e-17 of the line's maximum whatever
    the cell holds, so on inputs with a wide range (decades, single, edges) it misses the local bound by many orders of magnitude --
    seen on the CPU, and the reason the kernels are not compared with SciPy here."""
    import transition_cases as tc
    from scipy import ndimage
    from tolerances import FFT_TOL
    missed = 0
    for shape, ax in (((43, 20), 0), ((43, 20), 1), ((1000, 5), 0), ((3, 4097), 1)):
        for kind in tc.INPUTS:
            x = tc.state(kind, shape, ax)
            for d in tc.CONTROL_SHIFTS + tc.shifts(shape[ax]):
                want = hp.spline_shift(x, d, ax)
                got = ndimage.shift(x, [d, 0.0] if ax == 0 else [0.0, d], order=3, mode='nearest')
                err = np.abs(hp.LD(1) * got - want)
                assert np.all(err <= FFT_TOL['post_atol'] + FFT_TOL['post_rtol'] * np.abs(want)), (shape, ax, kind, d, float(err.max()))
                missed += hp.worst(got, want, hp.spline_shift_bound(x, d, ax)) > 1.0
    assert missed > 0          # (if SciPy ever met the local bound everywhere, the docstring above would be out of date)
