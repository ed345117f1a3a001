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


# ---- the Gaussian likelihood and the small forward-backward pass (tests/test_likelihood_kernels.py) ---------------------------------------

def _dec(x):
    return decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)


def _exact_likelihood(mu, s, record):
    """prod_k exp(-(x_k - mu)^2 / (2 s^2) - 0.5 ln(2 pi s^2)) per cell as (Fraction A = sum_k (x_k - mu)^2 / (2 s^2), Fraction L): the
    polynomial part exactly, ln / exp / pi with the decimal module at 60 digits"""
    out = []
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -999999, 999999
        pi = decimal.Decimal('3.14159265358979323846264338327950288419716939937510582097494')
        for m in mu:
            for sd in s:
                A, arg = F(0), decimal.Decimal(0)
                for x in record:
                    if x == x:
                        a = (F(float(x)) - F(float(m))) ** 2 / (2 * F(float(sd)) ** 2)
                        A += a
                        arg += -_dec(a) - (2 * pi * _dec(F(float(sd)) ** 2)).ln() / 2
                out.append((A, F(arg.exp())))
    return out


LIK_GRID = (np.array([-8.0, -0.1, 0.3, 2.0 / 3.0, 8.0]), np.array([4.0, 0.7, 0.032, 1.6e-4]))
LIK_RECORDS = [[0.3], [0.25, float('nan')], [-8.0, 8.0], [0.3, 0.3001, float('nan'), 0.2999], [float('nan')] * 3, [-24.0], [0.66, 0.67, 0.68, 0.69]]


@pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)
@pytest.mark.parametrize('k', range(len(LIK_RECORDS)))
def test_gaussian_likelihood_against_exact_arithmetic(k):
    """the polynomial part of the argument against rational arithmetic (a few longdouble roundings), the likelihood against 60-digit exp / ln:
    inside 1 / 8 of the bound it sets for the per-cell exponential -- and of the recurrence's bound, which is never the smaller one here"""
    mu, s = LIK_GRID
    rec = LIK_RECORDS[k]
    exact = _exact_likelihood(mu, s, rec)
    terms, _, _ = hp.gaussian_terms(mu, s, rec)
    A = sum((a for a, _ in terms), np.zeros((len(mu), len(s)), dtype=hp.LD)).reshape(-1)
    eps = float(np.finfo(hp.LD).eps)
    for i, (a, (Ax, _)) in enumerate(zip(A, exact)):
        hi = float(a)
        got = F(hi) + F(float(a - hp.LD(hi)))
        assert abs(got - Ax) <= 4 * (len(rec) + 1) * F(eps) * Ax, (i, a, float(Ax))
    L = hp.gaussian_likelihood(mu, s, rec)
    if all(x != x for x in rec):
        assert np.all(L == 1)
        return
    _assert_within(L, [l for _, l in exact], hp.likelihood_bound_exp(mu, s, rec), 'likelihood')
    assert np.all(hp.likelihood_bound_rec(mu, s, rec, 1, 0) >= 0)
    # GaussianMean (:705-706): the same expression with the datum's own s
    if len(rec) == 1:
        for j, sd in enumerate(s):
            assert np.array_equal(hp.gaussian_mean_likelihood(mu, rec[0], sd), L[:, j])
    assert np.all(hp.gaussian_mean_likelihood(mu, float('nan'), 1.0) == 1) and np.all(hp.gaussian_mean_likelihood(mu, 1.0, float('nan')) == 1)


def test_exp_mn_polynomial_and_reduction_counts():
    """the constants behind C_EXPMN: the degree-13 Taylor polynomial's truncation on |r| <= ln 2 / 2 and the exactness of kn * ln2_hi"""
    r = F(math.log(2.0)) / 2
    trunc = r ** 14 / math.factorial(14) * F(3, 2)                # the remainder of the series, bounded by its first term times 1 / (1 - r / 15) < 3 / 2
    assert trunc < F(hp.U) / 10
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    m, e = math.frexp(ln2_hi)
    # ln2_hi is a multiple of 2^-33 below 1: kn ln2_hi is one too, and so is the argument wherever |kn| >= 2^21 (its ulp is coarser): their
    # difference, below 1 / 2, has at most 33 bits -- the first fma is exact there and rounds once (u |r|) elsewhere
    assert int(m * 2 ** 53) % 2 ** 21 == 0 and e == 0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ln2 = F(decimal.Decimal(2).ln())
    split = abs(F(ln2_hi) + F(ln2_lo) - ln2) * F(2.02e9)           # what the split constant is off by, times the largest |kn|
    assert split < F(hp.U) * F(4, 10)
    # Horner's thirteen fmas, each damped by |r| <= 0.35; the two reduction fmas; truncation; the split
    assert hp.C_EXPMN >= 1 / (1 - 0.35) + 0.35 + 0.35 + 0.1 + 0.4


@pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)
def test_small_forward_backward_against_exact_arithmetic():
    """hp.gaussian_fit on a 3 x 2 grid, T = 2, a Static model: core.py:372-470 in rational arithmetic from the same float64 likelihoods"""
    rng = np.random.default_rng(5)
    shape, T = (3, 2), 2
    prior = rng.random(shape)
    liks = [rng.random(shape) * 10.0 ** rng.integers(-3, 3, shape) for _ in range(T)]
    grids, lattice = [np.array([-1.0, 0.5, 2.0]), np.array([0.1, 0.7])], [1.5, 1.0]
    out = hp.gaussian_fit(prior, [(L, np.zeros(shape)) for L in liks], [], grids, lattice, nblk=1, full=True)
    dV = F(1.5)
    P = _frac(prior)
    Ls = [_frac(L) for L in liks]
    alpha, norms, v = [], [], P
    for t in range(T):
        a = [x * l for x, l in zip(v, Ls[t])]
        N = sum(a)
        v = [x / N for x in a]
        alpha.append(v)
        norms.append(N)
    G = len(P)
    beta = [F(1, G)] * G
    for t in range(T - 1, -1, -1):
        p = [x * y for x, y in zip(alpha[t], beta)]
        sp = sum(p)
        p = [x / sp for x in p]
        _assert_within(out['post'][t][0], p, hp.SLACK * out['post'][t][1], 'post[%d]' % t)
        local = 1 / (sum(x / l for x, l in zip(p, Ls[t])) * dV)
        _assert_within([out['local'][t][0]], [local], [hp.SLACK * out['local'][t][1]], 'local[%d]' % t)
        g0 = [F(float(grids[0][i])) for i in range(3) for _ in range(2)]
        _assert_within([out['means'][t][0][0]], [sum(x * g for x, g in zip(p, g0))], [hp.SLACK * out['means'][t][1][0]], 'mean[%d]' % t)
        b = [x * l for x, l in zip(beta, Ls[t])]
        sb = sum(b)
        beta = [x / sb for x in b]
    for t in range(T):
        _assert_within(out['alpha'][t][0], alpha[t], hp.SLACK * out['alpha'][t][1], 'alpha[%d]' % t)
        _assert_within([out['local_fwd'][t][0]], [norms[t] * dV], [hp.SLACK * out['local_fwd'][t][1]], 'local_fwd[%d]' % t)


ORACLE_WORST = {}


def _oracle_families():
    import test_likelihood_kernels as tl
    return list(tl.FAMILIES)


@pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)
@pytest.mark.parametrize('fam', _oracle_families())
def test_float64_oracle_is_inside_the_bounds_of_the_gpu_file(fam):
    """oracle/bl_oracle.py (NumPy float64, the reference's own order of operations) on EVERY problem of tests/test_likelihood_kernels.py,
    held to the bound that file holds the kernels to: the bound is not tuned to the code under test.  Prints the worst error / bound."""
    import likelihood_cases as lc
    import test_likelihood_kernels as tl
    from oracle import bl_oracle as bo
    Fm = tl.FAMILIES[fam]
    top, bad = 0.0, []

    def within(got, want, bound, what):
        nonlocal top
        got = np.asarray(got, dtype=np.float64)
        want, bound = np.broadcast_to(np.asarray(want), got.shape), np.broadcast_to(np.asarray(bound), got.shape)
        nan = np.isnan(np.asarray(want, dtype=np.float64))
        if not np.array_equal(np.isnan(got), nan):
            bad.append('%s: NaN pattern differs' % what)
            return
        if nan.all():
            return
        q = hp.worst(got[~nan], want[~nan], hp.SLACK * bound[~nan])
        top = max(top, q)
        if not q <= 1.0:
            bad.append('%s: error / bound %.3g' % (what, q))

    problems = [(c, (k,), False) for c in lc.CASES for k in range(3)] + [(c, tuple(range(T)), True) for c in lc.BACKWARD_CASES for T in (2, 3)]
    for case, steps, full in problems:
        T = len(steps)
        problem, values, refs, liks, rec_ok = tl.setup(fam, case, steps, full, None if T == 1 else 1e150)
        g = bo.Grid(problem.marginal)
        ops = [('grw', op[1]) if op[0] == tl._abi.OP_GRW else (('regimeswitch',) if op[0] == tl._abi.OP_REGIMESWITCH else ('static',)) for op in problem.ops]
        for c, ref in enumerate(refs):
            with np.errstate(all='ignore'):
                r = bo.fit(g, 'gaussian', problem.data, problem.timestamps, problem.prior, ops, list(values[c]), forward_only=not full)
            what = '%s %s chain %d' % (case, steps, c)
            stop = tl.aborted_at(ref)
            if stop is not None:
                if r['abort'] != ('forward', stop):
                    bad.append('%s: abort %r, expected forward %d' % (what, r['abort'], stop))
                continue
            assert r['abort'] is None, what
            within([r['logEvidence']], [ref['log_evidence'][0]], [ref['log_evidence'][1]], what + ' logE')
            for t in range(T):
                want = ref['post'][t] if full else ref['alpha'][t]
                within(r['posteriorSequence'][t], want[0], want[1], what + ' posterior[%d]' % t)
                loc = ref['local'][t] if full else ref['local_fwd'][t]
                within([r['localEvidence'][t]], [loc[0]], [loc[1]], what + ' localEvidence[%d]' % t)
                within(np.asarray(r['posteriorMeanValues'])[:, t], ref['means'][t][0], ref['means'][t][1], what + ' means[%d]' % t)
    ORACLE_WORST[fam] = top
    print('float64 oracle, %s: worst error / bound %.3f over %d problems' % (fam, top, len(problems)))
    assert not bad, '\n'.join(bad[:20])


@pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)
def test_float64_oracle_is_inside_the_bounds_of_the_gaussian_mean_problems():
    """the same for the 1-D GaussianMean problems of tests/test_likelihood_kernels.py"""
    import test_likelihood_kernels as tl
    from oracle import bl_oracle as bo
    top, bad = 0.0, []
    problems = [(c, (k,), False) for c in tl.GM_CASES for k in range(3)] + \
               [(c, tuple(range(T)), full) for c in tl.GM_BACKWARD for T in (2, 3) for full in (False, True)]
    for case, steps, full in problems:
        problem, values, ref, liks = tl.gm_setup(case, steps, full)
        g = bo.Grid(problem.marginal)
        with np.errstate(all='ignore'):
            r = bo.fit(g, 'gaussian_mean', problem.data, problem.timestamps, problem.prior, [('grw', 0)], [values[0, 0]], forward_only=not full)
        stop = tl.aborted_at(ref)
        if stop is not None:
            assert r['abort'] == ('forward', stop), (case, steps, r['abort'])
            continue
        for t in range(len(steps)):
            want = ref['post'][t] if full else ref['alpha'][t]
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            for got, w, b, what in ((r['posteriorSequence'][t], want[0][:, 0], want[1][:, 0], 'posterior'), ([r['localEvidence'][t]], [loc[0]], [loc[1]], 'localEvidence'),
                                    (np.asarray(r['posteriorMeanValues'])[:1, t], ref['means'][t][0][:1], ref['means'][t][1][:1], 'mean')):
                if np.isnan(np.asarray(w, dtype=np.float64)).all():
                    assert np.isnan(got).all()
                    continue
                q = hp.worst(got, w, hp.SLACK * np.asarray(b))
                top = max(top, q)
                if not q <= 1.0:
                    bad.append('%s %s %s[%d]: error / bound %.3g' % (case, steps, what, t, q))
    print('float64 oracle, GaussianMean: worst error / bound %.3f over %d problems' % (top, len(problems)))
    assert not bad, '\n'.join(bad)


# ---- the host's tap tables and the transition stages of the fused step kernels (tests/test_step_transitions.py) --------------------------------

def _D(x):
    return decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)


def _dctx():
    ctx = decimal.getcontext().copy()
    ctx.prec = 80
    ctx.Emin, ctx.Emax = -999999, 999999
    return decimal.localcontext(ctx)


def _exp80(x):
    with _dctx():
        return F(_D(x).exp())


def _pi80():
    with _dctx():                                          # Machin: pi = 16 atan(1 / 5) - 4 atan(1 / 239)
        def atan_inv(q):
            t = s = decimal.Decimal(1) / q
            k = 1
            while abs(t) > decimal.Decimal(10) ** -85:
                t = -t / (q * q)
                k += 2
                s += t / k
            return s
        return 16 * atan_inv(decimal.Decimal(5)) - 4 * atan_inv(decimal.Decimal(239))


def _cos80(x):
    with _dctx():
        t = s = decimal.Decimal(1)
        k = 0
        while abs(t) > decimal.Decimal(10) ** -85:
            k += 2
            t = -t * x * x / ((k - 1) * k)
            s += t
        return s


def test_walk_and_bivariate_taps_against_exact_arithmetic():
    ns = 0.75
    r, w, e = hp.gaussian_walk_taps(ns)
    assert r == 3 and len(w) == 7
    phi = [_exp80(-F(1, 2) / (F(ns) * F(ns)) * k * k) for k in range(-r, r + 1)]
    _assert_within(w, [p / sum(phi) for p in phi], hp.SLACK * e, 'walk taps')
    assert hp.gaussian_walk_taps(0.1)[0] == 0 and hp.gaussian_walk_taps((40 - 0.25) / 4.0)[0] == 40
    s1, s2, rho = 0.8, 0.6, 0.5
    k, ek = hp.bivariate_taps(s1, s2, rho)
    assert k.shape == (7, 7)
    q = [(F(x * x) / (F(s1) * F(s1)) - 2 * F(rho) * x * y / (F(s1) * F(s2)) + F(y * y) / (F(s2) * F(s2))) / (2 * (1 - F(rho) * F(rho)))
         for x in range(-3, 4) for y in range(-3, 4)]
    v = [_exp80(-a) for a in q]
    _assert_within(k, [a / sum(v) for a in v], hp.SLACK * ek, 'bivariate taps')
    assert hp.bivariate_taps(1.3, 0.7, 0.0)[0].shape == (13, 7)


def test_alphastable_taps_against_the_exact_cosine_sum():
    c, alpha, n = 1.3, 1.5, 4
    k, e = hp.alphastable_taps(c, alpha, n)
    m, K = 7, 12
    with _dctx():
        pi = _pi80()
        X = [(-((_D(F(c)) * pi * q / (m - 1)) ** _D(F(alpha)))).exp() if q else decimal.Decimal(1) for q in range(m)]
        want = []
        for j in range(n):
            acc = X[0] + (-1) ** j * X[m - 1]
            for q in range(1, m - 1):
                acc += 2 * X[q] * _cos80(2 * pi * ((j * q) % K) / K)
            want.append(F(acc / K))
    _assert_within(k, want, hp.SLACK * e, 'alpha-stable taps')


def _exact_eta(u):
    z = F(hp.SPLINE_POLE)
    g = (1 - z) * (1 - 1 / z) * (-z) / (1 - z * z)          # SciPy's gain, and the response of its causal and anti-causal recursion
    n0 = math.floor(u)
    out = F(0)
    for n in range(n0 - 1, n0 + 3):
        a = abs(u - n)
        b = F(2, 3) - a * a + a * a * a / 2 if a < 1 else ((2 - a) ** 3 / 6 if a < 2 else F(0))
        out += g * z ** abs(n) * b
    return out


@needs_extended
@pytest.mark.parametrize('d', [0.5, -3.25, 11.999, 12.0])
def test_small_shift_taps_and_the_truncation_term_against_exact_arithmetic(d):
    """the cardinal-spline weights in rational arithmetic; the untruncated stencil over SciPy's extension IS SciPy's recursion (to |z|^(2 N - 2)); the
    stencil cut at ceil|d| + 34 differs from it by no more than tail(d) max |line|, and not by much less on a single-cell line"""
    K, e, _ = hp.small_shift_taps(d)
    r = hp.shift_stencil_radius(d)
    assert len(K) == 2 * r + 1 and r == math.ceil(abs(d)) + 34
    exact_K = [_exact_eta(-F(d) - m) for m in range(-r, r + 1)]
    _assert_within(K, exact_K, hp.SLACK * np.maximum(np.asarray(e, dtype=np.float64), 1e-300), 'shift taps')
    n = 9
    line = np.zeros(n)
    line[2] = 1.0
    want = _exact_shift(line, d)                                                  # (the float64 coordinate fl(fl(i - d) + 12), as SciPy forms it)
    ext = lambda i: F(float(line[int(hp.spline_extension_index(n, i))]))          # noqa: E731
    R = 150
    full = [sum(_exact_eta(-F(d) - m) * ext(i + m) for m in range(-R, R + 1)) for i in range(n)]
    cut = [sum(exact_K[m + r] * ext(i + m) for m in range(-r, r + 1)) for i in range(n)]
    pp_err = max(abs(F((float(i) - d) + 12.0) - (i - F(d) + 12)) for i in range(n))
    for i in range(n):
        # (SciPy's causal initialisation reads the running sum as c[0] in its last term: |z|^(2 N - 1) of the line away from the exact reflection)
        assert abs(full[i] - want[i]) <= abs(F(hp.SPLINE_POLE)) ** (2 * (n + 24) - 2) + 2 * pp_err, (i, float(full[i] - want[i]))
    tail = F(float(hp.shift_tail(d)))
    worst = max(abs(cut[i] - full[i]) for i in range(n))
    assert worst <= tail * F(1.0000001), (float(worst), float(tail))
    if abs(d) < 4:
        assert worst >= tail / 64, (float(worst), float(tail))                   # (the term is not a loose one: a single cell shows most of it)
    if not float(d).is_integer():
        assert 1e-23 < float(tail) < 1e-20                                        # |z|^35 = 9.7e-21: a quarter to all of it, by the fraction
    out, eo = hp.small_shift_stage(line, None, d, 0)
    _assert_within(out, want, hp.SLACK * eo, 'small shift stage')
    assert all(abs(F(float(c)) - w) <= F(float(hp.SLACK * b)) for c, w, b in zip([float(x) for x in cut], want, eo))


@needs_extended
def test_zero_boundary_and_dense_stages_against_exact_arithmetic():
    rng = np.random.default_rng(78)
    v = rng.random((4, 5)) ** 3
    vf = np.array(_frac(v), dtype=object).reshape(v.shape)
    for axis in (0, 1):
        n = v.shape[axis]
        k = rng.random(n)
        want = np.zeros(v.shape, dtype=object)
        for i in range(n):
            for j in range(n):
                idx_o, idx_i = [slice(None)] * 2, [slice(None)] * 2
                idx_o[axis], idx_i[axis] = i, j
                want[tuple(idx_o)] = want[tuple(idx_o)] + F(float(k[abs(i - j)])) * vf[tuple(idx_i)]
        got, eg = hp.zero_boundary_stage(v, None, k, axis)
        _assert_within(got, list(want.reshape(-1)), hp.SLACK * eg, 'zero boundary')
        _, eg2 = hp.zero_boundary_stage(v, None, k, axis, ew=np.full(n, 1e-18))
        assert np.all(eg2 >= eg) and np.any(eg2 > eg)
    kern = rng.random((3, 5))                                   # NOT point symmetric: a true convolution (scipy.signal.convolve2d)
    want = np.zeros(v.shape, dtype=object)
    for i in range(4):
        for j in range(5):
            for a in range(3):
                for b in range(5):
                    ii, jj = i - (a - 1), j - (b - 2)
                    if 0 <= ii < 4 and 0 <= jj < 5:
                        want[i, j] = want[i, j] + F(float(kern[a, b])) * vf[ii, jj]
    got, eg = hp.dense_stage(v, None, kern)
    _assert_within(got, list(want.reshape(-1)), hp.SLACK * eg, 'dense')
    from scipy.signal import convolve2d
    assert hp.worst(convolve2d(v, kern, mode='same'), got, hp.SLACK * eg) <= 1.0


@needs_extended
def test_transition_fit_is_gaussian_fit_for_one_walk_list():
    """the generalised pass restates the same lines of core.py: with one walk list for every step it returns gaussian_fit's values and bounds"""
    rng = np.random.default_rng(79)
    shape = (6, 5)
    prior = rng.random(shape)
    prior /= prior.sum()
    liks = [(rng.random(shape) + 0.1, np.full(shape, 1e-18)) for _ in range(3)]
    w = np.array([0.25, 0.5, 0.25])
    grids = [np.arange(6.0), np.arange(5.0)]
    a = hp.gaussian_fit(prior, liks, [(0, w), (1, w)], grids, [1.0, 1.0], nblk=2, clamp=-3.0)
    prog = ('prev', [('walk', 0, w), ('walk', 1, w), ('rs', float(10.0 ** -3.0))])
    b = hp.transition_fit(prior, liks, [dict(fwd=prog, bwd=prog)] * 3, grids, [1.0, 1.0], nblk=2)
    for key in ('alpha', 'post', 'norm', 'local', 'local_fwd', 'means'):
        for (va, ea), (vb, eb) in zip(a[key], b[key]):
            assert np.array_equal(np.asarray(va), np.asarray(vb)) and np.array_equal(np.asarray(ea), np.asarray(eb)), key
    assert a['log_evidence'] == b['log_evidence']


STEP_ORACLE_WORST = {}


def _step_names():
    import step_transition_cases as sc
    return sorted(sc.CASES)


@needs_extended
@pytest.mark.parametrize('name', _step_names())
def test_float64_oracle_is_inside_the_bounds_of_the_step_transition_problems(name):
    """oracle/bl_oracle.py (NumPy float64 with its own float64 tap tables, SciPy's recursion for the shifts) on EVERY problem of
    tests/test_step_transitions.py -- through the same driver, comparison and bounds, with the oracle test double in the engine's place.
    Inputs the reference itself cannot meet fail here, not on the card.  Prints the worst error / bound."""
    import step_transition_cases as sc
    from oracle_engine import OracleEngine
    eng = OracleEngine()
    case = sc.CASES[name]
    chk = sc.Check(name)
    for kind in case['inputs']:
        for driver in case['drivers']:
            refs, ok = sc.reference(name, kind, driver)
            keep = [b for b, o in enumerate(ok) if o]
            with np.errstate(all='ignore'):
                got = sc.run_problem(eng, name, kind, driver, keep, one_at_a_time=True)
            sc.compare(chk, name, kind, driver, keep, got, refs)
    fam = case['family']
    STEP_ORACLE_WORST[fam] = max(STEP_ORACLE_WORST.get(fam, 0.0), chk.top)
    print('float64 oracle, %s (%s): worst error / bound %.4f' % (name, fam, chk.top))
    assert not chk.bad, '\n'.join(chk.bad[:20])


@needs_extended
def test_what_the_step_transition_table_leaves_out():
    """the exact list of what transition_cases.well_conditioned (from the restatement alone) leaves out -- its class is an integer shift that moves
    the one occupied cell of a single-cell input off the grid -- and, named, not computed, NotEqual of the uniform alpha_0 of the backward driver, 0 / 0 in the reference"""
    import step_transition_cases as sc
    left = []
    for name, kind, driver in sc.combinations():
        if not any(m[0] in ('shift', 'as', 'biv') for m in sc.CASES[name]['models']):
            continue                                        # (no renormalising sum in the pass)
        _, ok = sc.reference(name, kind, driver)
        left += [(name, kind, driver, sc.CASES[name]['chains'][b]) for b, o in enumerate(ok) if not o]
    # nothing else is left out silently: every case runs all four inputs, and a case that does not run all three drivers is one of these
    assert all(c['inputs'] == sc.INPUTS for c in sc.CASES.values())
    three_only = sorted(n for n, c in sc.CASES.items() if c['drivers'] == ('three',))
    nd_three = ['%s_%s_%s' % (f, c, s) for f in ('chain_nd', 'nd') for c in ('cp_then_walk', 'independent', 'walk_then_cp')
                for s in ('3x3x7x6', '3x7x5', '5x18x14')]
    assert three_only == sorted(['chain1d_mixed_clamps_300', 'chain1d_mixed_shifts_300', 'chain1d_sources_300', 'chain_sources_128x16',
                                 'chainax_sources_32x32', 'fast_band8_sources_140x90', 'fused1d_sources_300', 'generic_change_point_24x20',
                                 'generic_composed_row_300', 'generic_independent_24x20', 'hwide_sources_40x300', 'mfma_band8_sources_140x90',
                                 'persist1d_sources_300', 'persist1d_walks_300', 'vwide_sources_140x64',
                                 # grids with three and four parameters, long rows: per-step programs; 8192 cells: the cost of the reference
                                 'chain1d_long_mixed_clamps_4100', 'chain1d_long_mixed_shifts_4100', 'chain1d_long_rs_or_shift_4100',
                                 'chain1d_long_sources_4100', 'chain1d_long_walks_8192', 'chain_nd_mixed_4x16x32', 'chain_nd_mixed_5x18x14',
                                 'nd_mixed_shifts_3x3x7x6', 'nd_mixed_shifts_5x18x14'] + nd_three), three_only     # per-step programs; T > 2 for bl1p::
    assert all(c['drivers'] in (sc.DRIVERS, ('three',), ('forward', 'three')) for c in sc.CASES.values())
    assert left == [], left                                 # (today: nothing; the single cells of the table's rows lie beyond 12 cells from the ends)
    assert sc.NOT_EQUAL_OF_UNIFORM == ['chain1d_long_not_equal_4100', 'chain1d_not_equal_300', 'chain1d_not_equal_600', 'generic_not_equal_20x140',
                                       'generic_not_equal_24x20', 'nd_ne_beside_restart_5x18x14', 'nd_ne_then_walk_5x18x14', 'nd_ne_walk_ne_5x18x14',
                                       'nd_not_equal_3x3x7x6', 'nd_not_equal_5x18x14', 'nd_walk_then_ne_5x18x14']
    for name in sc.NOT_EQUAL_OF_UNIFORM:
        assert 'backward' not in sc.CASES[name]['drivers'] and set(sc.CASES[name]['drivers']) == {'forward', 'three'}
    x = np.full((4, 5), 1.0 / 20)
    with np.errstate(all='ignore'):
        assert np.isnan(np.asarray(hp.not_equal_stage(x, None, 1e-4)[0], dtype=np.float64)).all()


# ---- the Poisson likelihood and the table models (tests/test_observation_kernels.py) -------------------------------------------------------------

def _d60(fn):
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        ctx.Emin, ctx.Emax = -999999999, 999999999
        return fn()


def _dfrac(x):
    return decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)


def _fexp(x):
    """exp of a Fraction at 60 digits -> Fraction (0 below 1e-100000: far below every bound)"""
    return _d60(lambda: F(_dfrac(x).exp()) if x > -230000 else F(0))


PO_RATES = np.array([0.0, 0.02, 1.0, 3.0, 59.8, 300.0, 740.0, 1000.0])
PO_RECORDS = [[0], [1], [6, float('nan')], [20, 50], [120], [170], [171], [200, float('nan'), 0], [400], [1000], [float('nan')] * 2]


@needs_extended
@pytest.mark.parametrize('k', range(len(PO_RECORDS)))
def test_poisson_likelihood_against_exact_arithmetic(k):
    """lambda^k / k! in rational arithmetic, exp(-lambda) with 60 digits: hp.poisson_likelihood stays within 1 / 8 of the bound of EITHER route;
    lambda = 0 gives 1 at k = 0 and 0 at k > 0; an all-NaN record 1"""
    rec = PO_RECORDS[k]
    L = hp.poisson_likelihood(PO_RATES, rec)
    counts = [int(c) for c in rec if c == c]
    if not counts:
        assert np.all(L == 1)
        return
    exact = []
    for lam in PO_RATES:
        v = F(1)
        for c in counts:
            v *= F(float(lam)) ** c / math.factorial(c) * _fexp(-F(float(lam)))
        exact.append(v)
    assert exact[0] == (1 if all(c == 0 for c in counts) else 0) and float(L[0]) == float(exact[0])
    for direct in (True, False):
        e, z = hp.poisson_bound(PO_RATES, rec, direct)
        assert np.all(e >= 0) and np.all(z > 0)
        _assert_within(L, exact, e + z, 'poisson, direct = %s' % direct)


def test_ln_factorial_and_the_host_factorial_count():
    """ln k! (exact from math.factorial up to 2000, Stirling's series beyond) against 60-digit ln of math.factorial; the host's loop of float64 products is exact while k! < 2^53 and within (k - 1) u beyond"""
    for k in (0, 1, 2, 18, 19, 107, 170, 171, 1000, 2000, 2001, 5000, 30000):            # (beyond 2000: Stirling's series)
        want = _d60(lambda: F(decimal.Decimal(math.factorial(k)).ln()))
        _assert_within([hp.ln_factorial(k)], [want], [float(want) * 2.0 ** -60 + 1e-30], 'ln %d!' % k)
    assert abs(hp.ln_factorial(30000) - hp.ln_factorial_exact(30000)) <= 4 * np.finfo(hp.LD).eps * hp.ln_factorial_exact(30000)
    f = 1.0
    for k in range(2, 171):
        f *= float(k)
        exact = math.factorial(k)
        assert (exact < 2 ** 53) == (k <= 18)
        if k <= 18:
            assert F(f) == exact
        assert abs(F(f) - exact) <= (k - 1) * F(hp.U) * exact
    assert math.isinf(f * 171.0)


def _host_ln_factorial(c):
    """build_records' factor of the log-space route: lgammal_r of the host's libm on (long double)c + 1, rounded to float64 once"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library('m'))
    libm.lgammal_r.restype = ctypes.c_longdouble
    libm.lgammal_r.argtypes = [ctypes.c_longdouble, ctypes.POINTER(ctypes.c_int)]
    return float(libm.lgammal_r(float(c) + 1.0, ctypes.byref(ctypes.c_int(0))))


@needs_extended
def test_the_hosts_ln_factorial_stays_inside_its_count():
    """lgammal_r rounded once against ln k! from math.factorial: inside C_LNFACT u ln k! on every count of tests/observation_cases.py"""
    import observation_cases as oc
    ks = sorted({int(c) for case in oc.POISSON_CASES for c in oc.poisson_records(case).reshape(-1) if c == c and c >= 2})
    assert ks[0] == 6 and ks[-1] == 1001500
    for k in ks:
        want = hp.ln_factorial(k)
        assert abs(hp.LD(_host_ln_factorial(k)) - want) <= hp.C_LNFACT * hp.LD(hp.U) * want, k


def _kernel_poisson64(rates, rec, direct):
    """blk::likelihood<OM_POISSON> restated in float64 NumPy, operation by operation, with build_records' factor (the float64 product loop, or
    -lgammal_r from the host's libm, rounded once)"""
    L = np.ones(len(rates))
    with np.errstate(all='ignore'):
        for c in rec:
            if c != c:
                continue
            if direct:
                f = 1.0
                for q in range(2, int(c) + 1):
                    f *= float(q)
                L = L * (np.power(rates, c) * np.exp(-rates) / f)
            else:
                arg = c * np.log(rates) - rates + (-_host_ln_factorial(c))
                L = L * np.where(rates == 0.0, 1.0 if c == 0.0 else 0.0, np.exp(arg))
    return L


@needs_extended
def test_both_poisson_routes_in_float64_on_the_cases_of_the_gpu_file():
    """the kernel's arithmetic restated in NumPy float64 on every grid and record of tests/observation_cases.py: the route the host selects stays
    inside the bound everywhere; the direct route outside its domain does not (0, inf or NaN where the likelihood is an ordinary number) --
    the defect the log-space route removes; inside the direct domain both routes hold"""
    import observation_cases as oc
    top, broken = 0.0, 0
    for case in oc.POISSON_CASES:
        for n in (300, 600):
            rates, recs = oc.poisson_rates(case, n), oc.poisson_records(case)
            for k, rec in enumerate(recs):
                direct = oc.direct_domain(rates, rec)
                L = hp.poisson_likelihood(rates, rec)
                for route in ((True, False) if direct else (False,)):
                    e, z = hp.poisson_bound(rates, rec, route)
                    q = hp.worst(_kernel_poisson64(rates, rec, route), L, hp.SLACK * (e + z))
                    top = max(top, q)
                    assert q <= 1.0, (case, n, k, route, q)
                if (case, k) in oc.POISSON_LEFT_OUT:
                    e, z = hp.poisson_bound(rates, rec, True)
                    got = _kernel_poisson64(rates, rec, True)
                    q = hp.worst(np.where(np.isfinite(got), got, np.inf), L, hp.SLACK * (e + z))
                    assert not q <= 1.0, (case, n, k)
                    broken += 1
    print('float64 restatement of the two Poisson routes: worst error / bound %.3f; %d records break the direct route' % (top, broken))
    assert broken == 2 * len(oc.POISSON_LEFT_OUT)


TB_G0 = {'bernoulli': [-0.25, 0.0, 0.3, 1.0, 1.25], 'white_noise': [1e-2, 0.7, 1e3], 'laplace': [-5.0, 0.1, 5.0],
         'ar1': [-(1.0 - 2.0 ** -20), -0.4, 0.0, 0.9, 1.0 - 2.0 ** -20]}
TB_G1 = {'laplace': [10.0, 0.3, 1e-4], 'ar1': [1e-2, 1.3, 1e3]}
TB_SEGS = {'bernoulli': [[[0.0]], [[1.0, 2.0, float('nan')]], [[-1.0, 0.5]], [[float('nan')]]],
           'white_noise': [[[0.0]], [[1.3, float('nan')]], [[1e3, -0.2]]],
           'laplace': [[[0.1]], [[0.1234, float('nan')]], [[-15.0, 1005.0]]],
           'ar1': [[[0.0], [0.0]], [[0.8, float('nan')], [-1.1, 0.3]], [[1e3, 0.4], [1e3, float('nan')]], [[0.5, 2.0], [0.45, -1.75]]]}


def _exact_table(model, g0, g1, seg):
    """the table model's likelihood per cell as a Fraction: rational arithmetic for the polynomial parts (sc^2 = g1^2 (1 - g0^2) included), 60-digit
    exp / ln / pi"""
    seg = np.asarray(seg, dtype=np.float64)
    dims = [k for k in range(seg.shape[1]) if not np.isnan(seg[:, k]).any()]
    pi = decimal.Decimal('3.14159265358979323846264338327950288419716939937510582097494')
    out = []
    for a in g0:
        for b in (g1 if g1 is not None else [None]):
            a_, b_ = F(float(a)), (None if b is None else F(float(b)))
            v = F(1)
            for k in dims:
                x0 = F(float(seg[0, k]))
                if model == 'bernoulli':
                    p = a_ if 0 <= a_ <= 1 else F(0)
                    v *= p if x0 != 0 else 1 - p
                elif model == 'laplace':
                    v *= _fexp(-abs(x0 - a_) / b_) / (2 * b_)
                else:
                    if model == 'white_noise':
                        r, s2 = x0, a_ * a_
                    else:
                        r = F(float(seg[1, k])) - a_ * x0
                        s2 = b_ * b_ * ((1 - a_ * a_) if model == 'scaled_ar1' else 1)
                    lnterm = _d60(lambda: F((2 * pi * _dfrac(s2)).ln() / 2))
                    v *= _fexp(-r * r / (2 * s2) - lnterm)
            out.append(v)
    return out


@needs_extended
@pytest.mark.parametrize('model', ['bernoulli', 'white_noise', 'laplace', 'ar1', 'scaled_ar1'])
def test_table_model_likelihoods_against_exact_arithmetic(model):
    base = 'ar1' if model == 'scaled_ar1' else model
    g0, g1 = np.array(TB_G0[base]), (np.array(TB_G1[base]) if base in TB_G1 else None)
    grids = [g0] if g1 is None else [g0, g1]
    for seg in TB_SEGS[base]:
        L, e, z = hp.TABLE_LIKELIHOODS[model](*grids, seg, bound=True)
        if np.isnan(np.asarray(seg)).any(axis=0).all():
            assert np.all(L == 1) and np.all(e == 0)
            continue
        _assert_within(L, _exact_table(model, g0, g1, seg), e + z, '%s %r' % (model, seg))


def test_scaled_ar1_cancellation_count():
    """g1 sqrt(1 - g0 g0) in float64 against the 60-digit root: inside (0.5 (1 + rho^2 / (1 - rho^2)) + 2) u for rho up to +-(1 - 2^-20) and beyond"""
    for rho in (0.0, 0.3, -0.9, 0.999, 1.0 - 2.0 ** -20, -(1.0 - 2.0 ** -20), 1.0 - 2.0 ** -30, 0.99999990000001):
        for s in (1e-2, 1.3, 1e3):
            got = s * math.sqrt(1.0 - rho * rho)
            one = 1 - F(rho) ** 2
            want = _d60(lambda: F(_dfrac(F(s) ** 2 * one).sqrt()))
            count = (F(1, 2) * (1 + F(rho) ** 2 / one) + 2) * F(hp.U)
            assert abs(F(got) - want) <= count * want, (rho, s)


OBS_ORACLE_WORST = {}


def _poisson_case_names():
    import observation_cases as oc
    return list(oc.POISSON_CASES)


@needs_extended
@pytest.mark.parametrize('case', _poisson_case_names())
def test_float64_oracle_is_inside_the_bounds_of_the_poisson_problems(case):
    """oracle/bl_oracle.py on every Poisson problem of tests/test_observation_kernels.py whose records it can evaluate, through the same driver,
    comparison and bounds (rows of 300 and of 600 rates); on the records of observation_cases.POISSON_LEFT_OUT it must FAIL -- raise, return a
    non-finite value, or miss the bound -- which checks the domain split in the case list itself.  The exception: the three records of `million`
    are NOT given to the oracle (it would form a factorial of five million digits, ten seconds each, before it raises as it does at 171); for
    them the split is held by oc.direct_domain alone"""
    import observation_cases as oc
    import test_observation_kernels as tk
    from oracle import bl_oracle as bo
    from oracle_engine import OracleEngine
    eng = OracleEngine()
    chk = tk.Check('poisson', OBS_ORACLE_WORST)
    ran = 0
    for n in (300, 600):
        for steps, full in tk.poisson_problems(case):
            if any((case, k) in oc.POISSON_LEFT_OUT for k in steps):
                continue
            with np.errstate(all='ignore'):
                tk.compare(eng, tk.poisson_setup(case, n, steps, full), full, chk, '%s n = %d records %s %s' % (case, n, list(steps), 'full' if full else 'forward'))
            ran += 1
        rates = oc.poisson_rates(case, n)
        for k, rec in enumerate(oc.poisson_records(case)):
            if (case, k) not in oc.POISSON_LEFT_OUT:
                continue
            assert not oc.direct_domain(rates, rec)
            if np.nanmax(rec) > 2000:                      # (the oracle would form a factorial of millions of digits before it raises as it does at 171)
                continue
            try:
                with np.errstate(all='ignore'):
                    got = bo.processed_pdf('poisson', [rates], rec.reshape(1, -1))
            except OverflowError:
                continue
            e, z = hp.poisson_bound(rates, rec, True)
            assert not np.isfinite(got).all() or hp.worst(got, hp.poisson_likelihood(rates, rec), hp.SLACK * (e + z)) > 1.0, (case, n, k)
    print('float64 oracle, Poisson %s: worst error / bound %.4f over %d problems' % (case, chk.top, ran))
    assert not chk.bad, '\n'.join(chk.bad[:20])


@needs_extended
@pytest.mark.parametrize('model', ['bernoulli', 'white_noise', 'laplace', 'ar1', 'scaled_ar1'])
def test_float64_oracle_is_inside_the_bounds_of_the_table_model_problems(model):
    """the same for EVERY table-model problem of tests/test_observation_kernels.py"""
    import observation_cases as oc
    import test_observation_kernels as tk
    from oracle_engine import OracleEngine
    eng = OracleEngine()
    chk = tk.Check('table_' + model, OBS_ORACLE_WORST)
    ran = 0
    for m, shape, case in tk.TABLE_ALL:
        if m != model:
            continue
        for steps, full in tk.table_problems(model, case):
            with np.errstate(all='ignore'):
                tk.compare(eng, tk.table_setup(model, shape, case, steps, full), full, chk, '%s %s records %s %s' % (shape, case, list(steps), 'full' if full else 'forward'))
            ran += 1
    print('float64 oracle, %s: worst error / bound %.4f over %d problems' % (model, chk.top, ran))
    assert not chk.bad, '\n'.join(chk.bad[:20])


def test_what_the_observation_table_leaves_out():
    """the float64 oracle runs every table-model problem and every Poisson problem but those with a record of this list: exactly the records
    outside the direct domain that hold a count above 0 -- 171 and more (OverflowError in the reference), lambda^k beyond the float64 range
    (inf, NaN), a subnormal or zero exp(-lambda) under a large lambda^k (no precision left, or inf * 0).  21 records of 9 cases; the oracle is
    asserted to fail on 18 of them, the three of `million` are not run (test_float64_oracle_is_inside_the_bounds_of_the_poisson_problems)"""
    import observation_cases as oc
    want = []
    for case in oc.POISSON_CASES:
        rates = oc.poisson_rates(case, 300)
        for k, rec in enumerate(oc.poisson_records(case)):
            assert oc.direct_domain(rates, rec) == oc.direct_domain(oc.poisson_rates(case, 600), rec)
            if not oc.direct_domain(rates, rec) and np.nanmax(np.append(rec, 0.0)) > 0:
                want.append((case, k))
    assert sorted(oc.POISSON_LEFT_OUT) == sorted(want) and len(want) == 21
    assert sorted(set(c for c, _ in oc.POISSON_LEFT_OUT)) == ['million', 'thousand_1', 'thousand_3', 'three_hundred_big', 'three_hundred_mixed_2',
                                                               'three_hundred_pow', 'tutorial_zero_normaliser', 'zero_first_log_2', 'zero_first_wide']
    # every count and every grid the case list has to hold is there
    counts = {int(c) for case in oc.POISSON_CASES for c in oc.poisson_records(case).reshape(-1) if c == c}
    assert {0, 1, 6, 20, 50, 120, 170, 171, 200, 400, 1000, 1000000} <= counts


# ---- long series: the scale history as a term of the bound (tests/scale_rules.py, tests/long_series_cases.py, tests/test_long_series.py) -------------

def _small_lazy_problem():
    rng = np.random.default_rng(791)
    shape = (6, 5)
    prior = rng.random(shape)
    prior /= prior.sum()
    liks = [((rng.random(shape) + 0.1) * 10.0 ** float(rng.integers(-80, 3)), np.full(shape, 1e-18)) for _ in range(7)]
    return shape, prior, liks, np.array([0.25, 0.5, 0.25])


@needs_extended
def test_unnamed_lazy_term_is_the_one_before_the_scale_rules():
    """No bound of an existing test changed: without a `scale` argument gaussian_fit and transition_fit return, bit for bit, the bounds that the
    file gave BEFORE the argument existed -- recorded then (tests/golden/lazy_term_bounds.npz: every alpha and posterior bound of a 6 x 5 problem
    over 7 steps whose normalisers reach 1e-80, as float64 (high, low) pairs of the longdouble; sums, products and quotients only, no libm) --
    and the same for three existing problems of the GPU files."""
    import os
    shape, prior, liks, w = _small_lazy_problem()
    grids = [np.arange(6.0), np.arange(5.0)]
    a = hp.gaussian_fit(prior, liks, [(0, w), (1, w)], grids, [1.0, 1.0], nblk=2, clamp=-3.0)
    prog = ('prev', [('walk', 0, w), ('walk', 1, w)])
    b = hp.transition_fit(prior, liks, [dict(fwd=prog, bwd=prog)] * 7, grids, [1.0, 1.0], nblk=2)
    then = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lazy_term_bounds.npz'))
    for nm, r in (('gaussian', a), ('transition', b)):
        for key in ('alpha', 'post'):
            now = np.stack([hp._ld(e) for _, e in r[key]])
            was = hp._ld(then['%s_%s' % (nm, key)][:, 0]) + hp._ld(then['%s_%s' % (nm, key)][:, 1])
            assert np.array_equal(now, was), (nm, key)
    # ... and of three problems of tests/test_step_transitions.py (their `decades` input, where the term is largest): every posterior bound of
    # the first chain, recorded before the change (tests/golden/lazy_term_bounds_cases.npz)
    import step_transition_cases as sc
    then = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lazy_term_bounds_cases.npz'))
    for name, kind, driver in (('chain_128x16', 'decades', 'three'), ('resident_32x32', 'decades', 'backward'), ('fused1d_walks_300', 'decades', 'three')):
        ref = sc.reference(name, kind, driver)[0][0]
        assert 'scale' not in ref
        was = then['%s_%s_%s' % (name, kind, driver)]
        now = np.stack([hp._ld(e) for _, e in ref['post']])
        assert np.array_equal(now, hp._ld(was[:, 0]) + hp._ld(was[:, 1])), name


RULES = [('step',), ('launch', 3), ('launch', 8), ('norm_lag', 2), ('norm_lag', 4), ('sum_lag', 1), ('sum_lag', 2), ('sum_lag', 3)]


def _rule_sums_exact(rule, n):
    """the sums a rule leaves, in rational arithmetic, each from its closed form where it has one (NOT by simulate_sums' recursion)"""
    T = len(n)
    if rule[0] == 'step':
        return list(n)
    if rule[0] == 'launch':
        return [math.prod(n[k - k % rule[1]:k + 1]) for k in range(T)]
    if rule[0] == 'norm_lag':                                   # the product of the last `lag` normalisers (blhip_chainres.hpp)
        return [math.prod(n[max(0, k - rule[1] + 1):k + 1]) for k in range(T)]
    S = []
    for k in range(T):                                          # the lagged sum has no closed form: S_k = S_(k-1) n_k / S_(k-lag)
        S.append((S[k - 1] if k else F(1)) * n[k] / (S[k - rule[1]] if k >= rule[1] else F(1)))
    return S


@needs_extended
@pytest.mark.parametrize('rule', RULES, ids=['%s%s' % (r[0], r[1] if len(r) > 1 else '') for r in RULES])
def test_scale_rule_term_against_exact_arithmetic(rule):
    """hp.transition_fit on a 3 x 2 grid, T = 8, a walk of three taps, under every scale rule: core.py:372-470 in rational arithmetic from the same float64
    likelihoods, whose normalisers span 1e-90 .. 1e+40 per step.  The sums the rule predicts (forward, backward in pass order behind the uniform
    message's 1, and S_fwd S_bwd sum(alpha beta) of every posterior) against their exact values; the three terms TINY / min(1, scale) rebuilt from
    those exact sums; and every posterior, forward state and local evidence inside its bound."""
    import scale_rules as sr
    rng = np.random.default_rng(17)
    shape, T = (3, 2), 8
    prior = rng.random(shape)
    prior /= prior.sum()
    decades = [-90, 40, -60, -75, 30, -88, 12, -50]
    liks = [rng.random(shape) * 10.0 ** decades[t] for t in range(T)]
    grids, lattice = [np.array([-1.0, 0.5, 2.0]), np.array([0.1, 0.7])], [1.5, 1.0]
    w = np.array([0.25, 0.5, 0.25])
    static = ('prev', [('walk', 0, w)])                         # (exact taps: the walk of the rational pass below)
    out = hp.transition_fit(prior, [(L, None) for L in liks], [dict(fwd=static, bwd=static)] * T, grids, lattice, nblk=1, full=True, scale=rule)
    base = hp.transition_fit(prior, [(L, None) for L in liks], [dict(fwd=static, bwd=static)] * T, grids, lattice, nblk=1, full=True, scale=('step',))
    P, Ls = _frac(prior), [_frac(L) for L in liks]

    def walk(x):                                                # reflecting, along the first parameter of the 3 x 2 grid (C order)
        rows = [x[0:2], x[2:4], x[4:6]]
        ext = [rows[0]] + rows + [rows[2]]
        return [F(1, 4) * ext[i][j] + F(1, 2) * ext[i + 1][j] + F(1, 4) * ext[i + 2][j] for i in range(3) for j in range(2)]
    alpha, norms, v = [], [], P
    for t in range(T):
        a = [x * l for x, l in zip(walk(v) if t else v, Ls[t])]
        N = sum(a)
        v = [x / N for x in a]
        alpha.append(v)
        norms.append(N)
    G = len(P)
    beta, Bs, Ds, posts = [F(1, G)] * G, [], {}, {}
    for t in range(T - 1, -1, -1):
        p = [x * y for x, y in zip(alpha[t], beta)]
        Ds[t] = sum(p)
        posts[t] = [x / Ds[t] for x in p]
        _assert_within(out['post'][t][0], posts[t], hp.SLACK * out['post'][t][1], 'post[%d]' % t)
        local = 1 / (sum(x / l for x, l in zip(posts[t], Ls[t])) * F(1.5))
        _assert_within([out['local'][t][0]], [local], [hp.SLACK * out['local'][t][1]], 'local[%d]' % t)
        if t > 0:
            b = walk([x * l for x, l in zip(beta, Ls[t])])
            Bs.append(sum(b))
            beta = [x / Bs[-1] for x in b]
    for t in range(T):
        _assert_within(out['alpha'][t][0], alpha[t], hp.SLACK * out['alpha'][t][1], 'alpha[%d]' % t)
    SF, SB = _rule_sums_exact(rule, norms), _rule_sums_exact(rule, [F(1)] + Bs)
    sc_ = out['scale']
    assert sc_['rule'] == sr.parse_rule(rule) and len(sc_['fwd']) == T and len(sc_['bwd']) == T

    def close(got, want, what):
        assert abs(F(*hp.LD(got).as_integer_ratio()) / want - 1) < F(1, 10 ** 13), (what, float(got), float(want))
    for k in range(T):
        close(sc_['fwd'][k], SF[k], 'forward sum %d' % k)
        close(sc_['bwd'][k], SB[k], 'backward sum %d' % k)
        close(sc_['post'][T - 1 - k], SF[T - 1 - k] * SB[k] * Ds[T - 1 - k], 'posterior sum %d' % (T - 1 - k))
    # the terms, from the exact sums: the un-normalised product of step k is held at S_k / n_k
    tiny = F(hp.TINY)
    H = hp.ScaleHistory(rule, {})
    for k in range(T):
        close(H.forward_term(False, False), tiny / min(F(1), SF[k] / norms[k]), 'forward term %d' % k)
        H.forward_done(hp._ld(float(norms[k])), False, False)
    for k in range(T):
        t = T - 1 - k
        close(H.posterior_term(t), tiny / (min(F(1), SF[t]) * min(F(1), SB[k])), 'posterior term %d' % t)
        if t > 0:
            close(H.backward_term(False, False), tiny / min(F(1), SB[k + 1] / Bs[k]), 'backward term %d' % t)
            H.backward_done(hp._ld(float(Bs[k])), False, False)
    # ... and they are IN the bounds: a rule whose state is smaller than the per-step rule's has the larger bound, cell by cell
    for t in range(T):
        smaller = min(F(1), SF[t]) * min(F(1), SB[T - 1 - t]) <= min(F(1), norms[t]) * min(F(1), ([F(1)] + Bs)[T - 1 - t])
        if smaller:
            assert np.all(out['post'][t][1] >= base['post'][t][1] * (1 - 1e-12)), t


@needs_extended
def test_scale_history_is_simulate_sums_with_restarts_and_clamped_steps():
    """the incremental form highprec uses (scale_rules.History) against the restatement tests/test_host_logic.py pins the host's inverse to
    (scale_rules.simulate_sums), at the schedules of the long series, with restarts behind steps 5 and 9 and clamped steps"""
    import long_series_cases as ls
    import scale_rules as sr
    for schedule in ls.SCHEDULES:
        n = np.exp2(hp._ld(ls.exponents(schedule))) * hp._ld(np.random.default_rng(3).uniform(0.9, 1.1, ls.steps_of(schedule)))
        T = len(n)
        kinds, clamped = np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.uint8)
        kinds[[6, 10]] = 2
        clamped[[3, 7, 8, 12]] = 1
        for lag in (1, 2, 3, 4):
            for scheme, rule in ((0, ('sum_lag', lag)), (1, ('norm_lag', lag)), (2, ('norm_lag', lag))):
                for kd in (None, kinds):
                    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
                        S, s = sr.simulate_sums(n, lag, scheme, kd, clamped if scheme == 2 else None)
                        H = sr.History(rule)
                        for k in range(T):
                            fresh, cl = kd is not None and bool(kd[k]), scheme == 2 and bool(clamped[k])
                            pre = H.pre(fresh, cl)
                            H.push(n[k], fresh, cl)
                            if np.isfinite(S[k]) and S[k] > 0:
                                assert abs(H.S[k] / S[k] - 1) < 1e-15 and abs(pre * n[k] / S[k] - 1) < 1e-15, (schedule, lag, scheme, k)
    assert sr.parse_rule('norm_lag(4)') == ('norm_lag', 4) and sr.parse_rule('step') == ('step',) and sr.parse_rule(('launch', 8)) == ('launch', 8)


@needs_extended
def test_gaussian_fit_under_a_scale_rule_is_transition_fit_with_clamped_steps():
    """gaussian_fit(scale = rule) is transition_fit over the one program; with a clamp every step behind the first runs at the exact scale
    (scheme 2): the sums it predicts are simulate_sums(.., 2) of its own normalisers with every step clamped; values as without a rule"""
    import scale_rules as sr
    shape, prior, liks, w = _small_lazy_problem()
    grids = [np.arange(6.0), np.arange(5.0)]
    plain = hp.gaussian_fit(prior, liks, [(0, w), (1, w)], grids, [1.0, 1.0], nblk=2, clamp=-3.0)
    for rule, scheme in ((('norm_lag', 2), 2), (('norm_lag', 4), 2), (('sum_lag', 2), 0), (('step',), None)):
        out = hp.gaussian_fit(prior, liks, [(0, w), (1, w)], grids, [1.0, 1.0], nblk=2, clamp=-3.0, scale=rule)
        for key in ('alpha', 'post'):
            for (va, _), (vb, eb) in zip(plain[key], out[key]):
                assert np.array_equal(np.asarray(va), np.asarray(vb)) and np.all(np.isfinite(np.asarray(eb, dtype=np.float64)))
        n = hp._ld([N for N, _ in out['norm']])
        if scheme is None:
            want = n
        else:
            with np.errstate(all='ignore'):
                want, _ = sr.simulate_sums(n, rule[1], scheme, None, np.ones(len(n), dtype=np.uint8) if scheme == 2 else None)
        assert np.all(np.abs(hp._ld(out['scale']['fwd']) / want - 1) < 1e-15), rule
    free = hp.gaussian_fit(prior, liks, [(0, w), (1, w)], grids, [1.0, 1.0], nblk=2, scale='norm_lag(2)')      # no clamp: the lagged rule itself
    n = hp._ld([N for N, _ in free['norm']])
    assert np.all(np.abs(hp._ld(free['scale']['fwd']) / sr.simulate_sums(n, 2, 1)[0] - 1) < 1e-15)


LONG_ORACLE_WORST, LONG_VERDICTS = {}, {}


def _long_families():
    import long_series_cases as ls
    return list(ls.FAMILIES)


@needs_extended
@pytest.mark.parametrize('fam', _long_families())
def test_float64_oracle_is_inside_the_bounds_of_the_long_series_problems(fam):
    """oracle/bl_oracle.py (NumPy float64; it normalises at every step) on EVERY problem of tests/test_long_series.py -- full fits, forward-only
    fits, and against the bounds of every rule of the lag sweep -- through the same driver, comparison and bounds.  Prints the worst error / bound."""
    import long_series_cases as ls
    import step_transition_cases as sc
    from oracle_engine import OracleEngine
    eng = OracleEngine()
    chk = sc.Check(fam)
    jobs = [(s, True, None) for f, s in ls.combinations() if f == fam] + [(s, False, None) for f, s in ls.forward_combinations() if f == fam] + \
           [(s, True, r) for f, s, r in ls.lag_combinations() if f == fam]
    runs = {}
    for schedule, full, rule in jobs:
        R = ls.reference(fam, schedule, full=full, rule=rule)
        LONG_VERDICTS[(fam, schedule, full, R['rule'])] = (R['verdict'], R['fwd'], R['bwd'], R['keep'], len(R['refs']))
        assert R['verdict'] != 'refused', (fam, schedule, full, rule)
        if (schedule, full) not in runs:
            with np.errstate(all='ignore'):
                runs[(schedule, full)] = ls.run_problem(eng, fam, schedule, list(range(len(R['refs']))), full=full, one_at_a_time=True)
        got = runs[(schedule, full)]
        top = chk.top
        chk.top = 0.0
        ls.compare(chk, fam, schedule, R['keep'], {k: [v[b] for b in R['keep']] for k, v in got.items() if k != 'timing'}, R['refs'], full=full)
        LONG_ORACLE_WORST[(fam, schedule, full, R['rule'])] = chk.top
        print('float64 oracle, %s %s %s %r (%s): worst error / bound %.4f' % (fam, schedule, 'full' if full else 'forward', R['rule'], R['verdict'], chk.top))
        chk.top = max(chk.top, top)
    assert not chk.bad, '\n'.join(chk.bad[:20])


@needs_extended
def test_long_series_schedules_meet_their_conditions():
    """Conditions, not measurements, from the reference alone: what each family's restated rule predicts its host guard to do on every schedule --
    the table below is exact --, every prediction a factor 1e6 clear of the threshold that decides it or the combination refused (the exact
    list), every predicted sum inside (1e-290, 1e290) (asserted where the prediction is formed), no chain dropped; the amplitudes of the resonant
    schedules as the restated sum_lag(2) rule chooses them; the family that is left out, and that nothing else is."""
    import long_series_cases as ls
    import scale_rules as sr

    def verdict(fam, schedule, full=True, rule=None):
        key = (fam, schedule, full, ls.FAMILIES[fam]['rule'] if rule is None else rule)
        if key not in LONG_VERDICTS:
            R = ls.reference(fam, schedule, full=full, rule=rule)
            LONG_VERDICTS[key] = (R['verdict'], R['fwd'], R['bwd'], R['keep'], len(R['refs']))
        return LONG_VERDICTS[key]

    assert (ls.RESONANT_IN, ls.RESONANT_OUT) == (27, 41)
    assert ls.FAMILIES['fused1d']['rule'] == ('launch', 6) and ls.FAMILIES['persist1d']['rule'] == ('launch', 2)
    assert ls.launch_steps(8, 14, 32) == 8 and ls.launch_steps(8, 3, 5) == 3 and ls.launch_steps(8, 14, 300) == 1
    assert max(c[0] for c in ls.sc.CASES['fused1d_walks_300']['chains']) == 40
    for a, lo, hi in ((ls.RESONANT_IN, 110, 120), (ls.RESONANT_OUT, 165, 175)):
        S, _ = sr.simulate_sums(np.exp2(hp._ld(ls._resonant(a, ls.T_RESONANT))), 2, 0)
        assert lo <= float(np.max(np.abs(np.log10(S)))) < hi                 # (each step is only 2^+-a = 1e+-8 / 1e+-12)
        Sc, _ = sr.simulate_sums(np.exp2(hp._ld(ls._resonant(a, ls.T_RESONANT))), 4, 1)
        assert float(np.max(np.abs(np.log10(Sc)))) < 19                      # the chain rule under the same drive
    special = {('resident', 'resonant_out'): 'range', ('fused1d', 'ramp'): 'repeat'}
    special.update({(f, 'burst_out'): 'range' for f in ('chain', 'chain_sources', 'chainax')})
    special.update({c: 'refused' for c in ls.REFUSED})
    for fam, schedule in ls.combinations(refused=True):
        v, fwd, bwd, keep, n = verdict(fam, schedule)
        assert v == special.get((fam, schedule), 'none'), (fam, schedule, v, fwd, bwd)
        assert keep == list(range(n)), (fam, schedule, keep)                 # no chain is dropped
    assert sorted(c for c in ls.combinations(refused=True) if verdict(*c)[0] == 'refused') == sorted(ls.REFUSED)
    # just inside the time-resident guard: 1e+-110 of 1e+-150; the chain rule stays far inside under both resonant schedules
    assert 1e108 < verdict('resident', 'resonant_in')[1][1] < 1e112
    for fam in ('chain', 'chain_sources', 'chainax'):
        for schedule in ('resonant_in', 'resonant_out'):
            lo, hi = verdict(fam, schedule)[1]
            assert 1e-40 < lo and hi < 1e40, (fam, schedule, lo, hi)
    for fam, schedule in ls.forward_combinations():
        assert verdict(fam, schedule, full=False)[0] == 'none', (fam, schedule)      # (fused1d, ramp: six steps per launch leave 2.4e-181, no repeat; the full fit's posterior sums repeat it)
    # the lag sweep: the chain rule at lag 2 and 3, the lagged sum at lag 1 and 3.  Lag 3 of the lagged sum is exponentially unstable
    # (|roots of r^3 - r^2 + 1| = 1.15): at T = 14 it stays inside the guard on `flat`, and a burst of five sends it beyond
    for fam, schedule, rule in ls.lag_combinations():
        want = 'range' if (fam, schedule, rule) == ('resident', 'burst_in', ('sum_lag', 3)) else 'none'
        assert verdict(fam, schedule, rule=rule)[0] == want, (fam, schedule, rule, verdict(fam, schedule, rule=rule))
    assert ls.NOT_RUN[:2] == [('chain1d_long', 'resonant_in'), ('chain1d_long', 'resonant_out')]
    assert sorted(set(f for f, _ in ls.NOT_RUN[2:])) == sorted(set(ls.FAMILIES) - set(ls.LAGGED)) and set(s_ for _, s_ in ls.NOT_RUN[2:]) == {'ramp_80', 'burst_mild'}
    # the shifts: two per chain keep every renormalising sum conditioned (no chain dropped, above); a shift at EVERY step would not
    case = ls.case_of('chain1d_shifts', ls.T_LONG)
    assert all(sum(1 for d in c[0] if d != 0.0) == 2 and len(c[0]) == ls.T_LONG - 1 for c in case['chains']) and len(case['chains']) == 8
    every = dict(case, chains=[(tuple(c[0][3] if k % 2 == 0 else -c[0][3] for k in range(ls.T_LONG - 1)),) for c in case['chains'][:1]])
    prior, lik, reset, indep = ls.tables('chain1d_shifts', 'flat')
    ref = hp.transition_fit(prior, [(L, None) for L in lik], ls.sc.stage_program(every, every['chains'][0], 'three', ls.T_LONG), [np.arange(300.0)], [1.0],
                            nblk=ls.sc.nblk_of((300,)), full=True, shared=dict(reset=reset, indep=indep), scale=('step',))
    assert ls.conditioned([ref]) == [False]


def _gaussian_long():
    import long_series_cases as ls
    return list(ls.GAUSSIAN)


@needs_extended
@pytest.mark.parametrize('fam', _gaussian_long())
def test_float64_oracle_is_inside_the_bounds_of_the_gaussian_long_series(fam):
    """oracle/bl_oracle.py on the Gaussian problems of tests/test_long_series.py, full and forward-only, held to the bounds the kernels are held
    to; the series fall in the classes they are named for, by their longdouble normalisers; none of them leaves a guard of its family's rule"""
    import long_series_cases as ls
    import test_likelihood_kernels as tl
    from oracle import bl_oracle as bo
    chk = tl.Check('oracle long ' + fam)
    for name in ls.SERIES:
        for full in (True, False):
            problem, values, refs, liks, rec_ok = ls.gaussian_setup(fam, name, full)
            assert rec_ok and all(tl.aborted_at(r) is None for r in refs)
            verdict, fwd, bwd = ls.prediction(refs, ls.GAUSSIAN[fam], full)
            assert verdict == 'none', (fam, name, full, verdict, fwd, bwd)
            low = min(float(N) for r in refs for N, _ in r['norm'][1:])
            assert {'calm': low >= ls.CALM, 'jumping': low < ls.JUMP, 'jumping_period6': ls.JUMP <= low < ls.CALM}[name], (fam, name, low)
            g = bo.Grid(problem.marginal)
            T = len(problem.data)
            for c, ref in enumerate(refs):
                with np.errstate(all='ignore'):
                    r = bo.fit(g, 'gaussian', problem.data, problem.timestamps, problem.prior, [('grw', op[1]) if op[0] == tl._abi.OP_GRW else ('regimeswitch',) for op in problem.ops], list(values[c]), forward_only=not full)
                assert r['abort'] is None
                w = '%s %s chain %d' % (name, 'full' if full else 'forward', c)
                chk.within([r['logEvidence']], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
                for t in range(T):
                    want = ref['post'][t] if full else ref['alpha'][t]
                    chk.within(r['posteriorSequence'][t], want[0], want[1], w + ' posterior[%d]' % t)
                    loc = ref['local'][t] if full else ref['local_fwd'][t]
                    chk.local(r['localEvidence'][t], loc[0], loc[1], w + ' localEvidence[%d]' % t)
                    chk.within(np.asarray(r['posteriorMeanValues'])[:, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)
    print('float64 oracle, gaussian %s: worst error / bound %.4f' % (fam, chk.top))
    assert not chk.bad, '\n'.join(chk.bad[:20])
