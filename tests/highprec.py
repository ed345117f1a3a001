"""
High-precision restatements of what the library computes AFTER the forward / backward passes, and the error bounds the float64
kernels are held to (tests/test_postfit_kernels.py on the GPU; tests/test_highprec.py checks this file against exact rational
arithmetic on the CPU).

Written from the formulas of include/blhip.h (the accumulator A[t, cell] = sum_h exp(logE_h + log prior_h - log_ref) max(post_h, 1e-300),
its per-step normalisation and means, the marginals and the time average of a sequence, the mixtures of carried states) and of the
reference (core.py:1358-1366 logaddexp accumulation, :1379-1382 normalisation, :1416-1419 means), not from the kernels.

Every quantity is a sum of n terms.  For float64 terms of one sign, summed in ANY order (tree, groups of four, fused or not),
    |fl(sum) - sum| <= n u / (1 - n u) * sum,        u = 2 ** -53,
and every further rounded operation adds one u.  The bound functions below are that count for each operation, times SLACK = 2 and nothing
more.  The references are carried in np.longdouble (64-bit mantissa on x86: 2 ** -11 of u per operation); on a platform whose long
double is a float64 the sums fall back to math.fsum (exact) per cell.

The second half of the file restates the stages of a TRANSITION the same way (the Deterministic model's spline shift with a running bound,
the renormalisation, RegimeSwitch, NotEqual, the random walk) for tests/test_transition_kernels.py; its recursions need the wider type.

The third part restates the GAUSSIAN LIKELIHOOD (observationModels.py:566-567, :49-54, :705-706), counts the rounded operations of the two
ways the kernels evaluate it (one exp per value and cell; the multiplicative recurrence along the rows, anchored with blmath::exp_mn) and
runs a small forward-backward pass with a running bound for tests/test_likelihood_kernels.py.

The fourth part restates the host's TAP TABLES (SciPy's Gaussian weights, the alpha-stable and the bivariate kernel, the cardinal-spline weights
of a small shift) with the bound of a float64 builder, the zero-boundary, dense and small-shift stages with the stencil's truncation term, and
generalises the small pass to a per-step stage program (transition_fit) for tests/test_step_transitions.py.
For tests/test_long_series.py the passes take the family's SCALE RULE (tests/scale_rules.py; ScaleHistory): the subnormal step through the scale
the rule gives a lazily normalised state, and in transition_fit a projective bound that grows linearly along time beside the running one.
"""
import math

import numpy as np

import scale_rules as sr

U = 2.0 ** -53
TINY = 2.0 ** -1074      # the subnormal step: below the normal range (2 ** -1022) a rounded product or quotient is off by up to half of it, whatever
                         # its size; sums are exact there.  Bounds of operations with a product or a division carry this absolute term per such operation.
SLACK = 2.0
CLAMP = 1e-300
LD = np.longdouble
EXTENDED = np.finfo(np.longdouble).nmant >= 63


def _ld(a):
    return np.asarray(a, dtype=LD)


def _sum(a, axis):
    """Sum along `axis` (an int or a tuple): longdouble where it is wider than float64, math.fsum per output cell otherwise."""
    a = np.asarray(a)
    if EXTENDED:
        return _ld(a).sum(axis=axis)
    axes = (axis,) if isinstance(axis, int) else tuple(axis)
    axes = tuple(x % a.ndim for x in axes)
    keep = [k for k in range(a.ndim) if k not in axes]
    b = np.transpose(np.asarray(a, dtype=np.float64), keep + list(axes))
    shape = b.shape[:len(keep)]
    b = b.reshape(int(np.prod(shape, dtype=np.int64)), -1)
    return _ld(np.array([math.fsum(row) for row in b]).reshape(shape))


# ---- the evidence-weighted average posterior ----------------------------------------------------------------------------------------

def fold(posts, log_w, prev=None, prev_ref=None):
    """Folds the chains `posts` (B, T, G) with float64 log-weights `log_w` (B,) into an accumulator.

    prev / prev_ref: what the accumulator holds already, (T, G) longdouble relative to the reference exponent prev_ref (None: nothing).
    Returns (A, ref, n): A[t, c] = prev exp(prev_ref - ref) + sum_h exp(log_w[h] - ref) max(posts[h, t, c], 1e-300) over the chains with a
    finite log_w, ref = max(prev_ref, max finite log_w), n = the number of chains that were folded.  With nothing to fold and no prev:
    (None, -inf, 0)."""
    posts = np.asarray(posts, dtype=np.float64)
    log_w = np.asarray(log_w, dtype=np.float64).reshape(-1)
    assert posts.ndim == 3 and posts.shape[0] == log_w.shape[0]
    ok = np.isfinite(log_w)
    ref = -math.inf if prev is None else float(prev_ref)
    if ok.any():
        ref = max(ref, float(log_w[ok].max()))
    if not math.isfinite(ref):
        return None, ref, 0
    refl = LD(ref)
    if prev is None:
        A = np.zeros(posts.shape[1:], dtype=LD)
    else:
        A = _ld(prev) * np.exp(LD(prev_ref) - refl)
    if EXTENDED:
        for h in np.nonzero(ok)[0]:
            A = A + np.exp(LD(log_w[h]) - refl) * _ld(np.maximum(posts[h], CLAMP))
    elif ok.any():
        # no wider type: products in float64 (one u each, inside the '3' of fold_bound), the sum over chains exact
        terms = [np.asarray(A, dtype=np.float64)] + [math.exp(log_w[h] - ref) * np.maximum(posts[h], CLAMP) for h in np.nonzero(ok)[0]]
        A = _sum(np.stack(terms), 0)
    return A, ref, int(ok.sum())


def fold_span(log_w, ref, earlier=()):
    """X of fold_bound: the largest |log-weight - ref| among the chains (finite log-weights) and the earlier references that contribute,
    i.e. whose weight exp(log_w - ref) is not zero in float64 (|.| <= 745)."""
    d = [abs(float(x) - ref) for x in list(np.asarray(log_w, dtype=np.float64).reshape(-1)) + list(earlier) if math.isfinite(x)]
    d = [x for x in d if x <= 745.2]
    return max(d) if d else 0.0


def fold_bound(A, n_chains, n_earlier, span):
    """|accumulator - fold()| for B = n_chains chains folded onto k = n_earlier earlier folds: (B + k + 3 + X) u relative -- B + k terms,
    3 for the exp, the product with the row normaliser and the rescale factor, X u for the rounded argument of the exp -- plus B 1e-300
    for clamp terms that underflow under a small weight (and for weights below exp(-745), which are zero in float64)."""
    return SLACK * ((n_chains + n_earlier + 3 + span) * U * np.abs(np.asarray(A, dtype=np.float64)) + n_chains * CLAMP)


def rescale(A, ref, new_ref):
    """The accumulator re-expressed against new_ref >= ref."""
    return _ld(A) * np.exp(LD(ref) - LD(new_ref))


def _grid_values(grids, k, shape):
    idx = [None] * len(shape)
    idx[k] = slice(None)
    return np.broadcast_to(np.asarray(grids[k], dtype=np.float64)[tuple(idx)], shape)


def row_stats(A, grids):
    """(T, 1 + ndim) [sum A, sum A grid_0, ...] of A (T, G) on the grid with marginal values `grids` (C order: last parameter fastest),
    and the same with |grid_k| (what the bounds of the signed sums are relative to)."""
    A = np.asarray(A)
    shape = tuple(len(g) for g in grids)
    T = A.shape[0]
    Ar = _ld(A).reshape((T,) + shape)
    axes = tuple(range(1, 1 + len(shape)))
    out = np.zeros((T, 1 + len(shape)), dtype=LD)
    out_abs = np.zeros((T, 1 + len(shape)), dtype=LD)
    out[:, 0] = out_abs[:, 0] = _sum(Ar, axes)
    for k in range(len(shape)):
        g = _ld(_grid_values(grids, k, shape))
        if EXTENDED:
            out[:, 1 + k] = (Ar * g).sum(axis=axes)
            out_abs[:, 1 + k] = (Ar * np.abs(g)).sum(axis=axes)
        else:
            out[:, 1 + k] = _sum(np.asarray(Ar, dtype=np.float64) * np.asarray(g, dtype=np.float64), axes)
            out_abs[:, 1 + k] = _sum(np.asarray(Ar, dtype=np.float64) * np.abs(np.asarray(g, dtype=np.float64)), axes)
    return out, out_abs


def row_stats_bound(stats_abs, G):
    """G terms, one product each: (G + 1) u relative to the sum of absolute values."""
    return SLACK * ((G + 1) * U * np.abs(np.asarray(stats_abs, dtype=np.float64)) + G * TINY)


def finalize(A, grids):
    """-> (norm (T,), normalised rows (T, G), means (ndim, T), absolute means (ndim, T)): norm = sum_c A, rows A / norm,
    means sum A grid_k / sum A, absolute means sum A |grid_k| / sum A."""
    A = np.asarray(A)
    st, st_abs = row_stats(A, grids)
    norm = st[:, 0]
    rows = _ld(A) / norm[:, None]
    means = (st[:, 1:] / norm[:, None]).T
    means_abs = (st_abs[:, 1:] / norm[:, None]).T
    return norm, rows, means, means_abs


def normalised_bound(rows, G):
    """A normalised row: the sum of G terms, the reciprocal and the product: (G + 2) u relative."""
    return SLACK * ((G + 2) * U * np.abs(np.asarray(rows, dtype=np.float64)) + TINY)


def mean_bound(means_abs, G):
    """sum A grid_k / sum A: two sums of G terms (one with a product), one division: (G + 3) u relative to sum A |grid_k| / sum A
    (the grid values change sign: the terms of the numerator cancel, its error does not)."""
    return SLACK * (G + 3) * U * np.abs(np.asarray(means_abs, dtype=np.float64))


# ---- reductions of a sequence ----------------------------------------------------------------------------------------------------------

def marginal(p, k):
    """p (T, n_0, .., n_(d-1)) -> (T, n_k): sums over the other parameters."""
    p = np.asarray(p)
    axes = tuple(a + 1 for a in range(p.ndim - 1) if a != k)
    if not axes:
        return _ld(p)
    return _sum(p, axes)


def marginal_bound(m, n_reduced):
    return SLACK * (n_reduced + 1) * U * np.abs(np.asarray(m, dtype=np.float64))


def time_average(p):
    """p (T, ...) -> (...): mean over the time steps."""
    p = np.asarray(p)
    return _sum(p, 0) / LD(p.shape[0])


def time_average_bound(m, T):
    return SLACK * ((T + 1) * U * np.abs(np.asarray(m, dtype=np.float64)) + TINY)


# ---- mixtures of carried states ----------------------------------------------------------------------------------------------------------

def mix(states, w, prev=None):
    """(prev or 0) + sum_j w[j] states[j]; states (n, G).  Returns (mix, magnitude): magnitude = |prev| + sum_j |w[j]| states[j], what
    mix_bound is relative to."""
    states = np.asarray(states, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    assert states.shape[0] == w.shape[0]
    if EXTENDED:
        m = (_ld(w)[:, None] * _ld(states)).sum(axis=0)
        mag = (np.abs(_ld(w))[:, None] * np.abs(_ld(states))).sum(axis=0)
    else:
        m = _sum(w[:, None] * states, 0)
        mag = _sum(np.abs(w)[:, None] * np.abs(states), 0)
    if prev is not None:
        m = m + _ld(prev)
        mag = mag + np.abs(_ld(prev))
    return m, mag


def mix_bound(magnitude, n_chains):
    """n products accumulated onto one earlier value: (n_chains + 1) u relative to |prev| + sum |w_j| state_j."""
    return SLACK * ((n_chains + 1) * U * np.abs(np.asarray(magnitude, dtype=np.float64)) + n_chains * TINY)


def worst_at(got, want, bound):
    """Where worst() is attained: (flat index, got, want, bound) there."""
    err = np.abs(_ld(got) - _ld(want)).reshape(-1)
    b = _ld(bound).reshape(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, LD(0), err / b)
    q = np.where(np.isnan(q), LD(np.inf), q)
    i = int(np.argmax(q))
    return i, np.asarray(got).reshape(-1)[i], np.asarray(want).reshape(-1)[i], np.asarray(bound).reshape(-1)[i]


def worst(got, want, bound):
    """max over the cells of |got - want| / bound (0 / 0 = 0): <= 1 passes.  For messages and assertions alike."""
    err = np.abs(_ld(got) - _ld(want))
    b = _ld(bound)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, LD(0), err / b)
    if q.size == 0:
        return 0.0
    return float(np.max(np.where(np.isnan(q), LD(np.inf), q)))


# ---- stages of a transition: the Deterministic model's spline shift and what can stand before or behind it -----------------------------
#
# Written from the reference (transitionModels.py:559-606: scipy.ndimage.shift(order = 3, mode = 'nearest') and the division by the sum;
# :405-412 RegimeSwitch; :462-471 NotEqual; :107-115 the random walk as scipy.ndimage.gaussian_filter1d) and from SciPy's ni_splines.c
# recursion as oracle/bl_oracle.py documents it (spline_prefilter_reflect, spline_shift_nearest), not from the kernels.
#
# Every stage function takes the stage's input v (float64 or longdouble) and the bound e >= |device input - v| the input comes with (0 or
# None for a caller's array) and returns the output and ITS bound: the incoming bound carried through the stage's magnitudes plus the
# stage's own rounded operations.  These `e` are first-order bounds WITHOUT the file's SLACK: a test multiplies the last one by SLACK, once.

SPLINE_POLE = -0.2679491924311227          # SciPy's float64 literal (ni_splines.c: get_filter_poles, order 3)
SPLINE_PAD = 12                            # edge samples per side (_prepad_for_spline_filter, mode 'nearest')
REQUIRES_EXTENDED = 'the spline recursion needs a long double wider than float64 (no exact-sum fallback exists for a recursion)'

# rounded float64 operations of the device per element, counted along the device's order of evaluation (blk::spline_prefilter_wave: a lane
# owns a chunk of C = spline_chunk(N) elements; blk::bigshift_kernel samples).  Counts, not measurements:
C_GAIN = 4        # x * gain: the product, and the float64 constant (1 - z) (1 - 1 / z) itself (a subtraction, a quotient and subtraction, a product)
C_PASS = 20       # one first-order pass, per element: the sweep with a zero carry-in and the sweep from the true carry-in, a product and a
#                   sum each (4); the carry that enters the chunk went through six affine_step()s, each a fused multiply-add of the carry (6)
#                   and a product of the factors z^len (6); those factors come from pow(): within 2 ulp = 4 u.  Every one of these
#                   acts on a value whose magnitude the running m[i] dominates, so the element collects (4 + 6 + 6 + 4) u m[i].
C_TOP = 3         # u[N-1] = y[N-1] * (z / (z - 1)): the constant's subtraction and quotient, the product
W_OPS = 6         # a B-spline weight in float64: |pp - k| (1), then 2/3 - a a + a a a / 2 (the constant, two products + one, two sums; the
#                   halving is exact) or (2 - a)^3 / 6: at most 6 operations on quantities <= 1, so the weight is off by <= 6 u ABSOLUTELY
C_SAMPLE = 5      # the four fused multiply-adds of the weighted sum and the product with the stage's input scale


def spline_chunk(N):
    """elements per lane of the device's prefilter for a padded line of N (its operation count enters the bound of c[0])"""
    return ((int(N) + 63) >> 6) | 1


def c_init(N):
    """Rounded operations behind the causal initialisation c[0] += z / (1 - z^2N) sum_i z^i (c[i] + z^N c[N-1-i]), per term of the sum:
    z^N from pow() (4) times c (1) plus c (1); z^i = pow() of the chunk's first index (4) times C products (C); the product with it (1);
    the lane's running sum (C) and the six steps of the wave's sum (6); the factor z / (1 - z^2N) (a product, a subtraction, a quotient: 3)
    and the product with it (1); the sum with c[0] (1): 22 + 2 C."""
    return 22 + 2 * spline_chunk(N)


def _moved(x, axis):
    return np.moveaxis(np.asarray(x), axis, 0)


_MEMO = {}


def _memo(tag, arrays, make):
    """the coefficients of a line do not depend on the shift: the last few results are kept, keyed by the content of their inputs"""
    import hashlib
    key = (tag,) + tuple(None if a is None else (a.shape, a.dtype.str, hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()) for a in arrays)
    if key not in _MEMO:
        if len(_MEMO) >= 8:
            _MEMO.clear()
        _MEMO[key] = make()
    return _MEMO[key]


def _need_extended():
    if not EXTENDED:
        raise NotImplementedError(REQUIRES_EXTENDED)


def _pad_index(n):
    return np.clip(np.arange(n + 2 * SPLINE_PAD) - SPLINE_PAD, 0, n - 1)


def _causal_init(c, z, zN):
    """SciPy's _init_causal_reflect, in its own (in-place) order: the last term reads the running sum as c[0]."""
    N = c.shape[0]
    acc = c[0] + zN * c[N - 1]
    zi = z
    for i in range(1, N):
        acc = acc + zi * (c[i] + zN * (c[N - 1 - i] if i < N - 1 else acc))
        zi = zi * z
    return acc * (z / (LD(1) - zN * zN)) + c[0]


def spline_coefficients(xm):
    """Cubic-spline coefficients of the lines xm (n, ...) along axis 0, padded by 12 edge samples per side -> (n + 24, ...) longdouble:
    gain, causal initialisation, causal recursion, anti-causal initialisation and recursion (ni_splines.c: apply_filter, reflect)."""
    _need_extended()
    n = xm.shape[0]
    N = n + 2 * SPLINE_PAD
    z = LD(SPLINE_POLE)
    with np.errstate(under='ignore'):
        c = _ld(xm)[_pad_index(n)] * ((LD(1) - z) * (LD(1) - LD(1) / z))
        zN = z ** N
        c[0] = _causal_init(c, z, zN)
        for i in range(1, N):
            c[i] = c[i] + z * c[i - 1]
        c[N - 1] = c[N - 1] * (z / (z - LD(1)))
        for i in range(N - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
    return c


def _coefficient_bound(am, e_in=None):
    """The running bound of spline_coefficients for lines of magnitudes am = |x| (n, ...): -> (m, e), both (n + 24, ...).
    m follows the same recursions with |z| and |x| (nothing cancels); e follows them too and collects c u m at every element:
        causal        e[i] = |z| e[i-1] + c m[i]
        anti-causal   e[i] = |z| (e[i+1] + e[i]) + c m[i]
    (+ c TINY per element for products below the normal range).  e_in: a bound the input came with (n, ...), carried along."""
    _need_extended()
    n = am.shape[0]
    N = n + 2 * SPLINE_PAD
    z = LD(SPLINE_POLE)
    az = abs(z)
    u, tiny = LD(U), LD(TINY)
    idx = _pad_index(n)
    with np.errstate(under='ignore'):
        g = abs((LD(1) - z) * (LD(1) - LD(1) / z))
        m = _ld(am)[idx] * g
        e = C_GAIN * (u * m + tiny)
        if e_in is not None:
            e = e + g * _ld(np.broadcast_to(e_in, am.shape))[idx]
        azN = az ** N
        m0 = _causal_init(m, az, azN)
        e[0] = _causal_init(e, az, azN) + c_init(N) * (u * m0 + tiny)
        m[0] = m0
        for i in range(1, N):
            m[i] = m[i] + az * m[i - 1]
            e[i] = e[i] + az * e[i - 1] + C_PASS * (u * m[i] + tiny)
        top = abs(z / (z - LD(1)))
        m2, e2 = np.empty_like(m), np.empty_like(e)
        m2[N - 1] = top * m[N - 1]
        e2[N - 1] = top * e[N - 1] + C_TOP * (u * m2[N - 1] + tiny)
        for i in range(N - 2, -1, -1):
            m2[i] = az * (m2[i + 1] + m[i])
            e2[i] = az * (e2[i + 1] + e[i]) + C_PASS * (u * m2[i] + tiny)
    return m2, e2


def _sample_points(n, d):
    """(index k, longdouble weight w, whether the weight is a computed one) of the four coefficients behind every output cell i: the
    coordinate is the FLOAT64 quantity fl(fl(i - d) + 12) that SciPy, the oracle and the device all form; everything after it is exact
    (pp - k is) or longdouble."""
    pp = (np.arange(n, dtype=np.float64) - np.float64(d)) + np.float64(SPLINE_PAD)
    fl = np.floor(pp)
    N = n + 2 * SPLINE_PAD
    out = []
    for dk in (-1, 0, 1, 2):
        a = np.abs(_ld(pp) - (_ld(fl) + LD(dk)))
        w = np.where(a < 1, LD(2) / LD(3) - a * a + a * a * a / LD(2), np.where(a < 2, (LD(2) - a) ** 3 / LD(6), LD(0)))
        k = np.clip(fl + dk, 0, N - 1).astype(np.int64)              # the coefficient index clipped to [0, N - 1]
        out.append((k, w, a < 2))
    return out


def _expand(w, ndim):
    return w.reshape((-1,) + (1,) * (ndim - 1))


def spline_shift(x, d, axis):
    """scipy.ndimage.shift(x, d along `axis`, order = 3, mode = 'nearest') in longdouble: out[i] = sum_k beta3(pp_i - k) c[clip(k, 0, N - 1)],
    pp_i = fl(fl(i - d) + 12), c = spline_coefficients of the lines along `axis`."""
    xm = _moved(x, axis)
    c = _memo('c', [xm], lambda: spline_coefficients(xm))
    out = np.zeros(xm.shape, dtype=LD)
    with np.errstate(under='ignore'):
        for k, w, _ in _sample_points(xm.shape[0], d):
            out = out + _expand(w, xm.ndim) * c[k]
    return np.moveaxis(out, 0, axis)


def _shift_err(x, d, axis, e_in=None):
    """first-order bound of the device's shift against spline_shift(x, d, axis), without SLACK: the coefficients' running bound through
    the four weights (sum_k w_k e_k), the weights' own rounding (W_OPS u m_k for every computed weight), the four fused multiply-adds and the
    product with the input scale (C_SAMPLE u sum_k w_k m_k), one TINY per product"""
    xm = _moved(x, axis)
    em = None if e_in is None else _moved(np.broadcast_to(e_in, np.shape(x)), axis)
    m, e = _memo('e', [xm, em], lambda: _coefficient_bound(np.abs(_ld(xm)), em))
    u = LD(U)
    out = np.zeros(xm.shape, dtype=LD)
    with np.errstate(under='ignore'):
        for k, w, computed in _sample_points(xm.shape[0], d):
            wk, ck = _expand(w, xm.ndim), _expand(computed.astype(LD), xm.ndim)
            out = out + wk * e[k] + (W_OPS * u * ck + C_SAMPLE * u * wk) * m[k] + LD(2 * TINY)
    return np.moveaxis(out, 0, axis)


def spline_shift_bound(x, d, axis):
    """|device shift - spline_shift(x, d, axis)| per cell: the running bound (_coefficient_bound, _shift_err) times SLACK.  Counts per
    element and pass: C_GAIN = 4, c_init(N) = 22 + 2 C for c[0], C_PASS = 20 for each recursion, C_TOP = 3, W_OPS = 6 per weight,
    C_SAMPLE = 5 -- derived above, none of them fitted to a device."""
    return SLACK * _shift_err(x, d, axis)


def shift_stage(v, e, d, axis):
    """the shift alone (no renormalisation): -> (spline_shift(v), bound)"""
    return spline_shift(v, d, axis), _shift_err(v, d, axis, e)


def normalise_stage(v, e, nblk=1):
    """v / sum(v) (transitionModels.py:603, :410, core.py:389): -> (r, bound of r, D = sum v, bound of D).  The device sums G = v.size values
    in nblk block partials: |D^ - D| <= sum e + (G + nblk) u sum |v|; the quotient (a reciprocal and a product): 2 u, one TINY."""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    G = v.size
    D = v.sum() if EXTENDED else _sum(v.reshape(-1), 0)
    eD = e.sum() + (G + nblk) * LD(U) * np.abs(v).sum()
    r = v / D
    er = e / abs(D) + np.abs(v) * eD / (D * D) + 2 * LD(U) * np.abs(r) + LD(TINY)
    return r, er, D, eD


def scale_stage(v, e, factor):
    """v * factor for a float64 factor: one product"""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    f = LD(float(factor))
    r = v * f
    return r, e * abs(f) + LD(U) * np.abs(r) + LD(TINY)


def deterministic_stage(v, e, d, axis, nblk=1):
    """Deterministic (transitionModels.py:581-583 / :600-603): the shift, then the division by the sum -> (r, bound, D, bound of D)"""
    o, eo = shift_stage(v, e, d, axis)
    return normalise_stage(o, eo, nblk)


def regime_switch_stage(v, e, limit, nblk=1):
    """RegimeSwitch (:405-412): cells below `limit` (a float64: 10^value dV, formed with pow() and a product: 2 u) are set to it, then
    the division by the sum.  Clamping does not enlarge a difference."""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    lim = LD(float(limit))
    w = np.where(v < lim, lim, v)
    return normalise_stage(w, e + 2 * LD(U) * lim, nblk)[:2]


def not_equal_stage(v, e, limit, nblk=1):
    """NotEqual (:462-471): (max - v) / (G max - sum v), then RegimeSwitch's clamp and division.  The maximum is off by at most max e; the
    denominator is formed from G max (one product) and the sum (G + nblk terms), which cancel: its bound is relative to G |max| + sum |v|,
    not to itself."""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    G, u = v.size, LD(U)
    mx, emx = v.max(), e.max()
    a = mx - v
    ea = e + emx + u * np.abs(a)
    den = a.sum()
    eden = G * emx + e.sum() + u * (2 * G * abs(mx) + (G + nblk) * np.abs(v).sum())
    r = a / den
    er = ea / abs(den) + np.abs(a) * eden / (den * den) + 2 * u * np.abs(r) + LD(TINY)
    return regime_switch_stage(r, er, limit, nblk)


def walk_stage(v, e, weights, axis):
    """GaussianRandomWalk (:107-115) as a reflect-boundary correlation with the float64 tap `weights` (odd count, centred), taken as DATA
    from the oracle's program for the same model: out[i] = sum_j w[j] v[reflect(i + j - r)].  Bound: the incoming one through the same
    weights, plus (taps + 2) u of sum_j |w_j| |v|: a product and a sum per tap, one u for a weight that the device formed itself, one spare
    for a fused order; one TINY per tap."""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    r = len(w) // 2
    assert len(w) == 2 * r + 1
    vm, em = np.moveaxis(v, axis, 0), np.moveaxis(e, axis, 0)
    n = vm.shape[0]
    out, mag, eo = (np.zeros(vm.shape, dtype=LD) for _ in range(3))
    for j in range(len(w)):
        idx = np.arange(n) + j - r
        idx = np.mod(idx, 2 * n)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)                 # half-sample symmetric: (d c b a | a b c d | d c b a)
        wj = LD(w[j])
        out = out + wj * vm[idx]
        mag = mag + abs(wj) * np.abs(vm[idx])
        eo = eo + abs(wj) * em[idx]
    eo = eo + (len(w) + 2) * LD(U) * mag + len(w) * LD(TINY)
    return np.moveaxis(out, 0, axis), np.moveaxis(eo, 0, axis)


# ---- the Gaussian likelihood and a small forward-backward pass ----------------------------------------------------------------------------
#
# Written from the reference: observationModels.py:566-567 (Gaussian.pdf: exp(-(x - mu)^2 / (2 s^2) - 0.5 log(2 pi s^2))), :49-54 (the product
# over the values of a record, a NaN value contributing 1), :705-706 (GaussianMean: the same expression with the datum's own s), and
# core.py:372-470 (the two passes).  The bounds are counted along the kernel sources (bayesloop_amd/csrc): blhip_fast.hpp / blhip_mfma.hpp /
# blhip_resident.hpp / blhip_chainres.hpp / blhip_chainax.hpp (anchor terms a0, d1, d2; blmath::exp_mn and inv_m of blhip_expmn.hpp; the
# products mE *= mR, mR *= mq) and blhip_batch.hpp (the column constants cA = 1 / (2 s s), cB = 0.5 log(2 pi s s) formed on the host).
#
# Per-cell exponential (REC = false, blk::step_kernel<2>, the GaussianMean kernels, and NumPy's evaluation in oracle/bl_oracle.py), per value:
#     q = x - mu                 1 u relative, 2 u in q q
#     q q                        1 u
#     cA = 1 / (2 s s)           2 u (the square, the reciprocal; the oracle: the square and the division)
#     (q q) cA  (or its fma)     1 u                                  -> C_ARG_A = 7 u A with the final subtraction, A = q^2 / (2 s^2)
#     cB: 2 pi s s               3 u in the argument of log = 3 u absolute, log itself 1 u |cB|, the subtraction 1 u |cB|   -> 2 u |cB| + 4 u
#     exp                        within 1 ulp = 2 u (C_EXP), one product per value.
# Recurrence (REC = true): the anchor every `rmax + 1` steps of `stride` rows; r steps later the kernel holds
#     exp(a0) exp(d1)^r exp(d2)^(r (r - 1) / 2)   as mantissa * 2^exponent,
# so the argument's error is e(a0) + r e(d1) + r (r - 1) / 2 e(d2), plus what the grid's own rounding does to the model (the true row
# coordinates are mu[0] + i step only to rounding: the anchors read the rounded ones, the second difference uses the host's step), and the
# mantissa collects C_EXPMN u per exponential it is a product of and one u per product.  Counts:
#     a0 = sum_k fma(-(q q), cA, a0) - cB     5 u A_k (q twice, q q, cA twice) + 2 u per partial sum (fma, subtraction) + cB's (3 + |cB|) u
#     s1 = sum_k (x - mu0) + (x - mu1)         (2 + dn) u sum_k (|x - mu0| + |x - mu1|)
#     d1 = cA (mu1 - mu0) s1                   cA 2 u, the difference 1 u, two products: 5 u |d1|, together (7 + dn) u cA |mu1 - mu0| sum_k (..)
#     d2 = -2 cA dn (stride step)^2            cA 2 u, four products: 6 u |d2|
#     blmath::exp_mn                           the two reduction fmas 1 u |r| each, |r| <= 0.35 (the first is exact for large |kn|: tests/test_highprec.py);
#                                              the split ln 2 = hi + lo is off by 2e-26, times |kn| <= 2.02e9: 0.4 u; thirteen Horner fmas whose
#                                              errors are damped by |r| each: 1 / (1 - 0.35) u; truncation 0.35^14 / 14! = 0.04 u   -> C_EXPMN = 3 u
#     blmath::inv_m                            v_rcp_f64 and one Newton step (two fmas)                      -> C_INVM = 2 u

C_ARG_A, C_ARG_B, C_ARG_0 = 7, 2, 4
C_EXP = 2
C_EXPMN = 3
C_INVM = 2
C_CELL = 6        # rounded products per cell and step around the likelihood: the step's (lagged) scale and its formation, the product with the
#                   likelihood, the product of the two messages, the stored normalisation
PI_LD = LD(4) * np.arctan(LD(1))
LAZY_LAG = 4      # steps a kernel's normaliser may lag behind (gaussian_fit: lazy)


class ScaleHistory:
    """The lazy() term of transition_fit (and, through it, gaussian_fit) under a NAMED scale rule (tests/scale_rules.py: 'step', 'launch(K)', 'norm_lag(lag)',
    'sum_lag(lag)'): TINY / min(1, state scale) wherever a value waits un-normalised, the state scale computed from the reference's own
    longdouble normalisers by the family's documented rule -- never from a device's output.  Three places, as in the unnamed term:
        forward_term     the product v L of step k, held at S_k / n_k (its own sum enters in normalise_stage: together TINY / S_k);
        posterior_term   the STORED forward row of step t (sums to S_t of the forward history) times the backward message (sums to the S of
                         the backward history's latest step);
        backward_term    the product beta L of the backward step, as forward_term, along the backward pass's own history.
    The backward history counts the kernels' steps k = T - 1 - t: step 0 holds the uniform message (normaliser 1).
    Leaves in out['scale'] what the rule predicts the kernels' sums to be: fwd [T] (S_k), bwd (pass order), post {t: S_t S_bwd sum(alpha_t beta_t)}."""

    def __init__(self, rule, out):
        self.rule = sr.parse_rule(rule)
        self.F, self.B = sr.History(self.rule), sr.History(self.rule)
        self.B.push(LD(1))
        self.post = {}
        out['scale'] = dict(rule=self.rule, fwd=self.F.S, bwd=self.B.S, post=self.post)

    @staticmethod
    def _term(scale):
        return LD(TINY) / min(LD(1), scale)

    def forward_term(self, fresh, clamped):
        return self._term(self.F.pre(fresh, clamped))

    def forward_done(self, N, fresh, clamped):
        self.F.push(N, fresh, clamped)

    def posterior_term(self, t):
        return LD(TINY) / (min(LD(1), self.F.S[t]) * min(LD(1), self.B.last()))

    def posterior_done(self, t, D):
        self.post[t] = self.F.S[t] * self.B.last() * D

    def backward_term(self, fresh, clamped):
        return self._term(self.B.pre(fresh, clamped))

    def backward_done(self, Bt, fresh, clamped):
        self.B.push(Bt, fresh, clamped)


def _values(record):
    return [float(x) for x in np.asarray(record, dtype=np.float64).reshape(-1) if x == x]


def gaussian_terms(mu, s, record):
    """Per non-NaN value of the record: (A_k, arg_k) on the grid (n0, n1) in longdouble, A_k = (x_k - mu)^2 / (2 s^2), arg_k = -A_k - cB;
    and cA = 1 / (2 s^2), cB = 0.5 log(2 pi s^2), both (1, n1)."""
    mu = _ld(mu).reshape(-1, 1)
    s = _ld(s).reshape(1, -1)
    cA = LD(1) / (LD(2) * s * s)
    cB = LD(0.5) * np.log(LD(2) * PI_LD * s * s)
    out = []
    for x in _values(record):
        q = LD(x) - mu
        A = q * q * cA
        out.append((A, -A - cB))
    return out, cA, cB


def gaussian_likelihood(mu, s, record):
    """prod over the non-NaN values x of exp(-(x - mu)^2 / (2 s^2) - 0.5 log(2 pi s^2)) on the grid mu (n0) x s (n1); all NaN: 1."""
    terms, _, _ = gaussian_terms(mu, s, record)
    L = np.ones((np.size(mu), np.size(s)), dtype=LD)
    with np.errstate(under='ignore'):
        for _, arg in terms:
            L = L * np.exp(arg)
    return L


def gaussian_mean_likelihood(mu, x, s):
    """GaussianMean (:705-706): the datum (x, s) on the grid of means; a NaN in either: 1."""
    if not (x == x and s == s):
        return np.ones(np.size(mu), dtype=LD)
    return gaussian_likelihood(mu, [s], [x])[:, 0]


def likelihood_bound_exp(mu, s, record, split=False, extra=0):
    """|L^ - L| per cell for the per-value exponential (no SLACK): L sum_k (7 A_k + 2 |cB| + 4 + C_EXP + 1 + extra) u, and the subnormal step of
    every factor through the other factors (which exceed 1 where s is small) and of every product.  split: the two parts separately."""
    terms, _, cB = gaussian_terms(mu, s, record)
    shape = (np.size(mu), np.size(s))
    if not terms:
        return (np.zeros(shape, dtype=LD),) * 2 if split else np.zeros(shape, dtype=LD)
    u, tiny = LD(U), LD(TINY)
    with np.errstate(under='ignore', over='ignore'):
        Ls = [np.exp(arg) for _, arg in terms]
        rel = np.zeros(shape, dtype=LD)
        for A, _ in terms:
            rel = rel + (C_ARG_A * A + C_ARG_B * np.abs(cB) + C_ARG_0 + C_EXP + 1 + extra) * u
        L = np.ones(shape, dtype=LD)
        for f in Ls:
            L = L * f
        sub = np.full(shape, tiny * len(Ls), dtype=LD)
        for k in range(len(Ls)):
            others = np.ones(shape, dtype=LD)
            for j in range(len(Ls)):
                if j != k:
                    others = others * Ls[j]
            sub = sub + tiny * others
        with np.errstate(invalid='ignore'):
            rel = np.where(L == 0, LD(0), L * np.expm1(np.minimum(rel, LD(11000))))
        return (rel, sub) if split else rel + sub


def host_step(mu):
    """the row step the host hands the recurrence kernels: (mu[n - 1] - mu[0]) / (n - 1) in float64 (blhip.hip, FP.step0)"""
    mu = np.asarray(mu, dtype=np.float64)
    return float((mu[-1] - mu[0]) / np.float64(len(mu) - 1))


def likelihood_bound_rec(mu, s, record, stride, rmax, dirs=(1,), split=False):
    """|L^ - L| per cell for the recurrence (no SLACK): a cell r <= rmax steps of `stride` rows behind its anchor (in a direction of `dirs`:
    +1 the anchor has the lower row index) -- the bound is the largest over these anchor positions, which covers every tiling."""
    xs = _values(record)
    shape = (np.size(mu), np.size(s))
    if not xs:
        return (np.zeros(shape, dtype=LD),) * 2 if split else np.zeros(shape, dtype=LD)
    dn = len(xs)
    u = LD(U)
    _, cA, cB = gaussian_terms(mu, s, [])
    mu_i = _ld(mu).reshape(-1, 1)
    step = LD(host_step(mu))
    lam = _ld(mu)[0] + np.arange(np.size(mu)).astype(LD) * step
    delta = np.max(np.abs(_ld(mu) - lam))                              # how far the rounded row coordinates are from the lattice
    H = LD(stride) * abs(step)
    S1_i = sum(np.abs(LD(x) - mu_i) for x in xs)
    worst_e = np.zeros(shape, dtype=LD)
    with np.errstate(under='ignore', over='ignore'):
        for dr in dirs:
            for r in range(rmax + 1):
                nu = mu_i - LD(dr * r) * H
                A_nu = sum((LD(x) - nu) ** 2 for x in xs) * cA
                S1_nu = sum(np.abs(LD(x) - nu) for x in xs)
                S1_nu1 = sum(np.abs(LD(x) - (nu + LD(dr) * H)) for x in xs)
                ea0 = u * ((5 + 2 * dn) * A_nu + dn * (3 + (1 + 2 * dn) * np.abs(cB)))
                ed1 = u * (7 + dn) * cA * H * (S1_nu + S1_nu1)
                ed2 = 6 * u * 2 * cA * dn * H * H
                egrid = 2 * cA * delta * (S1_nu * (1 + 2 * r) + r * dn * H + S1_i)
                tri = r * (r - 1) // 2
                e = ea0 + r * ed1 + tri * ed2 + egrid + u * (C_EXPMN * (1 + r + tri) + r + tri)
                worst_e = np.maximum(worst_e, e)
        L = gaussian_likelihood(mu, s, record)
        with np.errstate(invalid='ignore'):
            rel = np.where(L == 0, LD(0), L * np.expm1(np.minimum(worst_e + (C_INVM + 1) * u, LD(11000))))      # (0 stays 0 whatever the argument's error)
        return (rel, np.full(shape, LD(TINY), dtype=LD)) if split else rel + LD(TINY)


def product_stage(a, ea, b, eb, ops=C_CELL):
    """a * b for two quantities that come with bounds: -> (r, bound): first order in both, `ops` rounded operations, one TINY"""
    a, b = _ld(a), _ld(b)
    ea = np.zeros(a.shape, dtype=LD) if ea is None else _ld(np.broadcast_to(ea, a.shape))
    eb = np.zeros(b.shape, dtype=LD) if eb is None else _ld(np.broadcast_to(eb, b.shape))
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        r = a * b
        e = ea * np.abs(b) + np.abs(a) * eb + ea * eb + ops * LD(U) * np.abs(r) + LD(TINY)
    return r, e


def gaussian_fit(prior, liks, walks, grids, lattice, nblk=1, full=True, clamp=None, scale=None):
    """core.py:372-470 in longdouble with a running bound.  prior (n0, n1) float64 (taken as given); liks: per step (L, bound of L); walks:
    [(axis, float64 taps)] applied in list order between steps, in both directions (transitionModels.py:107-118); grids: the two marginal
    grids; lattice: the lattice constants; clamp: log10 pMin of a RegimeSwitch behind the walks (:405-412), or None.  -> dict of (value, bound) pairs, bounds WITHOUT SLACK:
        'alpha' [T] normalised forward states, 'norm' [T], 'local_fwd' [T] (norm dV), 'log_evidence',
        full: 'post' [T], 'local' [T] (1 / (sum(post / L) dV); value NaN where a likelihood rounds to 0 in float64), 'means' [T] of (2,)
        forward-only: 'means' from alpha.
    scale: None -- the unnamed lazy() term below --, or the family's scale rule (tests/scale_rules.py): the pass is then transition_fit's, over the one
    program (the walks, then the clamp) for every step, with its term from the rule's state scale, its projective bound and out['scale']."""
    _need_extended()
    T = len(liks)
    if scale is not None:
        dV0 = float(np.prod(np.asarray(lattice, dtype=np.float64)))
        prog = ('prev', [('walk', axis, taps) for axis, taps in walks] + ([('rs', float(10.0 ** clamp * dV0))] if clamp is not None else []))
        return transition_fit(prior, liks, [dict(fwd=prog, bwd=prog)] * T, grids, lattice, nblk=nblk, full=full, scale=scale)
    dV = LD(float(np.prod(np.asarray(lattice, dtype=np.float64))))
    u = LD(U)
    g = [_ld(_grid_values(grids, k, np.shape(prior))) for k in range(2)]
    G = int(np.size(prior))
    out = dict(alpha=[], norm=[], local_fwd=[], post=[], local=[], means=[])

    def transition(v, e):
        for axis, taps in walks:
            v, e = walk_stage(v, e, taps, axis)
        if clamp is not None:
            v, e = regime_switch_stage(v, e, float(10.0 ** clamp * float(dV)), nblk)
        return v, e

    def means_of(p, ep):
        m, em = [], []
        with np.errstate(under='ignore'):
            for k in range(2):
                m.append((p * g[k]).sum())
                em.append((ep * np.abs(g[k])).sum() + (G + 3) * u * (np.abs(p) * np.abs(g[k])).sum())
        return np.array(m, dtype=LD), np.array(em, dtype=LD)

    def lazy(norms):
        """>= 1: what a subnormal step of a kernel's UNNORMALISED state grows by until the row is normalised.  The kernels normalise lazily:
        a stored state is scaled by sums up to MAXLAG = 4 steps old (blr::MAXLAG, blc::MAXLAG; the launch-per-step kernels: 1), so it sums to
        the product of the last 1 .. 4 normalisers, not to 1 -- `norms`: those normalisers, latest first"""
        worst_p, prod = LD(1), LD(1)
        for N in norms[:LAZY_LAG]:
            prod = prod * N
            worst_p = min(worst_p, prod)
        return LD(1) / worst_p

    v, e = _ld(prior), None
    logE, elogE = LD(0), LD(0)
    Ns = []
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        for t in range(T):
            if t > 0:
                v, e = transition(v, e)
            a, ea = product_stage(v, e, liks[t][0], liks[t][1])
            ea = ea + LD(TINY) * lazy(Ns[::-1][:LAZY_LAG - 1])            # (the division by this step's own sum follows in normalise_stage)
            r, er, N, eN = normalise_stage(a, ea, nblk)
            Ns.append(N)
            out['alpha'].append((r, er))
            out['norm'].append((N, eN))
            out['local_fwd'].append((N * dV, eN * dV + 2 * u * N * dV))
            logE = logE + np.log(N)
            elogE = elogE + eN / N + 2 * u * (abs(np.log(N)) + abs(logE))
            v, e = r, er
        logE = logE + np.log(dV)
        out['log_evidence'] = (logE, elogE + 2 * u * abs(logE))
        if not full:
            out['means'] = [means_of(r, er) for r, er in out['alpha']]
            return out
        beta, eb = np.full(np.shape(prior), LD(1) / LD(G), dtype=LD), np.full(np.shape(prior), u / LD(G), dtype=LD)
        post, local, means = [None] * T, [None] * T, [None] * T
        Bs = []                                                              # the backward normalisers, latest (lowest t) last
        for t in range(T - 1, -1, -1):
            L, eL = _ld(liks[t][0]), _ld(liks[t][1])
            p, ep = product_stage(out['alpha'][t][0], out['alpha'][t][1], beta, eb)
            # the kernels multiply the STORED forward state (sums to a product of normalisers) by the lazily scaled backward message
            ep = ep + LD(TINY) * lazy(Ns[:t + 1][::-1]) * lazy(Bs[::-1])
            p, ep = normalise_stage(p, ep, nblk)[:2]
            post[t] = (p, ep)
            means[t] = means_of(p, ep)
            if np.any(L.astype(np.float64) == 0.0):
                local[t] = (LD(np.nan), LD(0))                           # 0 / 0 in a cell (core.py:463): the sum is NaN
            else:
                q = p / L
                relL = np.where(L > eL, eL / (L - eL), LD(np.inf))
                eq = ep / L + q * relL + 2 * u * q + LD(TINY)
                S = q.sum()
                eS = eq.sum() + (G + nblk) * u * S
                val = LD(1) / (S * dV)
                local[t] = (val, val * (eS / (S - eS) + 3 * u) + LD(TINY) if S > eS else LD(np.inf))
            b, ebl = product_stage(beta, eb, L, eL)
            ebl = ebl + LD(TINY) * lazy(Bs[::-1][:LAZY_LAG - 1])
            b, ebl = transition(b, ebl)
            beta, eb, Bt = normalise_stage(b, ebl, nblk)[:3]
            Bs.append(Bt)
        out['post'], out['local'], out['means'] = post, local, means
    return out


# ---- the host's tap tables and the transition half of the fused step kernels -----------------------------------------------------------------
#
# Written from the reference: scipy/ndimage/_filters.py (_gaussian_kernel1d: lw = int(4 sd + 0.5), exp(-0.5 / sd^2 x^2) / sum) behind
# transitionModels.py:107-115; :196-240 (AlphaStableRandomWalk.createKernel: numpy.fft.irfft of exp(-|c w|^alpha) on int(3 n / 2 + 1) points of
# [0, pi]) with :242-260 (the 3x zero-padded fftconvolve, 'same': out[i] = sum_j in[j] k[|i - j|] inside the grid); :898-911
# (BivariateRandomWalk.createKernel; the density's constant cancels in :910) with :892-893 (scipy.signal.convolve2d, 'same', zero fill, and the
# division by the sum); :559-606 (Deterministic: scipy.ndimage.shift, order 3, 'nearest') -- not from the kernels or the host's builders.
# The bounds count the float64 operations of a builder that evaluates these formulas as written (one rounding per operation; pow() within
# 2 ulp = 4 u as above, exp() and cos() within 1 ulp = 2 u).  Every function returns (weights in longdouble, bound of a float64 builder).

C_POW = 4
C_COS = 2
C_POLE = 7        # sqrt(3) - 2 formed in float64: the root within u (1.74 u absolutely), the subtraction exact: 6.5 u of 0.268
C_ETA_GAIN = 11   # g formed in float64 as -6 z / (1 - z^2): z (7), the square (1), 1 - z^2 (the 15 u of z^2 = 0.072 and its own u, over 0.928: 3), -6 z (1), the quotient (1):
#                   the pole's error enters numerator and denominator with the same sign and mostly cancels; counted as if it did not
SHIFT_STENCIL_MAX = 12      # |d| up to which the fused step kernels take the one-pass stencil
SHIFT_STENCIL_REACH = 34    # ... of radius ceil|d| + 34


def gaussian_walk_taps(ns):
    """SciPy's gaussian_filter1d weights for sigma = ns cells -> (r, w (2 r + 1), bound).  Float64 count per weight: the argument
    0.5 / (ns ns) k^2 = a: the square, the quotient, the product (3 u a); exp (2 u): phi_k (1 + (3 a_k + 2) u); the sum of 2 r + 1 positive terms
    ((2 r + 1) u, and the terms' own errors as their weighted mean); the quotient (1 u)."""
    ns = float(ns)
    r = int(4.0 * ns + 0.5)
    x = _ld(np.arange(-r, r + 1))
    with np.errstate(under='ignore'):
        a = LD(0.5) / (LD(ns) * LD(ns)) * x * x
        phi = np.exp(-a)
        w = phi / phi.sum()
        rel = 3 * a + C_EXP
        e = w * LD(U) * (rel + (w * rel).sum() + (2 * r + 1) + 1)
    return r, w, e


def alphastable_taps(c, alpha, n):
    """createKernel (transitionModels.py:196-240) for an axis of n points, c in cells -> (k[0 .. n-1], bound): the inverse real DFT as the
    exact cosine sum  k[j] = (X_0 + (-1)^j X_(m-1) + 2 sum_(q = 1)^(m-2) X_q cos(2 pi j q / K)) / K,  X_q = exp(-|c pi q / (m - 1)|^alpha),
    m = int(3 n / 2 + 1), K = 2 (m - 1) (numpy.fft.irfft's definition; j q is reduced modulo K in integers).  Float64 count: the argument
    c pi q / (m - 1) (pi, two products, a quotient: 4 u), pow (alpha times that and its own 4 u), exp (the argument's absolute error and 2 u):
    X_q (1 + ((4 alpha + 4) p_q + 2) u); a term 2 X_q cos: the cosine (2 u), the product (1 u); the m - 1 additions against
    sum |X| / K = (X_0 + X_(m-1) + 2 sum X_q) / K; the last quotient (1 u)."""
    c, alpha, n = float(c), float(alpha), int(n)
    m = int(3 * n / 2 + 1)
    K = 2 * (m - 1)
    q = np.arange(m)
    u = LD(U)
    with np.errstate(under='ignore'):
        p = np.abs(LD(c) * PI_LD * _ld(q) / LD(m - 1)) ** LD(alpha)
        X = np.exp(-p)
        eX = X * ((4 * alpha + C_POW) * p + C_EXP) * u
        jq = (np.arange(n, dtype=np.int64)[:, None] * q[None, 1:m - 1].astype(np.int64)) % K
        cosm = np.cos(LD(2) * PI_LD * _ld(jq) / LD(K))
        sign = np.where(np.arange(n) % 2 == 1, LD(-1), LD(1))
        k = (X[0] + sign * X[m - 1] + LD(2) * (cosm * X[None, 1:m - 1]).sum(axis=1)) / LD(K)
        S = X[0] + X[m - 1] + LD(2) * X[1:m - 1].sum()
        e = (eX[0] + eX[m - 1] + LD(2) * (np.abs(cosm) * eX[None, 1:m - 1]).sum(axis=1) + (C_COS + 1 + (m - 1)) * u * S) / LD(K) + u * np.abs(k)
    return k, e


def bivariate_taps(ns1, ns2, rho):
    """createKernel (transitionModels.py:898-911), sigmas in cells -> (kernel (2 r0 + 1, 2 r1 + 1), bound), r = 3 ceil(ns): exp(-q) / sum,
    q = (x^2 / ns1^2 - 2 rho x y / (ns1 ns2) + y^2 / ns2^2) / (2 (1 - rho^2)).  Float64 count: each of the three terms at most 4 u (a square or the
    products with rho, x and y; the product of the sigmas; the quotient), their two additions 2 u of the sum of their magnitudes A D; the
    denominator D = 2 (1 - rho^2): rho^2 (1 u) and the subtraction, relative to 1 - rho^2: (1 + rho^2) / (1 - rho^2) u; the quotient 1 u.
    So |dq| <= (7 + (1 + rho^2) / (1 - rho^2)) u A with A = (|T1| + |T2| + |T3|) / D >= |q|; exp 2 u; the sum of all taps; the quotient."""
    ns1, ns2, rho = float(ns1), float(ns2), float(rho)
    r0, r1 = 3 * int(math.ceil(ns1)), 3 * int(math.ceil(ns2))
    x = _ld(np.arange(-r0, r0 + 1))[:, None]
    y = _ld(np.arange(-r1, r1 + 1))[None, :]
    s1, s2, rh = LD(ns1), LD(ns2), LD(rho)
    with np.errstate(under='ignore'):
        T1, T2, T3 = x * x / (s1 * s1), LD(2) * rh * x * y / (s1 * s2), y * y / (s2 * s2)
        D = LD(2) * (LD(1) - rh * rh)
        qv = (T1 - T2 + T3) / D
        A = (np.abs(T1) + np.abs(T2) + np.abs(T3)) / D
        v = np.exp(-qv)
        w = v / v.sum()
        rel = (7 + (1 + rh * rh) / (1 - rh * rh)) * A + C_EXP
        e = w * LD(U) * (rel + (w * rel).sum() + w.size + 1)
    return w, e


def _beta3(a):
    a = np.abs(a)
    return np.where(a < 1, LD(2) / LD(3) - a * a + a * a * a / LD(2), np.where(a < 2, (LD(2) - a) ** 3 / LD(6), LD(0)))


def _beta3_slope(a):
    """|d beta3 / du| at |u| = a"""
    a = np.abs(a)
    return np.where(a < 1, np.abs(LD(1.5) * a * a - LD(2) * a), np.where(a < 2, (LD(2) - a) ** 2 / LD(2), LD(0)))


def cardinal_spline(uu, with_bound=False):
    """eta(u) = sum_n g z^|n| beta3(u - n), g = (1 - z) / (1 + z), z = SciPy's pole: the cubic CARDINAL spline -- the response of SciPy's
    prefilter (ni_splines.c: the gain (1 - z)(1 - 1 / z), then y[i] = x[i] + z y[i-1] and c[i] = z (c[i+1] - y[i]): together the two-sided sequence
    g z^|n|; g = sqrt(3) = -6 z / (1 - z^2) for the exact pole sqrt(3) - 2, to 1e-17 for SciPy's literal) sampled by the B-spline (:581:
    scipy.ndimage.shift, order 3).  Four terms are not zero: n = floor(u) - 1 .. + 2.
    with_bound: also (bound of a float64 evaluation WITHOUT the rounding of u, sum_n g |z|^|n| |beta3'(u - n)|): per term the gain (C_ETA_GAIN),
    z^|n| from pow() on a pole that is itself off by C_POLE u (C_POLE |n| + 4), two products, and the weight's W_OPS u absolutely; three
    additions against the sum of the magnitudes."""
    uu = _ld(uu)
    z = LD(SPLINE_POLE)
    g = (LD(1) - z) / (LD(1) + z)         # SciPy's gain (1 - z)(1 - 1 / z) times the response -z / (1 - z^2) of its two recursions
    n0 = np.floor(uu)
    val, err, slope = (np.zeros(uu.shape, dtype=LD) for _ in range(3))
    with np.errstate(under='ignore'):
        for k in (-1, 0, 1, 2):
            n = n0 + k
            zn = g * z ** np.abs(n)
            b = _beta3(uu - n)
            val = val + zn * b
            err = err + np.abs(zn) * ((C_ETA_GAIN + C_POLE * np.abs(n) + C_POW + 2 + 3) * b + W_OPS) * LD(U)
            slope = slope + np.abs(zn) * _beta3_slope(uu - n)
    return (val, err, slope) if with_bound else val


def shift_stencil_radius(d):
    return int(math.ceil(abs(float(d)))) + SHIFT_STENCIL_REACH


def small_shift_taps(d, r=None):
    """The shift by d cells as ONE stencil over the extension SciPy works on: out[i] = sum_m K[m] ext[i + m], K[m] = eta(-d - m), for every
    integer m (untruncated: exact for |d| <= 12, where no sample reads beyond the coefficients SciPy has) -> (K[-r .. r], bound, slope); r: default
    the radius ceil|d| + 34 the fused step kernels cut it at.  The bound is cardinal_spline's plus the rounding of the float64 argument -d - m
    through the slope (the exact difference, not an estimate)."""
    d = float(d)
    r = shift_stencil_radius(d) if r is None else int(r)
    m = np.arange(-r, r + 1)
    u64 = -np.float64(d) - m.astype(np.float64)
    exact = -LD(d) - _ld(m)
    K, e, slope = cardinal_spline(exact, with_bound=True)
    e = e + np.abs(_ld(u64) - exact) * slope
    return K, e, slope


def shift_tail(d, r=None, more=400):
    """tail(d) = sum over |m| > r of |eta(-d - m)|: what a stencil cut at radius r (default ceil|d| + 34) leaves out, per unit of the line's
    maximum.  Summed over the next `more` = 400 cells on either side; what lies beyond is below |z|^400 = 1e-229 of it."""
    d = float(d)
    r = shift_stencil_radius(d) if r is None else int(r)
    m = np.concatenate([np.arange(-r - more, -r), np.arange(r + 1, r + more + 1)])
    with np.errstate(under='ignore'):
        return np.abs(cardinal_spline(-LD(d) - _ld(m))).sum()


def spline_extension_index(n, idx):
    """the sample behind position idx (any integer) of the line SciPy's shift works on (_interpolation.py: _prepad_for_spline_filter, mode
    'nearest': 12 edge samples per side; ni_splines.c: the prefilter's half-sample symmetric boundary, period 2 (n + 24))"""
    N = n + 2 * SPLINE_PAD
    j = np.mod(np.asarray(idx) + SPLINE_PAD, 2 * N)
    j = np.where(j >= N, 2 * N - 1 - j, j)
    return np.clip(j - SPLINE_PAD, 0, n - 1)


def small_shift_stage(v, e, d, axis):
    """The shift alone for |d| <= 12 as the fused step kernels take it (no renormalisation): the VALUE is spline_shift (SciPy's algorithm); the
    bound is that of the one-pass stencil of radius lw = ceil|d| + 34:
        incoming bound through |K|;  2 lw + 1 fused multiply-adds over sum_m |K_m| |ext|;  the weights' bound (small_shift_taps) over |ext|;
        the rounding of the reference's OWN float64 coordinate fl(fl(i - d) + 12) (_sample_points) against i - d + 12, exactly, through the slope;
        the truncation tail(d) max |line|, absolute in the line's maximum: the stencil is a finite one by design;  one TINY per tap;
    and per cell at least the recursion's own bound (below)."""
    d = float(d)
    assert abs(d) <= SHIFT_STENCIL_MAX
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    out = spline_shift(v, d, axis)
    lw = shift_stencil_radius(d)
    K, eK, slope = small_shift_taps(d, lw)
    vm, em = np.abs(np.moveaxis(v, axis, 0)), np.moveaxis(e, axis, 0)
    n = vm.shape[0]
    i = np.arange(n)
    pp = (i.astype(np.float64) - np.float64(d)) + np.float64(SPLINE_PAD)
    dpp = np.abs(_ld(pp) - (_ld(i) - LD(d) + LD(SPLINE_PAD)))
    dpp = dpp.reshape((-1,) + (1,) * (vm.ndim - 1))
    mag, eo, sl = (np.zeros(vm.shape, dtype=LD) for _ in range(3))
    with np.errstate(under='ignore'):
        for j, m in enumerate(range(-lw, lw + 1)):
            idx = spline_extension_index(n, i + m)
            mag = mag + np.abs(K[j]) * vm[idx]
            eo = eo + np.abs(K[j]) * em[idx] + eK[j] * vm[idx]
            sl = sl + slope[j] * vm[idx]
        eo = eo + (2 * lw + 1) * LD(U) * mag + dpp * sl + shift_tail(d, lw) * vm.max(axis=0, keepdims=True) + (2 * lw + 1) * LD(TINY)
    # The reference evaluates the same function by the recursion, whose own counted bound (_shift_err) exceeds the stencil's where an integer
    # shift leaves nothing but the weights' rounding far from any mass.  A cell is held to the larger of the two counts, so that the float64
    # reference itself stays inside (tests/test_highprec.py runs it on every problem).  Where the second count wins: at d = +-12 (the only
    # integer shifts of the tables) on the single-cell and edge inputs, in cells k >= 20 cells from the nearest mass, where the reference's
    # value is about |z|^k of that mass (1e-12 .. 1e-38 of the line's maximum) and the recursion's count about 20 u |z|^k of it against the
    # stencil's 40 u |z|^(k + 34); at a fractional shift the truncation term, 1e-21 of the line's maximum, is the larger one in every such
    # cell, and within reach of any mass the stencil's 2 lw + 1 operations are.  It never widens the bound of a cell that holds mass.
    return out, np.maximum(np.moveaxis(eo, 0, axis), _shift_err(v, d, axis, e))


def zero_boundary_stage(v, e, weights, axis, ew=None):
    """AlphaStableRandomWalk's convolution (transitionModels.py:242-260) without its renormalisation: out[i] = sum_j v[j] k[|i - j|] inside the
    grid, nothing outside; weights: k[0 .. n-1] (float64 or longdouble), ew: their bound.  Bound as walk_stage's: n taps."""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    k = _ld(weights).reshape(-1)
    ek = np.zeros(k.shape, dtype=LD) if ew is None else _ld(ew).reshape(-1)
    vm, em = np.moveaxis(v, axis, 0), np.moveaxis(e, axis, 0)
    n = vm.shape[0]
    assert len(k) >= n
    out, mag, eo = (np.zeros(vm.shape, dtype=LD) for _ in range(3))
    i = np.arange(n)
    with np.errstate(under='ignore'):
        for j in range(n):
            kj, ekj = _expand(k[np.abs(i - j)], vm.ndim), _expand(ek[np.abs(i - j)], vm.ndim)
            out = out + kj * vm[j]
            mag = mag + np.abs(kj) * np.abs(vm[j])
            eo = eo + np.abs(kj) * em[j] + ekj * np.abs(vm[j])
        eo = eo + (n + 2) * LD(U) * mag + n * LD(TINY)
    return np.moveaxis(out, 0, axis), np.moveaxis(eo, 0, axis)


def dense_stage(v, e, kernel, ew=None):
    """scipy.signal.convolve2d(v, kernel, mode = 'same') with zero fill (transitionModels.py:892) without the renormalisation:
    out[i, j] = sum_(a, b) kernel[a, b] v[i - (a - r0), j - (b - r1)].  (The reference's kernels are point symmetric: the correlation is the same.)"""
    v = _ld(v)
    e = np.zeros(v.shape, dtype=LD) if e is None else _ld(np.broadcast_to(e, v.shape))
    k = _ld(kernel)
    ek = np.zeros(k.shape, dtype=LD) if ew is None else _ld(ew)
    r0, r1 = k.shape[0] // 2, k.shape[1] // 2
    assert k.shape == (2 * r0 + 1, 2 * r1 + 1)
    n0, n1 = v.shape
    pv, pe = (np.zeros((n0 + 2 * r0, n1 + 2 * r1), dtype=LD) for _ in range(2))
    pv[r0:r0 + n0, r1:r1 + n1], pe[r0:r0 + n0, r1:r1 + n1] = v, e
    out, mag, eo = (np.zeros(v.shape, dtype=LD) for _ in range(3))
    with np.errstate(under='ignore'):
        for a in range(k.shape[0]):
            for b in range(k.shape[1]):
                sv = pv[2 * r0 - a:2 * r0 - a + n0, 2 * r1 - b:2 * r1 - b + n1]
                out = out + k[a, b] * sv
                mag = mag + np.abs(k[a, b]) * np.abs(sv)
                eo = eo + np.abs(k[a, b]) * pe[2 * r0 - a:2 * r0 - a + n0, 2 * r1 - b:2 * r1 - b + n1] + ek[a, b] * np.abs(sv)
        eo = eo + (k.size + 2) * LD(U) * mag + k.size * LD(TINY)
    return out, eo


def apply_stage(st, v, e, nblk=1, sums=None):
    """one stage of a transition -> (v, e).  ('walk', axis, w, ew) reflecting correlation (:107-115); ('zero', axis, k, ek) and
    ('dense', K, eK) with the division by the sum (:183-185, :892-893); ('shift', axis, d) Deterministic with the division by the sum
    (:600-603): |d| <= 12 the one-pass stencil, beyond it SciPy's recursion over the whole line (shift_stage: the 1-D kernels), 0 the identity; ('rs', limit); ('ne', limit).
    sums: a list that receives (D, bound of D) of every renormalising sum of a shift, a zero-boundary or a dense stage."""
    kind = st[0]
    if kind == 'walk':
        o, eo = walk_stage(v, e, np.asarray(st[2], dtype=np.float64), st[1])
        if len(st) > 3 and st[3] is not None:       # the weights' own bound, through the same reflecting sum of |v| (rounded UP to float64)
            ew = np.nextafter(np.asarray(st[3], dtype=np.float64), np.inf)
            eo = eo + walk_stage(np.abs(_ld(v)), None, ew, st[1])[0]
        return o, eo
    if kind == 'rs':
        return regime_switch_stage(v, e, st[1], nblk)
    if kind == 'ne':
        return not_equal_stage(v, e, st[1], nblk)
    if kind == 'zero':
        o, eo = zero_boundary_stage(v, e, st[2], st[1], st[3] if len(st) > 3 else None)
    elif kind == 'dense':
        o, eo = dense_stage(v, e, st[1], st[2] if len(st) > 2 else None)
    elif kind == 'shift':
        if float(st[2]) == 0.0:
            return _ld(v), (np.zeros(np.shape(v), dtype=LD) if e is None else e)
        o, eo = (small_shift_stage if abs(float(st[2])) <= SHIFT_STENCIL_MAX else shift_stage)(v, e, st[2], st[1])
    else:
        raise ValueError(kind)
    r, er, D, eD = normalise_stage(o, eo, nblk)
    if sums is not None:
        sums.append((D, eD))
    return r, er


def _proj(eps):
    """the projective (Hilbert) distance log(max x^/x) - log(min x^/x) that a relative perturbation of up to eps per cell can open:
    log((1 + eps) / (1 - eps)); unbounded from eps = 1"""
    eps = LD(eps)
    return np.log1p(eps) - np.log1p(-eps) if eps < 1 else LD(np.inf)


def _rel(own, value):
    """max over the occupied cells of own / |value|.  A cell that is exactly 0 here is exactly 0 in a float64 evaluation too (sums and products
    of zeros under positive weights and likelihoods), so it opens no distance."""
    value = np.abs(_ld(value))
    own = _ld(np.broadcast_to(own, value.shape))
    m = value > 0
    return np.max(own[m] / value[m]) if m.any() else LD(0)


def _stage_distance(st, vin, vout):
    """what one stage adds to the projective distance between the device's state and the reference's, or inf where the stage is not a positive
    linear map (then only the running bound holds).  A walk with positive taps on a non-negative state is one (Birkhoff: it does not expand the
    distance); its float64 evaluation perturbs every output relatively by (taps + 2) u, by the taps' own relative bound, and by a subnormal
    step per tap."""
    if st[0] != 'walk':
        return LD(np.inf)
    w = _ld(np.asarray(st[2], dtype=np.float64).reshape(-1))
    if not (np.all(w > 0) and np.all(_ld(vin) >= 0)):
        return LD(np.inf)
    ew = LD(0) if len(st) <= 3 or st[3] is None else np.max(_ld(np.nextafter(np.asarray(st[3], dtype=np.float64), np.inf)).reshape(-1) / w)
    return _proj((len(w) + 2) * LD(U) + ew + _rel(len(w) * LD(TINY), vout))


def transition_fit(prior, liks, steps, grids, lattice, nblk=1, full=True, shared=None, scale=None):
    """core.py:372-470 in longdouble with a running bound, over a per-step stage program (gaussian_fit with one walk list for every step is the
    special case).  prior float64 on the grid (any number of parameters: every stage works along an axis moved to the front); liks: per step (L, bound of L); steps: per step t a dict
        fwd: (source, stages) of the transition INTO step t from t - 1 (unused for t = 0), bwd: the same INTO step t from t + 1 (unused for T - 1)
    source: 'prev' (the neighbour's state), 'reset' / 'indep' (shared[source], float64, as given: transitionModels.py:300-312, :351-360);
    stages: apply_stage's, in list order (:645-649).  -> the dict of gaussian_fit: (value, bound) pairs, bounds WITHOUT SLACK; and 'sums': (D, bound of D) of every renormalising
    sum of a shift, zero-boundary or dense stage, in the order of the pass.  scale: as gaussian_fit's; a step whose source is not 'prev' is a restart."""
    _need_extended()
    T = len(liks)
    dV = LD(float(np.prod(np.asarray(lattice, dtype=np.float64))))
    u = LD(U)
    nd = len(grids)
    g = [_ld(_grid_values(grids, k, np.shape(prior))) for k in range(nd)]
    G = int(np.size(prior))
    shared = shared or {}
    liks = [(L, np.zeros(np.shape(L), dtype=LD) if eL is None else eL) for L, eL in liks]
    out = dict(alpha=[], norm=[], local_fwd=[], post=[], local=[], means=[], sums=[])

    def transition(prog, v, e, d=None):
        """-> (v, e, d): d (only under a named scale rule) is the projective distance of the state, see tighten()"""
        source, stages = prog
        if source != 'prev':
            v, e, d = _ld(shared[source]), None, (None if d is None else LD(0))
        for st in stages:
            vin = v
            v, e = apply_stage(st, v, e, nblk, out['sums'])
            if d is not None:
                d = d + _stage_distance(st, vin, v)
        return v, e, d

    def tighten(r, er, d):
        """Under a named scale rule the running bound is joined by a second one, and a cell takes the smaller.  The running bound treats the error
        of every cell as free in sign, and the division by the sum then doubles a relative error at every step (2^13 behind 14 steps) although a
        common factor cancels there.  In the projective metric a positive linear map does not expand, a product with a positive likelihood and
        the division by the sum are isometries and the distances of two factors add: the distance d only collects what each step's OWN rounded
        operations open, and a normalised state is off by at most r (exp(d) - 1) per cell."""
        return er if not np.isfinite(d) else np.minimum(er, np.abs(r) * np.expm1(d))

    def means_of(p, ep):
        m, em = [], []
        with np.errstate(under='ignore'):
            for k in range(nd):
                m.append((p * g[k]).sum())
                em.append((ep * np.abs(g[k])).sum() + (G + 3) * u * (np.abs(p) * np.abs(g[k])).sum())
        return np.array(m, dtype=LD), np.array(em, dtype=LD)

    def lazy(norms):
        worst_p, prod = LD(1), LD(1)
        for N in norms[:LAZY_LAG]:
            prod = prod * N
            worst_p = min(worst_p, prod)
        return LD(1) / worst_p

    sh = None if scale is None else ScaleHistory(scale, out)

    def clamped(prog):
        """a step whose program clamps (RegimeSwitch, NotEqual) waits for the sum before it: under the lagged-normaliser rule it runs at the exact
        scale (blhip_chainclamp.hpp, scheme 2); the other rules have no such step"""
        return sh is not None and sh.rule[0] == 'norm_lag' and prog is not None and any(st[0] in ('rs', 'ne') for st in prog[1])

    v, e = _ld(prior), None
    logE, elogE = LD(0), LD(0)
    Ns = []
    d = None if sh is None else LD(0)                                   # projective distance of the forward state (tighten)
    dalpha = []
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        for t in range(T):
            if t > 0:
                v, e, d = transition(steps[t]['fwd'], v, e, d)
            a, ea = product_stage(v, e, liks[t][0], liks[t][1])
            fresh = t > 0 and steps[t]['fwd'][0] != 'prev'
            if sh is None:
                ea = ea + LD(TINY) * lazy(Ns[::-1][:LAZY_LAG - 1])
            else:
                cl = t > 0 and clamped(steps[t]['fwd'])
                term = sh.forward_term(fresh, cl)
                ea = ea + term
                d = d + _proj(C_CELL * u + _rel(liks[t][1], liks[t][0]) + _rel(LD(TINY) + term, a))
            r, er, N, eN = normalise_stage(a, ea, nblk)
            Ns.append(N)
            if sh is not None:
                sh.forward_done(N, fresh, cl)
                d = d + _proj(2 * u + _rel(LD(TINY), r))
                er = tighten(r, er, d)
                dalpha.append(d)
            out['alpha'].append((r, er))
            out['norm'].append((N, eN))
            out['local_fwd'].append((N * dV, eN * dV + 2 * u * N * dV))
            logE = logE + np.log(N)
            elogE = elogE + eN / N + 2 * u * (abs(np.log(N)) + abs(logE))
            v, e = r, er
        logE = logE + np.log(dV)
        out['log_evidence'] = (logE, elogE + 2 * u * abs(logE))
        if not full:
            out['means'] = [means_of(r, er) for r, er in out['alpha']]
            return out
        beta, eb = np.full(np.shape(prior), LD(1) / LD(G), dtype=LD), np.full(np.shape(prior), u / LD(G), dtype=LD)
        post, local, means = [None] * T, [None] * T, [None] * T
        Bs = []
        db = None if sh is None else _proj(u)                           # projective distance of the backward message
        for t in range(T - 1, -1, -1):
            L, eL = _ld(liks[t][0]), _ld(liks[t][1])
            p, ep = product_stage(out['alpha'][t][0], out['alpha'][t][1], beta, eb)
            if sh is not None:
                dp = dalpha[t] + db + _proj(C_CELL * u + _rel(LD(TINY) + sh.posterior_term(t), p))
            ep = ep + (LD(TINY) * lazy(Ns[:t + 1][::-1]) * lazy(Bs[::-1]) if sh is None else sh.posterior_term(t))
            p, ep, Dp = normalise_stage(p, ep, nblk)[:3]
            if sh is not None:
                sh.posterior_done(t, Dp)
                ep = tighten(p, ep, dp + _proj(2 * u + _rel(LD(TINY), p)))
            post[t] = (p, ep)
            means[t] = means_of(p, ep)
            if np.any(L.astype(np.float64) == 0.0):
                local[t] = (LD(np.nan), LD(0))
            else:
                q = p / L
                relL = np.where(L > eL, eL / (L - eL), LD(np.inf))
                eq = ep / L + q * relL + 2 * u * q + LD(TINY)
                S = q.sum()
                eS = eq.sum() + (G + nblk) * u * S
                val = LD(1) / (S * dV)
                local[t] = (val, val * (eS / (S - eS) + 3 * u) + LD(TINY) if S > eS else LD(np.inf))
            if t > 0:
                b, ebl = product_stage(beta, eb, L, eL)
                fresh = steps[t - 1]['bwd'][0] != 'prev'
                cl = clamped(steps[t - 1]['bwd'])
                if sh is not None:
                    db = db + _proj(C_CELL * u + _rel(eL, L) + _rel(LD(TINY) + sh.backward_term(fresh, cl), b))
                ebl = ebl + (LD(TINY) * lazy(Bs[::-1][:LAZY_LAG - 1]) if sh is None else sh.backward_term(fresh, cl))
                b, ebl, db = transition(steps[t - 1]['bwd'], b, ebl, db)
                beta, eb, Bt = normalise_stage(b, ebl, nblk)[:3]
                Bs.append(Bt)
                if sh is not None:
                    sh.backward_done(Bt, fresh, cl)
                    db = db + _proj(2 * u + _rel(LD(TINY), beta))
                    eb = tighten(beta, eb, db)
        out['post'], out['local'], out['means'] = post, local, means
    return out


# ---- the Poisson likelihood and the table models (tests/test_observation_kernels.py) ------------------------------------------------------------
#
# Written from the reference: observationModels.py:502 (Poisson), :419-439 (Bernoulli), :635 (Laplace), :767 (WhiteNoise), :830-831 (AR1),
# :893-896 (ScaledAR1), :49-54 (the product over the data dimensions; a dimension whose segment holds a NaN contributes 1).  The bounds are counted
# along blk::likelihood<OM_POISSON> and blk::lik_table_kernel (blhip_kernels.hpp), build_records (blhip_program.hpp) and the host column
# cA = exp(-lambda) (blhip_batch.hpp).  Every likelihood function returns L; every bound function returns (e, z): the relative part
# L (exp(rel) - 1) and the absolute part from results below the normal range, as likelihood_bound_exp(split = True) does -- WITHOUT SLACK.
#
# Poisson, per non-NaN count k of a record, DIRECT route  pow(lambda, k) * cA / k!  (times the running product):
#     pow                      within 2 ulp = C_POW = 4 u
#     cA = exp(-lambda)        the argument is exact; within 1 ulp = C_EXP = 2 u
#     k!                       k - 1 rounded products on the host, exact while k! < 2^53 (k <= 18): (k - 1) u beyond
#     pow * cA, / k!, L *=     3 u                                                          -> (C_POW + C_EXP + 3 + [k - 1]) u
#   every one of the four results (pow, pow * cA, / k!: sub = 3 in poisson_bound; L *= f: the one _combine adds) may lie below the normal
#   range; all factors are <= 1 there (k! >= 1, cA <= 1, a probability <= 1): 4 TINY.
# LOG-SPACE route  exp(k * log(lambda) - lambda + f),  f = -ln k! from the host:
#     log                      within 1 ulp = C_LOG = 2 u of |ln lambda|; the product with k: 1 u     -> (C_LOG + 1) u k |ln lambda|
#     - lambda                 1 u |k ln lambda - lambda|
#     + f                      1 u |argument|
#     f                        build_records calls lgammal_r on (long double)k + 1 and rounds the result to float64 once: C_LNFACT = 2 u ln k!
#                              (glibc's table of known errors states 4 ulp OF THE LONG DOUBLE for lgammal on x86-64, 2^-8 u; the rounding
#                              to float64 is 1 u).  The count is for the x86-64 host, the only one a gfx950 build has; it does not depend on
#                              the width of NumPy's longdouble in the test process.
#     exp, L *=                C_EXP + 1
#   so the argument is off by u ((C_LOG + 1) k |ln lambda| + |k ln lambda - lambda| + |arg| + C_LNFACT ln k!): it grows like
#   u (k |ln lambda| + lambda + ln k!), which is what limits the route (the largest count inside the 1e-9 bar).
#
# blk::lik_table_kernel, per data dimension (x0[, x1]) and cell (g0[, g1]); every factor is followed by L *= f (1 u, one TINY):
#   Bernoulli   p = g0 or 0, f = p or 1 - p:                                      1 u
#   Laplace     exp(-|x0 - g0| / g1) / (2 g1): the difference and the quotient 2 u a, a = |x0 - g0| / g1; exp C_EXP; 2 g1 exact; the quotient 1 u.
#               A subnormal exp() is off by TINY absolutely, and the division by 2 g1 carries that along: TINY / (2 g1), plus the quotient's own.
#   WhiteNoise  exp(-(x0 x0) / (2 g0 g0) - 0.5 log(2 pi g0 g0)): A = x0^2 / (2 g0^2): the square, the product 2 g0 * g0, the quotient: 3 u A;
#               B = 0.5 log(2 pi g0 g0): M_PI (1 u), two products: 3 u in the argument = 3 u absolutely in the log, halved; log C_LOG u |2 B|, halved:
#               1.5 u + C_LOG u |B|; the subtraction u (A + |B|)                        -> (4 A + (C_LOG + 1) |B| + 1.5) u, then exp C_EXP
#   AR1         r = x1 - g0 x0: the product u |g0 x0|, the difference u |r|: |dr| <= u (|g0 x0| + |r|), carried through the square EXACTLY
#               ((|r| + dr)^2 - r^2: where r cancels to 0 the first order vanishes and the second does not); r r, 2 g1 g1, the quotient: 3 u A; B as above with g1
#   ScaledAR1   sc = g1 sqrt(1 - g0 g0): g0 g0 1 u of rho^2, the difference 1 u of 1 - rho^2: relative to 1 - rho^2 that is
#               (1 + K) u, K = rho^2 / (1 - rho^2) -- the cancellation as |rho| -> 1; sqrt halves it and adds u; the product with g1 1 u:
#               rel(sc) = (0.5 (1 + K) + 2) u.  A = r^2 / (2 sc sc): r as AR1's, then (2 rel(sc) + 3 u) A; B: (3 u + 2 rel(sc)) / 2 + C_LOG u |B|.

C_LOG = 2
C_LNFACT = 2
LN2_LD = np.log(LD(2))
_LNFACT = {}


def ln_factorial_exact(k):
    """ln k! in longdouble, exactly from math.factorial: the top 64 bits of the integer (truncated: 2^-63 relative) and its binary exponent"""
    f = math.factorial(int(k))
    sh = max(f.bit_length() - 64, 0)
    return np.log(LD(f >> sh)) + LD(sh) * LN2_LD


STIRLING_FROM = 2000


def ln_factorial(k):
    """ln k! in longdouble: ln_factorial_exact up to k = 2000; beyond, Stirling's series k ln k - k + ln(2 pi k) / 2 + 1 / (12 k) - 1 / (360 k^3)
    + 1 / (1260 k^5), whose next term is below 1 / (1680 k^7) = 5e-27 there (tests/test_highprec.py pins it against the exact one at larger k)"""
    k = int(k)
    if k not in _LNFACT:
        if k <= STIRLING_FROM:
            _LNFACT[k] = ln_factorial_exact(k)
        else:
            n = LD(k)
            _LNFACT[k] = n * np.log(n) - n + LD(0.5) * np.log(LD(2) * PI_LD * n) + LD(1) / (12 * n) - LD(1) / (360 * n ** 3) + LD(1) / (1260 * n ** 5)
    return _LNFACT[k]


def _counts_of(record):
    return [int(x) for x in np.asarray(record, dtype=np.float64).reshape(-1) if x == x]


def _poisson_args(rate, k):
    """(k ln lambda, argument k ln lambda - lambda - ln k!) in longdouble, for rates > 0"""
    lam = _ld(rate)
    with np.errstate(divide='ignore', invalid='ignore'):
        kl = LD(k) * np.log(np.where(lam > 0, lam, LD(1)))
    return kl, kl - lam - ln_factorial(k)


def poisson_likelihood(rate, record):
    """prod over the non-NaN counts k of exp(k ln(lambda) - lambda - ln k!) on the rate grid; lambda = 0: 1 at k = 0, 0 at k > 0; all NaN: 1."""
    lam = _ld(rate).reshape(-1)
    L = np.ones(lam.shape, dtype=LD)
    with np.errstate(under='ignore'):
        for k in _counts_of(record):
            f = np.exp(_poisson_args(lam, k)[1])
            L = L * np.where(lam > 0, f, LD(1) if k == 0 else LD(0))
    return L


def _combine(factors):
    """[(f, rel, sub)] -> (L = prod f, e, z): rel the factor's relative error in units of 1 (u's already in), sub its absolute error in TINYs
    for results below the normal range; every product L *= f adds one u and one TINY"""
    shape = np.shape(factors[0][0]) if factors else ()
    L, rel = np.ones(shape, dtype=LD), np.zeros(shape, dtype=LD)
    z = np.zeros(shape, dtype=LD)
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        for f, r, _ in factors:
            L = L * f
            rel = rel + r + LD(U)
        for k, (_, _, sub) in enumerate(factors):
            others = np.ones(shape, dtype=LD)
            for j, (f, _, _) in enumerate(factors):
                if j != k:
                    others = others * f
            z = z + LD(TINY) * (sub * others + 1)
        e = np.where(L == 0, LD(0), L * np.expm1(np.minimum(rel, LD(11000))))
    return L, e, z


def poisson_bound(rate, record, direct):
    """(e, z) of blk::likelihood<OM_POISSON> for the record on the rate grid; direct: the route the host chose (observation_cases.direct_domain)"""
    lam = _ld(rate).reshape(-1)
    u = LD(U)
    factors = []
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        for k in _counts_of(record):
            kl, arg = _poisson_args(lam, k)
            f = np.where(lam > 0, np.exp(arg), LD(1) if k == 0 else LD(0))
            if direct:
                fact_ops = (k - 1) if k > 18 else 0                  # (18! < 2^53 < 19!)
                factors.append((f, (C_POW + C_EXP + 2 + fact_ops) * u * np.ones(lam.shape, dtype=LD), LD(3)))
            else:
                lnf = ln_factorial(k)
                earg = u * ((C_LOG + 1) * np.abs(kl) + np.abs(kl - lam) + np.abs(arg) + C_LNFACT * lnf)
                factors.append((f, np.where(lam > 0, earg + C_EXP * u, LD(0)), LD(1)))
    if not factors:
        return np.zeros(lam.shape, dtype=LD), np.zeros(lam.shape, dtype=LD)
    return _combine(factors)[1:]


def _segments(seg):
    """the data dimensions of a segment (seg_len, d) that hold no NaN: [(x0, x1 or None)]"""
    seg = np.asarray(seg, dtype=np.float64)
    seg = seg.reshape(seg.shape[0], -1)
    return [(float(seg[0, k]), float(seg[1, k]) if seg.shape[0] > 1 else None) for k in range(seg.shape[1]) if not np.isnan(seg[:, k]).any()]


def _log_term(s2_rel, s):
    """B = 0.5 ln(2 pi s^2) and its bound for a scale s whose square enters with the relative error s2_rel (beyond M_PI and the two products)"""
    B = LD(0.5) * np.log(LD(2) * PI_LD * s * s)
    return B, LD(0.5) * (3 * LD(U) + s2_rel) + C_LOG * LD(U) * np.abs(B)


def _gauss_factor(r, dr, s, s_rel):
    """exp(-r^2 / (2 s^2) - 0.5 ln(2 pi s^2)) for a residual r known to dr absolutely and a scale s known to s_rel relatively: (f, rel, 1)"""
    u = LD(U)
    with np.errstate(under='ignore', over='ignore'):
        den = LD(2) * s * s
        A = r * r / den
        eA = ((np.abs(r) + dr) ** 2 - r * r) / den + (3 * u + 2 * s_rel) * A
        B, eB = _log_term(2 * s_rel, s)
        f = np.exp(-A - B)
    return f, eA + eB + u * (A + np.abs(B)) + C_EXP * u, LD(1)


def _table_factors(model, g0, g1, seg):
    u = LD(U)
    out = []
    for x0, x1 in _segments(seg):
        if model == 'bernoulli':            # :430-439: values outside [0, 1] count as 0; any datum other than 0 is a success
            p = np.where((g0 > 1) | (g0 < 0), LD(0), g0)
            out.append((p if x0 != 0.0 else LD(1) - p, u * np.ones(np.shape(g0), dtype=LD), LD(1)))
        elif model == 'laplace':            # :635
            with np.errstate(under='ignore', over='ignore'):
                a = np.abs(LD(x0) - g0) / g1
                out.append((np.exp(-a) / (LD(2) * g1), (2 * a + C_EXP + 1) * u, LD(1) / (LD(2) * g1) + 1))
        elif model == 'white_noise':        # :767
            out.append(_gauss_factor(LD(x0) * np.ones(np.shape(g0), dtype=LD), LD(0), g0, LD(0)))
        elif model in ('ar1', 'scaled_ar1'):
            r = LD(x1) - g0 * LD(x0)
            dr = u * (np.abs(g0 * LD(x0)) + np.abs(r))
            if model == 'ar1':              # :830-831
                out.append(_gauss_factor(r, dr, g1, LD(0)))
            else:                           # :893-896
                one = LD(1) - g0 * g0
                out.append(_gauss_factor(r, dr, g1 * np.sqrt(one), (LD(0.5) * (1 + g0 * g0 / one) + 2) * u))
        else:
            raise ValueError(model)
    return out


def _table(model, grids, seg):
    g0 = _ld(grids[0]).reshape(-1, 1) if len(grids) == 2 else _ld(grids[0]).reshape(-1)
    g1 = _ld(grids[1]).reshape(1, -1) if len(grids) == 2 else None
    shape = (np.size(grids[0]), np.size(grids[1])) if len(grids) == 2 else (np.size(grids[0]),)
    factors = [(np.broadcast_to(f, shape), np.broadcast_to(r, shape), np.broadcast_to(s, shape)) for f, r, s in _table_factors(model, g0, g1, seg)]
    if not factors:
        return np.ones(shape, dtype=LD), np.zeros(shape, dtype=LD), np.zeros(shape, dtype=LD)
    return _combine(factors)


def bernoulli_likelihood(p, seg, bound=False):
    """observationModels.py:419-439 on the grid p; seg (1, d).  bound: -> (L, e, z) instead of L"""
    r = _table('bernoulli', [p], seg)
    return r if bound else r[0]


def white_noise_likelihood(sigma, seg, bound=False):
    """:767 on the grid sigma; seg (1, d)"""
    r = _table('white_noise', [sigma], seg)
    return r if bound else r[0]


def laplace_likelihood(mu, scale, seg, bound=False):
    """:635 on the grid mu x scale; seg (1, d)"""
    r = _table('laplace', [mu, scale], seg)
    return r if bound else r[0]


def ar1_likelihood(rho, sigma, seg, bound=False):
    """:830-831 on the grid rho x sigma; seg (2, d): rows x_(t-1), x_t"""
    r = _table('ar1', [rho, sigma], seg)
    return r if bound else r[0]


def scaled_ar1_likelihood(rho, sigma, seg, bound=False):
    """:893-896 on the grid rho x sigma; seg (2, d)"""
    r = _table('scaled_ar1', [rho, sigma], seg)
    return r if bound else r[0]


TABLE_LIKELIHOODS = dict(bernoulli=bernoulli_likelihood, white_noise=white_noise_likelihood, laplace=laplace_likelihood, ar1=ar1_likelihood,
                         scaled_ar1=scaled_ar1_likelihood)
