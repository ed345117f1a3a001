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
"""
import math

import numpy as np

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
