"""The reference's results for the seeded random configurations and parser queries (tests/golden/reference_*.npz, written by
tests/golden/gen_reference_random.py), read by tests/test_oracle_vs_reference_random.py and tests/test_parser.py.

Every output is stored whole except a posterior sequence (T, *grid), which at full size would be ~100 MB of float64 over all cases.
Of it the fixture holds the shape, a fixed sample of entries (compared entry for entry, as before) and, per time step, two sums
over every block of up to BLOCK cells along each grid axis: of the values, and of the logarithms of their magnitudes (clipped from
below at a floor).  The bounds of both sums follow from the entry-wise bound atol + rtol |b|, so whatever passes the entry-wise
comparison passes these; a relative difference in any one cell moves the sum of logarithms of its block, whatever the cell's mass.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SAMPLE = 1024          # entries of a posterior sequence stored one by one (all of them when it has fewer)
BLOCK = 16             # cells per grid axis of a block of the stored sums
SEEDS_PER_FILE = 20    # (every fixture file stays well under 1 MiB)


def fixture_path(family, seed=None):
    """tests/golden/reference_parser.npz, or the file of a family's cases that holds `seed`: reference_random_<family>_<k>.npz."""
    if family == 'parser':
        return os.path.join(GOLDEN, 'reference_parser.npz')
    return os.path.join(GOLDEN, 'reference_random_%s_%d.npz' % (family, seed // SEEDS_PER_FILE))


@functools.lru_cache(maxsize=None)
def _load(path):
    return np.load(path)


def load(family, seed=None):
    """-> {name: array} of one case of a family (seed), or of the parser record (seed None)."""
    z = _load(fixture_path(family, seed))
    if seed is None:
        return {k: z[k] for k in z.files}
    pre = '%d/' % seed
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def sample_index(size):
    """The flat indices of the stored sample: a fixed function of the size (the legacy RandomState stream does not change across numpy
    releases)."""
    if size <= SAMPLE:
        return np.arange(size)
    return np.sort(np.random.RandomState(size % 2 ** 32).permutation(size)[:SAMPLE])


def log_floor(atol):
    """Below this magnitude a cell enters the sum of logarithms as the floor itself (a cell near atol may differ by 100 %)."""
    return max(1e-280, 16.0 * atol)


def block_sums(P):
    """P (T, *grid) summed over blocks of up to BLOCK cells along every grid axis -> (T, *ceil(grid / BLOCK))."""
    for d in range(1, P.ndim):
        P = np.add.reduceat(P, np.arange(0, P.shape[d], BLOCK), axis=d)
    return P


def _logs(P, floor):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.log(np.maximum(np.abs(P), floor))


def reduce_posterior(P, atol):
    """What a fixture keeps of a posterior sequence (see the module's docstring); `atol` is the absolute tolerance of its test."""
    P = np.asarray(P, dtype=float)
    rec = {'shape': np.asarray(P.shape, dtype=np.int64), 'sample': P.reshape(-1)[sample_index(P.size)]}
    if P.ndim >= 2 and P.size:
        floor = log_floor(atol)
        rec.update(log_floor=np.float64(floor), sums=block_sums(P), log_sums=block_sums(_logs(P, floor)))
    return rec


def check_posterior(rec, b, rtol, atol, what):
    """The oracle's posterior sequence `b` against a reduced record of the reference's: the same shape; the sampled entries within
    atol + rtol |b|, with the same NaN / inf pattern; per block, the sum of the values within count * atol + rtol * (the sum of |b|),
    the sum of the clipped logarithms within the sum over its cells of -log(1 - rtol - atol / max(|b|, floor)) -- both as implied
    by the entry-wise bound -- plus the round-off of summing (1e-13 of the sum of magnitudes)."""
    b = np.asarray(b, dtype=float)
    assert tuple(int(n) for n in rec['shape']) == b.shape, what + ': shape'
    _close(rec['sample'], b.reshape(-1)[sample_index(b.size)], rtol, atol, what + ' (sampled entries)')
    if b.ndim < 2 or not b.size:
        return
    floor = float(rec['log_floor'])
    assert rtol + atol / floor < 1.0, what + ': log floor %g too low for atol %g' % (floor, atol)
    cell_log_bound = -np.log1p(-(rtol + atol / np.maximum(np.abs(b), floor)))
    lb = _logs(b, floor)
    for label, sa, sb, bound in (('sums', rec['sums'], block_sums(b), block_sums(np.full(b.shape, atol)) + (rtol + 1e-13) * block_sums(np.abs(b))),
                                 ('sums of logarithms', rec['log_sums'], block_sums(lb), block_sums(cell_log_bound) + 1e-13 * block_sums(np.abs(lb)))):
        label = '%s (block %s)' % (what, label)
        assert sa.shape == sb.shape, label + ': shape'
        assert np.array_equal(np.isnan(sa), np.isnan(sb)), label + ': NaN pattern'
        ok = np.isfinite(sa) & np.isfinite(sb)
        assert np.array_equal(sa[~ok & ~np.isnan(sa)], sb[~ok & ~np.isnan(sb)]), label + ': inf pattern'
        assert np.all(np.abs(sa - sb)[ok] <= bound[ok]), '%s: max diff %.3e' % (label, np.abs(sa - sb)[ok].max())


def _close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ': NaN pattern'
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(a[~ok & ~np.isnan(a)], b[~ok & ~np.isnan(b)]), what + ': inf pattern'
    assert np.all(np.abs(a[ok] - b[ok]) <= atol + rtol * np.abs(b[ok])), '%s: max diff %.3e' % (what, np.abs(a[ok] - b[ok]).max())
