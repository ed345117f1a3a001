"""
The inputs, shifts and grids of tests/test_transition_kernels.py (GPU: the large-shift and stage kernels against tests/highprec.py), kept apart
from it so that tests/test_highprec.py can hold the float64 oracle to the same bounds on the same table without a GPU: the table can only
hold what the reference alone passes.

Grids have the lattice constant 1 on both axes (marginal values 0, 1, 2, ...): a shift given in parameter units IS the shift in cells,
with no rounded division in between.  Axis 0 is the first parameter (lines are the columns of the (n0, n1) array, stride n1), axis 1 the
second (lines are rows).
"""
import numpy as np

# ---- launch geometry: the few lines of choose_tile (16 x 128 tiles) and launch_bigshift_t that decide it, restated ------------------
LDS_DOUBLES = (160 * 1024 - 512) // 8
SCRATCH = 16


def nblk_of(shape):
    """partial slots per chain: tiles of 16 x 128 cells (no filter radius shrinks them in these programs)"""
    n0, n1 = shape
    return -(-n0 // min(16, n0)) * -(-n1 // min(128, n1))


def pitch_of(N, L, axis):
    if axis == 1:
        return N | 1
    Lp = 1
    while Lp < L:
        Lp <<= 1
    r = 1 if Lp >= 32 else 32 // Lp
    return N + ((r - N) & 31)


def geometry(shape, axis):
    """-> dict(n, lines, nblk, L, Lp, nbb, pitch, last, lds_capped): what launch_bigshift_t chooses for a shift along `axis`"""
    n, lines = (shape[0], shape[1]) if axis == 0 else (shape[1], shape[0])
    nblk = nblk_of(shape)
    Lfit = min((LDS_DOUBLES - SCRATCH) // (n + 24 + 32), lines)
    Lmin = -(-lines // nblk)
    assert Lfit >= max(Lmin, 1), (shape, axis)
    want = max(Lmin, 8 if axis == 0 else 4)
    L = min(want, Lfit)
    nbb = -(-lines // L)
    L = -(-lines // nbb)
    Lp = 1
    while Lp < L:
        Lp <<= 1
    assert nbb <= nblk
    return dict(n=n, lines=lines, nblk=nblk, L=L, Lp=Lp, nbb=nbb, pitch=pitch_of(n + 24, L, axis), last=lines - (nbb - 1) * L,
                lds_capped=Lfit < min(want, lines))


# (shape, axes): the blocks of launch_bigshift_t the issue names, each on both axes where the formulas can reach it
GEOMETRIES = [
    ((16, 128), (0, 1)),        # axis 0: one block of L = 128 columns, Lp >= 32, nbb == nblk;  axis 1: L = 16 rows in one block
    ((128, 16), (0, 1)),        # the transpose
    ((40, 128), (0, 1)),        # axis 0: L = 43, not a power of two, a short last block
    ((43, 20), (0, 1)),         # axis 1: L = 15 rows, short last block;  axis 0: L = 7 < Lp = 8
    ((203, 77), (0, 1)),        # ragged both ways
    ((1000, 5), (0,)), ((5, 1000), (1,)),
    ((4096, 3), (0,)), ((3, 4096), (1,)),
    ((4097, 3), (0,)), ((3, 4097), (1,)),
    ((16384, 2), (0,)), ((2, 16384), (1,)),      # BIGSHIFT_MAX_LINE: L = 1 from the LDS capacity, nbb = 2 of many partial slots
]
SWEEP_N = list(range(13, 141))                   # N = n + 24 = 37 .. 164: chunks of C = 1 (empty lanes, N < 64) and 3 and their edges
SWEEP_LINES = 3


def sweep_shape(n, axis):
    return (n, SWEEP_LINES) if axis == 0 else (SWEEP_LINES, n)


def spline_chunks():
    """the chunk sizes C = ((N + 63) >> 6) | 1 of the device's prefilter that the sweep's padded lines N = n + 24 take"""
    return {((n + 24 + 63) >> 6) | 1 for n in SWEEP_N}


def coverage():
    """which of the launch classes the geometries reach, per axis"""
    seen = {0: set(), 1: set()}
    shapes = [(s, ax) for s, axes in GEOMETRIES for ax in axes] + [(sweep_shape(n, ax), ax) for n in SWEEP_N for ax in (0, 1)]
    for shape, ax in shapes:
        g = geometry(shape, ax)
        if g['Lp'] >= 32:
            seen[ax].add('Lp>=32')
        if g['L'] > 8 and g['L'] != g['Lp']:
            seen[ax].add('odd L>8')
        if g['L'] < g['Lp'] and g['last'] < g['L']:
            seen[ax].add('L<Lp, short last block')
        if g['L'] == 1 and g['lds_capped']:
            seen[ax].add('L=1 from LDS')
        seen[ax].add('nbb<nblk' if g['nbb'] < g['nblk'] else 'nbb==nblk')
    return seen


# ---- shifts, in cells ----------------------------------------------------------------------------------------------------------------
CONTROL_SHIFTS = [12.0, -12.0]                   # the small-shift stencil of the fused step kernel: no large-shift kernel


def shifts(n):
    """the large shifts for a line of n points: next to 12, integers, fractions, around and beyond the line (only the clamped tail is
    left), far beyond, and beyond the device's +-1e9 index clamp"""
    up = float(np.nextafter(12.0, 13.0))
    return [up, -up, 12.0000001, -12.0000001, 13.0, -13.0, 16.6, -23.25, n - 0.5, float(n), n + 30.7, -(n + 5.0), -(n - 0.5), 1e6, -1e6, 3e9, -3e9]


SWEEP_SHIFTS = lambda n: [13.0, -16.6, n - 0.5, -(n + 5.0)]     # noqa: E731


# ---- input states ----------------------------------------------------------------------------------------------------------------------
INPUTS = ('cube', 'decades', 'single', 'edges', 'zero_lines')


def state(kind, shape, axis, seed=0):
    """a normalised float64 distribution on the grid; `axis`: the axis whose lines the kind speaks of"""
    rng = np.random.default_rng(9000 + seed)
    n0, n1 = shape
    if kind == 'cube':                                   # bigshift_cases.distribution
        x = rng.random(shape) ** 3 + 1e-3
    elif kind == 'decades':                              # 600 e-folds (260 decades) of range, cell by cell
        x = np.exp(-600.0 * rng.random(shape))
    elif kind in ('single', 'edges', 'zero_lines'):
        xm = np.zeros((shape[axis], shape[1 - axis]))    # (position along the line, line)
        n, lines = xm.shape
        for l in range(lines):
            if kind == 'single':                         # within 150 cells of one end, alternately: the tail z^k that a shift beyond the
                k = int(rng.integers(0, min(n, 150)))    # line leaves of it stays above the float64 underflow (the chain's sum too)
                xm[k if l % 2 == 0 else n - 1 - k, l] = 0.5 + rng.random()
            elif kind == 'edges':
                xm[0, l] = 0.5 + rng.random()
                xm[n - 1, l] = 0.5 + rng.random()
            elif l % 2 == 0:                             # every other line is entirely zero
                xm[:, l] = rng.random(n) ** 3 + 1e-3
        x = xm if axis == 0 else xm.T
    else:
        raise ValueError(kind)
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x / x.sum()


def well_conditioned(D, eD, slack):
    """Deterministic divides the shifted distribution by its sum D.  Where an integer shift moves every occupied cell of a 'single' or
    'edges' input off the grid, the spline interpolates the zeros that are left: SciPy's own result is rounding noise around 0 and the
    reference divides by it.  Such a combination says nothing about a kernel; a chain is run when |D| is beyond 8 times the bound of D
    (computed from the longdouble restatement alone; tests/test_highprec.py lists what this leaves out and asserts it is only that class)."""
    return abs(D) > 8 * slack * eD
