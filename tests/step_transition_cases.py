"""
The problems of tests/test_step_transitions.py (GPU: the transition half of the fused step kernels against tests/highprec.py), kept apart from it
so that tests/test_highprec.py can run the float64 oracle on every one of them and hold it to the same bounds without a GPU.

A CASE is one engine call: a kernel family (engine options and a grid), a list of transition models shared by the chains of the batch and one
tuple of parameters per chain.  Lattice constants are 1 (marginal values 0, 1, 2, ...): widths and shifts are in cells.  Models, in the list
order of a CombinedTransitionModel (transitionModels.py:645-649):
    ('walk', axis)      GaussianRandomWalk; parameter: the SciPy radius r (sigma = (r - 1/4) / 4, so that int(4 sigma + 0.5) = r); 0: no walk
    ('rs',)             RegimeSwitch; parameter: log10 pMin            ('ne',)   NotEqual; parameter: log10 pMin
    ('biv',)            BivariateRandomWalk; parameter: (sigma1, sigma2, rho)
    ('as', axis)        AlphaStableRandomWalk; parameter: (c, alpha)
    ('shift', axis)     Deterministic; parameter: the shift d (|d| <= 12: the one-pass stencil; 1-D grids: beyond it the two-stage shift), applied
                        in the direction a driver looks at, 0 in the other; a tuple: one shift per transition (a number: d, then -d)
    ('cp',)             ChangePoint; parameter: the step it fires behind       ('indep',)  Independent; no parameter (None)
    ('bp',)             BreakPoint of a SerialTransitionModel; parameter: the time stamp from which the next sub-model acts.  A case with break
                        points names the sub-model of every model (`segments`, one entry per model; None: the model acts in every segment)
Grids with more than two parameters (the families `nd` and `chain_nd`) take walks, NotEqual, shifts of up to 12 cells and the sources.
DRIVERS (every step has a table likelihood, BLHIP_OM_TABLE):
    forward    T = 2, prior = x, likelihood 1, forward-only, posteriors kept: step 1's posterior is normalise(K x)
    backward   T = 2, uniform prior, likelihoods (1, x), full fit: step 0's posterior is the normalised backward transition of x
    three      T = 3, prior = x, likelihoods (1, y, y'), full fit: the normalisers are not 1 where the second transition acts
"""
import numpy as np

import highprec as hp
import transition_cases as tc
from bayesloop_amd import _abi

INPUTS = ('cube', 'single', 'edges', 'decades')          # dense, one cell per line, both edges of every line, 600 e-folds of range
DRIVERS = ('forward', 'backward', 'three')
OFF = dict(chain_resident=0, resident=0)


def sigma_of(radius):
    return 0.0 if radius == 0 else (radius - 0.25) / 4.0


SHIFTS_2D = [0.5, -0.5, 3.25, -3.25, 11.999, -11.999, 12.0, -12.0]
SHIFTS_1D = [0.5, -0.5, 3.25, -3.25, 12.0, -12.0]
BIG_1D = [12.0000001, 40.5]

# name -> dict(family, shape, opts, models, chains, drivers[, inputs])
CASES = {}


def _case(name, family, shape, opts, models, chains, drivers=DRIVERS, inputs=INPUTS, segments=None):
    assert name not in CASES
    segments = [None] * len(models) if segments is None else list(segments)
    assert len(segments) == len(models) and all(len(c) == len(models) for c in chains), name
    CASES[name] = dict(name=name, family=family, shape=tuple(shape), opts=opts, models=models, chains=[tuple(c) for c in chains],
                       drivers=tuple(drivers), inputs=tuple(inputs), segments=segments)


# ---- blk::step_kernel<100, 0 / 1, *>: 24 x 20 (two tiles of 16 rows) and 20 x 140 (two tiles of 128 columns) --------------------------------
GENERIC = dict(OFF, fast=0, mfma=0)
for tag, shape in (('24x20', (24, 20)), ('20x140', (20, 140))):
    _case('generic_walks_' + tag, 'generic', shape, GENERIC, [('walk', 0), ('walk', 1)], [(3, 0), (0, 2), (3, 2)])
    _case('generic_rs_then_walk_' + tag, 'generic', shape, GENERIC, [('rs',), ('walk', 0)], [(-4.0, 3), (-2.0, 2)])              # clamp mode 1
    _case('generic_walk_then_rs_' + tag, 'generic', shape, GENERIC, [('walk', 1), ('rs',)], [(2, -4.0), (3, -2.0)])              # clamp mode 2
    _case('generic_not_equal_' + tag, 'generic', shape, GENERIC, [('ne',)], [(-4.0,), (-7.0,)], drivers=('forward', 'three'))     # mode 3
    _case('generic_bivariate_' + tag, 'generic', shape, GENERIC, [('biv',)],
          [((1.3, 0.7, 0.0),), ((1.3, 0.7, 0.9),), ((0.7, 1.6, -0.9),)])                                                         # mode 4
    for ax in (0, 1):
        _case('generic_alphastable_axis%d_%s' % (ax, tag), 'generic', shape, GENERIC, [('as', ax)],
              [((1.3, 1.0),), ((0.8, 1.5),), ((1.1, 2.0),)])                                                                     # mode 5
        _case('generic_shift_axis%d_%s' % (ax, tag), 'generic', shape, GENERIC, [('shift', ax)], [(d,) for d in SHIFTS_2D])    # mode 6
_case('generic_change_point_24x20', 'generic', (24, 20), GENERIC, [('walk', 0), ('cp',), ('walk', 1)], [(3, 1, 2), (2, 0, 0)], drivers=('three',))
_case('generic_independent_24x20', 'generic', (24, 20), GENERIC, [('walk', 0), ('indep',), ('rs',)], [(3, None, -4.0)], drivers=('three',))

# ---- bl1c::chain1d_kernel<100, BWD, M, CL>: n = 300 (M = 1) and 600 (M = 2: beyond the block's 512 threads) ------------------------------------
CHAIN1D = dict(chain1d=2)
for n in (300, 600):
    _case('chain1d_walks_%d' % n, 'chain1d', (n,), CHAIN1D, [('walk', 0)], [(5,), (n - 1,)])                                    # CL = 0
    _case('chain1d_rs_then_walk_%d' % n, 'chain1d', (n,), CHAIN1D, [('rs',), ('walk', 0)], [(-4.0, 5), (-2.0, 3)])              # CL = 2
    _case('chain1d_walk_then_rs_%d' % n, 'chain1d', (n,), CHAIN1D, [('walk', 0), ('rs',)], [(5, -4.0), (3, -2.0)])
    _case('chain1d_not_equal_%d' % n, 'chain1d', (n,), CHAIN1D, [('ne',)], [(-4.0,), (-7.0,)], drivers=('forward', 'three'))
_case('chain1d_shifts_300', 'chain1d', (300,), CHAIN1D, [('shift', 0)], [(d,) for d in SHIFTS_1D + BIG_1D])                     # CL = 1: asym and two-stage
# a batch that mixes them per chain and per step: shifts of either kind and none (CL = 1); clamps in front of and behind a walk (CL = 2)
_case('chain1d_mixed_shifts_300', 'chain1d', (300,), CHAIN1D, [('shift', 0)], [((0.0, 3.25),), ((-12.0, 0.5),), ((40.5, 0.0),), ((0.5, -40.5),)],
      drivers=('three',))
_case('chain1d_mixed_clamps_300', 'chain1d', (300,), CHAIN1D, [('walk', 0), ('rs',)], [(5, -4.0), (0, -2.0), (3, -300.0)], drivers=('three',))
# ... and the composition one stage cannot hold (a walk, a shift and a clamp): the stage kernels in front of the generic one, on a row
_case('generic_composed_row_300', 'generic', (300,), CHAIN1D, [('walk', 0), ('shift', 0), ('rs',)],
      [(5, (0.0, 3.25), -300.0), (0, (-12.0, 0.5), -4.0), (3, (0.0, 0.0), -2.0), (0, (40.5, 0.0), -300.0)], drivers=('three',))

# ---- bl1f::fused1d_kernel / bl1p::persist1d_kernel, n = 300 (the persistent kernel needs more steps than one launch of the fused one takes) -------
for fam, opts, drv in (('fused1d', dict(chain1d=0, persist1d=0), DRIVERS), ('persist1d', dict(chain1d=0, fuse1d=2), ('three',))):
    _case(fam + '_walks_300', fam, (300,), opts, [('walk', 0)], [(5,), (40,)], drivers=drv)
    _case(fam + '_sources_300', fam, (300,), opts, [('walk', 0), ('cp',)], [(5, 1), (40, 0)], drivers=('three',))

# ---- blf::fast_step_kernel / blm::mfma_step_kernel<100, ..>: 140 x 90, one batch per radius bucket of the first parameter with both of its edges
#      (a batch takes the kernel of its widest chain); an axis-1 walk of radius 1 and 8; the lean form on 128 x 64 --------------------------------------
BUCKETS = {8: (1, 8), 16: (9, 16), 24: (17, 24), 32: (25, 32), 40: (33, 40)}
for r0, (lo, hi) in BUCKETS.items():
    _case('fast_band%d_140x90' % r0, 'fast', (140, 90), dict(OFF, mfma=0), [('walk', 0)], [(lo,), (hi,)])
    _case('fast_band%d_h_140x90' % r0, 'fast', (140, 90), dict(OFF, mfma=0), [('walk', 0), ('walk', 1)], [(lo, 8), (hi, 1)])
    _case('mfma_band%d_140x90' % r0, 'mfma', (140, 90), OFF, [('walk', 0)], [(lo,), (hi,)])
    _case('mfma_band%d_h_140x90' % r0, 'mfma', (140, 90), OFF, [('walk', 0), ('walk', 1)], [(lo, 8), (hi, 1)])
    _case('mfma_band%d_lean_128x64' % r0, 'mfma', (128, 64), OFF, [('walk', 0)], [(lo,), (hi,)])

# ---- blh::hwide_kernel (axis 1, radius 9 .. 256) and blh::vwide_kernel (axis 0, radius 41 .. 128) -------------------------------------------------
_case('hwide_40x300', 'hwide', (40, 300), OFF, [('walk', 0), ('walk', 1)], [(0, 9), (3, 64), (0, 256), (8, 0)])        # mixed radii; a chain without an axis-1 filter
_case('hwide_40x40', 'hwide', (40, 40), OFF, [('walk', 1)], [(39,)])
_case('vwide_140x64', 'vwide', (140, 64), OFF, [('walk', 0)], [(41,), (128,)])
_case('vwide_fallback_140x64', 'generic', (140, 64), OFF, [('walk', 0)], [(139,)])      # n0 - 1: beyond what the host admits, the generic kernel

# ---- the resident families with a table likelihood, at the shapes of tests/test_likelihood_kernels.py -------------------------------------------------------
_case('resident_32x32', 'resident', (32, 32), {}, [('walk', 0), ('walk', 1)], [(7, 5)])
_case('chainax_sources_32x32', 'chainax', (32, 32), {}, [('walk', 0), ('walk', 1), ('cp',)], [(7, 5, 1)], drivers=('three',))
_case('chain_128x16', 'chain', (128, 16), {}, [('walk', 0)], [(7,), (6,), (5,)])
_case('chain_sources_128x16', 'chain', (128, 16), {}, [('walk', 0), ('cp',)], [(7, 1), (6, 0), (5, 1)], drivers=('three',))
_case('chainax_100x90', 'chainax', (100, 90), {}, [('walk', 0), ('walk', 1)], [(7, 5), (6, 5)])

# ---- shared sources (P.shared[kind]) in the families above that have no such case yet: a change point IN FRONT of the walk, so that the stencil reads
#      the reset prior (transitionModels.py:300-312, then :107-115); chains that fire behind step 1 and behind step 0 -----------------------------------
_case('chain1d_sources_300', 'chain1d', (300,), CHAIN1D, [('cp',), ('walk', 0)], [(1, 5), (0, 299)], drivers=('three',))
_case('fast_band8_sources_140x90', 'fast', (140, 90), dict(OFF, mfma=0), [('cp',), ('walk', 0)], [(1, 8), (0, 1)], drivers=('three',))
_case('mfma_band8_sources_140x90', 'mfma', (140, 90), OFF, [('cp',), ('walk', 0)], [(1, 8), (0, 1)], drivers=('three',))
_case('hwide_sources_40x300', 'hwide', (40, 300), OFF, [('cp',), ('walk', 1)], [(1, 64), (0, 9)], drivers=('three',))
_case('vwide_sources_140x64', 'vwide', (140, 64), OFF, [('cp',), ('walk', 0)], [(1, 41), (0, 128)], drivers=('three',))

# ---- grids with three and four parameters: the plain path (bln::filter_axis_kernel, bln::step_kernel<BWD> and the renormalising stages
#      ne_max / ne_invert / ne_clamp / shift_axis_kernel; chain_nd = 0) and bln::chain_nd_kernel<BWD, 256 | 1024> (chain_nd = 2: walks and
#      restarts).  5 x 18 x 14: five blocks of 256 cells with a partial last one, inner = 252, 14 and 1; 3 x 7 x 5: less than a block;
#      3 x 3 x 7 x 6: four parameters.  The first walk is the one on the WIDE axis (18 resp. 7 cells), so that `single` and `edges` speak of its
#      lines: radii n, n + 1 (the kernels' other reflection branch) and beyond 2 n (several periods); walks on every axis and on all; a chain
#      without a walk ---------------------------------------------------------------------------------------------------------------------------------
ND, CHAIN_ND = dict(chain_nd=0), dict(chain_nd=2)
ND_SHAPES = {'5x18x14': (5, 18, 14), '3x7x5': (3, 7, 5), '3x3x7x6': (3, 3, 7, 6), '4x16x32': (4, 16, 32)}
ND_WALKS = {
    '5x18x14': ([('walk', 1), ('walk', 0), ('walk', 2)], [(18, 0, 0), (19, 0, 0), (23, 0, 0), (0, 2, 0), (0, 0, 3), (5, 2, 3), (0, 0, 0)]),
    '3x7x5': ([('walk', 1), ('walk', 0), ('walk', 2)], [(7, 0, 0), (8, 0, 0), (16, 0, 0), (0, 2, 0), (0, 0, 3), (3, 2, 3), (0, 0, 0)]),
    '3x3x7x6': ([('walk', 2), ('walk', 0), ('walk', 3), ('walk', 1)],
                [(7, 0, 0, 0), (8, 0, 0, 0), (16, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (3, 2, 3, 1), (0, 0, 0, 0)]),
    '4x16x32': ([('walk', 1), ('walk', 0), ('walk', 2)], [(16, 0, 0), (17, 0, 0), (35, 0, 0), (0, 3, 0), (0, 0, 5), (4, 3, 5), (0, 0, 0)]),
}


def _nd_walks_and_sources(fam, opts, tag):
    shape = ND_SHAPES[tag]
    wide = ND_WALKS[tag][0][0]                       # the walk on the axis of 18 (7, 16) cells
    n = shape[wide[1]]
    _case('%s_walks_%s' % (fam, tag), fam, shape, opts, *ND_WALKS[tag])
    # a change point in FRONT of the walk (the stencil reads the reset prior) and BEHIND it (the walk is dropped); chains that fire behind step 1
    # and behind step 0; Independent between two walks
    _case('%s_cp_then_walk_%s' % (fam, tag), fam, shape, opts, [('cp',), wide], [(1, 3), (0, n + 1)], drivers=('three',))
    _case('%s_walk_then_cp_%s' % (fam, tag), fam, shape, opts, [wide, ('cp',)], [(3, 1), (n + 1, 0)], drivers=('three',))
    _case('%s_independent_%s' % (fam, tag), fam, shape, opts, [wide, ('indep',), ('walk', len(shape) - 1)], [(3, None, 2)], drivers=('three',))


for tag in ('5x18x14', '3x7x5', '3x3x7x6'):
    _nd_walks_and_sources('nd', ND, tag)
    _nd_walks_and_sources('chain_nd', CHAIN_ND, tag)
# ... the 1024-thread block (two cells per thread), and a batch in which every chain has another radius on the same walks (one of them none)
# and another step at which its change point fires (7: never): the tap slots of a block, the source kind loaded a step ahead
_case('chain_nd_walks_4x16x32', 'chain_nd', ND_SHAPES['4x16x32'], CHAIN_ND, *ND_WALKS['4x16x32'])
for tag in ('5x18x14', '4x16x32'):
    _case('chain_nd_mixed_%s' % tag, 'chain_nd', ND_SHAPES[tag], CHAIN_ND, [('walk', 1), ('cp',), ('walk', 2)],
          [(3, 1, 2), (19, 0, 0), (0, 7, 5), (7, 0, 1), (0, 1, 0), (1, 7, 3)], drivers=('three',))

# NotEqual (three launches: the maximum, the inversion, the clamp) alone, behind a walk, in front of one, and twice with a walk between
for nm, models, chains in (('not_equal', [('ne',)], [(-4.0,), (-7.0,)]),
                           ('walk_then_ne', [('walk', 1), ('ne',)], [(3, -4.0), (19, -7.0)]),
                           ('ne_then_walk', [('ne',), ('walk', 1)], [(-4.0, 3), (-7.0, 19)]),
                           ('ne_walk_ne', [('ne',), ('walk', 2), ('ne',)], [(-4.0, 3, -7.0), (-7.0, 0, -4.0)])):
    _case('nd_%s_5x18x14' % nm, 'nd', (5, 18, 14), ND, models, chains, drivers=('forward', 'three'))
_case('nd_not_equal_3x3x7x6', 'nd', (3, 3, 7, 6), ND, [('ne',)], [(-4.0,), (-7.0,)], drivers=('forward', 'three'))
# shifts on the first, the middle and the last axis, and on an axis of the four-parameter grid
for ax in (0, 1, 2):
    _case('nd_shift_axis%d_5x18x14' % ax, 'nd', (5, 18, 14), ND, [('shift', ax)], [(d,) for d in SHIFTS_2D])
_case('nd_shift_axis2_3x3x7x6', 'nd', (3, 3, 7, 6), ND, [('shift', 2)], [(d,) for d in SHIFTS_2D])
_case('nd_shift_then_walk_5x18x14', 'nd', (5, 18, 14), ND, [('shift', 0), ('walk', 1)], [(0.5, 3), (-3.25, 19), (12.0, 0)])
# a batch that mixes a shift and none per chain and step: the chain without one passes through shift_axis_kernel BY COPY, values and the
# partial sums its scale is read from; a NotEqual chain beside chains whose change point restarts at that step (ne_clamp_kernel's copy)
_case('nd_mixed_shifts_5x18x14', 'nd', (5, 18, 14), ND, [('shift', 1)], [((0.0, 3.25),), ((-12.0, 0.5),), ((0.5, 0.0),)], drivers=('three',))
_case('nd_mixed_shifts_3x3x7x6', 'nd', (3, 3, 7, 6), ND, [('shift', 3)], [((0.0, 3.25),), ((-12.0, 0.5),), ((0.5, 0.0),)], drivers=('three',))
_case('nd_ne_beside_restart_5x18x14', 'nd', (5, 18, 14), ND, [('ne',), ('cp',)], [(-4.0, 7), (-4.0, 1), (-7.0, 0)], drivers=('forward', 'three'))


def chain_nd_threads(case):
    """bln::chain_nd_threads restated (blhip_chain_nd.hpp): 256 threads while two state buffers, a tap slot of the batch's widest radius per
    walk, the grid values and the reduction scratch take at most 32 KB of LDS, 1024 beyond"""
    shape = case['shape']
    walks = [k for k, m in enumerate(case['models']) if m[0] == 'walk']
    lw = max([c[k] for c in case['chains'] for k in walks] + [0])
    doubles = 2 * int(np.prod(shape)) + len(walks) * (lw + 1) + sum(shape) + 7 * (1024 // 64) + 8
    return 256 if doubles * 8 <= 32 * 1024 else 1024


# the large block runs on 4 x 16 x 32 alone, at two cells per thread; every other grid of the family is below the 32 KB
for _n, _c in CASES.items():
    if _c['family'] == 'chain_nd':
        assert chain_nd_threads(_c) == (1024 if _n.endswith('4x16x32') else 256), _n
assert 1024 < int(np.prod(ND_SHAPES['4x16x32'])) <= 2 * 1024
assert chain_nd_threads(dict(CASES['chain_nd_walks_4x16x32'], shape=(4, 16, 31))) == 1024      # (not THE threshold: 1984 cells are beyond it too)

# ---- bl1c::chain1d_long_kernel<BWD, M, CL>: rows of 4097 .. 8192 cells, the cases of bl1c::chain1d_kernel above on n = 4100 (the first partial
#      round of 512 threads beyond 4096); (M, CL) = (2, 0) walks, (2, 2) clamps, (1, 1) shifts, (1, 2) shifts and clamps in one program ----------
for nm in ('walks', 'rs_then_walk', 'walk_then_rs', 'not_equal', 'shifts', 'mixed_shifts', 'mixed_clamps', 'sources'):
    c = CASES['chain1d_%s_300' % nm]
    _case('chain1d_long_%s_4100' % nm, 'chain1d_long', (4100,), CHAIN1D, c['models'],
          [tuple(300 if p == 299 else p for p in ch) for ch in c['chains']], drivers=c['drivers'])
# a serial model: RegimeSwitch up to the break point, the shift from it on (one program cannot hold both at one step: that is the composed row)
_case('chain1d_long_rs_or_shift_4100', 'chain1d_long', (4100,), CHAIN1D, [('rs',), ('bp',), ('shift', 0)],
      [(-4.0, 1.0, (0.5, 3.25)), (-300.0, 1.0, (-12.0, 40.5)), (-5.0, 7.0, (3.25, 3.25))], drivers=('three',), segments=[0, None, 1])
_case('chain1d_long_walks_8192', 'chain1d_long', (8192,), CHAIN1D, [('walk', 0)], [(0,), (540,)], drivers=('three',))    # 2 n + 5 LW + 113 = 19 197 of 19 200 doubles

# NotEqual inverts around the maximum of its input: of the uniform alpha_0 of the backward driver it is 0 / 0 in the reference
# (transitionModels.py:462-465).  Named here, asserted by tests/test_highprec.py with what well_conditioned leaves out.
NOT_EQUAL_OF_UNIFORM = sorted(n for n, c in CASES.items() if any(m[0] == 'ne' for m in c['models']))


def steps_of(driver):
    return 3 if driver == 'three' else 2


def line_axis(case, seed):
    """the axis whose lines `single` and `edges` speak of on a grid with more than two parameters: the one the case's first walk or shift
    acts on -- the lines its stencil runs along --, seed % ndim for a case without one"""
    return next((m[1] for m in case['models'] if m[0] in ('walk', 'shift')), seed % len(case['shape']))


def state(kind, shape, seed=0, axis=None):
    """a normalised float64 distribution (transition_cases.state; 1-D grids: one line; more than two parameters: (n, lines) of the lines
    along `axis`, moved back into place)"""
    if len(shape) == 1:
        return tc.state(kind, (shape[0], 1), 0, seed)[:, 0].copy()
    if len(shape) == 2:
        return tc.state(kind, shape, seed % 2, seed)
    axis = seed % len(shape) if axis is None else axis
    rest = [n for k, n in enumerate(shape) if k != axis]
    x = tc.state(kind, (shape[axis], int(np.prod(rest))), 0, seed)
    return np.ascontiguousarray(np.moveaxis(x.reshape([shape[axis]] + rest), 0, axis))


def tables(case, kind, driver):
    """-> (prior, likelihood tables (T, *shape), reset prior, independent prior): float64, as given to the library"""
    shape = case['shape']
    G = int(np.prod(shape))
    seed = sum(ord(ch) for ch in case['name']) % 97
    axis = line_axis(case, seed)
    x = state(kind, shape, seed, axis)
    rng = np.random.default_rng(4000 + seed)
    T = steps_of(driver)
    lik = np.ones((T,) + shape)
    prior = x
    if driver == 'backward':
        prior = np.full(shape, 1.0 / G)
        lik[1] = x
    elif driver == 'three':
        lik[1] = 3.0 * (0.5 + rng.random(shape))
        lik[2] = 0.25 * (0.5 + rng.random(shape)) ** 2
    reset = state('cube', shape, seed + 1, axis)
    indep = state('decades', shape, seed + 2, axis)
    return prior, lik, reset, indep


def shifts_of(param, T, driver):
    """-> (forward shifts into step t, backward shifts into step t), each (T,)"""
    fwd, bwd = np.zeros(T), np.zeros(T)
    per = list(param) if isinstance(param, tuple) else [param, -param][:T - 1]        # (three: there and back, so that the line keeps its mass)
    if driver in ('forward', 'three'):
        fwd[1:] = per[:T - 1]
    if driver in ('backward', 'three'):
        bwd[:T - 1] = [-d for d in per[:T - 1]] if driver == 'three' else per[:T - 1]
    return fwd, bwd


def abi_program(case, driver, T=None):
    """-> (ops, values (chains, n_ops)) in the C-ABI's layout (include/blhip.h); T: the steps, where they are not the driver's own
    (tests/long_series_cases.py)"""
    T = steps_of(driver) if T is None else T
    ops, cols = [], []
    for m, seg in zip(case['models'], case['segments']):
        cols.append(len(ops))
        ax = m[1] if len(m) > 1 else 0
        first = len(ops)
        if m[0] == 'walk':
            ops.append((_abi.OP_GRW, ax, -1, 0))
        elif m[0] == 'rs':
            ops.append((_abi.OP_REGIMESWITCH, 0, -1, 0))
        elif m[0] == 'ne':
            ops.append((_abi.OP_NOTEQUAL, 0, -1, 0))
        elif m[0] == 'biv':
            ops += [(_abi.OP_BIVARIATE, 0, -1, 0)] + [(_abi.OP_BIVARIATE_ARG, 0, -1, 0)] * 2
        elif m[0] == 'as':
            ops += [(_abi.OP_ALPHASTABLE, ax, -1, 0), (_abi.OP_ALPHASTABLE_ARG, ax, -1, 0)]
        elif m[0] == 'shift':
            ops += [(_abi.OP_DETERMINISTIC, ax, -1, 0)] + [(_abi.OP_DETERMINISTIC_ARG, 0, -1, 0)] * (2 * T)
        elif m[0] == 'cp':
            ops.append((_abi.OP_CHANGEPOINT, 0, -1, 0))
        elif m[0] == 'indep':
            ops.append((_abi.OP_INDEPENDENT, 0, -1, 0))
        elif m[0] == 'bp':
            ops.append((_abi.OP_BREAKPOINT, 0, -1, 0))
        else:
            raise ValueError(m)
        if seg is not None:
            ops[first:] = [(o[0], o[1], seg, o[3]) for o in ops[first:]]
    values = np.full((len(case['chains']), len(ops)), np.nan)
    for b, params in enumerate(case['chains']):
        for m, col, p in zip(case['models'], cols, params):
            if m[0] == 'walk':
                values[b, col] = sigma_of(p)
            elif m[0] in ('rs', 'ne', 'cp', 'bp'):
                values[b, col] = p
            elif m[0] == 'biv':
                values[b, col:col + 3] = p
            elif m[0] == 'as':
                values[b, col:col + 2] = p
            elif m[0] == 'shift':
                fwd, bwd = shifts_of(p, T, driver)
                values[b, col + 1:col + 1 + T] = fwd
                values[b, col + 1 + T:col + 1 + 2 * T] = bwd
    return ops, values


_TAPS = {}


def _taps(kind, *args):
    """the restated weights ROUNDED to float64 and their bound (the builder's own and the rounding); never the library's tables"""
    key = (kind,) + args
    if key not in _TAPS:
        if kind == 'walk':
            _, w, e = hp.gaussian_walk_taps(*args)
        elif kind == 'as':
            w, e = hp.alphastable_taps(*args)
        else:
            w, e = hp.bivariate_taps(*args)
        w64 = np.asarray(w, dtype=np.float64)
        _TAPS[key] = (w64, np.asarray(e + np.abs(hp._ld(w64) - w), dtype=hp.LD))
    return _TAPS[key]


def stage_program(case, params, driver, T=None):
    """one chain's per-step programs for highprec.transition_fit: [dict(fwd = (source, stages), bwd = (source, stages))] * T"""
    T, shape = (steps_of(driver) if T is None else T), case['shape']

    def program(tau, step, fwd):
        source, stages = 'prev', []
        active = sum(1 for m, p in zip(case['models'], params) if m[0] == 'bp' and p <= tau)      # the sub-model of a serial model (transitionModels.py:768)
        for m, p, seg in zip(case['models'], params, case['segments']):
            if seg is not None and seg != active:
                continue
            if m[0] == 'walk':
                if p:
                    w, e = _taps('walk', sigma_of(p))
                    stages.append(('walk', m[1], w, e))
            elif m[0] == 'rs':
                stages.append(('rs', float(10.0 ** p)))
            elif m[0] == 'ne':
                stages.append(('ne', float(10.0 ** p)))
            elif m[0] == 'biv':
                stages.append(('dense',) + _taps('biv', *p))
            elif m[0] == 'as':
                stages.append(('zero', m[1]) + _taps('as', p[0], p[1], shape[m[1]]))
            elif m[0] == 'shift':
                d = shifts_of(p, T, driver)[0 if fwd else 1][step]
                if d != 0.0:
                    stages.append(('shift', m[1], float(d)))
            elif m[0] == 'cp':
                if tau == p:
                    source, stages = 'reset', []
            elif m[0] == 'indep':
                source, stages = 'indep', []
        return source, stages

    # forward into step t: evaluated at the time stamp of step t - 1 (core.py:411); backward into step t: at ts[t + 1] - 1 = t (:467, transitionModels.py:316-317)
    return [dict(fwd=program(t - 1, t, True) if t > 0 else None, bwd=program(t, t, False) if t < T - 1 else None) for t in range(T)]


def nblk_of(shape):
    return int(np.prod(shape)) // 64 + 1


_REF = {}


def reference(name, kind, driver):
    """per chain the longdouble pass (highprec.transition_fit) with its bounds, computed once and left unchanged; -> (refs, conditioned):
    conditioned[b]: whether every renormalising sum of the chain's pass is well conditioned (transition_cases.well_conditioned)"""
    key = (name, kind, driver)
    if key not in _REF:
        if len(_REF) > 48:
            _REF.clear()
        case = CASES[name]
        shape = case['shape']
        prior, lik, reset, indep = tables(case, kind, driver)
        grids = [np.arange(n, dtype=np.float64) for n in shape]
        refs, ok = [], []
        for params in case['chains']:
            ref = hp.transition_fit(prior, [(L, None) for L in lik], stage_program(case, params, driver), grids, [1.0] * len(shape),
                                    nblk=nblk_of(shape), full=driver != 'forward', shared=dict(reset=reset, indep=indep))
            refs.append(ref)
            ok.append(all(tc.well_conditioned(D, eD, hp.SLACK) for D, eD in ref['sums']))
        _REF[key] = (refs, ok)
    return _REF[key]


def combinations():
    return [(name, kind, driver) for name, c in CASES.items() for kind in c['inputs'] for driver in c['drivers']]


# ---- one engine call per case, input and driver: shared by the GPU file (the library) and tests/test_highprec.py (the float64 oracle) -------------

def run_problem(engine, name, kind, driver, keep, one_at_a_time=False):
    """-> dict(log_evidence (B,), local_evidence (B, T), means (B, ndim, T), posts [B] of (T, *shape)) for the chains `keep` (indices)"""
    from bayesloop_amd.engine import FitProblem
    case = CASES[name]
    shape, T = list(case['shape']), steps_of(driver)
    G = int(np.prod(shape))
    prior, lik, reset, indep = tables(case, kind, driver)
    ops, values = abi_program(case, driver)
    values = np.ascontiguousarray(values[list(keep)])
    problem = FitProblem(obs_model=_abi.OM_TABLE, marginal=[np.arange(n, dtype=np.float64) for n in shape], lattice=[1.0] * len(shape),
                         data=np.zeros((T, 1)), timestamps=np.arange(T, dtype=np.float64), prior=prior, ops=ops, lik=lik.reshape(T, G),
                         reset_prior=reset, indep_prior=indep, seg_len=1)
    out = dict(log_evidence=[], local_evidence=[], means=[], posts=[])
    for rows in ([[b] for b in range(len(values))] if one_at_a_time else [list(range(len(values)))]):
        res = engine.fit(problem, values[rows], forward_only=driver == 'forward', keep_posterior=True)
        assert np.all(res.abort_step < 0), (name, kind, driver, res.abort_step)
        out['log_evidence'] += list(res.log_evidence)
        out['local_evidence'] += list(res.local_evidence)
        out['means'] += list(res.posterior_mean)
        out['posts'] += [np.array(engine.posterior(b, T, shape)) for b in range(len(rows))]
    return out


class Check:
    """collects every miss of a test before failing; keeps the worst error / bound"""

    def __init__(self, what):
        self.what, self.bad, self.top = what, [], 0.0

    def within(self, got, want, bound, what):
        got = np.asarray(got, dtype=np.float64)
        want, bound = np.broadcast_to(np.asarray(want), got.shape), np.broadcast_to(np.asarray(bound), got.shape)
        if not np.all(np.isfinite(np.asarray(bound, dtype=np.float64))):      # (an infinite bound would pass anything)
            self.bad.append('%s: the restatement has no finite bound in %d cells' % (what, int((~np.isfinite(np.asarray(bound, dtype=np.float64))).sum())))
            return
        nan = np.isnan(np.asarray(want, dtype=np.float64))
        if not np.array_equal(np.isnan(got), nan):
            self.bad.append('%s: NaN in %d cells, the reference has it in %d' % (what, int(np.isnan(got).sum()), int(nan.sum())))
            return
        if nan.all():
            return
        q = hp.worst(got[~nan], want[~nan], hp.SLACK * bound[~nan])
        self.top = max(self.top, q)
        if not q <= 1.0:
            i, g, w, bd = hp.worst_at(got[~nan], want[~nan], hp.SLACK * bound[~nan])
            self.bad.append('%s: error / bound %.3g at %d of %s (got %r, want %r, bound %.3g)' % (what, q, i, got.shape, g, float(w), float(bd)))


def compare(chk, name, kind, driver, keep, got, refs):
    """every cell of every posterior, logEvidence, local_evidence and the means of the chains `keep` against their references"""
    T = steps_of(driver)
    full = driver != 'forward'
    for k, b in enumerate(keep):
        ref = refs[b]
        w = '%s %s %s chain %d %r' % (name, kind, driver, b, CASES[name]['chains'][b])
        chk.within([got['log_evidence'][k]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
        for t in range(T):
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            if np.isfinite(float(loc[1])) or np.isnan(float(loc[0])):
                chk.within([got['local_evidence'][k][t]], [loc[0]], [loc[1]], w + ' localEvidence[%d]' % t)
            else:
                chk.bad.append(w + ' localEvidence[%d]: the restatement has no finite bound' % t)
            want = ref['post'][t] if full else ref['alpha'][t]
            chk.within(got['posts'][k][t], want[0], want[1], w + ' posterior[%d]' % t)
            chk.within(got['means'][k][:, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)


# ---- which of the watched instantiations a case launches, per driver (asserted exactly by tests/test_step_transitions.py) --------------------------
# One rule per family; {p}: the pass as 0 / 1, {b}: as false / true.  A forward-only fit launches the forward ones alone.  The launch-per-step
# families send the steps without a stencil -- step 0 forward, the last step backward -- to the streaming kernel of radius bucket 0.

def _kernels(case):
    name, fam, shape = case['name'], case['family'], case['shape']
    stream = 'blf::fast_step_kernel<100, {p}, 0, false, false>'
    h = 'true' if sum(m[0] == 'walk' for m in case['models']) == 2 and fam in ('fast', 'mfma') else 'false'
    bucket = next((int(x[4:]) for x in name.split('_') if x.startswith('band')), 0)
    if fam == 'generic':
        composed = ['blk::step_kernel<100, 2, false>', 'blk::step_kernel<100, 3, false>'] if 'composed' in name else []
        return dict(forward=['blk::step_kernel<100, 0, true>'], full=['blk::step_kernel<100, 0, false>', 'blk::step_kernel<100, 1, true>'] + composed)
    if fam == 'nd':             # the fused step kernel behind one launch per pass of the transition: a filter per walk, three per NotEqual, one per shift
        kinds = {m[0] for m in case['models']}
        stages = (['bln::filter_axis_kernel'] if 'walk' in kinds else []) + (['bln::shift_axis_kernel'] if 'shift' in kinds else []) + \
                 (['bln::ne_max_kernel', 'bln::ne_invert_kernel', 'bln::ne_clamp_kernel'] if 'ne' in kinds else [])
        return ['bln::step_kernel<{b}>'] + stages
    if fam == 'chain_nd':       # one launch per pass, nothing else
        return ['bln::chain_nd_kernel<{b}, %d>' % chain_nd_threads(case)]
    if fam == 'chain1d_long':   # (M, CL) as launch_chain1d_long picks them: a shift keeps one cell per thread; a clamp is CL = 2
        kinds = {m[0] for m in case['models']}
        shift, clamp = 'shift' in kinds, bool(kinds & {'rs', 'ne'})
        return ['bl1c::chain1d_long_kernel<{b}, %d, %d>' % (1 if shift else 2, 2 if clamp else (1 if shift else 0))]
    if fam == 'chain1d':
        cl = 1 if any(m[0] == 'shift' for m in case['models']) else (2 if any(m[0] in ('rs', 'ne') for m in case['models']) else 0)
        return ['bl1c::chain1d_kernel<100, {b}, %d, %d>' % (1 if shape[0] <= 512 else 2, cl)]
    if fam in ('fused1d', 'persist1d'):
        return ['bl1%s::%s_kernel<100, {b}>' % (fam[0], fam)]
    if fam == 'fast':
        return [stream, 'blf::fast_step_kernel<100, {p}, %d, %s, false>' % (bucket, h)]
    if fam == 'mfma':
        return [stream, 'blm::mfma_step_kernel<100, {p}, %d, false, %s, %s>' % ((16 + 2 * bucket) // 4, h, 'true' if 'lean' in name else 'false')]
    if fam == 'hwide':          # (40 x 300: the chains with a walk on the first parameter take the band kernel behind the pre-pass)
        return [stream, 'blh::hwide_kernel'] + (['blm::mfma_step_kernel<100, {p}, 8, false, false, false>'] if ('walk', 0) in case['models'] else [])
    if fam == 'vwide':
        return [stream, 'blh::vwide_kernel']
    if fam == 'resident':
        return ['blr::resident_kernel<32, 32, 8, 8, {b}, 0, false, true>']
    if fam == 'chain':
        return ['blc::chain_kernel<8, 1, {b}, true, false, true>']
    if fam == 'chainax':
        return ['blc::chainax_kernel<8, 1, {b}, true, true>']
    raise ValueError(fam)


def expected(name, driver):
    k = _kernels(CASES[name])
    if isinstance(k, dict):
        return set(k['forward' if driver == 'forward' else 'full'])
    passes = [(0, 'false')] if driver == 'forward' else [(0, 'false'), (1, 'true')]
    return {f.format(p=p, b=b) for f in k for p, b in passes}


EXPECT = {name: {d: expected(name, d) for d in c['drivers']} for name, c in CASES.items()}
