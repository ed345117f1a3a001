"""
Chain batches on grids with three and four parameters: the cases of the chain-resident kernel bln::chain_nd_kernel
(bayesloop_amd/csrc/blhip_chain_nd.hpp), in the vocabulary of tests/cases.py.

A batch takes the kernel by default from CHAIN_ND_MIN_CHAINS = 16 chains on (a 4 x 4 hyper-grid, a change-point study over 16 time
stamps) where the cost model of bln::chain_nd_route expects it to be faster -- at 16 chains: grids of up to ~5000 cells --; option
chain_nd = 2 takes it wherever it fits, 0 never.  A batch with a walk whose radius exceeds its axis keeps the plain path by default.  A case states the options it is fitted under (`opts`) and the kernel id it must
report (`variant`) where they are not the defaults.  Shapes: the smallest at which the kernel can still go wrong --
3 x 7 x 5 = 105 cells (fewer cells than threads), 5 x 18 x 14 = 1260 (the block of 256 threads, 5 cells per thread, a partial last
round), 3 x 3 x 7 x 6 = 378 (four parameters), 4 x 16 x 147 = 9408 cells (the largest grid of that family the LDS envelope admits with two
walks: the block of 1024 threads; with radii up to 47 it fills the 150 KB but for one double) and 4 x 16 x 148 = 9472 (the first it
refuses: plain path).  T = 1 .. 6; 17 for the change-point study.
"""
import numpy as np

from nd_transition_cases import J4, t3

MIN_CHAINS = 16           # bln::CHAIN_ND_MIN_CHAINS
VARIANT = 10              # fwd_ / bwd_kernel_variant of a chain-resident N-D batch
PLAIN = 7                 # ... of the plain N-D path
LDS_LIMIT = 150 * 1024 // 8
RED = 7 * 16 + 8          # bln::CHAIN_ND_RED


def lds_doubles(G, lw, npass, n_sum):
    """bln::chain_nd_lds_doubles: two state buffers, a tap slot of the widest radius per walk, the grid values, the reduction scratch"""
    return 2 * G + npass * (lw + 1) + n_sum + RED


def lattice(om, name):
    """lattice constant of a parameter of an observation-model spec (cint: end points included; oint: excluded)"""
    kind, a, b, n = dict(om[1])[name]
    return (b - a) / (n - 1) if kind == 'cint' else (b - a) / (n + 1)


def radius(sigma, lat):
    return int(4.0 * sigma / lat + 0.5)          # transitionModels.py:108-111


def cells(om, name, k):
    """sigma of a walk on `name` whose radius is k cells (k + 0.2 cells / 4: well inside the rounding interval)"""
    return [float((kk + 0.2) / 4.0 * lattice(om, name)) if kk else 0.0 for kk in np.atleast_1d(k)]


T3 = t3()                 # 5 x 18 x 14
SMALL = t3(3, 7, 5)       # 105 cells
LARGEST = t3(4, 16, 147)  # 9408 cells: 2 G + 2 (47 + 1) + 167 + 120 = 19 199 doubles of the 19 200
REFUSED = t3(4, 16, 148)  # 9472 cells: 2 G + 2 (3 + 1) + 168 + 120 = 19 240


def _two_walks(om, first, last, k_first=(1, 2, 3, 1), k_last=(2, 1, 3, 2)):
    return ('Combined', [('GRW', 's_' + first, cells(om, first, k_first), first, None), ('GRW', 's_' + last, cells(om, last, k_last), last, None)])


# prior without mass on df < 5.5: the Student-t likelihood of the data point 1e80 is 0 wherever df >= 3.75 (1e80 ** -(df + 1) underflows)
# and ~1e-240 on the row df = 2, so the chain that never leaves its cells (sigma = 0) has the normaliser 0 at that step; the chains that
# walk along df (radius >= 2: two steps carry 1e-4 and more of the mass to df = 2) do not.  No chain's numbers come near the denormals:
# a likelihood that is tiny but not 0 under a denormal posterior cell would make sum(post / L) depend on the host's denormal handling.
_P = np.ones((5, 18, 14))
_P[:3] = 0.0
DEAD_PRIOR = ('array', _P.tolist())
_X = np.array([0.3, -0.4, 1e80, 0.2, 0.5])

ND = {
    # ---- 16 chains: the default route --------------------------------------------------------------------------------------------
    # walks on the first and the last axis, different radii within the batch
    'cnd_hyper_first_last': dict(study='HyperStudy', data=('series', 201, 6), om=T3, tm=_two_walks(T3, 'df', 'scale', (0, 1, 2, 3), (1, 2, 4, 6))),
    # the middle axis: sigma = 0 among the values, radii up to 23 cells on the axis of 18 (multi-period reflection: 40 > 2 x 18)
    'cnd_hyper_middle': dict(study='HyperStudy', data=('series', 202, 5), om=T3,
                             tm=('GRW', 's_loc', cells(T3, 'loc', [0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 17, 18, 19, 23, 40]), 'loc', None),
                             opts=dict(chain_nd=2)),
    'cnd_hyper_middle_default': dict(study='HyperStudy', data=('series', 202, 5), om=T3,
                                     tm=('GRW', 's_loc', cells(T3, 'loc', [0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 17, 18, 19, 23, 40]), 'loc', None), variant=PLAIN),
    # three walks, list order scale, df, loc
    'cnd_three_walks': dict(study='HyperStudy', data=('series', 203, 5), om=T3,
                            tm=('Combined', [('GRW', 's_scale', cells(T3, 'scale', [1, 3, 0, 16]), 'scale', None),
                                             ('GRW', 's_df', cells(T3, 'df', [1, 7]), 'df', None), ('GRW', 's_loc', cells(T3, 'loc', [2, 5]), 'loc', None)]),
                            opts=dict(chain_nd=2)),
    'cnd_small_grid': dict(study='HyperStudy', data=('series', 204, 6), om=SMALL, tm=_two_walks(SMALL, 'df', 'loc', (0, 1, 4, 9), (1, 2, 8, 3)), opts=dict(chain_nd=2)),
    'cnd_small_grid_default': dict(study='HyperStudy', data=('series', 204, 6), om=SMALL, tm=_two_walks(SMALL, 'df', 'loc', (0, 1, 2, 3), (1, 2, 7, 3))),
    'cnd_four_parameters': dict(study='HyperStudy', data=('series', 205, 5), om=J4, tm=_two_walks(J4, 'b', 'loc', (0, 1, 2, 4), (1, 2, 3, 8)), opts=dict(chain_nd=2)),
    'cnd_four_parameters_default': dict(study='HyperStudy', data=('series', 205, 5), om=J4, tm=_two_walks(J4, 'b', 'loc', (0, 1, 2, 3), (1, 2, 3, 7))),
    'cnd_largest': dict(study='HyperStudy', data=('series', 206, 3), om=LARGEST, tm=_two_walks(LARGEST, 'df', 'scale', (0, 1, 2, 3), (1, 2, 3, 47)),
                        opts=dict(chain_nd=2)),
    'cnd_largest_middle': dict(study='HyperStudy', data=('series', 207, 3), om=LARGEST, tm=_two_walks(LARGEST, 'loc', 'scale', (1, 2, 3, 0), (1, 3, 2, 1)),
                               fit=dict(evidenceOnly=True), opts=dict(chain_nd=2)),
    # the same batch under the default option: 16 chains of 9408 cells were measured slower on the kernel, the cost model keeps them plain
    'cnd_largest_default': dict(study='HyperStudy', data=('series', 207, 3), om=LARGEST, tm=_two_walks(LARGEST, 'loc', 'scale', (1, 2, 3, 0), (1, 3, 2, 1)),
                                variant=PLAIN),
    'cnd_refused': dict(study='HyperStudy', data=('series', 208, 3), om=REFUSED, tm=_two_walks(REFUSED, 'df', 'scale', (0, 1, 2, 3), (1, 2, 3, 3)),
                        variant=PLAIN, opts=dict(chain_nd=2)),
    # radius 48 on the largest grid: 2 G + 2 (48 + 1) + 167 + 120 doubles are 8 bytes too many
    'cnd_refused_radius': dict(study='HyperStudy', data=('series', 209, 3), om=LARGEST, tm=_two_walks(LARGEST, 'df', 'scale', (0, 1, 2, 3), (1, 2, 3, 48)),
                               variant=PLAIN, opts=dict(chain_nd=2)),
    # restarts: 'all' change points include the first and the last time stamp (16 candidates on T = 17)
    'cnd_changepoints_all': dict(study='ChangepointStudy', data=('series_jump', 210, 17, 9, 1.5), om=T3, tm=('ChangePoint', 'tc', 'all', None), store='sparse',
                                 opts=dict(chain_nd=2)),       # (no walk: one plain launch per step; the cost model keeps 16 such chains there)
    'cnd_changepoint_then_walk': dict(study='HyperStudy', data=('series_jump', 211, 6, 3, -1.5), om=T3,
                                      tm=('Combined', [('ChangePoint', 'tc', [0, 1, 3, 4], None), ('GRW', 's_loc', cells(T3, 'loc', [0, 1, 3, 20]), 'loc', None)]),
                                      opts=dict(chain_nd=2)),
    'cnd_walk_then_changepoint': dict(study='HyperStudy', data=('series_jump', 212, 6, 3, 1.5), om=T3,
                                      tm=('Combined', [('GRW', 's_scale', cells(T3, 'scale', [1, 2, 3, 0]), 'scale', None), ('ChangePoint', 'tc', [1, 2, 4, 5], None)])),
    'cnd_independent': dict(study='HyperStudy', data=('series', 213, 5), om=T3,
                            tm=('Serial', [('GRW', 's_loc', cells(T3, 'loc', [1, 2, 3, 4]), 'loc', None), ('BreakPoint', 'tb', [1, 2, 3, 4], None), ('Independent',)])),
    # chains of one batch in different segments at the same step; a segment with a walk, a static one, one with two walks
    'cnd_serial_segments': dict(study='HyperStudy', data=('series_jump', 214, 6, 3, 1.5), om=T3,
                                tm=('Serial', [('GRW', 's_loc', cells(T3, 'loc', [1, 3]), 'loc', None), ('BreakPoint', 'b1', [1, 2], None), ('Static',),
                                               ('ChangePoint', 'b2', [3, 4], None), _two_walks(T3, 'df', 'scale', (1, 2), (2,))])),
    # modes and shapes
    # (T = 1: no transition is ever applied -- step 0 consumes the prior, the backward pass the flat distribution --, so the cost model sees
    #  a batch without walks and keeps its 16 chains on the plain path: the kernel takes it under chain_nd = 2)
    'cnd_t1': dict(study='HyperStudy', data=('series', 215, 1), om=T3, tm=_two_walks(T3, 'df', 'loc'), opts=dict(chain_nd=2)),
    'cnd_t1_default': dict(study='HyperStudy', data=('series', 215, 1), om=T3, tm=_two_walks(T3, 'df', 'loc'), variant=PLAIN),
    'cnd_t2': dict(study='HyperStudy', data=('series', 216, 2), om=T3, tm=_two_walks(T3, 'loc', 'scale')),
    'cnd_missing_data': dict(study='HyperStudy', data=('series_nan', 217, 6, [0, 2, 3]), om=T3, tm=_two_walks(T3, 'df', 'loc')),
    'cnd_forward_only': dict(study='HyperStudy', data=('series', 218, 5), om=T3, tm=_two_walks(T3, 'loc', 'scale'), fit=dict(forwardOnly=True)),
    'cnd_evidence_only': dict(study='HyperStudy', data=('series', 219, 5), om=T3, tm=_two_walks(T3, 'df', 'scale'), fit=dict(evidenceOnly=True)),
    'cnd_largest_forward_only': dict(study='HyperStudy', data=('series', 220, 3), om=LARGEST, tm=_two_walks(LARGEST, 'df', 'loc', (1, 2, 3, 0), (3, 2, 1, 1)),
                                     fit=dict(forwardOnly=True), opts=dict(chain_nd=2)),
    # one chain of the batch (sigma_df = 0) has the normaliser 0 at step 2, its neighbours stay healthy
    'cnd_dead_chain': dict(study='HyperStudy', data=_X, om=T3[:2] + (DEAD_PRIOR,),
                           tm=('GRW', 's_df', cells(T3, 'df', [0, 2, 3, 2.5, 3.5, 4, 4.5, 5, 6, 7, 8, 9, 10, 11, 12, 13]), 'df', None),
                           opts=dict(chain_nd=2)),
}

# one chain fewer than the floor: the plain path by default, the kernel under chain_nd = 2
BELOW = {
    'cnd_fifteen_chains': dict(study='HyperStudy', data=('series', 221, 5), om=T3, tm=_two_walks(T3, 'df', 'scale', (0, 1, 2), (1, 2, 3, 4, 6))),
}

# plain studies under chain_nd = 2: a single chain, its posteriors handed out
FORCED = {
    'cnd_single_study': dict(study='Study', data=('series', 222, 6), om=T3,
                             tm=('Combined', [('GRW', 's_scale', cells(T3, 'scale', 2)[0], 'scale', None), ('GRW', 's_df', cells(T3, 'df', 1)[0], 'df', None)])),
    'cnd_single_study_four_parameters': dict(study='Study', data=('series', 223, 5), om=J4, tm=('GRW', 's_loc', cells(J4, 'loc', 3)[0], 'loc', None)),
}

# 35 chains for the batch-split test: max_batch = 16 -> 16 + 16 + 3 (two resident batches and a remainder below the floor)
SPLIT = dict(study='HyperStudy', data=('series', 224, 5), om=T3, tm=_two_walks(T3, 'df', 'loc', (0, 1, 2, 3, 4), (1, 2, 3, 4, 6, 8, 12)))

# fixtures written by the reference itself (tests/golden/gen_chain_nd_golden.py)
GOLDEN = ['cnd_hyper_first_last', 'cnd_changepoints_all']

