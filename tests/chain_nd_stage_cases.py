"""
Chain batches with NotEqual and Deterministic models on grids with three and four parameters: the cases of the stage flavour of the
chain-resident kernel (bayesloop_amd/csrc/blhip_chain_nd.hpp: bln::chain_nd_stage_kernel<BWD, 256 | 1024>), in the vocabulary of
tests/cases.py.  All of them are fitted under chain_nd = 2 (tests/test_chain_nd_stages.py); every hyper-study and change-point study has
exactly 16 chains.

Shapes: the smallest at which the kernel can still go wrong -- 5 x 18 x 14 = 1260 cells (the block of 256 threads, five cells per thread,
a partial last round), 3 x 7 x 5 = 105 (fewer cells than threads), 3 x 3 x 7 x 6 = 378 (four parameters), 5 x 24 x 18 = 2160 (the LDS
need exceeds 32 KB: the block of 1024 threads).  T = 5 .. 9; 17 for the break-point study (16 candidates).

Cases with a Deterministic model carry the registered FFT_FLOOR (tests/tolerances.py: FFT_TOL); everything else is compared at the bar.
"""
import numpy as np

import cases
from chain_nd_cases import LDS_LIMIT, RED, cells, lattice
from nd_transition_cases import J4, NE_VALUES, t3
from tolerances import FFT_TOL

CHAINS = 16
VARIANT = 10              # fwd_ / bwd_kernel_variant of a chain-resident N-D batch
PLAIN = 7                 # ... of the plain N-D path
NOTEQUAL_LAUNCHES = 3     # ne_max, ne_invert, ne_clamp (the plain path; the fused step kernel is what `forward_launches` counts)

T3 = t3()                 # 5 x 18 x 14
SMALL = t3(3, 7, 5)       # 105 cells
LARGE = t3(5, 24, 18)     # 2160 cells: 2 G alone are 34 560 bytes


def stage_slot(lw_walk, lw_shift):
    """bln::chain_nd_stage_slot: doubles of a tap slot -- a walk's half kernel, or all 2 lw + 1 weights of a shift"""
    return max(lw_walk + 1, 2 * lw_shift + 1 if lw_shift > 0 else 0)


def stage_lds_doubles(G, slot, npass, n_sum):
    """bln::chain_nd_stage_lds_doubles: two state buffers, one slot per pass, the grid values, the reduction scratch"""
    return 2 * G + npass * max(slot, 1) + n_sum + RED


def stage_threads(G, slot, npass, n_sum):
    return 256 if stage_lds_doubles(G, slot, npass, n_sum) * 8 <= 32 * 1024 else 1024


# log10 pMin over 16 values: from one clamped cell per step (the maximum: NE_VALUES[0]) over a share of the grid (NE_VALUES[1]) to every
# cell (NE_VALUES[2] and above); tests/test_chain_nd_stages_host.py asserts the three regimes on the oracle's posteriors
NE16 = [-6., -5.5, -5., -4.5, -4., -3.5, -3., -2.8, -2.6, -2.4, -2.3, -2.2, -2.1, -2.0, -1.9, -1.8]
assert len(NE16) == CHAINS and set(NE_VALUES) <= set(NE16)

# shifts per step in grid cells: zero (the identity: no stage), below one cell, close to but not above 12 in both directions
SHIFT_CELLS = [0., 0.3, -0.6, 1., -1.5, 2.5, -3., 4.2, -5., 6.5, -7.5, 9., -10., 11.2, -11.6, 11.9]
assert len(SHIFT_CELLS) == CHAINS


def _register_drift(name, om, parameter, shift_cells):
    """a linear drift on `parameter` whose slopes shift by `shift_cells` grid cells per step; cases.FUNCS is where both the package's
    and the oracle's builders look a Deterministic model's function up"""
    slopes = np.asarray(shift_cells, dtype=float) * lattice(om, parameter)
    if slopes.size == 1:
        slopes = float(slopes[0])

    def drift(t, slope=slopes):
        return slope * t
    drift.__name__ = name
    cases.FUNCS[name] = drift
    return name


_register_drift('cns_drift_df', T3, 'df', SHIFT_CELLS)
_register_drift('cns_drift_loc', T3, 'loc', SHIFT_CELLS)
_register_drift('cns_drift_scale', T3, 'scale', SHIFT_CELLS)
_register_drift('cns_drift_loc_4', T3, 'loc', [0., 0.4, -2.5, 3.])
_register_drift('cns_drift_scale_1', T3, 'scale', [1.7])
_register_drift('cns_drift_loc_j4', J4, 'loc', [0., 0.5, -1.2, 2.5])
_register_drift('cns_drift_loc_small', SMALL, 'loc', [0., 0.5, -1.5, 2.5])
_register_drift('cns_drift_loc_large', LARGE, 'loc', SHIFT_CELLS)
_register_drift('cns_drift_df_1', T3, 'df', [0.4])

NE4 = [-6., -3., -2.2, -2.0]

ND = {
    # 1. NotEqual alone, the three clamp regimes in one batch
    'cns_notequal': dict(study='HyperStudy', data=('series', 121, 7), om=T3, tm=('NE', 'p_min', NE16, None)),
    # 2. walk - NotEqual - walk on three different axes
    'cns_walk_notequal_walk': dict(study='HyperStudy', data=('series', 301, 6), om=T3,
                                   tm=('Combined', [('GRW', 's_loc', cells(T3, 'loc', [1, 3]), 'loc', None), ('NE', 'p_min', [-5., -3., -2.4, -2.], None),
                                                    ('GRW', 's_df', cells(T3, 'df', [0, 2]), 'df', None)])),
    # 3. two NotEqual in one model, a walk on the last axis between them (the first never clamps every cell: the second would meet a
    #    flat distribution)
    'cns_two_notequal': dict(study='HyperStudy', data=('series', 302, 6), om=T3,
                             tm=('Combined', [('NE', 'p1', [-6., -3., -2.6, -2.3], None), ('GRW', 's_scale', cells(T3, 'scale', 2)[0], 'scale', None),
                                              ('NE', 'p2', [-5., -3.5, -2.2, -1.9], None)])),
    # 4. NotEqual directly after a change point: its input is the shared reset distribution (not a flat one: max - p would be 0 everywhere)
    'cns_changepoint_notequal': dict(study='HyperStudy', data=('series_jump', 303, 8, 4, 1.5), om=T3[:2] + ('inv_s_3d',),
                                     tm=('Combined', [('ChangePoint', 'tc', [1, 2, 4, 6], None), ('NE', 'p_min', NE4, None)])),
    # 5. Deterministic over 16 slopes on the first, the middle and the last axis
    'cns_shift_first': dict(study='HyperStudy', data=('series', 304, 6), om=T3, tm=('Deterministic', 'cns_drift_df', 'df'), tol=FFT_TOL),
    'cns_shift_middle': dict(study='HyperStudy', data=('series', 305, 7), om=T3, tm=('Deterministic', 'cns_drift_loc', 'loc'), tol=FFT_TOL),
    'cns_shift_last': dict(study='HyperStudy', data=('series', 306, 6), om=T3, tm=('Deterministic', 'cns_drift_scale', 'scale'), tol=FFT_TOL),
    # 6. Deterministic, then a walk on another axis
    'cns_shift_walk': dict(study='HyperStudy', data=('series', 307, 6), om=T3,
                           tm=('Combined', [('Deterministic', 'cns_drift_loc_4', 'loc'), ('GRW', 's_scale', cells(T3, 'scale', [0, 1, 2, 4]), 'scale', None)]),
                           tol=FFT_TOL),
    # 7. chains of one batch in different segments at the same step: the stage (and the drift) runs for some, not for the others
    'cns_breakpoints': dict(study='ChangepointStudy', data=('series_jump', 308, 17, 8, -1.5), om=T3,
                            tm=('Serial', [('GRW', 's_loc', 0.3, 'loc', None), ('BreakPoint', 't_break', 'all', None),
                                           ('Combined', [('Deterministic', 'cns_drift_scale_1', 'scale'), ('NE', 'p_min', -3., None)])]),
                            store='sparse', tol=FFT_TOL),
    # 8. modes
    'cns_forward_only': dict(study='HyperStudy', data=('series', 309, 6), om=T3,
                             tm=('Combined', [('GRW', 's_loc', cells(T3, 'loc', [1, 2, 3, 5]), 'loc', None), ('NE', 'p_min', NE4, None)]),
                             fit=dict(forwardOnly=True)),
    'cns_evidence_only': dict(study='HyperStudy', data=('series', 310, 6), om=T3,
                              tm=('Combined', [('NE', 'p_min', NE4, None), ('GRW', 's_scale', cells(T3, 'scale', [0, 1, 2, 3]), 'scale', None)]),
                              fit=dict(evidenceOnly=True)),
    'cns_shift_forward_only': dict(study='HyperStudy', data=('series', 311, 6), om=T3, tm=('Deterministic', 'cns_drift_loc', 'loc'),
                                   fit=dict(forwardOnly=True), tol=FFT_TOL),
    # (no value that clamps every cell: a flat distribution through a step without data stays flat, and max - p is 0 everywhere)
    'cns_missing_data': dict(study='HyperStudy', data=('series_nan', 312, 8, [2, 3, 6]), om=T3,
                             tm=('Combined', [('NE', 'p_min', [-6., -4., -3., -2.4], None), ('GRW', 's_df', cells(T3, 'df', [0, 1, 2, 3]), 'df', None)])),
    # 9. four parameters
    'cns_four_parameters': dict(study='HyperStudy', data=('series', 313, 6), om=J4,
                                tm=('Combined', [('GRW', 's_b', cells(J4, 'b', [0, 1, 2, 3]), 'b', None), ('NE', 'p_min', [-5., -3., -2.2, -1.8], None)])),
    'cns_four_parameters_shift': dict(study='HyperStudy', data=('series', 314, 5), om=J4,
                                      tm=('Combined', [('Deterministic', 'cns_drift_loc_j4', 'loc'), ('NE', 'p_min', [-5., -3., -2.2, -1.8], None)]),
                                      tol=FFT_TOL),
    # 10. 105 cells: fewer cells than threads
    'cns_small_grid': dict(study='HyperStudy', data=('series', 315, 6), om=SMALL,
                           tm=('Combined', [('Deterministic', 'cns_drift_loc_small', 'loc'), ('NE', 'p_min', [-4., -2.5, -1.5, -1.], None)]), tol=FFT_TOL),
    # 11. 2160 cells: the block of 1024 threads
    'cns_large_notequal': dict(study='HyperStudy', data=('series', 316, 5), om=LARGE,
                               tm=('Combined', [('GRW', 's_scale', cells(LARGE, 'scale', [1, 2, 3, 5]), 'scale', None), ('NE', 'p_min', [-6., -3., -2.5, -2.2], None)])),
    'cns_large_shift': dict(study='HyperStudy', data=('series', 317, 5), om=LARGE, tm=('Deterministic', 'cns_drift_loc_large', 'loc'), tol=FFT_TOL),
}

# 12. single studies under chain_nd = 2: one chain, its posteriors handed out
FORCED = {
    'cns_single_study': dict(study='Study', data=('series', 318, 7), om=T3,
                             tm=('Combined', [('GRW', 's_loc', cells(T3, 'loc', 2)[0], 'loc', None), ('NE', 'p_min', -3., None)])),
    'cns_single_study_shift': dict(study='Study', data=('series', 319, 6), om=T3,
                                   tm=('Combined', [('Deterministic', 'cns_drift_df_1', 'df'), ('GRW', 's_scale', cells(T3, 'scale', 1)[0], 'scale', None)]),
                                   tol=FFT_TOL),
}

# 35 chains for the batch-split test: max_batch = 16 -> 16 + 16 + 3
SPLIT = dict(study='HyperStudy', data=('series', 320, 5), om=T3,
             tm=('Combined', [('GRW', 's_loc', cells(T3, 'loc', [0, 1, 2, 3, 5]), 'loc', None), ('NE', 'p_min', [-6., -4., -3., -2.6, -2.3, -2.1, -1.9], None)]))

# OnlineStudy.stepMany on three parameters: a walk over 16 widths and NotEqual over 16 values; 7 points
ONLINE = dict(om=t3(4, 8, 6),
              models=[('walk', ('GRW', 's_loc', cells(t3(4, 8, 6), 'loc', [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 20]), 'loc', None)),
                      ('different', ('NE', 'log10pMin', NE16, None))],
              tm_prior=[0.6, 0.4], data=('series', 321, 7))

ALL = dict(ND, **FORCED, cns_split=SPLIT)


def passes_of(spec):
    """the passes of a model in list order: ('walk' | 'ne' | 'shift', parameter or None)"""
    if spec[0] in ('Combined', 'Serial'):
        return [p for s in spec[1] for p in passes_of(s)]
    return {'GRW': [('walk', spec[3] if spec[0] == 'GRW' else None)], 'NE': [('ne', None)],
            'Deterministic': [('shift', spec[2] if spec[0] == 'Deterministic' else None)]}.get(spec[0], [])


def shift_cells_of(c):
    """every Deterministic model's shifts per step of a case, in grid cells"""
    def models(spec):
        if spec[0] in ('Combined', 'Serial'):
            return [m for s in spec[1] for m in models(s)]
        return [spec] if spec[0] == 'Deterministic' else []
    out = []
    for m in models(c['tm']):
        import inspect
        slope = np.atleast_1d(inspect.getfullargspec(cases.FUNCS[m[1]]).defaults[0])
        out += list(slope / lattice(c['om'], m[2]))
    return out
