"""
Study specs (tests/cases.py's DSL) of CombinedTransitionModel compositions whose sub-models do not fit into one step of the generic
kernel: the device runs them as stage lists (DESIGN.md "Composed transitions").  Fixtures: tests/golden/gen_combined_golden.py;
tests: tests/test_combined_models_oracle.py (CPU), tests/test_combined_models.py (GPU).

The specs live here, not in cases.CASES: the existing parity tests are parametrised over that dict.  Only the model functions are
added to cases.FUNCS (new keys), because cases.make_tm and the oracle adapter look them up there.
"""
import numpy as np

import cases
from tolerances import FFT_TOL


# ---- the reference's tutorial docs/source/tutorials/hyperparameteroptimization.ipynb, second model ----------------------------------
def _slope_1(t, slope_1=-0.2):
    return slope_1 * t


def _slope_2_fn(v):
    def f(t, slope_2=v):
        return slope_2 * t
    return f


# the log10-evidences the notebook prints for S.optimize(['slope_2'])
TUTORIAL_LOG10 = [(0.0, -72.78352), (1.0, -93.84882), (-1.0, -80.98325), (-0.5, -85.81409), (0.25, -82.83302), (-0.125, -73.27797),
                  (-0.046875, -72.54880)]


def _drift_h(t, slope=np.array([0.0, 0.1])):
    return slope * t


def _drift_1d(t, slope=np.array([-0.06, 0.0, 0.09])):
    return slope * t


cases.FUNCS.setdefault('tut_slope_1', _slope_1)
for _k, (_v, _) in enumerate(TUTORIAL_LOG10):
    cases.FUNCS.setdefault('tut_slope_2_%d' % _k, _slope_2_fn(_v))
cases.FUNCS.setdefault('tut_slope_2_cp', _slope_2_fn(-0.05))
cases.FUNCS.setdefault('drift_h', _drift_h)
cases.FUNCS.setdefault('drift_1d', _drift_1d)

COAL_OM = ('Poisson', [('accident_rate', ('oint', 0, 6, 1000))], 'default')


def tutorial_tm(slope_2_fn, first=1885, second=1895):
    return ('Serial', [('Combined', [('GRW', 'early_sigma', 0.05, 'accident_rate', None), ('RS', 'pmin', -7, None)]),
                       ('BreakPoint', 'first_break', first, None),
                       ('Deterministic', 'tut_slope_1', 'accident_rate'),
                       ('BreakPoint', 'second_break', second, None),
                       ('Combined', [('GRW', 'late_sigma', 0.25, 'accident_rate', None),
                                     ('Deterministic', slope_2_fn, 'accident_rate')])])


def _coal_study(study, tm, fit=None, **kw):
    c = dict(study=study, data=cases.COAL, timestamps=cases.COAL_T, om=COAL_OM, tm=tm, tol=FFT_TOL,
             store='sparse')
    if fit:
        c['fit'] = fit
    c.update(kw)
    return c


# (the std axis starts at 0.1, not 0: with std values near 0 the likelihood has DENORMAL cells, where the reference's own backward
#  localEvidence -- 1 / sum(post / L), core.py:463 -- is defined to a few digits only (tests/tolerances.py: ILL_LOCAL_EVIDENCE); this
#  grid keeps every likelihood value above 1e-138, so every number of these cases is held to the bar)
G2 = ('Gaussian', [('mean', ('cint', -3, 3, 48)), ('std', ('oint', 0.1, 3, 36))], 'default')


def _g2(seed, tm, T=12, fit=None, tol=None, study='Study'):
    c = dict(study=study, data=('series', seed, T), om=G2, tm=tm)
    if fit:
        c['fit'] = fit
    if tol:
        c['tol'] = tol
    return c


COMBINED = {}
# 1. the tutorial model: evidence at the seven published slope_2 values; full fits at 7.8 cells per step (small-shift stencil) and at
#    41.7 cells (the two-stage large shift)
for _k, (_v, _) in enumerate(TUTORIAL_LOG10):
    COMBINED['comb_tutorial_evidence_%d' % _k] = _coal_study('Study', tutorial_tm('tut_slope_2_%d' % _k), fit=dict(evidenceOnly=True))
# (slope_2 = 0: the Deterministic step is the identity, so the program stays single-stage: no stage kernel)
COMBINED['comb_tutorial_evidence_0']['single_stage'] = True
COMBINED['comb_tutorial_full_small_shift'] = _coal_study('Study', tutorial_tm('tut_slope_2_6'))
COMBINED['comb_tutorial_full_large_shift'] = _coal_study('Study', tutorial_tm('tut_slope_2_4'))
# 2. a change-point study over the tutorial's break-points (49 chains)
COMBINED['comb_tutorial_breakpoints'] = _coal_study('ChangepointStudy', tutorial_tm('tut_slope_2_cp', ('arange', 1882, 1889, 1),
                                                                                    ('arange', 1892, 1899, 1)))
# 3. 1-D hyper-study: walk + Deterministic on one parameter, the slope grid holds 0 (single-stage chains next to two-stage ones)
COMBINED['comb_hyper_1d'] = dict(study='HyperStudy', data=('coal', 40), om=('Poisson', [('rate', ('oint', 0, 6, 200))], 'default'),
                                 tm=('Combined', [('GRW', 's', [0.05, 0.2], 'rate', None), ('Deterministic', 'drift_1d', 'rate')]), tol=FFT_TOL)
# 4. one 2-D Gaussian study per kind of composition the single-stage program refuses
COMBINED['comb2d_walk_rs_walk'] = _g2(101, ('Combined', [('GRW', 's1', 0.2, 'mean', None), ('RS', 'p', -4, None), ('GRW', 's2', 0.3, 'mean', None)]))
COMBINED['comb2d_walk_alphastable'] = _g2(102, ('Combined', [('GRW', 's', 0.25, 'mean', None), ('AlphaStable', 'c', 0.15, 'alpha', 1.5, 'std')]), tol=FFT_TOL)
COMBINED['comb2d_bivariate_walk'] = _g2(103, ('Combined', [('Bivariate', 's1', 0.3, 's2', 0.15, 'rho', 0.4), ('GRW', 's', 0.2, 'std', None)]))
COMBINED['comb2d_det_then_walk'] = _g2(104, ('Combined', [('Deterministic', 'drift', 'mean'), ('GRW', 's', 0.3, 'mean', None)]), tol=FFT_TOL)
COMBINED['comb2d_two_walks'] = _g2(105, ('Combined', [('GRW', 's1', 0.2, 'mean', None), ('GRW', 's2', 0.3, 'mean', None)]))
COMBINED['comb2d_walk_then_det'] = _g2(106, ('Combined', [('GRW', 's', 0.3, 'mean', None), ('Deterministic', 'drift', 'mean')]), tol=FFT_TOL)
COMBINED['comb2d_walk_then_det_forward'] = _g2(106, ('Combined', [('GRW', 's', 0.3, 'mean', None), ('Deterministic', 'drift', 'mean')]),
                                               fit=dict(forwardOnly=True), tol=FFT_TOL)
COMBINED['comb2d_walk_notequal'] = _g2(107, ('Combined', [('GRW', 's', 0.3, 'mean', None), ('NE', 'p', -4, None)]))
COMBINED['comb2d_changepoint_notequal'] = _g2(108, ('Combined', [('ChangePoint', 'tc', 5, None), ('NE', 'p', -4, None)]))
COMBINED['comb2d_two_regimeswitch'] = _g2(109, ('Combined', [('RS', 'p1', -5, None), ('RS', 'p2', -3, None)]))
COMBINED['comb2d_det_then_clamp'] = _g2(110, ('Combined', [('Deterministic', 'drift', 'mean'), ('RS', 'p', -4, None)]), tol=FFT_TOL)
# ... and the stage flavours the cases above apply only in the LAST stage, in front of another stage: the two-stage large shift (41.7 cells
#     per step on a 1-D grid), zero-boundary alpha-stable taps, NotEqual
COMBINED['comb_bigshift_then_walk_1d'] = _coal_study('Study', ('Combined', [('Deterministic', 'tut_slope_2_4', 'accident_rate'),
                                                                            ('GRW', 's', 0.25, 'accident_rate', None)]))
COMBINED['comb2d_alphastable_then_walk'] = _g2(114, ('Combined', [('AlphaStable', 'c', 0.15, 'alpha', 1.5, 'std'), ('GRW', 's', 0.2, 'std', None)]), tol=FFT_TOL)
COMBINED['comb2d_notequal_then_rs'] = _g2(115, ('Combined', [('NE', 'p1', -4, None), ('RS', 'p2', -3, None)]))
# 5. a 2-D hyper-study whose chains have different stage counts at the same step (zero and non-zero shifts)
COMBINED['comb2d_hyper_mixed'] = _g2(111, ('Combined', [('GRW', 's', [0.2, 0.4], 'mean', None), ('Deterministic', 'drift_h', 'mean')]),
                                     study='HyperStudy', tol=FFT_TOL)

# the single-stage control: a composition one step of the generic kernel takes (no stage kernel)
SINGLE_STAGE = {'comb2d_single_walk_rs': _g2(112, ('Combined', [('GRW', 's', 0.3, 'mean', None), ('RS', 'p', -4, None)]))}

# 6. an OnlineStudy with a composed model among the competing ones
ONLINE = {'comb_online_2d': dict(om=G2, models=[('walks', ('Combined', [('GRW', 'sm', 0.2, 'mean', None), ('GRW', 'ss', 0.1, 'std', None)])),
                                                ('walk_ne', ('Combined', [('GRW', 'sm2', 0.2, 'mean', None), ('NE', 'p', -4, None)]))],
                                 data=('series', 113, 30))}

# cases whose model contains a Deterministic or AlphaStable sub-model: the registered FFT_FLOOR (tests/tolerances.py) applies
FFT_CASES = sorted(k for k, c in COMBINED.items() if c.get('tol') is FFT_TOL)
