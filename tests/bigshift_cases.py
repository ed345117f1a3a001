"""
Study specs (tests/cases.py's DSL) of Deterministic models that shift the distribution by MORE than 12 grid cells per time step on grids
with two parameters: the device runs such a shift as a stage of its own, blk::bigshift_kernel (DESIGN.md "Large shifts on 2-D grids").
Fixtures: tests/golden/gen_bigshift_golden.py; tests: tests/test_bigshift_oracle.py (CPU), tests/test_bigshift.py (GPU).

The specs live here, not in cases.CASES: the existing parity tests are parametrised over that dict.  Only the drift functions are added
to cases.FUNCS (new keys), because cases.make_tm and the oracle adapter look them up there.

Every drift but those of the two crossing cases is slope * t, so a step shifts by slope / lattice constant cells.  The likelihood pulls
the distribution back at every step:
the mass stays inside the grid and the renormalising sum stays O(1) -- none of the ill-conditioning DETERMINISTIC_FUZZ / COAL_NOISE_CHAINS
(tests/tolerances.py) exist for.  Every case takes the registered FFT_FLOOR (the reference's own spline round-off).
"""
import numpy as np

import cases
from tolerances import FFT_TOL


# slope * t, the slope being the model's hyper-parameter (the reference reads names and values off the defaults)
def _bs_mean(t, slope_m=0.5):
    return slope_m * t


def _bs_std(t, slope_s=0.25):
    return slope_s * t


def _bs_mean_mixed(t, slope_m=np.array([0.0, 0.1, 0.5, -0.7])):
    return slope_m * t


def _bs_std_ragged(t, slope_s=0.6):
    return slope_s * t


def _bs_mean_long(t, slope_m=0.03):
    return slope_m * t


def _bs_std_long(t, slope_s=0.03):
    return slope_s * t


def _bs_mean_small(t, slope_m=0.25):
    return slope_m * t


def _bs_mean_direct(t, slope_m=0.7):
    return slope_m * t


# accel * t^2: a step from t to t + 1 shifts by accel (2 t + 1) -- fewer than 12 cells early in the series, more later
def _bs_mean_cross(t, accel_m=0.045):
    return accel_m * t ** 2


def _bs_mean_cross_hyper(t, accel_m=np.array([0.03, 0.045, 0.07])):
    return accel_m * t ** 2


for _f in (_bs_mean, _bs_std, _bs_mean_mixed, _bs_std_ragged, _bs_mean_long, _bs_std_long, _bs_mean_small, _bs_mean_direct, _bs_mean_cross,
           _bs_mean_cross_hyper):
    cases.FUNCS.setdefault(_f.__name__[1:], _f)

# (the std axis starts at 0.1, not 0: no denormal likelihood cells, every number is held to the bar -- tests/combined_cases.py: G2)
# mean: 6 / 199 per cell -> slope 0.5 = 16.6 cells;  std: 2.9 / 181 per cell -> slope 0.25 = 15.6 cells
G2 = ('Gaussian', [('mean', ('cint', -3, 3, 200)), ('std', ('oint', 0.1, 3, 180))], 'default')
# partial line groups, the last block: 203 x 77; slope 0.5 on mean = 16.8 cells, 0.6 on std = 16.1
G_RAGGED = ('Gaussian', [('mean', ('cint', -3, 3, 203)), ('std', ('oint', 0.1, 3, 77))], 'default')
# the envelope's upper end: 4096 x 8, slope 0.03 on mean = 20.5 cells;  8 x 4096, slope 0.03 on std = 42.4 cells
G_LONG0 = ('Gaussian', [('mean', ('cint', -3, 3, 4096)), ('std', ('oint', 0.3, 3, 8))], 'default')
G_LONG1 = ('Gaussian', [('mean', ('cint', -3, 3, 8)), ('std', ('oint', 0.1, 3, 4096))], 'default')
G_LAPLACE = ('Laplace', [('mean', ('cint', -3, 3, 200)), ('std', ('oint', 0.1, 3, 180))], 'default')
# OnlineStudy: 150 x 30 (its golden holds every step's full posterior), slope 0.5 on mean = 12.4 cells
G_ONLINE = ('Gaussian', [('mean', ('cint', -3, 3, 150)), ('std', ('oint', 0.1, 3, 30))], 'default')

DET_MEAN, DET_STD = ('Deterministic', 'bs_mean', 'mean'), ('Deterministic', 'bs_std', 'std')
SERIAL = lambda b1, b2: ('Serial', [('Static',), ('BreakPoint', 'b1', b1, None), DET_MEAN, ('BreakPoint', 'b2', b2, None),   # noqa: E731
                                    ('GRW', 's', 0.3, 'mean', None)])


def _case(seed, tm, om=G2, T=6, study='Study', fit=None, axes=(0,)):
    c = dict(study=study, data=('series', seed, T), om=om, tm=tm, tol=FFT_TOL, axes=axes)
    if fit:
        c['fit'] = fit
    return c


# 'axes': the internal axes (0 = first parameter: columns of the grid array; 1 = second: rows) whose large-shift kernel must run
BIGSHIFT = {
    'bigshift_axis0': _case(201, DET_MEAN),
    'bigshift_axis1': _case(202, DET_STD, axes=(1,)),
    'bigshift_two_axes': _case(203, ('Combined', [DET_STD, DET_MEAN]), axes=(0, 1)),
    'bigshift_walk_then_shift': _case(204, ('Combined', [('GRW', 's', 0.3, 'mean', None), DET_MEAN])),
    'bigshift_shift_walk_rs': _case(205, ('Combined', [DET_STD, ('GRW', 's', 0.2, 'mean', None), ('RS', 'p', -6, None)]), axes=(1,)),
    'bigshift_hyper_mixed': _case(206, ('Combined', [('GRW', 's', [0.2, 0.4], 'mean', None), ('Deterministic', 'bs_mean_mixed', 'mean')]),
                                  study='HyperStudy'),
    'bigshift_serial': _case(207, SERIAL(2, 4)),
    'bigshift_changepoints': _case(208, SERIAL('all', 'all'), T=7, study='ChangepointStudy'),
    'bigshift_forward_only': _case(201, DET_MEAN, fit=dict(forwardOnly=True)),
    'bigshift_evidence_only': _case(201, DET_MEAN, fit=dict(evidenceOnly=True)),
    'bigshift_ragged0': _case(209, DET_MEAN, om=G_RAGGED),
    'bigshift_ragged1': _case(210, ('Deterministic', 'bs_std_ragged', 'std'), om=G_RAGGED, axes=(1,)),
    'bigshift_long0': _case(211, ('Deterministic', 'bs_mean_long', 'mean'), om=G_LONG0, T=3, fit=dict(evidenceOnly=True)),
    'bigshift_long1': _case(212, ('Deterministic', 'bs_std_long', 'std'), om=G_LONG1, T=3, fit=dict(evidenceOnly=True), axes=(1,)),
    'bigshift_laplace': _case(213, ('Combined', [('GRW', 's', 0.3, 'mean', None), DET_MEAN]), om=G_LAPLACE),
    # a drift that crosses 12 cells per step DURING the series: accel 0.045 on mean = 1.4925 (2 t + 1) cells, i.e. 1.5, 4.5, 7.5, 10.4,
    # 13.4, 16.4, 19.4 -- steps of the fused kernel's stencil and steps with the large-shift stage in ONE program, forward and backward;
    # the hyper-study's chains (0.995, 1.4925, 2.32 cells x (2 t + 1)) cross at the last step, at the fifth and at the fourth
    'bigshift_crossing': _case(215, ('Deterministic', 'bs_mean_cross', 'mean'), T=8),
    'bigshift_crossing_hyper': _case(216, ('Deterministic', 'bs_mean_cross_hyper', 'mean'), T=8, study='HyperStudy'),
}
CROSSING = ('bigshift_crossing', 'bigshift_crossing_hyper')

# the control: 8.3 cells per step -- the small-shift stencil inside the fused step kernel, no stage, no large-shift kernel
CONTROL = {'bigshift_small_control': _case(214, ('Deterministic', 'bs_mean_small', 'mean'), axes=())}

ONLINE = {'bigshift_online': dict(om=G_ONLINE, models=[('static', ('Static',)),
                                                       ('walk_drift', ('Combined', [('GRW', 'sm', 0.2, 'mean', None), DET_MEAN]))],
                                  data=('series', 301, 8))}


# ---- the built-in model's own computeForwardPrior / computeBackwardPrior on a 2-D grid, called directly (one-step device programs),
#      as tests/plugin_models.py: direct_calls does for the other models -------------------------------------------------------------------
DIRECT_CALLS = [('fwd', 'norm', 3), ('fwd', 'raw', 3), ('bwd', 'raw', 4), ('bwd', 'norm', 2)]


def direct_calls(bl):
    """name -> (study the model is attached to, model): mean 120 points, slope 0.7 = 13.9 cells;  std 150 points, slope 0.25 = 13.0 cells"""
    def study(n_mean, n_std):
        S = bl.Study(silent=True)
        S.loadData(cases.series(9, 12), silent=True)
        S.setObservationModel(bl.om.Gaussian('mean', bl.cint(-3, 3, n_mean), 'std', bl.oint(0.1, 3, n_std)), silent=True)
        return S
    return {'direct_axis0': (study(120, 20), bl.tm.Deterministic(cases.FUNCS['bs_mean_direct'], target='mean')),
            'direct_axis1': (study(16, 150), bl.tm.Deterministic(cases.FUNCS['bs_std'], target='std'))}


def distribution(kind, shape, seed=0):
    """a positive distribution with mass everywhere (normalised or not): shifting it moves no mass off the grid's support"""
    rng = np.random.default_rng(7000 + seed)
    x = rng.random(shape) ** 3 + 1e-3
    return x / np.sum(x) if kind == 'norm' else 7.5 * x
