"""
NotEqual, Independent, Serial and Deterministic transition models on grids with three and four parameters (the plain N-D path,
bayesloop_amd/csrc/blhip_nd.hpp + blhip_nd_stages.hpp), in the vocabulary of tests/cases.py.

Shapes: the smallest that still exercise something.  5 x 18 x 14 = 1260 cells are 5 blocks of 256 with a partial last one; 3 x 7 x 5 =
105 cells a single partial block; 3 x 3 x 7 x 6 = 378 cells four parameters; T = 5 .. 10; at most 6 chains, but for the break-point
study ('all' on T = 9: 8 chains, which the batch-split test cuts into 3 + 3 + 2).

Cases with a Deterministic model carry the registered FFT_FLOOR (tests/tolerances.py: FFT_TOL); everything else is compared at the bar.
"""
from tolerances import FFT_TOL


def t3(n_df=5, n_loc=18, n_scale=14):
    return ('SciPy:t', [('df', ('cint', 2.0, 9.0, n_df)), ('loc', ('cint', -3.0, 3.0, n_loc)), ('scale', ('oint', 0.2, 2.5, n_scale))], 'default')


J4 = ('SciPy:johnsonsu', [('a', ('cint', -1.0, 1.0, 3)), ('b', ('cint', 0.8, 2.5, 3)), ('loc', ('cint', -2.0, 2.0, 7)),
                         ('scale', ('oint', 0.3, 2.0, 6))], 'default')

# log10 pMin of the NotEqual hyper-study: on its data the oracle's posteriors put ONE cell (the maximum), 8.3 % of the cells and ALL
# cells below the limit (tests/test_nd_transitions_oracle.py asserts the three regimes)
NE_VALUES = [-6., -2.2, -2.0]

ND = {
    'ndt_independent': dict(study='Study', data=('series', 101, 6), om=t3(), tm=('Independent',)),
    'ndt_notequal_hyper': dict(study='HyperStudy', data=('series', 121, 7), om=t3(), tm=('NE', 'p_min', NE_VALUES, None)),
    # walks on different axes in front of and behind the stage
    'ndt_grw_notequal': dict(study='Study', data=('series', 102, 7), om=t3(),
                             tm=('Combined', [('GRW', 's_loc', 0.4, 'loc', None), ('NE', 'p_min', -3., None)])),
    'ndt_notequal_grw': dict(study='HyperStudy', data=('series', 103, 6), om=t3(),
                             tm=('Combined', [('NE', 'p_min', -2.5, None), ('GRW', 's_scale', [0.1, 0.3], 'scale', None)])),
    'ndt_two_notequal': dict(study='Study', data=('series', 104, 6), om=t3(),
                             tm=('Combined', [('NE', 'p1', -3., None), ('GRW', 's_df', 1.5, 'df', None), ('NE', 'p2', -2.2, None)])),
    # NotEqual directly after a restart: its input is the shared reset distribution (not a flat one: max - p would be 0 everywhere)
    'ndt_changepoint_notequal': dict(study='HyperStudy', data=('series_jump', 105, 8, 4, 1.5), om=t3()[:2] + ('inv_s_3d',),
                                     tm=('Combined', [('ChangePoint', 'tc', [2, 5], None), ('NE', 'p_min', -3., None)])),
    # chains of one batch in different segments: the stage runs for some, the others pass through by copy
    'ndt_breakpoints': dict(study='ChangepointStudy', data=('series_jump', 106, 9, 4, -1.5), om=t3(),
                            tm=('Serial', [('GRW', 's_loc', 0.3, 'loc', None), ('BreakPoint', 't_break', 'all', None),
                                           ('Combined', [('GRW', 's_scale', 0.2, 'scale', None), ('NE', 'p_min', -3., None)])])),
    'ndt_serial_hyper': dict(study='HyperStudy', data=('series_jump', 107, 9, 4, 1.5), om=t3(),
                             tm=('Serial', [('Static',), ('ChangePoint', 'tc', [2, 3], None), ('GRW', 's_loc', 0.3, 'loc', None),
                                            ('BreakPoint', 'tb', [5, 6], None), ('Independent',)])),
    # Deterministic: the first, the middle and the last axis
    'ndt_shift_first': dict(study='Study', data=('series', 108, 7), om=t3(), tm=('Deterministic', 'drift', 'df'), tol=FFT_TOL),
    'ndt_shift_middle': dict(study='HyperStudy', data=('series', 109, 7), om=t3(), tm=('Deterministic', 'quadratic', 'loc'), tol=FFT_TOL),
    'ndt_shift_last': dict(study='Study', data=('series', 110, 6), om=t3(), tm=('Deterministic', 'drift', 'scale'), tol=FFT_TOL),
    'ndt_shift_grw': dict(study='Study', data=('series', 111, 7), om=t3(),
                          tm=('Combined', [('Deterministic', 'drift', 'scale'), ('GRW', 's_loc', 0.3, 'loc', None)]), tol=FFT_TOL),
    'ndt_serial_shift': dict(study='HyperStudy', data=('series', 112, 9), om=t3(),
                             tm=('Serial', [('Static',), ('BreakPoint', 'b1', [2, 3], None), ('Deterministic', 'drift', 'loc'),
                                            ('BreakPoint', 'b2', [5, 6], None), ('Static',)]), tol=FFT_TOL),
    'ndt_forward_only': dict(study='Study', data=('series', 113, 7), om=t3(),
                             tm=('Combined', [('GRW', 's_loc', 0.4, 'loc', None), ('NE', 'p_min', -3., None)]), fit=dict(forwardOnly=True)),
    'ndt_shift_forward_only': dict(study='Study', data=('series', 114, 6), om=t3(), tm=('Deterministic', 'drift', 'loc'),
                                   fit=dict(forwardOnly=True), tol=FFT_TOL),
    'ndt_evidence_only': dict(study='HyperStudy', data=('series', 115, 7), om=t3(),
                              tm=('Combined', [('NE', 'p_min', [-4., -2.5], None), ('GRW', 's_loc', 0.3, 'loc', None)]), fit=dict(evidenceOnly=True)),
    'ndt_missing_data': dict(study='Study', data=('series_nan', 116, 8, [2, 3, 6]), om=t3(),
                             tm=('Combined', [('NE', 'p_min', -3., None), ('GRW', 's_scale', 0.2, 'scale', None)])),
    'ndt_four_parameters': dict(study='HyperStudy', data=('series', 117, 6), om=J4,
                                tm=('Combined', [('GRW', 's_b', 0.4, 'b', None), ('NE', 'p_min', [-4., -2.5], None)])),
    'ndt_four_parameters_shift': dict(study='Study', data=('series', 118, 5), om=J4,
                                      tm=('Serial', [('Deterministic', 'drift', 'loc'), ('BreakPoint', 'tb', 3, None), ('Independent',)]),
                                      tol=FFT_TOL),
    # 105 cells: a single partial block
    'ndt_single_block': dict(study='Study', data=('series', 119, 6), om=t3(3, 7, 5),
                             tm=('Combined', [('Deterministic', 'drift', 'loc'), ('NE', 'p_min', -2.5, None)]), tol=FFT_TOL),
}

ONLINE = {
    'ndt_online': dict(om=t3(4, 8, 6),
                       models=[('static', ('Static',)), ('independent', ('Independent',)),
                               ('different', ('NE', 'log10pMin', [-6., -3.], None)),
                               ('serial', ('Serial', [('GRW', 's_loc', 0.3, 'loc', None), ('BreakPoint', 'tb', 3, None), ('Static',)]))],
                       tm_prior=[0.4, 0.2, 0.2, 0.2], data=('series', 120, 7)),
}

# fixtures written by the reference itself (tests/golden/gen_nd_transition_golden.py)
GOLDEN = ['ndt_notequal_hyper', 'ndt_breakpoints', 'ndt_shift_middle', 'ndt_four_parameters']
GOLDEN_ONLINE = ['ndt_online']

# models refused on grids with more than two parameters
REFUSED = {
    'regimeswitch': ('RS', 'log10pMin', -4, None),
    'alphastable': ('AlphaStable', 'c', 0.2, 'alpha', 1.5, 'loc'),
    'bivariate': ('Bivariate', 'sigma1', 1., 'sigma2', 0.1, 'rho', 0.5),
}
