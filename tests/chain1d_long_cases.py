"""
Cases of the chain-resident 1-D kernel's long-row flavour (bayesloop_amd/csrc/blhip_chain1d.hpp: bl1c::chain1d_long_kernel, rows of 4097 ..
8192 grid points) in the neutral form of tests/cases.py, shared by tests/test_chain1d_long.py (GPU) and tests/test_chain1d_long_host.py
(the oracle alone).  The Deterministic models' functions of time are added to cases.FUNCS (new keys), because cases.make_tm and the
oracle adapter look them up there.

Radii: a GaussianRandomWalk of width sigma on a grid of lattice constant d has the SciPy radius int(4 sigma / d + 0.5)
(transitionModels.py:108-111); `_sigma(r, d)` is the width in the middle of the interval that gives radius r.
"""
import numpy as np

import cases


def _sigma(r, lattice):
    return 0.0 if r == 0 else (r - 0.25) / 4.0 * lattice


def _gm(n):
    return ('GaussianMean', [('mean', ('cint', -4, 4, n))], 'default')


def _poisson(n):
    return ('Poisson', [('rate', ('oint', 0, 6, n))], 'default')


def _bernoulli(n):
    return ('Bernoulli', [('p', ('oint', 0, 1, n))], 'default')


GM_LATTICE = lambda n: 8.0 / (n - 1.0)          # noqa: E731  cint(-4, 4, n)
PO_LATTICE = lambda n: 6.0 / (n + 1.0)          # noqa: E731  oint(0, 6, n)
BE_LATTICE = lambda n: 1.0 / (n + 1.0)          # noqa: E731  oint(0, 1, n)


# ---- Deterministic drifts of the mean on cint(-4, 4, n): cells per step = slope / lattice -------------------------------------------
def _c1l_slow(t, slope=0.008):                  # n = 5000: 5.0 cells per step (asymmetric stencil, <= 12 cells)
    return slope * t


def _c1l_fast(t, slope=0.0304):                 # n = 5000: 19.0 cells per step; n = 6200: 23.6 (two-stage form)
    return slope * t


for _f in (_c1l_slow, _c1l_fast):
    cases.FUNCS.setdefault(_f.__name__[1:], _f)


def _serial(fn, first=('Static',)):
    return ('Serial', [first, ('BreakPoint', 't_break', [3, 5], None), ('Deterministic', fn, 'mean')])


W4097 = [_sigma(r, GM_LATTICE(4097)) for r in (0, 3, 17, 64, 130)]
HYPER4097 = dict(study='HyperStudy', data=('gm', 9801, 8), om=_gm(4097), tm=('GRW', 'sigma', W4097, 'mean', None))

BERNOULLI7 = np.array([1, 0, 1, 1, 0, 1, 1, 0], dtype=float)


def _clamp_models(target, s):
    return {
        'switch_alone': ('RS', 'log10pMin', -4, None),
        'walk_then_switch': ('Combined', [('GRW', 's', s, target, None), ('RS', 'log10pMin', -5, None)]),
        'switch_then_walk': ('Combined', [('RS', 'log10pMin', -5, None), ('GRW', 's', s, target, None)]),
        'not_equal': ('NE', 'log10pMin', -6, None),
    }


def _clamp_hyper(target, lattice):
    """six chains over (width, pMin)"""
    return ('Combined', [('GRW', 's', [_sigma(r, lattice) for r in (2, 9, 31)], target, None), ('RS', 'log10pMin', [-7, -4], None)])


CLAMP_N = 4500
CLAMP_STUDY = {k: dict(study='Study', data=('gm', 9811, 7), om=_gm(CLAMP_N), tm=v)
               for k, v in _clamp_models('mean', _sigma(21, GM_LATTICE(CLAMP_N))).items()}
CLAMP_HYPER = {
    'walk_then_switch': dict(study='HyperStudy', data=('gm', 9812, 6), om=_gm(CLAMP_N), tm=_clamp_hyper('mean', GM_LATTICE(CLAMP_N))),
    'switch_then_walk': dict(study='HyperStudy', data=('gm', 9813, 6), om=_gm(CLAMP_N),
                             tm=('Combined', list(reversed(_clamp_hyper('mean', GM_LATTICE(CLAMP_N))[1])))),
    'switch_alone': dict(study='HyperStudy', data=('gm', 9814, 6), om=_gm(CLAMP_N), tm=('RS', 'log10pMin', ('cint', -7, -2, 6), None)),
    'not_equal': dict(study='HyperStudy', data=('gm', 9815, 6), om=_gm(CLAMP_N), tm=('NE', 'log10pMin', ('cint', -7, -2, 6), None)),
}

LONG = {
    # walks, two cells per thread (M = 2, CL = 0)
    'walks_gm4097': HYPER4097,
    'walks_gm4097_forward': dict(HYPER4097, fit=dict(forwardOnly=True)),
    'walks_gm4097_evidence': dict(HYPER4097, fit=dict(evidenceOnly=True)),
    # two chains (fewer than the four from which shorter rows share a table), one of radius 536: 2 * 8192 + 5 * 536 + 113 = 19 177 of
    # the 19 200 doubles
    'walks_poisson8192': dict(study='HyperStudy', data=('coal', 7), om=_poisson(8192),
                              tm=('GRW', 'sigma', [_sigma(40, PO_LATTICE(8192)), _sigma(536, PO_LATTICE(8192))], 'rate', None)),
    # restarts: a tabulated model, change points at six candidate times
    'restarts_bernoulli5001': dict(study='ChangepointStudy', data=BERNOULLI7, om=_bernoulli(5001),
                                   tm=('ChangePoint', 'tChange', [1, 2, 3, 4, 5, 6], None)),
    'restarts_bernoulli5001_evidence': dict(study='ChangepointStudy', data=BERNOULLI7, om=_bernoulli(5001),
                                            tm=('ChangePoint', 'tChange', [1, 2, 3, 4, 5, 6], None), fit=dict(evidenceOnly=True)),
    # spline shifts (M = 1, CL = 1): 5 cells per step (asymmetric stencil), 19 cells per step (two-stage form)
    'shift_slow5000': dict(study='ChangepointStudy', data=('gm', 9821, 8), om=_gm(5000), tm=_serial('c1l_slow'), tol=dict(cases.FFT_TOL)),
    'shift_fast5000': dict(study='ChangepointStudy', data=('gm', 9822, 8), om=_gm(5000), tm=_serial('c1l_fast'), tol=dict(cases.FFT_TOL)),
    # ... with a RegimeSwitch segment in front of the break point (M = 1, CL = 2)
    'shift_clamp5000': dict(study='ChangepointStudy', data=('gm', 9823, 8), om=_gm(5000),
                            tm=_serial('c1l_slow', ('RS', 'log10pMin', -5, None)), tol=dict(cases.FFT_TOL)),
}
LONG.update({'clamp_study_' + k: v for k, v in CLAMP_STUDY.items()})
LONG.update({'clamp_hyper_' + k: v for k, v in CLAMP_HYPER.items()})

# beyond the envelope: these keep the paths they have without the long flavour
EDGE = {
    # radius 541 on 8192 cells: 2 * 8192 + 5 * 541 + 113 = 19 202 doubles
    'edge_radius541': dict(study='HyperStudy', data=('coal', 6), om=_poisson(8192),
                           tm=('GRW', 'sigma', [_sigma(12, PO_LATTICE(8192)), _sigma(541, PO_LATTICE(8192))], 'rate', None)),
    'edge_8193': dict(study='HyperStudy', data=('gm', 9831, 6), om=_gm(8193),
                      tm=('GRW', 'sigma', [_sigma(r, GM_LATTICE(8193)) for r in (0, 5, 40)], 'mean', None)),
    # a two-stage shift (23.6 cells per step) on 6200 cells: 3 * 6200 + 6 * 46 + 433 = 19 309 doubles
    'edge_shift6200': dict(study='ChangepointStudy', data=('gm', 9832, 7), om=_gm(6200), tm=_serial('c1l_fast'), tol=dict(cases.FFT_TOL)),
}

# chain-resident shapes of at most 4096 cells, recorded from a build of the commit before the long flavour (tests/golden/
# chain1d_parent_results.npz): CL = 0 with one and with two cells per thread, CL = 1, CL = 2
PARENT = {
    'parent_gm300_walks': dict(study='HyperStudy', data=('gm', 9711, 12), om=_gm(300), tm=('GRW', 'sigma', ('cint', 0.05, 0.4, 5), 'mean', None)),
    'parent_poisson1000_walks': dict(study='HyperStudy', data=('coal', 8), om=_poisson(1000), tm=('GRW', 'sigma', ('cint', 0.002, 0.012, 64), 'rate', None)),
    'parent_gm300_shift': dict(study='ChangepointStudy', data=('gm', 9712, 10), om=_gm(300),
                               tm=('Serial', [('Static',), ('BreakPoint', 't_break', [3, 6], None), ('Deterministic', 'drift', 'mean')])),
    'parent_poisson701_clamp': dict(study='Study', data=('coal', 10), om=_poisson(701),
                                    tm=('Combined', [('GRW', 's', 0.12, 'rate', None), ('RS', 'log10pMin', -5, None)])),
}
PARENT_KERNELS = {
    'parent_gm300_walks': 'bl1c::chain1d_kernel<100, %s, 1, 0>',
    'parent_poisson1000_walks': 'bl1c::chain1d_kernel<100, %s, 2, 0>',
    'parent_gm300_shift': 'bl1c::chain1d_kernel<3, %s, 1, 1>',
    'parent_poisson701_clamp': 'bl1c::chain1d_kernel<1, %s, 2, 2>',
}
PARENT_KEYS = ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution')


def parent_results(S):
    """what tests/golden/chain1d_parent_results.npz keeps of a fitted study"""
    out = {}
    for key in PARENT_KEYS:
        v = getattr(S, key, None)
        if v is not None and np.size(v) > 0:
            out[key] = np.asarray(v, dtype=float)
    return out
