"""
Parity of the HIP path (through the C-ABI of libblhip.so) on a real MI355X against
  (a) the golden vectors generated from the reference (tests/golden), and
  (b) the CPU oracle on seeded inputs the fixtures do not cover.
Bar (BASELINE.json / SURVEY.md 8d, float64): log-evidence 1e-9 relative; posteriors |dp| <= 1e-12 + 1e-9 p.
"""
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import random_cases
import oracle_adapter as oa
from bayesloop_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()                    # raises BackendError if libblhip.so or the GPU is missing
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def result_of(S, case):
    c = cases.CASES[case] if isinstance(case, str) else case
    res = dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence)
    if not c.get('fit', {}).get('evidenceOnly', False) and np.isfinite(S.logEvidence):
        res['posteriorSequence'] = S.posteriorSequence
        res['posteriorMeanValues'] = S.posteriorMeanValues
    for key in ('logEvidenceList', 'hyperParameterDistribution', 'hyperGridValues', 'flatHyperPriorValues',
                'hyperGridConstant', 'mask'):
        if hasattr(S, key) and getattr(S, key) is not None and len(np.atleast_1d(getattr(S, key))) > 0:
            res[key] = np.asarray(getattr(S, key))
    return res


@pytest.mark.parametrize('case', list(cases.CASES))
def test_hip_matches_reference_golden(case):
    S = cases.build(bl, case)
    S.fit(**cases.fit_kwargs(case))
    compare.check(result_of(S, case), oa.load_golden(case), compare.GPU_TOL, case_tol=cases.CASES[case].get('tol'))


@pytest.mark.parametrize('option', ['fast', 'recurrence', 'mfma', 'mfma_h'])
@pytest.mark.parametrize('case', ['c3_small', 'c3_missing', 'multidim_data', 'c4_small', 'c5_cp_grw', 'c3_forward_only'])
def test_alternative_kernel_paths_match_golden(case, option):
    """The generic LDS-tile kernel (fast=0), the exact-exp likelihood (recurrence=0) and the vector-ALU streaming kernels
    (mfma=0: all launches, mfma_h=0: the both-axes launches) on the 2-D cases."""
    eng = bl.get_engine()
    eng.set_option(option, 0)
    eng.set_option('resident', 0)          # (single-chain 2-D cases would otherwise take the time-resident kernel, tested below)
    eng.set_option('chain_resident', 0)    # (and axis-0-only hyper-studies the chain-resident kernel)
    try:
        S = cases.build(bl, case)
        S.fit(**cases.fit_kwargs(case))
        if option == 'fast':
            assert S.lastTiming['fwd_kernel_variant'] == 0
        if option == 'mfma':
            assert S.lastTiming['fwd_kernel_variant'] in (0, 1)        # (0: the case is too small for the streaming kernels)
        compare.check(result_of(S, case), oa.load_golden(case), compare.GPU_TOL, case_tol=cases.CASES[case].get('tol'))
    finally:
        eng.set_option(option, 1)
        eng.set_option('resident', 1)
        eng.set_option('chain_resident', 1)


@pytest.mark.parametrize('case', ['c1_coal', 'c2_small', 'kat_changepoint', 'c1_coal_changepoint', 'kat_gaussianmean',
                                  'c1_coal_hyper', 'kat_study_prior_array', 'cp_nonunit_time'])
def test_one_launch_per_step_1d_kernels_match_golden(case):
    """1-D cases with the K-steps-per-launch kernel switched off (fuse1d=0: generic kernel) and with K = 1 / K = 3."""
    eng = bl.get_engine()
    eng.set_option('chain1d', 0)           # (batches of chains would otherwise take the chain-resident 1-D kernel, tested on its own)
    for k, variant in ((0, 0), (1, 4), (3, 4)):
        eng.set_option('fuse1d', k)
        try:
            S = cases.build(bl, case)
            S.fit(**cases.fit_kwargs(case))
            assert S.lastTiming['fwd_kernel_variant'] in (variant, 8 if variant == 4 else variant)       # (8: the persistent kernel of the same scheme)
            compare.check(result_of(S, case), oa.load_golden(case), compare.GPU_TOL)
        finally:
            eng.set_option('fuse1d', 8)
    eng.set_option('chain1d', 1)


@pytest.mark.parametrize('case', ['c1_coal', 'c2_small', 'kat_changepoint', 'c1_coal_changepoint', 'kat_gaussianmean',
                                  'c1_coal_hyper', 'kat_study_prior_array', 'cp_nonunit_time'])
def test_persistent_1d_kernel_is_bit_identical_to_the_launch_per_k_path(case):
    """blhip_persist1d.hpp (kernel variant 8: one launch per pass, supersteps handed over inside the kernel) against
    blhip_fused1d.hpp (variant 4: one launch per K steps): the same arithmetic in the same order -- identical bits; K = 8 and K = 3."""
    eng = bl.get_engine()
    eng.set_option('chain1d', 0)
    for k in (8, 3):
        eng.set_option('fuse1d', k)
        try:
            A = cases.build(bl, case)
            A.fit(**cases.fit_kwargs(case))
            eng.set_option('persist1d', 0)
            try:
                B = cases.build(bl, case)
                B.fit(**cases.fit_kwargs(case))
            finally:
                eng.set_option('persist1d', 1)
        finally:
            eng.set_option('fuse1d', 8)
            eng.set_option('chain1d', 1 if k == 3 else 0)
        # (a pass that fits in one superstep -- T <= K -- has no launch boundary to save and keeps the launch path)
        assert A.lastTiming['fwd_kernel_variant'] in ((8,) if case in ('c1_coal', 'c2_small', 'c1_coal_hyper') else (4, 8)) and A.lastTiming['resident_fallbacks'] == 0, A.lastTiming
        assert B.lastTiming['fwd_kernel_variant'] == 4, B.lastTiming
        ra, rb = result_of(A, case), result_of(B, case)
        for key in rb:
            if rb[key] is None:
                continue
            assert np.array_equal(np.asarray(ra[key]), np.asarray(rb[key]), equal_nan=True), (case, k, key)
        compare.check(ra, oa.load_golden(case), compare.GPU_TOL)


def test_persistent_1d_kernel_falls_back_when_a_block_gives_up():
    eng = bl.get_engine()
    eng.set_option('resident_force_abort', 1)
    eng.set_option('quiet', 1)
    try:
        S = cases.build(bl, 'c2_small')
        S.fit(**cases.fit_kwargs('c2_small'))
    finally:
        eng.set_option('resident_force_abort', 0)
        eng.set_option('quiet', 0)
        eng.set_option('resident_ok', 1)
    assert S.lastTiming['fwd_kernel_variant'] == 4 and S.lastTiming['resident_fallbacks'] == 1, S.lastTiming
    compare.check(result_of(S, 'c2_small'), oa.load_golden('c2_small'), compare.GPU_TOL)


EXTRA = {
    # seeded inputs beyond the fixtures: ragged grid sizes (tile remainders), wide/narrow filters, 1-D and 2-D
    'x_ragged_2d': dict(study='Study', data=('series', 21, 14), om=cases.gauss2d(131, -5, 5, 3),
                        tm=('Combined', [('GRW', 's1', 0.21, 'mean', None), ('GRW', 's2', 0.05, 'std', None)])),
    'x_ragged_2d_b': dict(study='Study', data=('series', 22, 9),
                          om=('Gaussian', [('mean', ('cint', -4, 4, 67)), ('std', ('oint', 0, 3, 301))], 'default'),
                          tm=('Combined', [('GRW', 's1', 0.5, 'mean', None), ('GRW', 's2', 0.03, 'std', None)])),
    'x_tall_2d': dict(study='Study', data=('series', 23, 9),
                      om=('Gaussian', [('mean', ('cint', -4, 4, 515)), ('std', ('oint', 0, 3, 33))], 'default'),
                      tm=('Combined', [('GRW', 's1', 0.05, 'mean', None), ('GRW', 's2', 0.3, 'std', None)])),
    'x_1d_long': dict(study='Study', data=('gm', 5, 64), om=('GaussianMean', [('mean', ('cint', -6, 6, 70001))], 'default'),
                      tm=('GRW', 'sigma', 0.002, 'mean', None)),
    'x_1d_static_forward': dict(study='Study', data=cases.COAL, timestamps=cases.COAL_T,
                                om=('Poisson', [('rate', ('oint', 0, 6, 777))], 'default'), tm=('Static',),
                                fit=dict(forwardOnly=True)),
    'x_hyper_many': dict(study='HyperStudy', data=('series', 24, 20), om=cases.gauss2d(72, -5, 5, 3),
                         tm=('Combined', [('GRW', 's1', ('cint', 0, 0.6, 9), 'mean', None),
                                          ('GRW', 's2', ('cint', 0, 0.12, 5), 'std', None)])),
    'x_hyper_forward': dict(study='HyperStudy', data=('series', 25, 16), om=cases.gauss2d(40, -5, 5, 3),
                            tm=('GRW', 'sigma', ('cint', 0.05, 0.5, 6), 'mean', None), fit=dict(forwardOnly=True)),
    # matrix-pipe kernels (blhip_mfma.hpp): wide axis-0 radius, ragged rows / columns, all radius buckets in one batch
    'x_mfma_wide': dict(study='Study', data=('series', 27, 12),
                        om=('Gaussian', [('mean', ('cint', -5, 5, 150)), ('std', ('oint', 0, 3, 70))], 'default'),
                        tm=('GRW', 's1', 0.537, 'mean', None)),
    'x_mfma_ragged': dict(study='Study', data=('series', 28, 10),
                          om=('Gaussian', [('mean', ('cint', -5, 5, 83)), ('std', ('oint', 0, 3, 129))], 'default'),
                          tm=('GRW', 's1', 0.9, 'mean', None)),
    'x_mfma_buckets': dict(study='HyperStudy', data=('series', 29, 14), om=cases.gauss2d(96, -5, 5, 3),
                           tm=('GRW', 'sigma', ('cint', 0, 1.0, 11), 'mean', None)),
    'x_mfma_cp': dict(study='HyperStudy', data=('series_jump', 30, 24, 11, 2.0), om=cases.gauss2d(80, -5, 7, 3),
                      tm=('Combined', [('GRW', 'sigma', ('cint', 0.1, 0.9, 4), 'mean', None),
                                       ('ChangePoint', 'tc', ('arange', 4, 20, 5), None)])),
    'x_mfma_both_ragged': dict(study='Study', data=('series', 32, 9),
                               om=('Gaussian', [('mean', ('cint', -4, 4, 203)), ('std', ('oint', 0, 3, 77))], 'default'),
                               tm=('Combined', [('GRW', 's1', 0.31, 'mean', None), ('GRW', 's2', 0.06, 'std', None)])),
    'x_mfma_axis1_only': dict(study='Study', data=('series', 33, 9),
                              om=('Gaussian', [('mean', ('cint', -4, 4, 97)), ('std', ('oint', 0, 3, 111))], 'default'),
                              tm=('GRW', 's2', 0.05, 'std', None)),
    # random walks on the SECOND parameter wider than the fused kernels' 8-column halo: axis-1 pre-pass (blhip_hwide.hpp) + fused kernels
    'x_wide_h': dict(study='Study', data=('series', 41, 10), om=cases.gauss2d(96, -6, 6, 3),
                     tm=('Combined', [('GRW', 's1', 0.25, 'mean', None), ('GRW', 's2', 0.3, 'std', None)])),            # radii 8 / 38
    'x_wide_h_only': dict(study='Study', data=('series', 42, 8),
                          om=('Gaussian', [('mean', ('cint', -4, 4, 67)), ('std', ('oint', 0, 3, 301))], 'default'),
                          tm=('GRW', 's2', 0.15, 'std', None)),                                                           # radius 60, ragged columns
    'x_wide_h_hyper': dict(study='HyperStudy', data=('series', 43, 12), om=cases.gauss2d(64, -4, 4, 3),
                           tm=('Combined', [('GRW', 's1', ('cint', 0, 0.4, 3), 'mean', None),
                                            ('GRW', 's2', ('cint', 0.05, 0.5, 4), 'std', None)])),                          # radii 4 .. 43 in one batch
    'x_wide_h_hyper_axis1': dict(study='HyperStudy', data=('series', 44, 12), om=cases.gauss2d(80, -4, 4, 3),
                                 tm=('GRW', 's2', ('cint', 0.02, 0.5, 6), 'std', None)),                                  # walk on the second parameter only
    'x_wide_h_cp': dict(study='ChangepointStudy', data=('series_jump', 45, 24, 12, 2.0), om=cases.gauss2d(40, -4, 6, 3),
                        tm=('Combined', [('ChangePoint', 'tChange', ('arange', 2, 22, 3), None),
                                         ('GRW', 'sigma', 0.4, 'std', None)])),                                             # restarts through the pre-pass
    'x_wide_h_200': dict(study='Study', data=('series', 47, 6),
                         om=('Gaussian', [('mean', ('cint', -4, 4, 64)), ('std', ('oint', 0, 3, 520))], 'default'),
                         tm=('Combined', [('GRW', 's1', 0.3, 'mean', None), ('GRW', 's2', 0.29, 'std', None)])),             # axis-1 radius 201, three column blocks
    'x_wide_h_with_zero': dict(study='HyperStudy', data=('series', 48, 11), om=cases.gauss2d(64, -4, 4, 3),
                               tm=('Combined', [('GRW', 's1', ('cint', 0, 0.4, 3), 'mean', None),
                                                ('GRW', 's2', ('cint', 0, 0.27, 4), 'std', None)])),                       # axis-1 radii 0 (no filter), 8, 16, 23 in one batch
    'x_wide_h_forward': dict(study='Study', data=('series', 46, 9), om=cases.gauss2d(72, -5, 5, 3),
                             tm=('Combined', [('GRW', 's1', 0.4, 'mean', None), ('GRW', 's2', 0.5, 'std', None)]),
                             fit=dict(forwardOnly=True)),
    # random walks on the FIRST parameter wider than the matrix-pipe kernels' largest band (radius 40): column pre-pass (blh::vwide_kernel)
    'x_wide_v': dict(study='Study', data=('series', 51, 9),
                     om=('Gaussian', [('mean', ('cint', -4, 4, 300)), ('std', ('oint', 0, 3, 40))], 'default'),
                     tm=('GRW', 's1', 0.516, 'mean', None)),                                                               # radius 77, three row tiles
    'x_wide_v_hyper': dict(study='HyperStudy', data=('series', 52, 10),
                           om=('Gaussian', [('mean', ('cint', -5, 5, 400)), ('std', ('oint', 0, 3, 33))], 'default'),
                           tm=('GRW', 'sigma', ('cint', 0, 0.7, 6), 'mean', None)),                                          # radii 9 .. 103 in one batch
    'x_wide_both': dict(study='HyperStudy', data=('series', 53, 8),
                        om=('Gaussian', [('mean', ('cint', -5, 5, 260)), ('std', ('oint', 0, 3, 200))], 'default'),
                        tm=('Combined', [('GRW', 's1', ('cint', 0.1, 0.6, 3), 'mean', None), ('GRW', 's2', ('cint', 0.02, 0.2, 2), 'std', None)])),   # both pre-passes
    'x_wide_v_narrow_h': dict(study='Study', data=('series', 54, 8),
                              om=('Gaussian', [('mean', ('cint', -5, 5, 333)), ('std', ('oint', 0, 3, 70))], 'default'),
                              tm=('Combined', [('GRW', 's1', 0.45, 'mean', None), ('GRW', 's2', 0.05, 'std', None)]), fit=dict(forwardOnly=True)),
    'x_wide_v_cp': dict(study='ChangepointStudy', data=('series_jump', 55, 16, 8, 2.0),
                        om=('Gaussian', [('mean', ('cint', -4, 6, 280)), ('std', ('oint', 0, 3, 24))], 'default'),
                        tm=('Combined', [('ChangePoint', 'tChange', ('arange', 2, 14, 4), None), ('GRW', 'sigma', 0.5, 'mean', None)])),
    # edge shapes: a single time step, minimal grids, a first step without data, one hyper-grid point
    'x_single_step': dict(study='Study', data=np.array([2.5]), om=cases.gauss2d(64, -5, 5, 3),
                          tm=('Combined', [('GRW', 's1', 0.3, 'mean', None), ('GRW', 's2', 0.1, 'std', None)])),
    'x_single_step_1d': dict(study='Study', data=np.array([3]), om=('Poisson', [('rate', ('oint', 0, 6, 33))], 'default'),
                             tm=('GRW', 'sigma', 0.4, 'rate', None)),
    'x_two_cells_1d': dict(study='Study', data=cases.D15, om=('Poisson', [('rate', ('cint', 1, 3, 2))], 'default'),
                           tm=('GRW', 'sigma', 0.7, 'rate', None)),
    'x_tiny_2d': dict(study='Study', data=('series', 35, 6),
                      om=('Gaussian', [('mean', ('cint', -2, 2, 3)), ('std', ('oint', 0, 3, 5))], 'default'),
                      tm=('Combined', [('GRW', 's1', 1.5, 'mean', None), ('GRW', 's2', 0.9, 'std', None)])),
    'x_first_step_missing': dict(study='Study', data=('series_nan', 36, 9, [0, 1, 8]), om=cases.gauss2d(40, -5, 5, 3),
                                 tm=('GRW', 's1', 0.3, 'mean', None)),
    'x_one_hyper_point': dict(study='HyperStudy', data=('series', 37, 7), om=cases.gauss2d(32, -5, 5, 3),
                              tm=('GRW', 'sigma', [0.25], 'mean', None)),
    'x_cp_all': dict(study='ChangepointStudy', data=('series_jump', 26, 30, 17, 2.5), om=cases.gauss2d(50, -5, 7, 3),
                     tm=('ChangePoint', 'tc', 'all', None)),
}


@pytest.mark.parametrize('case', list(EXTRA))
def test_hip_matches_oracle(case):
    c = EXTRA[case]
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL)


def test_reference_fixtures_on_the_chain_resident_path():
    """Fixtures generated from the reference (and the extra cases above) that the chain-resident kernels take since they accept padded
    grids and change points inside filtering chains: random walk + change point in one model in both list orders (40 x 40 grid),
    a hyper-study over walk width x change point (80 x 80), a change-point study over all time steps (50 x 50)."""
    for name in ('c5_cp_grw', 'c5_grw_cp', 'c5_small', 'c4_small'):
        S = cases.build(bl, name)
        S.fit(**cases.fit_kwargs(name))
        assert S.lastTiming['fwd_kernel_variant'] == 6 and S.lastTiming['bwd_kernel_variant'] == 6, (name, S.lastTiming)
        compare.check(result_of(S, name), oa.load_golden(name), compare.GPU_TOL)
    for name in ('x_mfma_cp', 'x_cp_all'):
        S = cases.build(bl, EXTRA[name])
        S.fit(silent=True)
        assert S.lastTiming['fwd_kernel_variant'] == 6 and S.lastTiming['bwd_kernel_variant'] == 6, (name, S.lastTiming)


def test_wide_axis1_walks_take_the_streaming_kernels():
    """Axis-1 radii above 8 no longer drop a batch to the generic LDS-tile kernel (variant 0): pre-pass + streaming kernels
    (variants 1 / 3); wide_h = 0 restores the old routing, with the same results."""
    eng = bl.get_engine()
    for name in ('x_wide_h', 'x_wide_h_only', 'x_wide_h_hyper', 'x_wide_h_hyper_axis1', 'x_wide_h_cp', 'x_wide_h_200', 'x_tall_2d', 'x_hyper_many'):
        # (round 5: radii <= 40 on grids inside 512 x 512 take the transposing chain-resident kernels by default -- variant 6, same results;
        #  this test is about the pre-pass path, which keeps everything else: chain_ax1 = 0)
        D = cases.build(bl, EXTRA[name])
        D.fit(silent=True)
        eng.set_option('chain_ax1', 0)
        try:
            S = cases.build(bl, EXTRA[name])
            S.fit(silent=True)
        finally:
            eng.set_option('chain_ax1', 1)
        np.testing.assert_allclose(D.logEvidence, S.logEvidence, rtol=1e-11)
        assert S.lastTiming['fwd_kernel_variant'] in (1, 3) and S.lastTiming['bwd_kernel_variant'] in (1, 3), (name, S.lastTiming)
        eng.set_option('wide_h', 0)
        eng.set_option('chain_ax1', 0)
        try:
            S0 = cases.build(bl, EXTRA[name])
            S0.fit(silent=True)
            assert S0.lastTiming['fwd_kernel_variant'] == 0, (name, S0.lastTiming)
        finally:
            eng.set_option('wide_h', 1)
            eng.set_option('chain_ax1', 1)
        np.testing.assert_allclose(S.logEvidence, S0.logEvidence, rtol=1e-11)
        np.testing.assert_allclose(S.posteriorMeanValues, S0.posteriorMeanValues, rtol=1e-9, atol=1e-12)


def test_big_read_backs_move_to_page_locked_arrays_after_the_first():
    """engine._PinnedPool: the first read-back of a size goes to an ordinary array and a block of that size is pinned in the background
    AFTER that copy is done; the next read-back of the size gets the block (same numbers), and the block returns to the pool with the
    array's last view."""
    eng = bl.get_engine()
    pool = eng._pinned
    if not pool.enabled:
        pytest.skip('BLHIP_PINNED_RESULTS=0')
    pool.release()
    pool.released = False                                 # (release() is the engine's teardown: re-open the pool for this test)
    c = dict(study='Study', data=('series', 77, 66), om=cases.gauss2d(256, -6, 6, 3), tm=('GRW', 's1', 0.2, 'mean', None))
    S = cases.build(bl, c); S.fit(silent=True)
    assert pool.free is None and pool.deferred == 0
    a = np.array(S.posteriorSequence)                    # 66 x 256 x 256 doubles = 34.6 MB > MIN_BYTES: pageable this time ...
    assert pool.deferred == 0 and pool.pending is not None
    pool.wait_ready()
    assert pool.free is not None and pool.free[1] >= a.nbytes       # ... and a block of that size is pinned now
    S2 = cases.build(bl, c); S2.fit(silent=True)
    b = S2.posteriorSequence
    assert pool.free is None                              # the block is out: b lives in it
    assert np.array_equal(a, np.asarray(b))
    del b
    S2.posteriorSequence = None
    S2._posterior_pending = None
    import gc; gc.collect()
    assert pool.free is not None                          # back in the pool


def test_chains_without_an_axis1_filter_skip_the_pre_pass():
    """A hyper-grid over the width of a walk on the second parameter usually includes 0: those chains have no axis-1 filter and skip the
    pre-pass (it would copy their state): same results bit for bit as with wide_h_split = 0, fewer bytes.  wide_h_fused_max = 8 also lets
    the narrow filters (radius <= 8) run inside the fused kernels (not the default: no faster) -- same results to rounding."""
    eng = bl.get_engine()
    c = EXTRA['x_wide_h_with_zero']
    eng.set_option('chain_ax1', 0)           # (the pre-pass path; by default the transposing chain-resident kernels take this study)
    try:
        _chains_without_an_axis1_filter_skip_the_pre_pass(eng, c)
    finally:
        eng.set_option('chain_ax1', 1)


def _chains_without_an_axis1_filter_skip_the_pre_pass(eng, c):
    A = cases.build(bl, c); A.fit(silent=True)
    assert A.lastTiming['fwd_kernel_variant'] in (1, 3), A.lastTiming
    eng.set_option('wide_h_split', 0)
    try:
        B = cases.build(bl, c); B.fit(silent=True)
    finally:
        eng.set_option('wide_h_split', 1)
    assert A.logEvidence == B.logEvidence
    assert np.array_equal(np.array(A.posteriorSequence), np.array(B.posteriorSequence), equal_nan=True)
    assert A.lastTiming['fwd_hbm_bytes'] < B.lastTiming['fwd_hbm_bytes'] and A.lastTiming['bwd_hbm_bytes'] < B.lastTiming['bwd_hbm_bytes']
    eng.set_option('wide_h_fused_max', 8)
    try:
        F = cases.build(bl, c); F.fit(silent=True)
    finally:
        eng.set_option('wide_h_fused_max', 0)
    assert F.lastTiming['fwd_hbm_bytes'] < A.lastTiming['fwd_hbm_bytes']
    np.testing.assert_allclose(F.logEvidence, A.logEvidence, rtol=1e-12)
    np.testing.assert_allclose(np.array(F.posteriorSequence), np.array(A.posteriorSequence), rtol=1e-10, atol=1e-300)
    with np.errstate(all='ignore'):
        want = oa.run(c)
    compare.check(dict(logEvidence=A.logEvidence, localEvidence=A.localEvidence, posteriorSequence=A.posteriorSequence, posteriorMeanValues=A.posteriorMeanValues),
                  dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'], posteriorSequence=want['posteriorSequence'],
                       posteriorMeanValues=want['posteriorMeanValues']), compare.GPU_TOL)


def test_wide_axis0_walks_take_the_streaming_kernels():
    """Axis-0 radii above 40 do not drop a batch to the generic LDS-tile kernel: column pre-pass + the no-stencil streaming kernel
    (variant 1) -- for walks on the first parameter only up to radius 80 that is the fall-back of the chain-resident kernels since round 4
    (chain_wide = 0 here); wide_v = 0 restores the old routing, with the same results; and the default routing agrees with both."""
    eng = bl.get_engine()
    for name in ('x_wide_v', 'x_wide_v_hyper', 'x_wide_both', 'x_wide_v_narrow_h', 'x_wide_v_cp'):
        c = EXTRA[name]
        eng.set_option('chain_wide', 0)
        try:
            S = cases.build(bl, c)
            S.fit(**cases.fit_kwargs(c))
            assert S.lastTiming['fwd_kernel_variant'] == 1, (name, S.lastTiming)
            eng.set_option('wide_v', 0)
            try:
                S0 = cases.build(bl, c)
                S0.fit(**cases.fit_kwargs(c))
                assert S0.lastTiming['fwd_kernel_variant'] == 0, (name, S0.lastTiming)
            finally:
                eng.set_option('wide_v', 1)
        finally:
            eng.set_option('chain_wide', 1)
        D = cases.build(bl, c)
        D.fit(**cases.fit_kwargs(c))
        assert D.lastTiming['fwd_kernel_variant'] in (1, 6), (name, D.lastTiming)
        for A in (S0, D):
            np.testing.assert_allclose(S.logEvidence, A.logEvidence, rtol=1e-11)
            np.testing.assert_allclose(S.posteriorMeanValues, A.posteriorMeanValues, rtol=1e-9, atol=1e-12)


def test_matrix_pipe_kernels_ran():
    """The cases above really go through blm::mfma_step_kernel (timing variant 3), in both directions -- the one-axis walk on its padded
    grid since round 4 only with the chain-resident kernels' de-padding path off (they are its fall-back)."""
    eng = bl.get_engine()
    for name in ('x_mfma_wide', 'x_mfma_both_ragged'):
        eng.set_option('chain_depad', 0)
        try:
            S = cases.build(bl, EXTRA[name])
            S.fit(silent=True)
        finally:
            eng.set_option('chain_depad', 1)
        assert S.lastTiming['fwd_kernel_variant'] == 3 and S.lastTiming['bwd_kernel_variant'] == 3, S.lastTiming
        want = cases.build(bl, EXTRA[name]); want.fit(silent=True)
        np.testing.assert_allclose(np.asarray(S.posteriorSequence), np.asarray(want.posteriorSequence), rtol=1e-9, atol=1e-14)


def test_matrix_pipe_table_likelihood_and_forced_both_axes():
    """Tabulated likelihood through the matrix-pipe kernels, and the both-axes variant forced on a launch larger than its
    default size limit: both equal the vector-ALU kernels (mfma=0) to rounding.  (chain_table = 0: the one-axis walk would take the
    chain-resident kernels' table flavour since round 4 -- these kernels are its fall-back.)"""
    eng = bl.get_engine()

    def fit(n0, n1, s1, s2, **opts):
        opts = dict(opts, chain_table=0)
        for k, v in opts.items():
            eng.set_option(k, v)
        try:
            S = bl.Study(silent=True)
            S.loadData(cases.series(34, 8), silent=True)
            tms = [bl.tm.GaussianRandomWalk('s1', s1, target='location')]
            if s2:
                tms.append(bl.tm.GaussianRandomWalk('s2', s2, target='scale'))
            S.set(bl.om.Laplace('location', bl.cint(-5, 5, n0), 'scale', bl.oint(0, 3, n1)),
                  bl.tm.CombinedTransitionModel(*tms), silent=True)
            S.fit(silent=True)
            return S
        finally:
            for k in opts:
                eng.set_option(k, 1 if k != 'mfma_h_max_cells' else 2.5e6)

    for (n0, n1, s1, s2) in ((140, 90, 0.6, 0.0), (140, 90, 0.3, 0.05)):
        A = fit(n0, n1, s1, s2, mfma_h_max_cells=1e15)
        assert A.lastTiming['fwd_kernel_variant'] == 3
        B = fit(n0, n1, s1, s2, mfma=0)
        assert B.lastTiming['fwd_kernel_variant'] == 1
        assert abs(A.logEvidence - B.logEvidence) <= 1e-11 * abs(B.logEvidence)
        np.testing.assert_allclose(A.posteriorSequence, B.posteriorSequence, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(A.posteriorMeanValues, B.posteriorMeanValues, rtol=1e-10)


def test_table_likelihood_path_on_device():
    """An observation model the kernels do not know (plug-in pdf) -> likelihood table path; equals the native model."""
    import math

    class MyGaussian(bl.om.ObservationModel):
        def __init__(self):
            self.name = 'plug-in gaussian'
            self.segmentLength = 1
            self.multiplyLikelihoods = True
            self.parameterNames = ['mean', 'std']
            self.parameterValues = [bl.cint(-5, 5, 60), bl.oint(0, 3, 44)]
            self.prior = lambda m, s: 1. / s ** 2.

        def pdf(self, grid, seg):
            return np.exp(-((seg[0] - grid[0]) ** 2.) / (2. * grid[1] ** 2.) - .5 * np.log(2. * np.pi * grid[1] ** 2.))

    x = cases.series(31, 12)
    T = bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s1', 0.3, target='mean'),
                                      bl.tm.GaussianRandomWalk('s2', 0.1, target='std'))
    A = bl.Study(silent=True); A.loadData(x, silent=True); A.set(MyGaussian(), T, silent=True); A.fit(silent=True)
    B = bl.Study(silent=True); B.loadData(x, silent=True)
    B.set(bl.om.Gaussian('mean', bl.cint(-5, 5, 60), 'std', bl.oint(0, 3, 44)), T, silent=True); B.fit(silent=True)
    assert abs(A.logEvidence - B.logEvidence) <= 1e-11 * abs(B.logEvidence)
    np.testing.assert_allclose(A.posteriorSequence, B.posteriorSequence, rtol=1e-9, atol=1e-13)
    L = bl.om.AR1('rho', bl.oint(-1, 1, 100), 'sigma', bl.oint(0, 1, 100))        # reference tests/test_observationmodels.py:198-208
    C = bl.Study(silent=True); C.loadData(np.array([1, 0, 1, 0, 0]), silent=True); C.set(L, bl.tm.Static(), silent=True)
    C.fit(silent=True)
    np.testing.assert_almost_equal(C.logEvidence, -4.3291291450463421, decimal=5)


# ---- size-independent properties at BASELINE.json sizes ----------------------------------------------------------

def _c3(n, T, seed=3, s1=None, s2=None, **fit):
    S = bl.Study(silent=True)
    S.loadData(cases.series(seed, T), silent=True)
    s1 = 0.03 * 1024 / n if s1 is None else s1
    s2 = 0.008 * 1024 / n if s2 is None else s2
    S.set(bl.om.Gaussian('mean', bl.cint(-8, 8, n), 'std', bl.oint(0, 4, n)),
          bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s1', s1, target='mean'),
                                        bl.tm.GaussianRandomWalk('s2', s2, target='std')), silent=True)
    S.fit(silent=True, **fit)
    return S


def test_full_size_c3_properties():
    """1024 x 1024 grid (config C3, shortened series): the identities the recursion must satisfy at any size."""
    T = 24
    S = _c3(1024, T)
    E = _c3(1024, T, evidenceOnly=True)
    F = _c3(1024, T, forwardOnly=True)
    # evidence does not depend on the mode
    assert S.logEvidence == E.logEvidence == F.logEvidence
    # logE = sum log(localEvidence_forward) - (T-1) log dV   
    dV = np.prod(S.latticeConstant)
    assert abs(np.sum(np.log(E.localEvidence)) - (T - 1) * np.log(dV) - E.logEvidence) < 1e-9 * abs(E.logEvidence)
    post = S.posteriorSequence
    assert post.shape == (T, 1024, 1024)
    np.testing.assert_allclose(post.reshape(T, -1).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.all(post >= 0)
    # means are the first moments of the stored posteriors
    np.testing.assert_allclose(S.posteriorMeanValues[0], (post.sum(axis=2) * S.marginalGrid[0]).sum(axis=1), rtol=1e-10)
    np.testing.assert_allclose(S.posteriorMeanValues[1], (post.sum(axis=1) * S.marginalGrid[1]).sum(axis=1), rtol=1e-10)
    # last smoothed posterior == last filtered posterior (beta_T is uniform)
    np.testing.assert_allclose(post[-1], F.posteriorSequence[-1], rtol=1e-9, atol=1e-14)
    # the first 10 steps of the series are the golden anchor c3_t10: forward local evidence must agree
    gold = oa.load_golden('c3_t10')
    S10 = _c3(1024, 10, evidenceOnly=True)
    assert abs(S10.logEvidence - float(gold['logEvidence'])) <= 1e-9 * abs(float(gold['logEvidence']))


def test_full_size_c2_evidence():
    """Config C2 at full size (4096-point grid, 10 000 steps): log-evidence against the golden value."""
    S = cases.build(bl, 'c2_full')
    S.fit(evidenceOnly=True, silent=True)
    gold = float(oa.load_golden('c2_full')['logEvidence'])
    assert abs(S.logEvidence - gold) <= 1e-9 * abs(gold)


def test_hyperstudy_sharding_invariance_on_device():
    """Splitting the hyper-grid into batches (what multi-GPU sharding does per rank) must not change the results."""
    eng = bl.get_engine()
    c = 'c4_small'
    S1 = cases.build(bl, c); S1.fit(silent=True)
    eng.set_option('max_batch', 3)
    try:
        S2 = cases.build(bl, c); S2.fit(silent=True)
    finally:
        eng.set_option('max_batch', 1024)
    assert np.array_equal(S1.logEvidenceList, S2.logEvidenceList)
    np.testing.assert_allclose(S1.posteriorSequence, S2.posteriorSequence, rtol=1e-10, atol=1e-15)
    assert abs(S1.logEvidence - S2.logEvidence) < 1e-12 * abs(S1.logEvidence)


def test_njobs_in_process_two_contexts_on_one_gpu(monkeypatch):
    """HyperStudy.fit(nJobs=2) / ChangepointStudy.fit(nJobs=3) inside ONE process: one libblhip context and one host thread per
    entry of BLHIP_NJOBS_DEVICES (here the same GPU several times: the 1-GPU box), round-robin shares, ONE gather through shared
    memory, the accumulators merged with blhip_accum_peer_reduce / _gather (reduce-scatter over time slices + gather) -- the
    reference's goldens at the bar, and the single-context fit to rounding."""
    for case, devs in (('c4_small', '0,0'), ('c4_2hp', '0,0,0'), ('c5_cp_grw', '0,0'), ('c4_small_evidence', '0,0'), ('kat_changepointstudy', '0,0,0')):
        S1 = cases.build(bl, case)
        S1.fit(**cases.fit_kwargs(case))
        monkeypatch.setenv('BLHIP_NJOBS_DEVICES', devs)
        S2 = cases.build(bl, case)
        S2.fit(nJobs=len(devs.split(',')), **cases.fit_kwargs(case))
        monkeypatch.delenv('BLHIP_NJOBS_DEVICES')
        assert len(S2.lastTimingPerDevice) == len(devs.split(','))
        # (not bit-identical in general: a share may run through another kernel family than the whole grid -- the bucket sizes decide)
        np.testing.assert_allclose(np.asarray(S2.logEvidenceList), np.asarray(S1.logEvidenceList), rtol=1e-12, atol=0)
        res = dict(logEvidence=S2.logEvidence, localEvidence=S2.localEvidence, logEvidenceList=np.array(S2.logEvidenceList),
                   hyperParameterDistribution=S2.hyperParameterDistribution)
        if not cases.CASES[case].get('fit', {}).get('evidenceOnly'):
            res.update(posteriorSequence=S2.posteriorSequence, posteriorMeanValues=S2.posteriorMeanValues)
            np.testing.assert_allclose(S2.posteriorSequence, S1.posteriorSequence, rtol=1e-10, atol=1e-300)
        compare.check(res, oa.load_golden(case), compare.GPU_TOL)


def test_njobs_merge_through_host_memory_when_there_is_no_peer_access(monkeypatch, capfd):
    """Devices without peer access (hipDeviceCanAccessPeer == 0) -- or a peer copy that fails -- merge their accumulators through
    page-locked host memory: an explicit copy, announced once on stderr, reported per device (peer_copy_path = BLHIP_PEER_HOST_STAGED).
    Option peer_copy_mode = 1 forces that branch, so it runs on the one GPU of this box too."""
    eng = bl.get_engine()
    case = 'c4_small'
    S1 = cases.build(bl, case)
    S1.fit(**cases.fit_kwargs(case))
    monkeypatch.setenv('BLHIP_NJOBS_DEVICES', '0,0,0')
    monkeypatch.setenv('BLHIP_NJOBS_MULTI_GPU', 'strict')
    base_opts = os.environ.get('BLHIP_ENGINE_OPTS', '')
    monkeypatch.setenv('BLHIP_ENGINE_OPTS', 'peer_copy_mode=1,quiet=0' + (',' + base_opts if base_opts else ''))
    eng.set_option('peer_copy_mode', 1)
    try:
        S2 = cases.build(bl, case)
        S2.fit(nJobs=3, **cases.fit_kwargs(case))
    finally:
        eng.set_option('peer_copy_mode', 0)
    assert [tm['peer_copy_path'] for tm in S2.lastTimingPerDevice] == [3, 3, 3], S2.lastTimingPerDevice
    assert capfd.readouterr().err.count('goes through host memory') <= 1
    np.testing.assert_allclose(S2.posteriorSequence, S1.posteriorSequence, rtol=1e-10, atol=1e-300)
    res = dict(logEvidence=S2.logEvidence, localEvidence=S2.localEvidence, logEvidenceList=np.array(S2.logEvidenceList),
               hyperParameterDistribution=S2.hyperParameterDistribution, posteriorSequence=S2.posteriorSequence, posteriorMeanValues=S2.posteriorMeanValues)
    compare.check(res, oa.load_golden(case), compare.GPU_TOL)
    monkeypatch.setenv('BLHIP_ENGINE_OPTS', base_opts)                     # (further contexts are created with the default again)
    S3 = cases.build(bl, case)                     # ... and the same-device copies of the default path say so
    S3.fit(nJobs=2, **cases.fit_kwargs(case))
    assert all(tm['peer_copy_path'] == 1 for tm in S3.lastTimingPerDevice[:2]), S3.lastTimingPerDevice


def test_njobs_on_two_physical_gpus_matches_unsharded(monkeypatch):
    """fit(nJobs = 2) over two DIFFERENT device ordinals (peer access, hipMemcpyPeerAsync between devices, kernels armed per device)
    against the unsharded fit and the reference's goldens; BLHIP_NJOBS_MULTI_GPU=strict so that nothing can fall back quietly.
    Skipped on the 1-GPU boxes this suite normally runs on -- the first multi-GPU node to run the suite runs it."""
    from bayesloop_amd import _abi
    if _abi.load().blhip_device_count() < 2:
        pytest.skip('needs two GPUs')
    monkeypatch.setenv('BLHIP_NJOBS_MULTI_GPU', 'strict')
    monkeypatch.delenv('BLHIP_NJOBS_DEVICES', raising=False)
    for case in ('c4_small', 'c4_2hp', 'c5_cp_grw', 'c4_small_evidence'):
        S1 = cases.build(bl, case)
        S1.fit(**cases.fit_kwargs(case))
        S2 = cases.build(bl, case)
        S2.fit(nJobs=2, **cases.fit_kwargs(case))
        assert len(S2.lastTimingPerDevice) == 2
        np.testing.assert_allclose(np.asarray(S2.logEvidenceList), np.asarray(S1.logEvidenceList), rtol=1e-12, atol=0)
        res = dict(logEvidence=S2.logEvidence, localEvidence=S2.localEvidence, logEvidenceList=np.array(S2.logEvidenceList),
                   hyperParameterDistribution=S2.hyperParameterDistribution)
        if not cases.CASES[case].get('fit', {}).get('evidenceOnly'):
            res.update(posteriorSequence=S2.posteriorSequence, posteriorMeanValues=S2.posteriorMeanValues)
            np.testing.assert_allclose(S2.posteriorSequence, S1.posteriorSequence, rtol=1e-10, atol=1e-300)
        compare.check(res, oa.load_golden(case), compare.GPU_TOL)


def test_linearity_of_transition_filter_only():
    """The stencil alone: filtering a one-hot distribution reproduces SciPy's reflect-boundary kernel row."""
    from oracle import bl_oracle as orc
    n = 97
    x = np.zeros((1, n)); x[0, 3] = 1.0
    want = orc.gaussian_filter1d(x, 2.3, 1)
    # drive one forward step with a flat likelihood (all data missing) so that alpha_1 = filter(alpha_0)
    S = bl.Study(silent=True)
    S.loadData(np.array([[np.nan, 1.0], [np.nan, 1.0]]), silent=True)
    grid = bl.cint(0, 96, n)
    prior = np.zeros(n); prior[3] = 1.0
    S.set(bl.om.GaussianMean('mean', grid, prior=prior), bl.tm.GaussianRandomWalk('sigma', 2.3, target='mean'), silent=True)
    S.fit(forwardOnly=True, silent=True)
    np.testing.assert_allclose(S.posteriorSequence[1], want[0], rtol=1e-13, atol=1e-300)


def test_rccl_path_single_rank():
    """The multi-GPU code path -- RCCL bound directly through the C-ABI (blhip_comm_*: unique id, ncclCommInitRank, ONE
    ncclAllGather of rows + trailer, ncclReduce of the accumulator in HBM), no PyTorch in the process -- with one rank must
    reproduce the plain single-GPU result; the small collectives bench.py times with are exercised too."""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent('''
        import os, sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))
        import bayesloop_amd as bl, cases, compare, oracle_adapter as oa
        comm = bl.dist.RcclCommunicator(rank=0, world=1)
        info = comm.info()
        assert info['world'] == 1 and info['rank'] == 0 and info['rccl_version'] > 0, info
        assert comm.allreduce_max(3.5) == 3.5 and list(comm.allreduce([1.0, 2.0])) == [1.0, 2.0]
        g = comm.all_gather(np.arange(7.0))
        assert len(g) == 1 and np.array_equal(g[0], np.arange(7.0))
        for case in ('c4_small', 'c5_cp_grw', 'c4_small_evidence'):
            S = cases.build(bl, case)
            S.communicator = comm
            S.fit(**cases.fit_kwargs(case))
            res = dict(logEvidence=S.logEvidence, localEvidence=S.localEvidence, logEvidenceList=np.array(S.logEvidenceList),
                       hyperParameterDistribution=S.hyperParameterDistribution)
            if 'evidence' not in case:
                res.update(posteriorSequence=S.posteriorSequence, posteriorMeanValues=S.posteriorMeanValues)
            compare.check(res, oa.load_golden(case), compare.GPU_TOL)
            print('ok', case)
        comm.barrier()
        comm.close()
        assert 'torch' not in sys.modules
        print('rccl', info['rccl_version'])
    ''') % (root, root)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count('ok ') == 3, out.stdout + out.stderr


def test_accumulator_row_stats_give_the_merged_means():
    """blhip_accum_row_stats (what a rank contributes to the ONE gather): per-step sums of the un-finalised accumulator reproduce
    the posterior means blhip_accum_finalize computes from the same accumulator."""
    from bayesloop_amd import dist as bdist
    eng = bl.get_engine()
    S = cases.build(bl, 'c4_small')
    S._formatData(); S._createHyperGrid(silent=True); S._checkConsistency()
    S._setAllHyperParameters(S.hyperGridValues[0])
    problem, program = S._compile(silent=True)
    S._setAllHyperParameters(S.flatHyperParameters)
    ov = S._opValueMatrix(program, np.asarray(S.hyperGridValues, dtype=float))
    eng.accum_begin(problem.T, problem.G)
    eng.fit(problem, ov, accumulate=True, log_chain_weight=np.log(np.asarray(S.flatHyperPriorValues, dtype=float)))
    st = eng.accum_row_stats(problem)
    means = eng.accum_finalize(problem)
    np.testing.assert_allclose((st[:, 1:] / st[:, :1]).T, means, rtol=1e-12)
    eng.accum_end()


@pytest.mark.parametrize('name', ['fwd2048', 'c3', 'c4', 'c5', 'c4_both_axes', 'c4_rows1024', 'c4_wide', 'c4_laplace'])
def test_bench_workloads_against_full_size_reference(name):
    """The workloads bench.py times, at FULL size, evidence-only, against the reference run at the same size
    (tests/golden/bench_*.npz from tests/golden/gen_bench_golden.py): logEvidence, forward localEvidence, per-point
    logEvidenceList and the hyper-parameter distribution at 1e-9."""
    import bench
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bench_%s.npz' % name))
    S, kw, units, desc = bench.make_study(bl, name)
    S.fit(silent=True, evidenceOnly=True)
    assert np.array_equal(np.asarray(S.rawData, dtype=float), gold['rawData'])
    assert abs(S.logEvidence - float(gold['logEvidence'])) <= 1e-9 * abs(float(gold['logEvidence']))
    np.testing.assert_allclose(S.localEvidence, gold['localEvidence'], rtol=1e-9, atol=0)
    if 'logEvidenceList' in gold.files:
        np.testing.assert_allclose(np.asarray(S.logEvidenceList), gold['logEvidenceList'], rtol=1e-9, atol=0)
        np.testing.assert_allclose(S.hyperParameterDistribution, gold['hyperParameterDistribution'], rtol=1e-9, atol=1e-300)
    S._posterior_pending = None
    bl.get_engine().release_posterior()


# ---- BASELINE.json grid sizes, short series: direct comparison with the oracle ---------------------------------------

FULL_SIZE = {
    'full_c4_512': dict(study='HyperStudy', data=('series', 4, 12), om=cases.gauss2d(512),
                        tm=('GRW', 'sigma', ('cint', 0, 0.3, 7), 'mean', None)),          # radii 0 .. 38: every bucket
    'full_c5_512': dict(study='ChangepointStudy', data=('series_jump', 5, 20, 10, 2.0), om=cases.gauss2d(512),
                        tm=('ChangePoint', 'tChange', ('arange', 3, 19, 4), None)),
    'full_fwd2048': dict(study='Study', data=('series', 3, 5), om=cases.gauss2d(2048),
                         tm=('Combined', [('GRW', 's1', 0.015, 'mean', None), ('GRW', 's2', 0.004, 'std', None)]),
                         fit=dict(evidenceOnly=True)),
    'full_c3_1024_fwd': dict(study='Study', data=('series', 9, 6), om=cases.gauss2d(1024),
                             tm=('Combined', [('GRW', 's1', 0.03, 'mean', None), ('GRW', 's2', 0.008, 'std', None)]),
                             fit=dict(forwardOnly=True)),
}


@pytest.mark.parametrize('case', list(FULL_SIZE))
def test_baseline_grid_sizes_match_oracle(case):
    c = FULL_SIZE[case]
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL)


def test_device_side_marginals():
    """blhip_posterior_marginal / _time_average against host reductions of the copied posterior (2-D and 1-D)."""
    for case in ('c3_small', 'c4_2hp', 'c1_coal'):
        S = cases.build(bl, case)
        S.fit(silent=True)
        names = S.observationModel.parameterNames
        got = [S.getParameterDistributions(n, density=False)[1] for n in names]
        avg = S.getParameterDistribution('avg', names[0], density=False)[1]
        assert S._posterior_pending is not None
        post = S.posteriorSequence
        for k in range(len(names)):
            axes = tuple(a + 1 for a in range(len(names)) if a != k)
            want = post.sum(axis=axes) if axes else post
            np.testing.assert_allclose(got[k], want, rtol=1e-12, atol=1e-300)
        axes = tuple(a for a in range(len(names)) if a != 0)
        want = post.mean(axis=0)
        np.testing.assert_allclose(avg, want.sum(axis=axes) if axes else want, rtol=1e-12, atol=1e-300)


@pytest.mark.gpu
def test_simulate_matches_reference_golden():
    """Study.simulate (core.py:566-597) on device-resident posteriors (time average / single row reads) vs the reference."""
    gold = oa.load_golden('simulate')
    for case in ('c1_coal', 'kat_gaussian', 'c4_small'):
        S = cases.build(bl, case)
        S.fit(**cases.fit_kwargs(case))
        x = gold[case + '_x']
        np.testing.assert_allclose(S.simulate(x), gold[case + '_avg'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(S.simulate(x, t=float(gold[case + '_t'])), gold[case + '_at'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(S.simulate(x, density=True), gold[case + '_avg_density'], rtol=1e-9, atol=1e-300)


@pytest.mark.gpu
def test_plugin_observation_models_on_device():
    """bl.om.SymPy / SciPy / NumPy (reference tests/test_observationmodels.py:11-120): host-evaluated likelihood tables,
    recursion on the GPU; the reference's log-evidence values (decimal=5 there)."""
    scipy_stats = pytest.importorskip('scipy.stats')
    sympy_stats = pytest.importorskip('sympy.stats')
    from sympy import Symbol

    def logE(L, data=np.array([1, 2, 3, 4, 5])):
        S = bl.Study(silent=True)
        S.loadData(data, silent=True)
        S.setOM(L, silent=True)
        S.setTM(bl.tm.Static(), silent=True)
        S.fit(silent=True)
        assert S.lastTiming['forward_launches'] > 0
        return S.logEvidence

    rate = Symbol('rate', positive=True)
    np.testing.assert_almost_equal(logE(bl.om.SymPy(sympy_stats.Poisson('poisson', rate), 'rate', bl.oint(0, 7, 100))),
                                   -10.238278174965238, decimal=9)
    mu, std = Symbol('mu'), Symbol('std', positive=True)
    np.testing.assert_almost_equal(logE(bl.om.SymPy(sympy_stats.Normal('norm', mu, std), 'mu', bl.cint(0, 7, 200), 'std',
                                                    bl.oint(0, 1, 200), prior=lambda x, y: 1.)), -13.663836264357226, decimal=9)
    np.testing.assert_almost_equal(logE(bl.om.SciPy(scipy_stats.poisson, 'mu', bl.oint(0, 7, 100), fixedParameters={'loc': 0})),
                                   -10.238278174965238, decimal=9)
    np.testing.assert_almost_equal(logE(bl.om.SciPy(scipy_stats.norm, 'loc', bl.cint(0, 7, 200), 'scale', bl.oint(0, 1, 200))),
                                   -13.663836264357225, decimal=9)


@pytest.mark.gpu
def test_matrix_pipe_lean_kernels_partial_column_blocks():
    """LEAN matrix-pipe kernels on a grid whose last 64-column block is mostly empty (450 columns: three of its four waves
    own no column) -- the in-place posterior of the backward step must only be touched by the owning lanes.  Compared with
    the vector-ALU kernels (mfma=0), several times (a race would not show every time)."""
    eng = bl.get_engine()

    def fit(**opts):
        for k, v in opts.items():
            eng.set_option(k, v)
        try:
            S = bl.HyperStudy(silent=True)
            S.loadData(cases.series(77, 10), silent=True)
            S.set(bl.om.Gaussian('mean', bl.cint(-6, 6, 256), 'std', bl.oint(0, 3, 450)),
                  bl.tm.GaussianRandomWalk('sigma', bl.cint(0.1, 0.45, 6), target='mean'), silent=True)
            S.fit(silent=True)
            return S
        finally:
            for k in opts:
                eng.set_option(k, 1)

    # (chain_resident = 0: the grid is inside the envelope of the chain-resident kernels since they take padded grids)
    B = fit(mfma=0, chain_resident=0)
    assert B.lastTiming['bwd_kernel_variant'] == 1
    want = np.array(B.posteriorSequence)
    for _ in range(4):
        A = fit(chain_resident=0)
        assert A.lastTiming['bwd_kernel_variant'] == 3
        assert abs(A.logEvidence - B.logEvidence) <= 1e-11 * abs(B.logEvidence)
        np.testing.assert_allclose(A.posteriorSequence, want, rtol=1e-9, atol=1e-14)
        np.testing.assert_allclose(A.posteriorMeanValues, B.posteriorMeanValues, rtol=1e-10)


@pytest.mark.gpu
def test_plain_c_program_through_the_abi(tmp_path):
    """examples/c_abi_demo.c: the coal-mining fit driven from C, no Python in the call path."""
    import shutil
    import subprocess
    from bayesloop_amd import _abi
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'c_abi_demo')
    libdir = os.path.dirname(_abi.library_path())
    subprocess.run(['gcc', '-std=c99', '-O2', '-I' + os.path.join(root, 'include'), os.path.join(root, 'examples', 'c_abi_demo.c'),
                    '-o', exe, '-L' + libdir, '-lblhip', '-Wl,-rpath,' + libdir, '-lm'], check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'log-evidence -171.6867218' in out.stdout


# A denormal likelihood value carries 1..52 significant bits; post / L at such a cell can dominate sum(post / L).  Seen in 3
# of 6000 random configurations: 1.6e-3 relative difference in ONE backward local-evidence entry, everything else < 1e-9.
from tolerances import ILL_LOCAL_RTOL   # noqa: E402  (registered exception ILL_LOCAL_EVIDENCE, tests/tolerances.py)


def _pin_hyper_chains(S, loose, liks):
    """What ILL_LOCAL_EVIDENCE leaves open for a HYPER-study, pinned at the bar.  Its localEvidence is the prior-weighted sum of
    the chains' (core.py:1410); a chain's entry 1 / (sum(post / L) dV) (core.py:463) is ill-conditioned only through the cells whose likelihood
    is denormal.  The chains are fitted once more as a BATCH that keeps its posteriors (the C-ABI's blhip_fit with BLHIP_KEEP_POSTERIOR: the
    batch kernels' storing flavour), and per chain the oracle (the test double's engine: the same FitProblem, chain by chain): at the loosened
    steps sum(post / L) over the cells whose likelihood is WELL inside the normal range must agree to 1e-9 on both sides, at every other
    step the chain's localEvidence itself.  ("Well inside": L >= 1e-290.  Next to the denormal range alpha = prior L / norm is itself a
    denormal number, rounded differently by the reference's order of operations -- (prior L) / norm -- and the kernels' -- (prior / norm) L --;
    such cells carry the same few-bit noise as the denormal-likelihood ones: first seen on seeded configuration 15, 3.6e-9.)  -> True when
    every chain was pinned (compare.check then counts the loosened entries of the comparison as pinned)."""
    from oracle_engine import OracleEngine
    T, gs = len(S.formattedData), list(S.gridSize)
    hv = np.asarray(S.hyperGridValues, dtype=float)
    if len(hv) < 2 or len(hv) > 96 or len(hv) * T * int(np.prod(gs)) > 6e7:
        return False
    S._setAllHyperParameters(S.hyperGridValues[0])
    try:
        problem, program = S._compile(silent=True)
    finally:
        S._setAllHyperParameters(S.flatHyperParameters)
    opv = S._opValueMatrix(program, hv)
    eng, oe = bl.get_engine(), OracleEngine()
    res = eng.fit(problem, opv, keep_posterior=True, owner=None)
    tiny = 1e-290
    for k in range(len(opv)):
        with np.errstate(all='ignore'):
            ro = oe.fit(problem, opv[k:k + 1], keep_posterior=True)
        if not np.isfinite(ro.log_evidence[0]):
            assert not np.isfinite(res.log_evidence[k])
            continue
        assert abs(res.log_evidence[k] - ro.log_evidence[0]) <= 1e-9 * abs(ro.log_evidence[0]), (k, res.log_evidence[k], ro.log_evidence[0])
        pg, pw = np.asarray(eng.posterior(k, T, gs)), np.asarray(oe.posterior(0, T, gs))
        for t in range(T):
            lw, lg = ro.local_evidence[0, t], res.local_evidence[k, t]
            if not loose[t]:
                assert (np.isnan(lw) and np.isnan(lg)) or abs(lg - lw) <= 1e-9 * abs(lw), (k, t, lg, lw)
                continue
            L = liks[t] * np.ones(gs)
            normal = L >= tiny
            with np.errstate(all='ignore'):
                sg, sw = float(np.sum(pg[t][normal] / L[normal])), float(np.sum(pw[t][normal] / L[normal]))
            assert abs(sg - sw) <= 1e-9 * abs(sw) + 1e-300, 'chain %d step %d: sum(post / L) over the normal cells %r vs %r' % (k, t, sg, sw)
    eng.release_posterior(None)
    return True


def _ill_tol(S, pin=True):
    """The registered exception ILL_LOCAL_EVIDENCE as a per-STEP mask: only the localEvidence entries of steps whose likelihood has
    DENORMAL cells (0 < L < 2.2e-308) are compared at ILL_LOCAL_RTOL -- the backward value 1 / sum(post / L) (core.py:463) is then
    only defined to a few digits in the reference itself (see cases.py: wide_filter_2d).  Steps with exact zeros only are NaN (0/0)
    on both sides and need no tolerance; every other entry keeps the 1e-9 bar.  -> case_tol dict, or None if no step qualifies."""
    with np.errstate(all='ignore'):
        liks = [np.asarray(S.observationModel.processedPdf(S.grid, seg), dtype=float) for seg in S.formattedData]
        loose = np.array([bool(((L > 0) & (L < 2.2250738585072014e-308)).any()) for L in liks])
    if not loose.any():
        return None
    out = dict(local_rtol=ILL_LOCAL_RTOL, local_loose_steps=loose)
    if pin and type(S).__name__ in ('HyperStudy', 'ChangepointStudy'):      # (pin = False: tests that count the context's fits -- the pin is one more)
        out['local_pinned'] = _pin_hyper_chains(S, loose, liks)       # (compare.check counts the loosened entries of THIS comparison as pinned)
    if type(S).__name__ == 'Study':
        # ... and what the loosened comparison leaves open is pinned at the bar: the SAME sum with the denormal-likelihood cells left
        # out on both sides (compare.check: `local_lik`), from the stored posteriors and the likelihood of the step
        out['local_lik'] = {int(t): liks[t] * np.ones(S.gridSize) for t in np.flatnonzero(loose)}
    return out



@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_FUZZ_SEEDS', 50))))     # more seeds: BLHIP_FUZZ_SEEDS=400
def test_seeded_random_configurations_match_oracle(seed):
    c = random_cases.random_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


# seeds that once failed: 434 / 1006 / 1110 = Deterministic shifts whose cubic-spline ringing makes a lazily dropped normaliser
# NEGATIVE (the zero-normaliser test must follow the reference's sign), 1258 = denormal likelihood without an exact zero,
# 1032 / 2228 = every / one chain of a hyper-study stops with a zero normaliser (logsumexp of all -inf, left-over local evidence)
ZOO_REGRESSION_SEEDS = [434, 1006, 1032, 1110, 1258, 2228]


@pytest.mark.parametrize('seed', list(range(int(os.environ.get('BLHIP_FUZZ_SEEDS', 39)))) + ZOO_REGRESSION_SEEDS)
def test_seeded_random_model_zoo_matches_oracle(seed):
    c, tol = random_cases.random_model_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    if 'logEvidenceList' in want and not np.all(np.isfinite(np.asarray(want['logEvidenceList'], dtype=float))):
        # a chain that stops with a zero normaliser leaves the rest of its localEvidence array as np.empty() left it in the
        # reference (core.py:360, :399): the hyper-study's sum over chains (core.py:1410) is then not defined
        got['localEvidence'] = gold['localEvidence']
    if _ill_tol(S) is not None:
        tol = dict(tol or {}, **_ill_tol(S))
    compare.check(got, gold, compare.GPU_TOL, case_tol=tol)


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_FUZZ_SEEDS', 36))))
def test_seeded_random_wide_axis1_walks_match_oracle(seed):
    """Random walks on the second parameter with stencil radii 9 .. 64: the axis-1 pre-pass in front of the streaming kernels."""
    c = random_cases.random_wide_axis1_case(seed)
    eng = bl.get_engine()
    eng.set_option('chain_ax1', 0)           # (the pre-pass path is what this test covers; the transposing kernels have their own seeds)
    try:
        S = cases.build(bl, c)
        with np.errstate(all='ignore'):
            S.fit(**cases.fit_kwargs(c))
            want = oa.run(c)
    finally:
        eng.set_option('chain_ax1', 1)
    # ... and whatever the default routing picks for the same study agrees with it
    D = cases.build(bl, c)
    with np.errstate(all='ignore'):
        D.fit(**cases.fit_kwargs(c))
    # (two summation orders of the same study: the bar itself -- 400 seeds: up to 3.6e-11 absolute on a logEvidence of -2.96)
    assert (np.isnan(D.logEvidence) and np.isnan(S.logEvidence)) or D.logEvidence == S.logEvidence or \
        abs(D.logEvidence - S.logEvidence) <= compare.GPU_TOL['logE_rtol'] * abs(S.logEvidence)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    # not the generic kernel -- unless the grid is outside the streaming kernels' envelope (rows < rounded axis-0 radius + 16, axis-1 radius > 256)
    n0, n1 = [int(v) for v in S.gridSize]
    def radius(tm, name, delta):
        vals = [np.max(np.atleast_1d(t[2] if not isinstance(t[2], tuple) else t[2][2])) for t in (tm[1] if tm[0] == 'Combined' else [tm]) if t[0] == 'GRW' and t[3] == name]
        return int(4.0 * max(vals) / delta + 0.5) if vals else 0
    lw0, lw1 = radius(c['tm'], 'mean', 10.0 / (n0 - 1)), radius(c['tm'], 'std', 3.0 / (n1 + 1))
    if lw1 <= 256 and (n0 >= (lw0 + 7) // 8 * 8 + 16 if lw0 <= 40 else (lw0 <= 128 and lw0 < n0)):
        # (6: no walk on the second parameter in this draw and the one on the first fits the chain-resident kernels' bands)
        assert S.lastTiming['fwd_kernel_variant'] in (1, 3) or (lw1 == 0 and S.lastTiming['fwd_kernel_variant'] == 6), (lw0, lw1, n0, n1, S.lastTiming)


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_FUZZ_SEEDS', 54))))
def test_seeded_random_both_axes_walks_on_square_grids_take_the_transposing_chain_kernels(seed):
    """Random walks on BOTH parameters of a square grid (128 / 256 points per axis, radii up to 40): blc::chainax_kernel keeps the chains
    resident and transposes the distribution between the two filters (blhip_chainax.hpp) -- against the oracle at the parity bar, and
    against the launch-per-step path (option chain_ax1 = 0: pre-pass + streaming kernels) of the same build."""
    c = random_cases.random_both_axes_square_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    tm = S.lastTiming
    ok = (6,) if c['study'] != 'Study' else (5, 6)          # (a single chain with radii <= 8 on both axes: the time-resident kernel)
    n0, n1 = [int(v) for v in S.gridSize]
    if min(n0, n1) >= 72:          # (smaller grids with walks of radius ~40 are outside the streaming / resident kernels' envelope altogether)
        assert tm['fwd_kernel_variant'] in ok and tm['resident_fallbacks'] == 0, tm
        if not (c['fit'].get('evidenceOnly') or c['fit'].get('forwardOnly')):
            assert tm['bwd_kernel_variant'] in ok, tm
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    eng = bl.get_engine()
    eng.set_option('chain_ax1', 0)
    try:
        S0 = cases.build(bl, c)
        with np.errstate(all='ignore'):
            S0.fit(**cases.fit_kwargs(c))
        assert S0.lastTiming['fwd_kernel_variant'] != 6 or c['study'] == 'Study', S0.lastTiming
    finally:
        eng.set_option('chain_ax1', 1)
    np.testing.assert_allclose(S.logEvidence, S0.logEvidence, rtol=1e-11)
    if seed % 5 == 0:              # bit-stable from run to run (fixed summation orders, no atomics; the exchange carries values, not sums)
        S1 = cases.build(bl, c)
        with np.errstate(all='ignore'):
            S1.fit(**cases.fit_kwargs(c))
        assert S1.logEvidence == S.logEvidence and np.array_equal(np.asarray(S1.localEvidence), np.asarray(S.localEvidence), equal_nan=True)
        if 'posteriorSequence' in got:
            assert np.array_equal(np.asarray(S1.posteriorSequence), np.asarray(got['posteriorSequence']), equal_nan=True)


@pytest.mark.parametrize('T', [1, 2])
@pytest.mark.parametrize('kind', ['study', 'hyper', 'hyper_evidence', 'study_forward_only'])
def test_both_axes_walks_over_one_and_two_time_steps(T, kind):
    """The transposing kernels alternate their layout with the time index (blk::ax_layout_b): series of ONE step (no transition at all) and of
    TWO (one exchange; the backward pass starts in the other layout than the forward pass ended in)."""
    om = ('Gaussian', [('mean', ('cint', -5, 5, 128)), ('std', ('oint', 0, 3, 128))], 'default')
    s1, s2 = 20 / 4.0 * 10 / 127, 14 / 4.0 * 3 / 129
    walks = lambda a, b: ('Combined', [('GRW', 's1', a, 'mean', None), ('GRW', 's2', b, 'std', None)])
    c = dict(study='Study', data=('series', 4242, T), om=om, fit=dict(), tm=walks(s1, s2))
    if kind.startswith('hyper'):
        c = dict(c, study='HyperStudy', tm=walks(('cint', 0, s1, 3), ('cint', 0, s2, 3)), fit=dict(evidenceOnly=True) if kind == 'hyper_evidence' else dict())
    if kind == 'study_forward_only':
        c = dict(c, fit=dict(forwardOnly=True))
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_FUZZ_SEEDS', 32))))
def test_seeded_random_hyper_studies_match_oracle(seed):
    c = random_cases.random_hyper_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    if 'logEvidenceList' in want and not np.all(np.isfinite(np.asarray(want['logEvidenceList'], dtype=float))):
        got['localEvidence'] = gold['localEvidence']         # (np.empty left-overs of stopped chains, see the model-zoo test)
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


def test_online_study_survives_pickling_on_device():
    """blhip_carry_read / blhip_carry_write: a pickled OnlineStudy re-creates its carried filter states in slots of its own and
    continues independently of the original (reference fileIO.py:10-37)."""
    import contextlib
    import io
    import pickle
    data = np.array([1.0, 2.0, 3.0, 2.0, 4.0, 3.0])

    def make():
        O = bl.OnlineStudy(storeHistory=True, silent=True)
        O.set(bl.om.Poisson('rate', bl.oint(0, 6, 50)), silent=True)
        O.add('static', bl.tm.Static())
        O.add('grw', bl.tm.GaussianRandomWalk('sigma', [0.1, 0.3], target='rate'))
        O.add('ne', bl.tm.NotEqual('pmin', -3))
        return O
    with contextlib.redirect_stdout(io.StringIO()):
        A = make()
        for x in data[:3]:
            A.step(x)
        B = pickle.loads(pickle.dumps(A))
        for x in data[3:]:
            B.step(x)
        for x in data[3:]:
            A.step(x)
        R = make()
        for x in data:
            R.step(x)
    for O in (A, B):
        np.testing.assert_allclose(O.logEvidence, R.logEvidence, rtol=1e-12)
        np.testing.assert_allclose(O.marginalizedPosterior, R.marginalizedPosterior, rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(O.transitionModelDistribution, R.transitionModelDistribution, rtol=1e-11)
    del B
    with contextlib.redirect_stdout(io.StringIO()):
        A.step(2.0)
    assert np.isfinite(A.logEvidence)


# ---- the time-resident kernel (blhip_resident.hpp): one launch per pass, tiles in LDS, halo strips between tiles ------------------

def _g2(n0, n1, lo=-8, hi=8, smax=4):
    return ('Gaussian', [('mean', cases._g('cint', lo, hi, n0)), ('std', cases._g('oint', 0, smax, n1))], 'default')


def _grw2(s1, s2):
    return ('Combined', [('GRW', 's1', s1, 'mean', None), ('GRW', 's2', s2, 'std', None)])


RESIDENT = {
    # tiles 32 x 32: 6 tiles, every kind of tile edge (grid edge / neighbour) on both axes; full fit
    'res_64x96_full': dict(study='Study', data=('series', 21, 9), om=_g2(64, 96), tm=_grw2(0.45, 0.08)),
    # missing data points, lag reaching over them
    'res_96x64_nan': dict(study='Study', data=('series_nan', 22, 11, [0, 4, 5]), om=_g2(96, 64), tm=_grw2(0.3, 0.12)),
    # forward-only: filtered posteriors + means
    'res_128_fwdonly': dict(study='Study', data=('series', 23, 8), om=_g2(128, 128), tm=_grw2(0.25, 0.06),
                            fit=dict(forwardOnly=True)),
    'res_256x128_evid': dict(study='Study', data=('series', 24, 12), om=_g2(256, 128), tm=_grw2(0.12, 0.06),
                             fit=dict(evidenceOnly=True)),
    # one filtered axis only / no filter at all on the other (identity pass)
    'res_128_axis0': dict(study='Study', data=('series', 25, 7), om=_g2(128, 64), tm=('GRW', 's1', 0.25, 'mean', None)),
    'res_128_axis1': dict(study='Study', data=('series', 26, 7), om=_g2(64, 128), tm=('GRW', 's2', 0.06, 'std', None)),
    'res_64_static': dict(study='Study', data=('series', 27, 6), om=_g2(64, 64), tm=('Static',)),
    # two data dimensions per step (product of likelihoods, one of them missing at one step)
    'res_96_multidim': dict(study='Study', data=('series2d', 28, 9), om=_g2(96, 96, -4, 4, 3), tm=_grw2(0.16, 0.06)),
    # T = 1 and T = 2 (shorter than the lag)
    'res_T1': dict(study='Study', data=('series', 29, 1), om=_g2(64, 64), tm=_grw2(0.3, 0.1)),
    'res_T2': dict(study='Study', data=('series', 30, 2), om=_g2(64, 64), tm=_grw2(0.3, 0.1)),
    # tiles 64 x 64 (128 tiles) and 128 x 128 (32 tiles)
    'res_1024x512_full': dict(study='Study', data=('series', 31, 5), om=_g2(1024, 512), tm=_grw2(0.03, 0.016)),
    'res_2048x256_full': dict(study='Study', data=('series', 32, 4), om=_g2(2048, 256), tm=_grw2(0.015, 0.03)),
    # 64 x 64 tiles: 3 x 3 (an interior tile with neighbours on every side), one tile row, one tile column
    'res_192_full': dict(study='Study', data=('series', 42, 7), om=_g2(192, 192), tm=_grw2(0.16, 0.04)),
    'res_64x256_full': dict(study='Study', data=('series', 43, 6), om=_g2(64, 256), tm=_grw2(0.4, 0.03)),
    'res_256x64_fwdonly': dict(study='Study', data=('series', 44, 6), om=_g2(256, 64), tm=_grw2(0.1, 0.12), fit=dict(forwardOnly=True)),
    # tiles 32 x 64 (256 tiles)
    'res_512x1024_full': dict(study='Study', data=('series', 33, 5), om=_g2(512, 1024), tm=_grw2(0.06, 0.008)),
    # grids that do not fill their last tile row / column (PAD kernels: mirror image beyond the true edge, masked cells)
    'res_pad_200x100_full': dict(study='Study', data=('series', 34, 9), om=_g2(200, 100), tm=_grw2(0.15, 0.07)),                   # 32 x 64 tiles, 7 x 2
    'res_pad_88x72_nan': dict(study='Study', data=('series_nan', 35, 10, [1, 6]), om=_g2(88, 72), tm=_grw2(0.35, 0.1)),           # smallest padding / remainder
    'res_pad_300x500_fwdonly': dict(study='Study', data=('series', 36, 7), om=_g2(300, 500), tm=_grw2(0.1, 0.015), fit=dict(forwardOnly=True)),
    'res_pad_168x120_axis1': dict(study='Study', data=('series', 37, 8), om=_g2(168, 120), tm=('GRW', 's2', 0.06, 'std', None)),
    'res_pad_1000_evid': dict(study='Study', data=('series', 38, 6), om=_g2(1000, 1000), tm=_grw2(0.03, 0.008), fit=dict(evidenceOnly=True)),   # 64 x 64 tiles, 256
    'res_pad_1000x520_full': dict(study='Study', data=('series', 39, 4), om=_g2(1000, 520), tm=_grw2(0.03, 0.015)),                # 64 x 64 tiles, 16 x 9
    'res_pad_2060x1100_fwdonly': dict(study='Study', data=('series', 41, 3), om=_g2(2060, 1100), tm=_grw2(0.015, 0.007), fit=dict(forwardOnly=True)),   # 128 x 128 tiles, 12 rows in the last tile row: the
                                                                                                                                    # first segment's walk starts in the padding
    'res_pad_2000x1100_evid': dict(study='Study', data=('series', 40, 3), om=_g2(2000, 1100), tm=_grw2(0.015, 0.007), fit=dict(evidenceOnly=True)),     # 128 x 128 tiles, 16 x 9 (full fits of
                                                                                                                                    # padded 128 x 128 grids keep the launch-per-step kernels)
}


@pytest.mark.parametrize('case', list(RESIDENT))
def test_resident_kernel_matches_oracle(case):
    c = RESIDENT[case]
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    assert S.lastTiming['fwd_kernel_variant'] == 5, S.lastTiming          # the resident path really ran
    if not cases.fit_kwargs(c).get('evidenceOnly') and not cases.fit_kwargs(c).get('forwardOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 5, S.lastTiming
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues'):
        if k in want and want[k] is not None and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_FUZZ_SEEDS', 36))))
def test_seeded_random_resident_grids_match_oracle(seed):
    """Random single-chain studies on grids of random sizes (most of them not whole tiles: the PAD variants of the time-resident kernel)."""
    c = random_cases.random_resident_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['fwd_kernel_variant'] == 5 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


def test_resident_kernel_degenerate_fit_does_not_stall():
    """A data point no grid cell can explain (likelihood exactly zero everywhere): the normaliser is zero, the states turn inf / NaN.  The
    tiles' hand-off (tag = sign bit of the value) accepts NaN elements, the host rejects the pass by its sums and the launch-per-step
    kernels reproduce the reference's result (logEvidence = -inf, core.py:390-400) -- without waiting for the resident kernel's time-out."""
    import time
    x = cases.series(28, 10)
    x[4] = 1.0e6
    c = dict(study='Study', data=x, om=_g2(128, 128), tm=_grw2(0.3, 0.1))
    S = cases.build(bl, c)
    t0 = time.time()
    with np.errstate(all='ignore'):
        S.fit(silent=True)
        want = oa.run(c)
    assert time.time() - t0 < 1.5                                   # (no in-kernel wait ran into its bound)
    # (a zero normaliser is the reference's ABORT, core.py:390-400, not a fall-back; if the pass was repeated, it says why)
    assert S.lastTiming['resident_fallbacks'] == 0 or S.lastTiming['resident_fallback_reason'] == 2, S.lastTiming       # BLHIP_FALLBACK_RANGE
    assert S.logEvidence == want['logEvidence'] == -np.inf


@pytest.mark.parametrize('lag', [1, 2, 3, 4])
def test_resident_kernel_lag_and_determinism(lag):
    """The lagged normaliser (resident_lag = 1 .. 4) only changes intermediate magnitudes; repeated runs are bit-identical
    (every sum has a fixed order: a hand-off race would show as a difference between runs)."""
    eng = bl.get_engine()
    c = dict(study='Study', data=('series', 41, 14), om=_g2(256, 256), tm=_grw2(0.12, 0.03))
    eng.set_option('resident', 0)
    try:
        B = cases.build(bl, c); B.fit(silent=True)
        assert B.lastTiming['fwd_kernel_variant'] != 5
        base = np.array(B.posteriorSequence)
    finally:
        eng.set_option('resident', 1)
    eng.set_option('resident_lag', lag)
    try:
        runs = []
        for _ in range(3):
            A = cases.build(bl, c); A.fit(silent=True)
            assert A.lastTiming['fwd_kernel_variant'] == 5 and A.lastTiming['bwd_kernel_variant'] == 5
            runs.append((A.logEvidence, np.array(A.posteriorSequence), np.array(A.localEvidence)))
    finally:
        eng.set_option('resident_lag', 2)
    for logE, post, loc in runs:
        assert abs(logE - B.logEvidence) <= 1e-11 * abs(B.logEvidence)
        np.testing.assert_allclose(post, base, rtol=1e-9, atol=1e-14)
        assert logE == runs[0][0] and np.array_equal(post, runs[0][1]) and np.array_equal(loc, runs[0][2], equal_nan=True)


def test_resident_kernel_full_chip():
    """256 tiles (one per CU): 2048 x 2048 forward (tiles 128 x 128) and 1024 x 1024 full fit (tiles 64 x 64) against the
    launch-per-step kernels, which the tests above and the goldens pin to the oracle / the reference."""
    eng = bl.get_engine()
    for c, T in ((dict(study='Study', data=('series', 3, 24), om=cases.gauss2d(2048), tm=_grw2(0.015, 0.004), fit=dict(evidenceOnly=True)), 24),
                 (dict(study='Study', data=('series', 3, 16), om=cases.gauss2d(1024), tm=_grw2(0.03, 0.008)), 16)):
        A = cases.build(bl, c); A.fit(**cases.fit_kwargs(c))
        assert A.lastTiming['fwd_kernel_variant'] == 5, A.lastTiming
        eng.set_option('resident', 0)
        try:
            B = cases.build(bl, c); B.fit(**cases.fit_kwargs(c))
            assert B.lastTiming['fwd_kernel_variant'] != 5
        finally:
            eng.set_option('resident', 1)
        assert abs(A.logEvidence - B.logEvidence) <= 1e-11 * abs(B.logEvidence)
        np.testing.assert_allclose(A.localEvidence, B.localEvidence, rtol=1e-9, atol=0, equal_nan=True)
        if not cases.fit_kwargs(c).get('evidenceOnly'):
            np.testing.assert_allclose(A.posteriorMeanValues, B.posteriorMeanValues, rtol=1e-10)
            for k in (0, 1):
                np.testing.assert_allclose(A.getParameterDistributions(A.observationModel.parameterNames[k], density=False)[1],
                                           B.getParameterDistributions(B.observationModel.parameterNames[k], density=False)[1],
                                           rtol=1e-9, atol=1e-14)
            np.testing.assert_allclose(A.posteriorSequence[T // 2], B.posteriorSequence[T // 2], rtol=1e-9, atol=1e-14)
        for S_ in (A, B):
            S_._posterior_pending = None
        eng.release_posterior()


def test_one_dimensional_batches_on_the_chain_resident_kernel_match_the_goldens():
    """bl1c::chain1d_kernel (one block per chain runs a whole pass of a 1-D study: blhip_chain1d.hpp), forced (`chain1d = 2`) for every
    fixture it is eligible for -- the reference's 1-D hyper- / change-point studies and single fits, Poisson / GaussianMean / tabulated
    likelihoods, random walks, change- and break-points, forward-only and evidence-only fits -- against the reference's goldens."""
    eng = bl.get_engine()
    took = []
    eng.set_option('chain1d', 2)
    try:
        for case, c in cases.CASES.items():
            if len(c['om'][1]) != 1 or c['study'] == 'OnlineStudy':
                continue
            S = cases.build(bl, case)
            with np.errstate(all='ignore'):
                S.fit(**cases.fit_kwargs(case))
            if S.lastTiming.get('fwd_kernel_variant') != 9:
                continue
            took.append(case)
            compare.check(result_of(S, case), oa.load_golden(case), compare.GPU_TOL, case_tol=cases.CASES[case].get('tol'))
    finally:
        eng.set_option('chain1d', 1)
    assert len(took) >= 12 and 'c1_coal_hyper' in took and 'c1_coal' in took, took


@pytest.mark.parametrize('case', ['kat_deterministic', 'serial_deterministic_bp', 'serial_deterministic_offset'])
def test_deterministic_steps_on_the_chain_resident_kernel(case):
    """Batches of 1-D chains whose programs contain Deterministic steps (spline shifts: clamp mode 6) run on the chain-resident
    kernel's SHIFT flavour (bl1c::chain1d_kernel<.., SHIFT>: asymmetric stencil over SciPy's 'nearest' extension, two-stage form
    beyond 12 cells, the shifted mass as one more sum per step); `chain1d_shift = 0` keeps them on the launch-per-step kernel.  Both
    against the reference's golden, and against each other."""
    eng = bl.get_engine()
    A = cases.build(bl, case)
    with np.errstate(all='ignore'):
        A.fit(**cases.fit_kwargs(case))
    assert A.lastTiming['fwd_kernel_variant'] == 9, A.lastTiming
    if not cases.fit_kwargs(case).get('evidenceOnly'):
        assert A.lastTiming['bwd_kernel_variant'] == 9, A.lastTiming
    compare.check(result_of(A, case), oa.load_golden(case), compare.GPU_TOL, case_tol=cases.CASES[case].get('tol'))
    eng.set_option('chain1d_shift', 0)
    try:
        B = cases.build(bl, case)
        with np.errstate(all='ignore'):
            B.fit(**cases.fit_kwargs(case))
    finally:
        eng.set_option('chain1d_shift', 1)
    assert B.lastTiming['fwd_kernel_variant'] == 0, B.lastTiming
    la, lb = np.asarray(A.logEvidenceList, dtype=float), np.asarray(B.logEvidenceList, dtype=float)
    assert np.array_equal(np.isfinite(la), np.isfinite(lb))
    np.testing.assert_allclose(la[np.isfinite(la)], lb[np.isfinite(lb)], rtol=1e-11)
    assert abs(A.logEvidence - B.logEvidence) <= 1e-11 * abs(B.logEvidence)


@pytest.mark.parametrize('name', ['c1_hyper', 'coal_hyper1000'])
def test_one_dimensional_hyper_studies_of_the_bench_against_full_size_reference(name):
    """bench.py's 1-D hyper-studies (SURVEY 8c's anchor C1-as-HyperStudy; the tutorial's 1000-point grid with 256 widths up to 667 grid
    steps) on the chain-resident 1-D kernel against the reference's own runs: evidences per chain and of the average model,
    hyper-parameter distribution, average posterior sequence, means, local evidence."""
    import bench
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bench_%s_full.npz' % name))
    S, kw, units, desc = bench.make_study(bl, name)
    with np.errstate(all='ignore'):
        S.fit(silent=True)
    assert S.lastTiming['fwd_kernel_variant'] == 9 and S.lastTiming['bwd_kernel_variant'] == 9, S.lastTiming
    assert abs(S.logEvidence - float(gold['logEvidence'])) <= 1e-9 * abs(float(gold['logEvidence']))
    if name == 'c1_hyper':
        assert abs(S.logEvidence - (-172.6703099789132)) < 1e-9 * 172.67
    np.testing.assert_allclose(np.asarray(S.logEvidenceList, dtype=float), gold['logEvidenceList'], rtol=1e-9)
    np.testing.assert_allclose(S.hyperParameterDistribution, gold['hyperParameterDistribution'], rtol=1e-9, atol=1e-300)
    ge = gold['localEvidence']
    np.testing.assert_allclose(np.asarray(S.localEvidence)[~np.isnan(ge)], ge[~np.isnan(ge)], rtol=1e-9, atol=0)
    post, want = np.asarray(S.posteriorSequence), gold['posteriorSequence']
    assert np.all(np.abs(post - want) <= 1e-12 + 1e-9 * np.abs(want))
    np.testing.assert_allclose(S.posteriorMeanValues, gold['posteriorMeanValues'], rtol=1e-9, atol=1e-11)


def test_the_references_published_break_point_study_at_full_size():
    """The one heavy workload the reference publishes (docs/source/tutorials/changepointstudy.ipynb, "Analyzing structural breaks":
    coal-mining disasters 1870-1910, Serial(Static, BreakPoint, Deterministic(30 slopes), BreakPoint, Static) on a 1000-point Poisson
    grid: 23 400 fits with shifts of up to 334 grid cells per step) against the reference's own run of it: every chain's evidence, the
    evidence of the average model, the hyper-parameter distribution over all 48 000 combinations, the distribution of the duration
    t_2 - t_1 the tutorial reads off, the average posterior sequence and its means.  Registered exception COAL_NOISE_CHAINS
    (tests/tolerances.py): a handful of chains whose backward message is shifted off the grid are decided by rounding noise in the
    reference (it renormalises a sum of 1e-75); they may differ in whether they stop, nothing else may."""
    import bench
    from scipy.special import logsumexp
    from tolerances import COAL_NOISE_TOL
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bench_coal_breakpoints_full.npz'))
    S, kw, units, desc = bench.make_study(bl, 'coal_breakpoints')
    with np.errstate(all='ignore'):
        S.fit(silent=True)
    assert S.lastTiming['fwd_kernel_variant'] == 9 and S.lastTiming['bwd_kernel_variant'] == 9, S.lastTiming      # (bl1c::chain1d_kernel, SHIFT)
    gl, rl = gold['logEvidenceList'], np.asarray(S.logEvidenceList, dtype=float)
    assert len(rl) == 23400
    both = np.isfinite(gl) & np.isfinite(rl)
    np.testing.assert_allclose(rl[both], gl[both], rtol=1e-9)                       # every chain that runs through on both sides
    # the 14 chains that stop in the reference stop here (SciPy's prefilter recursion on the device: round 5; its truncated response
    # stopped 3 of them); whether a chain of this kind stops is decided by the sign of rounding noise (tests/test_oracle_golden.py:
    # +-2 ulp on the prefilter's input flips them), so a registered handful may differ -- observed: ONE more chain stops here
    assert (~np.isfinite(gl)).sum() == 14
    noise = np.isfinite(rl) != np.isfinite(gl)
    assert noise.sum() <= COAL_NOISE_TOL['noise_chains'], (int((np.isfinite(rl) & ~np.isfinite(gl)).sum()), int((np.isfinite(gl) & ~np.isfinite(rl)).sum()))
    # evidence of the average model / hyper-parameter distribution (core.py:1391-1405) from the chains with the reference's stop pattern
    # (a chain that stops only here enters with the reference's value)
    prior = np.asarray(S.flatHyperPriorValues, dtype=float)[S.mask]
    with np.errstate(divide='ignore'):
        logHPD = np.where(np.isfinite(gl), np.where(np.isfinite(rl), rl, gl), -np.inf) + np.log(prior) + np.sum(np.log(S.hyperGridConstant))
    logE = float(logsumexp(logHPD))
    assert abs(logE - float(gold['logEvidence'])) <= 1e-9 * abs(float(gold['logEvidence']))
    assert abs(logE / np.log(10) - (-30.63948)) < 1e-3                              # the number printed in the tutorial (another SciPy)
    # ... and the study's own logEvidence -- the noise chains included -- keeps the 1e-9 bar (observed 6e-10)
    assert abs(S.logEvidence - float(gold['logEvidence'])) <= COAL_NOISE_TOL['logE_rtol'] * abs(float(gold['logEvidence']))
    hpd = np.zeros(len(S.allHyperGridValues))
    hpd[S.mask] = np.exp(logHPD - logHPD.max()) / np.sum(np.exp(logHPD - logHPD.max())) / np.prod(S.hyperGridConstant)
    np.testing.assert_allclose(hpd, gold['hyperParameterDistribution'], rtol=1e-9, atol=1e-300)
    names = list(S.flatHyperParameterNames)
    hv = np.asarray(S.allHyperGridValues, dtype=float)
    dur = hv[:, names.index('t_2')] - hv[:, names.index('t_1')]
    dd = np.array([hpd[dur == d].sum() for d in gold['durations']]) / hpd.sum()
    np.testing.assert_allclose(dd, gold['durationDistribution'], rtol=1e-9, atol=1e-300)
    # what the study object itself reports includes the chain(s) that differ: their weight in the average model is ~4e-8, but a chain the
    # reference keeps there is renormalised NOISE (signed cell values up to ~1400): registered absolute bounds (tests/tolerances.py)
    w = abs(1.0 - np.exp(logE - S.logEvidence))
    assert w <= COAL_NOISE_TOL['noise_weight_max'], w
    d2, p2 = S.getDurationDistribution(['t_1', 't_2'])
    keep = np.isin(gold['durations'], d2)
    ref_dd = gold['durationDistribution'][keep] / gold['durationDistribution'][keep].sum()
    assert np.all(np.abs(p2 - ref_dd) <= COAL_NOISE_TOL['duration_rtol'] * ref_dd)
    post, want = np.asarray(S.posteriorSequence), gold['posteriorSequence']
    assert np.all(np.abs(post - want) <= COAL_NOISE_TOL['post_atol'])
    assert np.all(np.abs(np.asarray(S.posteriorMeanValues) - gold['posteriorMeanValues']) <= COAL_NOISE_TOL['mean_atol'])


@pytest.mark.parametrize('name', ['c3', 'c4', 'c5', 'c4_both_axes', 'c4_rows1024', 'c4_wide', 'c4_laplace'])
def test_bench_workloads_full_fit_against_full_size_reference(name):
    """C3 (T = 2000, 16 GiB posterior), C4 (512 chains, T = 256) and C5 (250 change-points, T = 1000) as FULL forward-backward fits against the reference's own
    full-size results (tests/golden/bench_<name>_full.npz): log-evidence, local evidence, posterior means, both marginals of the
    (average) posterior sequence (reduced on the device) and strided posterior rows."""
    import bench
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bench_%s_full.npz' % name))
    S, kw, units, desc = bench.make_study(bl, name)
    S.fit(silent=True)
    if name == 'c4_both_axes':           # (round 5: the transposing chain-resident kernels, blhip_chainax.hpp)
        assert S.lastTiming['fwd_kernel_variant'] == 6 and S.lastTiming['bwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    assert abs(S.logEvidence - float(gold['logEvidence'])) <= 1e-9 * abs(float(gold['logEvidence']))
    ge = gold['localEvidence']
    assert np.array_equal(np.isnan(S.localEvidence), np.isnan(ge))
    np.testing.assert_allclose(S.localEvidence[~np.isnan(ge)], ge[~np.isnan(ge)], rtol=1e-9, atol=0)
    np.testing.assert_allclose(S.posteriorMeanValues, gold['posteriorMeanValues'], rtol=1e-9, atol=1e-11)
    if 'hyperParameterDistribution' in gold.files:
        np.testing.assert_allclose(S.hyperParameterDistribution, gold['hyperParameterDistribution'], rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(np.asarray(S.logEvidenceList, dtype=float), gold['logEvidenceList'], rtol=1e-9)
    tidx = gold['marginalTimeIndex'] if 'marginalTimeIndex' in gold.files else np.arange(gold['marginalSequence0'].shape[0])
    names = S.observationModel.parameterNames
    for k in (0, 1):
        got = S.getParameterDistributions(names[k], density=False)[1][tidx]
        want = gold['marginalSequence%d' % k]
        assert np.all(np.abs(got - want) <= 1e-12 + 1e-9 * np.abs(want)), 'marginal %d' % k
    stride = [int(x) for x in gold['posteriorRowsStride']]
    for t, want in zip(gold['posteriorRowsIndex'], gold['posteriorRows']):
        got = S._posterior_pending.row(int(t))[::stride[0], ::stride[1]]
        assert np.all(np.abs(got - want) <= 1e-12 + 1e-9 * np.abs(want)), 'posterior row %d' % t
    S._posterior_pending = None
    bl.get_engine().release_posterior()


# ---- the chain-resident kernel (blhip_chainres.hpp): hyper-studies over one random-walk width, rounds of chains resident in LDS ------

def _hyper(n0, n1, seed, T, sigmas, kind='series', extra=None, **fit):
    data = (kind, seed, T) if extra is None else (kind, seed, T, extra)
    c = dict(study='HyperStudy', data=data, om=_g2(n0, n1), tm=('GRW', 'sigma', sigmas, 'mean', None))
    if fit:
        c['fit'] = fit
    return c


CHAINRES = {
    # 3 strips, 9 widths from 0 (no filter) to radius 32: one launch, band of the widest chain
    'cres_128x48_full': _hyper(128, 48, 51, 9, ('cint', 0, 1.0, 9)),
    # 16 strips -> 16 chains per launch: 40 chains = 3 launches with bands of 16 + 2 x {16, 32, 40} columns
    'cres_128x256_rounds': _hyper(128, 256, 52, 6, ('cint', 0.01, 1.25, 40)),
    'cres_256x32_evidence': _hyper(256, 32, 53, 12, ('cint', 0, 0.6, 5), evidenceOnly=True),
    'cres_256x64_forward_only': _hyper(256, 64, 54, 7, ('cint', 0.05, 0.4, 4), forwardOnly=True),
    # missing data points, the lag reaching over them
    'cres_512x32_nan': _hyper(512, 32, 55, 11, ('cint', 0, 0.3, 6), kind='series_nan', extra=[0, 4, 5]),
    # two data dimensions per step (product of likelihoods)
    'cres_128x64_multidim': dict(study='HyperStudy', data=('series2d', 56, 8), om=_g2(128, 64, -4, 4, 3),
                                 tm=('GRW', 'sigma', ('cint', 0, 0.5, 5), 'mean', None)),
    # no stencil at all + one reset step per chain (change-point studies): the no-filter kernel, posteriors stored, separate fold
    'cres_changepoints_256x32': dict(study='ChangepointStudy', data=('series_jump', 59, 24, 11, 1.5), om=_g2(256, 32),
                                     tm=('ChangePoint', 'tChange', ('arange', 1, 23, 2), None)),
    'cres_changepoints_128x64_evidence': dict(study='ChangepointStudy', data=('series_jump', 60, 17, 8, -2.0), om=_g2(128, 64),
                                              tm=('ChangePoint', 'tChange', 'all', None), fit=dict(evidenceOnly=True)),
    # 64 strips per chain (every lane of the scale wave gathers one granule), 4 chains per launch
    'cres_128x1024_64_strips': _hyper(128, 1024, 65, 5, ('cint', 0.05, 0.9, 6)),
    # 1024 rows: ONE copy of the strip in LDS, the new state waits in registers for the step's barrier (blc::chain_kernel TALL); the
    # stored alpha of the backward pass in a ring of two tiles; full fit (single-chain fused fold), evidence-only, widest band (radius 40)
    'cres_1024x32_tall': _hyper(1024, 32, 66, 6, ('cint', 0.01, 0.15, 6)),
    'cres_1024x48_tall_evidence': _hyper(1024, 48, 67, 5, ('cint', 0.02, 0.12, 4), evidenceOnly=True),
    'cres_1024x16_tall_r40': _hyper(1024, 16, 68, 7, ('cint', 0.15, 0.156, 2)),
    # ... and the bands only the 1024-row kernels carry (radius 41 .. 80: rings of 26 .. 44 entries): narrow and wide chains in one study,
    # the widest band evidence-only, a forward-only fit
    'cres_1024x32_tall_wide': _hyper(1024, 32, 69, 6, ('cint', 0.1, 0.31, 7)),
    'cres_1024x16_tall_r80_evidence': _hyper(1024, 16, 70, 9, ('cint', 0.3, 0.312, 2), evidenceOnly=True),
    'cres_1024x16_tall_wide_forward_only': _hyper(1024, 16, 71, 5, ('cint', 0.2, 0.3, 3), forwardOnly=True),
    # ... and grids of 513 .. 1023 rows / columns not a multiple of 16 on that geometry (padded cells hold zeros; the single-chain kernel folds
    # into partial accumulators on the padded geometry): the 1000 x 500 study the round-3 verdict named, a grid just above 512 rows
    # evidence-only, ragged columns only
    'cres_1000x500_tall_pad': _hyper(1000, 500, 72, 4, ('cint', 0.02, 0.3, 4)),
    'cres_600x40_tall_pad_evidence': _hyper(600, 40, 73, 6, ('cint', 0.05, 0.45, 3), evidenceOnly=True),
    'cres_1024x40_tall_pad_columns': _hyper(1024, 40, 74, 5, ('cint', 0.0, 0.2, 5)),
    # change-point studies on the 1024-row geometry (no stencil: the state of a lane's 32 cells stays in registers; posteriors stored and
    # folded separately -- the two-chain fold kernel stops at 512 rows), evidence-only also on a padded grid
    'cres_changepoints_1024x32': dict(study='ChangepointStudy', data=('series_jump', 82, 14, 6, 1.5), om=_g2(1024, 32),
                                      tm=('ChangePoint', 'tChange', ('arange', 1, 13, 2), None)),
    'cres_changepoints_700x24_evidence': dict(study='ChangepointStudy', data=('series_jump', 83, 11, 5, -2.0), om=_g2(700, 24),
                                              tm=('ChangePoint', 'tChange', 'all', None), fit=dict(evidenceOnly=True)),
    # bands beyond radius 40 on the geometries of <= 512 rows (rings of 26 .. 44 entries; the two-chain kernel keeps its band tables in the
    # compact form there): narrow and wide chains in one study, every geometry, padded grids, evidence-only / forward-only fits, a
    # change point inside wide filtering chains
    'cres_512x32_wide': _hyper(512, 32, 75, 6, ('cint', 0.1, 0.62, 9)),
    'cres_256x48_wide_r80': _hyper(256, 48, 76, 7, ('cint', 1.2, 1.25, 2)),
    'cres_128x32_wide_evidence': _hyper(128, 32, 77, 9, ('cint', 0.5, 2.4, 5), evidenceOnly=True),
    'cres_384x16_wide_forward_only': _hyper(384, 16, 78, 5, ('cint', 0.3, 0.8, 4), forwardOnly=True),
    'cres_300x40_wide_pad': _hyper(300, 40, 79, 6, ('cint', 0.2, 1.0, 7)),
    'cres_500x20_wide_pad_evidence': _hyper(500, 20, 80, 5, ('cint', 0.3, 0.6, 3), evidenceOnly=True),
    'cres_wide_mixed_cp_256x16': dict(study='ChangepointStudy', data=('series_jump', 81, 12, 5, -1.5), om=_g2(256, 16, -4, 6, 3),
                                      tm=('Combined', [('GRW', 'sigma', 0.6, 'mean', None), ('ChangePoint', 'tChange', ('arange', 1, 11, 2), None)])),
    # T = 1 and T = 2 (shorter than the lag)
    'cres_T1': _hyper(128, 32, 57, 1, ('cint', 0, 0.5, 3)),
    'cres_T2': _hyper(128, 32, 58, 2, ('cint', 0, 0.5, 3)),
}


@pytest.mark.parametrize('case', list(CHAINRES))
def test_chain_resident_kernel_matches_oracle(case):
    c = CHAINRES[case]
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    kw = cases.fit_kwargs(c)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming          # the chain-resident path really ran
    if not kw.get('evidenceOnly') and not kw.get('forwardOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 6, S.lastTiming
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('lag', [2, 3, 4])
def test_chain_resident_kernel_lag_and_determinism(lag):
    """Against the launch-per-step kernels; the lag of the normaliser only changes intermediate magnitudes; repeated runs are
    bit-identical (a race on a tagged sum would show as a difference between runs)."""
    eng = bl.get_engine()
    c = _hyper(256, 128, 61, 10, ('cint', 0, 0.6, 37))
    eng.set_option('chain_resident', 0)
    try:
        B = cases.build(bl, c); B.fit(silent=True)
        assert B.lastTiming['fwd_kernel_variant'] != 6
        base = np.array(B.posteriorSequence)
    finally:
        eng.set_option('chain_resident', 1)
    eng.set_option('chain_resident_lag', lag)
    try:
        runs = []
        for _ in range(3):
            A = cases.build(bl, c); A.fit(silent=True)
            assert A.lastTiming['fwd_kernel_variant'] == 6 and A.lastTiming['bwd_kernel_variant'] == 6
            runs.append((A.logEvidence, np.array(A.posteriorSequence), np.array(A.localEvidence), np.array(A.logEvidenceList)))
    finally:
        eng.set_option('chain_resident_lag', 4)
    for logE, post, loc, lel in runs:
        assert abs(logE - B.logEvidence) <= 1e-11 * abs(B.logEvidence)
        np.testing.assert_allclose(lel, np.array(B.logEvidenceList), rtol=1e-11)
        np.testing.assert_allclose(post, base, rtol=1e-9, atol=1e-14)
        assert logE == runs[0][0] and np.array_equal(post, runs[0][1]) and np.array_equal(loc, runs[0][2], equal_nan=True)


def test_chain_resident_kernel_not_taken_outside_its_envelope():
    """A walk wider than 80 grid steps, a filter on the second parameter of a grid wider than 512 columns (inside 512 x 512 the
    transposing kernels take it: round 5), a grid of fewer than 32 rows, more than 64 strips: the
    launch-per-step kernels run (and the results are the oracle's: covered by the golden and fuzz tests)."""
    for c in (_hyper(128, 32, 62, 4, ('cint', 0.1, 3.0, 3)),
              dict(study='HyperStudy', data=('series', 63, 4), om=_g2(64, 528), tm=('GRW', 'sigma', ('cint', 0.1, 0.3, 3), 'std', None)),
              _hyper(24, 32, 64, 4, ('cint', 0.1, 0.5, 3)),               # fewer than 32 rows
              _hyper(128, 1040, 66, 3, ('cint', 0.1, 0.5, 2))):          # 65 strips: more than one granule per lane
        S = cases.build(bl, c); S.fit(**cases.fit_kwargs(c))
        assert S.lastTiming['fwd_kernel_variant'] != 6
        with np.errstate(all='ignore'):
            want = oa.run(c)
        assert abs(S.logEvidence - want['logEvidence']) <= 1e-9 * abs(want['logEvidence'])


def test_average_posterior_folded_by_the_separate_pass_over_three_batches():
    """fuse_accumulate = 0, max_batch = 32: the study is cut into three or more batches, each stored and folded by the separate fold
    pass.  Same results as the default (one batch, folded inside the backward kernel) up to the order of the sums."""
    eng = bl.get_engine()
    c = _hyper(128, 64, 71, 8, ('cint', 0, 0.9, 80))
    A = cases.build(bl, c); A.fit(silent=True)
    eng.set_option('fuse_accumulate', 0)
    eng.set_option('max_batch', 32)
    try:
        B = cases.build(bl, c); B.fit(silent=True)
        assert B.lastTiming['batches'] >= 3, B.lastTiming
    finally:
        eng.set_option('fuse_accumulate', 1)
        eng.set_option('max_batch', 1024)
    assert abs(A.logEvidence - B.logEvidence) <= 1e-12 * abs(A.logEvidence)
    np.testing.assert_allclose(np.array(B.posteriorSequence), np.array(A.posteriorSequence), rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(B.posteriorMeanValues, A.posteriorMeanValues, rtol=1e-11)
    np.testing.assert_allclose(B.hyperParameterDistribution, A.hyperParameterDistribution, rtol=1e-11)


def test_partial_accumulators_carried_from_batch_to_batch():
    """Round 6: the partial accumulators of the chain-resident fold are carried through the batches of a call (their weights share the first
    batch's reference) and go into the average posterior ONCE.  Same results as one fold per batch (carry_partials = 0) up to the order of
    the sums; a batch whose check fails after its backward pass has added to carried slots (forced here) makes the call repeat the batches
    the slots held on the launch-per-step kernels -- same results again."""
    eng = bl.get_engine()
    c = _hyper(128, 64, 93, 8, ('cint', 0, 0.9, 40))
    eng.set_option('max_batch', 16)
    try:
        A = cases.build(bl, c); A.fit(silent=True)
        assert A.lastTiming['batches'] == 3 and A.lastTiming['accumulate_launches'] == 1 and A.lastTiming['bwd_kernel_variant'] == 6, A.lastTiming
        eng.set_option('carry_partials', 0)
        try:
            B = cases.build(bl, c); B.fit(silent=True)
            assert B.lastTiming['accumulate_launches'] == 3, B.lastTiming
        finally:
            eng.set_option('carry_partials', 1)
        runs = [B]
        for bad in (1, 2):
            eng.set_option('fold_force_fail_batch', bad)
            try:
                C = cases.build(bl, c); C.fit(silent=True)
                assert C.lastTiming['resident_fallbacks'] >= 1 and C.lastTiming['resident_fallback_reason'] == 3, C.lastTiming      # BLHIP_FALLBACK_PREDICTION
            finally:
                eng.set_option('fold_force_fail_batch', -1)
            runs.append(C)
    finally:
        eng.set_option('max_batch', 1024)
    for R in runs:
        assert abs(A.logEvidence - R.logEvidence) <= 1e-12 * abs(A.logEvidence)
        np.testing.assert_allclose(np.array(R.posteriorSequence), np.array(A.posteriorSequence), rtol=1e-10, atol=1e-300)
        np.testing.assert_allclose(R.posteriorMeanValues, A.posteriorMeanValues, rtol=1e-10)
        np.testing.assert_allclose(R.hyperParameterDistribution, A.hyperParameterDistribution, rtol=1e-11)
    with np.errstate(all='ignore'):
        want = oa.run(c)
    compare.check(dict(logEvidence=A.logEvidence, localEvidence=A.localEvidence, posteriorSequence=A.posteriorSequence, posteriorMeanValues=A.posteriorMeanValues),
                  dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'], posteriorSequence=want['posteriorSequence'],
                       posteriorMeanValues=want['posteriorMeanValues']), compare.GPU_TOL)


def test_forward_sums_beside_the_backward_pass_change_nothing():
    """late_sums (round 6): batches of >= 64 chains on the launch-per-step / 1-D chain kernels queue their backward pass without waiting for the
    forward pass's sums, which travel to the host on a copy stream beside it.  Same numbers bit for bit as with the wait (late_sums = 0),
    on a 1-D hyper-study (chain kernel) and a 2-D one outside the resident envelopes (launch-per-step kernels); and the oracle's."""
    eng = bl.get_engine()
    for c in (dict(study='HyperStudy', data=cases.COAL, timestamps=cases.COAL_T, om=('Poisson', [('rate', ('oint', 0, 6, 200))], 'default'),
                   tm=('GRW', 'sigma', ('cint', 0, 1.0, 96), 'rate', None)),
              _hyper(24, 32, 91, 7, ('cint', 0.1, 0.5, 70))):                 # fewer than 32 rows: no resident path
        A = cases.build(bl, c); A.fit(silent=True)
        eng.set_option('late_sums', 0)
        try:
            B = cases.build(bl, c); B.fit(silent=True)
        finally:
            eng.set_option('late_sums', 1)
        assert A.logEvidence == B.logEvidence
        assert np.array_equal(np.array(A.logEvidenceList), np.array(B.logEvidenceList))
        assert np.array_equal(np.array(A.localEvidenceList), np.array(B.localEvidenceList), equal_nan=True)
        assert np.array_equal(np.array(A.posteriorSequence), np.array(B.posteriorSequence))
        with np.errstate(all='ignore'):
            want = oa.run(c)
        assert abs(A.logEvidence - want['logEvidence']) <= 1e-9 * abs(want['logEvidence'])


def test_fused_fold_matches_the_separate_fold():
    """fuse_accumulate = 0: the backward chain kernel stores the posteriors and the average posterior is folded by a separate pass."""
    eng = bl.get_engine()
    c = _hyper(256, 64, 72, 9, ('cint', 0, 0.6, 21))
    A = cases.build(bl, c); A.fit(silent=True)
    assert A.lastTiming['bwd_kernel_variant'] == 6
    eng.set_option('fuse_accumulate', 0)
    try:
        B = cases.build(bl, c); B.fit(silent=True)
        assert B.lastTiming['bwd_kernel_variant'] == 6
    finally:
        eng.set_option('fuse_accumulate', 1)
    assert A.logEvidence == B.logEvidence                      # (the forward pass is the same kernel)
    np.testing.assert_allclose(np.array(A.posteriorSequence), np.array(B.posteriorSequence), rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(A.posteriorMeanValues, B.posteriorMeanValues, rtol=1e-11)
    np.testing.assert_allclose(A.localEvidence, B.localEvidence, rtol=1e-11, equal_nan=True)


def test_change_point_chains_share_their_common_prefix():
    """Change-point batches: every chain repeats the steps before its FIRST restart.
    share_prefix (default on): those states are stored by ONE chain of the batch and read from there by the folding backward pass of the
    others -- same numbers bit for bit as every chain storing its own copy (share_prefix = 0).
    skip_prefix (default on): they are not computed twice either -- a chain's forward pass begins at its first restart, the sums of its
    earlier steps are the providing chain's.  The lagged scales of such a chain start at its restart, so the results agree with the
    full-length pass to rounding (asserted at 1e-12), not bit for bit; also for evidence-only fits."""
    eng = bl.get_engine()
    study_cases = [cases.CASES['c5_small'], EXTRA['x_cp_all'], RAGGED['pad_cp_150x40'],
                   dict(study='ChangepointStudy', data=('series_jump', 95, 40, 18, 1.5), om=_g2(128, 48), tm=('ChangePoint', 'tc', ('arange', 1, 39, 2), None)),
                   # two change points per chain: chains restart at different first steps, some share only a short prefix
                   dict(study='ChangepointStudy', data=('series_jump', 96, 18, 9, 2.0), om=_g2(128, 16),
                        tm=('Combined', [('ChangePoint', 't1', ('arange', 2, 16, 4), None), ('ChangePoint', 't2', ('arange', 3, 17, 5), None)]))]

    def fit_with(c, **opts):
        for k, v in opts.items():
            eng.set_option(k, v)
        try:
            S = cases.build(bl, c); S.fit(**cases.fit_kwargs(c))
        finally:
            for k in opts:
                eng.set_option(k, 1)
        assert S.lastTiming['fwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
        return S

    tight = dict(rtol=1e-12, atol=1e-300)
    for c in study_cases:
        A = fit_with(c)
        B = fit_with(c, skip_prefix=0)
        C = fit_with(c, skip_prefix=0, share_prefix=0)
        assert A.lastTiming['bwd_kernel_variant'] == 6
        assert B.logEvidence == C.logEvidence
        assert np.array_equal(np.array(B.posteriorSequence), np.array(C.posteriorSequence), equal_nan=True)
        assert np.array_equal(np.array(B.posteriorMeanValues), np.array(C.posteriorMeanValues), equal_nan=True)
        assert B.lastTiming['bwd_hbm_bytes'] <= C.lastTiming['bwd_hbm_bytes'] and B.lastTiming['fwd_hbm_bytes'] <= C.lastTiming['fwd_hbm_bytes']
        assert A.lastTiming['fwd_flops'] < B.lastTiming['fwd_flops'], (A.lastTiming, B.lastTiming)       # chain-steps really left out
        np.testing.assert_allclose(A.logEvidence, B.logEvidence, rtol=1e-13)
        np.testing.assert_allclose(np.array(A.localEvidence), np.array(B.localEvidence), equal_nan=True, **tight)
        np.testing.assert_allclose(np.array(A.posteriorSequence), np.array(B.posteriorSequence), equal_nan=True, **tight)
        np.testing.assert_allclose(np.array(A.hyperParameterDistribution), np.array(B.hyperParameterDistribution), rtol=1e-11, atol=1e-300)
        with np.errstate(all='ignore'):
            want = oa.run(c)
        compare.check(dict(logEvidence=A.logEvidence, localEvidence=A.localEvidence, posteriorSequence=A.posteriorSequence,
                           posteriorMeanValues=A.posteriorMeanValues),
                      dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'], posteriorSequence=want['posteriorSequence'],
                           posteriorMeanValues=want['posteriorMeanValues']), compare.GPU_TOL)
        # evidence-only fits skip the prefix too (nothing is stored: only the sums are shared)
        ce = dict(c, fit=dict(evidenceOnly=True))
        Ae = fit_with(ce)
        Be = fit_with(ce, skip_prefix=0)
        assert Ae.lastTiming['fwd_flops'] < Be.lastTiming['fwd_flops'], (Ae.lastTiming, Be.lastTiming)
        np.testing.assert_allclose(Ae.logEvidence, Be.logEvidence, rtol=1e-13)
        np.testing.assert_allclose(Ae.logEvidence, want['logEvidence'], rtol=1e-9)
        np.testing.assert_allclose(np.array(Ae.hyperParameterDistribution), np.array(Be.hyperParameterDistribution), rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(np.array(Ae.localEvidence), np.array(Be.localEvidence), equal_nan=True, **tight)


RAGGED = {
    # rows not 128 / 256 / 512 and / or columns not a multiple of 16: the chain-resident kernels on the padded geometry
    'pad_200x200_full': _hyper(200, 200, 81, 6, ('cint', 0, 0.7, 9)),
    'pad_100x37_full': _hyper(100, 37, 82, 9, ('cint', 0.02, 0.8, 21)),                 # odd number of columns, 3 strips, odd chain count
    'pad_48x17_evidence': _hyper(48, 17, 83, 7, ('cint', 0, 0.5, 4), evidenceOnly=True),
    'pad_511x33_full': _hyper(511, 33, 84, 5, ('cint', 0, 0.25, 5)),
    'pad_300x1000_evidence': _hyper(300, 1000, 85, 4, ('cint', 0.05, 0.5, 3), evidenceOnly=True),
    'pad_130x16_nan': _hyper(130, 16, 86, 10, ('cint', 0, 0.6, 8), kind='series_nan', extra=[2, 3]),
    'pad_300x64_full': _hyper(300, 64, 89, 7, ('cint', 0, 0.5, 10)),                     # the 384-row geometry (3 product tiles per wave)
    'aligned_384x32_full': _hyper(384, 32, 90, 6, ('cint', 0, 0.4, 6)),
    # random walk + change point in one model (restart inside a filtering chain): both list orders, hyper- and change-point studies
    'mixed_cp_grw_128x32': dict(study='ChangepointStudy', data=('series_jump', 91, 14, 7, 2.0), om=_g2(128, 32, -4, 6, 3),
                                tm=('Combined', [('ChangePoint', 'tChange', ('arange', 2, 12, 3), None), ('GRW', 'sigma', ('cint', 0.05, 0.45, 3), 'mean', None)])),
    'mixed_grw_cp_256x16': dict(study='ChangepointStudy', data=('series_jump', 92, 12, 5, -1.5), om=_g2(256, 16, -4, 6, 3),
                                tm=('Combined', [('GRW', 'sigma', 0.2, 'mean', None), ('ChangePoint', 'tChange', ('arange', 1, 11, 2), None)])),
    'mixed_hyper_80x80': dict(study='HyperStudy', data=('series_jump', 93, 16, 8, 2.0), om=_g2(80, 80, -5, 7, 3),
                              tm=('Combined', [('GRW', 'sigma', ('cint', 0.1, 0.9, 4), 'mean', None), ('ChangePoint', 'tc', ('arange', 4, 14, 5), None)])),
    'mixed_cp_grw_40x40_evidence': dict(study='ChangepointStudy', data=('series_jump', 94, 20, 9, 2.0), om=_g2(40, 40, -4, 6, 3),
                                        tm=('Combined', [('ChangePoint', 'tChange', ('arange', 2, 18, 3), None), ('GRW', 'sigma', ('cint', 0.05, 0.25, 3), 'mean', None)]),
                                        fit=dict(evidenceOnly=True)),
    'pad_cp_150x40': dict(study='ChangepointStudy', data=('series_jump', 87, 12, 6, 1.5), om=_g2(150, 40), tm=('ChangePoint', 'tc', 'all', None)),
    'pad_cp_60x70_evidence': dict(study='ChangepointStudy', data=('series_jump', 88, 9, 4, -1.0), om=_g2(60, 70), tm=('ChangePoint', 'tc', 'all', None),
                                  fit=dict(evidenceOnly=True)),
}


def _om2(name, p0, p1):
    return (name, [p0, p1], 'default')


CHAINTAB = {
    # observation models other than the Gaussian on the chain-resident kernels (blc::chain_kernel TAB: the likelihood of every step out of
    # the (T, G) table the launch-per-step kernels use too): Laplace / AR1 / ScaledAR1 hyper-studies over the width of a walk on the first
    # parameter -- full fits (single-chain fused fold), evidence-only, forward-only --, a change-point study (no stencil), a plain Study
    'ctab_laplace_128x32_full': dict(study='HyperStudy', data=('series', 101, 9), om=_om2('Laplace', ('mu', ('cint', -5, 5, 128)), ('b', ('oint', 0, 3, 32))),
                                     tm=('GRW', 'sigma', ('cint', 0, 0.7, 7), 'mu', None)),
    'ctab_ar1_256x48_evidence': dict(study='HyperStudy', data=('series', 102, 12), om=_om2('AR1', ('rho', ('oint', -1, 1, 256)), ('sigma', ('oint', 0, 3, 48))),
                                     tm=('GRW', 's', ('cint', 0.005, 0.07, 5), 'rho', None), fit=dict(evidenceOnly=True)),
    'ctab_scaled_ar1_512x16_full': dict(study='HyperStudy', data=('series', 103, 8), om=_om2('ScaledAR1', ('rho', ('oint', -1, 1, 512)), ('sigma', ('oint', 0, 3, 16))),
                                        tm=('GRW', 's', ('cint', 0.0, 0.035, 4), 'rho', None)),
    'ctab_laplace_384x32_forward_only': dict(study='HyperStudy', data=('series', 104, 7), om=_om2('Laplace', ('mu', ('cint', -5, 5, 384)), ('b', ('oint', 0, 3, 32))),
                                             tm=('GRW', 'sigma', ('cint', 0.05, 0.25, 3), 'mu', None), fit=dict(forwardOnly=True)),
    'ctab_laplace_changepoints_128x48': dict(study='ChangepointStudy', data=('series_jump', 105, 14, 7, 1.5),
                                             om=_om2('Laplace', ('mu', ('cint', -5, 5, 128)), ('b', ('oint', 0, 3, 48))), tm=('ChangePoint', 'tc', 'all', None)),
    # ... on padded grids: hyper-study (posteriors stored on the padded geometry, folded by accumulate_pad_kernel), evidence-only, a plain Study
    # (de-padding copy), a change-point study
    'ctab_pad_laplace_200x50_full': dict(study='HyperStudy', data=('series', 107, 8), om=_om2('Laplace', ('mu', ('cint', -5, 5, 200)), ('b', ('oint', 0, 3, 50))),
                                         tm=('GRW', 'sigma', ('cint', 0, 0.45, 6), 'mu', None)),
    'ctab_pad_ar1_100x37_evidence': dict(study='HyperStudy', data=('series', 108, 10), om=_om2('AR1', ('rho', ('oint', -1, 1, 100)), ('sigma', ('oint', 0, 3, 37))),
                                         tm=('GRW', 's', ('cint', 0.01, 0.18, 4), 'rho', None), fit=dict(evidenceOnly=True)),
    'ctab_pad_scaled_ar1_study_200x200': dict(study='Study', data=('series', 109, 9), om=_om2('ScaledAR1', ('rho', ('oint', -1, 1, 200)), ('sigma', ('oint', 0, 3, 200))),
                                              tm=('GRW', 's', 0.08, 'rho', None)),
    'ctab_pad_laplace_changepoints_150x40': dict(study='ChangepointStudy', data=('series_jump', 110, 12, 6, 1.5),
                                                 om=_om2('Laplace', ('mu', ('cint', -5, 5, 150)), ('b', ('oint', 0, 3, 40))), tm=('ChangePoint', 'tc', 'all', None)),
    'ctab_laplace_study_256x64': dict(study='Study', data=('series', 106, 10), om=_om2('Laplace', ('mu', ('cint', -5, 5, 256)), ('b', ('oint', 0, 3, 64))),
                                      tm=('GRW', 'sigma', 0.3, 'mu', None)),
}


@pytest.mark.parametrize('case', list(CHAINTAB))
def test_chain_resident_kernels_with_a_tabulated_likelihood_match_oracle(case):
    c = CHAINTAB[case]
    S = cases.build(bl, c)
    kw = cases.fit_kwargs(c)
    S.fit(**kw)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming
    if not kw.get('evidenceOnly') and not kw.get('forwardOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    # ... and the launch-per-step kernels (option off) agree
    eng = bl.get_engine()
    eng.set_option('chain_table', 0)
    try:
        R = cases.build(bl, c); R.fit(**kw)
    finally:
        eng.set_option('chain_table', 1)
    assert R.lastTiming['fwd_kernel_variant'] != 6
    assert abs(S.logEvidence - R.logEvidence) <= 1e-10 * abs(R.logEvidence)


RESTAB = {
    # observation models other than the Gaussian on the time-resident kernel (blr::Res TAB: likelihood out of the (T, G) table): walks on
    # both parameters with radius <= 8 -- ScaledAR1 (the reference's showcase model) on a padded 200 x 200 grid, AR1 / Laplace on whole
    # tiles, evidence-only and forward-only fits, a walk on one parameter only
    'rtab_scaled_ar1_200x200_full': dict(study='Study', data=('series', 111, 12), om=_om2('ScaledAR1', ('rho', ('oint', -1, 1, 200)), ('sigma', ('oint', 0, 3, 200))),
                                         tm=('Combined', [('GRW', 's1', 0.018, 'rho', None), ('GRW', 's2', 0.025, 'sigma', None)])),
    'rtab_ar1_128x128_full': dict(study='Study', data=('series', 112, 10), om=_om2('AR1', ('rho', ('oint', -1, 1, 128)), ('sigma', ('oint', 0, 3, 128))),
                                  tm=('Combined', [('GRW', 's1', 0.03, 'rho', None), ('GRW', 's2', 0.04, 'sigma', None)])),
    'rtab_laplace_64x96_evidence': dict(study='Study', data=('series', 113, 14), om=_om2('Laplace', ('mu', ('cint', -5, 5, 64)), ('b', ('oint', 0, 3, 96))),
                                        tm=('Combined', [('GRW', 's1', 0.3, 'mu', None), ('GRW', 's2', 0.05, 'b', None)]), fit=dict(evidenceOnly=True)),
    'rtab_laplace_150x80_forward_only': dict(study='Study', data=('series', 114, 9), om=_om2('Laplace', ('mu', ('cint', -5, 5, 150)), ('b', ('oint', 0, 3, 80))),
                                             tm=('Combined', [('GRW', 's1', 0.12, 'mu', None), ('GRW', 's2', 0.07, 'b', None)]), fit=dict(forwardOnly=True)),
    'rtab_laplace_96x96_nan': dict(study='Study', data=('series_nan', 115, 11, [4, 5]), om=_om2('Laplace', ('mu', ('cint', -5, 5, 96)), ('b', ('oint', 0, 3, 96))),
                                   tm=('Combined', [('GRW', 's1', 0.2, 'mu', None), ('GRW', 's2', 0.06, 'b', None)])),
}


@pytest.mark.parametrize('case', list(RESTAB))
def test_time_resident_kernel_with_a_tabulated_likelihood_matches_oracle(case):
    c = RESTAB[case]
    S = cases.build(bl, c)
    kw = cases.fit_kwargs(c)
    S.fit(**kw)
    assert S.lastTiming['fwd_kernel_variant'] == 5, S.lastTiming
    if not kw.get('evidenceOnly') and not kw.get('forwardOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 5 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    eng = bl.get_engine()
    eng.set_option('resident_table', 0)
    try:
        R = cases.build(bl, c); R.fit(**kw)
    finally:
        eng.set_option('resident_table', 1)
    assert R.lastTiming['fwd_kernel_variant'] != 5
    assert abs(S.logEvidence - R.logEvidence) <= 1e-10 * abs(R.logEvidence)


DEPAD = {
    # ordinary fits (one chain, the posterior sequence is the result) and forward-only hyper-studies on grids the chain-resident kernels
    # pad: the kernels work on a scratch sequence on the padded geometry, depad_kernel writes the grid's rows into the sequence handed out
    'depad_study_200x200_full': dict(study='Study', data=('series', 95, 12), om=_g2(200, 200), tm=('GRW', 'sigma', 0.25, 'mean', None)),
    'depad_study_100x37_forward_only': dict(study='Study', data=('series', 96, 9), om=_g2(100, 37), tm=('GRW', 'sigma', 0.6, 'mean', None),
                                            fit=dict(forwardOnly=True)),
    'depad_study_500x30_nan': dict(study='Study', data=('series_nan', 97, 10, [3, 4]), om=_g2(500, 30), tm=('GRW', 'sigma', 0.1, 'mean', None)),
    'depad_hyper_96x32_forward_only': _hyper(96, 32, 64, 4, ('cint', 0.1, 0.5, 3), forwardOnly=True),
    'depad_hyper_1000x20_forward_only': _hyper(1000, 20, 98, 4, ('cint', 0.05, 0.3, 3), forwardOnly=True),      # the 1024-row geometry: forward passes only
    'depad_study_cp_150x40': dict(study='Study', data=('series_jump', 99, 12, 6, 1.5), om=_g2(150, 40), tm=('ChangePoint', 'tc', 6, None)),
}


@pytest.mark.parametrize('case', list(DEPAD))
def test_padded_chain_resident_fits_hand_their_posteriors_out(case):
    c = DEPAD[case]
    S = cases.build(bl, c)
    kw = cases.fit_kwargs(c)
    S.fit(**kw)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming
    if not kw.get('forwardOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    assert 'posteriorSequence' in gold
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    # ... and the same fit with the option off (launch-per-step kernels) hands out the same sequence
    eng = bl.get_engine()
    eng.set_option('chain_depad', 0)
    try:
        R = cases.build(bl, c); R.fit(**kw)
    finally:
        eng.set_option('chain_depad', 1)
    assert R.lastTiming['fwd_kernel_variant'] != 6
    np.testing.assert_allclose(np.asarray(S.posteriorSequence), np.asarray(R.posteriorSequence), rtol=1e-9, atol=1e-14)


@pytest.mark.parametrize('opts', [dict(fold2=0), dict(fuse_accumulate=0), dict(fold2_cp=0)])
def test_padded_grids_through_the_storing_backward_kernel(opts):
    """Padded grids without the two-chain fold kernel: the backward chain kernel stores the posteriors on the padded geometry and the
    separate fold (accumulate_pad_kernel) reads them from there."""
    eng = bl.get_engine()
    for case in ('pad_100x37_full', 'pad_cp_150x40', 'pad_300x64_full'):
        c = RAGGED[case]
        for k, v in opts.items():
            eng.set_option(k, v)
        try:
            S = cases.build(bl, c); S.fit(**cases.fit_kwargs(c))
        finally:
            for k in opts:
                eng.set_option(k, 1)
        assert S.lastTiming['fwd_kernel_variant'] == 6 and S.lastTiming['bwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0
        with np.errstate(all='ignore'):
            want = oa.run(c)
        got = result_of(S, c)
        gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
        for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
            if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
                gold[k] = np.asarray(want[k])
        compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('case', list(RAGGED))
def test_chain_resident_kernels_on_padded_grids_match_oracle(case):
    c = RAGGED[case]
    S = cases.build(bl, c)
    kw = cases.fit_kwargs(c)
    S.fit(**kw)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming
    if not kw.get('evidenceOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    with np.errstate(all='ignore'):
        want = oa.run(c)
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_CHAIN_FUZZ_SEEDS', 36))))
def test_seeded_random_chain_resident_studies_on_padded_grids_match_oracle(seed):
    c = random_cases.random_chain_resident_case(seed, ragged=True)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming          # the chain-resident path really ran
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    if 'logEvidenceList' in want and not np.all(np.isfinite(np.asarray(want['logEvidenceList'], dtype=float))):
        got['localEvidence'] = gold['localEvidence']
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_CHAIN_TALL_FUZZ_SEEDS', 20))))
def test_seeded_random_chain_resident_studies_on_the_1024_row_geometry_match_oracle(seed):
    c = random_cases.random_chain_resident_case(seed, tall=True)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming          # the chain-resident path really ran
    if not cases.fit_kwargs(c).get('evidenceOnly') and not cases.fit_kwargs(c).get('forwardOnly'):
        assert S.lastTiming['bwd_kernel_variant'] == 6 and S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    if 'logEvidenceList' in want and not np.all(np.isfinite(np.asarray(want['logEvidenceList'], dtype=float))):
        got['localEvidence'] = gold['localEvidence']
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_CHAIN_FUZZ_SEEDS', 36))))
def test_seeded_random_walk_plus_change_point_studies_match_oracle(seed):
    c = random_cases.random_chain_mixed_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming          # the chain-resident path really ran
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    if 'logEvidenceList' in want and not np.all(np.isfinite(np.asarray(want['logEvidenceList'], dtype=float))):
        got['localEvidence'] = gold['localEvidence']
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


@pytest.mark.parametrize('seed', range(int(os.environ.get('BLHIP_CHAIN_FUZZ_SEEDS', 36))))
def test_seeded_random_chain_resident_studies_match_oracle(seed):
    c = random_cases.random_chain_resident_case(seed)
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['fwd_kernel_variant'] == 6, S.lastTiming          # the chain-resident path really ran
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
            gold[k] = np.asarray(want[k])
    if 'logEvidenceList' in want and not np.all(np.isfinite(np.asarray(want['logEvidenceList'], dtype=float))):
        got['localEvidence'] = gold['localEvidence']
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))


# ---- grids with 3 and 4 parameters (blhip_nd.hpp): the reference's plug-in models (bl.om.SciPy) on an N-D meshgrid ------------------

def _t3(n_df=5, n_loc=18, n_scale=14):
    return ('SciPy:t', [('df', ('cint', 2.0, 9.0, n_df)), ('loc', ('cint', -3.0, 3.0, n_loc)), ('scale', ('oint', 0.2, 2.5, n_scale))], 'default')


ND_CASES = {
    'nd3_static': dict(study='Study', data=('series', 81, 9), om=_t3(), tm=('Static',)),
    # random walks on the middle and the last parameter (in this list order), then on the first one
    'nd3_grw_loc_scale': dict(study='Study', data=('series', 82, 8), om=_t3(),
                              tm=('Combined', [('GRW', 's_loc', 0.6, 'loc', None), ('GRW', 's_scale', 0.25, 'scale', None)])),
    'nd3_grw_all_axes': dict(study='Study', data=('series', 83, 7), om=_t3(6, 12, 10),
                             tm=('Combined', [('GRW', 's_df', 2.5, 'df', None), ('GRW', 's_scale', 0.3, 'scale', None),
                                              ('GRW', 's_loc', 0.5, 'loc', None)])),
    'nd3_wide_walk': dict(study='Study', data=('series', 84, 5), om=_t3(4, 10, 8), tm=('GRW', 's_loc', 9.0, 'loc', None)),   # radius > axis length
    'nd3_forward_only': dict(study='Study', data=('series', 85, 8), om=_t3(), tm=('GRW', 's_loc', 0.4, 'loc', None), fit=dict(forwardOnly=True)),
    'nd3_evidence_only': dict(study='Study', data=('series', 86, 8), om=_t3(), tm=('GRW', 's_loc', 0.4, 'loc', None), fit=dict(evidenceOnly=True)),
    'nd3_missing_data': dict(study='Study', data=('series_nan', 87, 9, [2, 3, 7]), om=_t3(), tm=('GRW', 's_scale', 0.2, 'scale', None)),
    'nd3_prior_function': dict(study='Study', data=('series', 88, 6), om=(_t3()[0], _t3()[1], 'inv_s_3d'), tm=('GRW', 's_loc', 0.4, 'loc', None)),
    'nd3_hyper': dict(study='HyperStudy', data=('series', 89, 7), om=_t3(4, 14, 10), tm=('GRW', 's_loc', ('cint', 0, 1.2, 5), 'loc', None)),
    'nd3_hyper_two': dict(study='HyperStudy', data=('series', 90, 6), om=_t3(4, 12, 10),
                          tm=('Combined', [('GRW', 's_loc', ('cint', 0.1, 0.9, 3), 'loc', None),
                                           ('GRW', 's_scale', ('cint', 0.0, 0.3, 2), 'scale', None)])),
    'nd3_changepoints': dict(study='ChangepointStudy', data=('series_jump', 91, 10, 5, 1.5), om=_t3(4, 14, 10),
                             tm=('ChangePoint', 'tc', 'all', None)),
    'nd3_changepoint_then_walk': dict(study='ChangepointStudy', data=('series_jump', 92, 9, 4, -1.5), om=_t3(4, 12, 8),
                                      tm=('Combined', [('ChangePoint', 'tc', ('arange', 1, 8, 2), None), ('GRW', 's_loc', 0.4, 'loc', None)])),
    'nd4_johnsonsu': dict(study='Study', data=('series', 93, 6),
                          om=('SciPy:johnsonsu', [('a', ('cint', -1.0, 1.0, 5)), ('b', ('cint', 0.8, 2.5, 4)), ('loc', ('cint', -2.0, 2.0, 11)),
                                                  ('scale', ('oint', 0.3, 2.0, 9))], 'default'),
                          tm=('Combined', [('GRW', 's_loc', 0.5, 'loc', None), ('GRW', 's_b', 0.4, 'b', None)])),
}


@pytest.mark.parametrize('case', list(ND_CASES))
def test_three_and_four_parameter_grids_match_oracle(case):
    pytest.importorskip('scipy.stats')
    c = ND_CASES[case]
    S = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(c))
        want = oa.run(c)
    assert S.lastTiming['fwd_kernel_variant'] == 7, S.lastTiming
    got = result_of(S, c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    if 'posteriorSequence' in gold:
        # marginal distributions of every parameter (the device-side reductions are 2-D: reduced on the host here)
        post = np.asarray(want['posteriorSequence'])
        for k, name in enumerate(S.observationModel.parameterNames):
            axes = tuple(a + 1 for a in range(post.ndim - 1) if a != k)
            np.testing.assert_allclose(S.getParameterDistributions(name, density=False)[1], post.sum(axis=axes), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('case', ['nd3_reference', 'nd4_reference'])
def test_three_and_four_parameter_grids_against_the_reference_goldens(case):
    """tests/golden/nd3_reference.npz / nd4_reference.npz: bl.om.SciPy(scipy.stats.t, df, loc, scale) and
    bl.om.SciPy(scipy.stats.johnsonsu, a, b, loc, scale) with two random walks each, fitted by the reference itself in the build
    container (tests/golden/gen_golden.py)."""
    pytest.importorskip('scipy.stats')
    gold = oa.load_golden(case)
    S = cases.build(bl, cases.CASES[case])
    S.fit(silent=True)
    assert S.lastTiming['fwd_kernel_variant'] == 7
    compare.check(result_of(S, case), gold, compare.GPU_TOL)


def test_resident_paths_fall_back_when_a_block_gives_up():
    """A resident launch whose blocks cannot wait for each other (not all co-resident) gives up through the abort word; the batch is
    repeated with the launch-per-step kernels and the context stops using the resident paths.  (The give-up itself needs blocks that
    are not co-resident; the test makes the host read the abort word as set.)"""
    eng = bl.get_engine()
    c = _hyper(128, 64, 73, 9, ('cint', 0, 0.8, 11))
    with np.errstate(all='ignore'):
        want = oa.run(c)
    eng.set_option('resident_force_abort', 1)
    try:
        S = cases.build(bl, c); S.fit(silent=True)
        assert S.lastTiming['fwd_kernel_variant'] != 6 and S.lastTiming['bwd_kernel_variant'] != 6, S.lastTiming
        got = result_of(S, c)
        gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'], posteriorSequence=np.asarray(want['posteriorSequence']),
                    posteriorMeanValues=np.asarray(want['posteriorMeanValues']), logEvidenceList=np.asarray(want['logEvidenceList']))
        compare.check(got, gold, compare.GPU_TOL)
        eng.set_option('resident_force_abort', 0)
        S2 = cases.build(bl, c); S2.fit(silent=True)           # the context remembers
        assert S2.lastTiming['fwd_kernel_variant'] != 6
        R = cases.build(bl, RESIDENT['res_64x96_full']); R.fit(silent=True)      # ... for the single-chain path too
        assert R.lastTiming['fwd_kernel_variant'] != 5
    finally:
        eng.set_option('resident_force_abort', 0)
        eng.set_option('resident_ok', 1)
    S3 = cases.build(bl, c); S3.fit(silent=True)
    assert S3.lastTiming['fwd_kernel_variant'] == 6
    assert abs(S3.logEvidence - want['logEvidence']) <= 1e-9 * abs(want['logEvidence'])


@pytest.mark.parametrize('seed', [1, 2, 3, 6, 7, 13, 16])
def test_both_axes_batches_fall_back_too(seed):
    """The give-up of a batch of the transposing chain-resident kernels (blhip_chainax.hpp): its sequences live in the two alternating
    strip-major layouts of a square geometry, private to the fit or de-layouted afterwards -- the repeat through the launch-per-step
    kernels must find buffers of the right shape and give the oracle's results (hyper-studies that fold, ragged grids, change points,
    plain fits that hand their posteriors out)."""
    eng = bl.get_engine()
    c = random_cases.random_both_axes_square_case(seed)
    with np.errstate(all='ignore'):
        want = oa.run(c)
    eng.set_option('resident_force_abort', 1)
    try:
        S = cases.build(bl, c)
        with np.errstate(all='ignore'):
            S.fit(**cases.fit_kwargs(c))
        assert S.lastTiming['fwd_kernel_variant'] not in (5, 6) and S.lastTiming['resident_fallbacks'] >= 1, S.lastTiming
        got = result_of(S, c)
        gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
        for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
            if k in want and want[k] is not None and k in got and (k != 'posteriorMeanValues' or len(want[k])):
                gold[k] = np.asarray(want[k])
        compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S, pin=False))
    finally:
        eng.set_option('resident_force_abort', 0)
        eng.set_option('resident_ok', 1)
    S3 = cases.build(bl, c)
    with np.errstate(all='ignore'):
        S3.fit(**cases.fit_kwargs(c))
    assert S3.lastTiming['fwd_kernel_variant'] in (5, 6), S3.lastTiming
    assert abs(S3.logEvidence - want['logEvidence']) <= 1e-9 * abs(want['logEvidence'])


@pytest.mark.parametrize('case', ['pad_100x37_full', 'mixed_cp_grw_128x32', 'pad_cp_150x40'])
def test_padded_and_restarting_batches_fall_back_too(case):
    """The same give-up on a padded grid (its sequence buffer is laid out for the padded geometry) and on a batch with restarts
    inside filtering chains: the repeat through the launch-per-step kernels gives the oracle's results; the context re-arms after
    `resident_retry_after` further fits (here: at once), reports the give-up in `resident_fallbacks`."""
    eng = bl.get_engine()
    c = RAGGED[case]
    with np.errstate(all='ignore'):
        want = oa.run(c)
    eng.set_option('resident_force_abort', 1)
    try:
        S = cases.build(bl, c); S.fit(**cases.fit_kwargs(c))
        assert S.lastTiming['fwd_kernel_variant'] != 6 and S.lastTiming['resident_fallbacks'] >= 1 and S.lastTiming['resident_armed'] == 0, S.lastTiming
        assert S.lastTiming['resident_fallback_reason'] == 4, S.lastTiming        # BLHIP_FALLBACK_FORCED (a real give-up reports 1)
        got = result_of(S, c)
        gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'], posteriorSequence=np.asarray(want['posteriorSequence']),
                    posteriorMeanValues=np.asarray(want['posteriorMeanValues']), logEvidenceList=np.asarray(want['logEvidenceList']))
        compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S, pin=False))
        eng.set_option('resident_force_abort', 0)
        eng.set_option('resident_retry_after', 2)
        for want_variant in (False, True, True):         # parked for one more fit, then tried again
            S2 = cases.build(bl, c); S2.fit(**cases.fit_kwargs(c))
            assert (S2.lastTiming['fwd_kernel_variant'] == 6) == want_variant, S2.lastTiming
    finally:
        eng.set_option('resident_force_abort', 0)
        eng.set_option('resident_ok', 1)


def test_prior_stays_resident_between_fits_of_a_study_and_is_replaced_when_it_changes():
    """blhip_problem.prior_token (ABI v8): the read-only prior array a study caches is uploaded once; a study with ANOTHER prior on the
    same grid, fitted on the same context in between, gets its own (no stale prior), and so does the first study afterwards."""
    def study(prior):
        S = bl.Study(silent=True)
        S.loadData(cases.series(77, 6), silent=True)
        S.set(bl.om.Gaussian('mean', bl.cint(-8, 8, 64), 'std', bl.oint(0, 4, 64), prior=prior),
              bl.tm.CombinedTransitionModel(bl.tm.GaussianRandomWalk('s1', 0.3, target='mean'), bl.tm.GaussianRandomWalk('s2', 0.1, target='std')), silent=True)
        return S
    A, Bs = study(lambda m, s: 1.0 / s ** 2), study(lambda m, s: np.exp(-0.5 * m ** 2) / s)
    A.fit(silent=True)
    first = (A.logEvidence, np.array(A.posteriorSequence))
    A.fit(silent=True)                         # (the token says: same content -- not uploaded again)
    assert A.logEvidence == first[0] and np.array_equal(np.array(A.posteriorSequence), first[1])
    Bs.fit(silent=True)
    assert abs(Bs.logEvidence - first[0]) > 1e-3 * abs(first[0])
    Bs.fit(silent=True); lb = Bs.logEvidence
    A.fit(silent=True)
    assert A.logEvidence == first[0] and np.array_equal(np.array(A.posteriorSequence), first[1])
    Bs.fit(silent=True)
    assert Bs.logEvidence == lb
    # an ndarray prior may be modified in place between fits: never cached (token 0)
    pr = np.ones((64, 64))
    C = study(pr)
    C.fit(silent=True); l0 = C.logEvidence
    pr[:, :32] = 3.0
    C.fit(silent=True)
    assert C.logEvidence != l0
    c = dict(study='Study', data=('series', 77, 6), om=('Gaussian', [('mean', ('cint', -8, 8, 64)), ('std', ('oint', 0, 4, 64))], ('array', pr.tolist())),
             tm=_grw2(0.3, 0.1))
    with np.errstate(all='ignore'):
        want = oa.run(c)
    assert abs(C.logEvidence - want['logEvidence']) <= 1e-9 * abs(want['logEvidence'])


def test_co_residency_probe_routes_a_busy_chip_to_the_launch_per_step_kernels(capfd):
    """blhip_timing.resident_probe (ABI v8): before a fit may take a resident path the library asks whether a one-block-per-CU grid with the
    resident kernels' footprint gets onto the chip at once.  Free chip: the resident kernel runs.  Busy chip (forced here): the paths are parked
    up front -- no launch, no time-out, no fall-back batch --, the launch-per-step kernels give the same results, and a later probe re-arms."""
    eng = bl.get_engine()
    c = RESIDENT['res_64x96_full']
    eng.set_option('resident_probe_interval_s', 0)          # (every fit asks)
    try:
        A = cases.build(bl, c); A.fit(silent=True)
        assert A.lastTiming['resident_probe'] == 1 and A.lastTiming['fwd_kernel_variant'] == 5, A.lastTiming
        assert A.lastTiming['xcd_order'] in (0, 1)
        eng.set_option('resident_probe_force_busy', 1)
        try:
            t0 = __import__('time').perf_counter()
            B = cases.build(bl, c); B.fit(silent=True)
            dt = __import__('time').perf_counter() - t0
        finally:
            eng.set_option('resident_probe_force_busy', 0)
        assert B.lastTiming['resident_probe'] == 2 and B.lastTiming['resident_armed'] == 0, B.lastTiming
        assert B.lastTiming['fwd_kernel_variant'] != 5 and B.lastTiming['resident_fallbacks'] == 0, B.lastTiming
        assert B.lastTiming['resident_fallback_reason'] == 5            # BLHIP_FALLBACK_BUSY
        assert dt < 0.2, dt                                               # (a launch that sat out its time-out: >= 0.25 s)
        assert 'not exclusively ours' in capfd.readouterr().err
        assert abs(A.logEvidence - B.logEvidence) <= 1e-11 * abs(A.logEvidence)
        np.testing.assert_allclose(np.asarray(B.posteriorSequence), np.asarray(A.posteriorSequence), rtol=1e-9, atol=1e-14)
        eng.set_option('resident_ok', 1)
        C = cases.build(bl, c); C.fit(silent=True)
        assert C.lastTiming['resident_probe'] == 1 and C.lastTiming['fwd_kernel_variant'] == 5, C.lastTiming
    finally:
        eng.set_option('resident_probe_interval_s', 1)
        eng.set_option('resident_ok', 1)


def test_fits_beside_another_contexts_kernels_do_not_sit_out_time_outs():
    """A second context keeps the GPU busy with streaming kernels from another host thread (blhip_bandwidth_probe) while this one fits a
    resident-eligible study again and again: whatever the probe decides each time, every fit is right and none pays a launch's time-out."""
    import threading
    import time
    from bayesloop_amd import engine as em
    eng = bl.get_engine()
    hog = em.extra_engine(getattr(eng, 'device', 0))
    stop = threading.Event()

    def run():
        while not stop.is_set():
            hog.bandwidth_probe(1 << 28, 40)

    c = RESIDENT['res_192_full']
    ref = cases.build(bl, c); ref.fit(silent=True)
    want = (ref.logEvidence, np.array(ref.posteriorSequence))
    eng.set_option('resident_probe_interval_s', 0)
    eng.set_option('quiet', 1)
    th = threading.Thread(target=run)
    th.start()
    try:
        time.sleep(0.05)
        worst, probes = 0.0, []
        for _ in range(12):
            t0 = time.perf_counter()
            S = cases.build(bl, c); S.fit(silent=True)
            worst = max(worst, time.perf_counter() - t0)
            probes.append(S.lastTiming['resident_probe'])
            assert abs(S.logEvidence - want[0]) <= 1e-11 * abs(want[0])
            np.testing.assert_allclose(np.asarray(S.posteriorSequence), want[1], rtol=1e-9, atol=1e-14)
            eng.set_option('resident_ok', 1)
    finally:
        stop.set()
        th.join()
        eng.set_option('resident_probe_interval_s', 1)
        eng.set_option('quiet', 0)
        eng.set_option('resident_ok', 1)
        del hog
    print('probe results beside the hog:', probes, 'slowest fit %.1f ms' % (worst * 1e3))
    assert worst < 0.2, (worst, probes)
