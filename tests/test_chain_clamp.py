"""
RegimeSwitch inside the chain-resident kernel on two-parameter grids (bayesloop_amd/csrc/blhip_chainclamp.hpp: blc::chain_clamp_kernel;
selectors: chain_admit / chain_settle in blhip_chain_plan.hpp, run by ChainRun::setup in blhip_fit_paths.hpp; blcp::chain_clamp_envelope / chain_clamp_route in blhip_chainclamp_plan.hpp).

Every instantiation -- ring length 4, 8 .. 24 x 128 / 256 / 512 rows x {forward without storing, forward storing, backward storing} -- is
launched on the smallest grids with more than one strip and held to the CPU oracle at the parity bar (compare.GPU_TOL); every case asserts
the kernels it launched, the path's variant number in lastTiming and that nothing fell back.  Reference semantics pinned:
transitionModels.py:394-415 (RegimeSwitch), :632-662 (combined models), core.py:372-470 (Study.fit), :1349-1366 (hyper average).
See tests/CHAIN_CLAMP.md.
"""
import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import chain_clamp_cases as cc
import compare
import oracle_adapter as oa
from conftest import kernel_census
from test_gpu_parity import result_of, _ill_tol

pytestmark = pytest.mark.gpu

DEFAULTS = dict(chain_clamp=1, chain_force_fail_batch=-1, chain_force_fail_stage=0)


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)
    bl.set_engine(prev)


class Options:
    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        for k, v in self.opts.items():
            bl.get_engine().set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            bl.get_engine().set_option(k, DEFAULTS[k])


def _counts():
    return {name: c for c, name in kernel_census()}


_ORACLE = {}


def oracle(c):
    """the oracle's results of a case: computed once, shared by the tests that fit the case under several options, left unchanged"""
    key = repr(c)
    if key not in _ORACLE:
        with np.errstate(all='ignore'):
            _ORACLE[key] = oa.run(c)
    return _ORACLE[key]


def run(c, expect, forbid=(), fallbacks=0, variant=cc.VARIANT):
    """Fit the case; the kernels of `expect` were launched and none of `forbid`; the variant number of the path; the oracle's results."""
    before = _counts()
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    got = result_of(S, c)
    after = _counts()
    ran = sorted(k for k in after if after[k] > before.get(k, 0))
    missing = [k for k in expect if k not in ran]
    assert not missing, 'expected kernel(s) not launched: %s\nlaunched: %s\ntiming: %s' % (missing, ran, S.lastTiming)
    unwanted = [k for k in ran if any(k.startswith(f) for f in forbid)]
    assert not unwanted, 'kernel(s) launched that should not have been: %s' % unwanted
    if fallbacks == 0:
        assert S.lastTiming['resident_fallbacks'] == 0, S.lastTiming
    else:
        assert S.lastTiming['resident_fallbacks'] >= fallbacks, S.lastTiming
    if variant is not None:
        assert S.lastTiming['fwd_kernel_variant'] == variant, S.lastTiming
        if not c.get('fit'):
            assert S.lastTiming['bwd_kernel_variant'] == variant, S.lastTiming
    want = oracle(c)
    gold = dict(logEvidence=want['logEvidence'], localEvidence=want['localEvidence'])
    for k in ('posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution'):
        if k in want and want[k] is not None and k in got and len(np.atleast_1d(want[k])):
            gold[k] = np.asarray(want[k])
    compare.check(got, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
    return S


# ---- every instantiation: ring length x rows x pass, exact and padded grids ---------------------------------------------------------------

SWEEP = [(g, nk) for g in cc.GRIDS for nk in cc.RINGS]


@pytest.mark.parametrize('grid,nk', SWEEP, ids=['%dx%d-nk%d' % (g[0], g[1], nk) for g, nk in SWEEP])
def test_chain_clamp_kernel_instantiations(grid, nk):
    ntw = cc.ntw_of(grid[0])
    sig = cc.chain_sigmas(nk, grid[0])
    tm = cc.model('switch_alone' if nk == 4 else 'walk_then_switch', sig[0], -7)
    seed = cc.seed_of(grid, nk)
    with Options(chain_clamp=2):
        run(cc.study(grid, tm, seed, 'full'), cc.kernels_of(nk, ntw, 'full'))
        run(cc.study(grid, tm, seed, 'evidence'), cc.kernels_of(nk, ntw, 'evidence'))


# ---- the models, in the three forms of a Study ----------------------------------------------------------------------------------------------

MODEL_GRIDS = [(128, 32), (100, 40), (400, 40)]


@pytest.mark.parametrize('kind', ['full', 'forward', 'evidence'])
@pytest.mark.parametrize('name', ['walk_then_switch', 'switch_then_walk', 'switch_alone'])
@pytest.mark.parametrize('grid', MODEL_GRIDS, ids=['%dx%d' % g for g in MODEL_GRIDS])
def test_models_and_forms_of_a_study(grid, name, kind):
    nk = 4 if name == 'switch_alone' else 12
    sig = cc.chain_sigmas(12, grid[0])[1]                  # radius 14: ring length 12
    with Options(chain_clamp=2):
        run(cc.study(grid, cc.model(name, sig, -5), 12000 + grid[0], kind), cc.kernels_of(nk, cc.ntw_of(grid[0]), kind))


@pytest.mark.parametrize('pmin', cc.PMIN)
@pytest.mark.parametrize('name', ['walk_then_switch', 'switch_then_walk', 'switch_alone'])
def test_clamp_regimes(name, pmin):
    """nothing clamped (10**-330 is 0) ... every cell clamped (the prior becomes uniform); tests/test_chain_clamp_host.py asserts on the
    oracle's side that the four values sit in those regimes on these very cases"""
    grid = (100, 40)
    nk = 4 if name == 'switch_alone' else 8
    with Options(chain_clamp=2):
        run(cc.study(grid, cc.model(name, cc.chain_sigmas(8, grid[0])[0], pmin), 12500, 'full'), cc.kernels_of(nk, 1, 'full'))


def test_a_ring_length_between_the_instantiated_ones_and_a_384_row_grid():
    """radius 11 would be ring length 10: it runs on 12; 300 rows would be the 384-row geometry: it runs padded inside 512"""
    grid = cc.ROWS_384
    lattice = (cc.HI - cc.LO) / (grid[0] - 1.0)
    with Options(chain_clamp=2):
        run(cc.study(grid, cc.model('walk_then_switch', 11 / 4.0 * lattice, -6), 12600, 'full'), cc.kernels_of(12, 4, 'full'))


# ---- hyper-studies: the limit differs per chain of one launch -----------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['full', 'evidence'])
@pytest.mark.parametrize('grid', [(128, 32), (100, 40), (256, 32)], ids=['128x32', '100x40', '256x32'])
def test_hyper_study_over_width_and_pmin(grid, kind):
    sig = cc.chain_sigmas(12, grid[0])
    tm = ('Combined', [('GRW', 'sigma', sig, 'mean', None), ('RS', 'log10pMin', cc.PMIN, None)])         # 3 widths x 4 limits = 12 chains
    with Options(chain_clamp=2):
        S = run(cc.study(grid, tm, 13000 + grid[0], kind, study='HyperStudy'), cc.kernels_of(12, cc.ntw_of(grid[0]), kind))
    assert len(S.logEvidenceList) == 12


def test_hyper_study_of_the_switch_alone():
    tm = ('RS', 'log10pMin', cc.PMIN, None)
    with Options(chain_clamp=2):
        run(cc.study((200, 40), tm, 13500, 'full', study='HyperStudy'), cc.kernels_of(4, 2, 'full'))


# ---- recovery, options ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stage', [1, 2, 3])
def test_recovery_from_a_failed_check(stage):
    """chain_force_fail_batch / _stage make ONE host check of the batch fail (no kernel argument changes, nothing faults): the batch is
    repeated on the launch-per-step kernels, the results are the oracle's, and the next fit takes the resident kernels again (after a
    give-up -- stage 3 -- once the context's resident paths are re-armed, as tests/test_fold_recovery.py does)"""
    grid = (100, 40)
    c = cc.study(grid, cc.model('walk_then_switch', cc.chain_sigmas(8, grid[0])[0], -6), 14000, 'full')
    try:
        with Options(chain_clamp=2, chain_force_fail_batch=0, chain_force_fail_stage=stage):
            run(c, ['blk::step_kernel<2, 0, false>', 'blk::step_kernel<2, 1, true>'], fallbacks=1, variant=0)
    finally:
        if stage == 3:
            bl.get_engine().set_option('resident_ok', 1)
    with Options(chain_clamp=2):
        run(c, cc.kernels_of(8, 1, 'full'))


@pytest.mark.parametrize('kind', ['full', 'forward', 'evidence'])
@pytest.mark.parametrize('grid', [(128, 32), (100, 40)], ids=['128x32', '100x40'])
def test_option_off_keeps_the_launch_per_step_kernel(grid, kind):
    c = cc.study(grid, cc.model('walk_then_switch', cc.chain_sigmas(8, grid[0])[0], -6), 14500, kind)
    step = {'full': ['blk::step_kernel<2, 0, false>', 'blk::step_kernel<2, 1, true>'], 'forward': ['blk::step_kernel<2, 0, true>'],
            'evidence': ['blk::step_kernel<2, 0, false>']}[kind]
    with Options(chain_clamp=0):
        run(c, step, forbid=('blc::chain_clamp_kernel<',), variant=0)
    with Options(chain_clamp=2):
        run(c, cc.kernels_of(8, 1, kind), forbid=('blk::step_kernel<',))


def test_default_option_follows_the_routing_rule():
    """chain_clamp = 1: steps x passes >= 8 takes the resident kernels (profiles/chain_clamp_notes.md) -- a full fit of T = 6 steps does, an
    evidence-only fit of the same series keeps the launch-per-step kernel"""
    grid = (128, 32)
    tm = cc.model('walk_then_switch', cc.chain_sigmas(8, grid[0])[0], -6)
    run(cc.study(grid, tm, 14600, 'full'), cc.kernels_of(8, 1, 'full'))
    run(cc.study(grid, tm, 14600, 'evidence'), ['blk::step_kernel<2, 0, false>'], forbid=('blc::chain_clamp_kernel<',), variant=0)
