"""
RegimeSwitch inside the chain-resident kernel on two-parameter grids (bayesloop_amd/csrc/blhip_chainclamp.hpp), the part a CPU can check:

* blhip_host_unlag scheme 2 (include/blhip.h): the normalisers of a pass that mixes clamped steps -- exact scale, they waited for the sum of
  the step before -- with steps in mode 0 -- the lagged scale of blc::chain_kernel --, against a longdouble restatement;
* the envelope and the routing rule (blhip_chainclamp_plan.hpp: pure host functions) through the stand-alone program
  tests/host/chain_clamp_plan_main.cpp, built plain and with -fsanitize=address,undefined (host code only, its own main);
* the inputs of tests/test_chain_clamp.py: the radii select the ring lengths the cases are named after; the four log10pMin values sit in
  the regimes they stand for -- counted on the oracle's side.
See tests/CHAIN_CLAMP.md.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import chain_clamp_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'chain_clamp_plan_main.cpp')
CLAMPED = 0x40


# ---- the scale algebra ----------------------------------------------------------------------------------------------------------------------

def _simulate(norms, lag, clamped, units):
    """What blc::chain_clamp_kernel reports, in longdouble: S_k = S_(k-1) s_k n_k u_k with the kernel's rule for s_k -- exact at a clamped
    step, the lagged normaliser otherwise -- where n_k is the reference's normaliser (core.py:385) and u_k the mass of the clamped prior the
    reference renormalises by (transitionModels.py:410; sum slot 1: the host divides by it afterwards, so blhip_host_unlag returns n_k u_k)."""
    LD = np.longdouble
    T = len(norms)
    S, s = np.zeros(T, dtype=LD), np.ones(T, dtype=LD)
    for k in range(T):
        if k >= lag:
            s[k] = (S[k - lag - 1] if k - lag - 1 >= 0 else LD(1)) * s[k - lag] / S[k - lag]
        if k > 0 and clamped[k]:
            s[k] = LD(1) / S[k - 1]
        S[k] = (LD(1) if k == 0 else S[k - 1]) * s[k] * LD(norms[k]) * LD(units[k])
    return S, s


@pytest.mark.parametrize('lag', [2, 3, 4])
@pytest.mark.parametrize('pattern', ['all', 'none', 'alternating', 'random', 'bursts'])
def test_host_recovers_the_normalisers_of_a_pass_with_clamped_steps(pattern, lag):
    from bayesloop_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(1000 * lag + len(pattern))
    T = 300
    norms = np.exp(rng.normal(-3.0, 1.5, T))
    clamped = {'all': np.ones(T, bool), 'none': np.zeros(T, bool), 'alternating': np.arange(T) % 2 == 1, 'random': rng.random(T) < 0.4,
               'bursts': (np.arange(T) // 7) % 3 == 0}[pattern].copy()
    clamped[0] = False                                         # (the first step of a pass has no transition)
    units = np.where(clamped, 1.0 + rng.random(T) * 30.0, 1.0)  # mass of a clamped prior: >= 1 (cells are only ever raised)
    S, s = _simulate(norms, lag, clamped, units)
    assert np.all(np.abs(np.log(S.astype(np.float64))) < 60.0)  # (an exact scale resets the state's magnitude: nothing accumulates)
    sums, scales = S.astype(np.float64), np.zeros(T)
    kinds = np.where(clamped, CLAMPED, 0).astype(np.uint8)
    assert lib.blhip_host_unlag(2, _abi.dptr(sums), T, lag, kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), _abi.dptr(scales)) == 0
    np.testing.assert_allclose(sums, (norms * units), rtol=1e-12)
    np.testing.assert_allclose(scales, s.astype(np.float64), rtol=1e-12)
    if clamped.any():
        k = int(np.flatnonzero(clamped)[0])
        assert scales[k] == 1.0 / S.astype(np.float64)[k - 1]   # lag 0: the exact scale, bit for bit the kernel's division
        # scheme 1 -- the parent's only chain scheme -- does not know clamped steps: it reconstructs other normalisers
        plain = S.astype(np.float64)
        assert lib.blhip_host_unlag(1, _abi.dptr(plain), T, lag, None, None) == 0
        assert not np.allclose(plain, norms * units, rtol=1e-6)


def test_host_unlag_scheme_2_with_restart_kinds_and_out_of_range_sums():
    from bayesloop_amd import _abi
    lib = _abi.load()
    T, lag = 40, 4
    rng = np.random.default_rng(5)
    norms = np.exp(rng.normal(-2.0, 1.0, T))
    clamped = np.arange(T) % 3 == 1
    S, _ = _simulate(norms, lag, clamped, np.ones(T))
    bad = S.astype(np.float64)
    bad[17] = 1e-200
    kinds = np.where(clamped, CLAMPED, 0).astype(np.uint8)
    assert lib.blhip_host_unlag(2, _abi.dptr(bad), T, lag, kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), None) == 1
    ok = S.astype(np.float64)
    assert lib.blhip_host_unlag(2, _abi.dptr(ok), T, lag, None, None) == 0          # (no kinds: scheme 1's rule)


# ---- the envelope and the routing rule --------------------------------------------------------------------------------------------------------

def _hipcc():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    return hipcc


FIELDS = ('ndim', 'gaussian_recurrence', 'n0', 'n1', 'radius0', 'radius1', 'regime_switch_only', 'composed', 'restarts', 'same_taps', 'resumed',
          'carried', 'backward_init', 'cus')
INSIDE = dict(ndim=2, gaussian_recurrence=1, n0=200, n1=200, radius0=20, radius1=0, regime_switch_only=1, composed=0, restarts=0, same_taps=1,
              resumed=0, carried=0, backward_init=0, cus=256)


def _args(**over):
    f = dict(INSIDE, **over)
    return [str(int(f[k])) for k in FIELDS]


def _run(exe, groups, env=None):
    r = subprocess.run([exe] + [a for g in groups for a in g], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    consts = dict(zip(out[0].split()[0::2], map(int, out[0].split()[1::2])))
    facts = [tuple(int(v) for v in l.split('->')[1].split()) for l in out if l.startswith('facts ')]
    route = {tuple(int(v) for v in l.split()[1:8]): int(l.split()[8]) for l in out if l.startswith('route ')}
    return consts, facts, route, out[-1], r.stderr


@pytest.fixture(scope='module')
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('chain_clamp_plan') / 'chain_clamp_plan')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)
    return exe


OUTSIDE = {
    'restarts': dict(restarts=1),
    'not_equal': dict(regime_switch_only=0),
    'walk_on_the_second_parameter': dict(radius1=3),
    'radius_41': dict(radius0=41),
    '1024_rows': dict(n0=1024),
    '513_rows': dict(n0=513),
    '31_rows': dict(n0=31),
    'table_model': dict(gaussian_recurrence=0),
    'resumed': dict(resumed=1),
    'carried': dict(carried=1),
    'backward_init': dict(backward_init=1),
    'more_blocks_than_cus': dict(n1=1024, cus=63),
    '1025_columns': dict(n1=1025),
    'composed_stage_list': dict(composed=1),
    'tap_sets_that_change': dict(same_taps=0),
    'one_parameter': dict(ndim=1),
    'radius_beyond_the_rows': dict(n0=32, radius0=32),
}


def test_the_envelope_admits_what_it_should(plan_program):
    groups = [_args(), _args(n0=32, n1=16, radius0=0), _args(n0=512, n1=1024, radius0=40), _args(n0=384, n1=40), _args(n0=128, n1=32, radius0=39),
              _args(n1=1024, cus=64)]
    consts, facts, _, last, _ = _run(plan_program, groups)
    assert consts == dict(ROWS_MIN=32, ROWS_MAX=512, COLS_MAX=1024, RADIUS_MAX=40, STRIP_COLS=16, VARIANT=cc.VARIANT, MIN_PASS_STEPS=8)
    assert last == 'rings ok'
    assert [f[0] for f in facts] == [1] * len(groups)
    assert [f[1:] for f in facts] == [(256, 13, 16), (128, 1, 4), (512, 64, 24), (512, 3, 16), (128, 2, 24), (256, 64, 16)]


@pytest.mark.parametrize('why', sorted(OUTSIDE))
def test_the_envelope_is_off_for(plan_program, why):
    _, facts, _, _, _ = _run(plan_program, [_args(), _args(**OUTSIDE[why])])
    assert facts[0][0] == 1 and facts[1][0] == 0, why


def test_the_routing_rule(plan_program):
    """option 1: steps x passes >= 8 for any chains x strips the envelope admits (profiles/chain_clamp_notes.md: the classes measured
    faster; below it the fits were measured equal or slower, or not measured)"""
    _, _, route, _, _ = _run(plan_program, [])
    assert len(route) == 3 * 2 * 19
    for (opt, env, chains, strips, steps, passes, cus), got in route.items():
        want = bool(env) and chains >= 1 and strips <= cus and (opt == 2 or (opt == 1 and steps * passes >= 8))
        assert got == int(want), (opt, env, chains, strips, steps, passes, cus)
    on = lambda chains, strips, steps, passes, cus=256: route[(1, 1, chains, strips, steps, passes, cus)]
    assert on(1, 13, 1000, 2) == 1 and on(1, 13, 1000, 1) == 1                       # the single study of the notes
    assert on(64, 16, 256, 2) == 1 and on(64, 32, 256, 1) == 1 and on(17, 16, 256, 1) == 1      # the hyper-studies; a last round of one chain
    assert [on(1, 13, T, 2) for T in (2, 3, 4)] == [0, 0, 1]                         # full fits: from 4 steps
    assert [on(1, 13, T, 1) for T in (4, 7, 8)] == [0, 0, 1]                         # evidence-only / forward-only fits: from 8
    assert on(1, 2, 6, 2) == 1 and on(1, 2, 6, 1) == 0                               # the T = 6 cases of tests/test_chain_clamp.py
    assert on(9, 32, 4, 2) == 1 and on(3, 2, 3, 1) == 0 and on(200, 2, 16, 2) == 1
    assert route[(1, 1, 1, 64, 100, 2, 32)] == 0 and route[(2, 1, 1, 64, 100, 2, 32)] == 0     # more strips than CUs: never
    assert all(v == 0 for k, v in route.items() if k[0] == 0 or k[1] == 0)


def test_host_functions_under_the_sanitizers(tmp_path):
    """the planner with AddressSanitizer and UBSan on the host side, as a stand-alone executable (nothing sanitized is loaded into python)"""
    exe = str(tmp_path / 'chain_clamp_plan_san')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', SRC, '-o', exe, '-fsanitize=address,undefined'], check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    groups = [_args()] + [_args(**v) for v in OUTSIDE.values()] + [_args(n0=2 ** 30, n1=2 ** 30, radius0=2 ** 30, cus=1)]
    _, facts, _, last, err = _run(exe, groups, env=env)
    assert last == 'rings ok' and facts[0][0] == 1 and all(f[0] == 0 for f in facts[1:])
    assert 'runtime error' not in err and 'AddressSanitizer' not in err


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------

def _radius(sigma, n0):
    return int(4.0 * sigma / ((cc.HI - cc.LO) / (n0 - 1.0)) + 0.5)             # transitionModels.py:108-111 -> scipy.ndimage.gaussian_filter1d


@pytest.mark.parametrize('grid', cc.GRIDS + [cc.ROWS_384], ids=lambda g: '%dx%d' % g)
def test_radii_select_the_ring_lengths(grid):
    assert [(16 + 2 * ((max(_radius(cc.chain_sigmas(nk, grid[0])[0], grid[0]), 0) + 7) // 8 * 8)) // 4 if nk > 4 else 4 for nk in cc.RINGS] == cc.RINGS
    for nk in cc.RINGS[1:]:
        assert [_radius(s, grid[0]) for s in cc.chain_sigmas(nk, grid[0])] == [2 * nk - 9, 2 * nk - 10, 2 * nk - 11]
    assert grid[1] > 16                                                        # at least two strips: one strip needs no exchange
    assert (grid in cc.PADDED or grid == cc.ROWS_384) == (grid[0] % 128 != 0 or grid[1] % 16 != 0)


def test_the_likelihoods_of_the_cases_are_normal_numbers():
    """std >= 0.5 on a mean grid of +-8: every localEvidence entry of these cases is compared at the bar (no registered exception applies)"""
    import cases
    import oracle_adapter as oa
    from oracle import bl_oracle as orc
    for grid in cc.GRIDS:
        c = cc.study(grid, ('Static',), cc.seed_of(grid, 8))
        data = cases.make_data(c['data'])
        assert np.all(np.abs(data) < 8.0)
        g = orc.Grid([cases.make_values(oa._Orc, v) for _, v in c['om'][1]])
        with np.errstate(all='ignore'):
            L = np.array([orc.processed_pdf('gaussian', g.grid, seg) for seg in orc.moving_window(data, 1)])
        assert L.min() > 2.3e-308


@pytest.mark.parametrize('name', ['walk_then_switch', 'switch_then_walk', 'switch_alone'])
def test_the_four_limits_sit_in_their_regimes(name):
    """over the steps of tests/test_chain_clamp.py::test_clamp_regimes: -330 clamps no cell, +1 all of them, -7 and -3 strictly between"""
    grid = (100, 40)
    counts = {}
    for pmin in cc.PMIN:
        counts[pmin], G = cc.clamped_cells(cc.study(grid, cc.model(name, cc.chain_sigmas(8, grid[0])[0], pmin), 12500, 'full'))
        assert len(counts[pmin]) == cc.T - 1
    assert all(n == 0 for n in counts[-330])
    assert all(n == G for n in counts[1])
    assert all(0 < n < G for n in counts[-7]) and all(0 < n < G for n in counts[-3])
    assert all(a < b for a, b in zip(counts[-7], counts[-3]))
