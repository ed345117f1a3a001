"""
The posterior predictive (Study.simulate on the device, bayesloop_amd/csrc/blhip_predictive.hpp), the part a CPU can check:

* the plan of a call (blhip_host_predictive_plan / blpp::predictive_plan): over a sweep of grids, time ranges, numbers of values and
  budgets every cell lies in exactly one slab, every value in exactly one chunk, the workspace stays within the budget and a chunk has at
  least one row -- through the library's entry point and through the stand-alone program tests/host/predictive_plan_main.cpp, built plain
  and with -fsanitize=address,undefined (host code only; the program has its own main);
* ``simulate(x, t='all')`` over the engine double (no ``predictive`` on its posterior handle: the host code) against the fixture the
  reference wrote by looping its own ``simulate`` over every time stamp (tests/golden/gen_predictive_golden.py);
* what has not changed: the refusal of segment length 2, the error of an unknown time stamp, the host results of ``t=None`` / ``t``.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd.engine import HipEngine
import cases
import oracle_adapter as oa
import predictive_cases as pc
from oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'predictive_plan_main.cpp')


@pytest.fixture
def oracle_engine():
    prev = bl.set_engine(OracleEngine())
    yield
    bl.set_engine(prev)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------

def check_plan(G, T, X, average, budget, p):
    slab, ns, rows, nc = p['slab'], p['n_slabs'], p['rows_per_chunk'], p['n_chunks']
    assert slab >= pc.SLAB_MIN and slab % pc.KSTEP == 0
    assert (ns - 1) * slab < G <= ns * slab                          # every cell in exactly one of the slabs [s slab, min(G, (s + 1) slab))
    assert 1 <= rows <= min(X, pc.ROWS_MAX)
    assert (nc - 1) * rows < X <= nc * rows                          # every value in exactly one chunk
    assert p['min_budget_bytes'] <= p['workspace_bytes'] <= budget
    assert p['workspace_bytes'] >= 8 * (T * X + (G if average else 0) + rows * G + ns * T * rows)


def test_plan_sweep():
    n = 0
    for G in pc.PLAN_G:
        for T in pc.PLAN_T:
            for X in pc.PLAN_X:
                for average in (False, True):
                    Tn = 1 if average else T
                    big = HipEngine.predictive_plan(G, Tn, X, average)
                    check_plan(G, Tn, X, average, float(1 << 62), big)
                    lo = big['min_budget_bytes']
                    assert HipEngine.predictive_plan(G, Tn, X, average, lo - 1) is None
                    for budget in sorted({max(lo, b) for b in (lo, lo + 8 * G, (lo + big['workspace_bytes']) // 2, big['workspace_bytes'] - 1, big['workspace_bytes'])}):
                        p = HipEngine.predictive_plan(G, Tn, X, average, budget)
                        check_plan(G, Tn, X, average, budget, p)
                        assert p['slab'] == big['slab'] and p['rows_per_chunk'] <= big['rows_per_chunk']
                        n += 1
                    assert HipEngine.predictive_plan(G, Tn, X, average, lo)['workspace_bytes'] == lo          # (more than one row only where rounding to 256 bytes makes them free)
                    assert HipEngine.predictive_plan(G, Tn, X, average, big['workspace_bytes'])['rows_per_chunk'] == min(X, pc.ROWS_MAX)
    assert n > 1000


def test_plan_of_the_test_grids():
    grids = pc.contract_grids(lambda G, T, X: HipEngine.predictive_plan(G, T, X))
    assert grids['two-slabs+5'] == (2 * pc.SLAB_MIN + 5,)
    # a long series spreads the waves over the time tiles, a short one over the slabs
    assert HipEngine.predictive_plan(1 << 20, 1, 16)['n_slabs'] == 1024 and HipEngine.predictive_plan(1 << 20, 4096, 16)['n_slabs'] == 8
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(bl.exceptions.BackendError):
            HipEngine.predictive_plan(*bad)


def _hipcc():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    return hipcc


def _groups():
    out = []
    for G in pc.PLAN_G:
        for T, X in ((1, 1), (17, 16), (256, 17), (33, 1000)):
            for average in (0, 1):
                for budget in (0, 1e18, -1):
                    out += [G, 1 if average else T, X, average, budget]
    return [str(int(v)) for v in out]


def _run(exe, env=None):
    r = subprocess.run([exe] + _groups(), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0].split() == ['TM', '16', 'XT', '16', 'NXT', '8', 'RUN', '8', 'KSTEP', '32', 'SLAB_MIN', '256', 'SLABS_MAX', '1024']
    assert lines[-1] == 'covered'
    return [l for l in lines if l.startswith('plan ')], r


def test_plan_program_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / 'predictive_plan')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)
    plans, _ = _run(exe)
    assert len(plans) == len(pc.PLAN_G) * 4 * 2 * 3
    for line in plans:
        lhs, rhs = line[5:].split(' -> ')
        G, T, X, average, budget = [int(v) for v in lhs.split()]
        ok, slab, ns, rows, nc, ws, lo = [int(v) for v in rhs.split()[:7]]
        p = HipEngine.predictive_plan(G, T, X, bool(average), budget)
        assert (p is not None) == bool(ok) == (budget >= lo)
        if p is not None:
            assert (p['slab'], p['n_slabs'], p['rows_per_chunk'], p['n_chunks'], p['workspace_bytes'], p['min_budget_bytes']) == (slab, ns, rows, nc, ws, lo)
            check_plan(G, T, X, bool(average), budget, p)


def test_plan_program_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan on the host side, as a stand-alone executable"""
    exe = str(tmp_path / 'predictive_plan_san')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', SRC, '-o', exe, '-fsanitize=address,undefined'], check=True, capture_output=True, text=True, timeout=300)
    _, r = _run(exe, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


# ---- simulate(x, t='all') on the host path ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', sorted(pc.GOLDEN_X))
def test_simulate_all_matches_the_references_loop(oracle_engine, case):
    gold = oa.load_golden('predictive')
    S = cases.build(bl, case)
    with np.errstate(all='ignore'):
        S.fit(**cases.fit_kwargs(case))
    x = gold[case + '_x']
    assert np.array_equal(x, np.asarray(pc.GOLDEN_X[case], dtype=float)) and np.array_equal(gold[case + '_t'], S.formattedTimestamps)
    for density, key in ((False, '_prob'), (True, '_density')):
        got = S.simulate(x, t='all', density=density)
        assert got.shape == (len(S.formattedTimestamps), len(x))
        np.testing.assert_allclose(got, gold[case + key], rtol=1e-9, atol=1e-300)
        # row i is simulate(x, t=formattedTimestamps[i])
        i = len(S.formattedTimestamps) // 3
        np.testing.assert_allclose(S.simulate(x, t=S.formattedTimestamps[i], density=density), got[i], rtol=1e-13, atol=1e-300)


def test_simulate_all_on_a_posterior_already_on_the_host(oracle_engine):
    S = cases.build(bl, 'kat_grw')
    S.fit(silent=True)
    seq = S.posteriorSequence                      # (materialised: no handle left)
    assert S._posterior_pending is None
    x = np.arange(0, 6)
    got = S.simulate(x, t='all', density=True)
    want = np.array([[np.sum(S.observationModel.pdf(S.grid, [xi]) * row) for xi in x] for row in seq])
    np.testing.assert_allclose(got, want, rtol=1e-14)
    prob = S.simulate(x, t='all')
    np.testing.assert_allclose(prob, want / want.sum(axis=1, keepdims=True), rtol=1e-14)
    # a row without any probability under x: 0 / 0, as in the reference
    S.posteriorSequence = np.array(seq)
    S.posteriorSequence[2] = 0.0
    with np.errstate(all='ignore'):
        prob = S.simulate(x, t='all')
    assert np.all(np.isnan(prob[2])) and np.all(np.isfinite(prob[[0, 1, 3, 4]]))


def test_simulate_all_of_an_online_study(oracle_engine):
    import contextlib
    import io
    c = cases.ONLINE_CASES['online_poisson_3tm']
    S = cases.build_online(bl, c)
    data = np.asarray(cases.online_data(c)[:5], dtype=float)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        for d in data:
            S.step(d)
    seq = np.asarray(S.posteriorSequence)
    x = np.linspace(float(np.nanmin(data)), float(np.nanmax(data)), 5)
    want = np.array([[np.sum(S.observationModel.pdf(S.grid, [xi]) * row) for xi in x] for row in seq])
    got = S.simulate(x, t='all', density=True)
    assert got.shape == (len(seq), 5)
    np.testing.assert_allclose(got, want, rtol=1e-14)


# ---- unchanged behaviour -------------------------------------------------------------------------------------------------------------------

def test_errors_are_unchanged(oracle_engine):
    S = bl.Study(silent=True)
    S.loadData(np.array([1, 0, 1, 0, 0]), silent=True)
    S.set(bl.om.AR1('rho', bl.oint(-1, 1, 20), 'sigma', bl.oint(0, 1, 20)), bl.tm.Static(), silent=True)
    for t in (None, 1, 'all'):
        with pytest.raises(NotImplementedError):
            S.simulate([0.], t=t)
    S = cases.build(bl, 'kat_grw')
    S.fit(silent=True)
    for t in (17, -1, 2.5, 'avg', 'ALL'):
        with pytest.raises(bl.exceptions.PostProcessingError):
            S.simulate([0., 1.], t=t)
    assert S.simulate([0., 1.], t=2).shape == (2,)                 # the next call works
    S2 = cases.build(bl, 'kat_grw')
    with pytest.raises(bl.exceptions.PostProcessingError):
        S2.simulate([0., 1.], t='all')                             # nothing fitted
