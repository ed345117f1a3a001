"""
The fixtures of Deterministic shifts beyond 12 cells per step on 2-D grids (tests/bigshift_cases.py, tests/golden/gen_bigshift_golden.py)
against the CPU oracle, through the product's host logic with the oracle test double as its engine (tests/oracle_engine.py).  These pass
without the device path too: they show that the fixtures are the reference's.  Bar: compare.GPU_TOL with the registered FFT_FLOOR
(tests/tolerances.py).
"""
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import bigshift_cases as bc
import compare
import oracle_adapter as oa
from oracle_engine import OracleEngine
from test_combined_models_oracle import result_of, fit_case, run_online, check_online
from tolerances import FFT_TOL

ALL = dict(bc.BIGSHIFT, **bc.CONTROL)
DIRECT = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bigshift_direct_call.npz'))


@pytest.fixture(scope='module', autouse=True)
def oracle_engine():
    prev = bl.set_engine(OracleEngine())
    yield
    bl.set_engine(prev)


def check_direct(name):
    """the model's own computeForwardPrior / computeBackwardPrior against the reference model's; bar: 1e-9 relative above the FFT floor"""
    S, model = bc.direct_calls(bl)[name]
    S.setTransitionModel(model, silent=True)
    for k, (method, kind, t) in enumerate(bc.DIRECT_CALLS):
        x = bc.distribution(kind, S.gridSize, seed=k)
        fn = model.computeForwardPrior if method == 'fwd' else model.computeBackwardPrior
        got = np.asarray(fn(x.copy(), t), dtype=float)
        want = DIRECT['%s/%d' % (name, k)]
        assert got.shape == want.shape
        err = np.abs(got - want)
        print('%s call %d (%s, %s, t = %d): max |d| = %.3g, max |d| / |want| = %.3g' % (name, k, method, kind, t, err.max(), (err / np.abs(want)).max()))
        assert np.all(err <= FFT_TOL['post_atol'] + compare.GPU_TOL['post_rtol'] * np.abs(want)), (name, k, method, kind, t, err.max())


@pytest.mark.parametrize('case', sorted(ALL))
def test_oracle_matches_bigshift_fixture(case):
    c = ALL[case]
    S = fit_case(c)
    compare.check(result_of(S, c), oa.load_golden(case), compare.GPU_TOL, case_tol=c.get('tol'))


@pytest.mark.parametrize('case', sorted(bc.ONLINE))
def test_oracle_matches_bigshift_online_fixture(case):
    gold = oa.load_golden(case)
    check_online(run_online(bc.ONLINE[case]), gold, int(gold['n_models']))


@pytest.mark.parametrize('name', sorted(bc.direct_calls(bl)))
def test_oracle_matches_bigshift_direct_calls(name):
    check_direct(name)


def test_every_case_shifts_as_far_as_it_says():
    """the non-control cases shift by more than 12 cells in some step -- the largest step over the case's time stamps --, the control by
    less (what selects the kernel on the device); the crossing cases also stay below 12 cells in some step, in every chain"""
    import cases
    for name, c in ALL.items():
        S = cases.build(bl, c)
        lattice = dict(zip(S.observationModel.parameterNames, S.latticeConstant))
        ts = np.asarray(S.rawTimestamps, dtype=float)          # (segment length 1: the formatted time stamps are these)
        assert len(ts) >= 2 and ts[0] == 0.0
        steps = []                                   # per Deterministic model: |f(t + 1) - f(t)| in cells, (time stamps, chains)

        def walk(spec):
            if spec[0] == 'Deterministic':
                f = cases.FUNCS[spec[1]]
                steps.append(np.array([np.abs(np.atleast_1d(np.asarray(f(t + 1.0)) - np.asarray(f(t)))) for t in ts[:-1]]) / lattice[spec[2]])
            elif spec[0] in ('Combined', 'Serial'):
                for s in spec[1]:
                    walk(s)
        walk(c['tm'])
        far = max(float(s.max()) for s in steps)
        first = max(float(s[0].max()) for s in steps)
        assert far >= first
        assert (far < 12.0) if name in bc.CONTROL else (far > 12.0), (name, far)
        if name in bc.CROSSING:
            for s in steps:
                assert np.all(s.min(axis=0) < 12.0) and np.all(s.max(axis=0) > 12.0), (name, s)
