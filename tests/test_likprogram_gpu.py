"""Likelihood programs on the GPU: bllp::lik_program_kernel cell by cell against the longdouble interpreter (tests/likprogram_ref.py), fits
with the program path against the host-evaluated table and against the reference's own results, the library's refusals, the census.
Bounds and measured figures: tests/LIKELIHOOD_PROGRAMS.md.

for_grid_y (rows of T beyond one gridDim.y slice): the limit is the device's maxGridSize[1] (blhip_create); no option lowers it, and a
table of that many rows is no test of a few seconds -- the split is the shared helper's, exercised by the kernels it already serves."""
import dataclasses

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi, likprogram
from bayesloop_amd.exceptions import BackendError

import compare
import likprogram_cases as lc
import likprogram_ref as ref
import likprogram_studies as ls
import oracle_adapter as oa
from conftest import kernel_census

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.EXTENDED, reason='needs a long double wider than float64')]

CLASS_CAP = 0.05
KERNEL = 'bllp::lik_program_kernel'


def launches():
    return sum(c for c, n in kernel_census() if n.startswith(KERNEL))


@pytest.fixture(scope='module')
def reference_tables():
    """(case name, data dimensions) -> (program, L, E): computed once, shared, never modified"""
    out = {}
    for c in lc.cases():
        p = c.program()
        for dd in (1, 2):
            out[c.name, dd] = (p,) + ref.table(p, c.marginal, c.data[dd])
    return out


def device_table(program, marginal, data):
    eng = bl.get_engine()
    ops, consts = program.bind(marginal)
    eng.set_lik_program(ops, consts, program.step_values(data))
    return eng.lik_program_eval(marginal, data).reshape((len(data),) + tuple(len(m) for m in marginal))


def held(name, got, L, E):
    worst, frac, same = ref.compare(got, L, E, slack=ref.DEVICE_SLACK)
    print('%s: worst |error| / (2 x counted bound) %.3f, %.1f %% of the cells by class' % (name, worst, 100 * frac))
    assert frac <= CLASS_CAP, '%s: %.1f %% of the cells are compared by class only' % (name, 100 * frac)
    assert same, '%s: a cell differs in class (zero / subnormal, inf, NaN) from its longdouble value' % name
    assert worst <= 1.0, '%s: the device table misses twice the counted bound by a factor of %.3g' % (name, worst)


@pytest.mark.parametrize('dd', [1, 2])
@pytest.mark.parametrize('name', lc.case_names())
def test_device_table_cell_by_cell(name, dd, reference_tables):
    """37 cells, 33 x 19 and 5 x 7 x 6 by the density's number of parameters; T = 5 with one data dimension, T = 4 with two and one NaN in each."""
    c = [c for c in lc.cases() if c.name == name][0]
    p, L, E = reference_tables[name, dd]
    held('%s, %d data dimension(s)' % (name, dd), device_table(p, c.marginal, c.data[dd]), L, E)


def test_four_parameter_grid_cell_by_cell():
    expr, x, symbols, marg, d1, d2 = lc.four_parameter_expression()
    p = likprogram.compile_density(expr, x, symbols)
    for data in (d1, d2):
        L, E = ref.table(p, marg, data)
        held('3 x 4 x 5 x 3, %d data dimension(s)' % data.shape[1], device_table(p, marg, data), L, E)


def _hand(ops, consts=(), n_params=1):
    return likprogram.Program(ops, list(consts), [0] * len(consts), [], [], n_params)


def test_cos_and_sin_against_longdouble():
    """No density of the list holds a cosine: the two instructions alone, on 4001 arguments of [-40, 40].  Prints the largest error in u of
    the result -- the figure tests/LIKELIHOOD_PROGRAMS.md records and likprogram_ref.C_TRIG doubles."""
    arg = np.linspace(-40.0, 40.0, 4001)
    for code, fn in ((_abi.LP_COS, np.cos), (_abi.LP_SIN, np.sin)):
        p = _hand([(_abi.LP_PARAM, 0), (code, 0)])
        got = device_table(p, [arg], np.array([[0.5]]))[0]
        want = fn(arg.astype(ref.LD))
        with np.errstate(all='ignore'):
            rel = np.abs(got.astype(ref.LD) - want) / (ref.LD(ref.U) * np.abs(want))
        print('%s: largest error %.3f u of the result over [-40, 40]' % (likprogram.NAMES[code], float(np.nanmax(rel))))
        L, E = ref.table(p, [arg], np.array([[0.5]]))
        held(likprogram.NAMES[code], got[None], L, E)


def test_every_instruction_in_one_hand_written_program():
    """POW with a parameter exponent, ABS, LT / LE / EQ / AND / SELECT, COS / SIN inside an expression, POWI with a negative exponent:
    select(x < p0 and p0 <= p1, |sin(p0 x)| ** p1 + cos(p1) ** -3, (p0 == p0) * sqrt(p1) / exp(-p0) + log(p1)) on 33 x 19 cells."""
    P, D, C = _abi.LP_PARAM, _abi.LP_DATA, _abi.LP_CONST
    ops = [(P, 0), (D, 0), (_abi.LP_MUL, 0), (_abi.LP_SIN, 0), (_abi.LP_ABS, 0), (P, 1), (_abi.LP_POW, 0),
           (P, 1), (_abi.LP_COS, 0), (_abi.LP_POWI, -3), (_abi.LP_ADD, 0),
           (P, 0), (P, 0), (_abi.LP_EQ, 0), (P, 1), (_abi.LP_SQRT, 0), (_abi.LP_MUL, 0), (P, 0), (_abi.LP_NEG, 0), (_abi.LP_EXP, 0), (_abi.LP_DIV, 0),
           (P, 1), (_abi.LP_LOG, 0), (_abi.LP_ADD, 0),
           (D, 0), (P, 0), (_abi.LP_LT, 0), (P, 0), (P, 1), (_abi.LP_LE, 0), (_abi.LP_AND, 0), (_abi.LP_SELECT, 0), (C, 0), (_abi.LP_MUL, 0)]
    p = _hand(ops, consts=[0.75], n_params=2)
    marg = [lc.open_grid(0.2, 3.0, 33), lc.open_grid(0.3, 2.8, 19)]
    data = np.array([[0.4], [1.9], [2.7], [float('nan')]])
    L, E = ref.table(p, marg, data)
    cond = (data[:3, 0][:, None, None] < marg[0][None, :, None]) & (marg[0][None, :, None] <= marg[1][None, None, :])
    assert cond.any() and (~cond).any()                        # both branches of the SELECT are taken
    held('hand-written program', device_table(p, marg, data), L, E)


# ---- end to end: the program path against the host-evaluated table -----------------------------------------------------------------------------

def _fit_both_ways(make):
    """-> (results with lik_program = 1, results with 0, the problems the engine saw either way, timings)"""
    eng = bl.get_engine()
    seen, out, timing = {1: [], 0: []}, {}, {}
    orig = eng.fit
    try:
        for flag in (1, 0):
            eng.set_option('lik_program', flag)
            eng.fit = lambda problem, *a, _f=flag, **k: (seen[_f].append(problem), orig(problem, *a, **k))[1]
            S = make(bl)
            with np.errstate(all='ignore'):
                S.fit(silent=True)
            out[flag] = ls.results(S)
            timing[flag] = dict(S.lastTiming) if getattr(S, 'lastTiming', None) else {}
    finally:
        del eng.fit
        eng.set_option('lik_program', 1)
    return out[1], out[0], seen, timing


@pytest.mark.parametrize('study', ['normal_128x16', 'normal_128x16_hyper4', 'poisson_changepoint_200', 'frechet_6x8x5', 'scipy_t_5x16x12'])
def test_program_path_against_the_host_table(study):
    make = {'normal_128x16': ls.normal_study, 'normal_128x16_hyper4': lambda b: ls.normal_study(b, hyper=True),
            'poisson_changepoint_200': ls.poisson_changepoint_study, 'frechet_6x8x5': ls.frechet_study, 'scipy_t_5x16x12': ls.scipy_t_study}[study]
    before = launches()
    got, want, seen, timing = _fit_both_ways(make)
    assert seen[1] and all(p.obs_model == _abi.OM_PROGRAM and p.lik is None and p.lik_program is not None for p in seen[1])
    assert seen[0] and all(p.obs_model == _abi.OM_TABLE and p.lik is not None and p.lik_program is None for p in seen[0])
    assert launches() > before                                 # the kernel built the table of the first fit ...
    assert timing[1].get('fwd_kernel_variant') == timing[0].get('fwd_kernel_variant'), (timing[1], timing[0])      # ... for the same consumer
    print('%s: kernel variants %s / %s' % (study, timing[1].get('fwd_kernel_variant'), timing[1].get('bwd_kernel_variant')))
    compare.check(got, want, compare.GPU_TOL)


def test_no_table_is_uploaded_with_a_program():
    eng = bl.get_engine()
    S = ls.frechet_study(bl)
    S.fit(silent=True)
    assert eng.last_lik_upload_bytes == 0
    eng.set_option('lik_program', 0)
    try:
        S = ls.frechet_study(bl)
        S.fit(silent=True)
        assert eng.last_lik_upload_bytes == 8 * 10 * 6 * 8 * 5
    finally:
        eng.set_option('lik_program', 1)


@pytest.mark.parametrize('name', sorted(ls.GOLDEN))
def test_program_path_against_the_reference(name):
    """tests/golden/likprogram_*.npz: the reference itself fitted with bl.om.SymPy Normal (two parameters), Poisson (one), Frechet (three)
    (tests/golden/gen_likprogram_golden.py); compared at the parity bar with the program path on."""
    eng = bl.get_engine()
    assert eng.options.get('lik_program', 1.0) != 0
    before = launches()
    S = ls.GOLDEN[name](bl)
    S.fit(silent=True)
    assert launches() > before and eng.last_lik_upload_bytes == 0
    compare.check(ls.results(S), oa.load_golden(name), compare.GPU_TOL)


def test_the_library_refuses_what_it_cannot_evaluate():
    import bayesloop_amd.engine as em
    root = bl.get_engine()
    S = ls.poisson_study(bl, n=11, T=7)
    S._formatData()
    problem, program = S._compile()
    assert problem.obs_model == _abi.OM_PROGRAM
    ov = S._opValueMatrix(program)
    fresh = em.extra_engine(root.device)                       # a context nobody has armed
    with pytest.raises(BackendError, match='no likelihood program'):
        fresh.fit(dataclasses.replace(problem, lik_program=None), ov)
    ops, consts, step = problem.lik_program
    with pytest.raises(BackendError, match='step values'):     # (T, data_dim, n_step) of another T
        fresh.fit(dataclasses.replace(problem, lik_program=(ops, consts, step[:-1])), ov)
    with pytest.raises(BackendError, match='STEP'):            # validated when armed
        fresh.set_lik_program(np.array([[_abi.LP_STEP, 3]], dtype=np.int32), [], step)
    with pytest.raises(BackendError, match='AXIS'):            # a one-parameter table shorter than its axis
        fresh.set_lik_program(np.array([[_abi.LP_AXIS, 0]], dtype=np.int32), np.ones(5), np.zeros((7, 1, 0)))
        fresh.lik_program_eval([np.linspace(1, 2, 11)], np.ones((7, 1)))
    res = fresh.fit(problem, ov)                               # ... and the same context fits once the program is armed properly
    want = root.fit(problem, ov)
    assert res.log_evidence[0] == want.log_evidence[0]


def test_zz_census_shows_the_program_kernel_launched():
    rows = [(c, n) for c, n in kernel_census() if n.startswith(KERNEL)]
    assert len(rows) == 1 and rows[0][0] > 0, rows
