"""bl.Parser / Study.eval with a vector of time stamps, on the CPU (over the oracle engine, as tests/test_parser.py):

* ``P(query, t='all', series=...)`` against the reference's own loop over its scalar call (tests/golden/parser_series.npz, written by
  tests/golden/gen_parser_series_golden.py), at the bar tests/test_parser.py holds scalar queries to: 1e-9 + 1e-9 |want|;
* lists of time stamps, distribution queries, the errors;
* the query plan (bayesloop_amd/parser.py): the index spaces of every query, which subtrees became host tables, and the emitted program,
  evaluated in NumPy operation by operation, against the loop;
* the host-only parts of the C-ABI: blhip_host_query_plan (coverage of cells and steps, workspace within the budget, the refusal below
  the minimum) and blhip_host_query_check (every violation is refused with a message; no GPU, no context)."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import HipEngine
from bayesloop_amd.parser import _posterior_row
import parser_series_cases as psc
import query_program_ref as qref
from oracle_engine import OracleEngine

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'parser_series.npz'))
_built = {}


@pytest.fixture(autouse=True)
def oracle_engine():
    prev = bl.set_engine(OracleEngine())
    yield
    bl.set_engine(prev)


def studies(name):
    """Built once per session with the oracle engine and left unchanged."""
    if name not in _built:
        _built[name] = psc.BUILDERS[name](bl)
    return _built[name]


def parser(name):
    with psc._quiet():
        return bl.Parser(*studies(name))


def close(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.abs(got - want) > 1e-9 + 1e-9 * np.abs(want)
    assert not bad.any(), (got[bad], want[bad])


@pytest.mark.parametrize('case', sorted(psc.CASES))
def test_all_time_stamps_against_the_reference_loop(case):
    name, query, series, _, _ = psc.CASES[case]
    assert case + '_raises' not in GOLDEN
    got = parser(name)(query, t='all', silent=True, series=series)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    close(got, GOLDEN[case])
    assert 0.0 < GOLDEN[case].max() and GOLDEN[case].min() < 1.0          # (the fixture discriminates)


def test_study_eval_takes_the_vector_forms():
    S, = studies('gauss')
    close(S.eval('(mean - c)/std > 1', t='all', silent=True, series={'c': psc.GAUSS_C}), GOLDEN['gauss_series'])


def test_a_list_of_time_stamps_in_any_order_with_repeats():
    P = parser('gauss')
    stamps = list(studies('gauss')[0].formattedTimestamps)
    pick = [7, 0, 33, 7, 12, 1]
    t = [stamps[i] for i in pick]
    c = psc.GAUSS_C[pick]
    for form in (t, tuple(t), np.array(t)):
        got = P('(mean - c)/std > 1', t=form, silent=True, series={'c': c})
        want = [P(psc.textual('(mean - c)/std > 1', {'c': c}, i), t=ts, silent=True) for i, ts in enumerate(t)]
        assert np.array_equal(got, np.array(want))
    close(P('mean/std > 1', t=t, silent=True), GOLDEN['gauss_ratio'][pick])


def test_a_distribution_query_returns_the_pairs_of_the_loop():
    P = parser('two')
    t = [1, 3, 1]
    got = P('rate + rate2', t=t, silent=True)
    assert isinstance(got, list) and len(got) == 3
    for (x, p), ts in zip(got, t):
        xw, pw = P('rate + rate2', t=ts, silent=True)
        assert np.array_equal(x, xw) and np.array_equal(p, pw)


def test_one_summary_line():
    P = parser('two')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        P('rate - rate2 > 0', t='all')
    assert len(buf.getvalue().strip().split('\n')) == 1 and '5 time steps' in buf.getvalue()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        P('rate - rate2 > 0', t='all', silent=True)
    assert buf.getvalue() == ''


def test_errors():
    P = parser('two')
    ok = np.ones(5)
    for series in ({'rate': ok}, {'c': np.ones(4)}, {'c': np.ones((5, 1))}, {'c': np.array([1, 2, np.inf, 4, 5.0])}, {'c': np.array([1, 2, np.nan, 4, 5.0])},
                   {'1c': ok}):
        with pytest.raises(bl.ConfigurationError):
            P('rate - c > 0', t='all', silent=True, series=series)
    with pytest.raises(bl.ConfigurationError):
        P('rate - c > 0', t=2, silent=True, series={'c': ok})             # a series needs a vector t
    with pytest.raises(bl.ConfigurationError):
        P('rate - c > 0', silent=True, series={'c': ok})
    # what the scalar call raises is raised unchanged
    for query in ('rate@1 > 1', 'nonsense > 1', 'rate > 1 > 0', 'rate + > 1'):
        with pytest.raises(bl.ConfigurationError) as one:
            P(query, t=2, silent=True)
        with pytest.raises(bl.ConfigurationError) as many:
            P(query, t='all', silent=True)
        assert str(one.value) == str(many.value), query
    with pytest.raises(ValueError):
        P('rate > 1', t=[1, 17], silent=True)                             # no such time stamp
    with pytest.raises(bl.ConfigurationError):
        P('rate > 1', t=np.ones((2, 2)), silent=True)
    O = bl.OnlineStudy(storeHistory=False, silent=True)
    O.setOM(bl.om.Poisson('nu', bl.oint(0, 6, 30)), silent=True)
    with psc._quiet():
        O.add('walk', bl.tm.GaussianRandomWalk('sw', bl.cint(0.05, 0.4, 4), target='nu'))
        for d in [2, 3, 1]:
            O.step(d)
    with pytest.raises((bl.ConfigurationError, IndexError)) as one:          # (no history: nothing to select a time stamp from)
        O.eval('sw > 0.2', t=1, silent=True)
    with pytest.raises((bl.ConfigurationError, IndexError)) as many:
        O.eval('sw > 0.2', t=[1, 0], silent=True)
    assert type(one.value) is type(many.value) and str(one.value) == str(many.value)


def test_a_series_name_shadows_a_function_with_a_warning():
    P = parser('two')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = P('rate - sin > 0', t='all', silent=True, series={'sin': np.full(5, 2.5)})
    assert 'WARNING' in buf.getvalue() and '"sin"' in buf.getvalue()
    assert np.array_equal(got, P('rate - 2.5 > 0', t='all', silent=True))


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def evaluate_plan(plan):
    rows = np.array([np.ravel(_posterior_row(plan.study, int(i))) for i in plan.steps])
    return qref.weighted_count(plan.ops, plan.consts, plan.relation, plan.marginal, rows, **plan.spaces_kwargs())


@pytest.mark.parametrize('case', sorted(psc.CASES))
def test_plan_spaces_and_program(case):
    name, query, series, n_spaces, _ = psc.CASES[case]
    P = parser(name)
    plan = P.plan(query, 'all', series)
    assert plan.reason is None and plan.n_spaces == n_spaces == len(plan.spaces)
    assert plan.spaces[0][0] == 'param' and (plan.b_prob is None) == (n_spaces == 1)
    # the emitted program, evaluated in NumPy, is the loop
    want = np.array(P._loop(query, P._stamps('all'), P._series(series, len(plan.steps))))
    got = evaluate_plan(plan)
    assert np.all(np.abs(got - want) <= 1e-12 + 1e-12 * np.abs(want)), (got, want)
    # the library accepts it
    q, keep = make_query(plan.ops, plan.consts, plan.relation, plan.marginal, n_steps=len(plan.steps), **plan.spaces_kwargs())
    assert check(q, len(plan.steps)) == ''


def codes(plan):
    return [int(c) for c in plan.ops[:, 0]]


def test_which_subtrees_became_tables():
    L = _abi
    plan = parser('coal').plan('accident_rate < 1')
    assert plan.tables == [('axis0', '(-1.0 + accident_rate)')] and codes(plan) == [L.LP_AXIS]
    plan = parser('gauss').plan('mean/std > 1')
    assert plan.tables == [] and codes(plan) == [L.LP_CONST, L.LP_PARAM, L.LP_PARAM, L.LP_DIV, L.LP_ADD]
    plan = parser('gauss').plan('(mean - c)/std > 1', series={'c': psc.GAUSS_C})
    assert plan.tables == [('series', '<series>')] and plan.series.shape == (34, 1) and np.array_equal(plan.series[:, 0], psc.GAUSS_C)
    assert codes(plan) == [L.LP_CONST, L.LP_PARAM, L.LP_STEP, L.LP_NEG, L.LP_ADD, L.LP_PARAM, L.LP_DIV, L.LP_ADD]
    plan = parser('gauss').plan('(mean - 2*c)/std > 1', series={'c': psc.GAUSS_C})                 # a function of the series alone is a host column
    assert plan.tables == [('series', '<series>')] and np.array_equal(plan.series[:, 0], 2.0 * psc.GAUSS_C)
    plan = parser('gauss').plan('sin(mean) + cos(std) > 1')
    assert plan.tables == [('axis0', '(-1.0 + sin(mean))'), ('axis1', 'cos(std)')] and codes(plan) == [L.LP_AXIS, L.LP_AXIS, L.LP_ADD]
    S, = studies('gauss')
    off = int(plan.ops[1, 1]) >> 2                                                                # bit-identical to the host path's values
    assert np.array_equal(plan.consts[off:off + 20], np.cos(np.asarray(S.marginalGrid[1])))
    plan = parser('gauss').plan('exp(mean/std) > 2')
    assert plan.tables == [] and codes(plan) == [L.LP_CONST, L.LP_PARAM, L.LP_PARAM, L.LP_DIV, L.LP_EXP, L.LP_ADD]
    plan = parser('gauss').plan('std^mean > 1')
    assert codes(plan) == [L.LP_CONST, L.LP_PARAM, L.LP_PARAM, L.LP_POW, L.LP_ADD] and [int(a) for a in plan.ops[1:3, 1]] == [1, 0]
    plan = parser('gauss').plan('mean^2 + std > 1')
    assert codes(plan) == [L.LP_AXIS, L.LP_PARAM, L.LP_ADD]
    plan = parser('two').plan('rate*rate2 >= 4')
    assert plan.tables == [('b', 'rate2')] and codes(plan) == [L.LP_CONST, L.LP_PARAM, L.QP_BCOL, L.LP_MUL, L.LP_ADD]
    assert plan.b_prob.shape == (5, 50) and not plan.b_const and plan.study is studies('two')[0]
    plan = parser('two').plan('abs(rate - 3) + gamma(rate2 + 1) > 8')
    assert plan.tables == [('axis0', '(-8.0 + abs((rate - 3.0)))'), ('b', 'gamma((rate2 + 1.0))')] and codes(plan) == [L.LP_AXIS, L.QP_BCOL, L.LP_ADD]
    plan = parser('hyper').plan('mean*sigma > 0.5')
    assert plan.b_const and plan.b_prob.shape == (1, plan.b_values.shape[1]) and plan.study is studies('hyper')[0]
    plan = parser('hyper').plan('tc - lam > 0')
    assert plan.tables == [('b', '(-0.0 + tc)')] and plan.study is studies('hyper')[1] and plan.b_const
    assert codes(plan) == [L.QP_BCOL, L.LP_PARAM, L.LP_NEG, L.LP_ADD]
    plan = parser('hyper').plan('nu*sw < 0.6')
    assert plan.study is studies('hyper')[2] and not plan.b_const and plan.b_prob.shape == (5, 4)


def test_what_stays_on_the_loop():
    P = parser('two')
    plan = P.plan('(rate*rate2) + rate > 3')
    assert plan.reason is not None and plan.n_spaces == 3
    want = [P('(rate*rate2) + rate > 3', t=t, silent=True) for t in range(5)]
    assert np.array_equal(P('(rate*rate2) + rate > 3', t='all', silent=True), np.array(want))
    assert P.plan('gamma(rate*rate2) > 3').reason is not None                  # a function the device has not, over two spaces
    assert P.plan('rate*rate2 > 3', pair_max=2499).reason is not None and P.plan('rate*rate2 > 3', pair_max=2500).reason is None
    assert P.plan('rate + rate2').reason is not None                           # a distribution
    assert parser('hyper').plan('sigma > 0.15').reason is not None             # no parameter grid
    assert parser('hyper').plan('(mean + std)*sigma + tc > 1').n_spaces == 3


# ---- the host-only parts of the C-ABI ------------------------------------------------------------------------------------------------
def make_query(ops, consts, relation, marginal, n_steps=1, series=None, b_values=None, b_prob=None, b_const=False):
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 2)
    consts = np.ascontiguousarray(consts, dtype=float)
    ms = [np.ascontiguousarray(m, dtype=float) for m in marginal]
    q = _abi.Query()
    q.n_ops, q.n_consts, q.relation, q.ndim = len(ops), consts.size, relation, len(ms)
    q.ops, q.consts = ops.ctypes.data_as(C.POINTER(C.c_int32)), _abi.dptr(consts)
    for k, m in enumerate(ms):
        q.n[k], q.marginal[k] = len(m), _abi.dptr(m)
    keep = [ops, consts, ms]
    if series is not None:
        series = np.ascontiguousarray(series, dtype=float).reshape(n_steps, -1)
        q.n_series, q.series = series.shape[1], _abi.dptr(series)
        keep.append(series)
    if b_prob is not None:
        b_prob = np.ascontiguousarray(b_prob, dtype=float)
        b_values = np.ascontiguousarray(b_values, dtype=float).reshape(-1, b_prob.shape[-1])
        q.n_b, q.n_bcols, q.b_const = b_prob.shape[-1], len(b_values), int(b_const)
        q.b_values, q.b_prob = _abi.dptr(b_values), _abi.dptr(b_prob)
        keep += [b_values, b_prob]
    return q, keep


def check(q, n_steps=1):
    err = C.create_string_buffer(256)
    rc = _abi.load().blhip_host_query_check(C.byref(q) if q is not None else None, n_steps, err, 256)
    assert (rc == 0) == (err.value == b'') and rc in (0, -1)
    return err.value.decode()


def test_struct_layout():
    assert C.sizeof(_abi.Query) == 4 * 4 + 3 * 8 + 2 * 4 + 2 * 8 * _abi.MAX_DIM + 8 + 2 * 4 + 2 * 8
    assert _abi.Query.n.offset == 48 and _abi.Query.n_b.offset == 112 and _abi.Query.b_prob.offset == 136


def test_program_validation_without_a_gpu():
    L = _abi
    m = [np.linspace(0, 1, 5), np.linspace(1, 2, 3)]
    good = [(L.LP_PARAM, 0), (L.LP_PARAM, 1), (L.LP_DIV, 0)]
    assert check(make_query(good, [], L.QR_GT, m)[0]) == ''
    assert 'NULL' in check(None)
    bad = {
        'no ops': dict(ops=np.zeros((0, 2))),
        'underflow': dict(ops=[(L.LP_PARAM, 0), (L.LP_ADD, 0)]),
        'leaves': dict(ops=[(L.LP_PARAM, 0), (L.LP_PARAM, 1)]),
        'stack depth': dict(ops=[(L.LP_PARAM, 0)] * 17 + [(L.LP_ADD, 0)] * 16),
        'PARAM': dict(ops=[(L.LP_PARAM, 2)]),
        'CONST': dict(ops=[(L.LP_CONST, 1)], consts=[1.0]),
        'STEP': dict(ops=[(L.LP_STEP, 1)], series=[[1.0]]),
        'AXIS table': dict(ops=[(L.LP_AXIS, 0 | (1 << 2))], consts=np.ones(5)),             # 5 values of axis 0 from offset 1 of 5 constants
        'AXIS of parameter': dict(ops=[(L.LP_AXIS, 2)], consts=np.ones(5)),
        'BCOL without': dict(ops=[(L.QP_BCOL, 0)]),
        'BCOL 1 out of range': dict(ops=[(L.QP_BCOL, 1)], b_values=np.ones((1, 4)), b_prob=np.ones((1, 4))),
        'not part of a query': dict(ops=[(L.LP_DATA, 0)]),
        'unknown code': dict(ops=[(L.LP_PARAM, 0), (99, 0)]),
        'relation': dict(relation=5),
        'not finite': dict(ops=[(L.LP_STEP, 0)], series=[[np.nan]]),
        'ops (at most': dict(ops=[(L.LP_PARAM, 0)] + [(L.LP_NEG, 0)] * 256),
    }
    for want, change in bad.items():
        args = dict(ops=good, consts=[], relation=L.QR_GT, marginal=m)
        args.update(change)
        msg = check(make_query(**args)[0])
        assert want in msg, (want, msg)
    for select in ((L.LP_AND, 0), (L.LP_SELECT, 0)):
        assert 'not part of a query' in check(make_query([(L.LP_PARAM, 0), (L.LP_PARAM, 0), (L.LP_PARAM, 0), select], [], L.QR_GT, m)[0])
    q, keep = make_query(good, [], L.QR_GT, m)
    q.marginal[1] = None
    assert 'marginal[1] is NULL' in check(q)
    q, keep = make_query(good, [1.0], L.QR_GT, m)
    q.consts = None
    assert 'consts is NULL' in check(q)
    q, keep = make_query([(L.QP_BCOL, 0)], [], L.QR_GT, m, b_values=np.ones((1, 4)), b_prob=np.ones((1, 4)))
    q.b_prob = None
    assert 'b_prob is NULL' in check(q)
    assert 'n_steps' in check(make_query(good, [], L.QR_GT, m)[0], 0)
    q, keep = make_query(good, [], L.QR_GT, m)
    q.n[0] = 0
    assert 'grid axis' in check(q)


PLAN_SHAPES = [(2, 1, 0, 0), (105, 15, 1, 0), (1260, 16, 0, 0), (2053, 17, 2, 0), (512 * 512, 388, 1, 0), (1 << 24, 5000, 0, 0),
               (1000, 33, 0, 1), (1000, 400, 1, 257), (1260, 16, 0, 5), (256 * 256, 100, 0, 1000)]


@pytest.mark.parametrize('G,n_steps,n_series,n_b', PLAN_SHAPES)
def test_host_query_plan(G, n_steps, n_series, n_b):
    fixed = 4096 + 8 * n_b
    for b_const in ((False, True) if n_b else (False,)):
        full = HipEngine.query_plan(G, n_steps, n_series, n_b, b_const, fixed)
        assert full['n_chunks'] == 1 and full['steps_per_chunk'] == n_steps
        # the slabs cover the cells: the last one is not empty, none starts beyond the grid
        assert (full['n_slabs'] - 1) * full['slab'] < G <= full['n_slabs'] * full['slab'] and full['slab'] % 256 == 0
        if n_b:
            assert full['slab'] == 256
        else:
            assert full['slab'] >= 1024
        assert fixed <= full['min_budget_bytes'] <= full['workspace_bytes']
        # every budget between the minimum and the whole: the chunks cover the steps, the workspace stays within the budget
        lo, hi = full['min_budget_bytes'], full['workspace_bytes']
        for budget in sorted(b for b in {lo, lo + 1, (lo + hi) // 2, (lo + 3 * hi) // 4, hi - 1, hi} if b >= lo):
            plan = HipEngine.query_plan(G, n_steps, n_series, n_b, b_const, fixed, budget)
            assert plan is not None and plan['workspace_bytes'] <= budget and plan['min_budget_bytes'] == lo
            assert 1 <= plan['steps_per_chunk'] <= n_steps
            assert (plan['n_chunks'] - 1) * plan['steps_per_chunk'] < n_steps <= plan['n_chunks'] * plan['steps_per_chunk']
            assert (plan['slab'], plan['n_slabs']) == (full['slab'], full['n_slabs'])
            if budget < hi:
                assert plan['n_chunks'] > 1
        assert HipEngine.query_plan(G, n_steps, n_series, n_b, b_const, fixed, lo - 1) is None         # refused below the minimum


def test_host_query_plan_refuses_bad_arguments():
    from bayesloop_amd.exceptions import BackendError
    for args in ((0, 1), (1, 0), (1, 1, -1), (1, 1, 0, -1), (1 << 41, 1)):
        with pytest.raises(BackendError):
            HipEngine.query_plan(*args)
