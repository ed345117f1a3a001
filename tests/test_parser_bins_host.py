"""Distribution queries (no relation) of bl.Parser / Study.eval with a vector of time stamps, the parts that need no GPU:

* the binning of the scalar call, factored into parser._binning: the scalar call returns the bits of the commit before
  (tests/golden/parser_bins_parent.npz) and agrees with the reference's own loop over all stamps (tests/golden/parser_bins_reference.npz,
  both written by tests/golden/gen_parser_bins_golden.py); the figures of every case (bins, smallest and largest bin, cells left out) are
  pinned, so a case cannot silently stop exercising skew, NaNs or left-out cells;
* Parser.planDistribution: the map of a one-space query reproduces the scalar call bit for bit (np.bincount over the map adds the cells in
  the scalar call's order), every query that stays on the loop says why, and over the oracle engine -- which has no device path -- the vector
  call returns the loop's bits and raises what the scalar call raises;
* the host-only part of bayesloop_amd/csrc/blhip_bins.hpp through the stand-alone program tests/host/bins_plan_main.cpp (built plain and with
  -fsanitize=address,undefined; its own main, not loaded into Python): the per-slab order is a stable permutation, the groups and runs
  cover every cell with a bin exactly once, the NumPy restatement of the kernels' summation order (tests/parser_bins_cases.py) reproduces
  the program's sums bit for bit, the chunk plan stays within its budget and refuses one below its minimum;
* the same through the C-ABI: blhip_host_bins_check, blhip_host_bins_plan."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import HipEngine
from bayesloop_amd.exceptions import BackendError
from bayesloop_amd.parser import _posterior_row
import parser_bins_cases as pbc
from oracle_engine import OracleEngine

psc = pbc.psc
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(ROOT, 'tests', 'host', 'bins_plan_main.cpp')
PARENT = np.load(os.path.join(HERE, 'golden', 'parser_bins_parent.npz'))
REFERENCE = np.load(os.path.join(HERE, 'golden', 'parser_bins_reference.npz'))
_built = {}


@pytest.fixture(autouse=True)
def oracle_engine():
    prev = bl.set_engine(OracleEngine())
    yield
    bl.set_engine(prev)


def studies(name):
    """Built once per session with the oracle engine and left unchanged."""
    if name not in _built:
        _built[name] = pbc.BUILDERS[name](bl)
    return _built[name]


def parser(name):
    with psc._quiet():
        return bl.Parser(*studies(name))


CASES = [(b, q) for b in ('gauss', 'coal') for q in pbc.QUERIES[b]]


# ---- the scalar call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('builder,query', CASES)
def test_the_scalar_call_returns_the_bits_of_the_commit_before(builder, query):
    P = parser(builder)
    stamps = list(studies(builder)[0].formattedTimestamps)
    for i in pbc.PARENT_STAMP_INDICES:
        x, p = P(query, t=stamps[i], silent=True)
        assert np.array_equal(x, PARENT['%s|%d|x' % (pbc.key(builder, query), i)])
        assert np.array_equal(p, PARENT['%s|%d|p' % (pbc.key(builder, query), i)])


@pytest.mark.parametrize('builder,query', pbc.REFERENCE_CASES)
def test_the_loop_against_the_reference_loop(builder, query):
    P = parser(builder)
    got = P(query, t='all', silent=True)
    x, p = REFERENCE[pbc.key(builder, query) + '|x'], REFERENCE[pbc.key(builder, query) + '|p']
    assert len(got) == len(x)
    for (gx, gp), wx, wp in zip(got, x, p):
        assert np.allclose(gx, wx, rtol=1e-12, atol=1e-12)
        assert np.all(np.abs(gp - wp) <= 1e-9 + 1e-9 * np.abs(wp))
    assert p.max() > 0.05 and (p.sum(axis=1) > 0.5).all()                   # (the fixture discriminates)


@pytest.mark.parametrize('builder,query', sorted(pbc.FIGURES))
def test_the_figures_of_the_cases(builder, query):
    plan = parser(builder).planDistribution(query)
    assert plan.reason is None
    want = pbc.FIGURES[(builder, query)]
    got = pbc.figures(np.where(plan.bin >= 0, plan.bin, 0), plan.bin >= 0, plan.n_bins + 1)
    assert got[:3] == want[:3] and (want[3] is None or got[3] == want[3]), (got, want)
    if query in pbc.GAUSS_NAN and builder == 'gauss':
        S, = studies(builder)
        with np.errstate(all='ignore'):
            assert np.isnan(np.log(np.ravel(S.grid[0]))).sum() == pbc.GAUSS_NAN[query] and got[3] > pbc.GAUSS_NAN[query]


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('builder,query', CASES + [('hyper_alone', q) for q in pbc.QUERIES['hyper_alone']])
def test_the_map_reproduces_the_scalar_call(builder, query):
    P = parser(builder)
    S = studies(builder)[0]
    stamps = list(S.formattedTimestamps)
    pick = [len(stamps) - 1, 0, 2, 0]
    plan = P.planDistribution(query, t=[stamps[i] for i in pick])
    assert plan.reason is None and plan.study is S and plan.steps.tolist() == pick
    assert plan.bin.dtype == np.int32 and plan.bin.shape == (int(np.prod(S.gridSize)),)
    assert plan.bin.min() >= -1 and plan.bin.max() < plan.n_bins == len(plan.labels)
    inside = plan.bin >= 0
    for i in pick:
        x, p = P(query, t=stamps[i], silent=True)
        row = np.ravel(_posterior_row(S, i))
        assert np.array_equal(plan.labels, x)
        assert np.array_equal(np.bincount(plan.bin[inside], weights=row[inside], minlength=plan.n_bins), p)
    assert P.planDistribution(query).steps.tolist() == list(range(len(stamps)))


def test_queries_that_stay_on_the_loop_say_why():
    P2, PH, PC, PG = parser('two'), parser('hyper'), parser('coal'), parser('gauss')
    for P, query, kw, word in ((P2, 'rate + rate2', {}, 'two index spaces'), (P2, 'rate@1 + rate', {}, '"@"'), (P2, 'rate@1*2', {}, '"@"'),
                               (P2, 'rate*c', dict(series={'c': np.ones(5)}), 'series'), (PH, 'sigma*2', {}, 'hyper-parameters'),
                               (PH, 'mean*sigma', {}, 'two index spaces'), (PH, 'mean*sigma - nu', {}, 'three or more'),
                               (PG, 'mean > 1', {}, 'no distribution query'), (PG, 'mean/std', dict(t=[]), 'no time stamps'),
                               (PG, 'mean/std', dict(t=[0.0, 1e9]), 'ValueError'), (PG, 'mean +', {}, 'ConfigurationError'),
                               (PC, '1/accident_rate', {}, 'IndexError'), (PC, 'accident_rate*0', {}, 'ValueError')):
        plan = P.planDistribution(query, **kw)
        assert plan.reason is not None and word in plan.reason, (query, plan.reason)
        assert plan.bin is None
    # Parser.plan answers what it answered before
    assert P2.plan('rate + rate2').reason is not None and PG.plan('mean/std').reason == 'no probability query'
    assert PG.plan('mean/std > 1').reason is None


@pytest.mark.parametrize('builder,query,error', pbc.RAISING)
def test_the_vector_call_raises_what_the_scalar_call_raises(builder, query, error):
    P = parser(builder)
    stamps = list(studies(builder)[0].formattedTimestamps)
    with pytest.raises(error) as one:
        with np.errstate(all='ignore'):
            P(query, t=stamps[3], silent=True)
    with pytest.raises(error) as many:
        with np.errstate(all='ignore'):
            P(query, t='all', silent=True)
    assert str(one.value) == str(many.value)


@pytest.mark.parametrize('builder', sorted(pbc.QUERIES))
def test_the_vector_call_over_the_oracle_engine_is_the_loop(builder):
    P = parser(builder)
    S = studies(builder)[0]
    assert not hasattr(getattr(S, '_posterior_pending', None), 'bins')       # (a test double: no device path)
    stamps = list(S.formattedTimestamps)
    t = [stamps[i] for i in (3, 0, len(stamps) - 1, 3)]
    for query in pbc.QUERIES[builder]:
        for form in ('all', t, np.array(t)):
            got = P(query, t=form, silent=True)
            want = [P(query, t=ts, silent=True) for ts in (stamps if isinstance(form, str) else t)]
            assert isinstance(got, list) and len(got) == len(want)
            for (x, p), (xw, pw) in zip(got, want):
                assert np.array_equal(x, xw) and np.array_equal(p, pw)
        assert S.eval(query, t=t[:2], silent=True)[1][1].shape == want[1][1].shape


# ---- the stand-alone host program -------------------------------------------------------------------------------------------------------
def _hipcc():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    return hipcc


def _runner(exe, env=None):
    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
        return [line.split() for line in r.stdout.splitlines()]
    return run


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('bins_plan') / 'bins_plan')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)
    return _runner(exe)


SLAB, GW_MAX, N_ROWS = 64, 8, 3


def check_order(run, tmp_path, name, G, n_bins, m, slab=SLAB, gw_max=GW_MAX):
    """One map through `order`: the tables against the rules of the header, the sums against the NumPy restatement."""
    mp, rp = str(tmp_path / 'map.i32'), str(tmp_path / 'rows.f64')
    m.astype(np.int32).tofile(mp)
    fam = pbc.row_families(G, N_ROWS, 5)
    rows = np.concatenate([fam['tiny'][:2], fam['exact'][:1]])
    rows.tofile(rp)
    out = run('order', mp, n_bins, slab, gw_max, rp)
    head = [int(x) for x in out[0][1:]]
    assert out[0][0] == 'order' and head[:4] == [G, n_bins, slab, -(-G // slab)], name
    gw, n_runs, n_groups, n_multi, max_slots, cells_in = head[4:10]
    assert gw == pbc.group_width(m, slab, gw_max) and cells_in == int((m >= 0).sum()), name
    runs = pbc.runs_of(m, slab)
    assert n_runs == len(runs), name
    groups = [(int(w[1]), w[3], [int(c) for c in w[4:]]) for w in out if w[0] == 'group']
    assert len(groups) == n_groups and all(len(c) == gw for _, _, c in groups)
    per_slab = {int(w[1]): (int(w[2]), int(w[3])) for w in out if w[0] == 'slab'}
    multi = {int(w[1]): (int(w[2]), int(w[3])) for w in out if w[0] == 'multi'}
    assert len(multi) == n_multi and sum(v[0] for v in per_slab.values()) == n_groups and sum(v[1] for v in per_slab.values()) == n_multi
    # every run: its cells in ascending order (the order is stable), cut into groups of gw, padding only behind the last cell
    at, seen = 0, []
    for r, (k, b, cells) in enumerate(runs):
        n = -(-len(cells) // gw)
        mine = groups[at:at + n]
        assert all(kk == k for kk, _, _ in mine)
        flat = [c for _, _, cs in mine for c in cs]
        assert flat[:len(cells)] == cells.tolist() and all(c == -1 for c in flat[len(cells):]), (name, r)
        if n == 1:
            assert mine[0][1] == 'r%d' % r and r not in multi
        else:
            slot0, ng = multi[r]
            assert ng == n and [d for _, d, _ in mine] == ['s%d' % (slot0 + i) for i in range(n)]
        seen += cells.tolist()
        at += n
    assert at == n_groups and sorted(seen) == np.nonzero(m >= 0)[0].tolist()            # every cell with a bin exactly once, no other
    # the slots of a slab are dense from 0, and max_slots is the most any slab needs
    slots = {}
    for r, (slot0, ng) in multi.items():
        slots.setdefault(runs[r][0], []).extend(range(slot0, slot0 + ng))
    assert all(sorted(v) == list(range(len(v))) for v in slots.values()) and max_slots == max([len(v) for v in slots.values()] + [0])
    # the runs of a bin in ascending slab order
    bins = {int(w[1]): [int(r) for r in w[2:]] for w in out if w[0] == 'bin'}
    assert sorted(bins) == list(range(n_bins))
    for b, rs in bins.items():
        assert rs == [r for r, (k, bb, _) in enumerate(runs) if bb == b]
    sums = np.array([[float.fromhex(x) for x in w[2:]] for w in out if w[0] == 'sums'])
    want = pbc.kernel_order_sums(rows, m, n_bins, slab, gw)
    assert sums.shape == want.shape and np.array_equal(sums, want), name
    assert np.array_equal(sums[2], np.bincount(m[m >= 0], weights=rows[2][m >= 0], minlength=n_bins))       # (exact in any order)
    return head


def test_the_order_of_every_map(program, tmp_path):
    for name, (G, n_bins, m) in sorted(pbc.maps(SLAB).items()):
        check_order(program, tmp_path, name, G, n_bins, m)
    G, n_bins, m = pbc.maps(SLAB)['skewed']
    assert check_order(program, tmp_path, 'skewed, gw 2', G, n_bins, m, gw_max=2)[4] == 2
    assert check_order(program, tmp_path, 'skewed, odd slab length', G, n_bins, m, slab=50)[3] == -(-G // 50)
    G, n_bins, m = pbc.maps(SLAB)['one-bin']
    assert check_order(program, tmp_path, 'one bin, gw 16', G, n_bins, m, gw_max=16)[4] == 16


def test_the_order_of_the_parser_maps(program, tmp_path):
    for builder, query in CASES:
        plan = parser(builder).planDistribution(query)
        check_order(program, tmp_path, query, plan.bin.size, plan.n_bins, plan.bin)


def test_check_shape_and_plan(program, tmp_path):
    mp = str(tmp_path / 'map.i32')
    for m, n_bins, word in (([0, 1, -1, 2], 3, None), ([0, 3], 3, 'bin[1] = 3'), ([0, -2], 3, 'bin[1] = -2'), ([0], 0, 'n_bins = 0'), ([], 3, 'bin is NULL')):
        np.array(m, dtype=np.int32).tofile(mp)
        out = program('check', mp, n_bins)[0]
        assert (out[1] == '0') if word is None else (out[1] == '-1' and word in ' '.join(out[2:])), out
    # what a caller may ask for is brought into the kernel's ranges: an even slab, at most 16 steps, a power-of-two width, the LDS of a CU
    assert program('shape', 512, 8, 8) == [['shape', '512', '8', '8']]
    assert program('shape', 1001, 99, 5) == [['shape', '500', '16', '4']]
    assert program('shape', 4096, 16, 100) == [['shape', '512', '16', '16']] and program('shape', 1, 0, 0) == [['shape', '64', '1', '1']]
    for slab, sb, gw in ((512, 8, 8), (4096, 16, 16), (1024, 8, 2), (2048, 4, 4)):
        s = [int(x) for x in program('shape', slab, sb, gw)[0][1:]]
        assert 8 * s[1] * (2 * s[0] + 2) <= 160 * 1024 and s[0] % 2 == 0
    # the chunk plan
    up = lambda b: (b + 255) // 256 * 256
    for n_bins, n_runs, tb, n_steps, sb in ((21, 21, 5000, 34, 8), (700, 1400, 123456, 1000, 8), (1, 0, 256, 3, 16), (65536, 300000, 10 ** 7, 4096, 8)):
        ask = lambda budget: [int(x) for x in program('plan', n_bins, n_runs, tb, n_steps, sb, budget)[0][1:]]
        full = ask(2.0 ** 62)
        need = lambda s: up(tb) + up(8 * s) + up(8 * max(1, s * n_runs)) + up(8 * s * n_bins)
        assert full[:3] == [1, n_steps, 1] and full[3] == need(n_steps) and full[4] == need(1)
        assert full[5:] == [up(tb), up(tb) + up(8 * n_steps), up(tb) + up(8 * n_steps) + up(8 * max(1, n_steps * n_runs))]
        assert ask(full[4] - 1)[:2] == [0, 0] and ask(full[4] - 1)[4] == full[4]                # refused below the minimum, which it still tells
        for budget in (full[4], full[3] - 1, (full[3] + full[4]) // 2, need(sb) + 300, need(2 * sb + 3)):
            if budget < full[4]:
                continue
            ok, spc, chunks, ws = ask(budget)[:4]
            assert ok == 1 and ws == need(spc) <= budget and chunks == -(-n_steps // spc)
            assert spc == n_steps or need(spc + sb) > budget                                    # no larger chunk of whole blocks fits
            assert spc <= sb or spc % sb == 0
    assert program('plan', 0, 0, 0, 5, 8, 1e9)[0][1:3] == ['0', '0'] and program('plan', 5, 0, 0, 5, 17, 1e9)[0][1] == '0'


def test_host_functions_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan on the host side, as a stand-alone executable"""
    exe = str(tmp_path / 'bins_plan_san')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', SRC, '-o', exe, '-fsanitize=address,undefined'], check=True, capture_output=True, text=True, timeout=300)
    run = _runner(exe, dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    for name, (G, n_bins, m) in sorted(pbc.maps(SLAB).items()):
        check_order(run, tmp_path, name, G, n_bins, m)
    G, n_bins, m = pbc.maps(SLAB)['skewed']
    check_order(run, tmp_path, 'skewed, slab 50', G, n_bins, m, slab=50, gw_max=2)
    assert run('plan', 700, 1400, 123456, 1000, 8, 1e7)[0][1] == '1' and run('shape', 4096, 16, 100)[0][1] == '512'
    np.array([0, 7], dtype=np.int32).tofile(str(tmp_path / 'bad.i32'))
    assert run('check', str(tmp_path / 'bad.i32'), 3)[0][1] == '-1'


# ---- the C-ABI, host-only ----------------------------------------------------------------------------------------------------------------------
def test_host_bins_check_and_plan_through_the_abi():
    lib = _abi.load()
    err = C.create_string_buffer(256)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    good = np.array([0, -1, 2, 1], dtype=np.int32)
    assert lib.blhip_host_bins_check(ptr(good), 4, 3, err, 256) == 0
    for m, G, n_bins, word in ((good, 4, 2, 'bin[2] = 2'), (np.array([-2], dtype=np.int32), 1, 1, 'bin[0] = -2'), (good, 0, 3, 'G = 0'),
                               (good, 4, 0, 'n_bins = 0'), (good, 4, 2 ** 31, 'n_bins')):
        assert lib.blhip_host_bins_check(ptr(m), G, n_bins, err, 256) == -1 and word in err.value.decode(), (word, err.value)
    assert lib.blhip_host_bins_check(None, 4, 3, err, 256) == -1 and 'bin is NULL' in err.value.decode()
    shape = HipEngine.bins_plan(1000, 7, 50)
    assert shape['slab'] % 2 == 0 and 1 <= shape['sb'] <= 16 and shape['n_slabs'] == -(-1000 // shape['slab']) and shape['n_runs'] == 0
    slab = shape['slab']
    for name, (G, n_bins, m) in sorted(pbc.maps(slab).items()):
        plan = HipEngine.bins_plan(G, n_bins, 33, m)
        assert plan['n_runs'] == len(pbc.runs_of(m, slab)) and plan['gw'] == pbc.group_width(m, slab, 8), name
        assert (plan['steps_per_chunk'], plan['n_chunks']) == (33, 1) and plan['lds_bytes'] <= 160 * 1024
        lo = plan['min_budget_bytes']
        assert HipEngine.bins_plan(G, n_bins, 33, m, budget=lo - 1) is None
        two = HipEngine.bins_plan(G, n_bins, 33, m, budget=plan['workspace_bytes'] - 1)
        assert two['n_chunks'] >= 2 and two['workspace_bytes'] < plan['workspace_bytes']
    with pytest.raises(BackendError):
        HipEngine.bins_plan(4, 3, 5, np.array([0, 1, 2, 3]))                 # a bin outside the map's range
    with pytest.raises(BackendError):
        HipEngine.bins_plan(5, 3, 5, np.array([0, 1, 2]))
    with pytest.raises(BackendError):
        HipEngine.bins_plan(0, 3, 5)
