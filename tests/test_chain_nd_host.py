"""
The chain-resident N-D kernel (bayesloop_amd/csrc/blhip_chain_nd.hpp), the part a CPU can check:

* the LDS need bln::chain_nd_lds_doubles -- 2 G + walks x (LW + 1) + n_sum + 120 doubles: two state buffers, a tap slot of the batch's
  widest radius per walk, the grid values, the reduction scratch --, the envelope it gives under the 150 KB a block is allowed (19 200 doubles), the block size and the
  routing predicate, through the stand-alone program tests/host/chain_nd_lds_main.cpp, built plain and with
  -fsanitize=address,undefined (host code only; the program has its own main);
* the inputs of tests/test_chain_nd.py: the walks have the radii the cases are named after, the grids sit on the side of the envelope
  they are meant to, every hyper-study has exactly the number of chains its test is about;
* the oracle against the two fixtures the reference wrote (tests/golden/gen_chain_nd_golden.py).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import chain_nd_cases as cn
import compare
import oracle_adapter as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'chain_nd_lds_main.cpp')


def _hipcc():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    return hipcc


def _runner(exe):
    def run(*quads):
        args = [str(int(v)) for p in quads for v in p]
        out = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        consts = dict(zip(out[0].split()[0::2], map(int, out[0].split()[1::2])))
        rows = [tuple(int(v) for v in l.split()) for l in out[1:1 + len(quads)]]
        route = {tuple(int(v) for v in l.split()[1:7]): (int(l.split()[7]), float(l.split()[8]), float(l.split()[9]), int(l.split()[10])) for l in out if l.startswith('route ')}
        return consts, rows, route, out[-1]
    return run


@pytest.fixture(scope='module')
def lds_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('chain_nd_lds') / 'chain_nd_lds')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)
    return _runner(exe)


def test_constants_of_the_envelope(lds_program):
    consts, _, _, last = lds_program()
    assert consts == dict(NT_SMALL=256, NT_LARGE=1024, RED=cn.RED, MAXPASS=8, MIN_CHAINS=cn.MIN_CHAINS, LIMIT=150 * 1024, SMALL_BYTES=32 * 1024)
    assert consts['MIN_CHAINS'] >= 16
    assert last == 'monotonic'


@pytest.mark.parametrize('G,lw,np_,ns', [(1, 0, 0, 1), (105, 9, 2, 15), (378, 8, 2, 19), (1260, 40, 1, 37), (1260, 16, 3, 37), (8000, 12, 2, 73),
                                         (9408, 47, 2, 167), (9408, 48, 2, 167), (9472, 3, 2, 168), (2000, 5000, 2, 40), (4000, 5600, 2, 60), (1260, 40, 8, 37)])
def test_need_and_envelope(lds_program, G, lw, np_, ns):
    _, rows, _, _ = lds_program((G, lw, np_, ns))
    need = cn.lds_doubles(G, lw, np_, ns)
    assert rows[0][:5] == (G, lw, np_, ns, need)
    assert rows[0][5] == int(need <= cn.LDS_LIMIT)
    assert rows[0][6] == (256 if need * 8 <= 32 * 1024 else 1024)
    assert rows[0][7] == (8 if rows[0][6] == 256 else 10)
    assert rows[0][8] == (cn.LDS_LIMIT - cn.RED - np_ * (lw + 1) - ns) // 2


def test_envelope_edges(lds_program):
    """4 x 16 x 147 cells with two walks of radius <= 47 fill the 150 KB but for one double; one tap or one scale value more is refused;
    without walks 9539 cells fit beside 3 grid values; a radius far beyond any axis still counts"""
    _, rows, _, _ = lds_program((9408, 47, 2, 167), (9408, 48, 2, 167), (9472, 3, 2, 168), (9538, 0, 0, 3), (9539, 0, 0, 3), (1260, 8260, 2, 37),
                                (1260, 8261, 2, 37), (1969, 3, 2, 30), (1970, 3, 2, 30))
    assert [r[5] for r in rows] == [1, 0, 0, 1, 0, 1, 0, 1, 1]
    assert rows[0][4] == cn.LDS_LIMIT - 1
    assert [r[6] for r in rows[-2:]] == [256, 1024]           # the block size changes at 32 KB = 4096 doubles = 2 x 1969 + 8 + 30 + 120


def _model(G, B, walks, W, threads):
    """the cost model of bln::chain_nd_route, restated (256 CUs; a block of 256 threads -- up to 32 KB of LDS --: 4 blocks per CU)"""
    slots = 256 * (4 if threads == 256 else 1)
    kernel = -(-B // slots) * (5.0 + 0.125e-3 * W * G)
    plain = 4.7 * (walks + 1) + 0.3 * max(0, W - 7 * walks) + 27e-6 * B * G
    return kernel, plain


def test_routing_predicate(lds_program):
    _, _, route, _ = lds_program()
    assert len(route) == 3 * 2 * 20
    for (opt, env, G, B, walks, W), (got, kernel, plain, threads) in route.items():
        k, p = _model(G, B, walks, W, threads)
        assert abs(kernel - k) <= 1e-3 and abs(plain - p) <= 1e-3, (G, B, walks, W)
        beyond = (G, W) in ((1260, 81), (9408, 102))          # the two shapes of the table with a radius beyond its axis (40 on 18, 47 as one)
        want = bool(env) and (opt == 2 or (opt == 1 and B >= cn.MIN_CHAINS and 1.25 * k <= p and not beyond))
        assert got == int(want), (opt, env, G, B, walks, W)
    on = lambda G, B, walks, W: route[(1, 1, G, B, walks, W)][0]
    # the floor; the classes measured faster on the kernel; the classes measured slower (8000 and more cells at 16 chains) and their neighbours
    assert [on(1260, B, 2, 14) for B in (1, 8, 15, 16, 64, 512, 5000)] == [0, 0, 0, 1, 1, 1, 1]
    assert [on(8000, B, 2, 14) for B in (16, 32, 64, 400)] == [0, 0, 1, 1]
    assert [on(9408, 16, 2, 14), on(9408, 256, 2, 14), on(9408, 16, 2, 102)] == [0, 1, 0]
    assert [on(1260, 64, 2, 42), on(1260, 16, 1, 81), on(1260, 16, 0, 0), on(105, 16, 2, 28)] == [1, 0, 0, 1]
    assert [on(4000, 16, 2, 14), on(5600, 16, 2, 14)] == [1, 0]
    assert route[(2, 1, 1260, 1, 2, 14)][0] == 1 and route[(2, 1, 9408, 16, 2, 102)][0] == 1 and route[(0, 1, 1260, 512, 2, 14)][0] == 0
    assert all(v[0] == 0 for k, v in route.items() if k[1] == 0)


def test_host_functions_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan on the host side, as a stand-alone executable"""
    exe = str(tmp_path / 'chain_nd_lds_san')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', SRC, '-o', exe, '-fsanitize=address,undefined'], check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    r = subprocess.run([exe, '9408', '47', '2', '167', '9472', '3', '2', '168', '1', '0', '0', '1', '12000', '20000', '8', '400'], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == 'monotonic'
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------

def _walks(spec):
    if spec[0] in ('Combined', 'Serial'):
        return [w for s in spec[1] for w in _walks(s)]
    return [spec] if spec[0] == 'GRW' else []


def _widest(c):
    return max(cn.radius(s, cn.lattice(c['om'], w[3])) for w in _walks(c['tm']) for s in np.atleast_1d(w[2]))


def _cells(c):
    return int(np.prod([v[3] for _, v in c['om'][1]]))


ALL = dict(cn.ND, **cn.BELOW, **cn.FORCED, cnd_split=cn.SPLIT)


def test_lattice_constants_are_the_packages():
    import bayesloop_amd as bl
    for om in (cn.T3, cn.SMALL, cn.LARGEST, cn.REFUSED, cn.J4):
        S = cases.build(bl, dict(study='Study', data=('series', 1, 3), om=om, tm=('Static',)))
        for (name, _), lat in zip(om[1], S.latticeConstant):
            assert abs(cn.lattice(om, name) - lat) <= 1e-12 * lat


def test_radii_of_the_cases():
    assert [cn.radius(s, cn.lattice(cn.T3, 'loc')) for s in cn.cells(cn.T3, 'loc', [0, 1, 5, 18, 23, 40])] == [0, 1, 5, 18, 23, 40]
    assert _widest(cn.ND['cnd_hyper_middle']) == 40 > 2 * 18
    assert _widest(cn.ND['cnd_three_walks']) == 16 > 14
    assert _widest(cn.ND['cnd_small_grid']) == 9 > 2 * 3
    assert _widest(cn.ND['cnd_largest']) == 47 and _widest(cn.ND['cnd_largest_middle']) == _widest(cn.ND['cnd_largest_forward_only']) == 3
    assert _widest(cn.ND['cnd_refused']) == 3 and _widest(cn.ND['cnd_refused_radius']) == 48


@pytest.mark.parametrize('case', sorted(ALL))
def test_cases_sit_where_they_are_meant_to(case):
    c = ALL[case]
    walks = _walks(c['tm'])
    n_sum = sum(v[3] for _, v in c['om'][1])
    G = _cells(c)
    fits = cn.lds_doubles(G, _widest(c) if walks else 0, len(walks), n_sum) <= cn.LDS_LIMIT
    if c.get('opts', {}).get('chain_nd') == 2 or case in cn.FORCED or case in cn.BELOW:
        assert fits == (c.get('variant', cn.VARIANT) == cn.VARIANT)          # chain_nd = 2: wherever it fits
    else:                                                                    # the default option: the floor (all of these have 16 or more chains) and the cost model
        radii = [max(cn.radius(s, cn.lattice(c['om'], w[3])) for s in np.atleast_1d(w[2])) for w in walks]
        beyond = any(r > dict(c['om'][1])[w[3]][3] for r, w in zip(radii, walks))         # a radius beyond its axis: the plain path by default
        W, on = sum(2 * r + 1 for r in radii if r), sum(1 for r in radii if r)
        if len(cases.make_data(c['data'])) == 1:                                 # a single step: no transition is applied, no walk has a kernel
            W, on = 0, 0
        threads = 256 if cn.lds_doubles(G, _widest(c) if walks else 0, len(walks), n_sum) * 8 <= 32 * 1024 else 1024
        k, p = _model(G, 35 if case == 'cnd_split' else cn.MIN_CHAINS, on, W, threads)
        assert (fits and 1.25 * k <= p and not beyond) == (c.get('variant', cn.VARIANT) == cn.VARIANT), (k, p, beyond)
        assert not 0.9 < 1.25 * k / p < 1.1, 'a case on the edge of the cost model: %r' % ((k, p),)
    if case.startswith(('cnd_largest', 'cnd_refused_radius')):
        assert _cells(c) == 9408 and n_sum == 167
    if case == 'cnd_largest':
        assert cn.lds_doubles(9408, 47, 2, 167) == cn.LDS_LIMIT - 1
    if case == 'cnd_refused':
        assert _cells(c) == 9472 and cn.lds_doubles(9408 + 64, 3, 2, 168) > cn.LDS_LIMIT >= cn.lds_doubles(9408, 3, 2, 167)


@pytest.mark.parametrize('case', sorted(ALL))
def test_oracle_fits_the_case(case):
    c = ALL[case]
    with np.errstate(all='ignore'):
        r = oa.run(c)
    assert np.isfinite(r['logEvidence'])
    if c['study'] != 'Study':
        n = len(np.asarray(r['logEvidenceList']))
        assert n == (cn.MIN_CHAINS - 1 if case in cn.BELOW else 35 if case == 'cnd_split' else cn.MIN_CHAINS)
    nan = np.isnan(np.asarray(r['localEvidence'], dtype=float))
    if case == 'cnd_dead_chain':
        le = np.asarray(r['logEvidenceList'], dtype=float)
        assert np.isneginf(le[0]) and np.all(np.isfinite(le[1:])) and nan.tolist() == [False, False, True, False, False]
    else:
        assert not nan.any()


@pytest.mark.parametrize('case', cn.GOLDEN)
def test_oracle_matches_the_references_fixture(case):
    with np.errstate(all='ignore'):
        got = oa.run(cn.ND[case])
    compare.check(got, oa.load_golden(case), compare.ORACLE_TOL)
