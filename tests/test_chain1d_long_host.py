"""
The long-row flavour of the chain-resident 1-D kernel (bayesloop_amd/csrc/blhip_chain1d.hpp: bl1c::chain1d_long_kernel, rows of 4097 ..
8192 grid points), the part a CPU can check:

* the lean LDS layout bl1c::lds_doubles_long -- 2 n + 5 LW + 113 doubles for walks and clamps, 3 n + 6 LW + 433 with the shift flavour's
  coefficient row -- and the envelope it gives under the selector's 150 KB (19 200 doubles), through the stand-alone program
  tests/host/chain1d_lds_main.cpp;
* the inputs of tests/test_chain1d_long.py: the oracle fits every one of them without a warning of its own and to finite results, the
  walks have the radii the cases are named after, the Deterministic steps shift by the number of cells that selects the intended form.
"""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import cases
import chain1d_long_cases as clc
import oracle_adapter as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 150 * 1024 // 8           # doubles of LDS the selector allows a block (plan_geometry, blhip_batch.hpp)


@pytest.fixture(scope='module')
def lds_program(tmp_path_factory):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    exe = str(tmp_path_factory.mktemp('chain1d_lds') / 'chain1d_lds')
    subprocess.run([hipcc, '-std=c++17', '--offload-arch=gfx950', os.path.join(ROOT, 'tests', 'host', 'chain1d_lds_main.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=300)

    def run(*triples):
        args = [str(int(v)) for t in triples for v in t]
        lines = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
        consts = dict(zip(lines[0].split()[0::2], map(int, lines[0].split()[1::2])))
        return consts, [tuple(int(v) for v in l.split()) for l in lines[1:]]
    return run


def test_constants_of_the_envelope(lds_program):
    consts, _ = lds_program()
    assert consts == dict(NT=512, NMAX=4096, NMAX_LONG=8192, CPT_LONG=16)


@pytest.mark.parametrize('n,lw', [(4097, 0), (4097, 130), (4500, 21), (5001, 0), (8192, 536), (8192, 540), (7777, 1)])
def test_lean_layout_of_walks_and_clamps(lds_program, n, lw):
    _, rows = lds_program((n, lw, 0))
    assert rows[0][:3] == (n, lw, 0)
    assert rows[0][4] == 2 * n + 5 * lw + 113
    assert rows[0][3] == rows[0][4] + 2 * n            # the standard layout: + the grid values and exp(-lambda)


@pytest.mark.parametrize('n,lw', [(4097, 1), (5000, 7), (5000, 46), (6163, 46), (8000, 12)])
def test_lean_layout_with_the_shift_flavours_coefficient_row(lds_program, n, lw):
    _, rows = lds_program((n, lw, 1))
    assert rows[0][4] == 3 * n + 6 * lw + 433
    assert rows[0][3] == rows[0][4] + 2 * n


def test_envelope_edges(lds_program):
    _, rows = lds_program((8192, 540, 0), (8192, 541, 0), (6163, 46, 1), (6164, 46, 1))
    fits = [r[4] <= LIMIT for r in rows]
    assert fits == [True, False, True, False], rows


def test_the_gpu_cases_sit_where_they_are_meant_to(lds_program):
    """radius 536 on 8192 cells fits, 541 does not; the two-stage shift fits at 5000 cells and not at 6200"""
    _, rows = lds_program((8192, 536, 0), (8192, 541, 0), (5000, 46, 1), (6200, 46, 1), (4500, 31, 1))
    assert [r[4] <= LIMIT for r in rows] == [True, False, True, False, True], rows


def _radius(sigma, lattice):
    return int(4.0 * sigma / lattice + 0.5)          # transitionModels.py:108-111


def test_walk_radii_of_the_cases():
    assert [_radius(s, clc.GM_LATTICE(4097)) for s in clc.W4097] == [0, 3, 17, 64, 130]
    assert [_radius(s, clc.PO_LATTICE(8192)) for s in clc.LONG['walks_poisson8192']['tm'][2]] == [40, 536]
    assert [_radius(s, clc.PO_LATTICE(8192)) for s in clc.EDGE['edge_radius541']['tm'][2]] == [12, 541]


def test_shifts_of_the_cases_select_the_intended_form():
    """cells per step: at most 12 -> the asymmetric stencil, more -> the two-stage form"""
    slow, fast = cases.FUNCS['c1l_slow'](1.0), cases.FUNCS['c1l_fast'](1.0)
    assert 1.0 < slow / clc.GM_LATTICE(5000) < 12.0
    assert 12.0 < fast / clc.GM_LATTICE(5000) < 35.0
    assert 12.0 < fast / clc.GM_LATTICE(6200) < 35.0


ALL = dict(clc.LONG, **clc.EDGE)


@pytest.mark.parametrize('case', sorted(ALL))
def test_oracle_fits_the_case_without_warnings(case):
    c = ALL[case]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        r = oa.run(c)
    assert np.isfinite(r['logEvidence'])
    assert np.all(np.isfinite(np.asarray(r['localEvidence'], dtype=float)))
    if not c.get('fit', {}).get('evidenceOnly', False):
        post = np.asarray(r['posteriorSequence'], dtype=float)
        n = c['om'][1][0][1][3]
        assert post.shape[-1] == n and np.all(np.isfinite(post))
        np.testing.assert_allclose(post.sum(axis=-1), 1.0, rtol=1e-9)
