"""
The chain-resident 1-D kernel on rows of 4097 .. 8192 grid points (bayesloop_amd/csrc/blhip_chain1d.hpp: bl1c::chain1d_long_kernel<BWD, M, CL>;
selector: plan_geometry, blhip_batch.hpp; launcher: launch_chain1d_long, blhip_launch.hpp), on the GPU.  Cases: tests/chain1d_long_cases.py.

Every case is fitted, the kernels it launched are read from the library's registry (blhip_kernel_census) and everything it produced is
compared with the CPU oracle at compare.GPU_TOL (log-evidence 1e-9 relative, posteriors |dp| <= 1e-12 + 1e-9 p); cases with a Deterministic
model carry the registered cases.FFT_TOL -- tests/test_kernel_sweep.py: run.  Together the cases launch the eight instantiations of the
long-row kernel: (M, CL) = (2, 0) walks and restarts, (1, 1) spline shifts, (1, 2) shifts and clamps, (2, 2) clamps without a shift, forward
and backward.

Batches of walks and restarts are given to the kernel by the selector's cost model, which leaves a few chains of some thousand cells on
the kernels that spread a row over many compute units (profiles/chain1d_long_notes.md); the cases here have a few chains, so those run
with option chain1d = 2 ("wherever it fits").  Programs with clamps or shifts take the kernel by default, as on shorter rows.
"""
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import chain1d_long_cases as clc
import compare
from conftest import kernel_census
from test_gpu_parity import result_of
from test_kernel_sweep import run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LONG = 'bl1c::chain1d_long_kernel<%s, %d, %d>'
DEFAULTS = dict(chain1d=1, chain1d_long=1)


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


class options:
    """Engine options for the duration of a block (the library's defaults afterwards)."""
    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        for k, v in self.opts.items():
            bl.get_engine().set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            bl.get_engine().set_option(k, DEFAULTS[k])


def both(m, cl):
    return [LONG % ('false', m, cl), LONG % ('true', m, cl)]


def variants(S):
    return S.lastTiming['fwd_kernel_variant'], S.lastTiming['bwd_kernel_variant']


def launched(fn):
    """-> (result of fn, names of the kernels launched meanwhile)"""
    before = {n: c for c, n in kernel_census()}
    out = fn()
    after = {n: c for c, n in kernel_census()}
    return out, sorted(k for k in after if after[k] > before.get(k, 0))


# ---- walks and restarts: (M, CL) = (2, 0) -----------------------------------------------------------------------------------------------

def test_walks_on_4097_cells_full_fit():
    """the first long row, an odd length; five widths including 0 share ONE likelihood table"""
    with options(chain1d=2):
        S = run(clc.LONG['walks_gm4097'], both(2, 0) + ['bl1c::lik1d_table_kernel<3>'])
    assert variants(S) == (9, 9), S.lastTiming


def test_walks_on_4097_cells_forward_only():
    with options(chain1d=2):
        S = run(clc.LONG['walks_gm4097_forward'], [LONG % ('false', 2, 0), 'bl1c::lik1d_table_kernel<3>'])
    assert S.lastTiming['fwd_kernel_variant'] == 9, S.lastTiming


def test_walks_on_4097_cells_evidence_only():
    with options(chain1d=2):
        S = run(clc.LONG['walks_gm4097_evidence'], [LONG % ('false', 2, 0), 'bl1c::lik1d_table_kernel<3>'])
    assert S.lastTiming['fwd_kernel_variant'] == 9, S.lastTiming


def test_two_poisson_chains_on_8192_cells_near_the_lds_edge():
    """fewer than four chains: the table is built all the same (the long-row kernel has no likelihood of its own); radius 536 of 540"""
    with options(chain1d=2):
        S = run(clc.LONG['walks_poisson8192'], both(2, 0) + ['bl1c::lik1d_table_kernel<1>'])
    assert variants(S) == (9, 9), S.lastTiming


def test_restarts_on_5001_cells():
    """a tabulated model (the caller's table is used as it is), change points at six candidate times"""
    with options(chain1d=2):
        S = run(clc.LONG['restarts_bernoulli5001'], both(2, 0))
        assert variants(S) == (9, 9), S.lastTiming
        S = run(clc.LONG['restarts_bernoulli5001_evidence'], [LONG % ('false', 2, 0)])
        assert S.lastTiming['fwd_kernel_variant'] == 9, S.lastTiming


# ---- clamps without a shift: (M, CL) = (2, 2), by default ---------------------------------------------------------------------------------

@pytest.mark.parametrize('model', sorted(clc.CLAMP_STUDY))
def test_clamps_on_4500_cells_one_chain(model):
    S = run(clc.LONG['clamp_study_' + model], both(2, 2))
    assert variants(S) == (9, 9), S.lastTiming


@pytest.mark.parametrize('model', sorted(clc.CLAMP_HYPER))
def test_clamps_on_4500_cells_six_chains(model):
    S = run(clc.LONG['clamp_hyper_' + model], both(2, 2))
    assert variants(S) == (9, 9), S.lastTiming


# ---- spline shifts: (M, CL) = (1, 1), with a clamp (1, 2), by default ----------------------------------------------------------------------

@pytest.mark.parametrize('case', ['shift_slow5000', 'shift_fast5000'])
def test_shifts_on_5000_cells(case):
    """5 cells per step: the asymmetric stencil; 19 cells per step: the two-stage form"""
    c = clc.LONG[case]
    S = run(c, both(1, 1), tol=c['tol'])
    assert variants(S) == (9, 9), S.lastTiming


def test_shift_with_a_clamp_on_5000_cells():
    c = clc.LONG['shift_clamp5000']
    S = run(c, both(1, 2), tol=c['tol'])
    assert variants(S) == (9, 9), S.lastTiming


# ---- the edges of the envelope -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', sorted(clc.EDGE))
def test_beyond_the_envelope_the_old_paths_run(case):
    """radius 541 on 8192 cells, 8193 cells, a two-stage shift on 6200 cells: not chain-resident even when forced, and right"""
    c = clc.EDGE[case]
    with options(chain1d=2):
        (S, ran) = launched(lambda: run(c, [], tol=c.get('tol')))
    assert 9 not in variants(S), S.lastTiming
    assert not [k for k in ran if k.startswith('bl1c::chain1d')], ran


# ---- the option ------------------------------------------------------------------------------------------------------------------------------

def _fit(c):
    S = cases.build(bl, c)
    S.fit(**cases.fit_kwargs(c))
    return S, result_of(S, c)


KEYS = ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'logEvidenceList', 'hyperParameterDistribution')


def test_option_chain1d_long_switches_the_flavour():
    """A six-chain (width, pMin) study on 4500 cells takes the long-row kernel by default; with chain1d_long = 0 it keeps the launch-per-step
    kernel it had, and the two results agree at the parity bar."""
    c = clc.LONG['clamp_hyper_walk_then_switch']
    (S1, got1), ran1 = launched(lambda: _fit(c))
    assert variants(S1) == (9, 9), S1.lastTiming
    assert LONG % ('false', 2, 2) in ran1 and LONG % ('true', 2, 2) in ran1, ran1
    with options(chain1d_long=0):
        (S0, got0), ran0 = launched(lambda: _fit(c))
    assert 9 not in variants(S0), S0.lastTiming
    assert not [k for k in ran0 if k.startswith('bl1c::chain1d')], ran0
    compare.check({k: got1[k] for k in KEYS if k in got1}, {k: got0[k] for k in KEYS if k in got0}, compare.GPU_TOL)


def test_option_chain1d_long_on_the_4097_cell_walks():
    """... and the five walks on 4097 cells: chain-resident where the kernel is asked for wherever it fits (chain1d = 2), not with
    chain1d_long = 0 beside it, not with chain1d = 0; the same results at the parity bar."""
    c = clc.LONG['walks_gm4097']
    with options(chain1d=2):
        S2, got2 = _fit(c)
        assert variants(S2) == (9, 9), S2.lastTiming
        with options(chain1d_long=0):
            S0, got0 = _fit(c)
        assert 9 not in variants(S0), S0.lastTiming
    with options(chain1d=0):
        S00, _ = _fit(c)
    assert 9 not in variants(S00), S00.lastTiming
    compare.check({k: got2[k] for k in KEYS if k in got2}, {k: got0[k] for k in KEYS if k in got0}, compare.GPU_TOL)


# ---- nothing moved below 4097 cells ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', sorted(clc.PARENT))
def test_shorter_rows_are_bit_identical_to_the_parent_commit(case):
    """tests/golden/chain1d_parent_results.npz: the results of these shapes from a build of the commit before the long-row flavour, on the
    same hardware -- one each of CL = 0 (one and two cells per thread), 1 and 2.  The kernel body both flavours share compiles to the same
    arithmetic for the instantiations that existed, and the selector decides rows of at most 4096 cells as it did."""
    parent = np.load(os.path.join(HERE, 'golden', 'chain1d_parent_results.npz'))
    c = clc.PARENT[case]

    def fit():
        S = cases.build(bl, c)
        S.fit(**cases.fit_kwargs(c))
        return S, clc.parent_results(S)
    (S, got), ran = launched(fit)
    k = clc.PARENT_KERNELS[case]
    assert k % 'false' in ran and k % 'true' in ran, ran
    keys = [key.split('/', 1)[1] for key in parent.files if key.startswith(case + '/')]
    assert sorted(keys) == sorted(got) and 'posteriorSequence' in keys
    for key in keys:
        assert np.array_equal(got[key], parent['%s/%s' % (case, key)]), key
