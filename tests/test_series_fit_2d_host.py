"""
Study.fitMany on two-parameter grids without a GPU: the admission rules and the memory plan of the series path (blhip_host_series_check /
_plan through ctypes: host-only, no context) for the grids, models and transition programs the chain-resident kernels take, and the two
planning rules a series batch depends on -- no shared prefix, route or fail -- through a stand-alone host program around
blhip_chain_plan.hpp (tests/host/series_route_main.cpp).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from bayesloop_amd import _abi
from test_series_fit_host import check, plan, problem

GRW0, GRW1 = (_abi.OP_GRW, 0), (_abi.OP_GRW, 1)
WORD = 'grid of 2 parameters'


# ---- blhip_host_series_check --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [
    dict(n=(128, 16), om=_abi.OM_GAUSSIAN),
    dict(n=(33, 32), om=_abi.OM_GAUSSIAN),
    dict(n=(1024, 1024), om=_abi.OM_GAUSSIAN, data_dim=4),
    dict(n=(100, 37), om=_abi.OM_LAPLACE),
    dict(n=(128, 16), om=_abi.OM_SCALED_AR1, seg_len=2),
    dict(n=(128, 16), om=_abi.OM_AR1, seg_len=2),
    dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=((_abi.OP_STATIC, 0),)),
    dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=((_abi.OP_STATIC, 0), (_abi.OP_CHANGEPOINT, 0))),
    dict(n=(40, 36), om=_abi.OM_GAUSSIAN, ops=(GRW0, GRW1)),
])
def test_check_admits_the_chain_resident_envelope(kw):
    p, keep = problem(**kw)
    assert check(p) == (0, '')
    assert check(p, flags=_abi.FORWARD_ONLY | _abi.KEEP_POSTERIOR) == (0, '')
    assert check(p, flags=_abi.EVIDENCE_ONLY) == (0, '')


@pytest.mark.parametrize('kw, flags, word', [
    (dict(n=(20, 30), om=_abi.OM_GAUSSIAN), 0, '20 rows'),
    (dict(n=(1025, 16), om=_abi.OM_GAUSSIAN), 0, '1025 rows'),
    (dict(n=(128, 1025), om=_abi.OM_GAUSSIAN), 0, '1025 columns'),
    (dict(n=(600, 16), om=_abi.OM_LAPLACE), 0, '600 rows'),
    (dict(n=(300, 16), om=_abi.OM_LAPLACE), 0, 'padded'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN), _abi.SERIES_RAGGED, 'different lengths'),
    (dict(n=(600, 40), om=_abi.OM_GAUSSIAN), 0, 'padded inside 1024 rows'),
    (dict(n=(1024, 40), om=_abi.OM_GAUSSIAN), _abi.KEEP_POSTERIOR, 'padded inside 1024 rows'),
    (dict(n=(128, 16), om=_abi.OM_LAPLACE), _abi.SERIES_RAGGED | _abi.EVIDENCE_ONLY, 'different lengths'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=(GRW0, (_abi.OP_REGIMESWITCH, 0))), 0, 'RegimeSwitch'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=((_abi.OP_NOTEQUAL, 0),)), 0, 'NotEqual'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=((_abi.OP_ALPHASTABLE, 0), (_abi.OP_ALPHASTABLE_ARG, 0))), 0, 'op 0'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=((_abi.OP_DETERMINISTIC, 0), (_abi.OP_DETERMINISTIC_ARG, 0))), 0, 'op 0'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN, ops=((_abi.OP_BIVARIATE, 0), (_abi.OP_BIVARIATE_ARG, 0), (_abi.OP_BIVARIATE_ARG, 0))), 0, 'op 0'),
    (dict(n=(128, 128), om=_abi.OM_SCALED_AR1, seg_len=2, ops=(GRW0, GRW1)), 0, 'walks on both parameters'),
    (dict(n=(600, 40), om=_abi.OM_GAUSSIAN, ops=(GRW0, GRW1)), 0, 'walks on both parameters'),
    (dict(n=(128, 16), om=_abi.OM_TABLE, lik=True), 0, 'observation model 100'),
    (dict(n=(128, 16), om=_abi.OM_PROGRAM), 0, 'observation model 9'),
    (dict(n=(128, 16), om=_abi.OM_GAUSSIAN, data_dim=5), 0, 'data dimension 5'),
])
def test_check_refuses_with_a_reason_that_names_the_grid(kw, flags, word):
    p, keep = problem(**kw)
    rc, why = check(p, flags=flags)
    assert rc == 1 and WORD in why and word in why, (rc, why)


def test_padded_tall_grids_are_admitted_without_a_backward_pass():
    for n in ((600, 40), (1024, 40), (513, 16)):
        p, keep = problem(n=n, om=_abi.OM_GAUSSIAN)
        assert check(p, flags=_abi.EVIDENCE_ONLY) == (0, '') and check(p, flags=_abi.FORWARD_ONLY | _abi.KEEP_POSTERIOR) == (0, '')
        assert check(p)[0] == 1
    p, keep = problem(n=(1024, 48), om=_abi.OM_GAUSSIAN)
    assert check(p) == (0, '')


def test_flags_are_refused_as_on_one_parameter_grids():
    """a guard against regression, not coverage of the feature: these refusals were there before two-parameter grids were admitted"""
    p, keep = problem(n=(128, 16), om=_abi.OM_GAUSSIAN)
    for flag, word in ((_abi.RESUME, 'BLHIP_RESUME'), (_abi.CARRY | _abi.EVIDENCE_ONLY, 'BLHIP_CARRY'), (_abi.ACCUMULATE, 'BLHIP_ACCUMULATE')):
        rc, why = check(p, flags=flag)
        assert rc == 1 and word in why
    p3, keep3 = problem(n=(32, 32, 4), om=_abi.OM_TABLE, lik=True)
    rc, why = check(p3)
    assert rc == 1 and 'grid of 3 parameters' in why


# ---- blhip_host_series_plan: the byte formula, restated ----------------------------------------------------------------------------------
NRED, NW, WCOL = 7, 8, 16


def chain_bytes(n0, n1, T, om, seg_len, data_dim, both, evidence_only):
    """one chain of a series batch on a two-parameter grid (blhip_series.hpp: series_chain_bytes)"""
    if both:
        m = max(n0, n1)
        n0p = n1p = 128 if m <= 128 else (256 if m <= 256 else 512)
    else:
        n0p = 1024 if n0 > 512 else (n0 + 127) // 128 * 128
        n1p = (n1 + WCOL - 1) // WCOL * WCOL
    Gk, G, strips = n0p * n1p, n0 * n1, n1p // WCOL
    pad = (n0p, n1p) != (n0, n1)
    nbytes = (2 if evidence_only else T + 2) * Gk * 8 + T * NRED * 8 * 2 * 64      # state ping-pong + stored sequence, partial sums
    if (pad or both) and not evidence_only:
        nbytes += T * G * 8                                                        # the de-padding copy
    nbytes += T * seg_len * data_dim * 8                                           # the chain's data
    if om == _abi.OM_GAUSSIAN:
        if not both:
            nbytes += T * NW * strips * 64 * 32                                    # its anchors
    else:
        nbytes += T * G * 8                                                        # its likelihood table
    return nbytes


@pytest.mark.parametrize('n, om, seg, dd, ops', [
    ((128, 16), _abi.OM_GAUSSIAN, 1, 1, (GRW0,)),
    ((33, 32), _abi.OM_GAUSSIAN, 1, 2, (GRW0,)),
    ((1024, 48), _abi.OM_GAUSSIAN, 1, 1, ((_abi.OP_STATIC, 0),)),
    ((40, 36), _abi.OM_GAUSSIAN, 1, 1, (GRW0, GRW1)),
    ((200, 200), _abi.OM_GAUSSIAN, 1, 1, (GRW0, GRW1)),
    ((100, 37), _abi.OM_LAPLACE, 1, 1, (GRW0,)),
    ((128, 16), _abi.OM_SCALED_AR1, 2, 1, (GRW0,)),
])
@pytest.mark.parametrize('flags', [0, _abi.EVIDENCE_ONLY])
def test_plan_equals_the_byte_formula_and_is_monotone_in_the_budget(n, om, seg, dd, ops, flags):
    T = 11
    p, keep = problem(n=n, om=om, T=T, seg_len=seg, data_dim=dd, ops=ops)
    least = chain_bytes(n[0], n[1], T, om, seg, dd, len(ops) == 2, bool(flags))
    rc, (per, batches, nbytes, least1) = plan(p, 1, flags, 1e15)
    assert rc == 0 and (per, batches) == (1, 1) and nbytes == least1 == least
    for S in (1, 2, 7, 15, 16, 17, 100, 1024, 1025, 5000):
        last = 0
        for budget in (least, 3 * least + 5, 15 * least, 16 * least, 21 * least, 64 * least, 1e15):
            rc, (per, batches, nbytes, least2) = plan(p, S, flags, budget)
            assert rc == 0 and least2 == least
            fit = int(budget // least)
            if fit >= 16:
                fit -= fit % 8                                         # (whole launches: plan_batches cuts batches of >= 16 chains to a multiple of 8)
            assert per == min(S, 1024, fit) and nbytes == per * least and nbytes <= budget
            assert batches == -(-S // per) and (batches - 1) * per < S
            assert per >= last                                         # monotone in the budget
            last = per
    rc, out = plan(p, 5, flags, least - 1)
    assert rc == 1 and out[3] == least and out[0] == 0
    assert plan(p, 5, flags | _abi.SERIES_RAGGED, 1e15)[0] == -1
    assert plan(p, 5, flags | _abi.ACCUMULATE, 1e15)[0] == -1


# ---- the planning rules of a series batch (blhip_chain_plan.hpp), on the CPU ----------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def route_program(tmp_path_factory):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    exe = str(tmp_path_factory.mktemp('series_route') / 'series_route')
    src = os.path.join(ROOT, 'tests', 'host', 'series_route_main.cpp')
    subprocess.run([hipcc, '-std=c++17', '--offload-arch=gfx950', src, '-o', exe], check=True, capture_output=True, text=True, timeout=300)
    return exe


def test_series_batches_share_no_prefix_and_route_or_fail(route_program):
    out = subprocess.run([route_program], check=True, capture_output=True, text=True).stdout
    lines = dict(line.split(': ', 1) for line in out.strip().splitlines())
    # three change-point chains with the restart at step 3 of 6: a hyper-study skips 3 steps in two of them (evidence-only) -- series none
    assert lines['prefix hyper evidence_only'] == 'share 1 skip 1 saved 6'
    assert lines['prefix series evidence_only'] == 'share 0 skip 0 saved 0'
    assert lines['prefix hyper fused'] == 'share 1 skip 1 saved 6'
    assert lines['prefix series fused'] == 'share 0 skip 0 saved 0'
    # route or fail: only a batch on blc::chain_kernel / blc::chainax_kernel whose passes went through runs
    assert lines['route series 2d chain'] == 'runs'
    assert lines['route series 2d declined'].startswith('fails: the chain-resident kernels do not take')
    assert lines['route series 2d clamp'].startswith('fails: ')
    assert lines['route series 2d repeat'].startswith('fails: a chain-resident pass')
    assert lines['route series 1d declined'] == 'runs'                # (one-parameter grids: Row1dRun's own rule)
    assert lines['route fit 2d declined'] == 'runs' and lines['route fit 2d repeat'] == 'runs'
