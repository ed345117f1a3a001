"""
The route of a batch through the chain-resident kernels of two-parameter grids (bayesloop_amd/csrc/blhip_chain_plan.hpp), the part of
ChainRun::setup / ::pass (blhip_fit_paths.hpp) that needs no GPU: the geometry and the rounds (plan_chainres), the clamp kernels' route, whether
the backward pass folds, what a padded batch does, the shared prefix of change-point chains, the memory admission and what a launch moves.
The stand-alone program tests/host/chain_plan_main.cpp builds a batch from its command line (a tiny time axis, one tap set per radius)
and prints every stage; the expectations below are written out by hand from the rules:

* geometry: rows rounded up to 128 / 256 / 384 / 512, beyond 512 to 1024; columns to a multiple of 16, one strip per 16 columns, at most 64
  strips and at most one per compute unit; a wave works on rows / 128 product tiles (ntw); a launch holds cus / strips chains (cpr);
* rounds: chains sorted by radius, cpr per launch, ring length (16 + 2 r) / 4 with r the launch's widest radius rounded up to 4 (at least 4),
  4 for a batch without any stencil; both axes: a square geometry of 128 / 256 / 512, r rounded up to 8;
* RegimeSwitch (blhip_chainclamp_plan.hpp): 384 rows run inside 512, ring lengths rounded up to 4, 8, 12 .. 24, no restarts, at least 8
  pass-steps (steps x passes);
* fold: a full accumulating fit that keeps nothing owns its sequence (an even number of cells unless padded); it folds in the backward
  kernel unless a filtering chain restarts; two chains per block on <= 512 rows with the Gaussian recurrence (restarts: only where backward
  step t restarts exactly when forward step t + 1 does); without that kernel the Gaussian model folds in the kernel on 1024 rows only, the
  table on exact grids only;
* a padded batch whose sequence is not private copies it out afterwards (depad) if memory admits and, for a full fit, on <= 512 rows;
* prefix: without a stencil, the chain with the latest first restart provides the steps before the others' first restarts;
* the layout the separate fold reads (chain_fold_source): strip-major or padded only when the chain kernels ran; a batch that was planned and
  then declined, or repeated on the launch-per-step kernels, reads row-major (tests/DECLINED_BATCHES.md; the studies: test_declined_batches.py).

Built plain and with -fsanitize=address,undefined (host code only; the program has its own main).
"""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import declined_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'chain_plan_main.cpp')
CSRC = os.path.join(ROOT, 'bayesloop_amd', 'csrc')


def _hipcc():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    return hipcc


def _args(chains=(), **kw):
    """(a list as value: the key once per element)"""
    return ['chain=%s' % c for c in chains] + ['%s=%s' % (k, x) for k, v in kw.items() for x in (v if isinstance(v, list) else [v])]


def _parse(out):
    """'name k v k v ..' lines -> dict of ints; 'name v v ..' lines -> list of ints; 'plan refused' -> r['plan'] = None"""
    r = {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == 'plan' and w[1] == 'refused':
            r['plan'] = None
        elif w[0] in ('admit', 'plan', 'route', 'fold_plan', 'fold', 'fold_source', 'prefix'):
            r[w[0]] = dict(zip(w[1::2], map(int, w[2::2])))
        elif w[0] == 'source':
            r.setdefault('source', []).append(tuple(int(x) for x in w[1:]))
        elif w[0] == 'cost':
            r.setdefault('cost', []).append((float(w[1]), float(w[2])))
        elif w[0] == 'admits':
            r.setdefault('admits', []).append(int(w[1]))
        elif w[0] == 'constants':
            r['constants'] = w[1:]
        else:
            r[w[0]] = [int(x) for x in w[1:]]
    return r


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('chain_plan') / 'chain_plan')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)

    def run(chains=(), **kw):
        return _parse(subprocess.run([exe] + _args(chains, **kw), check=True, capture_output=True, text=True, timeout=120).stdout)
    return run


HYPER = dict(accumulate=1, full=1)                 # a hyper- / change-point study's full fit: the posteriors go into the average only


def test_the_stand_ins_of_the_launch_tables_are_the_librarys(plan):
    """FAST_R0_MAX and fold2_shape live in blhip_launch.hpp, which a stand-alone program cannot include (every kernel family)"""
    c = plan()['constants']
    text = open(os.path.join(CSRC, 'blhip_launch.hpp')).read()
    assert int(c[c.index('FAST_R0_MAX') + 1]) == int(re.search(r'constexpr int FAST_R0_MAX = (\d+);', text).group(1))
    lo, hi = map(int, re.search(r'bool fold2_shape\(int ntw\) \{ return ntw >= (\d+) && ntw <= (\d+); \}', text).groups())
    k = c.index('fold2_shape')
    assert [int(x) for x in c[k + 1:k + 10]] == [1 if lo <= ntw <= hi else 0 for ntw in range(9)]
    assert c[c.index('CHAIN_R0_MAX') + 1] == '80' and c[c.index('MAXLAG') + 1] == '4'


def test_geometry(plan):
    r = plan(['3'], n0=100, n1=20)
    assert r['admit'] == dict(gauss=1, tab=0, may_ax1=0, clamp_try=0, plan=1, r0_max=80, allow_ax1=0)
    assert r['plan'] == dict(n0p=128, n1p=32, pad=1, strips=2, ntw=1, cpr=128, ax1=0, has_reset=0, mixed=0)
    r = plan(['3'], n0=384, n1=16)
    assert r['plan'] == dict(n0p=384, n1p=16, pad=0, strips=1, ntw=3, cpr=256, ax1=0, has_reset=0, mixed=0)
    r = plan(['3'], n0=600, n1=16)
    assert r['plan'] == dict(n0p=1024, n1p=16, pad=1, strips=1, ntw=8, cpr=256, ax1=0, has_reset=0, mixed=0)
    for grid in (dict(n0=20, n1=16), dict(n0=128, n1=1040), dict(n0=128, n1=64, cus=2), dict(n0=1025, n1=16)):
        r = plan(['3'], **grid)
        assert r['admit']['plan'] == 1 and r['plan'] is None and r['route']['on'] == 0, grid
    assert plan(['3'], n0=128, n1=1024)['plan']['strips'] == 64            # 64 strips: the most
    assert plan(['3'], n0=128, n1=64, cus=4)['plan']['cpr'] == 1


def test_admit(plan):
    """what keeps a batch off the path before any planning"""
    for kw in (dict(chain_resident=0), dict(resident_ok=0), dict(allow_chainres=0), dict(resume=1), dict(carry=1), dict(backward_init=1),
               dict(om='table', chain_table=0)):
        assert plan(['3'], **kw)['admit']['plan'] == 0, kw
    r = plan(['3'], om='table')
    assert r['admit'] == dict(gauss=0, tab=1, may_ax1=0, clamp_try=0, plan=1, r0_max=40, allow_ax1=0)      # the table kernels: radius <= 40


def test_rounds(plan):
    r = plan(['3', '2', '1'])
    assert r['order'] == [2, 1, 0] and r['round_start'] == [0, 3] and r['round_nk'] == [(16 + 2 * 4) // 4] == [6]
    assert r['tap_lw'] == [3, 2, 1] and r['tap_id'] == [0, 1, 2] and r['tap_id1'] == [-1, -1, -1]
    assert plan(['0', '0', '0'])['round_nk'] == [4]                         # no stencil at all
    r = plan(['3', '3', '3'], cus=2)                                         # one strip: two chains per launch
    assert r['plan']['cpr'] == 2 and r['round_start'] == [0, 2, 3] and r['round_nk'] == [6, 6]
    # the launch's widest chain sets the ring: radii 1, 9 | 30 -> rounded 12 | 32
    r = plan(['30', '1', '9'], cus=2)
    assert r['order'] == [1, 2, 0] and r['round_nk'] == [(16 + 24) // 4, (16 + 64) // 4]
    # the two-chain fold kernel's rounds: 2 x cpr chains, one accumulator per block
    r = plan(['3'] * 5, cus=2, **HYPER)
    assert r['round_start'] == [0, 2, 4, 5]
    assert r['fold'] == dict(keep=1, needs_depad=0, depad=0, post_private=1, fused=1, fold2=1, slots_used=min(2, (5 + 1) // 2))
    assert r['round_start_b'] == [0, 4, 5] and r['round_nk_b'] == [6, 6]
    r = plan(['3'] * 3, cus=8, **HYPER)
    assert r['round_start_b'] == [0, 3] and r['fold']['slots_used'] == min(8, (3 + 1) // 2) == 2
    assert plan(['0'] * 3, cus=2, **HYPER)['round_nk_b'] == [4]


def test_radius_limits(plan):
    assert plan(['80'])['round_nk'] == [(16 + 160) // 4] == [44]
    assert plan(['81'])['plan'] is None
    r = plan(['40'], chain_wide=0)
    assert r['admit']['r0_max'] == 40 and r['round_nk'] == [24]
    assert plan(['41'], chain_wide=0)['plan'] is None
    assert plan(['41'], om='table')['plan'] is None                          # the table kernels: radius <= 40 whatever chain_wide says
    assert plan(['32'], n0=32)['plan'] is None and plan(['31'], n0=32)['plan'] is not None      # (single-period reflection: radius < rows)
    assert plan(['3:0:-:=:4/5'])['plan'] is None                            # a second tap set from step 4 on


def test_both_axes(plan):
    r = plan(['3:2'], n0=100, n1=90)
    assert r['admit']['may_ax1'] == 1 and r['admit']['allow_ax1'] == 1
    assert r['plan'] == dict(n0p=128, n1p=128, pad=1, strips=8, ntw=1, cpr=32, ax1=1, has_reset=0, mixed=0)
    assert r['round_nk'] == [(16 + 2 * 8) // 4] == [8] and r['tap_id'] == [0] and r['tap_id1'] == [1]
    assert plan(['20:12'], n0=100, n1=90)['round_nk'] == [(16 + 2 * 24) // 4]          # the wider walk, 20, rounded up to 24
    assert plan(['3:2'], n0=128, n1=128)['plan']['pad'] == 0
    assert plan(['3:2'], n0=200, n1=90)['plan']['n0p'] == 256 and plan(['3:2'], n0=300, n1=90)['plan']['n0p'] == 512
    assert plan(['3:90'], n0=100, n1=90)['plan'] is None                     # radius >= columns
    assert plan(['33:2'], n0=40, n1=40)['plan'] is None                      # 33 rounds up to 40 >= min(rows, columns)
    assert plan(['32:2'], n0=40, n1=40)['plan'] is not None
    assert plan(['41:2'], n0=100, n1=90)['plan'] is None                     # both axes: radius <= 40
    r = plan(['3:2'], n0=100, n1=90, chain_ax1=0)                            # walks on the columns and nothing to run them
    assert r['admit']['may_ax1'] == 0 and r['admit']['plan'] == 0


def test_clamp(plan):
    r = plan(['3'], n0=384, n1=16, clamp=1)
    assert r['admit']['clamp_try'] == 1 and r['admit']['r0_max'] == 40 and r['plan']['ntw'] == 3 and r['plan']['pad'] == 0
    assert r['route'] == dict(on=1, clamp=1, n0p=512, ntw=4, pad=1)
    assert r['round_nk'] == [6] and r['route_nk'] == [8]
    assert plan(['0'], clamp=1)['route_nk'] == [4]
    # one chain per launch: rings (16 + 2 r) / 4 = 6, 10, 14, 18, 24 -> the next multiple of 4
    r = plan(['3', '12', '20', '28', '40'], clamp=1, cus=1)
    assert r['round_nk'] == [6, 10, 14, 18, 24] and r['route_nk'] == [8, 12, 16, 20, 24]
    assert plan(['3', '0:0:4'], clamp=1)['route'] == dict(on=0, clamp=0, n0p=128, ntw=1, pad=0)      # restarts
    assert plan(['3'], clamp=1, chain_clamp=0)['admit'] == dict(gauss=1, tab=0, may_ax1=0, clamp_try=0, plan=0, r0_max=80, allow_ax1=0)
    assert plan(['3'], clamp=1, om='table')['admit']['plan'] == 0
    # pass-steps = steps x passes
    assert plan(['3'], clamp=1, T=7, full=0, evidence_only=1)['route']['on'] == 0
    assert plan(['3'], clamp=1, T=8, full=0, evidence_only=1)['route']['on'] == 1
    assert plan(['3'], clamp=1, T=3, full=1)['route']['on'] == 0 and plan(['3'], clamp=1, T=4, full=1)['route']['on'] == 1
    assert plan(['3'], clamp=1, T=3, full=1, chain_clamp=2)['route']['on'] == 1
    # clamped batches store and fold afterwards
    assert plan(['3'], clamp=1, **HYPER)['fold'] == dict(keep=1, needs_depad=0, depad=0, post_private=1, fused=0, fold2=0, slots_used=1)


def _fold(r):
    return {k: r['fold'][k] for k in ('keep', 'post_private', 'fused', 'fold2')}


def test_fold(plan):
    W = ['3', '2', '1']
    assert _fold(plan(W, **HYPER)) == dict(keep=1, post_private=1, fused=1, fold2=1)
    for kw in (dict(accumulate=0), dict(accumulate=1, keep=1), dict(accumulate=1, acc_aligned=0), dict(accumulate=1, full=0, forward_only=1)):
        assert _fold(plan(W, **kw)) == dict(keep=1, post_private=0, fused=0, fold2=0), kw
    assert _fold(plan(W, fuse_accumulate=0, **HYPER)) == dict(keep=1, post_private=1, fused=0, fold2=0)
    # <= 512 rows, Gaussian, without the two-chain kernel: stored and folded separately
    for kw in (dict(chain_means=1), dict(fold2=0)):
        r = plan(W, **HYPER, **kw)
        assert r['fold_plan']['fused'] == 1 and r['fold_plan']['fold2'] == 0
        assert _fold(r) == dict(keep=1, post_private=1, fused=0, fold2=0), kw
    assert _fold(plan(W, n0=512, fold2=0, **HYPER))['fused'] == 0
    # a table: the one-chain kernel folds on exact grids
    assert _fold(plan(W, om='table', **HYPER)) == dict(keep=1, post_private=1, fused=1, fold2=0)
    assert _fold(plan(W, om='table', n0=100, n1=20, **HYPER)) == dict(keep=1, post_private=1, fused=0, fold2=0)
    assert plan(W, om='table', n0=1024, **HYPER)['route']['on'] == 0            # no table kernel beyond 512 rows
    assert plan(W, om='table', n0=300, n1=20, **HYPER)['route']['on'] == 0      # ... nor on padded 384 rows
    # 1024 rows: the one-chain kernel
    assert _fold(plan(W, n0=1024, **HYPER)) == dict(keep=1, post_private=1, fused=1, fold2=0)
    assert _fold(plan(W, n0=600, **HYPER)) == dict(keep=1, post_private=1, fused=1, fold2=0)
    assert _fold(plan(W, n0=600, fuse_accumulate=0, **HYPER)) == dict(keep=0, post_private=1, fused=0, fold2=0)      # padded, stored: no kernel
    assert _fold(plan(W, n0=1024, fuse_accumulate=0, **HYPER)) == dict(keep=1, post_private=1, fused=0, fold2=0)
    # an odd number of cells: private only on a padded geometry (an exact one has a multiple of 16 columns)
    assert _fold(plan(W, n0=99, n1=17, **HYPER)) == dict(keep=1, post_private=1, fused=1, fold2=1)
    # a restart inside a filtering chain
    r = plan(['3:0:4', '3'], **HYPER)
    assert r['plan']['has_reset'] == 1 and r['plan']['mixed'] == 1
    assert _fold(r) == dict(keep=1, post_private=1, fused=0, fold2=0)


def test_restarts_of_the_two_passes_must_line_up(plan):
    r = plan(['0:0:3', '0:0:5'], **HYPER)                                   # backward restarts at 2 and 4
    assert r['plan']['has_reset'] == 1 and r['plan']['mixed'] == 0 and r['round_nk'] == [4]
    assert _fold(r) == dict(keep=1, post_private=1, fused=1, fold2=1)
    assert _fold(plan(['0:0:3', '0:0:5:5'], **HYPER)) == dict(keep=1, post_private=1, fused=0, fold2=0)      # chain 1 off by one step
    assert _fold(plan(['0:0:3', '0:0:5:-'], **HYPER))['fused'] == 0
    assert _fold(plan(['0:0:3+6', '0:0:5:4'], **HYPER))['fused'] == 1
    for kw in (dict(fold2_cp=0), dict(fold2=0), dict(chain_means=1), dict(n0=1024), dict(om='table')):
        assert _fold(plan(['0:0:3', '0:0:5'], **HYPER, **kw))['fused'] == 0, kw


def test_padding_rule(plan):
    W = ['3', '2']
    base = dict(n0=100, n1=20)
    assert plan(W, **base)['fold'] == dict(keep=1, needs_depad=1, depad=1, post_private=0, fused=0, fold2=0, slots_used=2)
    assert plan(W, admitted=0, **base)['fold']['keep'] == 0 and plan(W, chain_depad=0, **base)['fold']['keep'] == 0
    for kw in (dict(full=0, evidence_only=1), HYPER):                        # private sequences: nothing to copy out
        r = plan(W, **base, **kw)['fold']
        assert (r['keep'], r['needs_depad'], r['depad']) == (1, 0, 0), kw
    assert plan(W, n0=128, n1=16)['fold']['needs_depad'] == 0
    # 1024 rows: forward passes only
    r = plan(W, n0=600, n1=16)['fold']
    assert (r['keep'], r['needs_depad'], r['depad']) == (0, 1, 0)
    r = plan(W, n0=600, n1=16, full=0, forward_only=1)['fold']
    assert (r['keep'], r['needs_depad'], r['depad']) == (1, 1, 1)
    # both axes: never the caller's layout, also on an exact geometry
    r = plan(['3:2'], n0=128, n1=128)['fold']
    assert (r['keep'], r['needs_depad'], r['depad'], r['fused'], r['fold2']) == (1, 1, 1, 0, 0)


def test_prefix_plan(plan):
    r = plan(['0:0:3', '0:0:5', '0:0:2'], T=8, **HYPER)
    assert r['prefix'] == dict(share=1, skip=1, prov=1, saved=5) and r['tfirst'] == [3, 5, 2] and r['tsh'] == [3, 0, 2]
    r = plan(['0:0:4', '0:0:4'], T=8, **HYPER)
    assert r['prefix'] == dict(share=1, skip=1, prov=0, saved=4) and r['tsh'] == [0, 4]
    r = plan(['0:0:3', '0'], T=8, **HYPER)                                   # no restart: counts as T
    assert r['tfirst'] == [3, 8] and r['prefix'] == dict(share=1, skip=1, prov=1, saved=3) and r['tsh'] == [3, 0]
    none = dict(share=0, skip=0, prov=0, saved=0)
    assert plan(['3', '0:0:3'], T=8, **HYPER)['prefix'] == none and _fold(plan(['3', '0:0:3'], T=8, **HYPER))['fused'] == 1      # a stencil in the batch
    assert plan(['0:0:3'], T=8, **HYPER)['prefix'] == none                   # one chain
    assert plan(['0', '0'], T=8, **HYPER)['prefix'] == none                  # no restart at all
    assert plan(['0:0:3', '0:0:5'], T=8, share_prefix=0, skip_prefix=0, **HYPER)['prefix'] == none
    assert plan(['0:0:3', '0:0:5'], T=8, skip_prefix=0, **HYPER)['prefix'] == dict(share=1, skip=0, prov=1, saved=3)
    # evidence-only: nothing is stored, the prefix is skipped -- share_prefix is set all the same
    ev = dict(full=0, evidence_only=1)
    assert plan(['0:0:3', '0:0:5', '0:0:2'], T=8, **ev)['prefix'] == dict(share=1, skip=1, prov=1, saved=5)
    assert plan(['0:0:3', '0:0:5', '0:0:2'], T=8, share_prefix=0, **ev)['prefix'] == dict(share=1, skip=1, prov=1, saved=5)
    assert plan(['0:0:3', '0:0:5', '0:0:2'], T=8, skip_prefix=0, **ev)['prefix'] == none
    # a fit that stores and folds separately shares nothing (the stored states are overwritten)
    assert plan(['0:0:3', '0:0:5'], T=8, fold2_cp=0, **HYPER)['prefix'] == none


def test_admission(plan):
    r = plan(admits='100,0.5,150,50')                                        # need == 0.5 x (150 + 50): refused
    assert r['admits'] == [0]
    assert plan(admits='99.5,0.5,150,50')['admits'] == [1]
    assert plan(admits='100,0.5,150,51')['admits'] == [1] and plan(admits='100,0.5,150,0')['admits'] == [0]      # what the context holds counts
    assert plan(admits='160,0.8,100,100')['admits'] == [0] and plan(admits='159,0.8,100,100')['admits'] == [1]


def _launch(plan, nslots, bwd=0, fold=0, two=0, ax1=0, tab=0, ev=0, nk=6, share=0, skip=0, tsh=(), Gk=2048, T=8):
    v = [nslots, Gk, T, bwd, fold, two, ax1, tab, ev, nk, share, skip] + list(tsh)
    (cost,) = plan(launch=','.join(map(str, v)))['cost']
    return cost                                                             # (bytes, cells computed)


def test_traffic_model(plan):
    Gk, T = 2048, 8
    cells = 3.0 * Gk * T
    assert _launch(plan, 3) == (cells * 8.0, cells)
    assert _launch(plan, 3, ev=1) == (0.0, cells)
    assert _launch(plan, 3, bwd=1) == (cells * 16.0, cells)
    assert _launch(plan, 3, bwd=1, fold=1) == (cells * 24.0, cells)
    for n in (3, 4):
        per_cell = 8.0 + 16.0 * ((n + 1) // 2) / n
        assert _launch(plan, n, bwd=1, fold=1, two=1) == (n * Gk * T * per_cell, float(n * Gk * T))
    assert 8.0 + 16.0 * 2 / 4 == 16.0
    assert _launch(plan, 3, ax1=1, nk=8) == (cells * 24.0, cells) and _launch(plan, 3, bwd=1, ax1=1, nk=8) == (cells * 32.0, cells)
    assert _launch(plan, 3, bwd=1, fold=1, ax1=1, nk=8) == (cells * 40.0, cells) and _launch(plan, 3, ev=1, ax1=1, nk=8) == (cells * 16.0, cells)
    # the table of the pass, once per launch
    assert _launch(plan, 3, tab=1) == (cells * 8.0 + T * Gk * 8.0, cells)
    assert _launch(plan, 3, bwd=1, fold=1, tab=1) == (cells * 24.0 + T * Gk * 8.0, cells)
    # the shared prefix: forward neither computed nor stored; backward read once per launch (by the chain that shares most)
    tsh = (3, 0, 2)
    run = cells - 5.0 * Gk
    assert _launch(plan, 3, share=1, skip=1, tsh=tsh, nk=4) == (run * 8.0 - 5.0 * Gk * 8.0, run)
    assert _launch(plan, 3, share=1, skip=0, tsh=tsh, nk=4) == (cells * 8.0 - 5.0 * Gk * 8.0, cells)
    assert _launch(plan, 3, ev=1, share=1, skip=1, tsh=tsh, nk=4) == (0.0, run)
    assert _launch(plan, 3, bwd=1, fold=1, two=1, share=1, skip=1, tsh=tsh, nk=4) == (cells * (8.0 + 16.0 * 2 / 3) - (5 - 3) * Gk * 8.0, cells)
    assert _launch(plan, 3, bwd=1, share=1, skip=1, tsh=tsh, nk=4) == (cells * 16.0, cells)      # a storing backward pass shares nothing


ROW_MAJOR, STRIP_MAJOR, PADDED = dc.ROW_MAJOR, dc.STRIP_MAJOR, dc.PADDED
ROW_FROM_POST = (ROW_MAJOR, 0, 0)                  # (layout, sm_n0, through depad_kernel): row-major, written into blhip_ctx::post by the passes themselves


def test_fold_source_over_the_whole_product(plan):
    """chain_fold_source, the layout finish_batch hands the separate fold: strip-major or padded ONLY when the chain kernels ran -- a
    declined batch (on = 0, whatever the plan left in the other members: the late declines of chain_fold_settle and chain_padding_rule, and
    the memory admissions of both_axes_buffers, anchor_table and the de-padding copy, which no test can force on the card) and a batch the
    launch-per-step kernels repeated read row-major from blhip_ctx::post."""
    combos = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (100, 128, 520, 601, 1024)))
    got = plan(source=[','.join(map(str, c)) for c in combos])['source']
    assert len(got) == len(combos) == 320
    seen = set()
    for (on, failed, post_private, pad, ax1, depad, n0), s in zip(combos, got):
        what = dict(on=on, failed=failed, post_private=post_private, pad=pad, ax1=ax1, depad=depad, n0=n0)
        if not on or failed:
            assert s == ROW_FROM_POST, what
            continue
        # the chain kernels ran: a de-padded sequence is row-major; else the padded geometry or the both-axes layouts; else the exact
        # geometry, strip-major where the sequence is private to the fit (rows per strip: the grid's), row-major where it is handed out
        want = (ROW_MAJOR, 0, 1) if depad else (PADDED, 0, 0) if (pad or ax1) else (STRIP_MAJOR, n0, 0) if post_private else ROW_FROM_POST
        assert s == want, what
        seen.add(s[0])
    assert seen == {ROW_MAJOR, STRIP_MAJOR, PADDED}
    assert all(s[1] == 0 for s in got if s[0] != STRIP_MAJOR) and all(s[1] > 0 for s in got if s[0] == STRIP_MAJOR)


def _outcome(r, which):
    s = r['fold_source']
    return (s[which + '_layout'], s[which + '_n0'], s[which + '_depad'])


def test_fold_source_of_the_three_outcomes_of_a_planned_batch(plan):
    W = ['3', '2', '1']
    # stored strip-major on an exact geometry and folded separately; repeated or declined: row-major
    r = plan(W, fuse_accumulate=0, **HYPER)
    assert (_outcome(r, 'ran'), _outcome(r, 'declined'), _outcome(r, 'failed')) == ((STRIP_MAJOR, 128, 0), ROW_FROM_POST, ROW_FROM_POST)
    r = plan(W, n0=1024, n1=32, fuse_accumulate=0, **HYPER)
    assert (_outcome(r, 'ran'), _outcome(r, 'declined'), _outcome(r, 'failed')) == ((STRIP_MAJOR, 1024, 0), ROW_FROM_POST, ROW_FROM_POST)
    # a table on a padded grid: stored on the padded geometry
    r = plan(W, om='table', n0=100, n1=20, **HYPER)
    assert (_outcome(r, 'ran'), _outcome(r, 'declined'), _outcome(r, 'failed')) == ((PADDED, 0, 0), ROW_FROM_POST, ROW_FROM_POST)
    # a kept fit of a padded grid: through depad_kernel; of an exact one: row-major as stored
    r = plan(W, n0=100, n1=20, accumulate=1, keep=1)
    assert (_outcome(r, 'ran'), _outcome(r, 'declined'), _outcome(r, 'failed')) == ((ROW_MAJOR, 0, 1), ROW_FROM_POST, ROW_FROM_POST)
    assert _outcome(plan(W, accumulate=1, keep=1), 'ran') == ROW_FROM_POST
    # both axes, private: the alternating layouts
    assert _outcome(plan(['3:2', '2:2'], n0=128, n1=128, fuse_accumulate=0, **HYPER), 'ran') == (PADDED, 0, 0)


# a full change-point study, a walk with a change point inside, walks without the fused fold: ordinary studies on 513 .. 1023 rows (or 1024
# rows and ragged columns) that the route plans (on = 1) and chain_fold_settle declines with post_private left set
LATE_DECLINES = [(['0:0:3', '0:0:5'], dict(n0=600, n1=32)),
                 (['0:0:3', '0:0:5'], dict(n0=1024, n1=20)),
                 (['3:0:3', '3:0:5'], dict(n0=600, n1=32)),
                 (['3'], dict(n0=600, n1=32, fuse_accumulate=0))]


@pytest.mark.parametrize('chains,kw', LATE_DECLINES)
def test_a_late_decline_folds_row_major(plan, chains, kw):
    r = plan(chains, **HYPER, **kw)
    assert r['plan']['n0p'] == 1024 and r['plan']['pad'] == 1 and r['plan']['ntw'] == 8 and r['route']['on'] == 1
    assert _fold(r) == dict(keep=0, post_private=1, fused=0, fold2=0)
    for which in ('ran', 'declined', 'failed'):               # (on = keep = 0 in every one)
        assert _outcome(r, which) == ROW_FROM_POST, which
    assert 'prefix' not in r


@pytest.mark.parametrize('name', list(dc.DECLINED))
def test_the_planner_declines_the_cases_of_test_declined_batches(plan, name):
    """the same facts as the GPU case (tests/declined_cases.py): planned, on the route, then keep 0"""
    d = dc.DECLINED[name]
    r = plan(d['chains'], **d['facts'])
    assert r['admit']['plan'] == 1 and r['plan'] is not None and r['plan']['pad'] == 1 and r['route'] == dict(
        on=1, clamp=0, n0p=r['plan']['n0p'], ntw=r['plan']['ntw'], pad=1), r
    assert r['fold']['keep'] == 0 and r['fold']['post_private'] == d['post_private'] and r['fold']['depad'] == 0, r['fold']
    assert r['fold']['needs_depad'] == (0 if d['post_private'] else 1)
    assert _outcome(r, 'declined') == ROW_FROM_POST
    # with nothing declined the same plan would be a strip-major layout on the padded geometry: what the launch-per-step kernels never write
    assert plan(source='1,0,%d,1,0,0,%d' % (d['post_private'], d['grid'][0]))['source'] == [(PADDED, 0, 0)]


def test_the_planner_keeps_the_strip_major_case_of_test_declined_batches(plan):
    for name, d in dc.C_CASES.items():
        r = plan(d['chains'], **d['facts'])
        assert r['plan']['pad'] == 0 and r['plan']['strips'] == 2 and r['route']['on'] == 1, name
        assert _fold(r) == dict(keep=1, post_private=1, fused=0, fold2=0), name
        assert _outcome(r, 'ran') == (STRIP_MAJOR, d['grid'][0], 0) and _outcome(r, 'failed') == ROW_FROM_POST, name


def test_host_functions_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan on the host side, as a stand-alone executable"""
    exe = str(tmp_path / 'chain_plan_san')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', SRC, '-o', exe, '-fsanitize=address,undefined'], check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    runs = [_args(['3', '2', '1'], n0=100, n1=20, **HYPER),
            _args(['3'] * 5, cus=2, **HYPER),
            _args(['3:2', '20:12'], n0=100, n1=90),
            _args(['3', '12', '40'], n0=384, clamp=1, cus=1),
            _args(['0:0:3', '0:0:5', '0:0:2', '0'], T=8, **HYPER),
            _args(['0:0:3', '0:0:5:5'], T=8, full=0, evidence_only=1),
            _args(['3:0:4', '3'], n0=600, **HYPER),
            _args(['3'], n0=20),
            _args(admits='1,0.5,1,1', launch='3,2048,8,1,1,1,0,0,0,4,1,1,3,0,2'),
            _args(['0:0:3', '0:0:5'], n0=600, n1=32, **HYPER),
            _args(['3', '2'], n0=1024, n1=32, fuse_accumulate=0, **HYPER),
            _args(source=['1,0,1,0,0,0,128', '0,0,1,1,0,0,600', '1,1,0,1,1,1,100'])]
    for a in runs:
        r = subprocess.run([exe] + a, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.splitlines()[-1].startswith(('tsh', 'route ', 'cost ', 'round_nk_b', 'source '))
        assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
