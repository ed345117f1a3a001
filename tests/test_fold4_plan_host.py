"""The plan of the folding backward pass with FOUR chains per accumulator cell (chain_fold_plan, bayesloop_amd/csrc/blhip_chain_plan.hpp), host-only.

tests/host/fold4_plan_main.cpp is built around the plan header and run on a CPU: a hyper-study's full fit on a grid, a chip of `cus` compute
units, chains given by the radii of their walks.  What is held:
* the flavour takes a batch only when the fold is fused and two-chain-capable, the geometry exact, no chain restarts, every round's ring
  within 6 .. 24, and the batch has at least fold4_min_chains chains (32 unless set);
* rounds hold 4 x floor(cus / strips of 8 columns) chains, the ring of a round is its widest chain's, slots_used counts block QUADS;
* a ring beyond 24 ANYWHERE keeps the whole batch on the two-chain kernel (one layout per batch);
* fold4 = 0 gives the two-chain plan, entry for entry;
* a launch's traffic model: 8 + 16 / 4 bytes per cell and chain-step of a full quad.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'fold4_plan_main.cpp')


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    exe = str(tmp_path_factory.mktemp('fold4_plan') / 'fold4_plan')
    subprocess.run([hipcc, '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)

    def run(chains, **kw):
        out = subprocess.run([exe] + ['chain=%s' % c for c in chains] + ['%s=%s' % kv for kv in kw.items()], check=True, capture_output=True,
                             text=True, timeout=120).stdout
        r = {}
        for line in out.splitlines():
            w = line.split()
            if w[0] in ('plan', 'fold'):
                r[w[0]] = dict(zip(w[1::2], map(int, w[2::2])))
            elif w[0] == 'cost':
                r['cost'] = float(w[1])
            else:
                r[w[0]] = [int(x) for x in w[1:]]
        return r
    return run


def nk_of(radius):
    return (16 + 2 * max(4, (radius + 3) // 4 * 4)) // 4


def test_rounds_ring_lengths_and_slots(plan):
    # 128 x 16: one strip of 16 columns = two of 8; 8 compute units -> 4 quads = 16 chains per round
    radii = [3] * 10 + [9] * 10 + [17] * 10 + [40] * 10
    r = plan(radii, cus=8)
    assert r['plan'] == dict(strips=1, ntw=1, cpr=8, pad=0)
    assert r['fold'] == dict(keep=1, fused=1, fold2=1, fold4=1, slots_used=4)
    assert r['round_start_b'] == [0, 16, 32, 40]
    assert r['round_nk_b'] == [nk_of(9), nk_of(40), nk_of(40)] == [10, 24, 24]
    assert r['cost'] == pytest.approx(8.0 + 16.0 / 4, rel=1e-14)
    # C4: 512 x 512, 256 compute units: 64 strips of 8 columns x 4 quads = 16 chains per launch, 4 partial accumulators instead of 8
    r = plan(['%d' % (1 + k // 13) for k in range(512)], n0=512, n1=512, cus=256)
    assert r['plan'] == dict(strips=32, ntw=4, cpr=8, pad=0)
    assert r['fold']['fold4'] == 1 and r['fold']['slots_used'] == 4
    assert r['round_start_b'] == list(range(0, 513, 16)) and len(r['round_nk_b']) == 32
    assert r['round_nk_b'][0] == 6 and r['round_nk_b'][-1] == nk_of(1 + 511 // 13) == 24
    # the last round's odd end: 37 chains = 2 full rounds + 5 chains (a quad and a single chain): two block quads
    r = plan(['5'] * 37, cus=8)
    assert r['round_start_b'] == [0, 16, 32, 37] and r['fold']['slots_used'] == 4
    # fewer chains than a round: slots = block quads
    r = plan(['5'] * 6, cus=64, fold4_min_chains=1)
    assert r['round_start_b'] == [0, 6] and r['fold']['slots_used'] == 2
    assert r['cost'] == pytest.approx(8.0 + 16.0 * 2 / 6, rel=1e-14)


def test_threshold(plan):
    two = dict(keep=1, fused=1, fold2=1, fold4=0)
    r = plan(['3'] * 31, cus=8)
    assert {k: r['fold'][k] for k in two} == two and r['round_start_b'] == [0, 16, 31] and r['fold']['slots_used'] == 8
    assert plan(['3'] * 32, cus=8)['fold']['fold4'] == 1
    assert plan(['3'] * 5, cus=8)['fold']['fold4'] == 0
    r = plan(['3'] * 5, cus=8, fold4_min_chains=1)
    assert r['fold']['fold4'] == 1 and r['round_start_b'] == [0, 5] and r['fold']['slots_used'] == 2
    assert plan(['3'] * 40, cus=8, fold4_min_chains=41)['fold']['fold4'] == 0


def test_a_ring_beyond_24_anywhere_declines_the_whole_batch(plan):
    r = plan(['3'] * 39 + ['41'], cus=8)                      # radius 41 -> 44 -> ring 26 in the last round only
    assert r['fold']['fold2'] == 1 and r['fold']['fold4'] == 0
    assert r['round_start_b'] == [0, 16, 32, 40] and r['round_nk_b'] == [6, 6, 26] and r['fold']['slots_used'] == 8
    assert r['cost'] == pytest.approx(8.0 + 16.0 / 2, rel=1e-14)
    assert plan(['3'] * 39 + ['40'], cus=8)['fold']['fold4'] == 1


def test_what_else_keeps_the_two_chain_kernel(plan):
    for chains, kw in ((['3'] * 40, dict(n0=100)),                       # a padded geometry
                       (['0'] * 40, {}),                                    # no stencil at all: the NK = 4 kernels
                       (['3:0:4'] * 40, {}),                                # restarts
                       (['3'] * 40, dict(om='table')),                      # a tabulated likelihood
                       (['3'] * 40, dict(n0=128, n1=1024, cus=256)),        # 128 strips of 8 columns: more than a granule per lane
                       (['3'] * 40, dict(n0=128, n1=64, cus=7))):           # fewer compute units than strips of 8
        r = plan(chains, **kw)
        assert r['fold']['fold4'] == 0, (chains[0], kw)
    assert plan(['3'] * 40, fold2=0)['fold'] == dict(keep=1, fused=0, fold2=0, fold4=0, slots_used=40)
    # chains without a walk among walking ones are fine (identity band inside the round's ring)
    assert plan(['0'] * 8 + ['3'] * 32, cus=8)['fold']['fold4'] == 1


def test_fold4_off_reproduces_the_two_chain_plan(plan):
    for chains, kw in ((['3'] * 10 + ['9'] * 10 + ['17'] * 10 + ['40'] * 10, dict(cus=8)), (['5'] * 37, dict(cus=8)),
                       (['%d' % (1 + k // 13) for k in range(512)], dict(n0=512, n1=512))):
        off = plan(chains, fold4=0, **kw)
        below = plan(chains, fold4_min_chains=10 ** 6, **kw)
        assert off == below and off['fold']['fold4'] == 0 and off['fold']['fold2'] == 1
        cpr = off['plan']['cpr']
        assert off['round_start_b'] == list(range(0, len(chains), 2 * cpr)) + [len(chains)]
        assert off['fold']['slots_used'] == min(cpr, (len(chains) + 1) // 2)
