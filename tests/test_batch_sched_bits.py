"""
do_fit's batch loop after its decisions moved into host-only functions (bayesloop_amd/csrc/blhip_batch_sched.hpp: the path of an attempt, the
plan of its passes, the tail's decisions, the repeat schedule, the resident paths' retry wait) computes the bits, launches the kernels and
accounts the traffic of the commit before.  tests/golden/batch_sched_parent.npz holds, per case, the results of a library built from that
commit on the same hardware (tests/golden/gen_batch_sched_parent.py wrote it), the deterministic part of the fit's timing -- launches,
batches, kernel variants, fall-backs with their reason, the folds launched and the by-construction HBM bytes and flops --, the kernels the
fit launched with their counts (blhip_kernel_census before and after; the co-residency probe, which runs by the clock, left out) and the
number of chains the accumulator folded.  Every array must be np.array_equal (the posterior sequences: bit-equal by their SHA-256, see
test_chain_split_bits.DIGESTED), every figure and the census equal.

The cases cross the branches of the loop: the forced failures of tests/test_fold_recovery.py -- a batch repeated in place, a rewind to the
first batch of the carried slots with a direct batch inside the range, both in one call, a rewind behind a flush of the slots --; the
K-steps-per-launch 1-D pass repeated with K = 1; the time-resident path and its fall-back for full, evidence-only and kept forward-only
fits; many small batches (the fold nobody waits for) and batches of 64 chains (the forward bookkeeping and its sums behind the backward
launches) with the chain-resident path on and off; carry and resume from step to step of an OnlineStudy.

ORACLE_HELD: cases on which the parent commit's library does not agree with itself from process to process keep the exact route
figures; their arrays are held to the float64 oracle at the suite's bar instead.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import compare
import context_history_cases as ch
import long_series_cases as ls
import oracle_adapter as oa
import step_transition_cases as sc
import test_chain_split_bits as split
import test_fold_recovery as fr
from test_gpu_parity import _g2, _ill_tol, result_of
from test_kernel_sweep import _chain_sigmas
from test_step_transitions import Options

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'batch_sched_parent.npz')

ARRAYS = split.ARRAYS + ('log_evidence', 'local_evidence', 'means', 'posts', 'marginalizedPosterior', 'stepLogEvidence')
DIGESTED = split.DIGESTED + ('posts',)
COUNTS = split.COUNTS + ('accumulate_launches',)
SUMS = split.SUMS
DEFAULTS = dict(fr.DEFAULTS, resident_force_abort=0, chain_resident=1)
ORACLE_HELD = ()

CASES = {}


def _study_case(name, c, opts=None, rearm=False):
    CASES[name] = dict(kind='study', c=c, opts=dict(opts or {}), rearm=rearm)


# ---- the forced-failure matrix of tests/test_fold_recovery.py: 3 x 16 chains, max_batch = 16 ---------------------------------------------------
# fused, direct (a wide walk), fused: the last batch poisons the slots that carry the first
POISONED = {'unforced': {}, 'fold2': dict(fold_force_fail_batch=2), 'stage2_at2': dict(chain_force_fail_batch=2, chain_force_fail_stage=2),
            'stage3_at2': dict(chain_force_fail_batch=2, chain_force_fail_stage=3)}
# three fused batches: batch 1 fails its forward check and is repeated in place; ... and batch 2 then poisons the slots
IN_PLACE = {'unforced': {}, 'stage1_at1': dict(chain_force_fail_batch=1, chain_force_fail_stage=1),
            'stage1_at1_fold2': dict(chain_force_fail_batch=1, chain_force_fail_stage=1, fold_force_fail_batch=2)}
for _flavour in ('two_chain', 'single_chain_2strips', 'both_axes'):
    _F = fr.FLAVOURS[_flavour]
    for _name, _opts in POISONED.items():
        _study_case('%s-wide-%s' % (_flavour, _name), _F['wide'], dict(_F['opts'], max_batch=fr.NB, **_opts), rearm=True)
    for _name, _opts in IN_PLACE.items():
        _study_case('%s-plain-%s' % (_flavour, _name), _F['plain'], dict(_F['opts'], max_batch=fr.NB, **_opts), rearm=True)

# test_failure_after_a_flush_of_the_carried_slots: batch 1 starts the slots afresh, batch 2 is direct, batch 3 poisons them
FLUSH = fr._hyper(128, 64, 97, 8, fr._values(0.0, 0.5, nbatch=4, wide=3.0, wide_batch=2), prior=('array', [1e-240] * fr.NB + [1.0] * (3 * fr.NB)))
_study_case('flush-unforced', FLUSH, dict(max_batch=fr.NB))
_study_case('flush-fold3', FLUSH, dict(max_batch=fr.NB, fold_force_fail_batch=3), rearm=True)

# ---- the K-steps-per-launch 1-D pass repeated with K = 1: the one 'repeat' of tests/long_series_cases.py (T = 14) -----------------------------
CASES['fused1d-ramp-repeat'] = dict(kind='long_series', fam='fused1d', schedule='ramp')

# ---- one chain on 64 x 64, T = 8: the time-resident path, and (resident_force_abort: only what the host's check answers) its fall-back --------
for _mode, _fit in (('full', {}), ('evidence', dict(evidenceOnly=True)), ('forward_keep', dict(forwardOnly=True))):
    _c = dict(study='Study', data=('series', 7201, 8), om=_g2(64, 64), tm=('GRW', 'sigma', _chain_sigmas(6, 64, -8.0, 8.0)[0], 'mean', None), fit=_fit)
    _study_case('single-64x64-%s' % _mode, _c)
    _study_case('single-64x64-%s-abort' % _mode, _c, dict(resident_force_abort=1), rearm=True)


# ---- many small batches / batches of 64 chains on 32 x 32, T = 6; chain_resident = 0: the same on the launch-per-step kernels ------------------
def _hyper32(nchains, seed):
    return dict(study='HyperStudy', data=('series', seed, 6), om=_g2(32, 32),
                tm=('GRW', 'sigma', [float(x) for x in np.linspace(0.05, 1.5, nchains)], 'mean', None))


_study_case('hyper80-batches-of-16', _hyper32(80, 7202), dict(max_batch=16))
_study_case('hyper80-batches-of-16-step', _hyper32(80, 7202), dict(max_batch=16, chain_resident=0))
_study_case('hyper128-batches-of-64', _hyper32(128, 7203), dict(max_batch=64))
_study_case('hyper128-batches-of-64-step', _hyper32(128, 7203), dict(max_batch=64, chain_resident=0))

# ---- carry and resume: three steps of an OnlineStudy on 32 x 32 --------------------------------------------------------------------------------
ONLINE = dict(om=('Gaussian', [('mean', cases._g('cint', -5, 5, 32)), ('std', cases._g('oint', 0, 3, 32))], 'default'),
              models=[('walk', ('GRW', 'sm', [0.1, 0.3], 'mean', None)), ('static', ('Static',))], tm_prior=[0.6, 0.4], data=('series', 43, 3))
CASES['online-32x32-3-steps'] = dict(kind='online', c=ONLINE)


@pytest.fixture(scope='module', autouse=True)
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    bl.set_engine(prev)


def _arrays_of_study(S, c):
    for key in split.ARRAYS:
        value = getattr(S, key, None)
        if value is None or (key.startswith('posterior') and c.get('fit', {}).get('evidenceOnly')):
            continue
        yield key, np.asarray(value, dtype=float)


def collect(case):
    """runs the case on the library the engine has loaded -> ({'<case>/<array>': values, '<case>/counts': COUNTS, '<case>/sums': SUMS,
    '<case>/census': the kernels launched and their counts as JSON, '<case>/folded': chains in the accumulator (-1: none is open)}, study)"""
    D = CASES[case]
    eng = bl.get_engine()
    opts = D.get('opts', {})
    S, folded, arrays = None, -1, []
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
            if D['kind'] == 'study':
                S = cases.build(bl, D['c'])
                before = ch.census()
                S.fit(**cases.fit_kwargs(D['c']))
                launched = ch.census_delta(before, ch.census())          # (before the posteriors are read: that launches the normalisation)
                timing = eng.last_timing()
                if D['c']['study'] == 'HyperStudy':
                    folded = eng.accum_log_ref()[1]
                arrays = list(_arrays_of_study(S, D['c']))
            elif D['kind'] == 'long_series':
                fam, schedule = D['fam'], D['schedule']
                keep = list(range(len(ls.case_of(fam, ls.steps_of(schedule))['chains'])))
                with Options(eng, sc.CASES[ls.FAMILIES[fam]['case']]['opts']):
                    before = ch.census()
                    got = ls.run_problem(eng, fam, schedule, keep)
                    launched = ch.census_delta(before, ch.census())
                timing = eng.last_timing()
                arrays = [(k, np.asarray(got[k], dtype=float)) for k in ('log_evidence', 'local_evidence', 'means', 'posts')]
            else:
                S = cases.build_online(bl, D['c'], storeHistory=False)
                before = ch.census()
                steps, marginals = [], []
                for d in cases.online_data(D['c']):
                    S.step(d)
                    steps.append(float(S.logEvidence))
                    marginals.append(np.asarray(S.marginalizedPosterior, dtype=float))
                launched = ch.census_delta(before, ch.census())
                timing = eng.last_timing()
                arrays = [('stepLogEvidence', np.asarray(steps)), ('marginalizedPosterior', np.asarray(marginals))]
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])
        if D.get('rearm'):
            fr._rearm()
    out = {}
    for key, a in arrays:
        if a.size and key in DIGESTED:
            out['%s/%s.sha256' % (case, key)] = split.digest(a)
        elif a.size:
            out['%s/%s' % (case, key)] = a
    out['%s/counts' % case] = np.asarray([timing[k] for k in COUNTS], dtype=np.int64)
    out['%s/sums' % case] = np.asarray([timing[k] for k in SUMS], dtype=np.float64)
    out['%s/census' % case] = np.asarray(json.dumps(sorted(launched.items())))
    out['%s/folded' % case] = np.asarray(folded, dtype=np.int64)
    return out, S


def route_of(rec, case):
    return dict(zip(COUNTS, (int(x) for x in rec['%s/counts' % case]))), dict(zip(SUMS, (float(x) for x in rec['%s/sums' % case]))), \
        json.loads(str(rec['%s/census' % case])), int(rec['%s/folded' % case])


def test_the_cases_are_the_ones_listed():
    assert len(CASES) == 3 * (4 + 3) + 2 + 1 + 6 + 4 + 1
    assert set(DEFAULTS) >= {k for D in CASES.values() for k in D.get('opts', {})}
    assert all(D['kind'] == 'study' for name, D in CASES.items() if name in ORACLE_HELD)


@pytest.mark.parametrize('case', sorted(CASES))
def test_results_route_and_folds_are_the_parent_commits(case):
    parent = np.load(GOLDEN)
    got, S = collect(case)
    want = {k: parent[k] for k in parent.files if k.startswith(case + '/')}
    assert sorted(got) == sorted(want)
    got_route, want_route = route_of(got, case), route_of(want, case)
    print(case, got_route)
    assert got_route[0] == want_route[0]
    assert got_route[1] == want_route[1]                      # (deterministic sums of doubles: equal, not close)
    assert [tuple(x) for x in got_route[2]] == [tuple(x) for x in want_route[2]]
    assert got_route[3] == want_route[3]
    arrays = sorted(k for k in want if k.rsplit('/', 1)[1] in ARRAYS)
    assert arrays or any(k.endswith('.sha256') for k in want)
    if case in ORACLE_HELD:
        c = CASES[case]['c']
        with np.errstate(all='ignore'):
            ref = oa.run(c)
        res = result_of(S, c)
        gold = {k: np.asarray(ref[k]) for k in ('logEvidence', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues', 'logEvidenceList',
                                                'hyperParameterDistribution') if ref.get(k) is not None and k in res and len(np.atleast_1d(ref[k]))}
        compare.check(res, gold, compare.GPU_TOL, case_tol=_ill_tol(S))
        return
    for k in arrays:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
    for k in sorted(k for k in want if k.endswith('.sha256')):
        assert str(got[k]) == str(want[k]), '%s: shape and SHA-256 of the bytes, got %s, want %s' % (k, got[k], want[k])
