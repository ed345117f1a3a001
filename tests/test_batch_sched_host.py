"""
The host-only decisions of do_fit's batch loop (bayesloop_amd/csrc/blhip_batch_sched.hpp), none of which needs a GPU: the path an attempt of a
batch runs on (batch_path), what its passes do with their sums (pass_plan), the tail of the batch (keep_rows, carried_state_source,
fold_action), which batch runs next and whether it folds (BatchSchedule), and when a context whose resident launch gave up tries the
resident paths again (ResidentRetry).  The stand-alone program tests/host/batch_sched_main.cpp plays do_fit's loop around the schedule
with the device taken out -- a script says what the passes of each batch answer -- and keeps a ledger of what reaches the accumulator;
the expectations below are written out by hand from the rules:

* a resident pass that gives up or fails a check: the batch is repeated in place on the launch-per-step kernels and folded directly; a
  second failure there is an internal error; the raw sums of the K-steps-per-launch 1-D pass fail: repeated in place with K = 1;
* ... unless the failed backward pass has written carried slots that hold EARLIER batches: the slots are dropped, the call goes back to the
  first batch they carried, the chain-resident path is off up to the failed batch, and of the batches run again only those fold whose
  contribution was in the slots -- a batch that was folded directly (not chain-resident, or repeated in place) is in the accumulator already;
* every batch reaches the accumulator exactly once, whatever fails, and every call ends.

Built plain and with -fsanitize=address,undefined (host code only; the program has its own main).
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'batch_sched_main.cpp')

RESIDENT, CHAIN, ROW1D, STEP = range(4)
PATHS = ('RESIDENT', 'CHAIN', 'ROW1D', 'STEP')


def _hipcc():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.fail('no hipcc: the library itself could not have been built')
    return hipcc


@pytest.fixture(scope='module')
def sched(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('batch_sched') / 'batch_sched')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', SRC, '-o', exe], check=True, capture_output=True, text=True, timeout=300)

    def run(*args):
        return [line.split() for line in subprocess.run([exe] + list(args), check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()]
    return run


def _script(sched, letters, fresh=-1):
    """-> ([(batch, allow_chainres, action, from, refold_skip)], times each batch reached the accumulator or None, ok)"""
    rows = sched('script=%s/%d' % (letters, fresh))
    attempts = [(int(w[1]), int(w[2]), w[3], None if w[4] == '-' else int(w[4]), None if w[5] == '-' else int(w[5])) for w in rows if w[0] == 'attempt']
    last = rows[-1]
    if last[0] != 'ledger':
        return attempts, None, ' '.join(last)
    return attempts, [int(x) for x in last[1:-2]], int(last[-1])


def FINISH(b, allow=1, skip=0):
    return (b, allow, 'FINISH', None, skip)


def test_no_failure(sched):
    attempts, ledger, ok = _script(sched, 'S,S,S')
    assert attempts == [FINISH(0), FINISH(1), FINISH(2)] and ledger == [1, 1, 1] and ok == 1
    assert _script(sched, 'D,S,D,D') == ([FINISH(b) for b in range(4)], [1, 1, 1, 1], 1)


def test_fused_direct_fused_the_last_batch_poisons_the_slots_of_the_first(sched):
    """test_fold_recovery.py: test_wide_batch_between_fused_batches_is_folded_once -- back to batch 0; batches 0 and 2 fold again, the direct
    batch 1 does not; the chain-resident path is off up to batch 2 and on again behind it"""
    attempts, ledger, ok = _script(sched, 'S,D,P,S')
    assert attempts == [FINISH(0), FINISH(1), (2, 1, 'REWIND', 0, None),
                        FINISH(0, allow=0), FINISH(1, allow=0, skip=1), FINISH(2, allow=0), FINISH(3, allow=1)]
    assert ledger == [1, 1, 1, 1] and ok == 1


def test_a_batch_repeated_in_place_then_poisoned_slots(sched):
    """test_batch_repeated_in_place_then_poisoned_slots: batch 1 fails its forward check, is repeated in place and folded directly"""
    attempts, ledger, ok = _script(sched, 'S,E,P')
    assert attempts == [FINISH(0), (1, 1, 'REPEAT_ON_STEP_KERNELS', None, None), FINISH(1), (2, 1, 'REWIND', 0, None),
                        FINISH(0, allow=0), FINISH(1, allow=0, skip=1), FINISH(2, allow=0)]
    assert ledger == [1, 1, 1] and ok == 1


def test_failure_in_the_second_batch(sched):
    """fused, fused (poisons), direct: the direct batch behind the range is no repeat"""
    attempts, ledger, ok = _script(sched, 'S,P,D')
    assert attempts == [FINISH(0), (1, 1, 'REWIND', 0, None), FINISH(0, allow=0), FINISH(1, allow=0), FINISH(2, allow=1)]
    assert ledger == [1, 1, 1] and ok == 1


def test_failure_after_a_flush_of_the_carried_slots(sched):
    """four batches, batch 1 started the slots afresh (first_batch = 1), batch 3 poisons them: back to batch 1, not 0"""
    attempts, ledger, ok = _script(sched, 'S,S,D,P', fresh=1)
    assert attempts == [FINISH(0), FINISH(1), FINISH(2), (3, 1, 'REWIND', 1, None),
                        FINISH(1, allow=0), FINISH(2, allow=0, skip=1), FINISH(3, allow=0)]
    assert ledger == [1, 1, 1, 1] and ok == 1
    # without the flush the slots carry batch 0 too
    assert _script(sched, 'S,S,D,P')[0][3:5] == [(3, 1, 'REWIND', 0, None), FINISH(0, allow=0)]


def test_a_failure_that_touched_its_own_slots_only_is_repeated_in_place(sched):
    """part_fresh0: the failed backward pass started the slots itself -- nothing of an earlier batch is lost"""
    attempts, ledger, ok = _script(sched, 'D,P,S')
    assert attempts == [FINISH(0), (1, 1, 'REPEAT_ON_STEP_KERNELS', None, None), FINISH(1), FINISH(2)]
    assert ledger == [1, 1, 1] and ok == 1
    # ... also where it flushed the slots of the earlier batches first
    attempts, ledger, ok = _script(sched, 'S,P,S', fresh=1)
    assert attempts == [FINISH(0), (1, 1, 'REPEAT_ON_STEP_KERNELS', None, None), FINISH(1), FINISH(2)] and ledger == [1, 1, 1] and ok == 1


def test_the_raw_sums_of_the_k_steps_pass_fail(sched):
    attempts, ledger, ok = _script(sched, 'K,D')
    assert attempts == [(0, 1, 'REPEAT_K1', None, None), FINISH(0), FINISH(1)] and ledger == [1, 1] and ok == 1


def test_a_second_failure_on_the_launch_per_step_kernels(sched):
    attempts, ledger, what = _script(sched, 'S,EX')
    assert attempts == [FINISH(0), (1, 1, 'REPEAT_ON_STEP_KERNELS', None, None), (1, 1, 'INTERNAL_ERROR', None, None)]
    assert ledger is None and what == 'internal error'


def test_every_batch_reaches_the_accumulator_once_in_every_script_of_up_to_four_batches(sched):
    """first attempts over: into the slots / folded directly / fails before the backward pass / fails after touching the carried slots,
    crossed with every batch that starts the slots afresh (and none); repeats in place pass and fold directly"""
    rows = sched('exhaustive=4')
    assert rows[-1][0] == 'exhaustive' and len(rows) == 1, rows[:5]
    scripts, bad, longest = (int(x) for x in rows[-1][1:])
    assert scripts == sum(4 ** n * (n + 1) for n in range(1, 5)) == 1592 and bad == 0
    # the longest call: a batch fails at most once (behind a failure it runs with the chain-resident path off), finishes once, and the
    # ranges that are run again are disjoint (a rewind leaves no live slots behind): at most 4 failures + 4 tails + 3 tails again
    assert 4 <= longest <= 11


def test_the_ledger_has_teeth(sched):
    """the right sequence of fused, direct, poisoned, and the two mistakes the schedule was written against"""
    assert sched('ledger=n=3,f0,d1,x,d0,d2,+') == [['ledger', '1', '1', '1', 'ok', '1']]
    # the direct batch folded again after the rewind
    assert sched('ledger=n=3,f0,d1,x,d0,d1,d2,+') == [['ledger', '1', '2', '1', 'ok', '0']]
    # the rewound fused batch not folded again
    assert sched('ledger=n=3,f0,d1,x,d2,+') == [['ledger', '0', '1', '1', 'ok', '0']]
    # slots nobody flushed
    assert sched('ledger=n=2,f0,d1') == [['ledger', '0', '1', 'ok', '0']]


def test_batch_path(sched):
    """the resident paths only while nothing failed; behind a failure the 1-D kernels where the batch is 1-D, else the launch-per-step ones"""
    combos = list(itertools.product((0, 1), repeat=4))
    got = sched(*['path=%d,%d,%d,%d' % c for c in combos])
    for (rr, cr, r1, failed), w in zip(combos, got):
        want = RESIDENT if rr and not failed else CHAIN if cr and not failed else ROW1D if r1 else STEP
        assert w == ['path', PATHS[want]], (rr, cr, r1, failed)


def _pass(sched, path, full=1, r1_chain=0, B=64, copy_stream=1, late_sums=1):
    (w,) = sched('pass=%d,3,5,7,%d,%d,%d,%d,%d' % (path, full, r1_chain, B, copy_stream, late_sums))
    return tuple(int(x) for x in w[1:])


def test_pass_plan(sched):
    # the slots: the resident kernel's tiles, the chain-resident kernel's strips, the tile of the other kernels
    assert [_pass(sched, p, B=1)[0] for p in (RESIDENT, CHAIN, ROW1D, STEP)] == [3, 5, 7, 7]
    # the forward bookkeeping behind the backward launches: a full fit of >= 64 chains on the launch-per-step kernels or the 1-D chain kernel
    assert _pass(sched, STEP) == (7, 1, 1) and _pass(sched, STEP, B=63) == (7, 0, 0) and _pass(sched, STEP, full=0) == (7, 0, 0)
    assert _pass(sched, ROW1D) == (7, 0, 0) and _pass(sched, ROW1D, r1_chain=1) == (7, 1, 1)
    assert _pass(sched, RESIDENT, B=1000) == (3, 0, 0) and _pass(sched, CHAIN, B=1000, r1_chain=1) == (5, 0, 0)
    # its sums beside the backward pass: a copy stream and the option
    assert _pass(sched, STEP, copy_stream=0) == (7, 1, 0) and _pass(sched, STEP, late_sums=0) == (7, 1, 0)


def test_the_tail_of_a_batch(sched):
    def one(arg):
        (w,) = sched(arg)
        return w[1:]
    # keep_posterior: every row, but for the rows the resident kernel normalised in place
    for path in (CHAIN, ROW1D, STEP):
        assert one('keep=%d,1,10,4' % path) == ['0', '10'] and one('keep=%d,0,10,4' % path) == ['0', '10']
    assert one('keep=%d,1,10,4' % RESIDENT) == ['0', '0'] and one('keep=%d,0,10,4' % RESIDENT) == ['6', '10']
    assert one('keep=%d,0,3,4' % RESIDENT) == ['0', '3']
    # the carried state: the last row of the sequence (chains T x G apart), or the state buffer the last launch wrote (chains G apart)
    assert one('carry=0,0,8,1,100') == ['-1', '700', '800'] and one('carry=0,1,8,4,100') == ['-1', '700', '800']
    assert one('carry=1,0,8,1,100') == ['1', '0', '100'] and one('carry=1,0,9,1,100') == ['0', '0', '100']
    assert one('carry=1,0,8,4,100') == ['1', '0', '100']                      # (not 1-D: one step per launch whatever K says)
    assert one('carry=1,1,8,4,100') == ['1', '0', '100'] and one('carry=1,1,9,4,100') == ['0', '0', '100'] and one('carry=1,1,9,1,100') == ['0', '0', '100']
    assert one('carry=1,1,8,1,100') == ['1', '0', '100'] and one('carry=1,1,12,4,100') == ['0', '0', '100']      # (11 // 4 = 2 launches before the last)
    # the fold: not asked for; done by the kernel or before; nobody waits from 4 batches on unless something is kept or carried
    assert one('fold=0,1,1,9,0,0') == ['NOT_ASKED']
    assert one('fold=1,1,0,9,0,0') == ['SKIPPED'] and one('fold=1,0,1,9,0,0') == ['SKIPPED']
    assert one('fold=1,0,0,4,0,0') == ['UNWAITED'] and one('fold=1,0,0,3,0,0') == ['AND_WAIT']
    assert one('fold=1,0,0,4,1,0') == ['AND_WAIT'] and one('fold=1,0,0,4,0,1') == ['AND_WAIT']


def _retry(sched, ops):
    """-> per op (ok, retry_after, fits_since, giveups, rearmed)"""
    return [tuple(int(x) for x in w[2:]) for w in sched('retry=' + ','.join(ops))]


def test_resident_retry(sched):
    # give-ups in a row: the first waits 8 fits, then 16, 32 .. 1024 and no longer
    rows = _retry(sched, ['g'] * 10)
    assert [r[1] for r in rows] == [8, 16, 32, 64, 128, 256, 512, 1024, 1024, 1024]
    assert all(r[0] == 0 and r[2] == 0 for r in rows) and [r[3] for r in rows] == list(range(1, 11))
    # a pass that went through: the short wait again
    assert _retry(sched, ['g', 'g', 'g', 'p', 'g'])[2:] == [(0, 32, 0, 3, 0), (0, 8, 0, 0, 0), (0, 8, 0, 1, 0)]
    # re-armed by the fit that begins exactly retry_after fits later; a fit of an armed context counts nothing
    rows = _retry(sched, ['f', 'g'] + ['f'] * 9)
    assert rows[0] == (1, 8, 0, 0, 0) and rows[1] == (0, 8, 0, 1, 0)
    assert rows[2:9] == [(0, 8, k, 1, 0) for k in range(1, 8)] and rows[9] == (1, 8, 0, 1, 1) and rows[10] == (1, 8, 0, 1, 0)
    rows = _retry(sched, ['g', 'g'] + ['f'] * 16)
    assert [r[4] for r in rows[2:]] == [0] * 15 + [1]
    # a give-up between restarts the count
    assert _retry(sched, ['g', 'f', 'f', 'g', 'f'])[-1] == (0, 16, 1, 2, 0)
    # the options: resident_retry_after, resident_ok
    assert _retry(sched, ['g', 'r2', 'f', 'f']) == [(0, 8, 0, 1, 0), (0, 2, 0, 1, 0), (0, 2, 1, 1, 0), (1, 2, 0, 1, 1)]
    assert _retry(sched, ['g', 'g', 'f', 's1']) == [(0, 8, 0, 1, 0), (0, 16, 0, 2, 0), (0, 16, 1, 2, 0), (1, 8, 0, 0, 0)]
    assert _retry(sched, ['g', 'g', 'f', 's0']) [-1] == (0, 16, 0, 2, 0)         # parked by hand: the wait and the give-ups stay
    assert _retry(sched, ['s0'] + ['f'] * 8)[-1] == (1, 8, 0, 0, 1)


def test_host_functions_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan on the host side, as a stand-alone executable"""
    exe = str(tmp_path / 'batch_sched_san')
    subprocess.run([_hipcc(), '-std=c++17', '--offload-arch=gfx950', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                    '-fno-sanitize-recover=undefined', SRC, '-o', exe, '-fsanitize=address,undefined'], check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
    runs = [['script=S,D,P,S/-1', 'script=S,E,P/-1', 'script=S,S,D,P/1', 'script=D,P,S/-1', 'script=K,D/-1', 'script=S,EX/-1'],
            ['exhaustive=4'],
            ['ledger=n=3,f0,d1,x,d0,d1,d2,+', 'ledger=n=3,f0,d1,x,d2,+'],
            ['path=1,0,0,0', 'path=0,1,1,1', 'pass=3,3,5,7,1,0,64,1,1', 'keep=0,0,10,4', 'carry=1,1,9,4,100', 'carry=0,0,8,1,100', 'fold=1,0,0,4,0,0'],
            ['retry=' + ','.join(['g'] * 12 + ['f'] * 5 + ['p', 's0', 's1', 'r3', 'g', 'f', 'f', 'f'])]]
    for a in runs:
        r = subprocess.run([exe] + a, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.splitlines()[-1].startswith(('ledger ', 'internal error', 'exhaustive 1592 0 ', 'fold ', 'retry '))
        assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
