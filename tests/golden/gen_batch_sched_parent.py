"""Writes tests/golden/batch_sched_parent.npz: the results, route figures, launched kernels and folded counts of the cases of
tests/test_batch_sched_bits.py from the library the engine loads.  Run it on an MI355X with BLHIP_LIBRARY pointing at a library built from
the commit BEFORE do_fit's batch loop moved its decisions into blhip_batch_sched.hpp (git worktree of that commit,
python -m bayesloop_amd.csrc.build there):
    BLHIP_LIBRARY=/path/to/parent/libblhip.so python tests/golden/gen_batch_sched_parent.py [output.npz]
Record it twice, in two processes, and compare the files (np.array_equal per key) before committing one: a case on which the parent
differs from itself belongs into ORACLE_HELD of the test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_batch_sched_bits as t  # noqa: E402

if __name__ == '__main__':
    if not os.environ.get('BLHIP_LIBRARY'):
        sys.exit('BLHIP_LIBRARY is not set: this would record the current build, not the parent commit')
    out = {}
    for case in sorted(t.CASES):
        rec, _ = t.collect(case)
        out.update(rec)
        print(case, *t.route_of(rec, case), flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
