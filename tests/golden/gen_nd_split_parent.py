"""Writes tests/golden/nd_split_parent.npz: the results of the five cases of tests/test_nd_split_bits.py from the library the engine loads.
Run it on an MI355X with BLHIP_LIBRARY pointing at a library built from the commit BEFORE do_fit_nd was split (git worktree of that
commit, python -m bayesloop_amd.csrc.build there):
    BLHIP_LIBRARY=/path/to/parent/libblhip.so python tests/golden/gen_nd_split_parent.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_nd_split_bits as t  # noqa: E402

if __name__ == '__main__':
    if not os.environ.get('BLHIP_LIBRARY'):
        sys.exit('BLHIP_LIBRARY is not set: this would record the current build, not the parent commit')
    out = {}
    for case in sorted(t.CASES):
        out.update(t.collect(case))
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
