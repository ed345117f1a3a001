"""Writes tests/golden/core_dedup_parent.npz (and, with --gpu on an MI355X, core_dedup_parent_gpu.npz): the calls into the engine, the
printed text and the study state of the cases of tests/test_core_dedup_bits.py from the package of the commit BEFORE core.py's copies
were folded into shared helpers.  Give it a tree of that commit (git worktree add /path/to/parent <commit>); for --gpu that tree needs
the library too (bayesloop_amd/libblhip.so copied into it: core.py is all that differs, the library is the same build):
    python tests/golden/gen_core_dedup_parent.py /path/to/parent [--gpu] [output.npz]
It refuses to record the package of the tree it lies in.  Record twice, in two processes, and compare the files (np.array_equal per key)
before committing one: a case on which the parent differs from itself belongs into LEFT_OUT of the test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--gpu']
    gpu = '--gpu' in sys.argv[1:]
    if not args:
        sys.exit(__doc__)
    parent = os.path.realpath(args[0])
    if os.path.samefile(parent, ROOT):
        sys.exit('%s is the current tree: this would record the current tree, not the parent commit' % parent)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, parent)                  # (the parent's package, and its oracle, in front of everything)
    import bayesloop_amd
    where = os.path.realpath(bayesloop_amd.__file__)
    if not where.startswith(parent + os.sep):
        sys.exit('bayesloop_amd was imported from %s, not from %s: this would record the current tree, not the parent commit' % (where, parent))
    import test_core_dedup_bits as t
    out = {}
    for case in (t.GPU_CASES if gpu else t.CASES):
        rec = t.collect_gpu(case) if gpu else t.collect(case)[0]
        out.update(rec)
        print(case, flush=True)
    path = args[1] if len(args) > 1 else (t.GOLDEN_GPU if gpu else t.GOLDEN)
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
