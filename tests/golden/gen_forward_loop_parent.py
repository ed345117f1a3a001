"""Writes tests/golden/forward_loop_parent.json: per case of tests/test_forward_loop_gpu.py the shape and SHA-256 of logEvidence,
logEvidenceList, the posterior means and the (average) posterior sequence from the library the engine loads.  Run it on an MI355X with
BLHIP_LIBRARY pointing at a library built from the commit BEFORE the forward kernel's step loop changed:
    BLHIP_LIBRARY=/path/to/parent/libblhip.so python tests/golden/gen_forward_loop_parent.py [output.json]
Record it twice, in two processes, and compare the files before committing one."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bayesloop_amd as bl  # noqa: E402
import test_forward_loop_gpu as t  # noqa: E402

if __name__ == '__main__':
    if not os.environ.get('BLHIP_LIBRARY'):
        sys.exit('BLHIP_LIBRARY is not set: this would record the current build, not the parent commit')
    bl.set_engine(None)
    out = {}
    for case in sorted(t.CASES):
        rec, timing, _ = t.collect(case)
        out[case] = rec
        print(case, {k: timing[k] for k in ('fwd_kernel_variant', 'bwd_kernel_variant', 'resident_fallbacks', 'batches')}, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('%s: %d cases, %d bytes' % (path, len(out), os.path.getsize(path)))
