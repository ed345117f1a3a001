"""Wall time per ``OnlineStudy.step`` call on the MI355X (profiles/core_dedup_notes.md): the study of ``online_kat_2tm`` (tests/cases.py),
history off, its five data points fed over and over -- 100 calls of warm-up on a first study (code objects, the context's buffers), then
300 timed calls on a fresh one, the host clock around each call (a call ends in ``carry_read``, a device-to-host copy).  Prints one line
with the median.
    python tools/online_step_timing.py [TREE [LABEL]]
TREE: the tree whose ``bayesloop_amd`` package is measured (default: this one); a tree of another commit needs ``BLHIP_LIBRARY`` pointing at a
library.  To compare two commits run the two alternately, a process each, several times a side."""
import contextlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tree = os.path.realpath(sys.argv[1]) if len(sys.argv) > 1 else HERE
sys.path.insert(0, os.path.join(HERE, 'tests'))
sys.path.insert(0, tree)
import bayesloop_amd as bl  # noqa: E402
import cases  # noqa: E402


def run(n, data):
    S = cases.build_online(bl, 'online_kat_2tm', storeHistory=False)
    times = []
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(n):
            d = data[k % len(data)]
            t0 = time.perf_counter()
            S.step(d)
            times.append(time.perf_counter() - t0)
    return np.array(times), S


if __name__ == '__main__':
    if not os.path.realpath(bl.__file__).startswith(tree + os.sep):
        sys.exit('bayesloop_amd was imported from %s, not from %s' % (bl.__file__, tree))
    if type(bl.get_engine()).__name__ != 'HipEngine':
        sys.exit('no HipEngine: a time per step is a time on the GPU')
    data = cases.online_data(cases.ONLINE_CASES['online_kat_2tm'])
    run(100, data)
    t, S = run(300, data)
    print('STEP %s median_us %.2f mean_us %.2f p10_us %.2f p90_us %.2f calls %d logE %r' % (
        sys.argv[2] if len(sys.argv) > 2 else tree, 1e6 * np.median(t), 1e6 * np.mean(t), 1e6 * np.percentile(t, 10), 1e6 * np.percentile(t, 90),
        len(t), S.logEvidence), flush=True)
