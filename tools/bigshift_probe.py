"""Wall time of fit() for the large-shift workloads of tests/bigshift_cases.py: the change-point batch with the drift on the
first parameter (columns: blk::bigshift_kernel<0, .>) and on the second (rows: <1, .>), and the mixed hyper-study; the calibrated copy rate
beside them.  Under `rocprofv3 --kernel-trace --stats -- python tools/bigshift_probe.py` the kernel_stats CSV gives the time per launch.
    python tools/bigshift_probe.py [repeats]"""
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bayesloop_amd as bl   # noqa: E402
import cases                 # noqa: E402
import bigshift_cases as bc  # noqa: E402

DET_STD_FAR = ('Deterministic', 'bs_std', 'std')
WORKLOADS = {
    'changepoints_axis0': bc.BIGSHIFT['bigshift_changepoints'],
    'changepoints_axis1': dict(bc.BIGSHIFT['bigshift_changepoints'],
                               tm=('Serial', [('Static',), ('BreakPoint', 'b1', 'all', None), DET_STD_FAR, ('BreakPoint', 'b2', 'all', None),
                                              ('GRW', 's', 0.3, 'mean', None)])),
    'hyper_mixed': bc.BIGSHIFT['bigshift_hyper_mixed'],
}


def fit_once(c):
    S = cases.build(bl, c)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
        t0 = time.perf_counter()
        S.fit(**cases.fit_kwargs(c))
        return time.perf_counter() - t0, S.logEvidence


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    eng = bl.get_engine()
    for name, c in WORKLOADS.items():
        for _ in range(3):                      # warm-up: library load, buffers, ~25 ms of load before kernels reach their steady rate
            fit_once(c)
        t = sorted(fit_once(c)[0] for _ in range(reps))
        print('%-20s fit(): median %.2f ms  min %.2f ms  (%d repeats)  logE = %.12f' % (name, 1e3 * t[len(t) // 2], 1e3 * t[0], reps, fit_once(c)[1]), flush=True)
    if hasattr(eng, 'bandwidth_probe'):
        print('copy rate (blhip_bandwidth_probe): %.0f GB/s' % eng.bandwidth_probe(1 << 30, 20), flush=True)


if __name__ == '__main__':
    main()
