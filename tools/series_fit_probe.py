"""Many short series on a one-parameter grid: Study.fitMany (one device call per batch of series, a chain of the chain-resident 1-D kernel per
series) against the user's loop `for d in series: S.loadData(d); S.fit()`.  The shape is BASELINE C1's: a Poisson rate on 200 cells, 110 steps,
a GaussianRandomWalk of radius 27.  Full fits and evidenceOnly, for 1, 2, 4, 16, 256 and 4096 series; medians of repeated calls after a warm-up,
every call ended by a device synchronise.  profiles/series_fit_notes.md holds what it measured.

    python tools/series_fit_probe.py --mode many                      # fitMany of this tree
    python tools/series_fit_probe.py --mode loop --package-dir DIR    # the loop, with the bayesloop_amd package under DIR (another commit's build)

One JSON line per (count, flavour): {"mode", "series", "flavour", "median_ms", "min_ms", "max_ms", "reps", "per_series_us"}."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--mode', choices=('many', 'loop'), required=True)
ap.add_argument('--package-dir', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--counts', default='1,2,4,16,256,4096')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--budget-s', type=float, default=12.0, help='fewer repetitions (at least 3) where one call is long')
ap.add_argument('--out', default='')
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_dir))
import bayesloop_amd as bl  # noqa: E402

N, T, SIGMA = 200, 110, 0.2          # 4 sigma / lattice + 0.5 = 27 cells
eng = bl.get_engine()
rng = np.random.RandomState(1852)
pool = [rng.poisson(1.0 + 2.0 * rng.uniform(), size=T).astype(float) for _ in range(4096)]


def study():
    S = bl.Study(silent=True)
    S.set(bl.om.Poisson('rate', bl.oint(0, 6, N)), bl.tm.GaussianRandomWalk('sigma', SIGMA, target='rate'), silent=True)
    return S


def call(S, series, kw):
    if args.mode == 'many':
        R = S.fitMany(series, silent=True, **kw)
        eng.synchronize()
        return float(R.logEvidence[-1])
    for d in series:
        S.loadData(d, silent=True)
        S.fit(silent=True, **kw)
    eng.synchronize()
    return float(S.logEvidence)


rows = []
for count in [int(c) for c in args.counts.split(',')]:
    series = pool[:count]
    for flavour, kw in (('full', {}), ('evidenceOnly', dict(evidenceOnly=True))):
        S = study()
        t0 = time.perf_counter()
        last = call(S, series, kw)                     # warm-up: code objects, buffers of this shape
        warm = time.perf_counter() - t0
        reps = max(3, min(args.reps, int(args.budget_s / max(warm, 1e-6))))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call(S, series, kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        row = dict(mode=args.mode, series=count, flavour=flavour, median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts), reps=reps,
                   per_series_us=float(np.median(ts)) * 1e3 / count, last_log_evidence=last,
                   kernel=getattr(S, 'lastTiming', {}).get('fwd_kernel_variant') if args.mode == 'loop' else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
