"""Many data series, one study: Study.fitMany (one device call per batch of series, a chain of a chain-resident kernel per series) against the
user's loop `for d in series: S.loadData(d); S.fit()`.  Medians of repeated calls after a warm-up, every call ended by a device synchronise.

Cases (--case):
    c1          BASELINE C1's shape: a Poisson rate on 200 cells, 110 steps, a GaussianRandomWalk of radius 27; 1 .. 4096 series
                (profiles/series_fit_notes.md holds what it measured)
    gauss_mean  a 200 x 200 Gaussian study, 500 steps, a walk on the mean (blc::chain_kernel); 2 .. 512 series
    gauss_both  ... walks on both parameters (blc::chainax_kernel)
    scaled_ar1  a 100 x 100 ScaledAR1 study, 500 steps, a walk on the correlation coefficient (blc::chain_kernel, a table per chain)
                (profiles/series_fit_2d_notes.md)
    hyper1d     C1's shape under a HyperStudy: sigma over cint(0, 1, 20), a group of 20 chains per series folded into its own average
                (HyperStudy.fitMany against the loop over HyperStudy.fit; profiles/series_fit_hyper_notes.md); 2 .. 512 series.  Its rows
                carry accumulate_ms, the grouped fold's launch of the last batch.

    python tools/series_fit_probe.py --mode many                      # fitMany of this tree
    python tools/series_fit_probe.py --mode off                       # fitMany with option series_fit = 0: its loop, on the same build
    python tools/series_fit_probe.py --mode loop --package-dir DIR    # the user's loop, with the bayesloop_amd package under DIR (another commit's build)

Full fits keep every series' posterior sequence on the host (a 200 x 200 x 500 sequence is 160 MB): --full-max bounds the counts they run for.
One JSON line per (count, flavour): {"case", "mode", "series", "flavour", "median_ms", "min_ms", "max_ms", "reps", "per_series_us"}."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--mode', choices=('many', 'off', 'loop'), required=True)
ap.add_argument('--case', choices=('c1', 'gauss_mean', 'gauss_both', 'scaled_ar1', 'hyper1d'), default='c1')
ap.add_argument('--package-dir', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--counts', default='')
ap.add_argument('--flavours', default='full,evidenceOnly')
ap.add_argument('--full-max', type=int, default=0, help='largest count full fits run for (0: 4096 for c1, 8 for the two-parameter cases)')
ap.add_argument('--steps', type=int, default=0, help='time steps (0: the case\'s own)')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--budget-s', type=float, default=12.0, help='fewer repetitions (at least 3) where one call is long')
ap.add_argument('--out', default='')
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_dir))
import bayesloop_amd as bl  # noqa: E402

eng = bl.get_engine()
rng = np.random.RandomState(1852)
two = args.case not in ('c1', 'hyper1d')
counts = [int(c) for c in (args.counts or ('2,8,64,512' if two or args.case == 'hyper1d' else '1,2,4,16,256,4096')).split(',')]
full_max = args.full_max or (8 if two else 4096)

if args.case == 'hyper1d':
    N, T = 200, args.steps or 110
    pool = [rng.poisson(1.0 + 2.0 * rng.uniform(), size=T).astype(float) for _ in range(max(counts))]

    def study():
        S = bl.HyperStudy(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, N)), bl.tm.GaussianRandomWalk('sigma', bl.cint(0, 1, 20), target='rate'), silent=True)
        return S
elif args.case == 'c1':
    N, T, SIGMA = 200, args.steps or 110, 0.2          # 4 sigma / lattice + 0.5 = 27 cells
    pool = [rng.poisson(1.0 + 2.0 * rng.uniform(), size=T).astype(float) for _ in range(max(counts))]

    def study():
        S = bl.Study(silent=True)
        S.set(bl.om.Poisson('rate', bl.oint(0, 6, N)), bl.tm.GaussianRandomWalk('sigma', SIGMA, target='rate'), silent=True)
        return S
elif args.case in ('gauss_mean', 'gauss_both'):
    N, T = 200, args.steps or 500
    pool = [rng.normal(0.5 * rng.uniform(-1, 1), 0.8 + 0.4 * rng.uniform(), size=T) for _ in range(max(counts))]

    def study():
        S = bl.Study(silent=True)
        walk = bl.tm.GaussianRandomWalk('sigma', 0.1, target='mean')             # radius 4 sigma / lattice: 20 cells
        if args.case == 'gauss_both':
            walk = bl.tm.CombinedTransitionModel(walk, bl.tm.GaussianRandomWalk('sigma2', 0.05, target='std'))      # ... and 20 cells
        S.set(bl.om.Gaussian('mean', bl.cint(-2, 2, N), 'std', bl.oint(0, 2, N)), walk, silent=True)
        return S
else:
    N, T = 100, args.steps or 500
    pool = []
    for _ in range(max(counts)):
        rho, x = rng.uniform(-0.8, 0.8), [0.0]
        for _t in range(T):
            x.append(rho * x[-1] + np.sqrt(1.0 - rho * rho) * rng.normal())
        pool.append(np.array(x))

    def study():
        S = bl.Study(silent=True)
        S.set(bl.om.ScaledAR1('rho', bl.oint(-1, 1, N), 'sigma', bl.oint(0, 3, N)), bl.tm.GaussianRandomWalk('sigma', 0.1, target='rho'), silent=True)
        return S

if args.mode == 'off':
    eng.set_option('series_fit', 0)


def call(S, series, kw):
    if args.mode != 'loop':
        R = S.fitMany(series, silent=True, **kw)
        eng.synchronize()
        return float(R.logEvidence[-1]), R.lastTiming
    for d in series:
        S.loadData(d, silent=True)
        S.fit(silent=True, **kw)
    eng.synchronize()
    return float(S.logEvidence), S.lastTiming


rows = []
for count in counts:
    series = pool[:count]
    for flavour in args.flavours.split(','):
        kw = dict(evidenceOnly=True) if flavour == 'evidenceOnly' else {}
        if flavour == 'full' and count > full_max:
            continue
        S = study()
        t0 = time.perf_counter()
        last, timing = call(S, series, kw)             # warm-up: code objects, buffers of this shape
        warm = time.perf_counter() - t0
        reps = max(3, min(args.reps, int(args.budget_s / max(warm, 1e-6))))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call(S, series, kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        row = dict(case=args.case, mode=args.mode, series=count, flavour=flavour, median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts),
                   reps=reps, per_series_us=float(np.median(ts)) * 1e3 / count, last_log_evidence=last,
                   kernel=(timing or {}).get('fwd_kernel_variant'), batches=(timing or {}).get('batches'),
                   accumulate_ms=(timing or {}).get('accumulate_ms'))
        rows.append(row)
        print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
