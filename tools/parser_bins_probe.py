#!/usr/bin/env python
"""What a distribution query of the parser at every time step costs in one call -- ``P('mean/std', t='all')`` -- beside the loop over the
scalar call it replaces.  The loop is the path of the commit before: the SAME process with engine option parser_device = 0, under which
``P(query, t=stamps)`` is ``[P(query, t=t, silent=True) for t in stamps]`` (a row of the sequence is copied, the values are re-evaluated,
re-sorted and binned per stamp).  Recorded in profiles/parser_bins_notes.md, not gated.

    python tools/parser_bins_probe.py --json OUT/probe.json [--repeats 9] [--only sizes,shapes,few]

sizes   512 x 512 Gaussian, T = 256: ``mean/std`` (510 bins, 1 .. 131 841 cells), ``mean + std`` (2562 bins of at most 129 cells),
        ``log(mean)`` (5 bins, half the cells left out); 100 x 100, T = 500; Poisson, 1000 cells, T = 1000.  Beside the wall time of the
        public call: the entry point alone (HipEngine.posterior_bins with the plan already made: the order of the map on the host, the
        uploads, the two kernels, the read-back) and the bytes of the sequence it reads, T G 8, per that time, next to
        blhip_bandwidth_probe's copy rate on the same device.
shapes  the entry point alone under other slab lengths, steps per block and group widths (options bins_slab, bins_sb, bins_gw).
few     1, 2, 3, 4, 8 time stamps: the device path (Parser._device_distribution, whatever parser.DIST_MIN_STAMPS says) against the loop.

The loop is timed on at most --loop-stamps time stamps and scaled to all of them (every stamp costs the same).  Every figure is the
median of --repeats timed runs after at least 50 ms of the same work as load."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((512, 8, 8), (1024, 8, 8), (256, 8, 8), (512, 16, 8), (512, 4, 8), (512, 8, 4), (512, 8, 16))


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def median_time(work, repeats, load_s=0.05):
    t_end = time.perf_counter() + load_s
    work()
    while time.perf_counter() < t_end:
        work()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        work()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def gaussian(bl, n, T):
    S = bl.Study()
    S.loadData(np.random.default_rng(n).normal(1.0, 0.8, T) + np.linspace(-0.5, 0.9, T))
    S.setOM(bl.om.Gaussian('mean', bl.cint(-1, 3, n), 'std', bl.oint(0, 2, n)))
    S.setTM(bl.tm.GaussianRandomWalk('s1', 0.15, target='mean'))
    S.fit()
    return S


def poisson(bl, n, T):
    S = bl.Study()
    S.loadData(np.random.default_rng(T + n).poisson(3.0, T))
    S.setOM(bl.om.Poisson('rate', bl.oint(0, 6, n)))
    S.setTM(bl.tm.GaussianRandomWalk('sigma', 0.2, target='rate'))
    S.fit()
    return S


def loop_of(P, eng, query, stamps):
    """the loop over the scalar call through the public call, as the commit before ran it"""
    def work():
        eng.set_option('parser_device', 0.0)
        try:
            return P(query, t=stamps, silent=True)
        finally:
            eng.set_option('parser_device', 1.0)
    return work


def compare(bl, P, query, args, emit, row):
    eng = bl.get_engine()
    stamps = P._stamps('all')
    with np.errstate(all='ignore'):
        got = P(query, t='all', silent=True)
        pick = np.unique(np.linspace(0, len(stamps) - 1, min(args.loop_stamps, len(stamps))).astype(int))
        loop = loop_of(P, eng, query, [stamps[i] for i in pick])
        want = loop()
        err = max(float(np.max(np.abs(got[i][1] - w[1]))) for i, w in zip(pick, want))
        assert all(np.array_equal(got[i][0], w[0]) for i, w in zip(pick, want))
        t_call = median_time(lambda: P(query, t='all', silent=True), args.repeats)
        t_loop = median_time(loop, max(1, args.repeats // 3), load_s=0.0) * len(stamps) / len(pick)
        plan = P.planDistribution(query, 'all')
    pending = plan.study._posterior_pending
    t_dev = median_time(lambda: pending.bins(plan.steps, plan.bin, plan.n_bins), args.repeats)
    counts = np.bincount(plan.bin[plan.bin >= 0], minlength=plan.n_bins)
    row = dict(row, query=query, T=len(stamps), G=int(plan.bin.size), n_bins=plan.n_bins, largest_bin=int(counts.max()), left_out=int((plan.bin < 0).sum()),
               call_ms=1e3 * t_call, loop_ms=1e3 * t_loop, loop_stamps_timed=len(pick), speedup=t_loop / t_call, entry_ms=1e3 * t_dev,
               sequence_GB_per_s=8.0 * len(stamps) * plan.bin.size / t_dev / 1e9, max_abs_difference=err)
    emit(row)
    return plan, pending


def run_sizes(bl, args, emit, studies):
    copy = bl.get_engine().bandwidth_probe()
    for key, queries in (('gaussian 512 x 512', ('mean/std', 'mean + std', 'log(mean)')), ('gaussian 100 x 100', ('mean/std',)), ('poisson 1000', ('rate*2', 'rate^2'))):
        P = quiet(bl.Parser, studies[key])
        for query in queries:
            compare(bl, P, query, args, emit, dict(what='sizes', study=key, copy_GB_per_s=copy))


def run_shapes(bl, args, emit, studies):
    eng = bl.get_engine()
    for key, queries in (('gaussian 512 x 512', ('mean/std', 'mean + std', 'log(mean)')), ('poisson 1000', ('rate*2',))):
        P = quiet(bl.Parser, studies[key])
        for query in queries:
            with np.errstate(all='ignore'):
                plan = P.planDistribution(query, 'all')
            pending = plan.study._posterior_pending
            base = None
            for slab, sb, gw in SHAPES:
                try:
                    for k, v in (('bins_slab', slab), ('bins_sb', sb), ('bins_gw', gw)):
                        eng.set_option(k, v)
                    out = pending.bins(plan.steps, plan.bin, plan.n_bins)
                    t = median_time(lambda: pending.bins(plan.steps, plan.bin, plan.n_bins), args.repeats)
                finally:
                    for k, v in (('bins_slab', SHAPES[0][0]), ('bins_sb', SHAPES[0][1]), ('bins_gw', SHAPES[0][2])):
                        eng.set_option(k, v)
                base = out if base is None else base
                emit(dict(what='shapes', study=key, query=query, slab=slab, sb=sb, gw=gw, entry_ms=1e3 * t,
                          sequence_GB_per_s=8.0 * plan.steps.size * plan.bin.size / t / 1e9, max_abs_difference_to_default=float(np.max(np.abs(out - base)))))


def run_few(bl, args, emit, studies):
    eng = bl.get_engine()
    for key, query in (('gaussian 512 x 512', 'mean/std'), ('gaussian 100 x 100', 'mean/std'), ('poisson 1000', 'rate*2'), ('poisson 50', 'rate*2')):
        P = quiet(bl.Parser, studies[key])
        stamps = P._stamps('all')
        for n in (1, 2, 3, 4, 8):
            t = [stamps[i] for i in np.linspace(0, len(stamps) - 1, n).astype(int)]
            with np.errstate(all='ignore'):
                assert P._device_distribution(query, t, {}) is not None
                t_dev = median_time(lambda: P._device_distribution(query, t, {}), args.repeats)
                t_loop = median_time(loop_of(P, eng, query, t), args.repeats)
            emit(dict(what='few', study=key, query=query, stamps=n, device_ms=1e3 * t_dev, loop_ms=1e3 * t_loop, speedup=t_loop / t_dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--loop-stamps', type=int, default=8)
    ap.add_argument('--only', default='sizes,shapes,few')
    args = ap.parse_args()
    import bayesloop_amd as bl
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(rows, f, indent=1)
    # every study keeps its sequence on the device only while it is the last one fitted: one at a time
    makers = {'gaussian 512 x 512': lambda: gaussian(bl, 512, 256), 'gaussian 100 x 100': lambda: gaussian(bl, 100, 500),
              'poisson 1000': lambda: poisson(bl, 1000, 1000), 'poisson 50': lambda: poisson(bl, 50, 100)}

    class Lazy(dict):
        def __missing__(self, key):
            self.clear()
            self[key] = quiet(makers[key])
            return self[key]
    studies = Lazy()
    only = args.only.split(',')
    if 'sizes' in only:
        run_sizes(bl, args, emit, studies)
    if 'shapes' in only:
        run_shapes(bl, args, emit, studies)
    if 'few' in only:
        run_few(bl, args, emit, studies)


if __name__ == '__main__':
    main()
