#!/usr/bin/env python
"""What a probability query of the parser at every time step costs in one call -- ``P(query, t='all')`` -- beside the loop over the scalar
call it replaces, ``[P(query, t=t, silent=True) for t in stamps]`` (the scalar call is the code it was before vector time stamps existed:
a row of the sequence is copied, the values and the sums are NumPy's).  Recorded in profiles/parser_query_notes.md, not gated.

    python tools/parser_query_probe.py --json OUT/probe.json [--repeats 9] [--only rows,pairs,sweep]

rows    one space: 2-D Gaussian studies at 256 x 256 and 512 x 512 with ``mean/std > 1`` and the series form ``(mean - c)/std > 1``, a
        1000-cell Poisson study with ``rate < 3``.  Beside the wall time of the public call: the entry point alone
        (HipEngine.posterior_query with the plan already made) and the bytes of the sequence it reads, T G 8, per that time, next to
        blhip_bandwidth_probe's copy rate on the same device.
pairs   two spaces: two 1000-cell studies with ``rate*rate2 >= 4``; a HyperStudy with ``mean*sigma > 0.5`` (parameter x hyper-parameter).
sweep   the pair kernel against the loop over pair spaces of n x n cells, n = 50 .. 8000: where option parser_pair_max comes from.

The loop is timed on at most --loop-stamps time stamps and scaled to all of them (every stamp costs the same).  Every figure is the
median of --repeats timed runs after at least 50 ms of the same work as load."""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def poisson(bl, n, T, name='rate', walk=True):
    S = bl.Study()
    S.loadData(np.random.default_rng(T + n).poisson(3.0, T))
    S.setOM(bl.om.Poisson(name, bl.oint(0, 6, n)))
    S.setTM(bl.tm.GaussianRandomWalk('sigma_' + name, 0.2, target=name) if walk else bl.tm.Static())
    S.fit()
    return S


def compare(P, query, series, repeats, loop_stamps, emit, row, pair_max=None):
    stamps = P._stamps('all')
    series = series or {}
    got = P(query, t='all', silent=True, series=series or None)
    pick = np.unique(np.linspace(0, len(stamps) - 1, min(loop_stamps, len(stamps))).astype(int))

    def text(i):
        q = query
        for name, v in series.items():
            q = re.sub(r'\b%s\b' % name, repr(float(v[i])), q)
        return q

    def loop():
        return [P(text(i), t=stamps[i], silent=True) for i in pick]
    want = np.array(loop())
    err = float(np.max(np.abs(got[pick] - want)))
    t_call = median_time(lambda: P(query, t='all', silent=True, series=series or None), repeats)
    t_loop = median_time(loop, max(1, repeats // 3), load_s=0.0) * len(stamps) / len(pick)
    plan = P.plan(query, 'all', series or None)
    pending = plan.study._posterior_pending
    t_dev = median_time(lambda: pending.query(plan.steps, plan.ops, plan.consts, plan.relation, plan.marginal, **plan.spaces_kwargs()), repeats)
    G = int(np.prod([len(m) for m in plan.marginal]))
    row = dict(row, query=query, T=len(stamps), G=G, call_ms=1e3 * t_call, loop_ms=1e3 * t_loop, loop_stamps_timed=len(pick), speedup=t_loop / t_call,
               entry_ms=1e3 * t_dev, max_abs_difference=err)
    if plan.b_prob is None:
        row['sequence_GB_per_s'] = 8.0 * len(stamps) * G / t_dev / 1e9
    else:
        row['G_b'] = int(plan.b_prob.shape[1])
        row['pairs_per_s'] = float(len(stamps)) * G * row['G_b'] / t_dev
    emit(row)


def run_rows(bl, args, emit):
    copy = bl.get_engine().bandwidth_probe()
    for n, T in ((256, 256), (512, 256)):
        S = quiet(gaussian, bl, n, T)
        P = quiet(bl.Parser, S)
        c = 0.4 + 0.002 * np.arange(T)
        compare(P, 'mean/std > 1', None, args.repeats, args.loop_stamps, emit, dict(what='rows', study='gaussian %d x %d' % (n, n), copy_GB_per_s=copy))
        compare(P, '(mean - c)/std > 1', {'c': c}, args.repeats, args.loop_stamps, emit, dict(what='rows', study='gaussian %d x %d, series' % (n, n), copy_GB_per_s=copy))
    S = quiet(poisson, bl, 1000, 1000)
    compare(quiet(bl.Parser, S), 'rate < 3', None, args.repeats, args.loop_stamps, emit, dict(what='rows', study='poisson 1000', copy_GB_per_s=copy))


def run_pairs(bl, args, emit):
    S, S2 = quiet(poisson, bl, 1000, 200, 'rate', False), quiet(poisson, bl, 1000, 200, 'rate2')
    compare(quiet(bl.Parser, S, S2), 'rate*rate2 >= 4', None, args.repeats, args.loop_stamps, emit, dict(what='pairs', study='two poisson 1000'))
    H = bl.HyperStudy()
    H.loadData(np.random.default_rng(5).normal(1.0, 0.8, 64))
    H.setOM(bl.om.Gaussian('mean', bl.cint(-1, 3, 64), 'std', bl.oint(0, 2, 64)))
    H.setTM(bl.tm.GaussianRandomWalk('sigma', bl.cint(0, 0.4, 16), target='mean'))
    quiet(H.fit)
    compare(quiet(bl.Parser, H), 'mean*sigma > 0.5', None, args.repeats, args.loop_stamps, emit, dict(what='pairs', study='hyper 64 x 64, 16 hyper values'))


def run_sweep(bl, args, emit):
    eng = bl.get_engine()
    eng.set_option('parser_pair_max', 1e30)
    for n, T in ((50, 64), (300, 64), (1000, 64), (3000, 32), (8000, 16)):
        S, S2 = quiet(poisson, bl, n, T, 'rate', False), quiet(poisson, bl, n, T, 'rate2')
        compare(quiet(bl.Parser, S, S2), 'rate*rate2 >= 4', None, max(3, args.repeats // 3), min(args.loop_stamps, 4 if n >= 3000 else 16), emit,
                dict(what='sweep', study='two poisson %d' % n, pair_space=n * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--loop-stamps', type=int, default=16)
    ap.add_argument('--only', default='rows,pairs,sweep')
    args = ap.parse_args()
    import bayesloop_amd as bl
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(rows, f, indent=1)
    only = args.only.split(',')
    if 'rows' in only:
        run_rows(bl, args, emit)
    if 'pairs' in only:
        run_pairs(bl, args, emit)
    if 'sweep' in only:
        run_sweep(bl, args, emit)


if __name__ == '__main__':
    main()
