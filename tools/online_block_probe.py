#!/usr/bin/env python
"""What a block of an online study costs (OnlineStudy.stepMany) beside the loop over OnlineStudy.step it replaces.  Recorded in
profiles/online_block_notes.md, not gated.

    python tools/online_block_probe.py --json OUT/probe.json [--repeats 20] [--only blocks,mix,chain1d]

blocks   stepMany(N) against `for d in data: S.step(d)` (step and the one-step route of the library are what they were before blocks existed),
         wall time of a whole replay on a fresh study, with and without history:
           (a) Poisson, 1000 cells, two models x 64 hyper-values, N = 1000;  (b) Gaussian 256 x 256, 32 chains, N = 256;
           (c) SciPy:t 5 x 18 x 14, 16 chains, N = 256;  and the same studies at N = 2, 4, 8 (the break-even)
mix      blo::mix_sequence_kernel at B T G 8 >= 256 MB: its algorithmic bytes 8 (B T G + T G) per wall time of the call, as a fraction of
         blhip_bandwidth_probe's copy rate on the same device
chain1d  forward milliseconds per step (blhip_timing.forward_ms / N) of a resumed block on bl1c::chain1d_kernel (option chain1d = 2) and on the
         K-steps-per-launch path (chain1d = 0): Poisson grids of 200 and 4608 cells, 4 and 33 chains, radii 0 .. 9

Every figure is the median of --repeats timed runs after at least 50 ms of the same work as load."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


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


def shapes(bl):
    import scipy.stats
    rng = np.random.default_rng(7)

    def poisson(history):
        S = bl.OnlineStudy(storeHistory=history, silent=True)
        S.setOM(bl.om.Poisson('rate', bl.oint(0, 8, 1000)), silent=True)
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', np.linspace(0.0, 0.3, 64).tolist(), target='rate'))
        S.addTransitionModel('switch', bl.tm.RegimeSwitch('q', np.linspace(-9, -2, 64).tolist()))
        return S

    def gauss(history):
        S = bl.OnlineStudy(storeHistory=history, silent=True)
        S.setOM(bl.om.Gaussian('mean', bl.cint(-8, 8, 256), 'std', bl.oint(0, 4, 256)), silent=True)
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', np.linspace(0.02, 0.6, 32).tolist(), target='mean'))
        return S

    def student(history):
        S = bl.OnlineStudy(storeHistory=history, silent=True)
        S.setOM(bl.om.SciPy(scipy.stats.t, 'df', bl.cint(2, 8, 5), 'loc', bl.cint(-3, 3, 18), 'scale', bl.oint(0.2, 2.5, 14)), silent=True)
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', np.linspace(0.05, 0.8, 16).tolist(), target='loc'))
        return S
    return [('a poisson 1000 cells, 2 x 64 chains', poisson, rng.poisson(3.0, 1000).astype(float)),
            ('b gaussian 256 x 256, 32 chains', gauss, rng.normal(0.0, 1.0, 256)),
            ('c scipy t 5 x 18 x 14, 16 chains', student, rng.standard_t(4.0, 256) * 0.8)]


def run_blocks(bl, repeats, emit):
    for name, make, data in shapes(bl):
        for history in (False, True):
            for N in (2, 4, 8, len(data)):
                x = data[:N]

                def block():
                    S = quiet(make, history)
                    S.BLOCK_MIN_POINTS = 1          # (the block itself at every N: the break-even is what is measured)
                    quiet(S.stepMany, x)

                def loop():
                    S = quiet(make, history)
                    with contextlib.redirect_stdout(io.StringIO()):
                        for d in x:
                            S.step(d)
                tb, tl = median_time(block, repeats), median_time(loop, repeats)
                emit(dict(what='blocks', shape=name, history=history, N=N, block_ms=1e3 * tb, loop_ms=1e3 * tl, speedup=tl / tb))


def run_mix(bl, repeats, emit):
    from bayesloop_amd import _abi
    from bayesloop_amd.engine import FitProblem
    eng = bl.get_engine()
    n, B, T = 256, 64, 32
    G = n * n
    mean, std = np.linspace(-8, 8, n), np.linspace(0.02, 4, n)
    problem = FitProblem(obs_model=_abi.OM_GAUSSIAN, marginal=[mean, std], lattice=[mean[1] - mean[0], std[1] - std[0]],
                         data=np.random.default_rng(1).normal(0, 1, (T, 1)), timestamps=np.arange(T, dtype=float), prior=np.full(G, 1.0 / G),
                         ops=[(_abi.OP_GRW, 0, -1, 0)])
    eng.fit(problem, np.linspace(0.05, 0.6, B).reshape(B, 1), forward_only=True, keep_posterior=True)
    w = np.random.default_rng(2).uniform(0, 1, (T, B))
    t = median_time(lambda: eng.mix_sequence(w), repeats)
    copy = eng.bandwidth_probe()
    rate = 8.0 * (B * T * G + T * G) / t / 1e9
    emit(dict(what='mix', B=B, T=T, G=G, sequence_MB=8.0 * B * T * G / 1e6, call_us=1e6 * t, GB_per_s=rate, copy_GB_per_s=copy, fraction=rate / copy))


def run_chain1d(bl, repeats, emit):
    eng = bl.get_engine()
    N = 256
    data = np.random.default_rng(3).poisson(3.0, N + 1).astype(float)
    for n in (200, 4608):
        for chains in (4, 33):
            for mode in (2, 0):
                eng.set_option('chain1d', mode)
                try:
                    ms = []

                    def work():
                        S = bl.OnlineStudy(silent=True)
                        S.setOM(bl.om.Poisson('rate', bl.oint(0, 8, n)), silent=True)
                        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', (np.linspace(0.0, 2.2, chains) * 8.0 / (n + 1)).tolist(), target='rate'))
                        S.step(data[0])
                        S.stepMany(data[1:])
                        ms.append(eng.last_timing()['forward_ms'])
                    quiet(median_time, work, repeats)
                    emit(dict(what='chain1d', n=n, chains=chains, chain1d=mode, variant=eng.last_timing()['fwd_kernel_variant'],
                              forward_us_per_step=1e3 * float(np.median(ms[-repeats:])) / N))
                finally:
                    eng.set_option('chain1d', 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', default='blocks,mix,chain1d')
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
    if 'mix' in only:
        run_mix(bl, args.repeats, emit)
    if 'chain1d' in only:
        run_chain1d(bl, args.repeats, emit)
    if 'blocks' in only:
        run_blocks(bl, args.repeats, emit)


if __name__ == '__main__':
    main()
