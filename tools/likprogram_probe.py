#!/usr/bin/env python
"""What the likelihood programs cost: table-build time of bllp::lik_program_kernel for SymPy Normal and Laplace on 512 x 512 x 256 steps and
Frechet on 64^3 x 256, beside the host table it replaces (evaluation + upload) and, as the yardstick that already exists,
blk::lik_table_kernel for the built-in Laplace on the same grid.  Recorded in profiles/likprogram_notes.md, not gated.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/likprogram_probe.py --json OUT/probe.json
    python tools/likprogram_probe.py --kernel-trace OUT --json OUT/probe.json

The first command runs the fits (>= 50 ms of warm-up fits, then --fits >= 20 timed ones per configuration: one launch of the table kernel
per fit) and prints the host-side figures: wall time of the host evaluation, of a fit with the host table and of a fit with the program.
The second reads the kernel trace and prints the median duration per kernel and configuration (launches are attributed in order: every
configuration launches its table kernel exactly warm-up + fits times)."""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def studies(bl):
    import sympy
    import sympy.stats as st
    rng = np.random.RandomState(1)
    real, pos = 0.5 + rng.randn(256), 0.3 + rng.gamma(2.0, 0.7, 256)
    mu, s, a, m = sympy.Symbol('mu'), sympy.Symbol('s', positive=True), sympy.Symbol('a', positive=True), sympy.Symbol('m')

    def make(om, data):
        S = bl.Study()
        S.loadData(data, silent=True)
        S.setOM(om, silent=True)
        S.setTM(bl.tm.Static(), silent=True)
        return S
    with contextlib.redirect_stdout(io.StringIO()):
        return [
            ('SymPy Normal 512x512x256', 'program', lambda: make(bl.om.SymPy(st.Normal('rv', mu, s), 'mu', bl.cint(-3, 4, 512), 's', bl.oint(0, 3, 512), determineJeffreysPrior=False), real)),
            ('SymPy Laplace 512x512x256', 'program', lambda: make(bl.om.SymPy(st.Laplace('rv', mu, s), 'mu', bl.cint(-3, 4, 512), 's', bl.oint(0, 3, 512), determineJeffreysPrior=False), real)),
            ('SymPy Frechet 64x64x64x256', 'program', lambda: make(bl.om.SymPy(st.Frechet('rv', a, s, m), 'a', bl.cint(1, 4, 64), 's', bl.cint(0.5, 3, 64), 'm', bl.cint(-1.5, 0.2, 64), determineJeffreysPrior=False), pos)),
            ('built-in Laplace 512x512x256', 'closed form', lambda: make(bl.om.Laplace('mu', bl.cint(-3, 4, 512), 's', bl.oint(0, 3, 512)), real)),
        ]


def run(args):
    import bayesloop_amd as bl
    eng = bl.get_engine()
    record = []
    for name, kind, make in studies(bl):
        with contextlib.redirect_stdout(io.StringIO()):
            S = make()

            def fit():
                t0 = time.perf_counter()
                S.fit(evidenceOnly=True, silent=True)
                return (time.perf_counter() - t0) * 1e3
            warm, spent = 0, 0.0
            while spent < 50.0 or warm < 2:                   # >= 50 ms of warm-up
                spent += fit()
                warm += 1
            wall = sorted(fit() for _ in range(args.fits))
            row = dict(name=name, kind=kind, launches=warm + args.fits, warmup=warm, fit_ms=wall[len(wall) // 2])
            if kind == 'program':
                eng.set_option('lik_program', 0)
                try:
                    S._formatData()
                    t0 = time.perf_counter()
                    S._compile()
                    row['host_eval_ms'] = (time.perf_counter() - t0) * 1e3
                    host = sorted(fit() for _ in range(3))
                    row['host_fit_ms'] = host[1]
                finally:
                    eng.set_option('lik_program', 1)
        record.append(row)
        print('%-30s fit %8.1f ms' % (name, row['fit_ms']) + ('   host table: evaluation %8.1f ms, fit (evaluation + upload + passes) %8.1f ms'
                                                               % (row['host_eval_ms'], row['host_fit_ms']) if kind == 'program' else ''))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(record, f, indent=1)


def summarize(args):
    record = json.load(open(args.json))
    rows = []
    for path in glob.glob(os.path.join(args.kernel_trace, '**', '*kernel_trace.csv'), recursive=True):
        with open(path) as f:
            rows += [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(f)]
    rows.sort()
    for family, kind in (('lik_program_kernel', 'program'), ('lik_table_kernel', 'closed form')):
        dur = [(e - s) / 1e3 for s, e, n in rows if family in n and 'ax_lik' not in n and 'lik1d' not in n]
        at = 0
        for r in record:
            if r['kind'] != kind:
                continue
            mine = sorted(dur[at + r['warmup']:at + r['launches']])
            at += r['launches']
            if mine:
                cells = 512 * 512 * 256
                print('%-30s %-20s median of %d launches %9.1f us  (%.2f ps per cell, %.0f GB/s of table written)'
                      % (r['name'], family, len(mine), mine[len(mine) // 2], mine[len(mine) // 2] * 1e6 / cells, cells * 8 / mine[len(mine) // 2] / 1e3))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--fits', type=int, default=22)
    ap.add_argument('--json', default=None)
    ap.add_argument('--kernel-trace', default=None)
    a = ap.parse_args()
    summarize(a) if a.kernel_trace else run(a)
