#!/usr/bin/env python
"""
Generates tests/golden/parser_series.npz by IMPORTING THE REFERENCE (see gen_golden.py, whose shims this uses): for every case of
tests/parser_series_cases.py the reference's own loop over the time stamps of the first study,

    [P(query, t=t, silent=True) for t in stamps]

-- what ``P(query, t='all')`` of bayesloop_amd returns in one call.  A series is formatted into the query with ``repr``, step by step, as
the tutorials do (probabilityparser.ipynb: ``'(mu - ' + str(mu0[t]) + ')/sigma > 1'``).  A case the reference's evaluator trips on is
recorded as ``<case>_raises``.  Run:  python tests/golden/gen_parser_series_golden.py

While writing, the generator checks the condition the device tests rest on: for the queries whose device program calls exp / pow, no grid
cell lies within 1e-6 (relative) of the threshold, so an ulp of difference between two libms cannot flip an indicator.

The fixture is data only: the time stamps and the reference's probabilities, (T,) per case.
"""
import os
import sys

import numpy as np

import gen_golden as gg          # (installs the shims, imports the reference as gg.bl)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # (the cases share their small studies with tests/test_parser.py, which imports this package)
import parser_series_cases as psc      # noqa: E402


def check_margins(S):
    mean, std = np.ravel(S.grid[0]), np.ravel(S.grid[1])
    with np.errstate(all='ignore'):
        for lhs, rhs in ((np.exp(mean / std), 2.0), (std ** mean, 1.0)):
            gap = np.abs(lhs - rhs) / np.maximum(1.0, np.maximum(np.abs(lhs), abs(rhs)))
            assert np.nanmin(gap) >= 1e-6, np.nanmin(gap)


def run():
    out, built = {}, {}
    for name, (studies, query, series, _, _) in psc.CASES.items():
        if studies not in built:
            built[studies] = psc.BUILDERS[studies](gg.bl)
            if studies == 'gauss':
                check_margins(built[studies][0])
        S = built[studies]
        stamps = list(S[0].formattedTimestamps)
        out[name + '_t'] = np.asarray(stamps, dtype=float)
        with psc._quiet():
            P = gg.bl.Parser(*S)
            try:
                out[name] = np.array([P(psc.textual(query, series, i), t=t, silent=True) for i, t in enumerate(stamps)], dtype=float)
            except (ValueError, TypeError, IndexError):
                out[name + '_raises'] = np.bool_(True)
    return out


if __name__ == '__main__':
    path = os.path.join(HERE, 'parser_series.npz')
    rec = run()
    np.savez_compressed(path, **rec)
    print('parser_series.npz written, %.1f kB; raised: %s' % (os.path.getsize(path) / 1e3, [k for k in rec if k.endswith('_raises')]))
