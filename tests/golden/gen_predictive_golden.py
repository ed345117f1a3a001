#!/usr/bin/env python
"""
Generates tests/golden/predictive.npz by IMPORTING THE REFERENCE (see gen_golden.py, whose shims and case builder this uses): the
reference's own ``simulate`` (core.py:566-597) looped over EVERY time stamp of a fitted study, with ``density`` False and True -- what
``simulate(x, t='all')`` of bayesloop_amd returns in one call.  The three cases of simulate.npz (a Study on the coal-mining counts, a
two-parameter Gaussian Study, a HyperStudy on a two-parameter grid: its average posterior) plus a HyperStudy on the one-parameter Poisson
grid.  Run:  python tests/golden/gen_predictive_golden.py

The fixture is data only: the observation values and the reference's outputs, (T, len(x)) per case and density.
"""
import contextlib
import io
import os

import numpy as np

import gen_golden as gg          # (installs the shims, imports the reference as gg.bl)
from predictive_cases import GOLDEN_X

HERE = os.path.dirname(os.path.abspath(__file__))


def run():
    out = {}
    for case, x in GOLDEN_X.items():
        S = gg.cases.build(gg.bl, case)
        with contextlib.redirect_stdout(io.StringIO()):
            with np.errstate(all='ignore'):
                S.fit(**gg.cases.fit_kwargs(case))
        out[case + '_x'] = np.asarray(x, dtype=float)
        out[case + '_t'] = np.asarray(S.formattedTimestamps, dtype=float)
        for density in (False, True):
            with np.errstate(all='ignore'):
                rows = [np.asarray(S.simulate(x, t=t, density=density), dtype=float) for t in S.formattedTimestamps]
            out[case + ('_density' if density else '_prob')] = np.array(rows)
    return out


if __name__ == '__main__':
    path = os.path.join(HERE, 'predictive.npz')
    np.savez_compressed(path, **run())
    print('predictive.npz written, %.1f kB' % (os.path.getsize(path) / 1e3))
