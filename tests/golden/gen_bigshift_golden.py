#!/usr/bin/env python
"""
Generates the fixtures of tests/bigshift_cases.py (Deterministic shifts beyond 12 cells per step on 2-D grids) under tests/golden/ by
IMPORTING THE REFERENCE, exactly as gen_combined_golden.py does (its `run`, gen_golden.run_online; the direct calls as
gen_plugin_golden.py makes them: the reference model's own computeForwardPrior / computeBackwardPrior).  CPU only.
Run:  python tests/golden/gen_bigshift_golden.py [case ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_combined_golden as gcg   # noqa: E402  (imports gen_golden: the shims, the reference as gen_golden.bl)
import gen_golden                   # noqa: E402
import cases                        # noqa: E402
import bigshift_cases as bc         # noqa: E402

bl = gen_golden.bl


def run_direct():
    out = {}
    for name, (S, model) in bc.direct_calls(bl).items():
        S.setTransitionModel(model, silent=True)
        for k, (method, kind, t) in enumerate(bc.DIRECT_CALLS):
            x = bc.distribution(kind, S.gridSize, seed=k)
            fn = model.computeForwardPrior if method == 'fwd' else model.computeBackwardPrior
            out['%s/%d' % (name, k)] = np.asarray(fn(x.copy(), t), dtype=float)
    return out


def run_fit(c):
    """gen_combined_golden.run with the whole posterior sequence, then thinned here: the rows of cases.sparse_rows at a stride that keeps at
    most 4000 cells per row, plus both marginal sequences of EVERY cell (what gen_golden.run stores for its sparse fixtures)"""
    out = gcg.run(dict(c, store='full'))
    post = out.pop('posteriorSequence', None)
    if post is not None:
        rows = cases.sparse_rows(post.shape[0])
        stride = cases.sparse_stride(post.shape[1:], limit=4000)
        out['posteriorRowsIndex'] = np.array(rows)
        out['posteriorRowsStride'] = np.array(stride)
        out['posteriorRows'] = post[rows][(slice(None),) + tuple(slice(None, None, s) for s in stride)]
        out['marginalSequence0'] = post.sum(axis=2)
        out['marginalSequence1'] = post.sum(axis=1)
    return out


def main():
    allc = dict(bc.BIGSHIFT, **bc.CONTROL)
    names = sys.argv[1:] or (list(allc) + list(bc.ONLINE) + ['bigshift_direct_call'])
    for name in names:
        if name == 'bigshift_direct_call':
            out = run_direct()
        elif name in bc.ONLINE:
            cases.ONLINE_CASES.setdefault(name, bc.ONLINE[name])      # (gen_golden.run_online looks the spec up there; this process only)
            out = gen_golden.run_online(name)
        else:
            out = run_fit(allc[name])
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print('%-28s logE=%r  %6.1f kB' % (name, float(out.get('logEvidence', np.nan)), os.path.getsize(path) / 1e3), flush=True)


if __name__ == '__main__':
    main()
