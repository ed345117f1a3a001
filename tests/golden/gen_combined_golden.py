#!/usr/bin/env python
"""
Generates the fixtures of tests/combined_cases.py (composed CombinedTransitionModel programs) under tests/golden/ by IMPORTING THE
REFERENCE, exactly as gen_golden.py does (same two shims: ``numpy.math``, a stub ``pathos``).  CPU only.
Run:  python tests/golden/gen_combined_golden.py [case ...]
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden   # noqa: E402  (installs the shims, imports the reference as gen_golden.bl)
import cases         # noqa: E402
import combined_cases as cc   # noqa: E402

bl = gen_golden.bl


def run(c):
    """gen_golden.run for a spec dict (the specs are not in cases.CASES)."""
    out = {}
    S0 = cases.build(bl, c)
    for k, m in enumerate(S0.marginalGrid):
        out['marginal%d' % k] = np.asarray(m)
    out['marginal_count'] = len(S0.marginalGrid)
    out['latticeConstant'] = np.asarray(S0.latticeConstant, dtype=float)
    S = cases.build(bl, c)
    kw = cases.fit_kwargs(c)
    with contextlib.redirect_stdout(io.StringIO()):
        with np.errstate(all='ignore'):
            S.fit(**kw)
    out['logEvidence'] = np.float64(S.logEvidence)
    out['localEvidence'] = np.asarray(S.localEvidence, dtype=float)
    if not kw.get('evidenceOnly', False) and np.isfinite(S.logEvidence):
        out['posteriorMeanValues'] = np.asarray(S.posteriorMeanValues, dtype=float)
        post = np.asarray(S.posteriorSequence, dtype=float)
        if post.size <= gen_golden.FULL_LIMIT and c.get('store') != 'sparse':
            out['posteriorSequence'] = post
        else:
            rows = cases.sparse_rows(post.shape[0])
            out['posteriorRowsIndex'] = np.array(rows)
            stride = cases.sparse_stride(post.shape[1:], limit=20_000)
            out['posteriorRowsStride'] = np.array(stride)
            out['posteriorRows'] = post[rows][(slice(None),) + tuple(slice(None, None, s) for s in stride)]
    if c['study'] in ('HyperStudy', 'ChangepointStudy') and len(S.hyperGridValues) > 1:
        out['logEvidenceList'] = np.asarray(S.logEvidenceList, dtype=float)
        out['hyperParameterDistribution'] = np.asarray(S.hyperParameterDistribution, dtype=float)
        out['hyperGridValues'] = np.asarray(S.hyperGridValues, dtype=float)
    if c['study'] == 'ChangepointStudy':
        out['mask'] = np.asarray(S.mask, dtype=bool)
    return out


def main():
    allc = dict(cc.COMBINED, **cc.SINGLE_STAGE)
    names = sys.argv[1:] or (list(allc) + list(cc.ONLINE))
    for name in names:
        if name in cc.ONLINE:
            cases.ONLINE_CASES.setdefault(name, cc.ONLINE[name])      # (gen_golden.run_online looks the spec up there; this process only)
            out = gen_golden.run_online(name)
        else:
            out = run(allc[name])
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **out)
        print('%-34s logE=%r  %6.1f kB' % (name, float(out['logEvidence']), os.path.getsize(path) / 1e3), flush=True)


if __name__ == '__main__':
    main()
