#!/usr/bin/env python
"""
Records what the REFERENCE (the upstream ``bayesloop`` package, imported from source) computes for the seeded random
configurations of tests/random_cases.py and for the parser queries of tests/test_parser.py, so that the tests which pin the
oracle and this package's parser against it run without the reference:

    python tests/golden/gen_reference_random.py --reference <directory holding the bayesloop package> [family ...]

    families: grw zoo wide hyper online parser   (default: all of them)
    -> tests/golden/reference_random_<family>_<k>.npz (seeds 20 k .. 20 k + 19), tests/golden/reference_parser.npz

The reference is imported, never copied; the shim of gen_golden.py applies (``numpy.math = math``: Poisson.pdf calls
``np.math.factorial``).  A fixture is data only: the reference's outputs, keyed '<seed>/<attribute>'; of a posterior sequence
what tests/reference_fixtures.py keeps (shape, a fixed sample of entries, block sums), keyed '<seed>/<attribute>/<part>'.
"""
import argparse
import contextlib
import io
import math
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import cases                           # noqa: E402
import random_cases                    # noqa: E402
from reference_fixtures import SEEDS_PER_FILE, fixture_path, reduce_posterior     # noqa: E402

# family -> (number of seeds, seed -> (case, absolute tolerance of its posterior comparison)); the seed ranges and tolerances of
# tests/test_oracle_vs_reference_random.py
FAMILIES = dict(grw=(40, lambda s: (random_cases.random_case(s), 1e-300)),
                zoo=(52, lambda s: (lambda c, tol: (c, max(1e-300, (tol or {}).get('post_atol', 0.0))))(*random_cases.random_model_case(s))),
                wide=(24, lambda s: (random_cases.random_wide_axis1_case(s), 1e-300)),
                hyper=(40, lambda s: (random_cases.random_hyper_case(s), 1e-300)),
                online=(40, lambda s: (random_cases.random_online_case(s), 1e-13)))
STUDY_KEYS = ('logEvidence', 'logEvidenceList', 'hyperParameterDistribution', 'localEvidence', 'posteriorSequence', 'posteriorMeanValues')
ONLINE_KEYS = ('logEvidence', 'posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence')


def _quiet():
    stack = contextlib.ExitStack()
    stack.enter_context(contextlib.redirect_stdout(io.StringIO()))
    stack.enter_context(np.errstate(all='ignore'))
    stack.enter_context(warnings.catch_warnings())
    warnings.simplefilter('ignore')
    return stack


def record_study(ref, c, atol):
    data = np.asarray(cases.make_data(c['data']))
    if c['om'][0] == 'Poisson' and data.dtype.kind == 'f':
        return {}                        # the reference needs integer counts (factorial); the test skips such a case
    S = cases.build(ref, c)
    with _quiet():
        S.fit(**cases.fit_kwargs(c))
    out = {}
    for k in STUDY_KEYS:
        if hasattr(S, k) and getattr(S, k) is not None:
            out[k] = np.asarray(getattr(S, k), dtype=float)
    return _reduced(out, atol)


def _reduced(out, atol):
    if 'posteriorSequence' in out:
        out.update({'posteriorSequence/' + k: v for k, v in reduce_posterior(out.pop('posteriorSequence'), atol).items()})
    return out


def record_online(ref, c, atol):
    S = cases.build_online(ref, c)
    with _quiet():
        for d in cases.online_data(c):
            S.step(d)
    out = {k: np.asarray(getattr(S, k), dtype=float) for k in ONLINE_KEYS}
    for i in range(len(S.transitionModels)):
        out['hyperParameterSequence_%d' % i] = np.asarray([h[i] for h in S.hyperParameterSequence], dtype=float)
    return _reduced(out, atol)


def record_parser(ref):
    import test_parser as tp
    rec = {}
    with _quiet():
        Pr = ref.Parser(*tp.two_studies(ref))
        for j, (q, t) in enumerate(tp.QUERIES):
            try:
                rec['query%d' % j] = np.float64(Pr(q, t=t, silent=True))
            except (ValueError, TypeError, IndexError):
                rec['query%d_raises' % j] = np.bool_(True)
        for j, q in enumerate(tp.DISTRIBUTIONS):
            x, p = Pr(q, silent=True)
            rec['distribution%d/x' % j], rec['distribution%d/p' % j] = np.asarray(x, dtype=float), np.asarray(p, dtype=float)
        Ph = ref.Parser(*tp.hyper_studies(ref))
        for j, (q, t) in enumerate(tp.HYPER_QUERIES):
            try:
                rec['hyper_query%d' % j] = np.float64(Ph(q, t=t, silent=True))
            except (ValueError, TypeError, IndexError):
                rec['hyper_query%d_raises' % j] = np.bool_(True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='directory that holds the reference package (bayesloop/)')
    ap.add_argument('families', nargs='*', default=list(FAMILIES) + ['parser'])
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    np.math = math
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import bayesloop as ref
    for fam in args.families:
        if fam == 'parser':
            files = {fixture_path(fam): record_parser(ref)}
        else:
            n, gen = FAMILIES[fam]
            files = {}
            for seed in range(n):
                c, atol = gen(seed)
                got = (record_online if fam == 'online' else record_study)(ref, c, atol)
                files.setdefault(fixture_path(fam, seed), {}).update({'%d/%s' % (seed, k): v for k, v in got.items()})
        for path, rec in files.items():
            np.savez_compressed(path, **rec)
            print('%-28s %3d arrays, %7.1f KB' % (os.path.basename(path), len(rec), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
