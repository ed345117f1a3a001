"""
The N-D host path after its split into a program builder (bayesloop_amd/csrc/blhip_nd_program.hpp) and path runners (blhip_fit_nd.hpp)
computes the bits and launches the kernels of the commit before the split.  tests/golden/nd_split_parent.npz holds the results of five
small cases from a library built from that commit, on the same hardware (tests/golden/gen_nd_split_parent.py wrote it); together they
cross every branch that moved: renormalising stages (NotEqual; a Deterministic shift), three batches and the fold, the chain-resident
kernel with 16 chains, and a streaming fit that resumes and carries point by point.  Every array must be np.array_equal; the launch
counts, the number of batches and the kernel variants must be the parent's too.
"""
import contextlib
import io
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import cases
import chain_nd_cases as cn
import nd_transition_cases as ndc

pytest.importorskip('scipy.stats')
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'nd_split_parent.npz')

ARRAYS = ('logEvidence', 'localEvidence', 'logEvidenceList', 'posteriorMeanValues', 'hyperParameterDistribution', 'posteriorSequence')
TIMING = ('forward_launches', 'backward_launches', 'batches', 'fwd_kernel_variant', 'bwd_kernel_variant')

# case -> (definition, engine options of the fit, streaming)
CASES = {
    'ndt_grw_notequal': (ndc.ND['ndt_grw_notequal'], {}, False),
    'ndt_shift_middle': (ndc.ND['ndt_shift_middle'], {}, False),
    'ndt_breakpoints': (ndc.ND['ndt_breakpoints'], dict(max_batch=3), False),
    'cnd_hyper_first_last': (cn.ND['cnd_hyper_first_last'], {}, False),
    'ndt_online': (ndc.ONLINE['ndt_online'], {}, True),
}
DEFAULTS = dict(max_batch=1024)


def _flat(value):
    """an attribute as float arrays: one, or -- a list of arrays of different lengths, as an online study keeps per transition model -- several"""
    try:
        return {'': np.asarray(value, dtype=float)}
    except (ValueError, TypeError):
        out = {}
        for i, v in enumerate(value):
            out.update({'/%d%s' % (i, k): a for k, a in _flat(v).items()})
        return out


def collect(case):
    """fits the case on the library the engine has loaded -> {'<case>/<array>': values, '<case>/timing': TIMING}"""
    c, opts, streaming = CASES[case]
    eng = bl.get_engine()
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'):
            if streaming:
                S = cases.build_online(bl, c)
                for d in cases.online_data(c):
                    S.step(d)
            else:
                S = cases.build(bl, c)
                S.fit(**cases.fit_kwargs(c))
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])
    out = {}
    for key in ARRAYS:
        value = getattr(S, key, None)
        if value is None:
            continue
        for suffix, a in _flat(value).items():
            if a.size:
                out['%s/%s%s' % (case, key, suffix)] = a
    timing = eng.last_timing() if streaming else S.lastTiming
    out['%s/timing' % case] = np.asarray([timing[k] for k in TIMING], dtype=np.int64)
    return out


@pytest.mark.parametrize('case', sorted(CASES))
def test_results_and_launches_are_the_parent_commits(case):
    parent = np.load(GOLDEN)
    got = collect(case)
    want = {k: parent[k] for k in parent.files if k.startswith(case + '/')}
    assert sorted(got) == sorted(want)
    assert any(k.endswith('/posteriorSequence') or '/posteriorSequence/' in k for k in want) and '%s/logEvidence' % case in want
    assert dict(zip(TIMING, got['%s/timing' % case])) == dict(zip(TIMING, want['%s/timing' % case]))
    for k in sorted(want):
        assert np.all(np.isfinite(want[k])), k                 # (no NaN among the recorded values: array_equal compares every one)
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
