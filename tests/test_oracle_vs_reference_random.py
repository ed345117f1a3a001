"""Pins the oracle on SEEDED RANDOM configurations against the real reference's results for them.

The reference's results are recorded under tests/golden/reference_random_*.npz by tests/golden/gen_reference_random.py, which
imports the reference (never copied); of a posterior sequence the record keeps its shape, a fixed sample of entries and, per
time step, block sums of the values and of their logarithms (tests/reference_fixtures.py).  The same generators drive the GPU parity tests (tests/test_gpu_parity.py: HIP
path vs oracle), so random configuration -> reference == oracle (here) and oracle == HIP path (there).
"""
import contextlib
import io
import warnings

import numpy as np
import pytest

import cases
import oracle_adapter as oa
import random_cases
import reference_fixtures as rf

_close = rf._close


def _check(family, seed, c, tol=None):
    data = np.asarray(cases.make_data(c['data']))
    if c['om'][0] == 'Poisson' and data.dtype.kind == 'f':
        pytest.skip('the reference needs integer counts (factorial)')
    S = rf.load(family, seed)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        w = oa.run(c)
    a, b = float(S['logEvidence']), float(w['logEvidence'])
    assert a == b or abs(a - b) <= 1e-9 * abs(a), 'logEvidence %r (reference) vs %r (oracle)' % (a, b)
    stopped = not np.isfinite(a) or ('logEvidenceList' in w and not np.all(np.isfinite(np.asarray(w['logEvidenceList'], dtype=float))))
    if 'logEvidenceList' in w and len(np.atleast_1d(S['logEvidenceList'])) > 1:
        _close(S['logEvidenceList'], w['logEvidenceList'], 1e-9, 0.0, 'logEvidenceList')
        _close(S['hyperParameterDistribution'], w['hyperParameterDistribution'], 1e-8, 1e-300, 'hyperParameterDistribution')
    if stopped:
        return                           # the reference leaves np.empty() garbage behind a zero-normaliser stop (core.py:360, :399)
    _close(S['localEvidence'], w['localEvidence'], 1e-7, 0.0, 'localEvidence')
    if not cases.fit_kwargs(c).get('evidenceOnly') and w.get('posteriorSequence') is not None:
        atol = (tol or {}).get('post_atol', 0.0)
        rf.check_posterior(_part(S, 'posteriorSequence'), w['posteriorSequence'], 1e-9, max(1e-300, atol), 'posteriorSequence')
        _close(S['posteriorMeanValues'], w['posteriorMeanValues'], 1e-9, 1e-12, 'posteriorMeanValues')


def _part(rec, name):
    return {k[len(name) + 1:]: v for k, v in rec.items() if k.startswith(name + '/')}


@pytest.mark.parametrize('seed', range(40))
def test_oracle_equals_reference_on_random_grw_studies(seed):
    _check('grw', seed, random_cases.random_case(seed))


@pytest.mark.parametrize('seed', range(52))
def test_oracle_equals_reference_on_random_model_zoo(seed):
    c, tol = random_cases.random_model_case(seed)
    _check('zoo', seed, c, tol)


@pytest.mark.parametrize('seed', range(24))
def test_oracle_equals_reference_on_random_wide_walks(seed):
    """Walks on the second parameter with radii 9 .. 64 and on the first one with radii 41 .. 128 (the pre-pass kernels on the GPU side)."""
    _check('wide', seed, random_cases.random_wide_axis1_case(seed))


@pytest.mark.parametrize('seed', range(40))
def test_oracle_equals_reference_on_random_hyper_studies(seed):
    _check('hyper', seed, random_cases.random_hyper_case(seed))


@pytest.mark.parametrize('seed', range(40))
def test_oracle_equals_reference_on_random_online_studies(seed):
    c = random_cases.random_online_case(seed)
    S = rf.load('online', seed)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        w = oa.run_online(c)
    a, b = float(S['logEvidence']), float(w['logEvidence'])
    assert a == b or abs(a - b) <= 1e-9 * abs(a), 'logEvidence %r (reference) vs %r (oracle)' % (a, b)
    rf.check_posterior(_part(S, 'posteriorSequence'), np.asarray(w['posteriorSequence'], dtype=float), 1e-9, 1e-13, 'posteriorSequence')
    for key in ('posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence'):
        _close(S[key], np.asarray(w[key], dtype=float), 1e-9, 1e-13, key)
    n_models = sum(1 for k in S if k.startswith('hyperParameterSequence_'))
    assert n_models == len(w['hyperParameterSequence'][0]), 'number of transition models'
    for i in range(n_models):
        _close(S['hyperParameterSequence_%d' % i],
               np.asarray([h[i] for h in w['hyperParameterSequence']], dtype=float), 1e-9, 1e-13, 'hyperParameterSequence')
