"""OnlineStudy.stepMany on the device (-m gpu): the goldens of the reference and seeded random studies through blocks, the time-varying
mixture kernel (blo::mix_sequence_kernel) alone against a longdouble sum, a chunk seam forced by the memory budget, a chunk with a dead
chain, and the large-grid shape of test_online.py through a block."""
import contextlib
import io

import numpy as np
import pytest

import cases
import nd_transition_cases as ndc
import oracle_adapter as oa
import random_cases
import bayesloop_amd as bl
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem
from test_online import ATOL, RTOL, check_online, reference_accessor_checks

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def results(S):
    return dict(logEvidence=S.logEvidence, posteriorSequence=S.posteriorSequence, posteriorMeanValues=S.posteriorMeanValues,
                transitionModelSequence=S.transitionModelSequence, localTransitionModelSequence=S.localTransitionModelSequence,
                hyperParameterSequence=S.hyperParameterSequence, parameterPosterior=S.parameterPosterior, logEvidenceList=S.logEvidenceList)


def block_study(c, data=None, history=True):
    S = cases.build_online(bl, c, storeHistory=history)
    S.BLOCK_MIN_POINTS = 1                      # (a block whatever its length)
    quiet(S.stepMany, np.array(cases.online_data(c) if data is None else data))
    return S


def loop_study(c, data=None, history=True):
    S = cases.build_online(bl, c, storeHistory=history)
    for d in (cases.online_data(c) if data is None else data):
        quiet(S.step, d)
    return S


def assert_meets(S, W):
    """every public result of S against W at test_online.py's bar; the same NaN / inf pattern"""
    def close(a, b, what, rtol=RTOL, atol=ATOL):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        assert a.shape == b.shape, what
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), what
        ok = np.isfinite(a)
        np.testing.assert_allclose(a[ok], b[ok], rtol=rtol, atol=atol, err_msg=what)
    close(S.logEvidence, W.logEvidence, 'logEvidence', atol=0)
    for key in ('posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence', 'marginalizedPosterior',
                'hyperLogEvidenceList', 'transitionModelDistribution', 'localTransitionModelDistribution', 'transitionModelPosterior'):
        close(getattr(S, key), getattr(W, key), key)
    for i in range(len(S.transitionModels)):
        close([h[i] for h in S.hyperParameterSequence], [h[i] for h in W.hyperParameterSequence], 'hyperParameterSequence')
        close(S.hyperParameterDistribution[i], W.hyperParameterDistribution[i], 'hyperParameterDistribution')
        close(S.parameterPosterior[i], W.parameterPosterior[i], 'parameterPosterior')
        close(S.logEvidenceList[i], W.logEvidenceList[i], 'logEvidenceList', atol=0)
    assert np.array_equal(S.rawData, W.rawData, equal_nan=True) and np.array_equal(S.rawTimestamps, W.rawTimestamps)
    assert list(S.formattedTimestamps) == list(W.formattedTimestamps) and S.firstStep == W.firstStep


@pytest.mark.parametrize('case', list(cases.ONLINE_CASES) + list(ndc.GOLDEN_ONLINE))
def test_step_many_matches_reference_golden(case):
    c = cases.ONLINE_CASES[case] if case in cases.ONLINE_CASES else ndc.ONLINE[case]
    S = block_study(c)
    gold = oa.load_golden(case)
    check_online(results(S), gold, len(S.transitionModels))
    reference_accessor_checks(S, case)


@pytest.mark.parametrize('seed', range(10))
def test_step_many_seeded_random_models_match_oracle(seed):
    c = random_cases.random_online_case(seed)
    data = cases.online_data(c)
    S = cases.build_online(bl, c)
    S.BLOCK_MIN_POINTS = 1
    k = seed % len(data)                        # (a block, one step, a block: the block resumes from and carries into step's states)
    quiet(S.stepMany, np.array(data[:k]))
    quiet(S.step, data[k])
    quiet(S.stepMany, np.array(data[k + 1:]))
    with np.errstate(all='ignore'):
        w = oa.run_online(c)
    assert abs(S.logEvidence - w['logEvidence']) <= RTOL * abs(w['logEvidence'])
    for key in ('posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence'):
        np.testing.assert_allclose(np.asarray(getattr(S, key), dtype=float), np.asarray(w[key], dtype=float), rtol=RTOL, atol=ATOL, err_msg=key)
    for i in range(len(S.transitionModels)):
        np.testing.assert_allclose(np.asarray([h[i] for h in S.hyperParameterSequence], dtype=float),
                                   np.asarray([h[i] for h in w['hyperParameterSequence']], dtype=float), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('history', [True, False])
def test_step_many_without_and_with_history_meets_the_loop(history):
    c = cases.ONLINE_CASES['online_gauss2d']
    S, W = block_study(c, history=history), loop_study(c, history=history)
    assert_meets(S, W)


# ---- the mixture kernel alone ---------------------------------------------------------------------------------------------------------
GRIDS = {'3x7x5': [3, 7, 5], '1001': [1001], '64x48': [64, 48]}


def kept_sequence(eng, shape, B, T, seed):
    """A forward-only fit of B walks that keeps its sequence on the device -> the normalised sequence (B, T, G) as the host reads it."""
    rng = np.random.default_rng(seed)
    G = int(np.prod(shape))
    marginal = [np.linspace(0.5, 2.5, n) + 0.01 * k for k, n in enumerate(shape)]
    lattice = [m[1] - m[0] for m in marginal]
    problem = FitProblem(obs_model=_abi.OM_TABLE, marginal=marginal, lattice=lattice, data=np.zeros((T, 1)), timestamps=np.arange(T, dtype=float),
                         prior=np.full(G, 1.0 / G), ops=[(_abi.OP_GRW, len(shape) - 1, -1, 0)], lik=rng.uniform(0.05, 1.0, (T, G)))
    sig = (0.3 + 0.9 * rng.uniform(size=(B, 1))) * lattice[-1]
    eng.fit(problem, sig, forward_only=True, keep_posterior=True)
    return np.array([eng.posterior(b, T, shape) for b in range(B)]).reshape(B, T, G), marginal


@pytest.mark.parametrize('T', [1, 7])
@pytest.mark.parametrize('B', [1, 5, 16])
@pytest.mark.parametrize('grid', list(GRIDS))
def test_mix_sequence_kernel_against_longdouble_sum(grid, B, T):
    """Two models of B chains accumulated into one plane.  Every term is non-negative, so the bound is relative: (C + M + 2) u for C = 2 B
    chains in M = 2 models -- one rounding for the weight as the host forms it, one per product, C - 1 + M - 1 additions (the kernel's fma
    rounds product and addition once: it stays below the count) -- and (G + 2) u on top for the means."""
    from conftest import kernel_census
    eng = bl.engine.get_engine()
    shape = GRIDS[grid]
    G = int(np.prod(shape))
    rng = np.random.default_rng(100 * B + T)
    before = dict((n, c) for c, n in kernel_census())
    ref = np.zeros((T, G), dtype=np.longdouble)
    got = []
    for rep in range(2):                          # the whole thing twice: equal bits
        ref[:] = 0
        rng = np.random.default_rng(100 * B + T)
        for model in range(2):
            seq, marginal = kept_sequence(eng, shape, B, T, seed=7 * model + B + T)
            w = rng.uniform(0.0, 1.0, (T, B)) * 10.0 ** rng.integers(-6, 1, (T, B))
            eng.mix_sequence(w, accumulate=model > 0)
            ref += np.einsum('tb,btg->tg', w.astype(np.longdouble), seq.astype(np.longdouble))
        got.append((eng.mix_read(T, shape).reshape(T, G), eng.mix_means(marginal, T)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    H, means = got[0]
    C, M = 2 * B, 2
    err = np.abs(H.astype(np.longdouble) - ref)
    print('mix %s B %d T %d: max relative error %.3g u (bound %d u)' % (grid, B, T, float(np.max(err / ref)) / U, C + M + 2))
    assert np.all(err <= (C + M + 2) * U * ref)
    mesh = np.meshgrid(*marginal, indexing='ij')
    for k in range(len(shape)):
        gk = mesh[k].ravel().astype(np.longdouble)
        want = ref @ gk                            # (the grids are positive: the terms of the means are non-negative too)
        assert np.all(np.abs(means[:, k].astype(np.longdouble) - want) <= (C + M + 2 + G + 2) * U * want)
    # which flavour ran: 16-byte loads on the even grid, 8-byte ones on the odd grids (their row bases are not 16-byte aligned)
    after = dict((n, c) for c, n in kernel_census())
    ran = {n for n in after if 'mix_sequence_kernel' in n and after[n] > before.get(n, 0)}
    assert ran == {'blo::mix_sequence_kernel<%s>' % ('true' if G % 2 == 0 else 'false')}


def test_mix_sequence_planes_and_errors():
    """source 1: the per-model planes mixed into plane 0 equal the longdouble sum; a shape that does not match is refused."""
    eng = bl.engine.get_engine()
    shape, B, T = [64, 48], 5, 3
    G = int(np.prod(shape))
    rng = np.random.default_rng(5)
    ref = np.zeros((T, G), dtype=np.longdouble)
    tmd = rng.uniform(0.1, 1.0, (T, 2))
    for model in range(2):
        seq, _ = kept_sequence(eng, shape, B, T, seed=model)
        w = rng.uniform(0.0, 1.0, (T, B))
        eng.mix_sequence(w, plane=1 + model, n_planes=3)
        ref += tmd[:, [model]].astype(np.longdouble) * np.einsum('tb,btg->tg', w.astype(np.longdouble), seq.astype(np.longdouble))
    eng.mix_sequence(tmd, plane=0, n_planes=3, source=1)
    H = eng.mix_read(T, shape).reshape(T, G).astype(np.longdouble)
    assert np.all(np.abs(H - ref) <= (B + 2 + 2 + 2) * U * ref)          # (one more product per term than the single-plane form)
    with pytest.raises(bl.exceptions.BackendError):
        eng.mix_sequence(np.ones((T, B + 1)))
    with pytest.raises(bl.exceptions.BackendError):
        eng.mix_sequence(np.ones((T + 1, B)))
    with pytest.raises(bl.exceptions.BackendError):
        eng.mix_sequence(np.ones((T, B)), plane=0, n_planes=2, accumulate=True)      # no history of that shape to accumulate onto
    with pytest.raises(bl.exceptions.BackendError):
        eng.mix_read(T, shape, plane=3)


# ---- time chunks, a dead chain, a large grid -----------------------------------------------------------------------------------------
SNAP = ('logEvidence', 'posteriorSequence', 'posteriorMeanValues', 'transitionModelSequence', 'localTransitionModelSequence', 'marginalizedPosterior',
        'hyperLogEvidenceList', 'transitionModelDistribution', 'localTransitionModelDistribution', 'transitionModelPosterior', 'hyperParameterSequence',
        'hyperParameterDistribution', 'parameterPosterior', 'logEvidenceList', 'rawData', 'rawTimestamps', 'formattedTimestamps', 'firstStep',
        'transitionModels')


def snapshot(S):
    """the public results of a study as plain values (the device-resident ones are fetched from the engine installed NOW)"""
    import types
    return types.SimpleNamespace(**{k: getattr(S, k) for k in SNAP})


def test_chunk_seam_forced_by_the_memory_budget():
    """mem_budget_bytes such that N = 7 splits 3 + 3 + 1: the carried states make the seam exact, the study meets the unsplit run.  (On a
    context of its own: an option cannot be unset, and the budget is part of every later fit's memory plan.)"""
    c = cases.ONLINE_CASES['online_poisson_3tm']
    data = cases.online_data(c)[:7]
    whole = snapshot(block_study(c, data))
    eng = bl.engine.extra_engine(bl.engine.get_engine().device)
    shape, chains, planes = [150], 6, 4
    three = eng.online_block_plan(shape, chains, planes, 3, 1e30)['chunk_bytes']
    assert eng.online_block_plan(shape, chains, planes, 7, three)['steps'] == 3
    eng.set_option('mem_budget_bytes', three / 0.9 + 1.0)                  # (a fit plans with 0.9 of the option)
    prev = bl.set_engine(eng)
    try:
        launches = []
        S = cases.build_online(bl, c)
        orig = eng.fit

        def spy(problem, *a, **kw):
            launches.append(problem.T)
            return orig(problem, *a, **kw)
        eng.fit = spy
        quiet(S.stepMany, np.array(data))
        del eng.fit
        assert launches == [3, 3, 3, 3, 3, 3, 1, 1, 1]                       # three models, chunks of 3 + 3 + 1
        split = snapshot(S)
        del S
    finally:
        bl.set_engine(prev)
    assert_meets(split, whole)


DEAD = dict(om=('Bernoulli', [('p', ('cint', 0.0, 1.0, 11))], ('array', [0.5] + [0.0] * 9 + [0.5])),
            models=[('walks', ('GRW', 's', [0.0, 0.05, 0.2], 'p', None)), ('static', ('Static',))], data=[1, 1, 0, 1, 1, 0])


def test_chunk_with_a_dead_chain_ends_where_the_loop_ends():
    """A prior with mass on p = 0 and p = 1 only: the first 1 leaves p = 1, the first 0 after it nothing -- for the chains that never
    leave their cells (sigma = 0, Static).  The walking chains stay healthy."""
    with np.errstate(all='ignore'):
        w = oa.run_online(DEAD)
    dead = [~np.isfinite(np.asarray(le, dtype=float)) for le in w['logEvidenceList']]
    assert [d.tolist() for d in dead] == [[True, False, False], [True]]          # (on the CPU oracle: exactly the chains without a walk die)
    with np.errstate(all='ignore'):
        S, W = block_study(DEAD), loop_study(DEAD)
    assert not np.isfinite(S.logEvidenceList[0][0]) and np.isfinite(S.logEvidenceList[0][1])
    assert_meets(S, W)


def test_large_grid_block_matches_offline_fit():
    """512 x 512 Gaussian, two hyper-values, N = 10 (test_online.py's large-grid shape) through one block."""
    x = cases.series(51, 10)
    om = lambda: bl.om.Gaussian('mean', bl.cint(-8, 8, 512), 'std', bl.oint(0, 4, 512))
    S = bl.OnlineStudy(storeHistory=True, silent=True)
    S.setOM(om(), silent=True)
    with contextlib.redirect_stdout(io.StringIO()):
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', [0.1, 0.6], target='mean'))
        S.stepMany(x)
    assert len(S.posteriorSequence) == 10
    for j, s in enumerate([0.1, 0.6]):
        F = bl.Study(silent=True)
        F.loadData(x, silent=True)
        F.set(om(), bl.tm.GaussianRandomWalk('s', s, target='mean'), silent=True)
        F.fit(forwardOnly=True, silent=True)
        assert abs(S.logEvidenceList[0][j] - F.logEvidence) <= 1e-10 * abs(F.logEvidence)
        np.testing.assert_allclose(S.parameterPosterior[0][j], F.posteriorSequence[-1], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(np.sum(S.posteriorSequence[-1]), 1.0, rtol=1e-12)


# ---- resumed, carried fits on the chain-resident 1-D kernel ------------------------------------------------------------------------------
def poisson_walk_study(n, chains, history):
    """A Poisson rate grid of n cells; `chains` random walks whose stencil radii run from 0 (sigma = 0) to 9 cells, beside a Static model."""
    S = bl.OnlineStudy(storeHistory=history, silent=True)
    S.setOM(bl.om.Poisson('rate', bl.oint(0, 8, n)), silent=True)
    cell = 8.0 / (n + 1)
    with contextlib.redirect_stdout(io.StringIO()):
        S.addTransitionModel('walk', bl.tm.GaussianRandomWalk('s', (np.linspace(0.0, 2.2, chains) * cell).tolist(), target='rate'))
        S.addTransitionModel('static', bl.tm.Static())
    return S


def chain1d_launches():
    from conftest import kernel_census
    return sum(c for c, name in kernel_census() if 'bl1c::chain1d_kernel<' in name or 'bl1c::chain1d_long_kernel<' in name)


COUNTS = np.array([3, 1, 4, 2, 5, 0, 6, 2])


@pytest.mark.parametrize('history', [False, True])
@pytest.mark.parametrize('chains', [4, 33])
@pytest.mark.parametrize('n', [200, 4608])
def test_resumed_block_on_the_chain_resident_1d_kernel(n, chains, history):
    """N = 5 after three single steps: with option chain1d = 2 (the kernel wherever it is admitted; at 1 the cost model decides) each model's
    block is ONE launch of bl1c::chain1d_kernel / chain1d_long_kernel (variant 9) that starts from the carried states and leaves them; under
    chain1d = 0 the same block takes the K-steps-per-launch path.  Both meet the loop.  A one-step call keeps the route it had."""
    eng = bl.engine.get_engine()
    W = poisson_walk_study(n, chains, history)
    for d in COUNTS:
        quiet(W.step, d)
    assert eng.last_timing()['fwd_kernel_variant'] == 4            # (a resumed one-step fit: the K-steps-per-launch kernel, as ever)
    want = snapshot(W)
    for mode, variant in ((2, 9), (0, 4), (1, None)):
        eng.set_option('chain1d', mode)
        try:
            S = poisson_walk_study(n, chains, history)
            for d in COUNTS[:3]:
                quiet(S.step, d)
            seen, launched = [], []
            orig = eng.fit

            def spy(problem, *a, **kw):
                before = chain1d_launches()
                res = orig(problem, *a, **kw)
                seen.append((problem.T, eng.last_timing()['fwd_kernel_variant']))
                launched.append(chain1d_launches() - before)
                return res
            eng.fit = spy
            try:
                quiet(S.stepMany, COUNTS[3:])
            finally:
                del eng.fit
        finally:
            eng.set_option('chain1d', 1)
        assert [s[0] for s in seen] == [5, 5]
        if variant is not None:
            assert [s[1] for s in seen] == [variant, variant], (mode, seen)
            assert launched == ([1, 1] if variant == 9 else [0, 0])
        assert_meets(snapshot(S), want)
