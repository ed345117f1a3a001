"""Shapes, observation values and studies shared by tests/test_predictive_host.py (CPU) and tests/test_predictive.py (-m gpu), and by
tests/golden/gen_predictive_golden.py, which builds the same golden cases from the reference package."""
import numpy as np

# ---- the fixture tests/golden/predictive.npz: case of tests/cases.py -> observation values (the three of simulate.npz, plus a HyperStudy on a
# one-parameter grid)
GOLDEN_X = {'c1_coal': np.arange(0, 9), 'kat_gaussian': np.linspace(-2, 8, 11), 'c4_small': np.linspace(-3, 3, 7), 'c1_coal_hyper': np.arange(0, 9)}

# ---- the plan helper's sweep
PRIMES = (2, 3, 257, 521, 65537, 1048573)
PLAN_G = (2, 5, 31, 32, 33, 255, 256, 517, 1260, 4096, 100003, 262144, 1 << 20) + PRIMES
PLAN_T = (1, 15, 16, 17, 256, 1000)
PLAN_X = (1, 16, 17, 1000)

# the kernel's tiles (bayesloop_amd/csrc/blhip_predictive.hpp): what the shapes below are odd against
TM, XT, KSTEP, SLAB_MIN, ROWS_MAX = 16, 16, 32, 256, 128

# ---- the contraction alone
CONTRACT_T = (1, 15, 16, 17, 33)
CONTRACT_X = (1, 16, 17, 40)


def contract_grids(plan):
    """name -> the grid as the model of the call describes it.  plan(G, T, X) -> the helper's plan: the last grid is two of ITS slabs and
    5 cells (a 1-D grid; the slab of so small a grid is the shortest one the plan makes)."""
    slab = plan(2 * SLAB_MIN + 5, 1, 1)['slab']
    grids = {'2': (2,), '3x7x5': (3, 7, 5), '5x18x14': (5, 18, 14), 'two-slabs+5': (2 * slab + 5,)}
    assert plan(2 * slab + 5, 33, 40)['slab'] == slab and plan(2 * slab + 5, 33, 40)['n_slabs'] == 3
    return grids


def likelihood_rows(X, G, seed):
    """Caller-made likelihood rows: non-negative, spanning 300 decades, one value in eight exactly zero."""
    rng = np.random.default_rng(seed)
    rows = 10.0 ** rng.uniform(-150.0, 150.0, (X, G))
    rows[rng.random((X, G)) < 0.125] = 0.0
    rows.flat[0], rows.flat[-1] = 1e150, 1e-150             # (the span, however few values there are)
    return rows


def balanced_rows(seq, X, seed):
    """Rows that weigh every cell by the inverse of its mean posterior (1e300 where that is at or below the fold's floor): every cell
    that carries any mass contributes a term of order one, so no slab, tile or cell of the grid can go missing unnoticed -- the spread
    rows above let a handful of cells decide the sum."""
    rng = np.random.default_rng(seed)
    mean = np.maximum(np.asarray(seq).mean(axis=0), 1e-300)
    return rng.uniform(0.5, 1.5, (X, seq.shape[1])) / mean


# ---- rows built on the device: name -> (study, x).  A study is a case description of tests/cases.py or a builder of
# tests/likprogram_studies.py; where: 'formula' (blpp::tabulate_rows_kernel), 'table' (blk::lik_table_kernel), 'program'
# (bllp::lik_program_kernel), 'host' (om.pdf, uploaded)
def _case(om, tm, data, study='Study'):
    return dict(study=study, data=data, om=om, tm=tm)


MODELS = {
    'gaussian2d': (_case(('Gaussian', [('mean', ('cint', -4, 4, 37)), ('std', ('oint', 0, 3, 11))], 'default'), ('GRW', 's', 0.3, 'mean', None), ('series', 21, 19)),
                   np.linspace(-5.0, 5.5, 18), 'formula'),
    'poisson1d': (_case(('Poisson', [('rate', ('oint', 0, 6, 100))], 'default'), ('GRW', 's', 0.2, 'rate', None), ('coal', 17)),
                  np.arange(0.0, 17.0), 'formula'),
    'bernoulli': (_case(('Bernoulli', [('p', ('oint', 0, 1, 200))], 'default'), ('ChangePoint', 'tc', 5, None), np.array([1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0])),
                  np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0]), 'table'),
    'laplace': (_case(('Laplace', [('mu', ('cint', -4, 4, 60)), ('b', ('oint', 0, 3, 44))], 'default'), ('GRW', 's1', 0.3, 'mu', None), ('series', 71, 12)),
                np.linspace(-4.5, 4.5, 21), 'table'),
    'whitenoise': (_case(('WhiteNoise', [('std', ('oint', 0, 3, 300))], 'default'), ('GRW', 's', 0.05, 'std', None), ('series', 72, 10)),
                   np.linspace(-3.0, 3.0, 17), 'table'),
    'sympy_normal': ('normal_study', np.linspace(-2.5, 3.5, 19), 'program'),
    'sympy_poisson': ('poisson_study', np.arange(0.0, 12.0), 'program'),
    'scipy_t_5x18x14': ('scipy_t_study', np.linspace(-3.0, 4.0, 17), 'program'),
    'johnsonsu_3x3x7x6': (_case(('SciPy:johnsonsu', [('a', ('cint', -1.0, 1.0, 3)), ('b', ('cint', 0.8, 2.5, 3)), ('loc', ('cint', -2.0, 2.0, 7)),
                                                     ('scale', ('oint', 0.3, 2.0, 6))], 'default'),
                                ('Combined', [('GRW', 's_loc', 0.5, 'loc', None), ('GRW', 's_b', 0.4, 'b', None)]), ('series', 96, 6)),
                          np.linspace(-3.0, 3.0, 9), 'host'),
}


def build_model(bl, name):
    import cases
    import likprogram_studies as ls
    spec = MODELS[name][0]
    if spec == 'normal_study':
        return ls.normal_study(bl, sizes=(40, 12), T=12)
    if spec == 'poisson_study':
        return ls.poisson_study(bl)
    if spec == 'scipy_t_study':
        return ls.scipy_t_study(bl, sizes=(5, 18, 14), T=10)
    return cases.build(bl, spec)


def host_simulate(S, x, index, density):
    """Study.simulate as the parent computes it, on the posterior sequence on the host: index None (time average), a row, or 'all'."""
    seq = np.asarray(S.posteriorSequence)
    om = S.observationModel
    if isinstance(index, str):
        return np.array([host_simulate(S, x, i, density) for i in range(len(seq))])
    post = np.sum(seq, axis=0) / len(seq) if index is None else seq[index]
    prob = np.array([np.sum(om.pdf(S.grid, [xi]) * post) for xi in x])
    if not density:
        with np.errstate(all='ignore'):
            prob = prob / np.sum(prob)
    return prob
