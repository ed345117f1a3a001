"""Inputs of tests/test_declined_batches.py and of the planner-agreement tests in tests/test_chain_plan_host.py: batches the chain-resident
route of two-parameter grids (ChainRun::setup, bayesloop_amd/csrc/blhip_fit_paths.hpp) plans and then DECLINES, so that the launch-per-step
kernels run them, and batches whose separate fold reads the chain kernels' strip-major layout.  See tests/DECLINED_BATCHES.md."""
import numpy as np

import cases

T = 10
LO, HI = -8.0, 8.0
ROW_MAJOR, STRIP_MAJOR, PADDED = 0, 1, 2          # ChainFoldLayout (blhip_chain_plan.hpp)


def g2(n0, n1):
    # (std >= 0.5: the largest exponent is 13^2 / (2 x 0.25) = 338 < 708 -- no likelihood value is 0 or subnormal, so every localEvidence
    #  entry is compared at the bar; the choice of tests/chain_clamp_cases.py)
    return ('Gaussian', [('mean', cases._g('cint', LO, HI, n0)), ('std', cases._g('cint', 0.5, 4, n1))], 'default')


def radius(sigma, n0):
    """SciPy's radius of a Gaussian filter of width sigma on the first parameter: int(4 sigma / lattice + 0.5) (transitionModels.py:108-111)"""
    return int(4.0 * sigma / ((HI - LO) / (n0 - 1.0)) + 0.5)


DATA = ('series_jump', 311, T, 5, 2.0)
WALKS3 = [0.1, 0.2, 0.3]
POINTS3 = [2, 4, 6]
WALKS5 = [float(x) for x in np.linspace(0.05, 0.45, 5)]
WALKS5_TALL = [float(x) for x in np.linspace(0.02, 0.3, 5)]      # 1024 rows: radii 5 .. 77 of at most 80


def changepoints(n0, n1):
    """every position: T - 1 chains; the chain of tc restarts at forward step tc + 1 (transitionModels.py:300-312)"""
    c = dict(study='ChangepointStudy', data=DATA, om=g2(n0, n1), tm=('ChangePoint', 'tc', 'all', None))
    return c, ['0:0:%d' % (tc + 1) for tc in range(T - 1)]


def mixed(n0, n1):
    """a restart inside a filtering chain: the hyper-grid is walks x points, the walk's width the slower index"""
    c = dict(study='HyperStudy', data=DATA, om=g2(n0, n1),
             tm=('Combined', [('GRW', 'sigma', WALKS3, 'mean', None), ('ChangePoint', 'tc', POINTS3, None)]))
    return c, ['%d:0:%d' % (radius(s, n0), tc + 1) for s in WALKS3 for tc in POINTS3]


def walks(n0, n1, sigmas):
    c = dict(study='HyperStudy', data=DATA, om=g2(n0, n1), tm=('GRW', 'sigma', sigmas, 'mean', None))
    return c, ['%d' % radius(s, n0) for s in sigmas]


def study(n0, n1, sigma):
    """an ordinary fit that keeps its posteriors; the walk is wider than the single-chain resident kernel's radius of 8, which would take it first"""
    assert radius(sigma, n0) > 8
    c = dict(study='Study', data=DATA, om=g2(n0, n1), tm=('GRW', 'sigma', sigma, 'mean', None))
    return c, ['%d' % radius(sigma, n0)]


def _case(built, grid, opts=None, hyper=True, **expect):
    c, chains = built
    facts = dict(n0=grid[0], n1=grid[1], T=T, full=1, accumulate=1 if hyper else 0, **(opts or {}))
    return dict(case=c, grid=grid, opts=opts or {}, chains=chains, facts=facts, hyper=hyper, **expect)


# A: declined by chain_fold_settle with post_private = 1 (a padded 1024-row geometry has no storing backward kernel).  A4: an odd number of
# cells; A5: ragged columns (the strip-major index of such a grid runs past the step, for the last chain's last step past the buffer)
A_CASES = {
    'A1_changepoints_520x32': _case(changepoints(520, 32), (520, 32), post_private=1),
    'A2_mixed_520x32': _case(mixed(520, 32), (520, 32), post_private=1),
    'A3_walks_unfused_520x32': _case(walks(520, 32, WALKS5), (520, 32), dict(fuse_accumulate=0), post_private=1),
    'A4_changepoints_601x33_odd': _case(changepoints(601, 33), (601, 33), post_private=1),
    'A5_changepoints_600x20': _case(changepoints(600, 20), (600, 20), post_private=1),
    'A5_changepoints_1024x20': _case(changepoints(1024, 20), (1024, 20), post_private=1),
    'A5_changepoints_513x40': _case(changepoints(513, 40), (513, 40), post_private=1),
}
# the ones the unfixed fold may be given: a multiple of 16 columns (a permutation inside the buffer) or an odd number of cells (refused on the host)
A_BEFORE_THE_FIX = ('A1_changepoints_520x32', 'A2_mixed_520x32', 'A3_walks_unfused_520x32', 'A4_changepoints_601x33_odd')

# B: declined by chain_padding_rule with post_private = 0 (the posteriors are kept: de-padding, refused for a full fit beyond 512 rows / switched off)
B_CASES = {
    'B_study_520x32': _case(study(520, 32, 0.3), (520, 32), hyper=False, post_private=0),
    'B_study_100x20_no_depad': _case(study(100, 20, 0.5), (100, 20), dict(chain_depad=0), hyper=False, post_private=0),
}

# C: the chain kernels run and the separate fold reads two strips of 1024 rows: strip-major is not row-major there
C_CASES = {
    'C1_walks_unfused_1024x32': _case(walks(1024, 32, WALKS5_TALL), (1024, 32), dict(fuse_accumulate=0), post_private=1),
}

DECLINED = dict(A_CASES, **B_CASES)
OPTION_DEFAULTS = dict(fuse_accumulate=1, chain_depad=1)


def strip_major_misread(post, n0, n1):
    """What accumulate2_kernel makes of a ROW-major step when it is told the step is strip-major: cell (row, col) is read from flat index
    ((col >> 4) * n0 + row) * 16 + (col & 15).  post: (T, n0, n1); -> the same shape, or None where an index leaves the step."""
    row, col = np.meshgrid(np.arange(n0), np.arange(n1), indexing='ij')
    src = ((col >> 4) * n0 + row) * 16 + (col & 15)
    if src.max() >= n0 * n1:
        return None
    flat = np.asarray(post, dtype=float).reshape(len(post), n0 * n1)
    return flat[:, src.ravel()].reshape(len(post), n0, n1)
