"""Inputs of tests/test_chain_clamp.py and tests/test_chain_clamp_host.py: RegimeSwitch models on two-parameter grids inside the
chain-resident kernel (bayesloop_amd/csrc/blhip_chainclamp.hpp: blc::chain_clamp_kernel).  See tests/CHAIN_CLAMP.md."""
import numpy as np

import cases
import oracle_adapter as oa
from oracle import bl_oracle as orc

T = 6
LO, HI = -8.0, 8.0
VARIANT = 11                                      # blcp::VARIANT: lastTiming's fwd_ / bwd_kernel_variant of a pass on these kernels
# the smallest grids with at least two strips (one strip needs no exchange): exact 128 / 256 / 512 rows x 32 columns; padded: 100 x 40 runs
# as 128 x 48 (three strips, padding in rows and in columns), 200 x 40 as 256 x 48, 400 x 40 as 512 x 48
EXACT = [(128, 32), (256, 32), (512, 32)]
PADDED = [(100, 40), (200, 40), (400, 40)]
GRIDS = EXACT + PADDED
ROWS_384 = (300, 40)                              # runs padded inside 512 rows (no 384-row kernels)
RINGS = [4, 8, 12, 16, 20, 24]
# log10pMin: 10**-330 underflows to 0 (nothing is clamped) ... +1: every cell is clamped (the prior of the next step is uniform)
PMIN = [-330, -7, -3, 1]


def g2(n0, n1):
    # (std >= 0.5: the largest exponent is 16^2 / (2 x 0.25) = 512 < 708 -- no likelihood value is 0 or subnormal, so EVERY localEvidence entry
    #  is compared at the bar, none under the registered exception for ill-conditioned steps)
    return ('Gaussian', [('mean', cases._g('cint', LO, HI, n0)), ('std', cases._g('cint', 0.5, 4, n1))], 'default')


def ntw_of(n0):
    return 1 if n0 <= 128 else (2 if n0 <= 256 else 4)


def chain_sigmas(nk, n0, lo=LO, hi=HI):
    """Three walk widths whose SciPy radii int(4 sigma / lattice + 0.5) (transitionModels.py:108-111) are r0 - 1, r0 - 2, r0 - 3 for the
    band radius r0 of ring length nk; nk = 4: radius 0 (the walk is a copy, :113).  (The construction of tests/test_kernel_sweep.py.)"""
    lattice = (hi - lo) / (n0 - 1.0)
    if nk == 4:
        return [0.0, 1e-9 * lattice, 2e-9 * lattice]
    r0 = 2 * nk - 8
    return [(r0 - 1 - k) / 4.0 * lattice for k in range(3)]


def kernel(nk, ntw, bwd, store):
    return 'blc::chain_clamp_kernel<%d, %d, %s, %s>' % (nk, ntw, 'true' if bwd else 'false', 'true' if store else 'false')


def kernels_of(nk, ntw, kind):
    """what a fit of `kind` launches: 'evidence' / 'forward' / 'full'"""
    if kind == 'evidence':
        return [kernel(nk, ntw, False, False)]
    if kind == 'forward':
        return [kernel(nk, ntw, False, True)]
    return [kernel(nk, ntw, False, True), kernel(nk, ntw, True, True)]


def model(name, sigma, pmin):
    """walk then switch (clamp mode 2), switch then walk (mode 1), switch alone (mode 1 without a stencil: ring length 4)"""
    walk, rs = ('GRW', 'sigma', sigma, 'mean', None), ('RS', 'log10pMin', pmin, None)
    return {'walk_then_switch': ('Combined', [walk, rs]), 'switch_then_walk': ('Combined', [rs, walk]), 'switch_alone': rs}[name]


def study(grid, tm, seed, kind='full', study='Study'):
    fit = dict(evidence=dict(evidenceOnly=True), forward=dict(forwardOnly=True), full={})[kind]
    return dict(study=study, data=('series', seed, T), om=g2(*grid), tm=tm, fit=fit)


def seed_of(grid, nk):
    return 11000 + 97 * nk + grid[0] + grid[1]


def clamped_cells(case):
    """Per forward transition of a one-chain case (steps 1 .. T - 1): how many cells the RegimeSwitch raises -- counted on the ORACLE's
    side (the normalised filtered distributions of a forward-only oracle fit, the model's stages in front of the switch applied to them)."""
    c = dict(case, study='Study', fit=dict(forwardOnly=True))
    with np.errstate(all='ignore'):
        r = oa.run(c)
    g = r['grid']
    pnames = [p[0] for p in c['om'][1]]
    ops, vals, _ = oa.flatten_tm(c['tm'], pnames)
    vals = orc.align_values(ops, [float(np.ravel(v)[0]) for v in vals])
    k = [o[0] for o in ops].index('regimeswitch')
    limit = (10. ** vals[k]) * np.prod(g.lattice)
    counts = []
    for t in range(1, T):
        x = orc.transition_forward(ops[:k], vals[:k], np.array(r['posteriorSequence'][t - 1]), t - 1, g, None) if k > 0 else r['posteriorSequence'][t - 1]
        counts.append(int((np.asarray(x) < limit).sum()))
    return counts, int(np.prod(g.size))
