"""
Inputs of tests/test_likelihood_kernels.py (GPU) and of the CPU test that holds the float64 oracle to the same bounds
(tests/test_highprec.py): mean / std grids, data records, the prior that makes every cell observable, and the restatement of the host's
decision between the likelihood recurrence and the per-cell exponential (blhip_host_rec_envelope, include/blhip.h; pinned against the
library by tests/test_host_logic.py).

The mean grid is linspace(-8, 8, n0) for every geometry (range 16); the second axis is a custom log-spaced std grid -- only the row axis
has to be equally spaced for the recurrence.  Data positions are named relative to that grid:
    node / between   a grid node a third of the way up / 0.37 steps above it
    lo / hi          the grid's two ends
    lo-1, hi+1 ..    1, 10 and 100 grid ranges outside, on the side the rows recede from (lo-) and on the side they approach (hi+)
"""
import math

import numpy as np

LO, HI = -8.0, 8.0
RANGE = HI - LO
NAN = float('nan')


def mean_grid(n0, uneven=False):
    x = np.linspace(LO, HI, n0)
    if uneven:                                   # NOT equally spaced: the per-cell exponential flavours of the launch-per-step kernels
        x = x + 0.2 * RANGE / (n0 - 1) * np.sin(np.arange(n0))
    return x


STD_ENDS = {
    'wide': (RANGE / 4, RANGE / 16),             # no cell underflows for data inside the grid: the p / L sums are finite
    'narrow': (RANGE / 4, RANGE * 2e-3),         # inside the recurrence's envelope for data up to 10 ranges outside
    'decades': (RANGE / 4, RANGE * 1e-5),        # many decades narrower than the grid: beyond the envelope
    'outlier': (RANGE / 4, 1e-3),                # the first overflow case: a std column of 1e-3 (with the datum x = -100)
    'clamp': (RANGE / 4, 2e-4),                  # the second one: s ~ 2e-4, a datum at the far edge of the grid
    'edge': (RANGE / 4, None),                   # down to the narrowest column the envelope still admits (envelope_edge_std: s ~ 1e-3)
}


def std_grid(kind, n1, narrowest=None):
    a, b = STD_ENDS[kind]
    if b is None:
        b = narrowest
    s = np.geomspace(a, b, n1)
    s[-1] = b
    return s


def position(name, n0):
    mu = mean_grid(n0)
    h = RANGE / (n0 - 1)
    if name == 'node':
        return float(mu[n0 // 3])
    if name == 'node2':
        return float(mu[(2 * n0) // 3])
    if name == 'between':
        return float(mu[n0 // 3] + 0.37 * h)
    if name == 'lo':
        return LO
    if name == 'hi':
        return HI
    if name == 'nan':
        return NAN
    side, k = name[:2], float(name[3:])          # 'lo-10', 'hi+100'
    return LO - k * RANGE if side == 'lo' else HI + k * RANGE


# name -> (std grid, three records of d positions each: step 0, 1, 2)
CASES = {
    'inside_1': ('narrow', [['node'], ['between'], ['lo']]),
    'inside_nan_2': ('narrow', [['hi', 'nan'], ['nan', 'between'], ['nan', 'nan']]),
    'inside_wide_4': ('wide', [['node', 'between', 'lo', 'hi'], ['node', 'nan', 'between', 'nan'], ['nan', 'nan', 'nan', 'hi']]),
    'inside_wide_1': ('wide', [['between'], ['node2'], ['hi']]),
    'inside_3': ('narrow', [['node', 'node2', 'nan'], ['between', 'between', 'between'], ['nan', 'nan', 'nan']]),
    'outside_1': ('wide', [['lo-1'], ['hi+1'], ['node']]),
    'outside_1_narrow_2': ('narrow', [['lo-1', 'nan'], ['hi+1', 'hi+1'], ['lo-1', 'hi+1']]),       # (two values on opposite sides)
    'outside_10': ('wide', [['lo-10'], ['hi+10'], ['between']]),
    'outside_10_narrow_2': ('narrow', [['hi+10', 'node'], ['nan', 'lo-10'], ['node', 'nan']]),
    'outside_100': ('wide', [['lo-100'], ['hi+100'], ['node']]),
    'outside_100_narrow_2': ('narrow', [['nan', 'hi+100'], ['lo-100', 'node'], ['between', 'nan']]),
    'decades_1': ('decades', [['node'], ['between'], ['hi']]),
    'decades_4': ('decades', [['node', 'nan', 'lo', 'between'], ['nan', 'nan', 'nan', 'nan'], ['hi+1', 'nan', 'nan', 'nan']]),
    # the two routes of the exponent defect: x = -100 against a std column of 1e-3; a datum at either end of the grid against s = 2e-4
    'overflow_outlier': ('outlier', [[-100.0], ['node'], [-100.0]]),
    'overflow_clamp': ('clamp', [['hi'], ['lo'], ['node']]),
    # just INSIDE the envelope: the host's bound at 0.98e9, the recurrence still runs (its anchors' arguments reach ~1e8 here)
    'envelope_edge': ('edge', [['lo'], ['node'], ['hi']]),
}
BACKWARD_CASES = ['envelope_edge', 'inside_wide_4', 'inside_wide_1', 'inside_1', 'inside_nan_2', 'outside_1', 'decades_1', 'overflow_outlier', 'overflow_clamp']


def records(case, n0):
    """(3, d) float64: the case's three records on the mean grid of n0 rows"""
    return np.array([[p if isinstance(p, float) else position(p, n0) for p in rec] for rec in CASES[case][1]], dtype=np.float64)


def std_of(case, n1, n0=None):
    kind = CASES[case][0]
    return std_grid(kind, n1, envelope_edge_std(case, n0) if kind == 'edge' else None)


EDGE_FILL = 0.98          # how much of the envelope the 'edge' grid uses


def envelope_edge_std(case, n0):
    """the narrowest std column with which the case's three records together reach EDGE_FILL of the envelope on the mean grid of n0 rows
    (bisection on envelope_bound, which falls monotonically with s)"""
    mu, recs = mean_grid(n0), records(case, n0)
    lo, hi = 1e-5, 1.0
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if envelope_bound(mu, [mid], recs) > EDGE_FILL * ENVELOPE:
            lo = mid
        else:
            hi = mid
    return hi


def reciprocal_prior(L):
    """1 / L in float64 clipped to the float64 range, 1 where the rounded likelihood is 0: prior * L is O(1) wherever L is a normal number,
    so the T = 1 posterior shows every cell's own relative error.  L: the longdouble likelihood of step 0."""
    L64 = np.asarray(L).astype(np.float64)
    big = np.finfo(np.float64).max
    with np.errstate(divide='ignore', over='ignore'):
        p = np.where(L64 == 0.0, 1.0, np.minimum(1.0 / np.where(L64 == 0.0, 1.0, L64), big))
    return p


# ---- the host's decision (blhip_host_rec_envelope): restated --------------------------------------------------------------------------------

ENVELOPE = 1.0e9          # the largest |argument| the recurrence accepts: below exp_mn's clamp (1.4e9), times log2(e) below 2^31
PAD_ROWS = 256            # rows of lattice continued beyond either end (padded tiles of the resident and chain kernels)
MAX_STRIDE, MAX_STEPS = 4, 32


def envelope_bound(mu, s, recs):
    """The host's bound of |a0| + steps |d1| + steps^2 / 2 |d2| over the padded lattice, every record and every std column."""
    mu = np.asarray(mu, dtype=np.float64)
    n0 = len(mu)
    step = abs((mu[-1] - mu[0]) / (n0 - 1))
    lo, hi = min(mu[0], mu[-1]) - PAD_ROWS * step, max(mu[0], mu[-1]) + PAD_ROWS * step
    D, dn = 0.0, 0.0
    for rec in np.asarray(recs, dtype=np.float64).reshape(len(recs), -1):
        ok = rec[rec == rec]
        dn = max(dn, float(len(ok)))
        for x in ok:
            D = max(D, abs(x - lo), abs(x - hi))
    s = np.asarray(s, dtype=np.float64)
    cA = float(np.max(1.0 / (2.0 * s * s)))
    cB = float(np.max(np.abs(0.5 * np.log(2.0 * math.pi * s * s))))
    H = MAX_STRIDE * step
    return dn * (D * D * cA + cB) + MAX_STEPS * (2.0 * cA * H * dn * D) + 0.5 * MAX_STEPS * MAX_STEPS * (2.0 * cA * dn * H * H)


def recurrence_accepted(mu, s, recs):
    return bool(envelope_bound(mu, s, recs) <= ENVELOPE)
