"""
Inputs of tests/test_observation_kernels.py (GPU) and of the CPU tests that hold the float64 oracle to the same bounds (tests/test_highprec.py)
and the host's choice of the Poisson route to its restatement (tests/test_host_logic.py): named rate grids and count records for the Poisson
model, named grids and data segments for the five models whose likelihood table blk::lik_table_kernel builds, and the restatement of
blhip_host_poisson_direct (include/blhip.h).

Every case holds three records; a test takes each alone (T = 1) and, for the cases of the *_BACKWARD lists, the first two and all three.
The prior of step 0 is likelihood_cases.reciprocal_prior of the step's true likelihood.
"""
import math

import numpy as np

NAN = float('nan')


# ---- Poisson: rate grids (n cells) and count records ----------------------------------------------------------------------------------------------

def rate_grid(kind, n):
    if kind == 'tutorial':                       # oint(0, 6, n): the coal-mining tutorial's
        return np.linspace(0.0, 6.0, n + 2)[1:-1]
    if kind == 'sixty':                          # (0, 60]
        return np.linspace(0.0, 60.0, n + 1)[1:]
    if kind == 'three_hundred':                  # (0, 300]: pow(lambda, k) overflows from k = 150 on
        return np.linspace(0.0, 300.0, n + 1)[1:]
    if kind == 'thousand':                       # (0, 1000]: exp(-lambda) leaves the normal range at 708.4 and is 0 from 745.2 on
        return np.linspace(0.0, 1000.0, n + 1)[1:]
    if kind == 'zero_first':                     # a custom grid whose first value is exactly 0; direct domain for small counts
        return np.linspace(0.0, 40.0, n)
    if kind == 'zero_first_wide':                # ... and one beyond the direct domain for EVERY count (rates above 708)
        return np.linspace(0.0, 900.0, n)
    if kind == 'million':                        # 1e6 +- 3e3
        return np.linspace(1.0e6 - 3.0e3, 1.0e6 + 3.0e3, n)
    raise ValueError(kind)


# name -> (rate grid, three records of d counts each)
POISSON_CASES = {
    'tutorial_1': ('tutorial', [[0], [1], [6]]),
    'tutorial_3': ('tutorial', [[0, 1, 6], [NAN, 6, NAN], [NAN, NAN, NAN]]),
    'tutorial_zero_normaliser': ('tutorial', [[1000], [0], [1]]),              # 6^1000 e^-6 / 1000! = 1e-1792: every cell is 0, the fit stops there
    'sixty_1': ('sixty', [[20], [50], [6]]),
    'sixty_nan_2': ('sixty', [[20, NAN], [NAN, 50], [NAN, NAN]]),
    'sixty_3': ('sixty', [[1, 20, 50], [6, NAN, 20], [NAN, NAN, 0]]),
    'three_hundred_direct': ('three_hundred', [[120], [50], [20]]),            # 120 ln 300 = 684: the last counts inside the direct domain
    'three_hundred_pow': ('three_hundred', [[170], [150], [125]]),             # k! is finite, lambda^k is not: 125 ln 300 = 713
    'three_hundred_big': ('three_hundred', [[171], [200], [400]]),             # k! = inf
    'three_hundred_mixed_2': ('three_hundred', [[200, NAN], [1000, 120], [NAN, 171]]),
    'thousand_1': ('thousand', [[0], [107], [1000]]),                          # exp(-lambda) underflows: (lambda = 740, k = 107) is 3.5e-187
    'thousand_3': ('thousand', [[400, 1000, NAN], [6, NAN, NAN], [NAN, NAN, NAN]]),
    'zero_first': ('zero_first', [[0], [6], [1]]),                             # lambda = 0 on the direct route: pow(0, 0) = 1
    'zero_first_log_2': ('zero_first', [[0, 171], [171, NAN], [0, 0]]),        # ... and on the log-space route (a count of 171 beside it), k = 0 and k > 0
    'zero_first_wide': ('zero_first_wide', [[0], [6], [400]]),                 # ... with every record beyond the direct domain
    'million': ('million', [[1000000], [999000], [1001500]]),
}
POISSON_BACKWARD = ['tutorial_1', 'sixty_nan_2', 'three_hundred_direct', 'three_hundred_pow', 'three_hundred_mixed_2', 'thousand_1', 'zero_first_wide']


def poisson_records(case):
    """(3, d) float64"""
    return np.array(POISSON_CASES[case][1], dtype=np.float64)


def poisson_rates(case, n):
    return rate_grid(POISSON_CASES[case][0], n)


# ---- the host's decision (blhip_host_poisson_direct): restated ----------------------------------------------------------------------------------

MAX_COUNT = 170.0          # 171! is inf in float64
MAX_LOG_POW = 700.0        # k ln(max rate): lambda^k overflows at ln(DBL_MAX) = 709.78; the margin of 9.78 is 1e13 times pow()'s own rounding
MAX_RATE = 708.0           # exp(-708) = 3.3e-308 is a normal number, exp(-708.4) is the smallest one


def direct_domain(rates, record):
    """whether the record (d counts, NaN ignored) is evaluated as lambda^k exp(-lambda) / k! on the grid `rates`"""
    ks = [float(k) for k in np.asarray(record, dtype=np.float64).reshape(-1) if k == k]
    kmax, rmax = max(ks) if ks else 0.0, float(np.max(rates))
    if kmax > MAX_COUNT or not rmax <= MAX_RATE:
        return False
    return kmax == 0.0 or rmax <= 1.0 or kmax * math.log(rmax) <= MAX_LOG_POW


def poisson_in_domain(case, steps, n=300):
    """every record `steps` of the case is in the direct domain: the float64 oracle can be held to the bound"""
    rates, recs = poisson_rates(case, n), poisson_records(case)
    return all(direct_domain(rates, recs[k]) for k in steps)


# the Poisson records the float64 oracle CANNOT evaluate (the reference raises OverflowError from k = 171 on, returns inf / NaN where lambda^k
# overflows and values without any precision where lambda^k meets a subnormal exp(-lambda)): every (case, record) outside the direct domain
# that holds a count above 0.  (A record of zeros alone is exp(-lambda) itself, which underflows as the true value does: the oracle runs it.)
POISSON_LEFT_OUT = [
    ('three_hundred_pow', 0), ('three_hundred_pow', 1), ('three_hundred_pow', 2),
    ('three_hundred_big', 0), ('three_hundred_big', 1), ('three_hundred_big', 2),
    ('three_hundred_mixed_2', 0), ('three_hundred_mixed_2', 1), ('three_hundred_mixed_2', 2),
    ('thousand_1', 1), ('thousand_1', 2), ('thousand_3', 0), ('thousand_3', 1),
    ('zero_first_log_2', 0), ('zero_first_log_2', 1),
    ('zero_first_wide', 1), ('zero_first_wide', 2),
    ('million', 0), ('million', 1), ('million', 2),
    ('tutorial_zero_normaliser', 0),
]


# ---- the table models ---------------------------------------------------------------------------------------------------------------------------
# grids: 1-D models 300 cells; 2-D models 24 x 20 and 33 x 7 (unequal sides, G = 480 and 231: no multiple of 256, so that a swapped or
# mis-strided index shows in every cell); Laplace also on 20 x 20, where a swap of the two indices stays inside both marginal arrays and shows as the
# transposed table.  A segment is (seg_len, d): AR1 models read rows x_(t-1), x_t.

TABLE_SHAPES = {'bernoulli': [(300,)], 'white_noise': [(300,)], 'laplace': [(24, 20), (33, 7), (20, 20)], 'ar1': [(24, 20), (33, 7)], 'scaled_ar1': [(24, 20), (33, 7)]}
LO, HI = -5.0, 5.0         # Laplace's location grid: range 10
RHO_EDGE = 1.0 - 2.0 ** -20


def table_grids(model, shape):
    if model == 'bernoulli':                     # below 0, above 1, and exactly 0 and 1
        p = np.linspace(-0.25, 1.25, shape[0])
        p[np.argmin(np.abs(p))] = 0.0
        p[np.argmin(np.abs(p - 1.0))] = 1.0
        return [p]
    if model == 'white_noise':                   # sigma over five decades
        return [np.geomspace(1e-2, 1e3, shape[0])]
    if model == 'laplace':                       # location cint(-5, 5); scales from the range down to 1e-5 of it
        return [np.linspace(LO, HI, shape[0]), np.geomspace(HI - LO, 1e-5 * (HI - LO), shape[1])]
    rho = np.linspace(-RHO_EDGE, RHO_EDGE, shape[0])             # strictly inside (-1, 1); negative values, both edges 1 - 2^-20
    rho[shape[0] // 2] = 0.0
    return [rho, np.geomspace(1e-2, 1e3, shape[1])]


def _laplace_position(name, n0):
    mu = np.linspace(LO, HI, n0)
    h = (HI - LO) / (n0 - 1)
    if name == 'node':
        return float(mu[n0 // 3])
    if name == 'between':
        return float(mu[n0 // 3] + 0.37 * h)
    if name == 'nan':
        return NAN
    side, k = name[:2], float(name[3:])
    return LO - k * (HI - LO) if side == 'lo' else HI + k * (HI - LO)


# name -> three segments; a segment is seg_len rows of d values
TABLE_CASES = {
    'bernoulli': {
        'zero_one': [[[0.0]], [[1.0]], [[NAN]]],
        'other_data': [[[2.0]], [[-1.0]], [[0.5]]],                          # any datum other than 0 counts as a success (:434)
        'dims_3': [[[0.0, 1.0, NAN]], [[2.0, NAN, 0.0]], [[NAN, NAN, NAN]]],
    },
    'white_noise': {
        'sizes': [[[0.0]], [[1.3]], [[1e3]]],                                # 0, O(1), and 1e3 sigma of the unit column (1e5 of the narrowest)
        'dims_2': [[[0.7, NAN]], [[NAN, NAN]], [[-2.5, 40.0]]],
    },
    'laplace': {
        'inside': [[['node']], [['between']], [['lo-1']]],
        'outside': [[['hi+1']], [['lo-10']], [['hi+100']]],
        'dims_2': [[['node', 'nan']], [['nan', 'nan']], [['between', 'hi+1']]],
    },
    'ar1': {
        'sizes': [[[0.0], [0.0]], [[0.8], [-1.1]], [[1e3], [1e3]]],
        'nan': [[[NAN], [0.5]], [[0.5], [NAN]], [[NAN], [NAN]]],             # a NaN in the first, the second, both values of the segment
        'dims_2': [[[0.4, NAN], [0.6, 1.0]], [[0.4, 0.3], [NAN, -0.2]], [[1.5, -30.0], [1.2, 28.0]]],
    },
}
TABLE_CASES['scaled_ar1'] = TABLE_CASES['ar1']
TABLE_BACKWARD = {'bernoulli': ['zero_one', 'dims_3'], 'white_noise': ['sizes'], 'laplace': ['inside', 'dims_2'], 'ar1': ['sizes', 'dims_2'],
                  'scaled_ar1': ['sizes', 'nan']}
SEG_LEN = {'bernoulli': 1, 'white_noise': 1, 'laplace': 1, 'ar1': 2, 'scaled_ar1': 2}


def table_segments(model, case, shape):
    """(3, seg_len, d) float64"""
    segs = TABLE_CASES[model][case]
    return np.array([[[v if isinstance(v, float) else _laplace_position(v, shape[0]) for v in row] for row in seg] for seg in segs], dtype=np.float64)
