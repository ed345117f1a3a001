"""
The scale rules of the kernels that normalise lazily, restated from their documentation (blhip_book.hpp: resident_unlag, chain_unlag,
forward_bookkeeping; the headers of blhip_resident.hpp, blhip_chainres.hpp, blhip_chainclamp.hpp, blhip_fused1d.hpp): what the state of step k
sums to when the reference's normalisers are n_0, n_1, ...  Shared by tests/test_host_logic.py (which pins the host's inverse, blhip_host_unlag,
to it) and tests/highprec.py (whose bounds carry the subnormal step through these scales).  Plain arithmetic on the values it is given: float64
for float64 normalisers, longdouble for longdouble ones.  Nothing here reads a device's output.

A RULE is a tuple:
    ('step',)            the launch-per-step kernels, bl1c::chain1d_kernel / chain1d_long_kernel: the step divides by the sum of the step before,
                         the stored row of step k sums to n_k
    ('launch', K)        bl1f::fused1d_kernel / bl1p::persist1d_kernel: K steps per launch (superstep) without a division in between, the first
                         step of a launch divides by the last sum of the launch before: the product of the normalisers since that first step
    ('norm_lag', lag)    the chain-resident family: s_k = S_(k-lag-1) s_(k-lag) / S_(k-lag), 1 while k < lag, S_(-1) = 1 -- the state carries the
                         product of the last `lag` normalisers; a clamped step (blc::chain_clamp_kernel) runs at the exact scale 1 / S_(k-1)
    ('sum_lag', lag)     blr::resident_kernel: s_k = 1 / S_(k-lag), 1 while k < lag
In every rule S_k = (S_(k-1), or 1 at step 0 and at a restart -- a step that consumes a distribution of known mass) s_k n_k.
"""
import numpy as np

RANGE_LO, RANGE_HI = 1e-150, 1e150      # resident_unlag / chain_unlag and the backward checks: a lagged sum outside falls back (BLHIP_FALLBACK_RANGE)
POSTERIOR_FLOOR = 1e-250                # ... and so does a backward pass whose posterior sum is not above it
RAW_FLOOR = 1e-200                      # forward_ / backward_bookkeeping: a raw sum of a K-steps-per-launch pass not above it repeats the fit with K = 1
MARGIN = 1e6                            # a predicted sum within this factor of a threshold makes the prediction a matter of rounding: refused


def simulate_sums(norms, lag, scheme, kinds=None, clamped=None):
    """What a resident kernel reports: S_k = (S_(k-1) or 1 at a restart) * s_k * n_k with the kernel's rule for s_k.  scheme 0: the lagged SUM
    (time-resident), 1: the lagged NORMALISER (chain-resident), 2: scheme 1 with clamped steps (`clamped[k]` not 0: s_k = 1 / S_(k-1), which the
    lagged rule of the steps behind it reads like any other).  kinds[k] not 0: step k is a restart.  -> (S, s)"""
    T = len(norms)
    dt = np.longdouble if np.asarray(norms).dtype == np.longdouble else np.float64
    S, s = np.zeros(T, dtype=dt), np.ones(T, dtype=dt)
    one = dt(1.0)
    for k in range(T):
        if k >= lag:
            s[k] = one / S[k - lag] if scheme == 0 else (S[k - lag - 1] if k - lag - 1 >= 0 else one) * s[k - lag] / S[k - lag]
        if scheme == 2 and clamped is not None and k > 0 and clamped[k]:
            s[k] = one / S[k - 1]
        fresh = k == 0 or (kinds is not None and kinds[k] != 0)
        S[k] = (one if fresh else S[k - 1]) * s[k] * norms[k]
    return S, s


class History:
    """simulate_sums one step at a time, for a pass whose normalisers become known as it goes: pre() is the scale of the un-normalised state
    of the next step (S_k / n_k: what the kernel's values are relative to the reference's before its own sum enters), push(n) records the step."""

    def __init__(self, rule):
        self.rule = tuple(rule)
        assert self.rule[0] in ('step', 'launch', 'norm_lag', 'sum_lag') and (self.rule[0] == 'step' or int(self.rule[1]) >= 1), rule
        self.S, self.s = [], []

    def _scale(self, fresh, clamped):
        k, kind = len(self.S), self.rule[0]
        one = np.longdouble(1)
        if kind == 'step':
            return one if (k == 0 or fresh) else one / self.S[k - 1]
        if kind == 'launch':
            return one if (k == 0 or fresh or k % self.rule[1]) else one / self.S[k - 1]
        lag = self.rule[1]
        s = one
        if k >= lag:
            s = one / self.S[k - lag] if kind == 'sum_lag' else (self.S[k - lag - 1] if k - lag - 1 >= 0 else one) * self.s[k - lag] / self.S[k - lag]
        if clamped and k > 0:
            assert kind == 'norm_lag'
            s = one / self.S[k - 1]
        return s

    def pre(self, fresh=False, clamped=False):
        k = len(self.S)
        return (np.longdouble(1) if (k == 0 or fresh) else self.S[k - 1]) * self._scale(fresh, clamped)

    def push(self, n, fresh=False, clamped=False):
        s = self._scale(fresh, clamped)
        c = self.pre(fresh, clamped)
        self.s.append(s)
        self.S.append(c * np.longdouble(n))

    def last(self):
        """what the state left by the last recorded step sums to (1 before any)"""
        return self.S[-1] if self.S else np.longdouble(1)


def parse_rule(rule):
    """'step', 'launch(8)', 'norm_lag(4)', 'sum_lag(2)' or the tuple itself -> the tuple"""
    if isinstance(rule, str):
        if '(' in rule:
            name, arg = rule.rstrip(')').split('(')
            return (name.strip(), int(arg))
        return (rule.strip(),)
    return tuple(rule)
