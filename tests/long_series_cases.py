"""
The problems of tests/test_long_series.py (GPU: the kernels that carry a lazily scaled state ALONG TIME, over 14 and 26 steps, against
tests/highprec.py), kept apart from it so that tests/test_highprec.py can run the float64 oracle on every one of them, hold it to the same
bounds and assert the conditions on the schedules without a GPU.

A FAMILY extends one case of tests/step_transition_cases.py (its shape, engine options, transition list and chains; no new shape) to T steps
and names the family's scale rule (tests/scale_rules.py).  Every step has a table likelihood 2^(e_t) y_t, y_t dense in [0.5, 1.5]: a power of two
is exact, so the reference's posteriors do not depend on the SCHEDULE e_t, only its normalisers -- and with them the scale of every lazily
normalised state -- do.  The prior is the case's `cube` input (`edges` for the long row).

What a rule predicts from the reference's own longdouble normalisers -- the sums the kernels report -- decides, before anything runs, whether
the host's guard fires (scale_rules.RANGE_LO / RANGE_HI / POSTERIOR_FLOOR / RAW_FLOOR); a prediction within scale_rules.MARGIN of a threshold is
refused here (verdict 'refused': not run; tests/test_highprec.py asserts the exact list).  Every predicted sum is finite and inside (1e-290, 1e290): these
problems walk the documented range fallback and provoke nothing.
"""
import math

import numpy as np

import highprec as hp
import scale_rules as sr
import step_transition_cases as sc
import transition_cases as tc
from bayesloop_amd import _abi

T_LONG, T_RESONANT = 14, 26
BURST = (5, 6, 7, 8, 9)                 # the steps of a burst: across the boundary between two launches of the fused kernel (6 steps each) and across the ring's wrap at 8
FINITE = (1e-290, 1e290)


SHIFT_STEPS = (4, 9)


def _there_and_back(d, T):
    """a shift by d into step 4 and by -d into step 9, none elsewhere.  The running bound of the spline shift is a worst case over the signs of its
    weights and grows about twelvefold per shift: a shift at EVERY step outgrows the renormalising sum it bounds behind 13 of them
    (well_conditioned then drops every chain); two keep it at 1e-11 of the sum"""
    return tuple(d if k + 1 == SHIFT_STEPS[0] else (-d if k + 1 == SHIFT_STEPS[1] else 0.0) for k in range(T - 1))


def launch_steps(fuse1d, T, lw, TJ=128):
    """the steps per launch the host plans for a K-steps-per-launch pass, restated (blhip_batch.hpp): min(fuse1d, T), shortened until the halo
    that the neighbouring blocks recompute, K lw cells per side, is within twice the TJ = 128 cells a block owns and the window fits 96 KB"""
    K = max(1, min(int(fuse1d), int(T)))
    while K > 1 and (K * lw > 2 * TJ or (TJ + 2 * K * lw) * 32 > 96 * 1024):
        K -= 1
    return K


# family -> the case it extends, its scale rule, the input kind, chains (None: the case's own; a function of T otherwise)
FAMILIES = {
    'resident': dict(case='resident_32x32', rule=('sum_lag', 2), kind='cube'),
    'chain': dict(case='chain_128x16', rule=('norm_lag', 4), kind='cube'),
    # change points behind steps 5 and 9 (a restart while the lagged rule reads sums from before it, and one behind another); one chain never fires
    'chain_sources': dict(case='chain_sources_128x16', rule=('norm_lag', 4), kind='cube', chains=lambda T: [(7, 5), (6, 9), (5, 10 * T)]),
    'chainax': dict(case='chainax_100x90', rule=('norm_lag', 4), kind='cube'),
    'chain1d_walks': dict(case='chain1d_walks_300', rule=('step',), kind='cube'),
    'chain1d_shifts': dict(case='chain1d_shifts_300', rule=('step',), kind='cube',
                           chains=lambda T: [(_there_and_back(d, T),) for (d,) in sc.CASES['chain1d_shifts_300']['chains']]),
    'chain1d_long': dict(case='chain1d_long_walks_4100', rule=('step',), kind='edges'),
    # (fuse1d = 8, but the batch's widest walk has radius 40: the host plans 6 steps per launch -- launches of 6, 6 and 2 steps at T = 14)
    'fused1d': dict(case='fused1d_walks_300', rule=('launch', launch_steps(8, T_LONG, 40)), kind='cube'),
    'persist1d': dict(case='persist1d_walks_300', rule=('launch', launch_steps(2, T_LONG, 40)), kind='cube'),
    'generic': dict(case='generic_walks_24x20', rule=('step',), kind='cube'),          # the control: every range fallback lands on kernels of this rule
}
LAG_SWEEP = {'chain': [('norm_lag', lag) for lag in (2, 3, 4)], 'chain_sources': [('norm_lag', lag) for lag in (2, 3, 4)],
             'chainax': [('norm_lag', lag) for lag in (2, 3, 4)], 'resident': [('sum_lag', lag) for lag in (1, 2, 3)]}
LAG_OPTION = {'norm_lag': 'chain_resident_lag', 'sum_lag': 'resident_lag'}
LAG_SCHEDULES = ('flat', 'burst_in', 'burst_mild')
FORWARD_ONLY = ('resident', 'chain', 'chainax', 'chain1d_walks', 'fused1d', 'generic')     # families whose case has the forward driver ...
FORWARD_SCHEDULES = ('flat', 'ramp')                                                      # ... on these schedules


# ---- schedules ---------------------------------------------------------------------------------------------------------------------------------

def resonant_amplitude(decades, T=T_RESONANT):
    """the smallest integer a for which the time-resident rule, restated (scale_rules.simulate_sums(.., 2, 0)) on the normalisers
    2^round(a cos(pi t / 3)), predicts a sum beyond 1e+-decades within T steps: x_k = x_(k-1) - x_(k-2) + nu_k has period 6, so a drive of
    period 6 grows linearly"""
    for a in range(1, 200):
        S, _ = sr.simulate_sums(np.exp2(hp._ld(_resonant(a, T))), 2, 0)
        if float(np.max(np.abs(np.log10(S)))) >= decades:
            return a
    raise AssertionError(decades)


def _resonant(a, T):
    return np.array([round(a * math.cos(math.pi * t / 3.0)) for t in range(T)], dtype=np.int64)


RESONANT_IN, RESONANT_OUT = resonant_amplitude(110), resonant_amplitude(165)

SCHEDULES = {
    'flat': (T_LONG, lambda T: np.zeros(T, dtype=np.int64)),
    'ramp': (T_LONG, lambda T: np.full(T, -100, dtype=np.int64)),
    'ramp_80': (T_LONG, lambda T: np.full(T, -80, dtype=np.int64)),         # the ramp whose backward posterior sums stay clear of the 1e-250 floor (LAGGED)
    'burst_in': (T_LONG, lambda T: np.array([-110 if t in BURST else 0 for t in range(T)], dtype=np.int64)),
    'burst_out': (T_LONG, lambda T: np.array([-130 if t in BURST else 0 for t in range(T)], dtype=np.int64)),
    'burst_mild': (T_LONG, lambda T: np.array([-40 if t in BURST else 0 for t in range(T)], dtype=np.int64)),   # inside the guard at lag 3 of the lagged sum (LAGGED)
    'alternate': (T_LONG, lambda T: np.array([200 if t % 2 == 0 else -200 for t in range(T)], dtype=np.int64)),
    'resonant_in': (T_RESONANT, lambda T: _resonant(RESONANT_IN, T)),
    'resonant_out': (T_RESONANT, lambda T: _resonant(RESONANT_OUT, T)),
}


def steps_of(schedule):
    return SCHEDULES[schedule][0]


def exponents(schedule):
    T, f = SCHEDULES[schedule]
    return f(T)


# ---- problems ------------------------------------------------------------------------------------------------------------------------------------

def case_of(fam, T):
    F = FAMILIES[fam]
    base = sc.CASES[F['case']]
    chains = base['chains'] if F.get('chains') is None else [tuple(c) for c in F['chains'](T)]
    return dict(base, chains=chains)


def tables(fam, schedule):
    """-> (prior, likelihood tables (T, *shape), reset prior, independent prior): float64, as given to the library"""
    F = FAMILIES[fam]
    base = sc.CASES[F['case']]
    shape = base['shape']
    seed = sum(ord(ch) for ch in base['name']) % 97
    axis = sc.line_axis(base, seed)
    T = steps_of(schedule)
    rng = np.random.default_rng(5000 + seed)
    y = 0.5 + rng.random((T,) + shape)                           # (the same y for every schedule: the posteriors of a family are one set)
    lik = np.ldexp(y, exponents(schedule).reshape((T,) + (1,) * len(shape)).astype(np.int32))
    assert np.all(np.isfinite(lik)) and np.all(lik > 0) and np.array_equal(np.ldexp(lik, -exponents(schedule).reshape((T,) + (1,) * len(shape)).astype(np.int32)), y)
    return sc.state(F['kind'], shape, seed, axis), lik, sc.state('cube', shape, seed + 1, axis), sc.state('decades', shape, seed + 2, axis)


_REF = {}


def _fit(fam, schedule, full, rule):
    key = (fam, schedule, full, rule)
    if key not in _REF:
        if len(_REF) > 24:
            _REF.clear()
        T = steps_of(schedule)
        case = case_of(fam, T)
        shape = case['shape']
        prior, lik, reset, indep = tables(fam, schedule)
        grids = [np.arange(n, dtype=np.float64) for n in shape]
        drv = 'three' if full else 'forward'
        refs = [hp.transition_fit(prior, [(L, None) for L in lik], sc.stage_program(case, params, drv, T), grids, [1.0] * len(shape),
                                  nblk=sc.nblk_of(shape), full=full, shared=dict(reset=reset, indep=indep), scale=rule)
                for params in case['chains']]
        _REF[key] = refs
    return _REF[key]


def conditioned(refs):
    return [all(tc.well_conditioned(D, eD, hp.SLACK) for D, eD in ref['sums']) for ref in refs]


def predicted_sums(ref, full):
    """-> (forward sums [T], backward sums and posterior sums of the backward pass, [] for a forward-only fit): float, as the rule predicts them"""
    s = ref['scale']
    fwd = [float(x) for x in s['fwd']]
    back = ([float(x) for x in s['bwd']] + [float(s['post'][t]) for t in sorted(s['post'])]) if full else []
    return fwd, back


def _near(x, threshold):
    return threshold / sr.MARGIN < x < threshold * sr.MARGIN


def prediction(refs, rule, full):
    """What the host's guard does with the sums the rule predicts, over the chains of the batch: 'none' (the family's kernels deliver the result),
    'range' (BLHIP_FALLBACK_RANGE: the launch-per-step kernels do), 'repeat' (a K-steps-per-launch pass repeated with K = 1), or 'refused': a
    predicted sum lies within scale_rules.MARGIN of the threshold that decides.  The forward pass is judged first: the host does not launch
    the backward pass of a fit whose forward sums failed.  -> (verdict, extreme forward sums (min, max), extreme backward sums)"""
    kind = rule[0]
    lo_f = hi_f = lo_b = hi_b = 1.0
    fired, near = False, False
    for ref in refs:
        fwd, _ = predicted_sums(ref, full)
        lo_f, hi_f = min([lo_f] + fwd), max([hi_f] + fwd)
        assert all(FINITE[0] < x < FINITE[1] for x in fwd), (rule, fwd)
    if kind == 'step':
        return 'none', (lo_f, hi_f), (lo_b, hi_b)

    def judge(xs, lo, hi=None):
        """a sum clearly beyond a threshold decides whatever the others do; one within the margin of it, and none beyond, decides nothing"""
        nonlocal fired, near
        for x in xs:
            close = _near(x, lo) or (hi is not None and _near(x, hi))
            near = near or close
            fired = fired or (not close and (x <= lo or (hi is not None and x >= hi)))

    for ref in refs:
        fwd, _ = predicted_sums(ref, full)
        judge(fwd, sr.RAW_FLOOR) if kind == 'launch' else judge(fwd, sr.RANGE_LO, sr.RANGE_HI)
    if not fired and not near and full:
        for ref in refs:
            _, back = predicted_sums(ref, full)
            assert all(FINITE[0] < x < FINITE[1] for x in back), (rule, back)
            lo_b, hi_b = min([lo_b] + back), max([hi_b] + back)
            post = [float(ref['scale']['post'][t]) for t in sorted(ref['scale']['post'])]
            if kind == 'launch':
                judge(post, sr.RAW_FLOOR)
            else:
                judge([float(x) for x in ref['scale']['bwd']], sr.RANGE_LO, sr.RANGE_HI)
                judge(post, sr.POSTERIOR_FLOOR)
    verdict = ('repeat' if kind == 'launch' else 'range') if fired else ('refused' if near else 'none')
    return verdict, (lo_f, hi_f), (lo_b, hi_b)


def reference(fam, schedule, full=True, rule=None):
    """-> dict(refs: per chain the longdouble pass with the bounds of the rule that DELIVERS the result, keep: the chains that are run, verdict,
    fwd / bwd: the extreme sums the family's rule predicts).  A fit the guard sends to the launch-per-step kernels, or repeats with one step per
    launch, is held to the bounds of the rule `step` -- those kernels' own."""
    rule = FAMILIES[fam]['rule'] if rule is None else tuple(rule)
    mine = _fit(fam, schedule, full, rule)
    verdict, fwd, bwd = prediction(mine, rule, full)
    refs = mine if verdict in ('none', 'refused') else _fit(fam, schedule, full, ('step',))
    ok = conditioned(refs)
    return dict(refs=refs, keep=[b for b, o in enumerate(ok) if o], verdict=verdict, fwd=fwd, bwd=bwd, rule=rule)


# the 26-step schedules exist for the lagged rules; the long row's rule is `step`, and its longdouble reference (a walk of radius 300 on 4100 cells)
# costs more CPU time than every other family together: it runs the 14-step schedules
NOT_RUN = [('chain1d_long', 'resonant_in'), ('chain1d_long', 'resonant_out')]
# ... and the two schedules that exist for the lagged rules alone run on the families that have one
LAGGED = ('resident', 'chain', 'chain_sources', 'chainax')
NOT_RUN += [(fam, schedule) for fam in FAMILIES if fam not in LAGGED for schedule in ('ramp_80', 'burst_mild')]


# ... and the full fits whose prediction is 'refused' (named here so that nothing is computed when the GPU file is collected; computed and
# asserted equal by tests/test_highprec.py).  ramp: the forward sums of the chain family reach 4e-121 as intended, but the backward pass's posterior
# sum is the product of the forward row's and the backward message's scales, 7e-245: at the 1e-250 floor.  The forward-only fits run the ramp.
REFUSED = [('chain', 'ramp'), ('chain_sources', 'ramp'), ('chainax', 'ramp')]


def combinations(refused=False):
    return [(fam, schedule) for fam in FAMILIES for schedule in SCHEDULES if (fam, schedule) not in NOT_RUN and (refused or (fam, schedule) not in REFUSED)]


def forward_combinations():
    return [(fam, schedule) for fam in FORWARD_ONLY for schedule in FORWARD_SCHEDULES]


def lag_combinations():
    return [(fam, schedule, rule) for fam, rules in LAG_SWEEP.items() for schedule in LAG_SCHEDULES for rule in rules if rule != FAMILIES[fam]['rule']]


# ---- one engine call per problem: shared by the GPU file (the library) and tests/test_highprec.py (the float64 oracle) ------------------------

def run_problem(engine, fam, schedule, keep, full=True, one_at_a_time=False):
    """-> dict(log_evidence (B,), local_evidence (B, T), means (B, ndim, T), posts [B] of (T, *shape), timing [per call]) for the chains `keep`"""
    from bayesloop_amd.engine import FitProblem
    T = steps_of(schedule)
    case = case_of(fam, T)
    shape = list(case['shape'])
    G = int(np.prod(shape))
    prior, lik, reset, indep = tables(fam, schedule)
    ops, values = sc.abi_program(case, 'three' if full else 'forward', T)
    values = np.ascontiguousarray(values[list(keep)])
    problem = FitProblem(obs_model=_abi.OM_TABLE, marginal=[np.arange(n, dtype=np.float64) for n in shape], lattice=[1.0] * len(shape),
                         data=np.zeros((T, 1)), timestamps=np.arange(T, dtype=np.float64), prior=prior, ops=ops, lik=lik.reshape(T, G),
                         reset_prior=reset, indep_prior=indep, seg_len=1)
    out = dict(log_evidence=[], local_evidence=[], means=[], posts=[], timing=[])
    for rows in ([[b] for b in range(len(values))] if one_at_a_time else [list(range(len(values)))]):
        res = engine.fit(problem, values[rows], forward_only=not full, keep_posterior=True)
        assert np.all(res.abort_step < 0), (fam, schedule, res.abort_step)
        out['log_evidence'] += list(res.log_evidence)
        out['local_evidence'] += list(res.local_evidence)
        out['means'] += list(res.posterior_mean)
        out['posts'] += [np.array(engine.posterior(b, T, shape)) for b in range(len(rows))]
        out['timing'].append(dict(res.timing or {}))
    return out


def compare(chk, fam, schedule, keep, got, refs, full=True):
    """every cell of every posterior, logEvidence, local_evidence and the means of the chains `keep` against their references"""
    T = steps_of(schedule)
    chains = case_of(fam, T)['chains']
    for k, b in enumerate(keep):
        ref = refs[b]
        w = '%s %s %s chain %d %r' % (fam, schedule, 'full' if full else 'forward', b, chains[b] if len(repr(chains[b])) < 40 else chains[b][0][:2])
        chk.within([got['log_evidence'][k]], [ref['log_evidence'][0]], [ref['log_evidence'][1]], w + ' logE')
        for t in range(T):
            loc = ref['local'][t] if full else ref['local_fwd'][t]
            if np.isfinite(float(loc[1])) or np.isnan(float(loc[0])):
                chk.within([got['local_evidence'][k][t]], [loc[0]], [loc[1]], w + ' localEvidence[%d]' % t)
            else:
                chk.bad.append(w + ' localEvidence[%d]: the restatement has no finite bound' % t)
            want = ref['post'][t] if full else ref['alpha'][t]
            chk.within(got['posts'][k][t], want[0], want[1], w + ' posterior[%d]' % t)
            chk.within(got['means'][k][:, t], ref['means'][t][0], ref['means'][t][1], w + ' means[%d]' % t)


# ---- which watched instantiations a problem launches -------------------------------------------------------------------------------------------

def expected(fam, full=True):
    return sc.expected(FAMILIES[fam]['case'], 'three' if full else 'forward')


def forward_launches(fam, T, verdict):
    """launches of the forward instantiation of a K-steps-per-launch family: ceil(T / K) of the fused kernel, one of the persistent; a pass
    whose raw sum came near the bottom of the range is repeated with K = 1 (forward_bookkeeping, blhip_book.hpp) -- T more, resp. one more"""
    K = FAMILIES[fam]['rule'][1]
    if fam == 'fused1d':
        return -(-T // K) + (T if verdict == 'repeat' else 0)
    return 1 + (1 if verdict == 'repeat' else 0)


# ---- the Gaussian families: the scale rides on the recurrence's mantissa (blmath::inv_m) ---------------------------------------------------------
# The families, shapes, walks, engine options and recurrence counts are those of tests/test_likelihood_kernels.py (FAMILIES there), on the `wide` std
# grid only, so that every localEvidence bound is finite.  The schedule comes from the DATA: one value per step that sits still or jumps between
# the two ends of the mean grid under a walk of radius 7 cells.  The series are chosen by their longdouble normalisers (classified on the CPU).

GAUSSIAN = {'resident_exact': ('sum_lag', 2), 'resident_padded': ('sum_lag', 2), 'chain_exact': ('norm_lag', 4), 'chain_padded': ('norm_lag', 4),
            'chain_fold2': ('norm_lag', 4), 'chainax': ('norm_lag', 4),
            'chain_clamp': ('norm_lag', 4)}     # every step behind the first is clamped: it runs at the exact scale (scheme 2)
CLAMP_SHAPE, CLAMP_RADIUS, CLAMP_PMIN = (128, 32), 7, -7.0


def clamp_family():
    """the 128 x 32 geometry of tests/test_chain_clamp_bounds.py: a walk of radius 7 on the first parameter, then RegimeSwitch at -7"""
    import chain_clamp_cases as cc
    return dict(shape=CLAMP_SHAPE, opts={}, chains=[[(0, CLAMP_RADIUS)]], clamp=CLAMP_PMIN, rec=(4, 4 * cc.ntw_of(CLAMP_SHAPE[0]) - 1, (1,)),
                kinds=('full', 'evidence'))
SERIES = {
    'calm': (T_LONG, lambda t: 0.5 * math.sin(1.3 * t)),
    'jumping': (T_LONG, lambda t: -7.5 if t % 2 == 0 else 7.5),
    'jumping_period6': (T_RESONANT, lambda t: 7.5 * math.cos(math.pi * t / 3.0)),
}
# the classes, by the smallest normaliser of any chain behind step 0 (step 0 divides the reciprocal prior: its normaliser is the cell count):
# `calm` none below CALM; `jumping` one below JUMP; `jumping_period6` between the two, from a drive of period 6
CALM, JUMP = 0.02, 1e-3


def series(name):
    T, f = SERIES[name]
    return np.array([[f(t)] for t in range(T)], dtype=np.float64)


_GREF = {}


def gaussian_setup(fam, name, full):
    """test_likelihood_kernels.setup for a long series: -> (problem, op values, per chain the longdouble reference under the family's scale rule,
    likelihoods, whether the recurrence is accepted)"""
    import likelihood_cases as lc
    import test_likelihood_kernels as tl
    from oracle import bl_oracle as bo
    from bayesloop_amd.engine import FitProblem
    key = (fam, name, full)
    if key in _GREF:
        return _GREF[key]
    if len(_GREF) > 12:
        _GREF.clear()
    F = clamp_family() if fam == 'chain_clamp' else tl.FAMILIES[fam]
    n0, n1 = F['shape']
    mean, std = lc.mean_grid(n0), lc.std_grid('wide', n1)
    recs = series(name)
    T = len(recs)
    g = bo.Grid([mean, std])
    rec_ok = lc.recurrence_accepted(mean, std, recs)
    liks = []
    for r in recs:
        L = hp.gaussian_likelihood(mean, std, r)
        e, z = hp.likelihood_bound_rec(mean, std, r, *F['rec'], split=True)
        if 'rec_also' in F:
            e1, z1 = hp.likelihood_bound_rec(mean, std, r, *F['rec_also'], split=True)
            e, z = np.maximum(e, e1), np.maximum(z, z1)
        if F.get('both'):
            e2, z2 = hp.likelihood_bound_exp(mean, std, r, split=True, extra=hp.C_EXPMN)
            e, z = np.maximum(e, e2), np.maximum(z, z2)
        liks.append((L, e + z, e))
    prior = np.minimum(lc.reciprocal_prior(liks[0][0]), 1e150)
    refs, values = [], []
    for walks in F['chains']:
        taps = [(ax, bo.gaussian_kernel1d(tl._sigma(rad, g.lattice[ax]) / g.lattice[ax])[1]) for ax, rad in walks]
        refs.append(hp.gaussian_fit(prior, [(L, e) for L, e, _ in liks], taps, [mean, std], g.lattice, nblk=n0 * n1 // 64 + 1, full=full, clamp=F.get('clamp'), scale=GAUSSIAN[fam]))
        values.append([tl._sigma(rad, g.lattice[ax]) for ax, rad in walks] + ([F['clamp']] if 'clamp' in F else []))
    ops = [(_abi.OP_GRW, ax, -1, 0) for ax, _ in F['chains'][0]] + ([(_abi.OP_REGIMESWITCH, 0, -1, 0)] if 'clamp' in F else [])
    problem = FitProblem(obs_model=_abi.OM_GAUSSIAN, marginal=[mean, std], lattice=list(g.lattice), data=recs.reshape(T, 1, -1),
                         timestamps=np.arange(T, dtype=np.float64), prior=prior, ops=ops)
    _GREF[key] = (problem, np.asarray(values, dtype=np.float64), refs, liks, rec_ok)
    return _GREF[key]


def gaussian_combinations():
    return [(fam, name) for fam in GAUSSIAN for name in SERIES]
