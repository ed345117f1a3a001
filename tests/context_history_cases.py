"""
The table of engine calls of tests/test_context_history.py (GPU: a call's results on a context that has served other calls are, bit for bit,
those of the same call on a context created a moment ago) and of tests/test_context_history_host.py (CPU: the table's own consistency, and
the harness run through the float64 oracle and through an engine that leaks on purpose).

A TARGET is a name and a function run(engine, variant): it makes one engine call, or the few that belong together.  The engine it is given is
a Tap around the real one: everything an engine call hands back -- the arrays of every FitResult, every posterior, reduction, predictive, query,
accumulator, carried state and history row read -- is recorded in call order, so a target only has to MAKE the calls.  `variant` (0, 1, ...)
selects other data on the same geometry.  The targets reuse the drivers and the shapes of the files that hold each kernel family to its
reference (tests/step_transition_cases.py, test_likelihood_kernels.py, observation_cases.py, likprogram_cases.py, bigshift_cases.py,
test_postfit_kernels.py, test_online_block.py, predictive_cases.py, test_parser_series.py); no reference is computed here.

USES declares, per target, the reusable device buffers of blhip_ctx (bayesloop_amd/csrc/blhip_host.hpp) its calls allocate or read.
What is covered and what the card showed: tests/CONTEXT_HISTORY.md.
"""
import collections
import contextlib
import dataclasses
import os
import re

import numpy as np

from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- comparison ---------------------------------------------------------------------------------------------------------------------------------

def bits(a):
    """the array as unsigned integers of its items' width: NaN payloads and the sign of zero count"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == 'f':
        return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def same_bits(got, want):
    """-> list of differences (empty: identical keys, shapes, dtypes and bits).  No tolerance."""
    bad = []
    if list(got) != list(want):
        return ['the calls differ: got %s, want %s' % (list(got), list(want))]
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append('%s: shape / dtype %s %s, want %s %s' % (k, g.shape, g.dtype, w.shape, w.dtype))
            continue
        diff = bits(g) != bits(w)
        if diff.any():
            i = np.unravel_index(int(np.argmax(diff)), diff.shape) if diff.ndim else ()
            bad.append('%s: %d of %d values differ, first at %s: got %r, want %r' % (k, int(diff.sum()), diff.size, tuple(int(x) for x in i), g[i], w[i]))
    return bad


ROUTE_FIELDS = ('fwd_kernel_variant', 'resident_fallbacks', 'resident_fallback_reason', 'resident_armed')
BY_THE_CLOCK = ('blr::residency_probe_kernel',)          # runs on a context's first fit and then at most once per second


def census():
    from conftest import kernel_census
    try:
        return {name: c for c, name in kernel_census()}
    except Exception:        # noqa: BLE001 -- no library (the CPU harness runs on engines that launch nothing)
        return {}


def census_delta(before, after):
    return {k: after[k] - before.get(k, 0) for k in after if after[k] > before.get(k, 0) and not k.startswith(BY_THE_CLOCK)}


# ---- the recording engine --------------------------------------------------------------------------------------------------------------------------

RECORDED = ('posterior', 'marginal', 'time_average', 'predictive', 'posterior_query', 'accum_read', 'accum_finalize', 'carry_read', 'mix_read', 'mix_means')


class Tap:
    """the engine with every result it hands back recorded: self.out[<call number>.<method>[.<field>]] = a copy of the array;
    self.route: per fit the ROUTE_FIELDS of its timing"""

    def __init__(self, engine):
        self.__dict__.update(_e=engine, out=collections.OrderedDict(), route=[], _n=[0])

    def _key(self, name):
        self._n[0] += 1
        return '%02d.%s' % (self._n[0], name)

    def fit(self, *a, **kw):
        res = self._e.fit(*a, **kw)
        k = self._key('fit')
        for f in ('log_evidence', 'local_evidence', 'posterior_mean', 'abort_step', 'abort_phase'):
            v = getattr(res, f)
            if v is not None:
                self.out['%s.%s' % (k, f)] = np.array(v)
        self.route.append(tuple((res.timing or {}).get(f) for f in ROUTE_FIELDS))
        return res

    def __getattr__(self, name):
        attr = getattr(self._e, name)
        if name not in RECORDED:
            return attr

        def call(*a, **kw):
            r = attr(*a, **kw)
            self.out[self._key(name)] = np.array(r)
            return r
        return call

    def __setattr__(self, name, value):
        setattr(self._e, name, value)


OPTION_DEFAULTS = dict(chain_resident=1, resident=1, mfma=1, fast=1, chain1d=1, persist1d=1, fuse1d=8, chain_nd=1, chain1d_long=1, chain_clamp=1,
                       fuse_accumulate=1, fold2=1, chain_depad=1, max_batch=1024, fold_force_fail_batch=-1, chain_force_fail_batch=-1,
                       chain_force_fail_stage=0, resident_force_abort=0)


@contextlib.contextmanager
def options(engine, opts):
    """the engine options of a case, set and restored as test_step_transitions.Options does (an engine without options -- the float64 oracle --
    has no kernel families to choose between)"""
    on = hasattr(engine, 'set_option')
    try:
        for k, v in opts.items():
            if on:
                engine.set_option(k, v)
        yield
    finally:
        for k in opts:
            if on:
                engine.set_option(k, OPTION_DEFAULTS[k])


def arm(engine):
    """tests/conftest.py re-arms the process-wide engine only: the resident paths of this file's own contexts"""
    if hasattr(engine, 'set_option'):
        engine.set_option('resident_ok', 1)


def run_target(engine, name, variant=0):
    """-> (results {key: ndarray}, route dict(census = {instantiation: launches}, fits = [ROUTE_FIELDS per fit]))"""
    t = TARGETS[name]
    arm(engine)
    tap = Tap(engine)
    before = census()
    with np.errstate(all='ignore'):
        t.run(tap, variant % t.variants)
    return tap.out, dict(census=census_delta(before, census()), fits=tap.route)


def same_route(got, want):
    bad = []
    if got['fits'] != want['fits']:
        bad.append('%s per fit: got %s, want %s' % (ROUTE_FIELDS, got['fits'], want['fits']))
    if got['census'] != want['census']:
        keys = sorted(k for k in set(got['census']) | set(want['census']) if got['census'].get(k, 0) != want['census'].get(k, 0))
        bad.append('launches: ' + ', '.join('%s got %d want %d' % (k, got['census'].get(k, 0), want['census'].get(k, 0)) for k in keys))
    return bad


def compare(got, want, what):
    """the route first, with its own message; then the bits"""
    route = same_route(got[1], want[1])
    assert not route, '%s: ANOTHER ROUTE than on a fresh context -- %s' % (what, '; '.join(route))
    bad = same_bits(got[0], want[0])
    assert not bad, '%s: other bits than on a fresh context\n  %s' % (what, '\n  '.join(bad[:20]))


def after_every_predecessor(dirty, fresh, x, order=None, report=None):
    """test_after_every_predecessor's loop: on the engine `dirty`, for every target P in table order: P (thrown away), then X, held to
    fresh(X, variant).  P = X runs with another variant: the same geometry with other data."""
    history = []
    for p in (order or list(TARGETS)):
        pv = 1 if p == x else 0
        run_target(dirty, p, pv)
        history.append('%s[%d]' % (p, pv))
        got = run_target(dirty, x, 0)
        if report:
            report(x, history[-1], got[1])
        compare(got, fresh(x, 0), '%s after %s (before it: %s)' % (x, history[-1], ', '.join(history[-3:-1]) or 'nothing'))
        history.append('%s[0]' % x)


# ---- the targets ------------------------------------------------------------------------------------------------------------------------------------

Target = collections.namedtuple('Target', 'name family run variants')
TARGETS = collections.OrderedDict()
USES = {}

FIT = {'state', 'psumF', 'redF', 'meta', 'tables'}
FULL = FIT | {'psumB', 'redB'}
KEPT = {'post', 'postinv'}


def _target(name, family, run, uses, variants=2):
    assert name not in TARGETS
    TARGETS[name] = Target(name, family, run, variants)
    USES[name] = set(uses)


# -- table-likelihood fits: tests/step_transition_cases.py, every chain kept, the case's drivers `forward` and `three` -------------------------------
TABLE_CASES = [
    # (case, extra buffers)
    ('generic_walks_24x20', ()), ('generic_composed_row_300', ('stagebuf', 'stagemeta')), ('chain1d_sources_300', ()),
    ('fused1d_sources_300', ()), ('persist1d_sources_300', ('p1d', 'p1w')), ('fast_band8_sources_140x90', ()),
    ('mfma_band8_sources_140x90', ()), ('hwide_40x300', ('hsrc',)), ('hwide_sources_40x300', ('hsrc',)), ('vwide_140x64', ()),
    ('vwide_sources_140x64', ()), ('resident_32x32', ('resx',)), ('chain_sources_128x16', ('resx',)),
    ('chainax_sources_32x32', ('resx', 'xch', 'axlik', 'postpad')), ('chainax_100x90', ('resx', 'xch', 'axlik', 'postpad')),
    ('nd_shift_then_walk_5x18x14', ()), ('nd_cp_then_walk_3x7x5', ()), ('chain_nd_mixed_5x18x14', ()), ('chain1d_long_sources_4100', ()),
]
TABLE_DRIVERS = ('forward', 'three')


def table_run(case, drivers=TABLE_DRIVERS, chains=None):
    import step_transition_cases as sc
    c = sc.CASES[case]

    def run(engine, variant):
        kind = c['inputs'][variant]
        keep = list(range(len(c['chains']))) if chains is None else chains
        with options(engine, c['opts']):
            for driver in c['drivers']:
                if driver in drivers:
                    sc.run_problem(engine, case, kind, driver, keep)
    return run


def _table_targets():
    import step_transition_cases as sc
    for case, extra in TABLE_CASES:
        c = sc.CASES[case]
        _target('table_' + case, c['family'], table_run(case), FULL | KEPT | {'likbuf'} | set(extra), variants=len(c['inputs']))


# -- Gaussian-recurrence fits: the families, options and kinds of tests/test_likelihood_kernels.py on two of its records -------------------------------
GAUSS_FAMILIES = ('resident_exact', 'resident_padded', 'chain_exact', 'chain_padded', 'chain_fold2', 'chainax', 'chain_clamp', 'fast_rec', 'mfma_rec',
                  'mfma_lean_rec')
GAUSS_RECORDS = ('inside_1', 'inside_wide_1')          # the variants: narrow and wide std columns, other data positions
GAUSS_USES = {'resident_exact': {'resx'}, 'resident_padded': {'resx'}, 'chain_exact': {'resx', 'anchbuf'},
              'chain_padded': {'resx', 'anchbuf', 'postpad'}, 'chain_fold2': {'resx', 'anchbuf', 'accum_own', 'accpart', 'accw'},
              'chainax': {'resx', 'xch', 'axlik', 'postpad'}, 'chain_clamp': {'resx', 'anchbuf'}, 'fast_rec': set(), 'mfma_rec': set(),
              'mfma_lean_rec': set()}
_GAUSS = {}


def gauss_family(fam):
    import test_likelihood_kernels as tl
    if fam == 'chain_clamp':
        import long_series_cases as ls
        return dict(ls.clamp_family(), engine_opts=dict(chain_clamp=2))
    return dict(tl.FAMILIES[fam], engine_opts=tl.FAMILIES[fam]['opts'])


def gauss_problem(fam, case, T=3, shape=None, chains=None):
    """test_likelihood_kernels.setup without its longdouble reference: the family's grid, walks and clamp, the case's first T records (cycled
    beyond three), the prior the reciprocal of step 0's float64 likelihood capped at 1e150"""
    import likelihood_cases as lc
    import test_likelihood_kernels as tl
    from oracle import bl_oracle as bo
    key = (fam, case, T, shape, chains)
    if key not in _GAUSS:
        F = gauss_family(fam)
        n0, n1 = shape or F['shape']
        mean, std = lc.mean_grid(n0), lc.std_of(case, n1, n0)
        recs = lc.records(case, n0)[[t % 3 for t in range(T)]]
        g = bo.Grid([mean, std])
        L = np.ones((n0, n1))
        for x in recs[0]:
            if x == x:
                L = L * np.exp(-(x - mean[:, None]) ** 2 / (2.0 * std[None, :] ** 2)) / np.sqrt(2.0 * np.pi * std[None, :] ** 2)
        prior = np.minimum(lc.reciprocal_prior(L), 1e150)
        # (chains beyond the family's own repeat its walks a hundredth narrower per round: the same radii, other weights)
        walks = (F['chains'] * (chains or 1))[:chains or len(F['chains'])]
        values = [[tl._sigma(rad, g.lattice[ax]) * (1.0 - 0.01 * (b // len(F['chains']))) for ax, rad in w] +
                  ([F['clamp']] if 'clamp' in F else []) for b, w in enumerate(walks)]
        ops = [(_abi.OP_GRW, ax, -1, 0) for ax, _ in F['chains'][0]] + ([(_abi.OP_REGIMESWITCH, 0, -1, 0)] if 'clamp' in F else [])
        if not ops:
            ops, values = [(_abi.OP_STATIC, 0, -1, 0)], [[np.nan]] * len(walks)
        problem = FitProblem(obs_model=_abi.OM_GAUSSIAN, marginal=[mean, std], lattice=list(g.lattice), data=recs.reshape(T, 1, -1),
                             timestamps=np.arange(T, dtype=np.float64), prior=prior, ops=ops)
        _GAUSS[key] = (problem, np.asarray(values, dtype=np.float64), F)
    return _GAUSS[key]


def gauss_call(engine, problem, values, kind):
    """one fit of test_likelihood_kernels.run_kind's kinds, with the reads that belong to it"""
    T, shape, G = problem.T, problem.grid_size, problem.G
    if kind == 'fold':
        engine.accum_begin(T, G)
        try:
            res = engine.fit(problem, values, accumulate=True, log_chain_weight=np.zeros(len(values)))
            if np.all(res.abort_step < 0):
                engine.accum_read(T, [G])
        finally:
            engine.accum_end()
        return
    if kind == 'evidence':
        engine.fit(problem, values, evidence_only=True)
        return
    res = engine.fit(problem, values, forward_only=kind == 'forward', keep_posterior=True)
    if np.all(res.abort_step < 0):
        for b in range(len(values)):
            engine.posterior(b, T, shape)


def gauss_run(fam, T=3, shape=None, chains=None):
    def run(engine, variant):
        problem, values, F = gauss_problem(fam, GAUSS_RECORDS[variant], T, shape, chains)
        with options(engine, F['engine_opts']):
            for kind in F['kinds']:
                gauss_call(engine, problem, values, kind)
    return run


def _gauss_targets():
    for fam in GAUSS_FAMILIES:
        _target('gauss_' + fam, fam, gauss_run(fam), FULL | KEPT | GAUSS_USES[fam])


# -- problems compiled from a study description (tests/cases.py): the likelihood program, the device-built table, the large shift ---------------------
_COMPILED = {}


def compiled(key, build, engine):
    """-> (FitProblem, op values) of a plain Study, compiled once (the engine in place decides whether a density becomes a program)"""
    import bayesloop_amd as bl
    if key not in _COMPILED:
        prev = bl.set_engine(engine)
        try:
            S = build(bl)
            S._checkConsistency()
            S._formatData()
            problem, program = S._compile(silent=True)
            _COMPILED[key] = (problem, np.array(S._opValueMatrix(program), dtype=np.float64))
        finally:
            bl.set_engine(prev)
    return _COMPILED[key]


def kept_fit(engine, problem, values, **kw):
    res = engine.fit(problem, values, keep_posterior=True, **kw)
    if np.all(res.abort_step < 0):
        for b in range(len(values)):
            engine.posterior(b, problem.T, problem.grid_size)
    return res


def likprogram_run(engine, variant):
    """a bl.om.SymPy Normal density on a 40 x 12 grid (tests/likprogram_studies.py, the shape tests/predictive_cases.py uses): the program the
    fit arms replaces whatever program the context's previous problem armed"""
    import likprogram_studies as lps
    problem, values = compiled(('likprogram', variant), lambda bl: lps.normal_study(bl, sizes=(40, 12), T=12 - 2 * variant), engine)
    assert problem.lik_program is not None
    kept_fit(engine, problem, values)


def device_table_run(engine, variant):
    """Laplace on 60 x 44 (tests/cases.py: laplace_grw_2d): blk::lik_table_kernel builds the table from the data it uploads"""
    import cases
    c = dict(cases.CASES['laplace_grw_2d'], data=('series', 71 + variant, 12))
    problem, values = compiled(('laplace', variant), lambda bl: cases.build(bl, c), engine)
    kept_fit(engine, problem, values)


def bigshift_run(engine, variant):
    """a walk, then a drift of 16.6 cells per step on 200 x 180 (tests/bigshift_cases.py: bigshift_walk_then_shift): the stage buffers"""
    import bigshift_cases as bc
    import cases
    c = dict(bc.BIGSHIFT['bigshift_walk_then_shift'])
    c['data'] = ('series', c['data'][1] + 1000 * variant, c['data'][2])
    problem, values = compiled(('bigshift', variant), lambda bl: cases.build(bl, c), engine)
    kept_fit(engine, problem, values)


def poisson_run(engine, variant):
    """a row of 300 rates, walks of radius 5 and less, three count records (tests/observation_cases.py; tests/test_observation_kernels.py:
    poisson_setup): two chains on the default route, then five on the chain-resident 1-D kernel (chain1d = 2), whose chains share ONE
    likelihood table, built per batch (lik1d: four chains and more)"""
    import observation_cases as oc
    import test_likelihood_kernels as tl
    case = ('tutorial_1', 'sixty_1')[variant]
    rates, recs = oc.poisson_rates(case, 300), oc.poisson_records(case)
    lattice = rates[1] - rates[0]
    problem = FitProblem(obs_model=_abi.OM_POISSON, marginal=[rates], lattice=[lattice], data=recs.reshape(3, 1, -1), timestamps=np.arange(3.0),
                         prior=np.full(300, 1.0 / 300), ops=[(_abi.OP_GRW, 0, -1, 0)])
    kept_fit(engine, problem, np.array([[tl._sigma(5, lattice)], [tl._sigma(3, lattice)]]))
    with options(engine, dict(chain1d=2)):
        kept_fit(engine, problem, np.array([[tl._sigma(r, lattice)] for r in (5, 4, 3, 2, 1)]))


# -- a hyper-study's fold (tests/test_postfit_kernels.py: problem_2d, sigmas) ------------------------------------------------------------------------------
def hyper_fold_run(fuse, n0=128, n1=16, T=6, B=9):
    def run(engine, variant):
        import test_postfit_kernels as tp
        problem, ov = tp.problem_2d(n0, n1, T, seed=6 + variant), tp.sigmas(B)
        G = n0 * n1
        with options(engine, dict(fuse_accumulate=fuse)):
            engine.accum_begin(T, G)
            try:
                for lw in (-np.linspace(0.0, 6.0, B), -np.linspace(3.0, 0.5, B)):
                    engine.fit(problem, ov, accumulate=True, log_chain_weight=lw)
                engine.accum_finalize(problem)
                engine.accum_read(T, [n0, n1])
                for axis, n in ((0, n0), (1, n1)):
                    engine.marginal(1, 0, axis, T, n)
                engine.time_average(1, 0, [n0, n1])
            finally:
                engine.accum_end()
    return run


# -- carried fits and a block with history (tests/test_postfit_kernels.py: test_carried_states_of_a_fit; tests/test_online_block.py) -----------------
def carried_run(engine, variant, G=201, T=4, B=5):
    import test_postfit_kernels as tp
    slot = 3
    first = dataclasses.replace(tp.problem_1d(G, T, seed=5 + variant), carry_slot=slot)
    then = dataclasses.replace(tp.problem_1d(G, 1, seed=15 + variant), carry_slot=slot)
    ov = tp.sigmas(B)
    try:
        res = engine.fit(first, ov, forward_only=True, keep_posterior=True, carry=True)
        if np.all(res.abort_step < 0):
            engine.posterior(B - 1, T, [G])
        engine.fit(then, ov, evidence_only=True, resume=True, carry=True)
        engine.carry_mix(slot, np.array([0.5, 0.0, 0.25, 0.125, 0.125]))
        engine.carry_read(slot, -1, [G])
        engine.carry_mix(slot, np.linspace(0.1, 0.3, B), accumulate=True)
        engine.carry_read(slot, -1, [G])
        for b in range(B):
            engine.carry_read(slot, b, [G])
    finally:
        engine.carry_release(slot)


def history_block_run(engine, variant, shape=(64, 48), B=5, T=3):
    import test_online_block as tob
    rng = np.random.default_rng(5 + variant)
    tmd = rng.uniform(0.1, 1.0, (T, 2))
    for model in range(2):
        _, marginal = tob.kept_sequence(engine, list(shape), B, T, seed=model + 10 * variant)
        engine.mix_sequence(rng.uniform(0.0, 1.0, (T, B)), plane=1 + model, n_planes=3)
    engine.mix_sequence(tmd, plane=0, n_planes=3, source=1)
    engine.mix_read(T, list(shape))
    engine.mix_read(T, list(shape), plane=2)
    engine.mix_means(marginal, T)


# -- readers of a kept posterior -----------------------------------------------------------------------------------------------------------------------
READ_SHAPE, READ_T, READ_B = (40, 63), 4, 5


def _kept(engine, variant, shape=READ_SHAPE, T=READ_T, B=READ_B):
    import test_postfit_kernels as tp
    problem = tp.problem_2d(shape[0], shape[1], T, seed=6 + variant)
    engine.fit(problem, tp.sigmas(B), keep_posterior=True)
    return problem


def reductions_run(engine, variant):
    _kept(engine, variant)
    n0, n1 = READ_SHAPE
    for chain in (0, READ_B - 1):
        engine.posterior(chain, READ_T, [n0, n1])
        engine.marginal(0, chain, 0, READ_T, n0)
        engine.marginal(0, chain, 1, READ_T, n1)
        engine.time_average(0, chain, [n0, n1])


def predictive_run(engine, variant):
    """one Gaussian call (rows tabulated on the device) and one with the caller's rows, 18 values (tests/predictive_cases.py)"""
    import predictive_cases as pc
    problem = _kept(engine, variant)
    x = np.linspace(-5.0, 5.5, 18)
    G = int(np.prod(READ_SHAPE))
    engine.predictive(0, READ_B - 1, problem.marginal, _abi.OM_GAUSSIAN, x, 0, READ_T, False)
    engine.predictive(0, 0, problem.marginal, _abi.OM_GAUSSIAN, x, 0, READ_T, True)
    engine.predictive(0, 1, problem.marginal, _abi.OM_TABLE, x, 1, READ_T, False, host_rows=pc.likelihood_rows(x.size, G, 3 + variant))


def query_run(engine, variant):
    """a rows program with a series and a pairs program (tests/test_parser_series.py: exact_programs, pair_programs, b_space), 17 steps"""
    import test_parser_series as tps
    _kept(engine, variant)
    marg = tps.marginals(READ_SHAPE)
    steps = np.arange(17, dtype=np.int64) * 3 % READ_T
    ops, consts, series = tps.exact_programs(READ_SHAPE)['series']
    engine.posterior_query(0, READ_B - 1, steps, ops, consts, _abi.QR_GE, marg, series=series[:17])
    ops, consts, series = tps.pair_programs(READ_SHAPE)['series']
    b_values, b_prob = tps.b_space(5, 17, 3 + variant)
    engine.posterior_query(0, 0, steps, ops, consts, _abi.QR_GT, marg, series=series[:17], b_values=b_values, b_prob=b_prob)


def _build():
    _table_targets()
    _gauss_targets()
    _target('likprogram_normal_40x12', 'likprogram', likprogram_run, FULL | KEPT | {'likbuf', 'likprog_dev'})
    _target('device_table_laplace_60x44', 'device_table', device_table_run, FULL | KEPT | {'likbuf', 'databuf', 'resx', 'xch', 'axlik', 'postpad'})
    _target('poisson_row_300', 'poisson', poisson_run, FULL | KEPT | {'lik1d'})
    _target('bigshift_walk_then_shift_200x180', 'bigshift', bigshift_run, FULL | KEPT | {'stagebuf', 'stagemeta'})
    _target('hyper_fold_fused_128x16', 'hyper_fold', hyper_fold_run(1), FULL | {'post', 'accum_own', 'accpart', 'accw', 'stats', 'resx', 'anchbuf'})
    _target('hyper_fold_separate_128x16', 'hyper_fold', hyper_fold_run(0), FULL | {'post', 'accum_own', 'stats', 'resx', 'anchbuf'})
    _target('carried_row_201', 'carried', carried_run, FIT | KEPT | {'unit', 'mix', 'small'})
    _target('history_block_64x48', 'history', history_block_run, FIT | KEPT | {'likbuf', 'resx', 'xch', 'axlik', 'postpad', 'mixseq', 'mixw', 'stats'})
    _target('readers_reductions_40x63', 'readers', reductions_run, FULL | KEPT | {'resx', 'anchbuf', 'postpad', 'stats'})
    _target('readers_predictive_40x63', 'readers', predictive_run, FULL | KEPT | {'predws', 'predx'})
    _target('readers_query_40x63', 'readers', query_run, FULL | KEPT | {'queryws'})


_build()

NOT_IN_THE_TABLE = {'commbuf': 'multi-GPU exchange only (blhip_comm.hpp)', 'probebuf': 'the co-residency probe only, zeroed before every probe (blhip_fit_paths.hpp:74)'}


def devbuf_members():
    """the DevBuf members of struct blhip_ctx, parsed from bayesloop_amd/csrc/blhip_host.hpp"""
    text = open(os.path.join(ROOT, 'bayesloop_amd', 'csrc', 'blhip_host.hpp')).read()
    body = text[text.index('struct blhip_ctx {'):]
    body = body[:body.index('\n};')]
    names = []
    for m in re.finditer(r'^    DevBuf ([\w, ]+);', body, flags=re.M):
        names += [n.strip() for n in m.group(1).split(',')]
    return names


# ---- the same family, larger: more chains and more steps on the same grid, and a larger grid where the family admits one ----------------------------
def larger_runs(name):
    """-> [run(engine, variant)] to make before the target `name`: buffers grown beyond its extent, post_T / post_G / post_chains above its own"""
    t = TARGETS[name]
    if name.startswith('gauss_'):
        fam = name[len('gauss_'):]
        F = gauss_family(fam)
        runs = [gauss_run(fam, T=7, chains=2 * len(F['chains']) + 1)]
        if fam == 'resident_exact':
            runs.append(gauss_run('resident_padded', T=5))                  # 48 x 40 before 32 x 32
        return runs
    if name.startswith('table_'):
        import step_transition_cases as sc
        case = name[len('table_'):]
        fam = sc.CASES[case]['family']
        bigger = {'table_chain1d_sources_300': 'chain1d_walks_600', 'table_nd_cp_then_walk_3x7x5': 'nd_walks_5x18x14',
                  'table_chain_nd_mixed_5x18x14': 'chain_nd_walks_4x16x32', 'table_nd_shift_then_walk_5x18x14': 'chain_nd_walks_4x16x32',
                  'table_generic_walks_24x20': 'generic_walks_20x140', 'table_chainax_sources_32x32': 'chainax_100x90',
                  'table_resident_32x32': 'chainax_100x90', 'table_hwide_sources_40x300': 'hwide_40x300', 'table_vwide_sources_140x64': 'vwide_140x64'}
        # more chains on the same grid: the family's case with the most chains (itself, where it is the one); more steps: a Gaussian series is
        # not this family's kernel, so the steps grow through the kept block of T = 7 on the same number of cells
        same_grid = max((n for n, c in sc.CASES.items() if c['family'] == fam and c['shape'] == sc.CASES[case]['shape']),
                        key=lambda n: len(sc.CASES[n]['chains']))
        runs = [table_run(same_grid), long_table_run(sc.CASES[case]['shape'])]
        if name in bigger:
            runs.append(table_run(bigger[name]))
        return runs
    if t.family == 'hyper_fold':
        return [hyper_fold_run(1 if 'fused' in name else 0, T=9, B=19), hyper_fold_run(1 if 'fused' in name else 0, n0=256, n1=32, T=7, B=11)]
    if name == 'carried_row_201':
        return [lambda e, v: carried_run(e, v, G=300, T=7, B=5), poisson_run]
    if name == 'history_block_64x48':
        return [lambda e, v: history_block_run(e, v, shape=(64, 48), B=9, T=6), lambda e, v: history_block_run(e, v, shape=(80, 64), B=5, T=3)]
    if t.family == 'readers':
        def big(engine, variant):
            _kept(engine, variant, shape=(48, 80), T=7, B=8)
            for chain in (0, 7):
                engine.marginal(0, chain, 1, 7, 80)
                engine.time_average(0, chain, [48, 80])
        return [big, lambda e, v: _kept(e, v, T=9, B=9)]
    # compiled problems: the readers' larger kept batch grows post, postinv and the sums beyond them; then the target's other variant
    return [lambda e, v: _kept(e, v, shape=(256, 200), T=8, B=3), lambda e, v: t.run(e, 1)]


def long_table_run(shape, T=7, B=6):
    """a kept forward-only block of B walks over T steps with a table likelihood on the grid `shape` (tests/test_online_block.py: kept_sequence)"""
    def run(engine, variant):
        import test_online_block as tob
        tob.kept_sequence(engine, list(shape), B, T, seed=20 + variant)
    return run
