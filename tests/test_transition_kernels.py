"""
The large-shift kernel blk::bigshift_kernel<AXIS, BWD> and the stage flavours of blk::step_kernel (<100, 2, false> forward, <100, 3, false>
backward) on the MI355X, fed their own inputs and held to a rounding bound: every output cell against tests/highprec.py (longdouble
restatements of the reference's formulas, pinned on the CPU by tests/test_highprec.py) through worst(got, want, bound) <= 1.  No
tolerance here is a literal: every bound is an operation count of tests/highprec.py.  What is covered, what the card showed and which
in-bounds changes of the kernels these tests catch: tests/TRANSITION_KERNELS.md.

One-step problems at engine level, as transitionModels._device_transition drives them:
  forward   carry_write(slot, one state per chain), ONE resumed forward step with a flat OM_TABLE likelihood, carry_read per chain;
            local_evidence / dV is the sum before the step's normalisation.
  backward  a two-step problem with a uniform prior and a flat likelihood, posteriors kept: the caller's distribution enters as
            FitProblem.backward_init (the stage path takes it: such fits run the launch-per-step kernels), the forward shift is 0, and
            step 0's posterior is the normalised backward transition of that distribution (times the uniform alpha_0, normalised again).
Grids, shifts and inputs: tests/transition_cases.py.  Every test takes census deltas and asserts which large-shift / stage instantiations
ran and that the others did not.  BLHIP_TRANSITION_REPORT=<file> appends, per test, the instantiations that ran and the worst
error / bound.
"""
import os

import numpy as np
import pytest

import bayesloop_amd as bl
import highprec as hp
import transition_cases as tc
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitProblem
from conftest import kernel_census
from oracle import bl_oracle as bo

gpu = pytest.mark.gpu
needs_extended = pytest.mark.skipif(not hp.EXTENDED, reason=hp.REQUIRES_EXTENDED)

BIG = {(ax, bwd): 'blk::bigshift_kernel<%d, %s>' % (ax, 'true' if bwd else 'false') for ax in (0, 1) for bwd in (False, True)}
STAGE_FWD, STAGE_BWD = 'blk::step_kernel<100, 2, false>', 'blk::step_kernel<100, 3, false>'
WATCHED = set(BIG.values()) | {STAGE_FWD, STAGE_BWD}
SLOT = 0x7fff0003                         # a carried-state slot of the context that nothing else uses
WORST = {}                                # kernel flavour -> worst error / bound seen in this session
WROTE_SLOT = []


@pytest.fixture(scope='module')
def hip_engine():
    prev = bl.set_engine(None)
    eng = bl.get_engine()
    assert type(eng).__name__ == 'HipEngine'
    yield eng
    if WROTE_SLOT:                        # (only a forward problem creates the slot)
        eng.carry_release(SLOT)
    bl.set_engine(prev)
    for k in sorted(WORST):
        print('worst error / bound, %s: %.3f' % (k, WORST[k]))
    _report('worst', ', '.join('%s %.3f' % (k, WORST[k]) for k in sorted(WORST)))


def _report(what, text):
    path = os.environ.get('BLHIP_TRANSITION_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write('%s\t%s\t%s\n' % (os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0], what, text))


def _counts():
    return {name: c for c, name in kernel_census()}


class Census:
    """with Census(expect) as c: ...  -- asserts on exit that exactly the `expect`ed ones of the watched instantiations ran"""

    def __init__(self, expect):
        self.expect = set(expect)

    def __enter__(self):
        self.before = _counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        after = _counts()
        self.ran = {k for k in after if after[k] > self.before.get(k, 0)}
        _report('ran', ', '.join(sorted(self.ran)))
        watched = self.ran & WATCHED
        assert watched == self.expect, 'expected %s, ran %s (all launches: %s)' % (sorted(self.expect), sorted(watched), sorted(self.ran))
        return False


# ---- programs: a list of stages ('shift', axis) / ('walk', axis) / ('rs',) / ('ne',), and per chain one value per stage ---------------

def _ops_and_values(program, chains, T, backward):
    ops, cols = [], []
    for st in program:
        if st[0] == 'shift':
            cols.append(len(ops) + 1 + (T if backward else 0))          # the backward shift into step 0 / the forward shift into step 0
            ops += [(_abi.OP_DETERMINISTIC, st[1], -1, 0)] + [(_abi.OP_DETERMINISTIC_ARG, 0, -1, 0)] * (2 * T)
        else:
            cols.append(len(ops))
            ops.append(({'walk': _abi.OP_GRW, 'rs': _abi.OP_REGIMESWITCH, 'ne': _abi.OP_NOTEQUAL}[st[0]], st[1] if len(st) > 1 else 0, -1, 0))
    values = np.full((len(chains), len(ops)), np.nan)
    for k, op in enumerate(ops):
        if op[0] == _abi.OP_DETERMINISTIC_ARG:
            values[:, k] = 0.0
    for b, vals in enumerate(chains):
        for col, v in zip(cols, vals):
            values[b, col] = v
    return ops, values


def _grid(shape):
    return [np.arange(n, dtype=np.float64) for n in shape], [1.0, 1.0]


def run_forward(eng, shape, program, chains, states):
    """-> (outputs (B, n0, n1), sums before the step's normalisation (B,))"""
    B, G = len(chains), int(np.prod(shape))
    ops, values = _ops_and_values(program, chains, 1, False)
    marginal, lattice = _grid(shape)
    eng.carry_write(SLOT, np.asarray(states).reshape((B,) + tuple(shape)))
    WROTE_SLOT.append(True)
    problem = FitProblem(obs_model=_abi.OM_TABLE, marginal=marginal, lattice=lattice, data=np.zeros((1, 1)), timestamps=np.asarray([1.0]),
                         prior=np.asarray(states[0]), ops=ops, lik=np.ones((1, G)), seg_len=1, resume_time=0.0, carry_slot=SLOT)
    res = eng.fit(problem, values, evidence_only=True, resume=True, carry=True)
    assert np.all(res.abort_step < 0), res.abort_step
    out = np.stack([eng.carry_read(SLOT, b, list(shape)) for b in range(B)])
    return out, res.local_evidence[:, 0] / 1.0


def run_backward(eng, shape, program, chains, state):
    """-> step 0's posterior per chain (B, n0, n1)"""
    B, G = len(chains), int(np.prod(shape))
    ops, values = _ops_and_values(program, chains, 2, True)
    marginal, lattice = _grid(shape)
    problem = FitProblem(obs_model=_abi.OM_TABLE, marginal=marginal, lattice=lattice, data=np.zeros((2, 1)), timestamps=np.asarray([0.0, 1.0]),
                         prior=np.full(shape, 1.0 / G), ops=ops, lik=np.ones((2, G)), seg_len=1, backward_init=np.asarray(state))
    res = eng.fit(problem, values, keep_posterior=True)
    assert np.all(res.abort_step < 0), res.abort_step
    return np.stack([eng.posterior(b, 2, list(shape))[0] for b in range(B)])


def reference(shape, program, vals, x, backward=False):
    """the stage list in longdouble with its composed bound -> (result, bound of it, sum before the last normalisation, bound of that sum),
    bounds without SLACK; and whether every Deterministic stage divided by a well-conditioned sum"""
    nblk, G = tc.nblk_of(shape), int(np.prod(shape))
    v, e, ok = x, None, True
    for st, val in zip(program, vals):
        if st[0] == 'shift':
            if val == 0.0:
                continue                                               # no shift: the identity (its renormalisation is a no-op)
            v, e, D, eD = hp.deterministic_stage(v, e, val, st[1], nblk)
            ok = ok and tc.well_conditioned(D, eD, hp.SLACK)
        elif st[0] == 'walk':
            v, e = hp.walk_stage(v, e, bo.gaussian_kernel1d(val)[1], st[1])    # (lattice constant 1: sigma in cells; the oracle's taps as data)
        elif st[0] == 'rs':
            v, e = hp.regime_switch_stage(v, e, 10.0 ** val, nblk)
        elif st[0] == 'ne':
            v, e = hp.not_equal_stage(v, e, 10.0 ** val, nblk)
    if backward:                                                       # beta /= sum(beta); posterior_0 = alpha_0 beta_0, alpha_0 = 1 / G
        v, e = hp.normalise_stage(v, e, nblk)[:2]
        v, e = hp.scale_stage(v, e, 1.0 / G)
    r, er, S, eS = hp.normalise_stage(v, e, nblk)
    return r, er, S, eS, ok


def check_chains(flavour, shape, program, chains, states, got, sums=None, backward=False):
    """every chain against its reference; collects all misses before failing"""
    bad, top, ran = [], 0.0, 0
    for b, vals in enumerate(chains):
        r, er, S, eS, ok = reference(shape, program, vals, states[b], backward)
        assert ok, (shape, program, vals)
        q = hp.worst(got[b], r, hp.SLACK * er)
        ran += 1
        top = max(top, q)
        if not q <= 1.0:
            i, g, w, bd = hp.worst_at(got[b], r, hp.SLACK * er)
            bad.append('chain %d %r: error / bound %.3g at cell %s of %s (got %r, want %r, bound %.3g)' %
                       (b, vals, q, np.unravel_index(i, shape), shape, g, float(w), float(bd)))
        if sums is not None:
            qs = hp.worst([sums[b]], [S], [hp.SLACK * eS])
            top = max(top, qs)
            if not qs <= 1.0:
                bad.append('chain %d %r: sum %r, want %r, error / bound %.3g' % (b, vals, sums[b], float(S), qs))
    WORST[flavour] = max(WORST.get(flavour, 0.0), top)
    _report('worst ' + flavour, '%.4f over %d chains' % (top, ran))
    print('%s %s: worst error / bound %.3f over %d chains' % (flavour, shape, top, ran))
    assert not bad, '\n'.join(bad)


def usable_shifts(shape, ax, x, ds):
    """the shifts whose renormalising sum is well conditioned (transition_cases.well_conditioned; from the longdouble restatement alone)"""
    keep = []
    for d in ds:
        o, eo = hp.shift_stage(x, None, d, ax)
        _, _, D, eD = hp.normalise_stage(o, eo, tc.nblk_of(shape))
        if tc.well_conditioned(D, eD, hp.SLACK):
            keep.append(d)
    return keep


def _flavour(ax, bwd):
    return 'bigshift_kernel<%d, %s>' % (ax, 'true' if bwd else 'false')


GEOM = [(shape, ax) for shape, axes in tc.GEOMETRIES for ax in axes]
GEOM_IDS = ['%dx%d-axis%d' % (s[0], s[1], ax) for s, ax in GEOM]


def test_geometries_cover_the_launch_classes():
    """the grids reach every branch of launch_bigshift_t / bigshift_pitch the kernel's indexing depends on (restated in transition_cases)"""
    seen = tc.coverage()
    for ax in (0, 1):
        assert {'odd L>8', 'L<Lp, short last block', 'L=1 from LDS', 'nbb<nblk', 'nbb==nblk'} <= seen[ax], (ax, seen[ax])
    # Lp >= 32 changes the pitch on axis 0 only; on axis 1 a block never holds more than 16 rows (one partial slot per 16 x 128 tile)
    assert 'Lp>=32' in seen[0]
    g = tc.geometry((16, 128), 0)
    assert (g['L'], g['nbb'], g['Lp'], g['pitch'] % 32) == (128, 1, 128, 1)
    g = tc.geometry((40, 128), 0)
    assert (g['L'], g['nbb'], g['last']) == (43, 3, 42)
    for shape, ax in (((16384, 2), 0), ((2, 16384), 1)):
        g = tc.geometry(shape, ax)
        assert (g['n'], g['L'], g['nbb']) == (16384, 1, 2) and g['nbb'] < g['nblk']
    assert tc.spline_chunks() == {1, 3}


@gpu
@needs_extended
@pytest.mark.parametrize('kind', tc.INPUTS)
@pytest.mark.parametrize('shape,ax', GEOM, ids=GEOM_IDS)
def test_large_shift_forward(hip_engine, shape, ax, kind):
    x = tc.state(kind, shape, ax)
    ds = usable_shifts(shape, ax, x, tc.shifts(shape[ax]))
    assert len(ds) >= len(tc.shifts(shape[ax])) - 2
    program, chains = [('shift', ax)], [(d,) for d in ds]
    with Census({BIG[(ax, False)]}):
        got, sums = run_forward(hip_engine, shape, program, chains, [x] * len(chains))
    check_chains(_flavour(ax, False), shape, program, chains, [x] * len(chains), got, sums)


BWD = [(s, ax, k) for s, ax in GEOM for k in tc.INPUTS]


@gpu
@needs_extended
@pytest.mark.parametrize('shape,ax,kind', BWD, ids=['%dx%d-axis%d-%s' % (s[0], s[1], ax, k) for s, ax, k in BWD])
def test_large_shift_backward(hip_engine, shape, ax, kind):
    """BWD = true, every geometry, input and shift.  (Which slot the input scale is read from does not show here or anywhere: the kernel
    writes D = sum of its scaled output and every consumer divides by it -- tests/TRANSITION_KERNELS.md, "Can the tests fail".)"""
    x = tc.state(kind, shape, ax, seed=1)
    ds = usable_shifts(shape, ax, x, tc.shifts(shape[ax]))
    assert len(ds) >= len(tc.shifts(shape[ax])) - 2
    program, chains = [('shift', ax)], [(d,) for d in ds]
    with Census({BIG[(ax, True)]}):
        got = run_backward(hip_engine, shape, program, chains, x)
    check_chains(_flavour(ax, True), shape, program, chains, [x] * len(chains), got, backward=True)


@gpu
@needs_extended
@pytest.mark.parametrize('backward', [False, True], ids=['forward', 'backward'])
@pytest.mark.parametrize('kind', tc.INPUTS)
@pytest.mark.parametrize('shape,ax', GEOM[:10], ids=GEOM_IDS[:10])
def test_shift_of_exactly_12_launches_no_large_shift_kernel(hip_engine, shape, ax, kind, backward):
    """the control: the small-shift stencil of the fused step kernel, at the same bound"""
    x = tc.state(kind, shape, ax, seed=2)
    program, chains = [('shift', ax)], [(d,) for d in tc.CONTROL_SHIFTS]
    with Census(set()):
        if backward:
            got, sums = run_backward(hip_engine, shape, program, chains, x), None
        else:
            got, sums = run_forward(hip_engine, shape, program, chains, [x] * 2)
    check_chains('step_kernel, shift of 12', shape, program, chains, [x] * 2, got, sums, backward=backward)


@gpu
@needs_extended
@pytest.mark.parametrize('backward', [False, True], ids=['forward', 'backward'])
@pytest.mark.parametrize('ax', [0, 1])
def test_every_line_length_from_13_to_140(hip_engine, ax, backward):
    """N = n + 24 through the prefilter's chunk sizes C = 1 (empty lanes) and 3, last chunks of one element and the change of C"""
    for n in tc.SWEEP_N:
        shape = tc.sweep_shape(n, ax)
        x = tc.state(('cube', 'single')[n % 2], shape, ax)
        ds = usable_shifts(shape, ax, x, tc.SWEEP_SHIFTS(n))
        assert len(ds) >= 3
        program, chains = [('shift', ax)], [(d,) for d in ds]
        with Census({BIG[(ax, backward)]}):
            if backward:
                got, sums = run_backward(hip_engine, shape, program, chains, x), None
            else:
                got, sums = run_forward(hip_engine, shape, program, chains, [x] * len(ds))
        check_chains(_flavour(ax, backward), shape, program, chains, [x] * len(ds), got, sums, backward=backward)


@gpu
@needs_extended
@pytest.mark.parametrize('ax', [0, 1])
def test_batch_of_chains_with_different_shifts(hip_engine, ax):
    """one call: no shift, shifts the stencil takes (|d| <= 12) and large ones side by side, every chain with its own state"""
    shape = (203, 77)
    ds = [0.0, 5.0, -12.0, 12.0, 16.6, -23.25, float(shape[ax]), 0.0, 3e9, -7.5, 40.0]
    # (the chains of the fused step kernel's stencil, |d| <= 12, get dense lines: it applies the prefilter's impulse response up to 34 cells,
    #  which at a fractional shift is the reference's result to rounding only where a line has mass nearby -- by design, see
    #  tests/TRANSITION_KERNELS.md, "Not held to this bound"; at an integer shift the cardinal spline vanishes at the other cells anyway)
    kinds = ['cube', 'cube', 'cube', 'zero_lines', 'cube', 'decades', 'edges', 'decades', 'single', 'zero_lines', 'decades']
    states = [tc.state(k, shape, ax, seed=10 + b) for b, k in enumerate(kinds)]
    program, chains = [('shift', ax)], [(d,) for d in ds]
    # (the chains without a large shift run the same stage index through the generic stage kernel, as an identity in front of their step)
    with Census({BIG[(ax, False)], STAGE_FWD}):
        got, sums = run_forward(hip_engine, shape, program, chains, states)
    check_chains('mixed batch, axis %d' % ax, shape, program, chains, states, got, sums)


TWO_AXES = [(20.0, 0.0), (0.0, 20.0), (20.0, 20.0), (5.0, 20.0)]


@gpu
@needs_extended
@pytest.mark.parametrize('shape', [(203, 77), (40, 128)], ids=['203x77', '40x128'])
def test_two_op_program_with_different_stage_counts_per_chain(hip_engine, shape):
    """Deterministic along axis 0, then along axis 1; chains shift (20, 0), (0, 20), (20, 20), (5, 20) cells: stage counts and shifted axes
    differ inside one launch.  (5, 20): the small shift is a stage of the generic kernel in front of the large one."""
    program = [('shift', 0), ('shift', 1)]
    states = [tc.state(k, shape, 0, seed=20 + b) for b, k in enumerate(('cube', 'decades', 'cube', 'zero_lines'))]
    with Census({BIG[(0, False)], BIG[(1, False)], STAGE_FWD}):
        got, sums = run_forward(hip_engine, shape, program, TWO_AXES, states)
    check_chains('two-op batch', shape, program, TWO_AXES, states, got, sums)
    with Census({BIG[(0, True)], BIG[(1, True)], STAGE_BWD}):
        gotb = run_backward(hip_engine, shape, program, TWO_AXES, states[0])
    check_chains('two-op batch, backward', shape, program, TWO_AXES, [states[0]] * 4, gotb, backward=True)


# name -> (program, one chain's values, whether a stage of the generic stage kernel runs).  build_program (blhip_program.hpp) makes the
# backward program with the same run() in the same list order, so the rule is one for both directions: a large shift always closes the
# stage in front of it and is a stage of its own; what FOLLOWS it is the last StepProg, which the fused step kernel takes; a small shift
# (<= 12 cells: the stencil) is closed into a stage by a RegimeSwitch / NotEqual behind it, whose clamp then reads 1 / slot 5 of that
# stage's partials.  With one chain a stage launch is issued only if that chain has such a stage (blhip.hip: n_other > 0).
COMPOSITIONS = {
    'walk_then_shift': ([('walk', 0), ('shift', 0)], (2.5, 16.6), True),
    'walk_other_axis_then_shift': ([('walk', 1), ('shift', 0)], (1.5, -23.25), True),
    'shift_then_walk': ([('shift', 1), ('walk', 1)], (16.6, 2.5), False),
    'shift_then_shift_other_axis': ([('shift', 0), ('shift', 1)], (16.6, -23.25), False),
    'shift_then_regime_switch': ([('shift', 0), ('rs',)], (-16.6, -4.0), False),
    'shift_then_not_equal': ([('shift', 1), ('ne',)], (23.25, -4.0), False),
    # the clamp modes of the stage kernel itself, closed by the large shift behind them
    'walk_regime_switch_then_shift': ([('walk', 0), ('rs',), ('shift', 0)], (2.5, -4.0, 16.6), True),
    'regime_switch_then_shift': ([('rs',), ('shift', 1)], (-4.0, -23.25), True),
    'not_equal_then_shift': ([('ne',), ('shift', 0)], (-4.0, 16.6), True),
    # a Deterministic stage INSIDE the stage kernel (5 cells) whose consumer clamps: the one place that needs the stage's slot 5
    'small_shift_then_regime_switch': ([('shift', 0), ('rs',)], (5.0, -4.0), True),
    'small_shift_then_not_equal': ([('shift', 1), ('ne',)], (-7.0, -4.0), True),
}


def _expected(program, vals, stage, backward):
    out = {BIG[(st[1], backward)] for st, v in zip(program, vals) if st[0] == 'shift' and abs(v) > 12.0}
    if stage:
        out.add(STAGE_BWD if backward else STAGE_FWD)
    return out


# backward where the handle allows: the two-step problem runs the program forward on the uniform alpha_0 first, and NotEqual of a uniform
# distribution is 0 / 0 in the reference (max - p = 0 everywhere) -- programs with a NotEqual run forward only
COMPOSED = [(name, kind, bwd) for name in sorted(COMPOSITIONS) for kind in ('cube', 'decades') for bwd in (False, True)
            if not (bwd and any(st[0] == 'ne' for st in COMPOSITIONS[name][0]))]


@gpu
@needs_extended
@pytest.mark.parametrize('name,kind,backward', COMPOSED, ids=['%s-%s-%s' % (n, k, 'backward' if b else 'forward') for n, k, b in COMPOSED])
def test_compositions_with_the_stage_kernel(hip_engine, name, kind, backward):
    """stage lists around a shift against the composed longdouble restatement; the exact set of large-shift and stage instantiations"""
    program, vals, stage = COMPOSITIONS[name]
    for shape in ((203, 77), (40, 128)):
        x = tc.state(kind, shape, 0, seed=30)
        with Census(_expected(program, vals, stage, backward)):
            if backward:
                got, sums = run_backward(hip_engine, shape, program, [vals], x), None
            else:
                got, sums = run_forward(hip_engine, shape, program, [vals], [x])
        check_chains('composition ' + name + (', backward' if backward else ''), shape, program, [vals], [x], got, sums, backward=backward)
