"""
Arithmetic on (hyper-)parameter distributions: ``Parser(S1, S2, ...)('log(rate2@1*2) + rate@2^2 > 20')``.

Own implementation of the query language of the reference's ``bayesloop.Parser`` (bayesloop/parser.py:50-440; surface:
``Parser(*studies)``, ``parser(query, t=None, silent=False)``, ``Study.eval`` core.py:604-621): a query is an arithmetic
expression over parameter names, hyper-parameter names, numbers and NumPy / scipy.special function names with the operators
``+ - * / ^`` and ``@`` (time stamp selection), optionally followed by ONE relation ``< > <= >= ==`` and a right-hand side.
With a relation the probability of the statement is returned, without it the binned distribution of the derived quantity.

Semantics kept from the reference (file:line refer to bayesloop/parser.py):

* precedence, tightest first: function application, ``@``, ``^`` (right-assoc.), unary sign, ``* /``, ``+ -`` (:121-127);
* a parameter lives on the FULL joint grid of its study (values = ravelled mesh grid, probabilities = ravelled posterior
  of one time step), so two parameters of the same study combine element by element, i.e. with their joint distribution;
  quantities of different studies, the same parameter at two time stamps, hyper-parameter x parameter and derived x derived
  combine as independent variables (outer product of values and probabilities, :229-243); everything else is element-wise
  and keeps the probabilities of the first operand that carries any (NumPy's subclass rule, :246-247);
* a parameter needs a time stamp (``@`` or ``t=``) before arithmetic (:213-223); hyper-parameters of an ``OnlineStudy`` with
  history as well;
* ``lhs REL rhs`` is evaluated as ``-1*(rhs)+lhs REL 0`` (:383-390); the distribution uses
  ``int((max-min)/max gap)`` equal bins labelled by their upper edge (:399-418).

Not kept: the reference prints debugging output while binning (:404-406) and needs ``pyparsing``; only the time steps a query
selects are copied from the GPU (``DevicePosterior.row``) instead of the whole posterior sequence.

Added: ``t='all'`` or a list / tuple / 1-D array of time stamps evaluates a query at every one of them in ONE call, and
``series={name: values}`` binds a name to a number per time stamp -- the loops of the reference's tutorials
(``[P('rho < 0.', t=t, silent=True) for t in range(1, 389)]``, ``P('(mu - ' + str(mu0[t]) + ')/sigma > 1', t=t, silent=True)``).
Entry i of the result is by definition ``P(query, t=t[i], silent=True)``.  A probability query whose plan has one or two index
spaces is summed on the GPU while the posterior sequence lives there (the plan: further down; the kernels:
bayesloop_amd/csrc/blhip_query.hpp); a distribution query over the parameters of one study is binned once on the host and summed per bin
on the GPU (the plan: at the end of this file; the kernels: bayesloop_amd/csrc/blhip_bins.hpp); every other query is the loop over the scalar call.
"""
from __future__ import annotations

import operator
import re

import numpy as np
import scipy.special as _sp

from .exceptions import ConfigurationError

_ARITH = {'+': operator.add, '-': operator.sub, '*': operator.mul, '/': operator.truediv, '^': operator.pow}
_RELATIONS = (('>=', operator.ge), ('<=', operator.le), ('==', operator.eq), ('>', operator.gt), ('<', operator.lt))
_NUMBER = re.compile(r'(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?')
_NAME = re.compile(r'[A-Za-z_][A-Za-z_0-9]*')


class _Quantity:
    """Values on a grid with their probabilities.  kind: 'param' | 'hyper' | 'derived'; ``rows`` (callable index -> 1-D
    probabilities) stands for the time-resolved probabilities until a time stamp is selected."""

    def __init__(self, values, prob=None, rows=None, name=None, time=None, study=None, kind='param', timestamps=None):
        self.values = np.asarray(values, dtype=float)
        self.prob, self.rows = prob, rows
        self.name, self.time, self.study, self.kind, self.timestamps = name, time, study, kind, timestamps

    def copy(self):
        return _Quantity(self.values.copy(), self.prob, self.rows, self.name, self.time, self.study, self.kind, self.timestamps)

    def with_values(self, values):
        q = self.copy()
        q.values = np.asarray(values, dtype=float)
        return q

    @property
    def needs_time(self):
        return self.rows is not None and self.prob is None

    def select(self, stamp):
        """``quantity @ stamp`` (:203-208)."""
        q = self.copy()
        try:
            index = list(self.timestamps).index(stamp)
        except ValueError:
            raise ValueError('{} is not in list'.format(stamp))
        q.prob, q.rows, q.time = np.asarray(self.rows(index), dtype=float), None, stamp
        return q


def _tokenize(text, names, functions, numbers=None):
    """numbers: names bound to a number for this call (the series of a vector-t query at one step); they shadow functions."""
    tokens, i = [], 0
    while i < len(text):
        ch = text[i]
        if ch.isspace():
            i += 1
            continue
        if ch in '+-*/^@()':
            tokens.append(('op', ch))
            i += 1
            continue
        m = _NUMBER.match(text, i)
        if m:
            tokens.append(('num', float(m.group(0))))
            i = m.end()
            continue
        m = _NAME.match(text, i)
        if m:
            word = m.group(0)
            if numbers and word in numbers:
                tokens.append(('num', numbers[word]))
            elif word in names:
                tokens.append(('name', word))
            elif word in functions:
                tokens.append(('func', word))
            else:
                raise ConfigurationError('Unknown name "{}" in query.'.format(word))
            i = m.end()
            continue
        raise ConfigurationError('Cannot parse "{}" in query.'.format(text[i:]))
    return tokens


class Parser:
    """Computes derived probability values and distributions from arithmetic on (hyper-)parameters of one or more studies."""

    def __init__(self, *studies):
        self.studies = studies
        if len(studies) == 0:
            raise ConfigurationError('Parser instance takes at least one Study instance as argument.')
        self.names = []
        for study in studies:
            self.names.extend(study.observationModel.parameterNames)
            if _is_online(study):
                for names in study.hyperParameterNames:
                    self.names.extend(names)
            elif hasattr(study, 'flatHyperParameterNames'):
                self.names.extend(study.flatHyperParameterNames)
        if len(set(self.names)) != len(self.names):
            raise ConfigurationError('Specified study objects contain duplicate parameter names.')
        self.functions = set(n for n in dir(np) if callable(getattr(np, n, None)))
        self.functions |= set(n for n in dir(_sp) if callable(getattr(_sp, n, None)))
        for name in self.names:
            if name in self.functions:
                self.functions.discard(name)
                print('! WARNING: Function "{}" will not be available in parser, as it collides with '
                      '(hyper-)parameter names.'.format(name))

    # ---- quantities of the studies ---------------------------------------------------------------------------------
    def _load(self, t):
        out = {}
        for study in self.studies:
            online = _is_online(study)
            history = getattr(study, 'storeHistory', True)
            stamps = list(study.formattedTimestamps)
            for index, name in enumerate(study.observationModel.parameterNames):
                values = np.ravel(study.grid[index])
                if t is not None:
                    ti = list(self.studies[0].formattedTimestamps).index(t)                 # (:291, first study's stamps)
                    out[name] = _Quantity(values, prob=np.ravel(_posterior_row(study, ti)), name=name, time=t, study=study)
                elif online and not history:
                    out[name] = _Quantity(values, prob=np.ravel(study.marginalizedPosterior), name=name, time=stamps[-1], study=study)
                else:
                    out[name] = _Quantity(values, rows=(lambda i, s=study: np.ravel(_posterior_row(s, i))), name=name, study=study,
                                          timestamps=stamps)
            if online:
                for j, names in enumerate(study.hyperParameterNames):
                    for name in names:
                        k = list(names).index(name)                 # column of this hyper-parameter in the model's value grid
                        values = np.asarray(study.hyperParameterValues[j])[:, k]
                        if t is None and history:
                            seq = study.hyperParameterSequence
                            rows = (lambda i, s=seq, jj=j: np.asarray(s[i][jj]) / np.sum(s[i][jj]))
                            out[name] = _Quantity(values, rows=rows, name=name, study=study, kind='hyper', timestamps=stamps)
                        elif t is None:
                            d = np.asarray(study.hyperParameterDistribution[j], dtype=float)
                            out[name] = _Quantity(values, prob=d / d.sum(), name=name, time=stamps[-1], study=study, kind='hyper')
                        elif history:
                            ti = list(self.studies[0].formattedTimestamps).index(t)
                            d = np.asarray(study.hyperParameterSequence[ti][j], dtype=float)
                            out[name] = _Quantity(values, prob=d / d.sum(), name=name, time=t, study=study, kind='hyper')
                        else:
                            raise ConfigurationError('OnlineStudy instance is not configured to store history, '
                                                     'cannot access t={}.'.format(t))
            elif hasattr(study, 'flatHyperParameterNames'):
                for name in study.flatHyperParameterNames:
                    k = study._getHyperParameterIndex(study.transitionModel, name)
                    d = np.asarray(study.hyperParameterDistribution, dtype=float)
                    grid = getattr(study, 'allHyperGridValues', None)
                    if grid is None or len(grid) == 0:
                        grid = study.hyperGridValues
                    out[name] = _Quantity(np.asarray(grid)[:, k], prob=d / d.sum(), name=name, study=study, kind='hyper')
        return out

    # ---- expression evaluation (precedence climbing) -----------------------------------------------------------------
    def _expression(self, tokens, pos, quantities):
        """sum := product (('+'|'-') product)*"""
        left, pos = self._product(tokens, pos, quantities)
        while pos < len(tokens) and tokens[pos] in (('op', '+'), ('op', '-')):
            sym = tokens[pos][1]
            right, pos = self._product(tokens, pos + 1, quantities)
            left = self._arith(sym, left, right)
        return left, pos

    def _product(self, tokens, pos, quantities):
        left, pos = self._signed(tokens, pos, quantities)
        while pos < len(tokens) and tokens[pos] in (('op', '*'), ('op', '/')):
            sym = tokens[pos][1]
            right, pos = self._signed(tokens, pos + 1, quantities)
            left = self._arith(sym, left, right)
        return left, pos

    def _signed(self, tokens, pos, quantities):
        if pos < len(tokens) and tokens[pos] in (('op', '+'), ('op', '-')):
            sign = -1.0 if tokens[pos][1] == '-' else 1.0
            operand, pos = self._signed(tokens, pos + 1, quantities)
            return self._arith('*', sign, operand), pos                       # "-x" is "(-1)*x" (:152-157)
        return self._power(tokens, pos, quantities)

    def _power(self, tokens, pos, quantities):
        base, pos = self._at(tokens, pos, quantities)
        if pos < len(tokens) and tokens[pos] == ('op', '^'):
            # right-associative; the exponent may carry its own sign ("2^-1")
            exponent, pos = self._signed_power(tokens, pos + 1, quantities)
            return self._arith('^', base, exponent), pos
        return base, pos

    def _signed_power(self, tokens, pos, quantities):
        if pos < len(tokens) and tokens[pos] in (('op', '+'), ('op', '-')):
            sign = -1.0 if tokens[pos][1] == '-' else 1.0
            operand, pos = self._signed_power(tokens, pos + 1, quantities)
            return self._arith('*', sign, operand), pos
        return self._power(tokens, pos, quantities)

    def _at(self, tokens, pos, quantities):
        left, pos = self._applied(tokens, pos, quantities)
        while pos < len(tokens) and tokens[pos] == ('op', '@'):
            stamp, pos = self._applied(tokens, pos + 1, quantities)
            if isinstance(left, _Quantity) and left.needs_time and not isinstance(stamp, _Quantity):
                left = left.select(stamp)
            else:
                raise ConfigurationError('"@" selects a time stamp of a (hyper-)parameter with a history.')
        return left, pos

    def _applied(self, tokens, pos, quantities):
        if pos >= len(tokens):
            raise ConfigurationError('Unexpected end of query.')
        kind, val = tokens[pos]
        if kind == 'func':
            fn = getattr(np, val) if hasattr(np, val) and callable(getattr(np, val)) else getattr(_sp, val)
            operand, pos = self._applied(tokens, pos + 1, quantities)
            return self._apply(fn, val, operand), pos
        if kind == 'num':
            return val, pos + 1
        if kind == 'name':
            return quantities[val].copy(), pos + 1
        if (kind, val) == ('op', '('):
            inner, pos = self._expression(tokens, pos + 1, quantities)
            if pos >= len(tokens) or tokens[pos] != ('op', ')'):
                raise ConfigurationError('Missing ")" in query.')
            return inner, pos + 1
        if (kind, val) in (('op', '+'), ('op', '-')):                        # a sign directly behind a function / "@"
            return self._signed(tokens, pos, quantities)
        raise ConfigurationError('Unexpected "{}" in query.'.format(val))

    def _apply(self, fn, name, operand):
        if isinstance(operand, _Quantity):
            with np.errstate(all='ignore'):
                return operand.with_values(fn(operand.values))
        return fn(operand)

    def _arith(self, sym, a, b):
        op = _ARITH[sym]
        qa, qb = isinstance(a, _Quantity), isinstance(b, _Quantity)
        for q in (a, b):
            if isinstance(q, _Quantity) and q.needs_time:
                if q.kind == 'hyper':
                    raise ConfigurationError('No timestamp defined for hyper-parameter "{}"'.format(q.name))
                raise ConfigurationError('No timestamp defined for parameter "{}"'.format(q.name))
        with np.errstate(all='ignore'):
            if not qa and not qb:
                return op(a, b)
            if qa and qb and self._independent(a, b):
                values = op(a.values[:, None], b.values[None, :]).ravel()      # (a_i, b_j), a slow (:239-240)
                prob = (np.asarray(a.prob)[:, None] * np.asarray(b.prob)[None, :]).ravel()
                return _Quantity(values, prob=prob / prob.sum(), name='_derived', kind='derived')
            if qa and qb:
                return a.with_values(op(a.values, b.values))                   # joint grid of one study: element by element
            if qa:
                return a.with_values(op(a.values, b))
            return b.with_values(op(a, b.values))

    @staticmethod
    def _independent(a, b):
        pa, pb = a.kind != 'hyper', b.kind != 'hyper'                          # derived quantities are "parameters" (:243)
        if pa and pb:
            return (a.study is not b.study) or (a.study is None and b.study is None) or (a.name == b.name and a.time != b.time)
        if not pa and not pb:
            return (a.study is not b.study) or (a.study is None and b.study is None)
        return True

    # ---- queries -----------------------------------------------------------------------------------------------------
    def __call__(self, query, t=None, silent=False, series=None):
        """t: a time stamp, None, 'all' (every time stamp of the first study) or a list / tuple / 1-D array of time stamps.  With a vector
        of time stamps a probability query returns the (len(t),) array whose entry i is ``self(query, t=t[i], silent=True)``, a
        distribution query the list of those results.  series: {name: array of len(t)} binds names to a number that changes with the time
        stamp (entry i at t[i]) -- the numeric token a loop over time stamps would format into the query."""
        if _is_vector(t):
            return self._call_many(query, t, silent, series)
        if series is not None:
            raise ConfigurationError('series binds a name to one number per time stamp: it needs t="all" or a sequence of time stamps.')
        return self._call_one(query, t, silent)

    def _call_one(self, query, t, silent, numbers=None):
        quantities = self._load(t)
        parts = re.split('>=|<=|==|>|<', query)
        if len(parts) > 2:
            raise ConfigurationError('Use exactly one operator out of (<, >, <=, >=, ==) to obtain probability value, '
                                     'or none to obtain derived distribution.')
        reduced = query if len(parts) == 1 else '-1*(' + parts[1] + ')+' + parts[0]
        tokens = _tokenize(reduced, set(self.names), self.functions, numbers)
        derived, pos = self._expression(tokens, 0, quantities)
        if pos != len(tokens):
            raise ConfigurationError('Cannot parse query behind "{}".'.format(tokens[pos][1]))
        if not isinstance(derived, _Quantity):
            raise ConfigurationError('Query contains no (hyper-)parameter.')
        if derived.needs_time:
            raise ConfigurationError('No timestamp defined for {}parameter "{}"'.format('hyper-' if derived.kind == 'hyper' else '',
                                                                                        derived.name))
        values, prob = derived.values, np.asarray(derived.prob, dtype=float)

        if len(parts) == 2:
            rel = next(fn for sym, fn in _RELATIONS if sym in query)
            with np.errstate(invalid='ignore'):
                p = float(np.sum(prob[rel(values, 0.)]))
            if not silent:
                print('P({}) = {}'.format(query, p))
            return p

        n_bins, bins, index, ok = _binning(values)
        if not silent:
            print('+ Computing distribution: {}'.format(query))
        binned = np.bincount(index[ok], weights=prob[ok], minlength=max(n_bins - 1, 0))[:max(n_bins - 1, 0)]
        return bins[:-1] + (bins[1] - bins[0]), binned

    # ---- a vector of time stamps ---------------------------------------------------------------------------------------
    def _stamps(self, t):
        if isinstance(t, str):
            return list(self.studies[0].formattedTimestamps)                  # 'all': the first study's stamps, the rule for t (:291)
        return np.asarray(t).ravel().tolist() if isinstance(t, np.ndarray) else list(t)

    def _series(self, series, n):
        out = {}
        for name, values in (series or {}).items():
            if name in self.names:
                raise ConfigurationError('Series name "{}" collides with a (hyper-)parameter name.'.format(name))
            if not _NAME.fullmatch(str(name)):
                raise ConfigurationError('Series name "{}" is no name the query language can use.'.format(name))
            v = np.asarray(values, dtype=float)
            if v.ndim != 1 or v.size != n:
                raise ConfigurationError('Series "{}" needs one value per time stamp ({}), got shape {}.'.format(name, n, v.shape))
            if not np.all(np.isfinite(v)):
                raise ConfigurationError('Series "{}" contains values that are not finite.'.format(name))
            if name in self.functions:
                print('! WARNING: Function "{}" will not be available in this query, as it collides with a series name.'.format(name))
            out[name] = v
        return out

    def _loop(self, query, stamps, series):
        """The scalar call at every time stamp: the definition of the vector call and the path of every query the device does not take."""
        return [self._call_one(query, ts, True, {k: float(v[i]) for k, v in series.items()} or None) for i, ts in enumerate(stamps)]

    def plan(self, query, t='all', series=None, pair_max=None):
        """The query plan of a probability query with a vector of time stamps (:class:`QueryPlan`); ``plan.reason`` says why a query
        stays on the host loop (None: the device takes it if the sequence of ``plan.study`` is resident there)."""
        stamps = self._stamps(t)
        return _plan(self, query, stamps, self._series(series, len(stamps)), pair_max)

    def planDistribution(self, query, t='all', series=None):
        """The plan of a distribution query (no relation) with a vector of time stamps (:class:`DistributionPlan`); ``plan.reason`` says why
        a query stays on the host loop (None: the device takes it if the sequence of ``plan.study`` is resident there)."""
        stamps = self._stamps(t)
        return _plan_distribution(self, query, stamps, self._series(series, len(stamps)))

    def _call_many(self, query, t, silent, series):
        stamps = self._stamps(t)
        series = self._series(series, len(stamps))
        relational = len(re.split('>=|<=|==|>|<', query)) == 2
        out = None
        if relational and len(stamps) > 0:
            out = self._device_query(query, stamps, series)
        elif not relational and len(stamps) >= DIST_MIN_STAMPS:
            out = self._device_distribution(query, stamps, series)
        if out is None:
            out = self._loop(query, stamps, series)
            if relational:
                out = np.array(out, dtype=float)
        if not silent:
            if relational and len(stamps) > 0:
                print('P({}) at {} time steps: min = {}, max = {}'.format(query, len(stamps), np.nanmin(out), np.nanmax(out)))
            else:
                print('+ Computed {} at {} time steps'.format(query, len(stamps)))
        return out

    def _device_query(self, query, stamps, series):
        """The probabilities from the device, or None: the plan does not fit it, no study of the plan has its sequence there, or the
        engine has no such path (option parser_device = 0, the test doubles)."""
        candidates = [getattr(s, '_posterior_pending', None) for s in self.studies]
        candidates = [p for p in candidates if p is not None and hasattr(p, 'query')]
        if not candidates:
            return None
        options = getattr(getattr(candidates[0], 'engine', None), 'options', {})
        if options.get('parser_device', 1.0) == 0:
            return None
        try:
            plan = _plan(self, query, stamps, series, options.get('parser_pair_max', PAIR_MAX))
        except (ConfigurationError, ValueError):
            return None                              # (the loop raises what the scalar call raises)
        if plan.reason is not None:
            return None
        pending = getattr(plan.study, '_posterior_pending', None)
        if pending is None or not hasattr(pending, 'query') or list(pending.grid_size) != [len(m) for m in plan.marginal]:
            return None
        return pending.query(plan.steps, plan.ops, plan.consts, plan.relation, plan.marginal, **plan.spaces_kwargs())

    def _device_distribution(self, query, stamps, series):
        """The (bin labels, probabilities) of every time stamp with the sums from the device, or None: the plan does not fit it, the
        study's sequence is not resident there, the engine has no such path (option parser_device = 0, the test doubles) -- or anything at
        all went wrong while planning (the loop raises what the scalar call raises)."""
        try:
            candidates = [getattr(s, '_posterior_pending', None) for s in self.studies]
            candidates = [p for p in candidates if p is not None and hasattr(p, 'bins')]
            if not candidates:
                return None
            if getattr(getattr(candidates[0], 'engine', None), 'options', {}).get('parser_device', 1.0) == 0:
                return None
            plan = _plan_distribution(self, query, stamps, series)
            if plan.reason is not None:
                return None
            pending = getattr(plan.study, '_posterior_pending', None)
            if pending is None or not hasattr(pending, 'bins') or int(np.prod(pending.grid_size)) != plan.bin.size:
                return None
        except Exception:           # noqa: BLE001
            return None
        prob = pending.bins(plan.steps, plan.bin, plan.n_bins)
        return [(plan.labels.copy(), prob[i]) for i in range(len(stamps))]


def _binning(values):
    """The equal bins of a derived quantity (:399-418): ``int((max - min) / largest gap)`` edges from min to max; -> (n_bins, edges, the
    half-open bin [lower, upper) of every value, which values take part).  The scalar call and the device plan both bin with this."""
    values = values.copy()
    values[np.isinf(values)] = np.nan
    dmin, dmax = np.nanmin(values), np.nanmax(values)
    gap = np.nanmax(np.diff(np.sort(values)))                               # bin size = largest gap between two derived values
    n_bins = int((dmax - dmin) / gap)
    bins = np.linspace(dmin, dmax, n_bins)
    # probabilities of the half-open bins [lower, upper), labelled by their upper edge (:408-418)
    index = np.searchsorted(bins, values, side='right') - 1
    ok = ~np.isnan(values) & (index >= 0) & (index < n_bins - 1)
    return n_bins, bins, index, ok


def _is_vector(t):
    if isinstance(t, str):
        return t == 'all'
    if isinstance(t, np.ndarray):
        if t.ndim > 1:
            raise ConfigurationError('t takes a 1-D array of time stamps, got shape {}.'.format(t.shape))
        return t.ndim == 1
    return isinstance(t, (list, tuple))


# ---- the plan of a probability query at many time stamps ---------------------------------------------------------------------------------
# A vector-t probability query is a weighted count: the sum, over the product of its index spaces, of the product of the spaces'
# probabilities wherever lhs - rhs REL 0 holds.  The plan walks the expression ONCE with symbolic quantities through the very
# precedence-climbing and the very _arith / _independent rules of the scalar call, and assigns every node an index space:
#   * the parameters of one study (at the one time stamp of the step) share the space of that study's grid;
#   * the hyper-parameters of one study share the space of its hyper-grid (an OnlineStudy: one space per transition model);
#   * every outer product opens a new space, and -- the scalar call's quirk, kept -- anything combined with a derived quantity is
#     independent of it: a third space.
# The device (bayesloop_amd/csrc/blhip_query.hpp) takes one space (A, a parameter grid whose sequence is resident there) or two (A x B, B
# held by the host).  Every maximal subtree that depends on ONE axis of A, on B alone or on the series alone is evaluated HERE, with the
# NumPy / scipy.special calls the scalar call uses, and enters the program as a table; only nodes that mix axes or spaces are interpreted on
# the device, and only + - * / ^ abs sqrt exp log cos sin can be.  Everything else stays on the loop over the scalar call.
# default of engine option parser_pair_max, the largest G_a * G_b the pair kernel takes: the largest pair space measured (8000 x 8000 cells;
# the kernel was 13 to 326 times faster than the loop at every size from 50 x 50 up, profiles/parser_query_notes.md) -- no break-even was found
PAIR_MAX = 6.4e7
_DEVICE_FUNCS = {'abs': 'ABS', 'absolute': 'ABS', 'fabs': 'ABS', 'sqrt': 'SQRT', 'exp': 'EXP', 'log': 'LOG', 'cos': 'COS', 'sin': 'SIN'}
_REL_CODES = {'<': 0, '<=': 1, '==': 2, '>': 3, '>=': 4}
_SET = object()                # stands for "probabilities selected" in a symbolic quantity


class _NoPlan(Exception):
    def __init__(self, reason, n_spaces=None):
        Exception.__init__(self, reason)
        self.reason, self.n_spaces = reason, n_spaces


class _Steps:
    """A number that changes with the step: one Python float per step, combined float by float, as the loop over scalar calls does."""

    def __init__(self, v):
        self.v = [float(x) for x in v]


def _number_node(x):
    return ('steps', x.v) if isinstance(x, _Steps) else ('const', x)


class _Sym(_Quantity):
    """A quantity of the plan: its expression tree and index space instead of values and probabilities."""

    def __init__(self, node, space, name, kind, study, time):
        _Quantity.__init__(self, np.zeros(1), prob=_SET, name=name, time=time, study=study, kind=kind)
        self.node, self.space = node, space

    def copy(self):
        return _Sym(self.node, self.space, self.name, self.kind, self.study, self.time)

    def over(self, node):
        return _Sym(node, self.space, self.name, self.kind, self.study, self.time)


class _Planner(Parser):
    def __init__(self, parser):
        self.studies, self.names, self.functions = parser.studies, parser.names, parser.functions
        self.pair = None           # the two spaces of the one outer product a device plan may hold

    def _apply(self, fn, name, operand):
        if isinstance(operand, _Sym):
            return operand.over(('fn', name, fn, operand.node))
        if isinstance(operand, _Steps):
            with np.errstate(all='ignore'):
                return _Steps([fn(x) for x in operand.v])
        return fn(operand)

    def _arith(self, sym, a, b):
        op = _ARITH[sym]
        qa, qb = isinstance(a, _Sym), isinstance(b, _Sym)
        if not qa and not qb:
            with np.errstate(all='ignore'):
                if isinstance(a, _Steps) or isinstance(b, _Steps):
                    n = len(a.v) if isinstance(a, _Steps) else len(b.v)
                    va, vb = (a.v if isinstance(a, _Steps) else [a] * n), (b.v if isinstance(b, _Steps) else [b] * n)
                    return _Steps([op(x, y) for x, y in zip(va, vb)])
                return op(a, b)
        if qa and qb:
            node = ('op', sym, a.node, b.node)
            if self._independent(a, b):
                if self.pair is not None or a.space == b.space:
                    raise _NoPlan('three or more index spaces', 3)
                self.pair = (a.space, b.space)
                return _Sym(node, 'pair', '_derived', 'derived', None, None)
            if a.space != b.space:
                raise _NoPlan('hyper-parameters of two transition models of an OnlineStudy combined element by element')
            return a.over(node)
        if qa:
            return a.over(('op', sym, a.node, _number_node(b)))
        return b.over(('op', sym, _number_node(a), b.node))


def _node_text(node):
    kind = node[0]
    if kind == 'const':
        return repr(float(node[1]))
    if kind == 'steps':
        return '<series>'
    if kind == 'leaf':
        return node[1]
    if kind == 'fn':
        return '{}({})'.format(node[1], _node_text(node[3]))
    return '({} {} {})'.format(_node_text(node[2]), node[1], _node_text(node[3]))


def _node_eval(node, env, step=None):
    """The subtree with the calls of the scalar path: leaves from env (name -> array), a series at `step`."""
    kind = node[0]
    if kind == 'const':
        return node[1]
    if kind == 'steps':
        return node[1][step]
    if kind == 'leaf':
        return env[node[1]]
    with np.errstate(all='ignore'):
        if kind == 'fn':
            return node[2](_node_eval(node[3], env, step))
        return _ARITH[node[1]](_node_eval(node[2], env, step), _node_eval(node[3], env, step))


class QueryPlan:
    """What a vector-t probability query needs from the device.  reason: None, or why the query stays on the host loop; n_spaces: index
    spaces of the query (None: not counted); study: whose parameter grid is space A; steps: rows of its sequence; ops / consts / relation /
    marginal / series / b_values / b_prob / b_const: the arguments of HipEngine.posterior_query; tables: (kind, text of the subtree) of every
    subtree evaluated on the host -- kind 'axis<k>', 'b', 'series' or 'const'."""

    def __init__(self, reason=None, n_spaces=None):
        self.reason, self.n_spaces = reason, n_spaces
        self.study = None
        self.steps = self.ops = self.consts = self.relation = self.marginal = self.series = self.b_values = self.b_prob = None
        self.b_const, self.tables, self.spaces = False, [], []

    def spaces_kwargs(self):
        kw = {}
        if self.series is not None:
            kw['series'] = self.series
        if self.b_prob is not None:
            kw.update(b_values=self.b_values, b_prob=self.b_prob, b_const=self.b_const)
        return kw


def _plan(parser, query, stamps, series, pair_max=None):
    from . import _abi
    parts = re.split('>=|<=|==|>|<', query)
    if len(parts) != 2:
        return QueryPlan('no probability query')
    try:
        return _plan_relational(parser, query, parts, stamps, series, pair_max, _abi)
    except _NoPlan as e:
        return QueryPlan(e.reason, e.n_spaces)


def _symbols(parser):
    """Symbolic quantities: what _load(t) gives for a scalar t, without values -> (leaves, quantities)"""
    leaves, quantities = {}, {}
    for study in parser.studies:
        online = _is_online(study)
        if online and not getattr(study, 'storeHistory', True):
            raise _NoPlan('an OnlineStudy without history')
        for index, name in enumerate(study.observationModel.parameterNames):
            space = ('param', id(study))
            leaves[name] = dict(space=space, study=study, axis=index)
            quantities[name] = _Sym(('leaf', name), space, name, 'param', study, 0)
        if online:
            for j, names in enumerate(study.hyperParameterNames):
                for k, name in enumerate(names):
                    space = ('hyper', id(study), j)
                    leaves[name] = dict(space=space, study=study, model=j, values=np.asarray(study.hyperParameterValues[j], dtype=float)[:, list(names).index(name)])
                    quantities[name] = _Sym(('leaf', name), space, name, 'hyper', study, 0)
        elif hasattr(study, 'flatHyperParameterNames'):
            for name in study.flatHyperParameterNames:
                k = study._getHyperParameterIndex(study.transitionModel, name)
                grid = getattr(study, 'allHyperGridValues', None)
                if grid is None or len(grid) == 0:
                    grid = study.hyperGridValues
                space = ('hyper', id(study), 0)
                leaves[name] = dict(space=space, study=study, model=None, values=np.asarray(grid, dtype=float)[:, k])
                quantities[name] = _Sym(('leaf', name), space, name, 'hyper', study, None)
    return leaves, quantities


def _step_indices(parser, stamps):
    """The rows of the time stamps: their first places among the stamps of the first study, the rule for t (:291)"""
    stamps0 = list(parser.studies[0].formattedTimestamps)
    first = {}
    for i, ts in enumerate(stamps0):
        first.setdefault(ts, i)
    try:
        return np.array([first[ts] for ts in stamps], dtype=np.int64)
    except (KeyError, TypeError):
        return np.array([stamps0.index(ts) for ts in stamps], dtype=np.int64)       # (ValueError for an unknown stamp, as the scalar call)


def _plan_relational(parser, query, parts, stamps, series, pair_max, _abi):
    n_steps = len(stamps)
    steps = _step_indices(parser, stamps)
    leaves, quantities = _symbols(parser)
    # ---- the expression, walked once
    planner = _Planner(parser)
    reduced = '-1*(' + parts[1] + ')+' + parts[0]
    numbers = {name: _Steps(v) for name, v in series.items()}
    tokens = _tokenize(reduced, set(parser.names), parser.functions, numbers or None)
    derived, pos = planner._expression(tokens, 0, quantities)
    if pos != len(tokens) or not isinstance(derived, _Sym):
        raise ConfigurationError('Cannot parse query.')                             # (the scalar call says what is wrong)
    spaces = list(planner.pair) if derived.space == 'pair' else [derived.space]
    a_space = None
    for want_resident in (True, False):
        for sp in spaces:
            if sp[0] != 'param' or a_space is not None:
                continue
            study = next(s for s in parser.studies if id(s) == sp[1])
            pending = getattr(study, '_posterior_pending', None)
            if not want_resident or (pending is not None and hasattr(pending, 'query')):
                a_space = sp
    if a_space is None:
        raise _NoPlan('no parameter grid among the index spaces', len(spaces))
    b_space = next((sp for sp in spaces if sp != a_space), None)
    plan = QueryPlan(None, len(spaces))
    plan.spaces = [a_space] + ([b_space] if b_space is not None else [])
    plan.study = A = next(s for s in parser.studies if id(s) == a_space[1])
    plan.steps = steps
    plan.relation = _REL_CODES[next(sym for sym, _ in _RELATIONS if sym in query)]
    plan.marginal = [np.asarray(m, dtype=float) for m in A.marginalGrid]
    n_a = [len(m) for m in plan.marginal]
    if len(n_a) > _abi.MAX_DIM:
        raise _NoPlan('a grid of more than {} parameters'.format(_abi.MAX_DIM), len(spaces))
    T_a = len(A.formattedTimestamps)
    if n_steps and (steps.min() < 0 or steps.max() >= T_a):
        raise _NoPlan('a time stamp of the first study beyond the sequence of the study queried', len(spaces))
    n_b = 0
    if b_space is not None:
        B = next(s for s in parser.studies if id(s) == b_space[1])
        n_b = int(np.prod(B.gridSize)) if b_space[0] == 'param' else len(next(l['values'] for l in leaves.values() if l['space'] == b_space))
        if pair_max is not None and float(np.prod(n_a)) * n_b > pair_max:
            raise _NoPlan('a pair space of {} x {} cells, above parser_pair_max'.format(int(np.prod(n_a)), n_b), 2)

    # ---- what every node depends on: axes of A, B, the series
    def deps(node):
        kind = node[0]
        if kind == 'const':
            return frozenset()
        if kind == 'steps':
            return frozenset(['S'])
        if kind == 'leaf':
            leaf = leaves[node[1]]
            return frozenset([('A', leaf['axis'])]) if leaf['space'] == a_space else frozenset(['B'])
        if kind == 'fn':
            return deps(node[3])
        return deps(node[2]) | deps(node[3])

    def b_column(name):
        leaf = leaves[name]
        return np.ravel(leaf['study'].grid[leaf['axis']]) if leaf['space'][0] == 'param' else leaf['values']

    ops, consts, series_cols, b_cols = [], [], [], []

    def push_const(x):
        consts.append(float(x))
        ops.append((_abi.LP_CONST, len(consts) - 1))

    def emit(node):
        """-> the stack depth the code of this node needs"""
        d = deps(node)
        if not d:
            value = _node_eval(node, {})
            if node[0] != 'const':
                plan.tables.append(('const', _node_text(node)))
            push_const(value)
            return 1
        if d == {'S'}:
            with np.errstate(all='ignore'):
                series_cols.append([float(_node_eval(node, {}, i)) for i in range(n_steps)])
            plan.tables.append(('series', _node_text(node)))
            ops.append((_abi.LP_STEP, len(series_cols) - 1))
            return 1
        if d == {'B'}:
            env = {name: b_column(name) for name, leaf in leaves.items() if leaf['space'] == b_space}
            b_cols.append(np.asarray(_node_eval(node, env), dtype=float) * np.ones(n_b))
            plan.tables.append(('b', _node_text(node)))
            ops.append((_abi.QP_BCOL, len(b_cols) - 1))
            return 1
        if len(d) == 1:
            (_, axis), = d
            if node[0] == 'leaf':
                ops.append((_abi.LP_PARAM, axis))
                return 1
            env = {name: plan.marginal[axis] for name, leaf in leaves.items() if leaf['space'] == a_space and leaf['axis'] == axis}
            table = np.asarray(_node_eval(node, env), dtype=float) * np.ones(n_a[axis])
            plan.tables.append(('axis%d' % axis, _node_text(node)))
            ops.append((_abi.LP_AXIS, axis | (len(consts) << 2)))
            consts.extend(table.tolist())
            return 1
        if node[0] == 'fn':
            code = _DEVICE_FUNCS.get(node[1])
            if code is None or getattr(np, node[1], None) is not node[2]:
                raise _NoPlan('function "{}" over more than one axis or space'.format(node[1]), len(spaces))
            depth = emit(node[3])
            ops.append((getattr(_abi, 'LP_' + code), 0))
            return depth
        sym, left, right = node[1], node[2], node[3]
        if sym == '^' and right[0] == 'const' and right[1] == 2.0:
            depth = emit(left)                        # NumPy squares by one multiplication
            ops.append((_abi.LP_POWI, 2))
            return depth
        depth = max(emit(left), 1 + emit(right))
        if sym == '-':
            ops.append((_abi.LP_NEG, 0))              # a - b = a + (-b), exactly
        ops.append(({'+': _abi.LP_ADD, '-': _abi.LP_ADD, '*': _abi.LP_MUL, '/': _abi.LP_DIV, '^': _abi.LP_POW}[sym], 0))
        return depth

    depth = emit(derived.node)
    if depth > _abi.LP_MAX_STACK or len(ops) > _abi.LP_MAX_OPS:
        raise _NoPlan('a program of {} ops and stack depth {}'.format(len(ops), depth), len(spaces))
    plan.ops = np.array(ops, dtype=np.int32).reshape(-1, 2)
    plan.consts = np.array(consts, dtype=float)
    if series_cols:
        plan.series = np.ascontiguousarray(np.array(series_cols, dtype=float).T)
    # ---- B: its columns and its probabilities at the steps
    if b_space is not None:
        plan.b_values = np.array(b_cols, dtype=float).reshape(len(b_cols), n_b)
        if b_space[0] == 'param':
            plan.b_prob = np.array([np.ravel(_posterior_row(B, int(i))) for i in steps], dtype=float).reshape(n_steps, n_b)
        elif _is_online(B):
            seq, j = B.hyperParameterSequence, b_space[2]
            plan.b_prob = np.array([np.asarray(seq[int(i)][j], dtype=float) / np.sum(seq[int(i)][j]) for i in steps]).reshape(n_steps, n_b)
        else:
            d = np.asarray(B.hyperParameterDistribution, dtype=float)
            plan.b_prob, plan.b_const = (d / d.sum()).reshape(1, n_b), True
    return plan


# ---- the plan of a distribution query at many time stamps ------------------------------------------------------------------------------------
# A query without a relation over the parameters of ONE study is element-wise arithmetic on that study's grid: its values, the bins of the
# scalar call and the bin of every cell are functions of the grid alone, only the probabilities change with the time stamp.  The plan bins the
# grid ONCE -- with the scalar call's own host arithmetic (_load at the first stamp, _expression, _binning): the bin of a cell is decided by
# comparisons of values, so they never come from the device interpreter -- and the device sums every selected row of the sequence over the
# cells of each bin (bayesloop_amd/csrc/blhip_bins.hpp).  Two spaces, hyper-parameters, "@" and series (the bins would change with the step) stay
# on the loop over the scalar call, and so does every query the scalar call raises on: the loop raises it.
# fewest time stamps the device path takes, measured (profiles/parser_bins_notes.md): the plan is one scalar call's host work (its _load, its
# values, its sort) plus the order of the map and two launches, so at 1 stamp the loop was 1.2 to 2.3 times faster at every size, at 2 stamps
# still faster on grids of 50 and 1000 cells (the device 0.88 and 0.94 of the loop's speed) and slower on 100 x 100 and 512 x 512 cells; from 3
# stamps on the device was faster everywhere (1.3 to 2.7 times, 2.2 to 8.1 times at 8) -- fewer than 3 stamps: the loop
DIST_MIN_STAMPS = 3


class DistributionPlan:
    """What a vector-t distribution query needs from the device.  reason: None, or why the query stays on the host loop; study: whose
    parameter grid the query lives on; steps: rows of its sequence; labels: the bin labels of the scalar call (upper edges); bin: int32 per
    cell of the grid, the bin of the cell or -1 where the scalar call leaves it out; n_bins = len(labels)."""

    def __init__(self, reason=None):
        self.reason = reason
        self.study = self.steps = self.labels = self.bin = None
        self.n_bins = 0


def _plan_distribution(parser, query, stamps, series):
    if len(re.split('>=|<=|==|>|<', query)) != 1:
        return DistributionPlan('no distribution query')
    if series:
        return DistributionPlan('a series: the bins change with the time stamp')
    if '@' in query:
        return DistributionPlan('a time stamp pinned with "@"')
    if len(stamps) == 0:
        return DistributionPlan('no time stamps')
    try:
        steps = _step_indices(parser, stamps)
        _, quantities = _symbols(parser)
        planner = _Planner(parser)
        tokens = _tokenize(query, set(parser.names), parser.functions)
        derived, pos = planner._expression(tokens, 0, quantities)
        if pos != len(tokens) or not isinstance(derived, _Sym):
            raise ConfigurationError('Cannot parse query.')
    except _NoPlan as e:
        return DistributionPlan(e.reason)
    except Exception as e:          # noqa: BLE001 -- whatever it is, the loop over the scalar call raises it
        return DistributionPlan('the scalar call raises {}: {}'.format(type(e).__name__, e))
    if derived.space == 'pair':
        return DistributionPlan('two index spaces: the values are an outer product')
    if derived.space[0] != 'param':
        return DistributionPlan('hyper-parameters: no sequence of theirs is resident on the device')
    A = next(s for s in parser.studies if id(s) == derived.space[1])
    if steps.min() < 0 or steps.max() >= len(A.formattedTimestamps):
        return DistributionPlan('a time stamp of the first study beyond the sequence of the study queried')
    try:
        # the values of the scalar call at the first stamp, by its own arithmetic
        value, _ = Parser._expression(parser, tokens, 0, parser._load(stamps[0]))
        with np.errstate(all='ignore'):
            n_bins, bins, index, ok = _binning(value.values)
        labels = bins[:-1] + (bins[1] - bins[0])
    except Exception as e:          # noqa: BLE001
        return DistributionPlan('the scalar call raises {}: {}'.format(type(e).__name__, e))
    if index.size != int(np.prod(A.gridSize)) or n_bins - 1 != labels.size:
        return DistributionPlan('values that do not live on the grid of the study')
    plan = DistributionPlan()
    plan.study, plan.steps, plan.labels, plan.n_bins = A, steps, labels, int(labels.size)
    plan.bin = np.where(ok, index, -1).astype(np.int32)
    return plan


def _is_online(study):
    return hasattr(study, 'transitionModels') and hasattr(study, 'hyperParameterSequence')


def _posterior_row(study, index):
    """One time step of the study's posterior sequence without materialising the sequence when it still lives on the GPU."""
    pending = getattr(study, '_posterior_pending', None)
    if pending is not None and hasattr(pending, 'row'):
        return pending.row(index)
    return np.asarray(study.posteriorSequence[index])
