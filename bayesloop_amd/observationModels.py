"""
Observation models (likelihood functions) -- the ``bl.om`` namespace.

Same constructor arguments and attributes as the reference (bayesloop/observationModels.py), so user code reads the
same.  What differs is who evaluates the likelihood on the grid during ``fit()``:

* ``Poisson``, ``Gaussian``, ``GaussianMean`` are evaluated INSIDE the fused HIP step kernels from the data point and
  per-axis tables (``device_model`` is their C-ABI code; reference pdfs at observationModels.py:502, 566-567, 705-706).
* ``Bernoulli``, ``Laplace``, ``WhiteNoise``, ``AR1``, ``ScaledAR1``: their (T, G) likelihood table is built ON THE DEVICE
  from the data (``blk::lik_table_kernel``; reference pdfs at observationModels.py:428-430, 635, 767, 830-831, 893-896):
  no host evaluation, no upload.
* ``SymPy`` and ``SciPy``: where the density is an expression the package can see (``SymPy``: always; ``SciPy``: a fixed list of
  distributions written out in bayesloop_amd/likprogram.py) it is compiled into a small postfix program and the (T, G) table is built
  ON THE DEVICE by ``bllp::lik_program_kernel`` -- no host evaluation, no upload.  Densities with a function outside the program's
  instruction set (``besseli`` of a parameter in VonMises), SciPy distributions off the list and subclasses that override ``pdf``
  take the next path.
* any other model -- user subclasses with a ``pdf(grid, dataSegment)`` method (the reference's duck-typed plug-in
  interface, observationModels.py:35-56), including subclasses that override the ``pdf`` of a model above -- is
  evaluated once on the host with the model's own ``pdf`` and uploaded as a (T, G) likelihood table; the recursion
  itself still runs on the GPU.
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from .exceptions import ConfigurationError
from .helper import cint, oint

try:
    from inspect import getfullargspec as _argspec
except ImportError:  # pragma: no cover
    from inspect import getargspec as _argspec


class ObservationModel:
    """Base class: missing data and multi-dimensional data handling (reference observationModels.py:35-56)."""

    device_model = _abi.OM_TABLE     # subclasses evaluated in-kernel override this
    segmentLength = 1
    multiplyLikelihoods = True
    name = 'observation model'

    def __str__(self):
        return self.name

    def processedPdf(self, grid, dataSegment):
        dataSegment = np.asarray(dataSegment)
        if dataSegment.ndim == 2 and self.multiplyLikelihoods:
            # one likelihood per data dimension, multiplied
            factors = [self.processedPdf(grid, column) for column in dataSegment.T]
            return np.prod(np.array(factors), axis=0)
        if np.isnan(dataSegment).any():
            return np.ones_like(grid[0])       # a missing observation leaves the distribution untouched
        return self.pdf(grid, dataSegment)

    def _init_params(self, names, values, prior, jeffreys=None):
        self.parameterNames = list(names)
        self.parameterValues = list(values)
        if isinstance(prior, str) and prior == 'Jeffreys':
            self.prior = jeffreys
        else:
            self.prior = prior


class Poisson(ObservationModel):
    """Poisson counts with rate ``name`` (reference observationModels.py:467-526)."""
    device_model = _abi.OM_POISSON

    def __init__(self, name='lambda', value=None, prior='Jeffreys'):
        self.name = 'Poisson'
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        self._init_params([name], [value], prior, self.jeffreys)

    def pdf(self, grid, dataSegment):
        k = dataSegment[0]
        return (grid[0] ** k) * np.exp(-grid[0]) / math.factorial(int(k))

    def estimateParameterValues(self, name, rawData):
        if name != self.parameterNames[0]:
            raise ConfigurationError('Poisson model does not contain a parameter "{}".'.format(name))
        return oint(0, 1.25 * np.nanmax(np.ravel(rawData)), 1000)

    def jeffreys(self, x):
        return np.sqrt(1. / x)


class Gaussian(ObservationModel):
    """Independent Gaussian observations with parameters mean, std (reference observationModels.py:529-595)."""
    device_model = _abi.OM_GAUSSIAN

    def __init__(self, name1='mean', value1=None, name2='std', value2=None, prior='Jeffreys'):
        self.name = 'Gaussian observations'
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        self._init_params([name1, name2], [value1, value2], prior, self.jeffreys)

    def pdf(self, grid, dataSegment):
        x = dataSegment[0]
        return np.exp(-((x - grid[0]) ** 2.) / (2. * grid[1] ** 2.) - .5 * np.log(2. * np.pi * grid[1] ** 2.))

    def estimateParameterValues(self, name, rawData):
        mean = np.nanmean(np.ravel(rawData))
        std = np.nanstd(np.ravel(rawData))
        if name == self.parameterNames[0]:
            return cint(mean - 2 * std, mean + 2 * std, 200)
        if name == self.parameterNames[1]:
            return oint(0, 2 * std, 200)
        raise ConfigurationError('Gaussian model does not contain a parameter "{}".'.format(name))

    def jeffreys(self, mu, sigma):
        return 1. / sigma ** 2.


class GaussianMean(ObservationModel):
    """Observed mean values with given error: data rows are (value, std) (reference observationModels.py:666-728)."""
    device_model = _abi.OM_GAUSSIAN_MEAN

    def __init__(self, name='mean', value=None, prior=None):
        self.name = 'Gaussian mean model'
        self.segmentLength = 1
        self.multiplyLikelihoods = False
        self._init_params([name], [value], prior)

    def pdf(self, grid, dataSegment):
        x, s = dataSegment[0, 0], dataSegment[0, 1]
        return np.exp(-((x - grid[0]) ** 2.) / (2. * s ** 2.) - .5 * np.log(2. * np.pi * s ** 2.))

    def estimateParameterValues(self, name, rawData):
        if name != self.parameterNames[0]:
            raise ConfigurationError('Gaussian mean model does not contain a parameter "{}".'.format(name))
        obs = np.array([d[0] for d in rawData])
        lo, hi = np.nanmin(obs), np.nanmax(obs)
        return oint(lo - (hi - lo), hi + (hi - lo), 1000)


# ---- closed-form models evaluated through the likelihood-table path ----------------------------------------------


class Bernoulli(ObservationModel):
    """Bernoulli trials with success probability p (reference observationModels.py:394-464)."""

    device_model = _abi.OM_BERNOULLI    # likelihood table built on the device (include/blhip.h)

    def __init__(self, name='p', value=None, prior='Jeffreys'):
        self.name = 'Bernoulli'
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        self._init_params([name], [value], prior, self.jeffreys)

    def pdf(self, grid, dataSegment):
        p = np.array(grid[0], dtype=float)
        p[(p > 1.) | (p < 0.)] = 0.
        return p if dataSegment[0] else 1. - p

    def estimateParameterValues(self, name, rawData):
        if name != self.parameterNames[0]:
            raise ConfigurationError('Bernoulli model does not contain a parameter "{}".'.format(name))
        return cint(0, 1, 1000)

    def jeffreys(self, x):
        return 1. / np.sqrt(x * (1. - x))


class Laplace(ObservationModel):
    """Laplace observations with mean and scale (reference observationModels.py:598-663)."""

    device_model = _abi.OM_LAPLACE    # likelihood table built on the device (include/blhip.h)

    def __init__(self, name1='mean', value1=None, name2='scale', value2=None, prior='Jeffreys'):
        self.name = 'Laplace observations'
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        self._init_params([name1, name2], [value1, value2], prior, self.jeffreys)

    def pdf(self, grid, dataSegment):
        return np.exp(-np.abs(dataSegment[0] - grid[0]) / grid[1]) / (2. * grid[1])

    def estimateParameterValues(self, name, rawData):
        mean = np.nanmean(np.ravel(rawData))
        std = np.nanstd(np.ravel(rawData))
        if name == self.parameterNames[0]:
            return cint(mean - 2 * std, mean + 2 * std, 200)
        if name == self.parameterNames[1]:
            return oint(0, np.sqrt(2) * std, 200)
        raise ConfigurationError('Laplace model does not contain a parameter "{}".'.format(name))

    def jeffreys(self, mu, scale):
        return 1. / scale ** 2.


class WhiteNoise(ObservationModel):
    """Zero-mean Gaussian noise with amplitude std (reference observationModels.py:731-792)."""

    device_model = _abi.OM_WHITE_NOISE    # likelihood table built on the device (include/blhip.h)

    def __init__(self, name='std', value=None, prior='Jeffreys'):
        self.name = 'White noise process (Zero-mean Gaussian)'
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        self._init_params([name], [value], prior, self.jeffreys)

    def pdf(self, grid, dataSegment):
        return np.exp(-(dataSegment[0] ** 2.) / (2. * grid[0] ** 2.) - .5 * np.log(2. * np.pi * grid[0] ** 2.))

    def estimateParameterValues(self, name, rawData):
        if name != self.parameterNames[0]:
            raise ConfigurationError('White noise model does not contain a parameter "{}".'.format(name))
        return oint(0, 2 * np.nanstd(np.ravel(rawData)), 1000)

    def jeffreys(self, sigma):
        return 1. / sigma


class AR1(ObservationModel):
    """Auto-regressive process of first order, segment length 2 (reference observationModels.py:795-852)."""

    device_model = _abi.OM_AR1    # likelihood table built on the device (include/blhip.h)

    def __init__(self, name1='correlation coefficient', value1=None, name2='noise amplitude', value2=None, prior=None):
        self.name = 'Autoregressive process of first order (AR1)'
        self.segmentLength = 2
        self.multiplyLikelihoods = True
        self._init_params([name1, name2], [value1, value2], prior)

    def pdf(self, grid, dataSegment):
        resid = dataSegment[1] - grid[0] * dataSegment[0]
        return np.exp(-(resid ** 2.) / (2. * grid[1] ** 2.) - .5 * np.log(2. * np.pi * grid[1] ** 2.))

    def estimateParameterValues(self, name, rawData):
        if name == self.parameterNames[0]:
            return oint(-1, 1, 200)
        if name == self.parameterNames[1]:
            return oint(0, 2 * np.nanstd(np.ravel(rawData)), 200)
        raise ConfigurationError('AR1 model does not contain a parameter "{}".'.format(name))


class ScaledAR1(ObservationModel):
    """AR1 parametrised by the standard deviation of the observations (reference observationModels.py:855-917)."""

    device_model = _abi.OM_SCALED_AR1    # likelihood table built on the device (include/blhip.h)

    def __init__(self, name1='correlation coefficient', value1=None, name2='standard deviation', value2=None,
                 prior=None):
        self.name = 'Scaled autoregressive process of first order (AR1)'
        self.segmentLength = 2
        self.multiplyLikelihoods = True
        self._init_params([name1, name2], [value1, value2], prior)

    def pdf(self, grid, dataSegment):
        r, s = grid[0], grid[1]
        scaled = s * np.sqrt(1 - r ** 2.)
        resid = dataSegment[1] - r * dataSegment[0]
        return np.exp(-(resid ** 2.) / (2. * scaled ** 2.) - .5 * np.log(2. * np.pi * scaled ** 2.))

    def estimateParameterValues(self, name, rawData):
        if name == self.parameterNames[0]:
            return oint(-1, 1, 200)
        if name == self.parameterNames[1]:
            return oint(0, 2 * np.nanstd(np.ravel(rawData)), 200)
        raise ConfigurationError('AR1 model does not contain a parameter "{}".'.format(name))


class NumPy(ObservationModel):
    """User-defined likelihood ``function(data, *parameter_arrays)`` (reference observationModels.py:59-143)."""

    def __init__(self, function, *args, **kwargs):
        if not hasattr(function, '__call__'):
            raise ConfigurationError('Expected a function as the first argument of NumPy observation model')
        for key in kwargs:
            if key not in ['prior']:
                raise TypeError("__init__() got an unexpected keyword argument '{}'".format(key))
        self.function = function
        self.name = function.__name__
        self.segmentLength = 1
        self.multiplyLikelihoods = False
        self.parameterNames = list(args[::2])
        self.parameterValues = list(args[1::2])
        spec = _argspec(function).args
        if len(self.parameterNames) != len(spec) - 1:
            raise ConfigurationError('Supplied function has {} parameters, observation model has {}'
                                     .format(len(spec) - 1, len(self.parameterNames)))
        if spec[0] != 'data':
            raise ConfigurationError('First argument of supplied function must be called "data"')
        self.prior = kwargs.get('prior', None)

    def pdf(self, grid, dataSegment):
        return self.function(dataSegment[0], *grid)


def _free_symbols(rv):
    """Free parameters of a SymPy random variable, in SymPy's own order (reference helper.py:122-145)."""
    try:
        symbols = rv._sorted_args[0].distribution.free_symbols          # SymPy <= 1.0
    except AttributeError:
        symbols = rv._sorted_args[1].distribution.free_symbols          # SymPy >= 1.1
    return list(symbols)


def jeffreys_prior_of(rv):
    """Jeffreys prior sqrt(det Fisher information) of a SymPy random variable, symbolically (reference jeffreys.py:18-60):
    returns (symbolic expression, numpy lambda of the free parameters)."""
    import sympy
    import sympy.abc as abc
    from sympy.stats import density
    try:
        support = rv._sorted_args[0].distribution.set
    except AttributeError:
        support = rv._sorted_args[1].distribution.set
    params = _free_symbols(rv)
    x = abc.x
    pdf = density(rv)(x)
    accumulate = sympy.summation if support.is_iterable else sympy.integrate
    fisher = sympy.Matrix.zeros(len(params), len(params))
    for i, pi in enumerate(params):
        for j, pj in enumerate(params):
            fisher[i, j] = accumulate(sympy.simplify(pdf * sympy.diff(sympy.ln(pdf), pi) * sympy.diff(sympy.ln(pdf), pj)),
                                      (x, support.inf, support.sup))
    expr = sympy.simplify(sympy.sqrt(fisher.det()))
    if expr == 0:
        raise ValueError('Jeffreys prior could not be computed.')
    return expr, sympy.lambdify(params, expr, 'numpy')


class SciPy(ObservationModel):
    """Observation model from a ``scipy.stats`` distribution (reference observationModels.py:146-269):
    ``bl.om.SciPy(scipy.stats.poisson, 'mu', bl.oint(0, 6, 1000), fixedParameters={'loc': 0})``.  Flat prior by default.
    The likelihood is the distribution's own pdf / pmf, evaluated on the host once per time step (table path)."""

    def __init__(self, rv, *args, **kwargs):
        module = getattr(rv, '__module__', '').split('.')
        if module[:2] != ['scipy', 'stats']:
            raise ConfigurationError('SciPy observation model must contain SciPy probability distribution')
        for key in kwargs:
            if key not in ['prior', 'fixedParameters']:
                raise TypeError("__init__() got an unexpected keyword argument '{}'".format(key))
        self.rv = rv
        self.name = rv.name
        if len(args) == 1 and isinstance(args[0], dict):
            self.parameterNames, self.parameterValues = list(args[0].keys()), list(args[0].values())
        else:
            self.parameterNames, self.parameterValues = list(args[::2]), list(args[1::2])
        self.prior = kwargs.get('prior', None)
        self.fixedParameterDict = kwargs.get('fixedParameters', {})
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        self.isContinuous = hasattr(rv, 'pdf')
        shapes = [] if rv.shapes is None else rv.shapes.split(', ')
        shapes.append('loc')
        if self.isContinuous:
            shapes.append('scale')
        free = [name for name in shapes if name not in self.fixedParameterDict]
        if len(self.parameterNames) == 0:
            self.parameterNames, self.parameterValues = free, [None] * len(free)
        unknown = set(self.parameterNames).difference(free)
        if unknown:
            raise ConfigurationError('The following parameter names from the observation model do not match the parameter '
                                     'names of the SciPy distribution: {} (options: {})'.format(list(unknown), free))

    def pdf(self, grid, dataSegment):
        params = dict(zip(self.parameterNames, grid))
        params.update(self.fixedParameterDict)
        f = self.rv.pdf if self.isContinuous else self.rv.pmf
        return f(dataSegment[0], **params)

    def likelihoodProgram(self):
        """The density as a program for the device (bayesloop_amd/likprogram.py), or None: the distribution is not among those written
        out there, a fixed parameter is no number, or ``pdf`` is overridden.  fixedParameters are folded as constants."""
        if '_program' not in self.__dict__:
            self._program = None
            if type(self).pdf is SciPy.pdf:
                from . import likprogram
                import sympy
                spec = likprogram.scipy_density(getattr(self.rv, 'name', None))
                try:
                    if spec is not None:
                        expr, x, symbols = spec
                        fixed = {symbols[k]: sympy.Float(float(v)) if float(v) != int(float(v)) else sympy.Integer(int(float(v)))
                                 for k, v in self.fixedParameterDict.items()}
                        if set(self.parameterNames) | set(self.fixedParameterDict) == set(symbols):
                            self._program = likprogram.compile_density(expr.subs(fixed), x, [symbols[n] for n in self.parameterNames],
                                                                       modules=['scipy', 'numpy'], axis_functions=True)
                except (KeyError, TypeError, ValueError):
                    self._program = None
        return self._program

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_program', None)          # (compiled again on first use: it holds host functions that need not pickle)
        return state


class SymPy(ObservationModel):
    """Observation model from a ``sympy.stats`` random variable (reference observationModels.py:272-391):
    ``bl.om.SymPy(sympy.stats.Normal('norm', mu, std), 'mu', bl.cint(0, 7, 200), 'std', bl.oint(0, 1, 200))``.
    The lambdified density is evaluated on the host once per time step (table path).

    Prior: the reference means to derive the Jeffreys prior symbolically when no prior is given, but reads ``self.rv``
    before assigning it (observationModels.py:351), so the attempt always fails and the prior is FLAT -- its published
    results (tests/test_observationmodels.py:11-27) are flat-prior results.  ``determineJeffreysPrior=True`` (default)
    therefore gives the flat prior here too, with the reference's warning; ``determineJeffreysPrior='symbolic'`` really
    derives sqrt(det Fisher information) with SymPy (:func:`jeffreys_prior_of`)."""

    def __init__(self, rv, *args, **kwargs):
        module = getattr(rv, '__module__', '').split('.')
        if module[:2] != ['sympy', 'stats']:
            raise ConfigurationError('SymPy observation model must contain SymPy random variable.')
        for key in kwargs:
            if key not in ['prior', 'determineJeffreysPrior']:
                raise TypeError("__init__() got an unexpected keyword argument '{}'".format(key))
        import sympy
        import sympy.abc as abc
        from sympy.stats import density
        from scipy.special import factorial, iv
        self.rv = rv
        self.name = str(rv)
        if len(args) == 1 and isinstance(args[0], dict):
            self.parameterNames, self.parameterValues = list(args[0].keys()), list(args[0].values())
        else:
            self.parameterNames, self.parameterValues = list(args[::2]), list(args[1::2])
        symbols = _free_symbols(rv)
        names = [str(p) for p in symbols]
        if len(self.parameterNames) == 0:
            self.parameterNames, self.parameterValues = names, [None] * len(names)
        unknown = set(self.parameterNames).difference(names)
        if unknown:
            raise ConfigurationError('The following parameter names from the observation model do not match the names '
                                     'of SymPy random variables: {}'.format(list(unknown)))
        ordered = [symbols[names.index(name)] for name in self.parameterNames]
        self.prior = kwargs.get('prior', None)
        self.segmentLength = 1
        self.multiplyLikelihoods = True
        mode = kwargs.get('determineJeffreysPrior', True)
        if self.prior is None and mode:
            print('    + Trying to determine Jeffreys prior. This might take a moment...')
            try:
                if mode != 'symbolic':
                    raise AttributeError("'SymPy' object has no attribute 'rv'")     # what happens in the reference
                expr, self.prior = jeffreys_prior_of(rv)
                print('    + Successfully determined Jeffreys prior: {}. Will use corresponding lambda function.'.format(expr))
            except Exception:
                print('    ! WARNING: Failed to determine Jeffreys prior. Will use flat prior instead.')
                self.prior = None
        x = abc.x
        self.densityExpression, self.densitySymbols = density(rv)(x), [x] + ordered
        self.density = sympy.lambdify([x] + ordered, self.densityExpression, modules=['numpy', {'factorial': factorial, 'besseli': iv}])

    def pdf(self, grid, dataSegment):
        return self.density(dataSegment[0], *grid)

    def likelihoodProgram(self):
        """The density as a program for the device (bayesloop_amd/likprogram.py), compiled on first use; None when the expression holds
        anything outside the program's instruction set, or ``pdf`` is overridden."""
        if '_program' not in self.__dict__:
            self._program = None
            if type(self).pdf is SymPy.pdf:
                from . import likprogram
                self._program = likprogram.compile_density(self.densityExpression, self.densitySymbols[0], self.densitySymbols[1:])
        return self._program

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_program', None)          # (compiled again on first use: it holds host functions that need not pickle)
        return state


def device_code(om):
    """C-ABI code of the observation model, or OM_TABLE when its ``pdf`` is not the built-in one (user subclass)."""
    for cls in type(om).__mro__:
        code = cls.__dict__.get('device_model')
        if code is not None:
            return code if getattr(type(om), 'pdf', None) is cls.__dict__.get('pdf', None) and code != _abi.OM_TABLE else _abi.OM_TABLE
    return _abi.OM_TABLE
