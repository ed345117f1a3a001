"""
TEST DOUBLE: wraps an engine (the CPU doubles of tests/oracle_engine.py and tests/online_block_engine.py, or the HipEngine) and writes
down every call the package makes into it -- the method's name, its scalar and flag arguments as they are, and of every array its shape,
dtype and the SHA-256 of its bytes; the arrays inside a FitProblem field by field.  The calls into the engine are what the study classes
of bayesloop_amd/core.py decide: two versions of core.py that record the same trace have asked the device for the same work.

Calls an engine makes into itself (a double's ``fit`` reaching its base class) are not calls of the package and are not recorded.
"""
import dataclasses
import hashlib

import numpy as np

from bayesloop_amd.engine import FitProblem


def encode(v):
    """A call argument as a string: arrays by digest, containers element by element, studies and other objects by their type."""
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return 'nd[%s %s %s]' % ('x'.join(map(str, v.shape)), a.dtype.str, hashlib.sha256(a.tobytes()).hexdigest())
    if isinstance(v, FitProblem):
        return 'FitProblem{%s}' % ', '.join('%s=%s' % (f.name, encode(getattr(v, f.name))) for f in dataclasses.fields(v))
    if isinstance(v, (bool, np.bool_)):
        return repr(bool(v))
    if isinstance(v, (int, np.integer)):
        return 'i%d' % int(v)
    if isinstance(v, (float, np.floating)):
        return 'f%s' % float(v).hex()
    if v is None or isinstance(v, str):
        return repr(v)
    if isinstance(v, (list, tuple)):
        return '%s%s%s' % ('[(' [isinstance(v, tuple)], ', '.join(encode(x) for x in v), '])'[isinstance(v, tuple)])
    if isinstance(v, dict):
        return '{%s}' % ', '.join('%s: %s' % (k, encode(v[k])) for k in sorted(v))
    return '<%s>' % type(v).__name__


class RecordingEngine:
    """``RecordingEngine(inner)``: every attribute is the inner engine's; a method is the inner engine's method behind a line in
    ``self.trace``."""

    def __init__(self, inner):
        self.__dict__['inner'] = inner
        self.__dict__['trace'] = []

    def __getattr__(self, name):
        target = getattr(self.inner, name)          # (AttributeError where the inner engine has no such thing: hasattr sees through)
        if not callable(target) or isinstance(target, type):
            return target

        def recorded(*args, **kwargs):
            self.trace.append('%s(%s)' % (name, ', '.join([encode(a) for a in args] + ['%s=%s' % (k, encode(kwargs[k])) for k in sorted(kwargs)])))
            return target(*args, **kwargs)
        return recorded

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)
