"""NumPy float64 evaluation of a query program (bayesloop_amd/csrc/blhip_query.hpp), operation by operation in the order the device
interpreter executes it -- the indicator the device tests compare with -- and the weighted count in float64 for the host tests."""
import numpy as np

from bayesloop_amd import _abi

RELATIONS = {_abi.QR_LT: np.less, _abi.QR_LE: np.less_equal, _abi.QR_EQ: np.equal, _abi.QR_GT: np.greater, _abi.QR_GE: np.greater_equal}


def _powi(x, n):
    e, r, b, first = abs(int(n)), None, x, True
    while e:
        if e & 1:
            r = b if first else r * b
            first = False
        e >>= 1
        if e:
            b = b * b
    r = np.ones_like(x) if r is None else r
    return 1.0 / r if n < 0 else r


def interpret(ops, consts, marginal, step_values=None, b_values=None):
    """f over the cells of A, (G_a,), or -- with b_values (n_bcols, G_b) -- over the pairs, (G_a, G_b)."""
    consts = np.asarray(consts, dtype=float)
    n = [len(m) for m in marginal]
    G = int(np.prod(n))
    idx = np.unravel_index(np.arange(G), n)
    pair = b_values is not None
    over_a = (lambda v: v[:, None]) if pair else (lambda v: v)
    shape = (G, np.asarray(b_values).shape[1]) if pair else (G,)
    stack = []
    with np.errstate(all='ignore'):
        for code, arg in np.asarray(ops).reshape(-1, 2).tolist():
            if code == _abi.LP_CONST:
                stack.append(np.float64(consts[arg]))
            elif code == _abi.LP_PARAM:
                stack.append(over_a(np.asarray(marginal[arg], dtype=float)[idx[arg]]))
            elif code == _abi.LP_STEP:
                stack.append(np.float64(step_values[arg]))
            elif code == _abi.LP_AXIS:
                stack.append(over_a(consts[(arg >> 2) + idx[arg & 3]]))
            elif code == _abi.QP_BCOL:
                stack.append(np.asarray(b_values, dtype=float)[arg][None, :])
            elif code == _abi.LP_NEG:
                stack.append(-stack.pop())
            elif code == _abi.LP_ABS:
                stack.append(np.abs(stack.pop()))
            elif code == _abi.LP_SQRT:
                stack.append(np.sqrt(stack.pop()))
            elif code == _abi.LP_EXP:
                stack.append(np.exp(stack.pop()))
            elif code == _abi.LP_LOG:
                stack.append(np.log(stack.pop()))
            elif code == _abi.LP_COS:
                stack.append(np.cos(stack.pop()))
            elif code == _abi.LP_SIN:
                stack.append(np.sin(stack.pop()))
            elif code == _abi.LP_POWI:
                x = stack.pop()
                stack.append(x * x if arg == 2 else _powi(x, arg))
            else:
                b, a = stack.pop(), stack.pop()
                if code == _abi.LP_ADD:
                    stack.append(a + b)
                elif code == _abi.LP_MUL:
                    stack.append(a * b)
                elif code == _abi.LP_DIV:
                    stack.append(a / b)
                elif code == _abi.LP_POW:
                    stack.append(np.power(a, b))
                elif code == _abi.LP_LT:
                    stack.append(np.where(a < b, 1.0, 0.0))
                elif code == _abi.LP_LE:
                    stack.append(np.where(a <= b, 1.0, 0.0))
                elif code == _abi.LP_EQ:
                    stack.append(np.where(a == b, 1.0, 0.0))
                else:
                    raise ValueError('code %d' % code)
    assert len(stack) == 1
    return np.broadcast_to(np.asarray(stack[0], dtype=float), shape)


def indicator(relation, f):
    with np.errstate(invalid='ignore'):
        return RELATIONS[relation](f, 0.0)


def weighted_count(ops, consts, relation, marginal, p_a, series=None, b_values=None, b_prob=None, b_const=False):
    """float64 restatement of blhip_posterior_query over the rows p_a (n_steps, G_a) of the sequence."""
    out = np.empty(len(p_a))
    f = None
    for s, row in enumerate(p_a):
        if f is None or series is not None:
            f = interpret(ops, consts, marginal, None if series is None else series[s], b_values)
        ind = indicator(relation, f)
        if b_prob is None:
            out[s] = np.sum(np.ravel(row)[ind])
        else:
            pb = np.asarray(b_prob)[0 if b_const else s]
            w = np.ravel(row)[:, None] * pb[None, :]
            out[s] = np.sum(w[ind]) / np.sum(w)
    return out
