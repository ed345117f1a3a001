"""
TEST DOUBLE for blocks of an online study: tests/oracle_engine.py's OracleEngine with what OnlineStudy.stepMany asks of an engine on top --
resumed, carried fits of SEVERAL steps (built from the oracle's transition_forward), the kept sequence of a forward-only fit, the
time-varying mixture (a tensordot per step) in history planes, copies of carried states and the planner's answer.  Installed with
``bayesloop_amd.set_engine`` by the non-GPU tests only.
"""
import numpy as np

from oracle import bl_oracle as orc
from bayesloop_amd import _abi
from bayesloop_amd.engine import FitResult
from oracle_engine import OracleEngine


class BlockOracleEngine(OracleEngine):
    name = 'oracle-block-test-double'

    def __init__(self, chunk_steps=None):
        super().__init__()
        self.options = {}
        self.chunk_steps = chunk_steps        # steps per time chunk the planner answers with (None: the whole block)
        self.block_fits = []                  # (T, resume, keep_posterior) of every resumed / carried fit
        self._seq = None
        self._planes = None

    def set_option(self, key, value):
        self.options[key] = float(value)

    def online_block_steps(self, grid_size, chains, planes, N):
        return N if self.chunk_steps is None else self.chunk_steps

    def carry_copy(self, src_slot, dst_slot):
        self._carry[dst_slot] = np.array(self._carry[src_slot], dtype=float)

    def _step_values(self, row, k):
        """one chain's oracle value list for step k of a block: a DETERMINISTIC op takes entry k of its table of forward shifts"""
        vals, T = [], len(self._ts)
        for j, op in enumerate(self._abi_ops):
            if op[0] == _abi.OP_DETERMINISTIC_ARG:
                continue
            if op[0] == _abi.OP_DETERMINISTIC:
                vals.append((np.zeros(0), np.asarray([row[j + 1 + k]], dtype=float)))
            elif op[0] in (_abi.OP_STATIC, _abi.OP_INDEPENDENT):
                vals.append(None)
            else:
                vals.append(row[j])
        return vals

    def fit(self, problem, op_values, forward_only=False, evidence_only=False, keep_posterior=False, accumulate=False,
            log_chain_weight=None, owner=None, resume=False, carry=False):
        if not (resume or carry):
            return super().fit(problem, op_values, forward_only=forward_only, evidence_only=evidence_only, keep_posterior=keep_posterior,
                               accumulate=accumulate, log_chain_weight=log_chain_weight, owner=owner)
        assert evidence_only or forward_only
        g, om, ops, data, lik, reset = self._unpack(problem)
        n, T = len(op_values), problem.T
        self.block_fits.append((T, bool(resume), bool(keep_posterior)))
        ts = np.asarray(problem.timestamps, dtype=float)
        logE, local = np.zeros(n), np.zeros((n, T))
        astep = np.full(n, -1, dtype=np.int64)
        states = np.zeros([n] + g.size)
        seq = np.zeros([n, T] + g.size)
        for c in range(n):
            state = self._carry[problem.carry_slot][c] if resume else None
            with np.errstate(all='ignore'):
                for k in range(T):
                    L = orc.processed_pdf(om, g.grid, data[k]) if lik is None else lik[k]
                    if k == 0 and not resume:
                        alpha = np.asarray(problem.prior, dtype=float).reshape(g.size) * L
                    else:
                        tau = problem.resume_time if k == 0 else ts[k - 1]
                        alpha = orc.transition_forward(ops, self._step_values(op_values[c], k), state, tau, g, reset, self._indep) * L
                    ni = np.sum(alpha)
                    local[c, k] = ni * g.dV
                    logE[c] += np.log(ni) + np.log(g.dV)
                    if ni == 0 and astep[c] < 0:
                        astep[c] = k
                    state = alpha / ni
                    seq[c, k] = state
            states[c] = state
        if carry:
            self._carry[problem.carry_slot] = states
        self._seq = seq if keep_posterior and not evidence_only else None
        return FitResult(logE, local, None, astep, np.zeros(n, dtype=np.int32), {})

    def mix_sequence(self, weights, plane=0, n_planes=1, source=0, accumulate=False):
        w = np.asarray(weights, dtype=float)
        seq = self._seq if source == 0 else self._planes[1:]
        assert w.shape == seq.shape[:2][::-1]
        if self._planes is None or self._planes.shape != (n_planes,) + seq.shape[1:]:
            assert not accumulate and source == 0
            self._planes = np.zeros((n_planes,) + seq.shape[1:])
        m = np.array([np.tensordot(w[t], seq[:, t], axes=(0, 0)) for t in range(w.shape[0])])
        self._planes[plane] = m + (self._planes[plane] if accumulate else 0.0)

    def mix_means(self, marginal, T):
        g = orc.Grid(marginal)
        return np.array([[np.sum(self._planes[0][t] * g.grid[k]) for k in range(len(g.size))] for t in range(T)])

    def mix_read(self, T, grid_size, t0=0, t1=None, plane=0):
        return self._planes[plane][t0:t1].copy()
