"""Restatement of the single-particle VMC sweep (engine.VmcEnsemble(move=
'particle')), from its definition, with NumPy and the CPU oracle's bindings
as they stand -- nothing here touches the device.

Chain c has Philox slot chain0 + c; the sweep of step counter t visits the
particles in label order k = 0 .. N - 1:

    (w0, w1) = oracle.vmc_move_block(seed, slot, t, k)
    z'       = wrap(z_k + oracle.vmc_move_unit(w0) * move_spread)
    D        = log f1(z') - log f1(z_k)
               + sum_{j != k} [log f2(|d(z', z_j)|) - log f2(|d(z_k, z_j)|)]
    u        = (w1 + 1/2) 2^-32             accept  <=>  log u < 2 D

with z_j the current positions (moves accepted earlier in the sweep included).
D is the logarithm of ith(k, s) of tests/_obdm_restatement.py at s = z' - z_k
unwrapped, one row of it: the factors `_log_f1`, `_log_f2` and the minimum
image are that module's (the whole ith costs N rows per move).  The yielded
log|psi| and energy are oracle.wf_abs_log / oracle.energy_drift of the
configuration after the sweep; a sweep that accepted nothing carries both
over.  Yield 0 of a fresh chain is the initial state.
"""
import numpy as np

from ._obdm_restatement import _log_f1, _log_f2, _min_image


def model_dicts(cfc):
    """What tests/_obdm_restatement.py takes, from a CFCSpec."""
    return {'params': cfc.model_params._asdict(),
            'obf_params': cfc.obf_params._asdict(),
            'tbf_params': cfc.tbf_params._asdict()}


def log_ratio(z, k, z_new, p):
    """log |psi(R')| - log |psi(R)| for particle k of row z moved to z_new
    (inside the box)."""
    mp = p['params']
    sc = mp['supercell_size']
    d = 0.0
    if not mp['is_free']:
        d += float(_log_f1(np.float64(z_new), p) - _log_f1(np.float64(z[k]), p))
    if not mp['is_ideal']:
        others = np.delete(z, k)
        new = np.abs(_min_image(z_new - others, sc))
        old = np.abs(_min_image(z[k] - others, sc))
        d += float(np.sum(_log_f2(new, p) - _log_f2(old, p)))
    return d


class Chain:
    """One chain: `run(nyield)` -> dict of the yields' positions [nyield, N]
    (label order), wf_abs_log, energy [nyield], move_stat [nyield], and per
    SWEEP (yield 0 of a fresh chain has none) accepted [nsweep, N], margin
    2 D - log u [nsweep, N], delta D [nsweep, N], proposals [nsweep, N]."""

    def __init__(self, oracle, model, p, pos, move_spread, seed, slot):
        self.oracle, self.model, self.p = oracle, model, p
        self.L = float(p['params']['supercell_size'])
        self.pos = np.array(pos, dtype=np.float64)
        self.spread, self.seed, self.slot = float(move_spread), seed, slot
        self.step = 0
        self.initial = True
        self.wf = self.energy = None

    def _evaluate(self):
        self.wf = self.oracle.wf_abs_log(self.model, self.pos)
        self.energy = self.oracle.energy_drift(self.model, self.pos)[0]

    def sweep(self):
        n = self.pos.size
        acc = np.zeros(n, dtype=bool)
        margin, delta, prop = np.zeros(n), np.zeros(n), np.zeros(n)
        for k in range(n):
            w0, w1 = self.oracle.vmc_move_block(self.seed, self.slot,
                                                self.step, k)
            zp = np.mod(self.pos[k] +
                        self.oracle.vmc_move_unit(w0) * self.spread, self.L)
            delta[k] = log_ratio(self.pos, k, zp, self.p)
            margin[k] = 2.0 * delta[k] - np.log((w1 + 0.5) * 2.0 ** -32)
            prop[k] = zp
            acc[k] = margin[k] > 0.0
            if acc[k]:
                self.pos[k] = zp
        self.step += 1
        if acc.any():
            self._evaluate()
        return acc, margin, delta, prop

    def run(self, nyield):
        n = self.pos.size
        out = dict(pos=np.zeros((nyield, n)), wf_abs_log=np.zeros(nyield),
                   energy=np.zeros(nyield),
                   move_stat=np.zeros(nyield, dtype=bool))
        sw = []
        for y in range(nyield):
            if self.initial:
                self.initial = False
                self._evaluate()
                out['move_stat'][y] = True
            else:
                sw.append(self.sweep())
                out['move_stat'][y] = sw[-1][0].any()
            out['pos'][y] = self.pos
            out['wf_abs_log'][y], out['energy'][y] = self.wf, self.energy
        for i, name in enumerate(('accepted', 'margin', 'delta', 'proposal')):
            out[name] = np.array([s[i] for s in sw]).reshape(len(sw), n)
        return out


def run_ensemble(oracle, model, p, pos0, move_spread, seed, nyield, chain0=0):
    """Every chain of an ensemble -> dict of arrays with the chain as the
    SECOND axis, as engine.VmcEnsemble.run_block hands them out."""
    runs = [Chain(oracle, model, p, row, move_spread, seed, chain0 + c)
            .run(nyield) for c, row in enumerate(pos0)]
    return {k: np.stack([r[k] for r in runs], axis=1) for k in runs[0]}
