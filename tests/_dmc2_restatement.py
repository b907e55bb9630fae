"""The second-order DMC propagator (`propagator='quadratic'`,
csrc/qmc_evolve2.h) restated in numpy: a walker population stepped on the
host with the CPU oracle's local energy and drift (`oracle.energy_drift`), its
diffusion normals (`oracle.dmc_normal`) and its branching draws
(`oracle.philox_uniform2`, stream 2).  Branching, cloning and the E_ref
bookkeeping are the oracle's (oracle/qmc_oracle.c: orc_dmc_step; the rule
itself: tests/_branch_ref.py); only the move and the weight differ.  Nothing
here touches the device.

One step of child slot s with parent p = ref[s] at step counter t, units
hbar^2 / 2m = 1, F = grad log psi:

    R_a = wrap(R_p + sqrt(dt) xi1)          half diffusion
    R_m = wrap(R_a + dt F(R_a))             midpoint of the drift flow
    R_b = wrap(R_a + 2 dt F(R_m))           full drift, RK2
    R'  = wrap(R_b + sqrt(dt) xi2)          half diffusion
    log w' = -dt ((E(R') + E_p) / 2 - E_ref)

xi1 = dmc_normal(seed, slot, 2 t, label), xi2 = dmc_normal(seed, slot,
2 t + 1, label): the two Box-Muller normals of the Philox block the device
keys with t.
"""
import numpy as np

STREAM_DMC_BRANCH = 2           # oracle/qmc_oracle.h: ORC_STREAM_DMC_BRANCH


def wrap(z, L):
    """Floor-mod into [0, L) (qmc_base/utils.py:55-66)."""
    return np.mod(z, L)


def closest_pair(row, L):
    """The smallest pair separation on the ring, as a fraction of L: where
    it vanishes the sign of the pair's drift term flips."""
    z = np.sort(np.mod(row, L))
    gaps = np.diff(np.concatenate([z, z[:1] + L]))
    return float(gaps.min()) / L


def drift_flow(oracle, m, r_a, dt, rows=None):
    """R_a -> R_b: the drift over one time step (velocity 2 F), second order
    through the midpoint.  `rows` collects the two configurations the drift is
    evaluated at."""
    L = float(m.supercell_size)
    f_a = oracle.energy_drift(m, r_a)[2]
    r_m = wrap(r_a + dt * f_a, L)
    f_m = oracle.energy_drift(m, r_m)[2]
    if rows is not None:
        rows += [r_a, r_m]
    return wrap(r_a + 2 * dt * f_m, L)


def move(oracle, m, r_p, dt, xi1, xi2, rows=None):
    """R_p -> R' of one walker."""
    L = float(m.supercell_size)
    s = np.sqrt(dt)
    r_a = wrap(r_p + s * xi1, L)
    r_b = drift_flow(oracle, m, r_a, dt, rows)
    r_n = wrap(r_b + s * xi2, L)
    if rows is not None:
        rows.append(r_n)
    return r_n


def normals(oracle, seed, slot, t, n):
    """(xi1[N], xi2[N]) of walker slot `slot` at step counter t, by particle
    label."""
    xi1 = np.array([oracle.dmc_normal(seed, slot, 2 * t, i) for i in range(n)])
    xi2 = np.array([oracle.dmc_normal(seed, slot, 2 * t + 1, i)
                    for i in range(n)])
    return xi1, xi2


class Population:
    """The population a device ensemble with propagator='quadratic' holds,
    yield by yield.  After `step()`: `num_walkers`, `cloning_ref[:nw]`, and
    the YIELDED state -- the parents as cloned, `confs[:nw]` ([nw, 2, N]:
    positions, drift) and `energy[:nw]` -- which is what
    `DmcEnsemble.get_state()` returns and what every estimator sees.
    `branch_margin`: the smallest distance of a branching w + u from an
    integer so far; `pair_margin[s]`: per slot of the LAST step the smallest
    pair separation, of L, over its three evaluated rows; `min_pair_margin`:
    the smallest so far."""

    def __init__(self, oracle, m, ini_pos, time_step, max_num_walkers,
                 target_num_walkers, control_factor, seed=0, slot0=0,
                 ref_energy=None):
        self.oracle, self.m = oracle, m
        self.n = int(m.boson_number)
        self.L = float(m.supercell_size)
        self.dt = float(time_step)
        self.maxw, self.target = int(max_num_walkers), int(target_num_walkers)
        self.kappa, self.seed, self.slot0 = float(control_factor), seed, slot0
        pos = np.asarray(ini_pos, dtype=np.float64)[-self.target:]
        nw = len(pos)
        # build_state: energy and drift of every configuration, unit weights
        self.prev_confs = np.zeros((self.maxw, 2, self.n))
        self.prev_energy = np.zeros(self.maxw)
        self.prev_logw = np.zeros(self.maxw)
        for s in range(nw):
            e, _, f = oracle.energy_drift(m, pos[s])
            self.prev_confs[s, 0], self.prev_confs[s, 1] = pos[s], f
            self.prev_energy[s] = e
        self.prev_nw = nw
        self.ref_energy = float(self.prev_energy[:nw].mean()
                                if ref_energy is None else ref_energy)
        self.total_energy = self.total_weight = 0.0
        self.t = 0
        self.num_walkers = nw
        self.confs = self.prev_confs.copy()
        self.energy = self.prev_energy.copy()
        self.cloning_ref = np.zeros(self.maxw, dtype=np.int64)
        self.branch_margin = 1.0
        self.min_pair_margin = 1.0
        self.pair_margin = np.ones(self.maxw)
        self.crossed = 0

    def step(self):
        """-> (num_walkers, E_t, E_ref) of the yield."""
        o, m, n, dt = self.oracle, self.m, self.n, self.dt
        # --- branching (qmc_base/dmc.py:622-653), serial
        nw = 0
        ref = np.zeros(self.maxw, dtype=np.int64)
        for s in range(self.prev_nw):
            if nw >= self.maxw:
                break
            u = o.philox_uniform2(self.seed, self.slot0 + s, self.t, 0,
                                  STREAM_DMC_BRANCH)[0]
            x = np.exp(self.prev_logw[s]) + u
            self.branch_margin = min(self.branch_margin,
                                     float(abs(x - np.round(x))))
            clone = int(x)
            if not clone:
                continue
            a, nw = nw, min(nw + clone, self.maxw)
            ref[a:nw] = s
        # --- the move of every child and its weight
        next_confs = np.zeros_like(self.prev_confs)
        next_energy = np.zeros(self.maxw)
        next_logw = np.zeros(self.maxw)
        self.pair_margin = np.ones(self.maxw)
        for s in range(nw):
            p = ref[s]
            xi1, xi2 = normals(o, self.seed, self.slot0 + s, self.t, n)
            rows = []
            r_p = self.prev_confs[p, 0]
            r_n = move(o, m, r_p, dt, xi1, xi2, rows)
            self.pair_margin[s] = min(closest_pair(r, self.L) for r in rows)
            self.crossed += int((np.abs(r_n - np.mod(r_p, self.L)) >
                                 0.5 * self.L).sum())
            e_n, _, f_n = o.energy_drift(m, r_n)
            next_confs[s, 0], next_confs[s, 1] = r_n, f_n
            next_energy[s] = e_n
            # always the parent's energy
            next_logw[s] = -dt * ((e_n + self.prev_energy[p]) / 2 -
                                  self.ref_energy)
        if nw:
            self.min_pair_margin = min(self.min_pair_margin,
                                       float(self.pair_margin[:nw].min()))
        # --- the yielded state: the parents as cloned, unit weights
        self.confs = self.prev_confs[ref].copy()
        self.energy = self.prev_energy[ref].copy()
        self.cloning_ref = ref
        self.num_walkers = nw
        e_t, w_t = o.np_sum(self.energy[:nw]), float(nw)
        self.total_energy += e_t
        self.total_weight += w_t
        accum = self.total_energy / self.total_weight
        self.ref_energy = accum - self.kappa * np.log(w_t / self.target) / dt
        self.prev_confs, self.prev_energy = next_confs, next_energy
        self.prev_logw, self.prev_nw = next_logw, nw
        self.t += 1
        return nw, e_t, self.ref_energy
