"""The cases of tests/test_gpu_dmc2_float_steps.py -- the second-order DMC step
(`propagator='quadratic'`) on an engine with the float pair loop (`fast_math`)
-- and their preconditions, from the model parameters, numpy, the fp64
restatement (tests/_dmc2_restatement.py) and the CPU oracle alone: no function
takes a device result.  tests/test_dmc2_float_host.py runs every precondition
without a GPU.

`LaunchEvolve2` (csrc/qmcwalk.hip) picks `dmc_evolve2_kernel<G, P, PAD, ZC,
float>` on such an engine at the six shapes csrc/qmc_inst.h instantiates
(ZC = false throughout: the float loop exists with the sine classifier only):

  N     instantiation <G, P, PAD>  path of a stage               zero-move tag
  64    <64, 1, false>             sorted-64, exact              box64
  37    <64, 1, true>              sorted-64, ring of 37         box37, box48
  128   <64, 2, false>             sorted-128, exact             box128
  100   <64, 2, true>              sorted-128, ring of 50 lanes  deep100, box100,
                                                                 box126
  101   <64, 2, true>              odd N: the general float sum at all three
                                   stages, counted
  130   <64, 4, true>              general float sum             (oracle rows)
  260   <64, 8, true>              general float sum             (oracle rows)

The real steps run on the unit-filling 'box' model of tests/_generic_cases.py
(`gc.lean_case('box', n)`) at the time step of the float DMC test, 1e-3, and
at 8e-3: 12 walkers (cap 16, target 12, kappa 0.5), every one a jittered
lattice rotated by its own uniform offset modulo L, so particles sit next to
the seam; two steps, so that the yielded state holds the children of step 0
-- moved once from exact parents, E and F from the third stage.

What a float drift may do to a child.  With F off by TOL_DRIFT max|F| at
every stage, R_m = R_a + dt F(R_a) is off by dt TOL_DRIFT fa, F(R_m) by its
own TOL_DRIFT fm plus ||J(R_m)|| times that, and R_b = R_a + 2 dt F(R_m) --
hence R' -- by

    2 dt TOL_DRIFT (fm + kappa fa),   kappa = dt ||J(R_m)||_inf

to first order; B_s is twice that (the second-order terms) plus 4 ulp of L
(the wraps).  J: the Jacobian of the oracle's drift by forward differences
(N + 1 evaluations; the same N + 1 evaluations at R' give dE / dz_i and
J(R')).  The energy of a child may then differ by TOL_ENERGY max(1, |E|) +
G_s B_s, G_s = sum_i |dE / dz_i| at R', its drift by TOL_DRIFT max|F| +
||J(R')||_inf B_s.  A walker whose B_s exceeds 1e-2 of the closest pair
distance over its three rows is LEFT OUT of the value comparisons (the pair
drift flips sign at contact: the linearisation means nothing there); it still
counts in the populations.

Seeds: the smallest Philox seed >= 1 with which the restated case meets every
precondition of `Reference.ok`; SEEDS holds them and the host test asserts
that every smaller seed fails.  (Staying below the cap is not one of them: at
N = 260 and 8e-3 the second step of every seed below 40 fills all 16 slots.
The serial rule cut at the cap is what restatement and device both apply --
tests/test_gpu_dmc_tiles.py pins it -- and the branching margin keeps every
clone count out of a float energy's reach.)
"""
import numpy as np

from . import _dmc2_restatement as r2
from . import _generic_cases as gc
from ._steps import (far_partner_distances, jittered_lattice, sort_slots,
                     takes_sorted_rows)
from .test_gpu_fastmath import TOL_DRIFT, TOL_ENERGY

SIZES = (64, 37, 128, 100, 101, 130, 260)
SORTED_SIZES = (64, 37, 128, 100)       # every stage on the sorted rows
TIME_STEPS = (1e-3, 8e-3)
W, MAXW, KAPPA, STEPS = 12, 16, 0.5, 2
LEFT_OUT_CAP = {1e-3: 0, 8e-3: 2}       # walkers of 12
LEFT_OUT_RATIO = 1e-2                   # B_s of the closest pair distance
FAR_MIN = 1e-6                          # far partner from L - rm, of L
FD_STEP = 1e-6                          # forward differences
CASES = [(n, dt) for n in SIZES for dt in TIME_STEPS]

# (N, time step) -> Philox seed; see `find_seed`
SEEDS = {case: 1 for case in CASES}
SEEDS[(260, 1e-3)] = 3          # (seeds 1, 2: no particle crosses the seam)

# golden tag of the zero-move step -> the instantiation it launches
ZERO_MOVE_SHAPE = {'box64': (64, 1, False), 'box37': (64, 1, True),
                   'box48': (64, 1, True), 'box128': (64, 2, False),
                   'deep100': (64, 2, True), 'box100': (64, 2, True),
                   'box126': (64, 2, True)}


# the sweep cases (tests/_vmc_sweep_cases.py) run on a fast-math engine
SWEEP_CASES = ('box64', 'box128', 'hard130')


def case_id(case):
    return f'n{case[0]}-dt{case[1]:g}'


def start_rows(n, L):
    """12 jittered lattices, each rotated by its own uniform offset."""
    rng = np.random.RandomState(9200 + n)
    rows = []
    for _ in range(W):
        row = jittered_lattice(rng, n, L)
        rows.append(np.mod(row + L * rng.random_sample(), L))
    rows = np.array(rows)
    assert np.all((rows >= 0.0) & (rows < L))
    return rows


def cyclic_order(row):
    """The particle labels in ascending position, turned so that label 0
    comes first: what a rotation of the row leaves alone."""
    o = np.argsort(row, kind='stable')
    k = int(np.nonzero(o == 0)[0][0])
    return np.concatenate([o[k:], o[:k]])


def energy_drift_rows(oracle, m, rows):
    """`oracle.energy_drift` of every row -> (energy [K], drift [K, N]):
    the oracle's own batch entry (orc_dmc_prepare, the same C function per
    row, rows shared among its threads)."""
    import ctypes as C
    rows = np.asarray(rows, dtype=np.float64)
    k, n = rows.shape
    confs = np.zeros((k, 2, n))
    confs[:, 0] = rows
    energy = np.zeros(k)
    as_dp = C.POINTER(C.c_double)
    oracle.lib().orc_dmc_prepare(C.byref(m), k, confs.ctypes.data_as(as_dp),
                                 energy.ctypes.data_as(as_dp),
                                 min(16, oracle.max_threads()))
    return energy, confs[:, 1].copy()


def energy_gradient_and_jacobian(oracle, m, row):
    """Forward differences of the oracle's energy and drift at `row`, N + 1
    evaluations -> (dE / dz [N], J [N, N]: J[i, j] = dF_i / dz_j)."""
    L = float(m.supercell_size)
    n = len(row)
    rows = np.tile(row, (n + 1, 1))
    j = np.arange(n)
    rows[j + 1, j] = row + FD_STEP
    h = rows[j + 1, j] - row                # the steps as represented
    rows[j + 1, j] = np.mod(rows[j + 1, j], L)
    e, f = energy_drift_rows(oracle, m, rows)
    return (e[1:] - e[0]) / h, ((f[1:] - f[0]) / h[:, None]).T


def inf_norm(jac):
    return float(np.abs(jac).sum(axis=1).max())


class Reference:
    """Two steps of the restated population of a case under one Philox seed,
    with the three rows every child evaluates rebuilt from the same draws."""

    def __init__(self, oracle, case, seed):
        n, dt = case
        self.case, self.seed, self.n, self.time_step = case, seed, n, dt
        self.model_case = gc.lean_case('box', n)
        _, m = gc.oracle_model(oracle, self.model_case)
        self.oracle, self.m = oracle, m
        L = self.L = self.model_case[2]
        rm = self.model_case[3] * L
        self.pos0 = start_rows(n, L)
        pop = r2.Population(oracle, m, self.pos0, dt, MAXW, W, KAPPA,
                            seed=seed)
        self.e_max = float(np.abs(pop.prev_energy[:W]).max())
        # per step: [(parent, R_p, R_a, R_m, R')] of every child
        self.rows, self.yields, self.tables = [], [], []
        self.order_changed = 0
        self.far_margin = 1.0
        self.sorted_rows = True
        # the slot order a parent's row was left in (set_state sorts the rows)
        order = [np.argsort(r, kind='stable') for r in self.pos0]
        for t in range(STEPS):
            parents = pop.prev_confs[:, 0].copy()
            y = pop.step()
            nw = y[0]
            ref = pop.cloning_ref[:nw].copy()
            self.yields.append(y)
            self.tables.append(ref)
            step_rows, new_order = [], []
            for s in range(nw):
                xi1, xi2 = r2.normals(oracle, seed, s, t, n)
                three = []
                r_n = r2.move(oracle, m, parents[ref[s]], dt, xi1, xi2, three)
                # (the rebuilt move IS the population's)
                assert np.array_equal(r_n, pop.prev_confs[s, 0])
                r_p = np.mod(parents[ref[s]], L)
                step_rows.append((int(ref[s]), r_p) + tuple(three))
                self.order_changed += int(
                    not np.array_equal(cyclic_order(r_p),
                                       cyclic_order(three[0])) or
                    not np.array_equal(cyclic_order(three[1]),
                                       cyclic_order(three[2])))
                o = order[ref[s]]
                for r in three:
                    if n in SORTED_SIZES:
                        d = far_partner_distances(r, n, L)
                        self.far_margin = min(
                            self.far_margin,
                            float(np.abs(d - (L - rm)).min()) / L)
                        trips, o = sort_slots(r, o)
                        self.sorted_rows &= trips is not None and \
                            takes_sorted_rows(r, n, L, rm)
                new_order.append(o)
            self.rows.append(step_rows)
            order = new_order
            self.e_max = max(self.e_max,
                             float(np.abs(pop.prev_energy[:nw]).max()))
        self.pop = pop
        self.branch_floor = 4 * dt * TOL_ENERGY * max(1.0, self.e_max)
        self._bounds = None

    # ---- what needs the Jacobians: once per reference ----------------------
    def bounds(self):
        """Per child s of step 0 -> dict of arrays [nw0]: fa, fm, kappa, B, G
        (sum |dE / dz_i| at R'), JR (||J(R')||_inf), pair (the closest pair
        distance over the three rows, absolute), left_out."""
        if self._bounds is None:
            o, m, dt = self.oracle, self.m, self.time_step
            out = {k: [] for k in ('fa', 'fm', 'kappa', 'B', 'G', 'JR',
                                   'pair')}
            for _, _, r_a, r_m, r_n in self.rows[0]:
                fa = float(np.abs(o.energy_drift(m, r_a)[2]).max())
                fm = float(np.abs(o.energy_drift(m, r_m)[2]).max())
                _, jm = energy_gradient_and_jacobian(o, m, r_m)
                grad, jn = energy_gradient_and_jacobian(o, m, r_n)
                kappa = dt * inf_norm(jm)
                out['fa'].append(fa)
                out['fm'].append(fm)
                out['kappa'].append(kappa)
                out['B'].append(2 * 2 * dt * TOL_DRIFT * (fm + kappa * fa) +
                                4 * np.spacing(self.L))
                out['G'].append(float(np.abs(grad).sum()))
                out['JR'].append(inf_norm(jn))
                out['pair'].append(self.L * min(r2.closest_pair(r, self.L)
                                                for r in (r_a, r_m, r_n)))
            out = {k: np.array(v) for k, v in out.items()}
            out['left_out'] = out['B'] > LEFT_OUT_RATIO * out['pair']
            self._bounds = out
        return self._bounds

    def expected_general(self):
        """What `general_path_walkers()` reads after the block, or None where
        the shape does not count (four and eight particles per lane)."""
        if self.n in SORTED_SIZES:
            return 0
        if self.n == 101:
            return 3 * sum(y[0] for y in self.yields)
        return None

    def ok(self):
        """None, or the first precondition that fails (the cheap ones
        first)."""
        n, dt = self.case
        if min(y[0] for y in self.yields) == 0:
            return 'the population died out'
        if not self.pop.branch_margin > self.branch_floor:
            return f'a marginal branching draw ({self.pop.branch_margin:.1e}' \
                   f' <= {self.branch_floor:.1e})'
        if self.pop.crossed < 1:
            return 'no particle crossed the boundary'
        if dt == TIME_STEPS[1] and self.order_changed < 1:
            return 'no walker changed its cyclic particle order'
        if n in SORTED_SIZES:
            if not self.sorted_rows:
                return 'an evaluated row leaves the sorted path'
            if not self.far_margin > FAR_MIN:
                return f'a far partner {self.far_margin:.1e} L from L - rm'
        left = int(self.bounds()['left_out'].sum())
        if left > LEFT_OUT_CAP[dt]:
            return f'{left} walkers left out'
        return None


_cache = {}


# ---------------------------------------------------------------------------
# the linear float step at the masked shapes
# ---------------------------------------------------------------------------

# `test_dmc_float_steps_follow_the_oracle` (tests/test_gpu_fastmath_steps.py)
# at N = 130, 260 on the box: its own population and its own rule -- on the
# oracle no branching draw of the two steps within 1e-4 of an integer, the
# population below the cap; the smallest such seed >= 1
LINEAR_SIZES = (130, 260)
LINEAR_W, LINEAR_MAXW, LINEAR_DT, LINEAR_MARGIN = 64, 96, 1e-3, 1e-4
LINEAR_SEEDS = {130: 1, 260: 1}


def linear_start_rows(n, L):
    """(the rows that test draws)"""
    from .test_gpu_fastmath_steps import jittered_rows
    return jittered_rows(np.random.RandomState(20261019), LINEAR_W, n, L)


def linear_margin(oracle, n, seed):
    """-> the smallest |w + u - round(w + u)| over the two steps of the
    oracle's linear population, or None where it reaches the cap."""
    key = ('linear', n, seed)
    if key not in _cache:
        case = gc.lean_case('box', n)
        _, m = gc.oracle_model(oracle, case)
        orc = oracle.DmcEnsemble(m, linear_start_rows(n, case[2]), LINEAR_DT,
                                 LINEAR_MAXW, LINEAR_W, KAPPA, seed=seed)
        margin, weights = 1.0, np.ones(LINEAR_W)
        for t in range(2):
            u = np.array([oracle.philox_uniform2(seed, s, t, 0,
                                                 r2.STREAM_DMC_BRANCH)[0]
                          for s in range(len(weights))])
            x = weights + u
            margin = min(margin, float(np.abs(x - np.round(x)).min()))
            y = orc.step()
            if not int(np.floor(x).sum()) == y.num_walkers < LINEAR_MAXW:
                margin = None
                break
            weights = orc.bufs['next_weight'][:y.num_walkers].copy()
        _cache[key] = margin
    return _cache[key]


def linear_seed_ok(oracle, n, seed):
    margin = linear_margin(oracle, n, seed)
    return margin is not None and margin > LINEAR_MARGIN


def reference(oracle, case, seed):
    key = (case, seed)
    if key not in _cache:
        _cache[key] = Reference(oracle, case, seed)
    return _cache[key]


def find_seed(oracle, case, limit=40):
    for seed in range(1, limit):
        if reference(oracle, case, seed).ok() is None:
            return seed
    raise AssertionError(f'{case}: no seed below {limit}')


def preconditions(oracle, case):
    """The restated population of the case under its seed of SEEDS ->
    Reference (computed once, shared, not modified), every precondition
    asserted."""
    ref = reference(oracle, case, SEEDS[case])
    assert ref.ok() is None, (case, ref.ok())
    return ref
