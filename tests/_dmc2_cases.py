"""The cases of tests/test_gpu_dmc2_steps.py and their preconditions, from
the model parameters, numpy and the CPU oracle alone: no function takes a
device result.  tests/test_dmc2_host.py runs every precondition without a GPU.

One N per lane-group shape `dispatch_shape` (csrc/qmcwalk.hip) can pick for
`dmc_evolve2_kernel<G, P, PAD, ZC>` -- (G, P) from `pick_shape`, PAD = N != G P
(always on from P = 4), ZC = the position classifier (cutoff > 0.45 L):

  case        N    shape (G, P)  PAD  ZC   path of a stage
  dilute16    16   (16, 1)       -    -    general sum
  dilute9     9    (16, 1)       x    -    general sum
  boxz16      16   (16, 1)       -    x    general sum
  box32       32   (16, 2)       -    -    general sum
  offlat24    24   (16, 2)       x    -    general sum
  box48s32    48   (32, 2)       x    -    general sum (QMCWALK_SHAPE=32,2:
                                           the shape is a tuning knob only)
  offlat64    64   (64, 1)       -    -    sorted-64, exact
  offlat37    37   (64, 1)       x    -    sorted-64, ring of 37
  boxz64      64   (64, 1)       -    x    general sum, linear order
  dilute128   128  (64, 2)       -    -    sorted-128, exact
  hard100     100  (64, 2)       x    -    sorted-128, ring of 50 lanes
  defect101   101  (64, 2)       x    -    odd N: general sum at every stage
  boxz100     100  (64, 2)       x    x    general sum, consecutive slots
  box130      130  (64, 4)       x    -    general sum, four per lane
  offlat260   260  (64, 8)       x    -    general sum, eight per lane

The generic models and their time steps are those of tests/_generic_cases.py
(imported, not edited); 'box' is the unit-filling box of the rest of the
suite at the suite's DMC time step, 'boxz' the same with cutoff 0.48 L.  Every
case runs at its own time step and at 8 x that.

Seeds: the smallest seed >= 1 with which the RESTATEMENT of the case
(tests/_dmc2_restatement.py) meets the preconditions asserted in
`preconditions`; chosen on the host, no device result enters.  (The box at
N = 9, 16 keeps the identity table at its own time step with every seed below
12 -- walkers of nearly equal energy --: 'dilute' takes its place there.)
"""
import numpy as np

from . import _dmc2_restatement as r2
from . import _generic_cases as gc
from ._steps import (DMC_DT, DMC_KAPPA, DMC_MAXW, DMC_STEPS, DMC_W, dmc_start,
                     jittered_lattice)

MARGIN = 1e-9                   # a walker this close to a decision is left out
MULTS = (1, 8)                  # multiples of the case's own time step

# id: (model, N, cutoff / L, QMCWALK_SHAPE or None)
_SPEC = {
    'dilute16': ('dilute', 16, None, None),
    'dilute9': ('dilute', 9, None, None),
    'boxz16': ('box', 16, 0.48, None),
    'box32': ('box', 32, 0.25, None),
    'offlat24': ('offlat', 24, None, None),
    'box48s32': ('box', 48, 0.25, '32,2'),
    'offlat64': ('offlat', 64, None, None),
    'offlat37': ('offlat', 37, None, None),
    'boxz64': ('box', 64, 0.48, None),
    'dilute128': ('dilute', 128, None, None),
    'hard100': ('hard', 100, None, None),
    'defect101': ('defect', 101, None, None),
    'boxz100': ('box', 100, 0.48, None),
    'box130': ('box', 130, 0.25, None),
    'offlat260': ('offlat', 260, None, None),
}
IDS = list(_SPEC)
# (id, mult) -> seed; 1 where not listed
SEEDS = {('dilute16', 1): 2, ('dilute9', 1): 4, ('boxz16', 1): 5,
         ('box32', 1): 2, ('offlat24', 1): 4, ('offlat24', 8): 2,
         ('box48s32', 1): 2, ('box48s32', 8): 2, ('offlat37', 1): 5,
         ('offlat37', 8): 2, ('boxz64', 8): 2, ('dilute128', 8): 2,
         ('hard100', 8): 3, ('box130', 8): 2}


def case_of(cid):
    """-> ((model, N, L, c) as tests/_generic_cases.py has it, time step,
    forced shape)."""
    name, n, c, shape = _SPEC[cid]
    L = gc.supercell_size(name, n)
    if c is None:
        c = gc.MODELS[name][2]
    dt = gc.DMC_TIME_STEP.get(name, DMC_DT)
    return (name, n, L, c), dt, shape


def seed_of(cid, mult):
    return SEEDS.get((cid, mult), 1)


class Reference:
    """The restated population of a case over DMC_STEPS steps."""

    def __init__(self, oracle, cid, mult, seed):
        case, dt, self.shape = case_of(cid)
        _, n, L, c = case
        _, m = gc.oracle_model(oracle, case)
        self.case, self.seed = case, seed
        self.time_step = mult * dt
        self.pos0 = dmc_start(n, L, c * L, 7000 + n)
        pop = r2.Population(oracle, m, self.pos0, self.time_step, DMC_MAXW,
                            DMC_W, DMC_KAPPA, seed=seed)
        self.yields, self.tables = [], []
        self.left_out = 0       # walker-steps within MARGIN of a decision
        for _ in range(DMC_STEPS):
            if pop.prev_nw == 0:
                break
            y = pop.step()
            self.yields.append(y)
            self.tables.append(pop.cloning_ref[:y[0]].copy())
            self.left_out += int((pop.pair_margin[:y[0]] < MARGIN).sum())
        self.pop = pop

    def ok(self):
        """None, or the first precondition that fails."""
        if len(self.yields) < DMC_STEPS or self.yields[-1][0] == 0:
            return 'the population died out'
        if max(y[0] for y in self.yields) >= DMC_MAXW:
            return 'the population reached the cap'
        if not self.pop.branch_margin > MARGIN:
            return f'a marginal branching draw ({self.pop.branch_margin:.1e})'
        if self.left_out:
            return f'{self.left_out} walker-steps with a pair closer than ' \
                   f'{MARGIN:g} L'
        if self.pop.crossed < 1:
            return 'no particle crossed the boundary'
        if all(len(tab) == DMC_W and np.array_equal(tab, np.arange(DMC_W))
               for tab in self.tables):
            return 'every cloning table is the identity'
        return None


_cache = {}


def preconditions(oracle, cid, mult):
    """The restated population of the case (12 walkers from `dmc_start`, cap
    16, 8 steps at `mult` x the case's time step) -> Reference.  Asserted: the
    share of walkers left out is 0 -- no branching draw w + u within 1e-9 of
    an integer, no pair closer than 1e-9 L in any of the three rows a step
    evaluates --, the population neither dies out nor reaches the cap, >= 1
    particle crosses the box boundary, some cloning table is not the
    identity."""
    key = (cid, mult)
    if key not in _cache:
        _cache[key] = Reference(oracle, cid, mult, seed_of(cid, mult))
    ref = _cache[key]
    assert ref.ok() is None, (cid, mult, ref.ok())
    return ref


def lattice_rows(n, L, seed, walkers=DMC_W):
    """Walkers on jittered lattices: rows the sorted-row sums take."""
    rng = np.random.RandomState(seed)
    return np.array([jittered_lattice(rng, n, L) for _ in range(walkers)])
