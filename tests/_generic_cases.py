"""The cases of tests/test_gpu_generic_steps.py and their preconditions.

Everything here comes from the model parameters, numpy and the CPU oracle: no
function takes a device result.  The GPU tests call the precondition
functions before they compare the device, tests/test_generic_steps_host.py
runs them for every case without a GPU.  The oracle's trajectories are
computed once per case and shared (they are not modified)."""
from fractions import Fraction
from math import ceil, pi

import numpy as np

from ._steps import (DMC_MAXW, DMC_STEPS, DMC_W, VMC_SPREAD, VMC_W,
                     VMC_YIELDS, dmc_start, far_partner_distances,
                     general_path_yields, oracle_dmc_run, oracle_vmc_chains,
                     start_rows, takes_sorted_rows)

FAR_MIN = 1e-9                  # no far-partner distance closer to L - rm, of L

# name: (Spec keywords, filling N / L, cutoff / L)
MODELS = {
    # non-integer L, half-integer number of lattice periods, leading loop long
    'offlat': (dict(lattice_depth=30, lattice_ratio=2.5,
                    interaction_strength=0.7), 24 / 17.5, 0.41),
    # ratio < 1, short leading loop
    'dilute': (dict(lattice_depth=37, lattice_ratio=0.6,
                    interaction_strength=7.5), 1 / 1.1, 0.12),
    # no one-body factor; L - rm = 0.56 L: uniform rows fail the far-partner
    # check
    'free': (dict(lattice_depth=0, lattice_ratio=1,
                  interaction_strength=0.4), 1 / 0.93, 0.44),
    # nearly every pair long, trailing loop only
    'hard': (dict(lattice_depth=80, lattice_ratio=2.3,
                  interaction_strength=25), 1 / 1.317, 0.03),
    # per-particle one-body constants
    'defect': (dict(lattice_depth=5 * pi ** 2, lattice_ratio=0.5,
                    interaction_strength=3, num_defects=4,
                    defect_magnitude=2 * pi ** 2), 20 / 24, 0.23),
    # the unit-filling box of the rest of the suite (part 4 only)
    'box': (dict(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                 interaction_strength=2), 1.0, 0.25),
}

# every ring variant of eval_sorted64 / eval_sorted128, exact and padded, and
# the odd-N (64, 2) shape (101), which has no sorted rows
SIZES = (37, 48, 64, 66, 100, 101, 128)
MORE_SIZES = (33, 63, 126)      # 'offlat' and 'hard' as well
STEP_MODELS = ('offlat', 'dilute', 'free', 'hard', 'defect')


def supercell_size(name, n):
    """L = round(N / filling, 3).  'defect': `Spec` wants the number of
    lattice sites ceil(L) to be a multiple of num_defects; where it is not, L
    is the nearest value on the same 0.001 grid that is -- the multiple below
    itself, or 0.001 past the multiple above less one."""
    kw, filling, _ = MODELS[name]
    L = round(n / filling, 3)
    nd = kw.get('num_defects', 0)
    if nd and ceil(L) % nd:
        below = float(ceil(L) // nd * nd)
        above = round(below + nd - 1 + 0.001, 3)
        L = below if L - below <= above - L else above
    return L


# (model, N, L, c): parts 1-3
CASES = [(name, n, supercell_size(name, n), MODELS[name][2])
         for name in STEP_MODELS
         for n in SIZES + (MORE_SIZES if name in ('offlat', 'hard') else ())]


def case_id(case):
    return f'{case[0]}{case[1]}'


IDS = [case_id(c) for c in CASES]

# Philox seeds and DMC time steps, chosen with the oracle alone (no device
# result enters), by the rule of tests/test_gpu_zclass_steps.py: the smallest
# seed >= 1 with which the oracle's case meets the preconditions asserted
# below.  The DMC time step of a model: the smallest of {5e-4, 1e-3, 2e-3}
# with which every size of the model finds such a seed below 10.  (At 5e-4
# 'offlat' at N = 33, 63 keeps the identity table with every seed below 10.
# 'free' -- walkers of nearly equal energy, weights within a few per cent of
# 1 -- rarely branches at all: at N = 37 no seed below 10 does at any of the
# three steps, so it gets the largest, and N = 37 the first seed that does.)
# (VMC: seed 1 gives 3-22 crossings and 19-120 accepted steps of 138 in every
# case)
VMC_SEEDS = {cid: 1 for cid in IDS}
DMC_TIME_STEP = dict(offlat=1e-3, dilute=5e-4, free=2e-3, hard=5e-4,
                     defect=5e-4)
DMC_SEEDS = dict({cid: 1 for cid in IDS}, **{
    'offlat37': 5, 'offlat66': 2, 'offlat101': 6, 'offlat128': 4,
    'offlat33': 2, 'offlat63': 2,
    'dilute37': 2, 'dilute64': 4,
    'free37': 24, 'free48': 2, 'free100': 4, 'free128': 2,
    'hard100': 2, 'hard126': 3,
    'defect37': 2, 'defect64': 2, 'defect100': 2})


def make_spec(name, n, L, cutoff):
    from phd_qmclib_amd.mrbp_qmc import Spec
    return Spec(boson_number=n, supercell_size=L, tbf_contact_cutoff=cutoff,
                **MODELS[name][0])


_cache = {}


def oracle_model(oracle, case):
    key = ('model',) + tuple(case)
    if key not in _cache:
        name, n, L, c = case
        cfc = make_spec(name, n, L, c * L).cfc_spec
        m = oracle.model_from_cfc(cfc)
        assert float(m.tbf_contact_cutoff) == c * L
        assert float(m.supercell_size) == L
        _cache[key] = (cfc, m)
    return _cache[key]


class VmcReference:
    """The oracle's chains of a case and what part 2 derives from the rows
    they evaluate."""

    def __init__(self, oracle, case, seed):
        name, n, L, c = case
        _, m = oracle_model(oracle, case)
        self.seed = seed
        self.pos0 = start_rows(n, L, c * L, 7000 + n)
        (self.stat, self.energy, self.wf, self.pos, self.crossings,
         self.rows) = oracle_vmc_chains(oracle, m, self.pos0, VMC_SPREAD,
                                        seed, VMC_YIELDS, rows=True)
        self.accepted = int(self.stat[1:].sum())
        # general[t, chain]: the yield leaves the sorted-row path; trips[t,
        # chain] of the exact sort before it (-1: it gave up)
        per_chain = [general_path_yields(self.rows[:, w], self.stat[:, w], n,
                                         L, c * L) for w in range(VMC_W)]
        self.general = np.array([g for g, _ in per_chain]).T
        self.trips = np.array([t for _, t in per_chain]).T
        # ... for the far partner alone
        self.far_fails = np.array([[not takes_sorted_rows(r, n, L, c * L)
                                    for r in rows_t] for rows_t in self.rows])
        if n > 64 and n % 2:
            self.far_margin = None      # (no far-partner test is reached)
        else:
            self.far_margin = min(
                float(np.abs(far_partner_distances(r, n, L) -
                             (L - c * L)).min())
                for rows_t in self.rows for r in rows_t) / L

    def ok(self):
        """None, or the first precondition that fails."""
        if self.crossings < 3:
            return f'{self.crossings} crossings of the box boundary'
        if not 0 < self.accepted < VMC_W * (VMC_YIELDS - 1):
            return f'{self.accepted} accepted: one outcome only'
        if self.far_margin is not None and self.far_margin < FAR_MIN:
            return f'a far partner {self.far_margin:.1e} L from L - rm'
        return None


def vmc_preconditions(oracle, case):
    """The oracle's chains of the case (6 chains from `start_rows`, 24 yields,
    move_spread 0.6) -> VmcReference.  Asserted: >= 3 crossings of the box
    boundary; both accept outcomes after yield 0; no evaluated row has a
    far-partner distance within 1e-9 L of L - rm; at N = 101 every yield of
    every chain is on the general path (the static test `(n & 1) == 0`); the
    'free' model at N = 64, 128 has yields on both paths."""
    key = ('vmc',) + tuple(case)
    if key not in _cache:
        _cache[key] = VmcReference(oracle, case, VMC_SEEDS[case_id(case)])
    ref = _cache[key]
    name, n = case[0], case[1]
    assert ref.ok() is None, ref.ok()
    count = int(ref.general.sum())
    if n > 64 and n % 2:
        assert count == VMC_W * VMC_YIELDS, 'no sorted rows at an odd N'
    if name == 'free' and n in (64, 128):
        assert 0 < count < VMC_W * VMC_YIELDS, count
        # N = 128: chains leave the sorted path and return to it (at N = 64
        # the uniform start rows stay off it for all 24 yields and the
        # spread ones on it)
        if n == 128:
            assert np.any(ref.general[1:] & ~ref.general[:-1]) and \
                np.any(~ref.general[1:] & ref.general[:-1]), \
                ref.general.sum(0)
    return ref


class DmcReference:
    """The oracle's population of a case."""

    def __init__(self, oracle, case, seed, time_step):
        name, n, L, c = case
        _, m = oracle_model(oracle, case)
        self.seed, self.time_step = seed, time_step
        self.pos0 = dmc_start(n, L, c * L, 7000 + n)
        self.tables = []
        self.failed = None
        try:
            self.orc, self.yields, self.margin, self.crossed = oracle_dmc_run(
                oracle, m, self.pos0, seed, time_step, tables=self.tables)
        except AssertionError:
            self.failed = 'the population reached the cap'

    def branches(self):
        """A step whose cloning table is not the identity."""
        return any(len(tab) != DMC_W or
                   not np.array_equal(tab, np.arange(DMC_W))
                   for tab in self.tables)

    def ok(self):
        if self.failed:
            return self.failed
        if not self.margin > 1e-6:
            return f'a marginal branching draw ({self.margin:.1e})'
        if max(y[0] for y in self.yields) >= DMC_MAXW:
            return 'the population reached the cap'
        if self.crossed < 1:
            return 'no particle crossed the boundary'
        if not self.branches():
            return 'every cloning table is the identity'
        return None


def dmc_preconditions(oracle, case):
    """The oracle's population of the case (12 walkers from `dmc_start`, cap
    16, 8 steps at the model's time step) -> DmcReference.  Asserted: no
    branching draw w + u within 1e-6 of an integer; the population below the
    cap; >= 1 particle crosses the box boundary; the cloning table of some
    step is not the identity."""
    key = ('dmc',) + tuple(case)
    if key not in _cache:
        _cache[key] = DmcReference(oracle, case, DMC_SEEDS[case_id(case)],
                                   DMC_TIME_STEP[case[0]])
    ref = _cache[key]
    assert ref.ok() is None, ref.ok()
    assert len(ref.yields) == DMC_STEPS
    return ref


# ---------------------------------------------------------------------------
# part 4: production against series
# ---------------------------------------------------------------------------

LEAN_MODELS = ('box', 'offlat')
LEAN_CUTOFF = 0.25
# every shape without a fused loop, padded and exact, then the shapes with
# one.  N = 16, 32 -- the exact (16, 1) and (16, 2) shapes -- are the sizes at
# which a compiler left to contract z + d does so in the sine-classifier
# kernels (the code of every other steady kernel here comes out the same,
# instruction for instruction, with and without the `fp contract(off)` block:
# their d is not always the product); tests/test_gpu_zclass_steps.py pins them
# on the box at spread 0.6 alone.
LEAN_SIZES = (9, 16, 24, 32, 130, 256, 300, 512, 48, 64, 99, 128)
LEAN_FLOAT_SIZES = (48, 64, 100, 128)
LEAN_BLOCKS = (17, 66)


def lean_spreads(n, L):
    """Neither product vmc_move_unit * move_spread is exact (0.125, the
    spread of the rest of the suite, is a power of two)."""
    return (0.6, 0.37 * L / n)


def lean_case(name, n):
    L = supercell_size(name, n)
    return (name, n, L, LEAN_CUTOFF)


def product_rounds(oracle, spread):
    """vmc_move_unit * spread is not exact: a fused multiply-add z + unit *
    spread differs from the sum with the rounded product."""
    units = [oracle.vmc_move_unit(w0)
             for w0 in (1, 0x12345678, 0x9abcdef0, 0xffffffff)]
    return any(Fraction(u) * Fraction(spread) != Fraction(u * spread)
               for u in units)
