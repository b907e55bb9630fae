"""Real VMC and DMC steps of the sorted-row stepping kernels -- the kernels
bench.py times -- on generic models, against the CPU oracle, and the
production VMC block against the series kernel at spreads whose product
vmc_move_unit * move_spread rounds.

Every other multi-step trajectory of the sine-classifier kernels runs on the
unit-filling box (depth 5 pi^2, ratio 1, coupling 2, L = N, cutoff L / 4) at
move_spread 0.125, where that product is exact; random models reached the
sorted rows only through the forced first yield and a zero-move DMC step.
What happens BETWEEN two pair sums was pinned on one model: `wrap_box` on a
non-integer L, `sort_lanes64` / `sort_rows128` with `anchor_seam*` after real
displacements on rings of every length, `far_partner_ok*` with L - rm anywhere
between 0.56 L and 0.97 L, the one-body table across a wrap in a supercell that
is not a whole number of lattice periods, the carried energy and log|psi|,
`vmc_accept_thresholds` and the register-resident row of the fused loop, the
DMC drift step, the spare normals, the weights and branching.

Reference: the CPU oracle (`oracle.VmcChain`, `oracle.DmcEnsemble`) on the
same Philox streams; it is pinned bit for bit to the reference implementation
on trajectories of the off-lattice and the defect model
(tests/test_oracle_golden.py).

Models (tests/_generic_cases.py), L = round(N / filling, 3), cutoff c L:

  name    depth  ratio  coupling  filling   c
  offlat  30     2.5    0.7       24/17.5   0.41  non-integer L, half-integer
                                                  number of lattice periods
  dilute  37     0.6    7.5       1/1.1     0.12  ratio < 1, short leading loop
  free    0      1      0.4       1/0.93    0.44  no one-body factor; L - rm =
                                                  0.56 L: uniform rows fail the
                                                  far-partner check
  hard    80     2.3    25        1/1.317   0.03  nearly every pair long
  defect  5pi^2  0.5    3         20/24     0.23  num_defects 4, magnitude
                                                  2 pi^2: per-particle one-body
                                                  constants

all five at N = 37, 48, 64, 66, 100, 101, 128, 'offlat' and 'hard' at 33, 63,
126 as well: every ring variant of `eval_sorted64` / `eval_sorted128`, exact
and padded, and the odd-N (64, 2) shape, which has no sorted rows.
`Spec` wants ceil(L) of 'defect' to be a multiple of its 4 defects and refuses
L = 1.2 N at N = 37, 48, 64, 101, 128: L moved to the nearest accepted value
on the 0.001 grid -- 44.0, 59.001, 76.0, 120.0, 155.001.

1. VMC real steps: 6 chains from `start_rows`, 24 yields, move_spread 0.6,
   series kernel, against `oracle.VmcChain` (accept series through
   `explain_flips`; energy, log|psi| of every yield and the final positions
   at 1e-9); the production block (one forced launch + one fused launch of 23
   yields) bit-equal to the series run.
2. The path taken is the path claimed: the counter of walker evaluations that
   left the sorted rows equals the number of (chain, yield) pairs whose
   evaluated row -- the oracle's proposal -- fails the once-per-walker
   condition restated in numpy (`_steps.far_partner_distances`).
3. DMC real steps: 12 walkers, cap 16, 8 steps, at a time step per model at
   which the oracle's population branches, against `oracle.DmcEnsemble`.
4. Production equals series, bit for bit, at move_spread 0.6 and 0.37 L / N:
   the box and 'offlat' (cutoff L / 4) at N = 9, 16, 24, 32, 130, 256, 300,
   512 and on the fused shapes 48, 64, 99, 128, blocks of 17 and 66 yields,
   two in a row; the float variant at N = 48, 64, 100, 128.  On a library
   built without the `fp contract(off)` block around z + d in
   `vmc_step_kernel` this part fails at N = 16 and 32, both models, both
   block lengths, and nowhere else: the compiler contracts only where d is always
   the product -- the steady kernels of the exact shapes without a fused loop
   -- and every other steady kernel of the sine classifier, the fused ones
   included, comes out instruction for instruction the same.

Every precondition is a function of tests/_generic_cases.py that takes no
device result; tests/test_generic_steps_host.py runs them without a GPU.
Every test prints its worst deviation as a fraction of its tolerance (`-s`);
DESIGN.md section 2 quotes one run.
"""
import numpy as np
import pytest

from . import _generic_cases as gc
from ._generic_cases import CASES, IDS, case_id
from ._steps import (DMC_KAPPA, DMC_MAXW, DMC_STEPS, DMC_W, VMC_SPREAD, VMC_W,
                     VMC_YIELDS, report, start_rows)
from ._traj import explain_flips, first_difference
from .test_gpu_parity import close, worst

pytestmark = pytest.mark.gpu

RTOL = 2e-11                    # the suite's double-path tolerance


def say(part, cid, figures):
    report(part, cid, figures, module='generic')


@pytest.fixture(scope='module')
def engines(oracle):
    """(case, fast_math) -> engine; the float variant must be granted where
    it is asked for."""
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(case, fast_math=False):
        key = (tuple(case), fast_math)
        if key not in cache:
            assert case[3] <= 0.44, 'the sine classifier'
            cfc, _ = gc.oracle_model(oracle, case)
            cache[key] = ModelEngine(cfc, fast_math=fast_math)
            assert cache[key].fast_math is fast_math
        return cache[key]
    yield get
    for eng in cache.values():
        eng.close()


def vmc_block(eng, pos0, spread, seed, blocks, series):
    """`blocks` (yields each) on a fresh ensemble -> per block (output, state,
    counter of the general path)."""
    from phd_qmclib_amd.engine import VmcEnsemble
    v = VmcEnsemble(eng, pos0.shape[0], spread, rng_seed=seed)
    runs = []
    try:
        v.set_state(pos0)
        for b in blocks:
            eng.general_path_walkers(reset=True)
            out = v.run_block(b, series=series)
            runs.append((out, v.get_state(),
                         eng.general_path_walkers(reset=True)))
    finally:
        v.close()
    return runs


@pytest.fixture(scope='module')
def vmc_runs(oracle, engines):
    """The device's series and production block of a case, run once for parts
    1 and 2."""
    cache = {}

    def get(case):
        if case not in cache:
            ref = gc.vmc_preconditions(oracle, case)
            eng = engines(case)
            cache[case] = tuple(
                vmc_block(eng, ref.pos0, VMC_SPREAD, ref.seed, [VMC_YIELDS],
                          series)[0] for series in (True, False))
        return cache[case]
    return get


# ---------------------------------------------------------------------------
# 1. VMC real steps
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_vmc_real_steps_follow_the_oracle(vmc_runs, oracle, case):
    """6 chains, 24 yields with move_spread 0.6: accept / reject series equal
    (a differing chain must show a rounding-level Metropolis margin, at most
    one: tests/_traj.py), energy and log|psi| of every yield at 1e-9, final
    positions in particle order at 1e-9 (minimum image); the production block
    from the same start: state bit-equal to the series run's, equal
    acceptance, equal counter of the general path, block sum = sum of the
    series."""
    cid = case_id(case)
    _, n, L, _ = case
    ref = gc.vmc_preconditions(oracle, case)
    _, m = gc.oracle_model(oracle, case)
    (out, state, general), (lean, lean_state, lean_general) = vmc_runs(case)
    same = explain_flips(oracle, m, ref.pos0, VMC_SPREAD, ref.seed,
                         out['move_stat'], ref.stat)
    dev = dict(energy=worst(out['energy'][:, same], ref.energy[:, same]) / 1e-9,
               wf=worst(out['wf_abs_log'][:, same], ref.wf[:, same]) / 1e-9)
    dz = np.abs(np.mod(state[0][same], L) - ref.pos[same])
    dev['pos'] = float(np.minimum(dz, L - dz).max()) / 1e-9
    say('part1', cid, dict(
        dev, crossings=ref.crossings, accepted=ref.accepted,
        pos_bit_equal=bool(np.array_equal(np.mod(state[0], L), ref.pos))))
    assert dev['energy'] <= 1.0 and dev['wf'] <= 1.0 and dev['pos'] <= 1.0, dev
    assert close(state[1][same], ref.wf[-1, same], 1e-9)
    # the production path
    for a, b in zip(lean_state, state):
        assert np.array_equal(a, b)
    assert np.array_equal(lean['num_accepted'], out['num_accepted'])
    assert np.array_equal(out['num_accepted'], out['move_stat'].sum(0))
    assert close(lean['sum_energy'], out['energy'].sum(0),
                 rtol=1e-12 * VMC_YIELDS)
    assert lean_general == general


# ---------------------------------------------------------------------------
# 2. the path taken is the path claimed
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_general_path_counter_is_the_restated_condition(vmc_runs, oracle,
                                                        case):
    """`vmc_step_kernel` counts a walker evaluation (one per chain and yield)
    when `fast` is false and the model interacts (`_steps.general_path_yields`
    restates it): N is odd on the (64, 2) shape, or the exact sort
    (`sort_lanes64` / `sort_rows128`, restated pass by pass in
    `_steps.sort_slots`) gives up at its bound, or the ascending row fails
    `far_partner_ok64` / `_ring` / `128` / `_ring128`.  The rows are the
    oracle's: the start row at yield 0, its proposal afterwards, none of them
    within 1e-9 L of the edge of the far-partner condition
    (`vmc_preconditions`).  A chain that left the oracle at a marginal
    Metropolis test (part 1) evaluates other rows from there on: its later
    yields bound the count instead of entering it.

    Found here: 'hard' at N = 100, chain 4 (two particles start within 1e-3
    of 0), yield 16 -- three particles leave through z = 0 in one step,
    `anchor_seam_rows` turns the row the wrong way trip after trip (it takes
    "the last slot is below the second" for a particle that left through
    z = L) and `sort_rows128` gives up after its 66 trips.  The general pair
    sum evaluates the walker, correctly (part 1); the counter shows it, and
    the restated sort gives up on the same row."""
    cid = case_id(case)
    n = case[1]
    ref = gc.vmc_preconditions(oracle, case)
    (out, _, general), _ = vmc_runs(case)
    lo = hi = 0
    for c in range(VMC_W):
        t = first_difference(out['move_stat'][:, c], ref.stat[:, c])
        # (the rows up to the proposal after the first differing test agree)
        upto = VMC_YIELDS if t is None else t + 1
        lo += int(ref.general[:upto, c].sum())
        hi += int(ref.general[:upto, c].sum()) + VMC_YIELDS - upto
    say('part2', cid, dict(general=general, expected=lo,
                           per_chain=ref.general.sum(0).tolist(),
                           sort_gave_up=int((ref.trips < 0).sum()),
                           most_trips=int(ref.trips.max()),
                           far_margin=ref.far_margin or 0.0))
    assert lo <= general <= hi, (general, lo, hi)
    if n > 64 and n % 2:
        # N = 101: every chain at every yield -- not a sign of clustered
        # walkers: the shape has no sorted rows
        assert general == VMC_W * VMC_YIELDS


# ---------------------------------------------------------------------------
# 3. DMC real steps
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_dmc_real_steps_follow_the_oracle(engines, oracle, case):
    """12 walkers (max 16), 8 steps at the model's time step: population exact
    and E_t / E_ref at 1e-9 every step; after the last step, per walker:
    cloning table exact, energy at 2e-11, positions (minimum image) and drift
    at 1e-10."""
    from phd_qmclib_amd.engine import DmcEnsemble
    cid = case_id(case)
    L = case[2]
    ref = gc.dmc_preconditions(oracle, case)
    orc, ys = ref.orc, ref.yields
    d = DmcEnsemble(engines(case), ref.time_step, DMC_MAXW, DMC_W, DMC_KAPPA,
                    rng_seed=ref.seed)
    try:
        d.set_state(ref.pos0)
        ser = d.run_block(DMC_STEPS)
        st = d.get_state()
    finally:
        d.close()
    dev = dict(E_t=0.0, E_ref=0.0)
    for t, (nw, e_t, e_ref) in enumerate(ys):
        assert int(ser.num_walkers[t]) == nw, t
        dev['E_t'] = max(dev['E_t'], worst(ser.energy[t], e_t) / 1e-9)
        dev['E_ref'] = max(dev['E_ref'],
                           worst(ser.ref_energy[t], e_ref) / 1e-9)
    nw = ys[-1][0]
    z_o, f_o = orc.confs[:nw, 0], orc.confs[:nw, 1]
    dz = np.abs(st.confs[:nw, 0] - z_o)
    dz = np.minimum(dz, L - dz)
    dev['energy'] = worst(st.energy[:nw], orc.energy[:nw]) / RTOL
    dev['pos'] = float((dz / np.maximum(1.0, np.abs(z_o))).max()) / 1e-10
    dev['drift'] = worst(st.confs[:nw, 1], f_o) / 1e-10
    say('part3', cid, dict(dev, dt=ref.time_step, crossed=ref.crossed,
                           populations='/'.join(str(y[0]) for y in ys)))
    for t, (nw_t, e_t, e_ref) in enumerate(ys):
        assert ser.energy[t] == pytest.approx(e_t, rel=1e-9), t
        assert ser.ref_energy[t] == pytest.approx(e_ref, rel=1e-9), t
    assert st.num_walkers == nw
    assert np.array_equal(st.cloning_ref[:nw], orc.cloning_ref[:nw])
    assert dev['energy'] <= 1.0 and dev['pos'] <= 1.0 and \
        dev['drift'] <= 1.0, dev


# ---------------------------------------------------------------------------
# 4. production equals series at a spread that rounds
# ---------------------------------------------------------------------------

def lean_equals_series(oracle, eng, case, b):
    """Two blocks of b yields at either spread of `lean_spreads`, production
    and series ensemble of the same seed: everything bit-equal after every
    block, as `lean_against_series` of tests/test_gpu_vmc_steady_lean.py
    demands."""
    _, n, L, c = case
    pos0 = start_rows(n, L, c * L, 7000 + n)
    for spread in gc.lean_spreads(n, L):
        assert gc.product_rounds(oracle, spread)
        full = vmc_block(eng, pos0, spread, 1, [b, b], True)
        lean = vmc_block(eng, pos0, spread, 1, [b, b], False)
        accepted = sum(int(y['num_accepted'].sum()) for y, _, _ in full)
        assert VMC_W < accepted < VMC_W * 2 * b, 'both outcomes occur'
        for k, ((x, sx, gx), (y, sy, gy)) in enumerate(zip(lean, full)):
            what = (case_id(case), spread, b, k)
            for key in ('sum_energy', 'sum_energy2', 'num_accepted'):
                assert np.array_equal(x[key], y[key]), (key,) + what
            assert gx == gy, what
            for u, v in zip(sx, sy):
                assert np.array_equal(u, v), what
            assert np.array_equal(sx[1], y['wf_abs_log'][-1]), what
            assert np.array_equal(sx[2], y['energy'][-1]), what


@pytest.mark.parametrize('b', gc.LEAN_BLOCKS)
@pytest.mark.parametrize('n', gc.LEAN_SIZES)
@pytest.mark.parametrize('name', gc.LEAN_MODELS)
def test_production_equals_series_at_a_spread_that_rounds(engines, oracle,
                                                           name, n, b):
    """The steady production kernel formed z + d with one rounding (an fma)
    on the unpadded shapes without a fused loop (N = 16, 32 here); the fix
    sits in source every shape shares.  66 yields: the fused launch (N = 48,
    64, 99, 128) refills its accept thresholds."""
    case = gc.lean_case(name, n)
    lean_equals_series(oracle, engines(case), case, b)


@pytest.mark.parametrize('b', gc.LEAN_BLOCKS)
@pytest.mark.parametrize('n', gc.LEAN_FLOAT_SIZES)
@pytest.mark.parametrize('name', gc.LEAN_MODELS)
def test_float_production_equals_float_series(engines, oracle, name, n, b):
    """The `R = float` instantiations: float production against float series
    (no oracle needed); the variant must be in effect."""
    case = gc.lean_case(name, n)
    eng = engines(case, fast_math=True)
    assert eng.fast_math is True
    lean_equals_series(oracle, eng, case, b)
