"""The position-classified (`ZC = true`) instantiations of the four walker
kernels -- `evaluate_kernel`, `prepare_kernel`, `vmc_step_kernel`,
`dmc_evolve_kernel` -- at every lane-group shape, padded and exact.

A contact cutoff above 0.45 L (`DevModel.zclass`, `build_dev_model` in
csrc/qmcwalk.hip) makes the library classify pairs from |z_a - z_b| instead of
sin(pi r / L): a fifth LDS row of positions, the `wrapped` / `neg` logic of
`pair_core` / `pair_core4` from the positions, no ROTCOPY / TWOCASE /
LEAD_SHORT form, no sorted-row pair sum at N <= 128 (the stepping kernels keep
the lanes ascending with `anchor_seam` + `resort_linear<64>` at (64, 1) and
`anchor_seam_rows` + `resort_linear_rows` from (64, 2) on), no fused VMC loop
(a production block is one launch per yield).  `tbf_contact_cutoff` is the
variational parameter `wf_opt` moves, so these are production kernels.

Reference in every part: the CPU oracle, `oracle.evaluate_set` or its chains /
populations on the same Philox streams.

Models: the unit-filling box of the suite (depth 5 pi^2, ratio 1, coupling 2,
L = N) with cutoff c L -- c = 0.47 at every size (5-6 % of the pairs of a
uniform row are then long: both classes and both sides of `wrapped` in every
walker), c = 0.4501 (just past the switch), 0.4999 and 0.5 exactly
(rm == L - rm, sin_rm = 1) at N = 32, 64, 128, 300 -- and the off-lattice
model of 'odd24' (half-integer number of lattice periods, non-integer L) at
(N, L, c) = (40, 29.5, 0.46) and (100, 72.5, 0.47).

Sizes, the smallest that reach each variant padded and exact: (16, 1): 9, 16;
(16, 2): 24, 32; (64, 1): 37, 64; (64, 2): 66, 101, 128; (64, 4): 130, 256;
(64, 8): 300, 512.

1. single evaluations: `qmc_evaluate`, the forced first VMC yield (series and
   production kernel) and the zero-move DMC step on six rows per model, one of
   them holding pairs 1e-6 L on either side of every edge of the classifier
   (rm, L - rm, L / 2), at the suite's 2e-11;
2. real VMC steps: 6 chains, 24 yields, move_spread 0.6 (box-boundary
   crossings and many inversions per step; six resort passes), against
   `oracle.VmcChain`, and the production path bit-equal to the series path;
3. real DMC steps: 12 walkers, 8 steps, walkers die and clone and cross the
   seam; the per-walker state after the last step against the oracle's;
4. either side of the switch: c = 0.45 (sine classifier, sorted rows, float
   variant available) and c = 0.4501 (position classifier).

Part 2 found the production block an ulp away from the series run at the
exact sizes 16, 32, 64, 128: the steady kernel of the unfused, unpadded shapes
fused z + d into an fma (fixed in `vmc_step_kernel`; invisible at the
move_spread 0.125 of the rest of the suite, where the product is exact).  The
last test pins the same kernels of the sine classifier at N = 16, 32.

The start rows, the oracle's chains and populations and the once-per-walker
condition of the sorted rows are shared with tests/test_gpu_generic_steps.py
(the sine classifier on generic models): tests/_steps.py.

Every precondition (classifier-edge distances, box crossings, branching
margins) is asserted from the oracle / numpy before the device is compared.
Every test prints its worst deviation as a fraction of its tolerance (`-s`);
DESIGN.md section 2 quotes one run.
"""
from math import pi

import numpy as np
import pytest

from ._steps import (DMC_DT, DMC_KAPPA, DMC_MAXW, DMC_STEPS, DMC_W, EDGE_EPS,
                     VMC_SPREAD, VMC_W, VMC_YIELDS, dmc_start,
                     oracle_dmc_run, oracle_vmc_chains, report, six_rows,
                     start_rows, takes_sorted_rows)
from ._traj import explain_flips
from .test_gpu_parity import close, worst

pytestmark = pytest.mark.gpu

RTOL = 2e-11                    # the suite's double-path tolerance
EDGE_MIN = 1e-9                 # no pair closer to an edge of the classifier, of L

SIZES = (9, 16, 24, 32, 37, 64, 66, 101, 128, 130, 256, 300, 512)
EDGE_SIZES = (32, 64, 128, 300)
EDGE_CUTS = (0.4501, 0.4999, 0.5)
ODD = ((40, 29.5, 0.46), (100, 72.5, 0.47))

# (kind, N, L, c): 'box' -- the unit-filling box; 'odd' -- the off-lattice model
CASES = [('box', n, float(n), 0.47) for n in SIZES] + \
        [('box', n, float(n), c) for c in EDGE_CUTS for n in EDGE_SIZES] + \
        [('odd', n, L, c) for n, L, c in ODD]


def case_id(case):
    kind, n, _, c = case
    return f'{kind}{n}-c{c}'


IDS = [case_id(c) for c in CASES]

# Philox seeds, chosen with the oracle alone (no device result enters): the
# smallest seed >= 1 with which the oracle's chains of the case cross the box
# boundary at least 3 times (VMC), and with which no branching draw w + u of
# the oracle's population lies within 1e-6 of an integer, the population stays
# below max_num_walkers and a particle crosses the boundary (DMC).  The tests
# assert these properties again from the oracle.
# (VMC: seed 1 gives 3-16 crossings and 22-47 accepted steps of 138 in every
# case; DMC: with seeds 1 / 2 the larger boxes below run into the cap of 16)
VMC_SEEDS = {cid: 1 for cid in IDS}
DMC_SEEDS = dict({cid: 1 for cid in IDS}, **{
    'box128-c0.47': 2, 'box300-c0.47': 3, 'box512-c0.47': 3,
    'box128-c0.4501': 2, 'box300-c0.4501': 3,
    'box128-c0.4999': 2, 'box300-c0.4999': 3, 'box300-c0.5': 3})


def make_spec(golden_params, kind, n, L, cutoff):
    from phd_qmclib_amd.mrbp_qmc import Spec
    if kind == 'odd':
        kw = dict(golden_params['odd24']['spec'])
    else:
        kw = dict(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                  interaction_strength=2)
    kw.update(boson_number=n, supercell_size=L, tbf_contact_cutoff=cutoff)
    return Spec(**kw)


class Model:
    """Spec, oracle model and engine of one case.  The engine is created with
    the float variant REQUESTED where it could exist (N > 32): that the
    request is refused is the one observable sign that the engine classifies
    pairs from the positions."""

    def __init__(self, oracle, golden_params, case, fast_math=None):
        from phd_qmclib_amd.engine import ModelEngine
        self.kind, self.n, self.L, self.c = case
        self.rm = self.c * self.L
        self.cfc = make_spec(golden_params, self.kind, self.n, self.L,
                             self.rm).cfc_spec
        self.m = oracle.model_from_cfc(self.cfc)
        assert float(self.m.tbf_contact_cutoff) == self.rm
        assert float(self.m.supercell_size) == self.L
        if fast_math is None:
            fast_math = self.n > 32
        self.eng = ModelEngine(self.cfc, fast_math=fast_math)

    def assert_position_classifier(self):
        assert self.rm / self.L > 0.45
        if self.n > 32:
            assert self.eng.fast_math is False, \
                'the float variant exists: pairs are classified from the sines'


@pytest.fixture(scope='module')
def models(oracle, golden_params):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Model(oracle, golden_params, case)
        return cache[case]
    yield get
    for mod in cache.values():
        mod.eng.close()


# ---------------------------------------------------------------------------
# configurations
# ---------------------------------------------------------------------------

def edge_distance(pos, L, rm):
    """The smallest distance of any |z_a - z_b| of any row from the edges rm
    and L - rm of the position classifier, and the number of pairs closer
    than 2 EDGE_EPS L to one."""
    n = pos.shape[1]
    ia, ib = np.triu_indices(n, 1)
    d = np.abs(pos[:, ia] - pos[:, ib])
    e = np.minimum(np.abs(d - rm), np.abs(d - (L - rm)))
    return float(e.min()), int((e < 2 * EDGE_EPS * L).sum())


def assert_off_the_edges(pos, L, rm):
    """The energy jumps at rm: a pair exactly on an edge has no defined
    class."""
    dist, _ = edge_distance(pos, L, rm)
    assert dist >= EDGE_MIN * L, dist / L


def row_scales(en, ie, wf, fd):
    """Scales of tests/test_sweep.py::test_device_vs_reference, per
    configuration: the largest magnitude of the quantity, for log|psi| and the
    energy that of the per-particle energies as well, at least 1."""
    top_ie = np.abs(ie).max(1)
    return dict(wf_abs_log=np.maximum(1.0, np.maximum(np.abs(wf), top_ie)),
                energy=np.maximum(1.0, np.maximum(np.abs(en), top_ie)),
                ith_energy=np.maximum(1.0, top_ie),
                drift=np.maximum(1.0, np.abs(fd).max(1)))


def deviation(got, ref, scale):
    """max over the configurations of max |got - ref| / scale."""
    ref = np.asarray(ref, dtype=np.float64)
    ref2 = ref.reshape(ref.shape[0], -1)
    got2 = np.asarray(got, dtype=np.float64).reshape(ref2.shape)
    return float((np.abs(got2 - ref2).max(1) / scale).max())


def vmc_first_yield(eng, pos, series):
    """The forced first yield of chains started at pos[W, N] -> (energy[W],
    log|psi|[W])."""
    from phd_qmclib_amd.engine import VmcEnsemble
    W = pos.shape[0]
    v = VmcEnsemble(eng, W, 0.125, rng_seed=1)
    v.set_state(pos)
    out = v.run_block(1, series=series)
    # (the block sums of a one-yield block ARE the first yield: the production
    # kernel has no series)
    en = out['energy'][0] if series else out['sum_energy']
    assert np.all(out['num_accepted'] == 1)
    p, wf, ec = v.get_state()
    if series:
        assert np.array_equal(out['wf_abs_log'][0], wf)
        assert out['move_stat'].all()
    assert np.array_equal(p, pos)           # the state is handed back as given
    assert close(ec, en, 1e-14)             # the carried energy IS that yield
    v.close()
    return np.array(en), wf


def dmc_zero_move_step(eng, pos, L):
    """Two steps of time_step = 1e-300 under a tape of zero normals: positions
    do not move, weights are 1, every walker has one child -> (E_t of the
    second yield, energy[W], drift[W, N] of the first step's children, which
    the energy + drift pass of `dmc_evolve_kernel` computed)."""
    from phd_qmclib_amd.engine import DmcEnsemble
    W, n = pos.shape
    d = DmcEnsemble(eng, 1e-300, W, W, 0.5, rng_seed=1)
    d.set_state(pos)
    d.set_tape(np.zeros(2 * W), np.zeros(2 * W * n), [0, W], [0, W * n])
    ser = d.run_block(2)
    assert np.array_equal(ser.num_walkers, [W, W])
    st = d.get_state()
    assert st.num_walkers == W
    assert np.array_equal(st.cloning_ref[:W], np.arange(W))
    dz = np.abs(st.confs[:W, 0] - pos)
    assert np.all(np.minimum(dz, L - dz) <= 1e-250)
    assert np.array_equal(ser.weight, [W, W])
    d.close()
    return float(ser.energy[1]), st.energy[:W].copy(), st.confs[:W, 1].copy()


def check_single_evaluations(what, mod, oracle, pos):
    """`qmc_evaluate`, the forced first VMC yield of both step kernels and
    the zero-move DMC step on pos[W, N] against `oracle.evaluate_set`, 2e-11
    of the scales of `row_scales` -> {quantity: deviation / tolerance}."""
    W = pos.shape[0]
    wf, en, ie, fd = oracle.evaluate_set(mod.m, pos)
    sc = row_scales(en, ie, wf, fd)
    dev = {}

    def check(name, quantity, got, ref):
        dev[name] = deviation(got, ref, sc[quantity]) / RTOL
        assert dev[name] <= 1.0, (what, name, dev[name] * RTOL)

    out = mod.eng.evaluate(pos)
    check('eval wf', 'wf_abs_log', out.wf_abs_log, wf)
    check('eval energy', 'energy', out.energy, en)
    check('eval ith', 'ith_energy', out.ith_energy, ie)
    check('eval drift', 'drift', out.drift, fd)
    for series in (True, False):
        tag = 'vmc' if series else 'vmc lean'
        en_v, wf_v = vmc_first_yield(mod.eng, pos, series)
        check(tag + ' energy', 'energy', en_v, en)
        # (log|psi| of the step kernels: of max(1, |log psi|) alone, as in
        # tests/test_gpu_sorted_pins.py)
        dev[tag + ' wf'] = deviation(wf_v, wf,
                                     np.maximum(1.0, np.abs(wf))) / RTOL
        assert dev[tag + ' wf'] <= 1.0, (what, tag, 'wf')
    e_t, en_d, dr_d = dmc_zero_move_step(mod.eng, pos, mod.L)
    check('dmc energy', 'energy', en_d, en)
    check('dmc drift', 'drift', dr_d, fd)
    # E_t of the second yield: the sum of those energies (unit weights)
    assert close(e_t, en.sum(), rtol=RTOL * W), (what, 'E_t')
    return dev


# ---------------------------------------------------------------------------
# 1. single evaluations
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_single_evaluations_vs_oracle(models, oracle, case):
    """`evaluate_kernel`, `prepare_kernel` + the energy pass of
    `vmc_step_kernel` (series and production) and the energy + drift pass of
    `dmc_evolve_kernel`, ZC = true, on the six rows of `six_rows`."""
    mod = models(case)
    mod.assert_position_classifier()
    pos = six_rows(mod.n, mod.L, mod.rm, 7000 + mod.n)
    assert len(pos) == (5 if mod.c == 0.5 else 6)
    assert_off_the_edges(pos, mod.L, mod.rm)
    if mod.c != 0.5:
        # the straddling pairs are there: 6 per chosen particle at the least
        _, near = edge_distance(pos[5:], mod.L, mod.rm)
        assert near >= (8 if mod.n >= 14 else 4), near
    # both pair classes and both sides of `wrapped` are there
    ia, ib = np.triu_indices(mod.n, 1)
    d = np.abs(pos[:, ia] - pos[:, ib])
    short = (d < mod.rm) | (d > mod.L - mod.rm)
    assert short.any() and (d > 0.5 * mod.L).any() and (d < 0.5 * mod.L).any()
    if mod.c != 0.5:
        assert (~short).any()
    dev = check_single_evaluations(case_id(case), mod, oracle, pos)
    report('part1', case_id(case), dev)


# ---------------------------------------------------------------------------
# 2. VMC real steps
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_vmc_real_steps_follow_the_oracle(models, oracle, case):
    """6 chains, 24 yields with move_spread 0.6 from the rows of part 1:
    accept / reject series equal (a differing chain must show a
    rounding-level Metropolis margin, at most one: tests/_traj.py), energy and
    log|psi| of every yield at 1e-9, final positions in particle order at
    1e-9; the production kernel (one launch per yield on these shapes) from
    the same start: state bit-equal to the series run's, equal acceptance,
    block sum = sum of the series."""
    from phd_qmclib_amd.engine import VmcEnsemble
    mod = models(case)
    mod.assert_position_classifier()
    cid = case_id(case)
    n, L, seed = mod.n, mod.L, VMC_SEEDS[cid]
    pos0 = start_rows(n, L, mod.rm, 7000 + n)
    st_o, en_o, wf_o, pos_o, crossings = oracle_vmc_chains(
        oracle, mod.m, pos0, VMC_SPREAD, seed, VMC_YIELDS)
    assert crossings >= 3, 'the chains did cross the boundary'
    accepted = int(st_o[1:].sum())
    assert 0 < accepted < VMC_W * (VMC_YIELDS - 1), 'both outcomes occur'
    v = VmcEnsemble(mod.eng, VMC_W, VMC_SPREAD, rng_seed=seed)
    v.set_state(pos0)
    out = v.run_block(VMC_YIELDS, series=True)
    state = v.get_state()
    v.close()
    same = explain_flips(oracle, mod.m, pos0, VMC_SPREAD, seed,
                         out['move_stat'], st_o)
    dev = dict(energy=worst(out['energy'][:, same], en_o[:, same]) / 1e-9,
               wf=worst(out['wf_abs_log'][:, same], wf_o[:, same]) / 1e-9)
    dz = np.abs(np.mod(state[0][same], L) - pos_o[same])
    dev['pos'] = float(np.minimum(dz, L - dz).max()) / 1e-9
    report('part2', cid, dict(dev, crossings=crossings, accepted=accepted))
    assert dev['energy'] <= 1.0 and dev['wf'] <= 1.0 and dev['pos'] <= 1.0, dev
    assert close(state[1][same], wf_o[-1, same], 1e-9)
    # the production path
    p = VmcEnsemble(mod.eng, VMC_W, VMC_SPREAD, rng_seed=seed)
    p.set_state(pos0)
    lean = p.run_block(VMC_YIELDS, series=False)
    lean_state = p.get_state()
    p.close()
    for a, b in zip(lean_state, state):
        assert np.array_equal(a, b)
    assert np.array_equal(lean['num_accepted'], out['num_accepted'])
    assert np.array_equal(out['num_accepted'], out['move_stat'].sum(0))
    assert close(lean['sum_energy'], out['energy'].sum(0),
                 rtol=1e-12 * VMC_YIELDS)


# ---------------------------------------------------------------------------
# 3. DMC real steps
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_dmc_real_steps_follow_the_oracle(models, oracle, case):
    """12 walkers (max 16), time_step 5e-4, 8 steps: population exact and
    E_t / E_ref at 1e-9 every step; after the last step, per walker: cloning
    table exact, energy at 2e-11, positions (minimum image) and drift at
    1e-10."""
    from phd_qmclib_amd.engine import DmcEnsemble
    mod = models(case)
    mod.assert_position_classifier()
    cid = case_id(case)
    n, L, seed = mod.n, mod.L, DMC_SEEDS[cid]
    pos0 = dmc_start(n, L, mod.rm, 7000 + n)
    orc, ys, margin, crossed = oracle_dmc_run(oracle, mod.m, pos0, seed)
    assert margin > 1e-6, 'a marginal branching draw'
    assert crossed >= 1, 'a particle did cross the boundary'
    d = DmcEnsemble(mod.eng, DMC_DT, DMC_MAXW, DMC_W, DMC_KAPPA,
                    rng_seed=seed)
    d.set_state(pos0)
    ser = d.run_block(DMC_STEPS)
    st = d.get_state()
    d.close()
    dev = dict(E_t=0.0, E_ref=0.0)
    for t, (nw, e_t, e_ref) in enumerate(ys):
        assert int(ser.num_walkers[t]) == nw, t
        dev['E_t'] = max(dev['E_t'], worst(ser.energy[t], e_t) / 1e-9)
        dev['E_ref'] = max(dev['E_ref'],
                           worst(ser.ref_energy[t], e_ref) / 1e-9)
        assert ser.energy[t] == pytest.approx(e_t, rel=1e-9), t
        assert ser.ref_energy[t] == pytest.approx(e_ref, rel=1e-9), t
    nw = ys[-1][0]
    assert st.num_walkers == nw
    assert np.array_equal(st.cloning_ref[:nw], orc.cloning_ref[:nw])
    z_o, f_o = orc.confs[:nw, 0], orc.confs[:nw, 1]
    dz = np.abs(st.confs[:nw, 0] - z_o)
    dz = np.minimum(dz, L - dz)
    dev['energy'] = worst(st.energy[:nw], orc.energy[:nw]) / RTOL
    dev['pos'] = float((dz / np.maximum(1.0, np.abs(z_o))).max()) / 1e-10
    dev['drift'] = worst(st.confs[:nw, 1], f_o) / 1e-10
    report('part3', cid, dict(dev, crossed=crossed,
                              populations='/'.join(str(y[0]) for y in ys)))
    assert dev['energy'] <= 1.0 and dev['pos'] <= 1.0 and \
        dev['drift'] <= 1.0, dev


# ---------------------------------------------------------------------------
# 4. either side of the switch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [64, 128])
def test_either_side_of_the_switch(oracle, golden_params, n):
    """c = 0.45: the sine classifier -- the float variant is granted, the
    sorted rows answer the first yield; c = 0.4501: the position classifier --
    the float variant is refused.  Both against the oracle at 2e-11 on the
    rows of part 1.

    The sorted-row path takes a walker only when its farthest rotation
    partner is closer than L - rm = 0.55 L, which 2 % (N = 64) / 6 % (N = 128)
    of uniform random rows meet: the counter of walkers that left it must
    equal the number of rows that fail this condition (numpy, above), and the
    jittered-lattice rows must be among those that stay."""
    L = float(n)
    for c, zclass in ((0.45, False), (0.4501, True)):
        case = ('box', n, L, c)
        fast = Model(oracle, golden_params, case, fast_math=True)
        assert fast.eng.fast_math is (not zclass), c
        fast.eng.close()
        mod = Model(oracle, golden_params, case, fast_math=False)
        pos = six_rows(n, L, mod.rm, 7000 + n)
        assert_off_the_edges(pos, L, mod.rm)
        wf, en, ie, fd = oracle.evaluate_set(mod.m, pos)
        sc = row_scales(en, ie, wf, fd)
        out = mod.eng.evaluate(pos)
        dev = {}
        for name, got, ref in (('wf_abs_log', out.wf_abs_log, wf),
                               ('energy', out.energy, en),
                               ('ith_energy', out.ith_energy, ie),
                               ('drift', out.drift, fd)):
            dev[name] = deviation(got, ref, sc[name]) / RTOL
            assert dev[name] <= 1.0, (n, c, name, dev[name] * RTOL)
        if not zclass:
            stay = np.array([takes_sorted_rows(r, n, L, mod.rm) for r in pos])
            assert stay[3] and stay[4], 'the spread rows take the sorted path'
            for series in (True, False):
                mod.eng.general_path_walkers(reset=True)
                en_v, wf_v = vmc_first_yield(mod.eng, pos, series)
                assert mod.eng.general_path_walkers() == int((~stay).sum()), \
                    (n, series, stay)
                dev['vmc energy'] = deviation(en_v, en, sc['energy']) / RTOL
                dev['vmc wf'] = deviation(
                    wf_v, wf, np.maximum(1.0, np.abs(wf))) / RTOL
                assert dev['vmc energy'] <= 1.0 and dev['vmc wf'] <= 1.0, dev
        report('part4', case_id(case), dev)
        mod.eng.close()


@pytest.mark.parametrize('n', [16, 32])
def test_production_block_equals_series_on_unpadded_small_shapes(golden_params,
                                                                 n):
    """The steady production kernel of the shapes without a fused loop and
    without padding formed z + d with one rounding (an fma) where the series
    kernels -- and the reference -- round the product first: part 2 found
    the production state an ulp away from the series run's at N = 16, 32, 64,
    128.  The same kernels exist for the sine classifier at (16, 1) and
    (16, 2): cutoff L / 4, the comparison of part 2."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    L = float(n)
    eng = ModelEngine(make_spec(golden_params, 'box', n, L, 0.25 * L).cfc_spec)
    pos0 = start_rows(n, L, 0.25 * L, 7000 + n)
    runs = []
    for series in (True, False):
        v = VmcEnsemble(eng, VMC_W, VMC_SPREAD, rng_seed=1)
        v.set_state(pos0)
        runs.append((v.run_block(VMC_YIELDS, series=series), v.get_state()))
        v.close()
    eng.close()
    (out, state), (lean, lean_state) = runs
    assert 0 < int(out['move_stat'][1:].sum()) < VMC_W * (VMC_YIELDS - 1)
    for a, b in zip(lean_state, state):
        assert np.array_equal(a, b)
    assert np.array_equal(lean['num_accepted'], out['num_accepted'])
    assert close(lean['sum_energy'], out['energy'].sum(0),
                 rtol=1e-12 * VMC_YIELDS)
