"""The float pair loop (`fast_math`) inside the SECOND-ORDER DMC step
(`propagator='quadratic'`): `dmc_evolve2_kernel<G, P, PAD, false, float>`
(csrc/qmc_evolve2.h), which `LaunchEvolve2` picks on a fast-math engine at the
six shapes csrc/qmc_inst.h instantiates.  tests/test_gpu_dmc2_steps.py runs
that kernel in double only, tests/test_gpu_fastmath_steps.py the float loop
of `vmc_step_kernel` and `dmc_evolve_kernel` only.  The kernel is its own: the
sorted-row float sums run three times per step as one loop body, every stage
decides sorted or general for itself, and the by-label rows R_a and xi2 sit
behind the float pair tables in the same LDS block.

  case               instantiation <G, P, PAD>  launched by
  box64              <64, 1, false>             parts 1, 2 (N = 64)
  box37, box48       <64, 1, true>              parts 1, 2 (N = 37)
  box128             <64, 2, false>             parts 1, 2 (N = 128)
  deep100, box100,   <64, 2, true>              parts 1, 2 (N = 100, and
  box126                                        N = 101: general sum)
  N = 130            <64, 4, true>              parts 1, 2
  N = 260            <64, 8, true>              parts 1, 2

1. The zero-move quadratic step (time step 1e-300, a tape of zeros with TWO
   rows of normals per walker and step: all three stages evaluate the same
   row) on the golden configurations of every sorted-row shape against
   kernels.npz, and at N = 130, 260 against the oracle, at TOL_ENERGY /
   TOL_DRIFT of tests/test_gpu_fastmath.py.
2. Real steps against the fp64 restatement (tests/_dmc2_restatement.py) at
   1e-3 and 8e-3; cases, seeds, preconditions and the bounds B_s, G_s B_s and
   ||J(R')|| B_s a float child is granted: tests/_dmc2_float_cases.py (run
   without a GPU by tests/test_dmc2_float_host.py).  The drift is checked at
   TOL_DRIFT of the row's largest |drift| plus ||J(R')||_inf B_s -- the
   Jacobian at R' comes with the evaluations G_s needs.
3. The LINEAR float step (`dmc_evolve_kernel<64, 4 | 8, true, false, float>`)
   at N = 130, 260: the body of `test_dmc_float_steps_follow_the_oracle`, which
   the suite ran at N = 64, 100 only.
4. Single-particle sweeps on a fast-math engine are the fp64 sweeps: the
   body of `test_sweeps_against_restatement` at its double tolerances.

Every achieved maximum goes to fastmath_report.json under `steps_quadratic`
(quoted in DESIGN.md).

What part 2 notices, tried once on a build whose float kernel scaled the
drift of the second stage by 1 + 1e-4 (five times TOL_DRIFT): all fourteen
cases fail on the positions, at 2.4 B_s (1e-3) and 1.9 B_s (8e-3) -- the
1e-4 / (4e-5 (1 + kappa)) the bound predicts; an error of TOL_DRIFT itself
sits at half of B_s.  The zero-move steps cannot see it (dt = 1e-300).
"""
import numpy as np
import pytest

from . import _dmc2_float_cases as fc
from . import _generic_cases as gc
from . import _vmc_sweep_cases as sc
from . import conftest as ct
from . import test_gpu_fastmath_steps as fs
from . import test_gpu_vmc_sweep as vs
from ._models import spec_from_golden
from .test_gpu_dmc2_steps import run_block
from .test_gpu_fastmath import (TOL_DRIFT, TOL_ENERGY, _report,
                                min_separation)
from .test_gpu_fastmath_steps import (check_float_rows, errors, golden_keep,
                                      jittered_rows, summary)
from .test_gpu_parity import close

pytestmark = pytest.mark.gpu

_RECORD = {}


def _record(name, rows):
    _RECORD[name] = rows
    _report({'steps_quadratic': dict(_RECORD)})


@pytest.fixture(scope='module')
def box_engines(oracle):
    """Fast-math engines of the box at N particles."""
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(n):
        if n not in cache:
            cfc, _ = gc.oracle_model(oracle, gc.lean_case('box', n))
            cache[n] = ModelEngine(cfc, fast_math=True)
            assert cache[n].fast_math
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


# ---------------------------------------------------------------------------
# 1. the zero-move step
# ---------------------------------------------------------------------------

def quadratic_zero_move_step(eng, pos):
    """`dmc_zero_move_step` of tests/test_gpu_fastmath_steps.py under
    propagator='quadratic': two steps of time_step = 1e-300 under a tape of
    zeros, [slot][2][N] normals per step -> (energy, drift) of the first
    step's children; the exact asserts of that helper are made here."""
    from phd_qmclib_amd.engine import DmcEnsemble
    W, n = pos.shape
    L = float(eng.cfc_spec.model_params.supercell_size)
    d = DmcEnsemble(eng, 1e-300, W, W, 0.5, rng_seed=1,
                    propagator='quadratic')
    try:
        d.set_state(pos)
        d.set_tape(np.zeros(2 * W), np.zeros(2 * 2 * W * n), [0, W],
                   [0, 2 * W * n])
        ser = d.run_block(2)
        st = d.get_state()
    finally:
        d.close()
    assert np.array_equal(ser.num_walkers, [W, W])
    assert st.num_walkers == W
    assert np.array_equal(st.cloning_ref[:W], np.arange(W))
    # the positions come back as given (a particle at exactly 0: see the
    # linear helper)
    dz = np.abs(st.confs[:W, 0] - pos)
    assert np.all(np.minimum(dz, L - dz) <= 1e-250)
    assert np.array_equal(ser.weight, [W, W])
    assert close(ser.energy[1], st.energy[:W].sum(), rtol=1e-13 * W)
    return st.energy[:W].copy(), st.confs[:W, 1].copy()


@pytest.mark.parametrize('tag', fs.TAGS)
def test_zero_move_quadratic_step_float_on_golden_configurations(
        golden_params, golden_kernels, tag):
    from phd_qmclib_amd.engine import ModelEngine
    assert tag in fc.ZERO_MOVE_SHAPE
    eng = ModelEngine(spec_from_golden(golden_params, tag).cfc_spec,
                      fast_math=True)
    try:
        assert eng.fast_math
        L = float(eng.cfc_spec.model_params.supercell_size)
        pos, keep = golden_keep(golden_kernels, tag, L)
        eng.general_path_walkers(reset=True)
        en, dr = quadratic_zero_move_step(eng, pos)
        general = eng.general_path_walkers()
    finally:
        eng.close()
    g = golden_kernels
    err = dict(energy=errors(en, g[tag + '/energy']),
               drift=errors(dr, g[tag + '/ith_drift'], drift=True))
    _record(f'zero_move/{tag}',
            dict(summary(err, keep), general_path_walkers=general,
                 energy_of_tol=float(err['energy'].max() / TOL_ENERGY),
                 drift_of_tol=float(err['drift'][keep].max() / TOL_DRIFT)))
    check_float_rows((tag, 'dmc2'), err, keep)
    assert general == 0, 'a golden row left the sorted path'
    assert max(e.max() for e in err.values()) > 1e-10


@pytest.mark.parametrize('n', [130, 260])
def test_zero_move_quadratic_step_float_general_sum(oracle, box_engines, n):
    """Four and eight particles per lane: the general pair sum in float at
    all three stages, against the oracle on jittered rows (as
    `test_float_general_pair_sum_inside_the_steps_n130`)."""
    case = gc.lean_case('box', n)
    _, m = gc.oracle_model(oracle, case)
    eng = box_engines(n)
    pos = jittered_rows(np.random.RandomState(n), 6, n, case[2])
    keep = np.array([min_separation(p, case[2]) > 1e-3 for p in pos])
    assert keep.all()
    _, en, _, fd = oracle.evaluate_set(m, pos)
    en_d, dr_d = quadratic_zero_move_step(eng, pos)
    err = dict(energy=errors(en_d, en), drift=errors(dr_d, fd, drift=True))
    _record(f'zero_move/n{n}',
            dict(summary(err, keep),
                 energy_of_tol=float(err['energy'].max() / TOL_ENERGY),
                 drift_of_tol=float(err['drift'].max() / TOL_DRIFT)))
    check_float_rows((f'n{n}', 'dmc2'), err, keep)
    assert max(e.max() for e in err.values()) > 1e-10


# ---------------------------------------------------------------------------
# 2. real steps against the fp64 restatement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('case', fc.CASES, ids=fc.case_id)
def test_quadratic_float_steps_follow_the_restatement(oracle, box_engines,
                                                      case):
    n, dt = case
    ref = fc.preconditions(oracle, case)
    b, pop, L = ref.bounds(), ref.pop, ref.L
    eng = box_engines(n)
    ser, st, general = run_block(eng, ref.pos0, dt, ref.seed, steps=fc.STEPS,
                                 maxw=fc.MAXW, target=fc.W,
                                 propagator='quadratic')
    nw = ref.yields[-1][0]
    # the yielded walkers: children of step 0, as cloned by step 1
    child = ref.tables[-1]
    keep = ~b['left_out'][child]
    assert keep.any()
    z_o, f_o, e_o = pop.confs[:nw, 0], pop.confs[:nw, 1], pop.energy[:nw]
    figures = dict(E_t=0.0)
    for t, (nw_t, e_t, _) in enumerate(ref.yields):
        figures['E_t'] = max(figures['E_t'], float(
            abs(ser.energy[t] - e_t) / max(1.0, abs(e_t)) / TOL_ENERGY))
    got_z = np.asarray(st.confs[:nw, 0]) if st.num_walkers == nw else None
    if got_z is not None:
        dz = np.abs(got_z - z_o)
        dz = np.minimum(dz, L - dz).max(axis=1)
        e_abs = np.abs(st.energy[:nw] - e_o)
        e_bound = TOL_ENERGY * np.maximum(1.0, np.abs(e_o)) + \
            (b['G'] * b['B'])[child]
        f_abs = np.abs(st.confs[:nw, 1] - f_o).max(axis=1)
        f_bound = TOL_DRIFT * np.abs(f_o).max(axis=1) + \
            (b['JR'] * b['B'])[child]
        e_en = errors(st.energy[:nw], e_o)
        e_dr = errors(st.confs[:nw, 1], f_o, drift=True)
        figures.update(
            pos_abs=float(dz[keep].max()),
            pos_of_bound=float((dz / b['B'][child])[keep].max()),
            energy=float(e_en[keep].max()),
            energy_of_bound=float((e_abs / e_bound)[keep].max()),
            drift=float(e_dr[keep].max()),
            drift_of_bound=float((f_abs / f_bound)[keep].max()),
            largest_error=float(max(e_en.max(), e_dr.max())))
    figures.update(
        left_out_share=float((~keep).mean()), general_path_walkers=general,
        populations='/'.join(str(y[0]) for y in ref.yields),
        device_populations='/'.join(str(int(x)) for x in ser.num_walkers),
        crossed=pop.crossed, order_changes=ref.order_changed,
        note=f'{fc.W} walkers, {fc.STEPS} steps of {dt:g}, seed {ref.seed}')
    print(fc.case_id(case), figures)
    _record(f'real_step/{fc.case_id(case)}', figures)
    for t, (nw_t, e_t, _) in enumerate(ref.yields):
        assert int(ser.num_walkers[t]) == nw_t, t
        assert close(ser.energy[t], e_t, TOL_ENERGY), t
    assert st.num_walkers == nw
    assert np.array_equal(st.cloning_ref[:nw], child)
    assert np.all(np.isfinite(st.confs[:nw])) and \
        np.all(np.isfinite(st.energy[:nw]))
    assert np.all(dz[keep] <= b['B'][child][keep]), figures
    assert np.all(e_abs[keep] <= e_bound[keep]), figures
    assert np.all(f_abs[keep] <= f_bound[keep]), figures
    if ref.expected_general() is not None:
        assert general == ref.expected_general()
    assert figures['largest_error'] > 1e-10     # the float loop was measured


# ---------------------------------------------------------------------------
# 3. the linear float step at the masked shapes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', fc.LINEAR_SIZES)
def test_linear_float_steps_at_the_masked_shapes(oracle, box_engines,
                                                 monkeypatch, n):
    """`test_dmc_float_steps_follow_the_oracle` as it stands, handed the box
    at N = 130 / 260: its engine, its oracle model (through
    `gc.oracle_model`, not a golden tag) and its seed (its own 1e-4 rule,
    applied on the oracle: tests/_dmc2_float_cases.py)."""
    tag = f'box{n}'
    assert fc.linear_seed_ok(oracle, n, fc.LINEAR_SEEDS[n])
    _, m = gc.oracle_model(oracle, gc.lean_case('box', n))
    monkeypatch.setitem(fs.DMC_SEEDS, tag, fc.LINEAR_SEEDS[n])
    monkeypatch.setattr(ct, 'oracle_model', lambda o, params, t: m)
    fs.test_dmc_float_steps_follow_the_oracle(
        lambda t: box_engines(n), oracle, None, tag)
    _record(f'linear_step/n{n}', fs._RECORD['steps_real_step'][f'{tag}/dmc'])


# ---------------------------------------------------------------------------
# 4. sweeps ignore the switch
# ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def fast_sweep_engines():
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = ModelEngine(sc.make_spec(cid).cfc_spec,
                                     fast_math=True)
        return cache[cid]
    yield get
    for e in cache.values():
        e.close()


@pytest.mark.parametrize('spread', sc.SPREADS)
@pytest.mark.parametrize('cid', fc.SWEEP_CASES)
def test_sweeps_on_a_fast_math_engine_are_the_double_sweeps(
        fast_sweep_engines, oracle, monkeypatch, cid, spread):
    """`move='particle'` is "fp64 whatever `set_fast_math` says"
    (engine.py, csrc/qmc_vmc_sweep.h): the body of
    `test_sweeps_against_restatement` -- same restatement, seeds and double
    tolerances -- on an engine with the switch on.  (A run cache of its own:
    that module shares its device runs between tests.)"""
    eng = fast_sweep_engines(cid)
    if sc._SPEC[cid][0] in (64, 128):
        assert eng.fast_math, 'the switch was on'
    monkeypatch.setattr(vs, '_runs', {})
    vs.test_sweeps_against_restatement(fast_sweep_engines, oracle, cid,
                                       spread)
