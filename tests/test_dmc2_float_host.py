"""The preconditions of tests/test_gpu_dmc2_float_steps.py without a GPU:
everything tests/_dmc2_float_cases.py derives from the fp64 restatement of
the second-order step and the CPU oracle -- the seeds, the left-out caps, the
branching margins, the seam crossings and order changes, the sorted-row path
of every evaluated row, and the size of the bounds B_s and G_s B_s the device
test grants a float child."""
import numpy as np
import pytest

from . import _dmc2_float_cases as fc
from . import _generic_cases as gc
from . import _vmc_sweep_cases as sc
from .test_gpu_fastmath import TOL_DRIFT, TOL_ENERGY


def test_every_float_instantiation_has_a_case():
    """One N per shape `dmc_evolve2_kernel<G, P, PAD, false, float>` exists
    at (csrc/qmc_inst.h: QMC_INST_EVO2_SMALL_F at (64, 1), (64, 2),
    QMC_INST_EVO2_MASKED_F at (64, 4), (64, 8)), by the arithmetic of
    `pick_shape`: P particles per lane of one wavefront, PAD = N != 64 P
    (always on from P = 4)."""
    def shape(n):
        p = next(p for p in (1, 2, 4, 8) if n <= 64 * p)
        return 64, p, p >= 4 or n != 64 * p
    want = {(64, 1, False), (64, 1, True), (64, 2, False), (64, 2, True),
            (64, 4, True), (64, 8, True)}
    assert {shape(n) for n in fc.SIZES} == want
    assert {shape(n) for n in fc.SORTED_SIZES} == \
        set(fc.ZERO_MOVE_SHAPE.values())
    assert [shape(n)[1] for n in fc.LINEAR_SIZES] == [4, 8]


def test_start_rows_sit_next_to_the_seam():
    for n in fc.SIZES:
        L = gc.lean_case('box', n)[2]
        rows = fc.start_rows(n, L)
        assert rows.shape == (fc.W, n)
        # rotated lattices: ascending but for the one wrap
        assert np.all((np.diff(rows, axis=1) < 0).sum(axis=1) <= 1)
        # gaps of at most 1.6 spacings: a particle within one of the seam
        edge = np.minimum(rows, L - rows).min(axis=1)
        assert np.all(edge < L / n)


def test_cyclic_order():
    row = np.array([0.3, 0.1, 0.7, 0.5])
    assert np.array_equal(fc.cyclic_order(row), [0, 3, 2, 1])
    assert np.array_equal(fc.cyclic_order(np.mod(row + 0.35, 1.0)),
                          fc.cyclic_order(row))
    swapped = row.copy()
    swapped[[0, 3]] = swapped[[3, 0]]
    assert not np.array_equal(fc.cyclic_order(swapped), fc.cyclic_order(row))


def test_forward_differences_against_central_ones(oracle):
    """The Jacobian and the energy gradient of the bounds: forward differences
    of step 1e-6 against central differences of step 1e-4 on one row, to 1 %
    of the largest entry."""
    case = gc.lean_case('box', 37)
    _, m = gc.oracle_model(oracle, case)
    row = fc.start_rows(37, case[2])[0]
    grad, jac = fc.energy_gradient_and_jacobian(oracle, m, row)
    # (the batch entry is `oracle.energy_drift`, row by row)
    rows = fc.start_rows(37, case[2])[:3]
    e, f = fc.energy_drift_rows(oracle, m, rows)
    for k in range(3):
        e1, _, f1 = oracle.energy_drift(m, rows[k])
        assert e[k] == e1 and np.array_equal(f[k], f1)
    h = 1e-4
    for j in (0, 11, 36):
        up, dn = row.copy(), row.copy()
        up[j] += h
        dn[j] -= h
        eu, _, fu = oracle.energy_drift(m, up)
        ed, _, fd = oracle.energy_drift(m, dn)
        assert abs(grad[j] - (eu - ed) / (2 * h)) <= 1e-2 * np.abs(grad).max()
        assert np.abs(jac[:, j] - (fu - fd) / (2 * h)).max() <= \
            1e-2 * np.abs(jac).max()


@pytest.mark.parametrize('case', fc.CASES, ids=fc.case_id)
def test_preconditions_of_the_device_cases(oracle, case):
    n, dt = case
    ref = fc.preconditions(oracle, case)
    # the seed is the smallest that meets them all
    for seed in range(1, fc.SEEDS[case]):
        assert fc.reference(oracle, case, seed).ok() is not None, seed
    assert len(ref.yields) == fc.STEPS
    assert 0 < min(y[0] for y in ref.yields) and \
        max(y[0] for y in ref.yields) <= fc.MAXW
    b = ref.bounds()
    nw0 = ref.yields[0][0]
    assert all(len(v) == nw0 for v in b.values())
    # the left-out cap
    assert int(b['left_out'].sum()) <= fc.LEFT_OUT_CAP[dt]
    assert np.array_equal(b['left_out'],
                          b['B'] > fc.LEFT_OUT_RATIO * b['pair'])
    # branching: 2 for E and E_ref, times 2
    assert ref.branch_floor == 4 * dt * TOL_ENERGY * max(1.0, ref.e_max)
    assert ref.pop.branch_margin > ref.branch_floor
    assert ref.pop.crossed >= 1
    if dt == fc.TIME_STEPS[1]:
        assert ref.order_changed >= 1
    if n in fc.SORTED_SIZES:
        assert ref.sorted_rows and ref.far_margin > fc.FAR_MIN
        assert ref.expected_general() == 0
    if n == 101:
        assert ref.expected_general() == 3 * sum(y[0] for y in ref.yields)
    # what the bounds grant: B_s is the first-order formula, and stays a small
    # part of the float tolerances themselves
    assert np.allclose(b['B'], 4 * dt * TOL_DRIFT *
                       (b['fm'] + b['kappa'] * b['fa']) +
                       4 * np.spacing(ref.L), rtol=1e-14, atol=0)
    share = (b['G'] * b['B'])[~b['left_out']].max() / (TOL_ENERGY * ref.e_max)
    print(fc.case_id(case), 'seed', ref.seed, 'kappa %.3f-%.3f' %
          (b['kappa'].min(), b['kappa'].max()), 'B max %.2e' % b['B'].max(),
          'G B / (TOL_ENERGY |E|) %.3f' % share,
          'left out', int(b['left_out'].sum()), 'crossed', ref.pop.crossed,
          'order changes', ref.order_changed,
          'branch margin %.1e' % ref.pop.branch_margin)
    assert b['kappa'].max() < 0.5           # the first-order bracket means it
    assert share < 0.25


@pytest.mark.parametrize('n', fc.LINEAR_SIZES)
def test_linear_seeds_meet_the_float_tests_own_rule(oracle, n):
    seed = fc.LINEAR_SEEDS[n]
    assert fc.linear_seed_ok(oracle, n, seed)
    for lower in range(1, seed):
        assert not fc.linear_seed_ok(oracle, n, lower), lower


def test_sweep_cases_exist():
    """Part 4 of the device module takes these from the sweep module."""
    assert set(fc.SWEEP_CASES) <= set(sc.IDS)
    assert sc.SPREADS == (0.125, 0.75)
