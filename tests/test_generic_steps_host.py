"""The preconditions of tests/test_gpu_generic_steps.py, for every case,
without a GPU: they come from the CPU oracle and numpy alone
(tests/_generic_cases.py), so the seeds and time steps chosen there can be
checked -- and chosen again -- on any machine."""
import numpy as np
import pytest

from . import _generic_cases as gc
from ._generic_cases import CASES, IDS
from ._steps import (VMC_W, VMC_YIELDS, far_partner_distances, six_rows,
                     sort_slots, takes_sorted_rows)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_vmc_preconditions(oracle, case):
    ref = gc.vmc_preconditions(oracle, case)
    assert ref.rows.shape == (VMC_YIELDS, VMC_W, case[1])
    # the rows the yields evaluate ARE the chain: an accepted proposal is the
    # next state, so the last accepted one is the final configuration
    for c in range(VMC_W):
        t = int(np.nonzero(ref.stat[:, c])[0][-1])
        assert np.array_equal(ref.rows[t, c], ref.pos[c])
    # the exact sort gives up nowhere but on the one row of 'hard' at N = 100
    # on which three particles leave through z = 0 in one step
    gave_up = [tuple(x) for x in np.argwhere(ref.trips < 0).tolist()]
    assert gave_up == ([(16, 4)] if gc.case_id(case) == 'hard100' else [])
    # ... and only there does the counter exceed the far-partner failures
    assert np.array_equal(ref.general, ref.far_fails | (ref.trips < 0))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_dmc_preconditions(oracle, case):
    ref = gc.dmc_preconditions(oracle, case)
    assert ref.time_step in (5e-4, 1e-3, 2e-3)


def test_constants_cover_every_case():
    assert set(gc.DMC_TIME_STEP) == set(gc.STEP_MODELS)
    assert sorted(gc.DMC_SEEDS) == sorted(IDS) == sorted(gc.VMC_SEEDS)


@pytest.mark.parametrize('name,n,dt', [('offlat', 33, 5e-4), ('offlat', 63, 5e-4),
                                       ('free', 37, 5e-4), ('free', 37, 1e-3),
                                       ('free', 66, 1e-3)])
def test_time_step_too_small_to_branch(oracle, name, n, dt):
    """At the time steps below the chosen one the oracle's population of
    these sizes keeps the identity cloning table for 8 steps with every seed
    below 10: such a run would hide the branching kernels."""
    case = next(c for c in CASES if c[:2] == (name, n))
    assert dt < gc.DMC_TIME_STEP[name]
    for seed in range(1, 10):
        ref = gc.DmcReference(oracle, case, seed, dt)
        assert ref.ok() is not None, seed


def test_every_part4_model_is_accepted_and_its_spreads_round(oracle):
    for name in gc.LEAN_MODELS:
        for n in gc.LEAN_SIZES + gc.LEAN_FLOAT_SIZES:
            case = gc.lean_case(name, n)
            gc.oracle_model(oracle, case)
            for spread in gc.lean_spreads(n, case[2]):
                assert gc.product_rounds(oracle, spread), (name, n, spread)
    # the spread of the rest of the suite: a power of two, an exact product
    assert not gc.product_rounds(oracle, 0.125)


def pair_distance_on_the_ring(z, i, j, L):
    d = abs(z[i] - z[j])
    return min(d, L - d)


@pytest.mark.parametrize('n', [33, 37, 48, 63, 64, 66, 100, 126, 128])
def test_far_partner_restatement(n):
    """The four forms against the meaning they share: on the ascending ring
    of N slots, slot k against slot k - K (K = N / 2 rounded down for one
    particle per lane; for two per lane, own upper slot against the lower
    slot of the lane N / 4, rounded down, lanes below), measured upwards
    from the partner round the ring."""
    L = 0.93 * n
    for row in six_rows(n, L, 0.3 * L, 11 + n)[:5]:
        z = np.sort(row)
        d = far_partner_distances(row, n, L)
        if n <= 64:
            k = np.arange(n)
            j = (k - n // 2) % n
        else:
            lanes = n // 2
            k = 2 * np.arange(lanes) + 1
            j = 2 * ((np.arange(lanes) - lanes // 2) % lanes)
        up = np.mod(z[k] - z[j], L)
        assert np.allclose(d, up, rtol=0, atol=1e-12 * L)
        for rm in (0.1 * L, 0.44 * L):
            assert takes_sorted_rows(row, n, L, rm) == bool(np.all(up < L - rm))


def test_odd_sizes_above_64_have_no_sorted_rows():
    # (an evenly spread row, which every even size takes)
    for n in (100, 101):
        row = np.arange(n) + 0.5
        assert takes_sorted_rows(row, n, float(n), 0.25 * n) is (n == 100)


@pytest.mark.parametrize('n', [33, 48, 64, 66, 100, 128])
def test_sort_restatement_sorts(n):
    """Rows in any order (the forced first yield takes the start row as it
    comes) end ascending within the bound; an ascending row takes no trip;
    one particle across either end of the box takes one."""
    rng = np.random.RandomState(n)
    for _ in range(20):
        z = n * rng.random_sample(n)
        trips, order = sort_slots(z, np.arange(n))
        assert trips is not None and trips <= (64 if n > 64 else 140)
        assert np.array_equal(z[order], np.sort(z))
    z = np.sort(z)
    assert sort_slots(z, np.arange(n))[0] == 0
    for moved, to in ((n - 1, 1e-3), (0, n - 1e-3)):
        y = z.copy()
        y[moved] = to
        trips, order = sort_slots(y, np.arange(n))
        assert trips == 1 and np.array_equal(y[order], np.sort(y))
