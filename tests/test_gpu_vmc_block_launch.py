"""A production (LEAN) block of the VMC stepper against the series kernel.

On the sorted-row shapes (33 <= N <= 128) a LEAN `run_block` is ONE launch of
the fused steady kernel for all its yields: the kernel zeroes the block sums
at its record load, and it draws the accept thresholds of 32 yields at a time,
half a wavefront per particle.  Only the forced initial yield of a generator
still takes the per-yield kernel, and the fused launch that follows it in the
same block carries that yield's sums on.  `series=True` runs the tape-pinned
per-yield kernel, one launch per yield, with the accept draw taken in the
yield: two ensembles with the same seed and start run the same schedule of
blocks, one each way, and after EVERY block the positions, log|psi|, the
carried energy and the three block sums are the same to the bit.

Schedules (yields per block; the first block of a schedule is the first of a
generator -- forced yield, then a fused launch that must not reset the sums;
every later block starts its sums from zero, and consecutive later blocks
follow each other):
  LONG   16, 1, 2, 16, 33, 65, 130   (33, 65 and 130 cross the 32-yield refill)
  FIRST1 1, 130, 65                  (the forced yield alone; then later blocks)
  FIRST34 34, 33, 2                  (the launch after the forced yield refills)
N = 64, 63, 48, 33: one particle per lane, unpadded and padded.  N = 128, 66:
two per lane.  N = 32, 130: shapes without a fused kernel (controls), N = 1 as
well (on a fused shape the draw takes both words from particle 0 when N = 1;
no shape that the library picks holds a single particle, the per-yield rule
is what runs).  256 chains: more than one workgroup.  The benchmark box and
the free model.  The edge ensemble of tests/test_gpu_vmc_fused_hoist.py has
chains that leave and re-enter the sorted-row path between yields.  A move
spread just below and just above twice the box length, and 3 L, where the
periodic wrap takes its wide-excursion path."""

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu

W = 256
SEED = 67
MODELS = {'box': {}, 'free': dict(lattice_depth=0)}
LONG = (16, 1, 2, 16, 33, 65, 130)
FIRST1 = (1, 130, 65)
FIRST34 = (34, 33, 2)


def lattice(n, seed, w=W):
    # one particle per well, jittered: the sorted-row path
    rng = np.random.RandomState(seed)
    return np.arange(n)[None, :] + 0.25 + 0.3 * (rng.random_sample((w, n)) - 0.5)


def edge(n, seed):
    """tests/test_gpu_vmc_fused_hoist.py: even chains with the farthest
    partner of the rotation at L - r_m give or take less than a move -- the
    once-per-walker test of the sorted-row path fails in some yields and holds
    in others.  Odd chains: the lattice."""
    rng = np.random.RandomState(seed)
    pos = lattice(n, seed + 1)
    m = n // 2 + 1
    for w in range(0, W, 2):
        arc = 0.25 * n + 0.08 * (rng.random_sample() - 0.5)
        z0 = 0.75 * n * rng.random_sample()
        pos[w, :m] = z0 + arc * np.arange(m) / (m - 1)
        pos[w, m:] = z0 + arc + (n - arc) * np.arange(1, n - m + 1) / (n - m + 1)
    return pos % n


def run_pair(n, model, schedule, start=lattice, spread=None):
    """Both ensembles through `schedule`; asserts equality after every block.
    -> (general-path count of the LEAN engine, accepted moves, yields)."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n, **MODELS[model])
    spread = 0.25 * spec.well_width if spread is None else spread
    pos = start(n, 700 + n)
    engs = [ModelEngine(spec.cfc_spec, device=0) for _ in range(2)]
    vs = [VmcEnsemble(e, W, spread, rng_seed=SEED) for e in engs]
    try:
        for v in vs:
            v.set_state(pos)
        for e in engs:
            e.general_path_walkers(reset=True)
        accepted = 0
        for b, k in enumerate(schedule):
            lean = vs[0].run_block(k)
            full = vs[1].run_block(k, series=True)
            where = f'N={n} {model} block {b} of {schedule}'
            for name, x, y in zip(('pos', 'wf', 'ecarry'), vs[0].get_state(),
                                  vs[1].get_state()):
                assert np.array_equal(x, y), f'{name}: {where}'
            for name in ('sum_energy', 'sum_energy2', 'num_accepted'):
                assert np.array_equal(lean[name], full[name]), f'{name}: {where}'
            # (the series kernel's own record of the block: its sums are those
            # of the yields of THIS block alone)
            assert np.array_equal(full['num_accepted'],
                                  full['move_stat'].sum(axis=0)), where
            accepted += int(lean['num_accepted'].sum())
        general = [e.general_path_walkers(reset=True) for e in engs]
        assert general[0] == general[1]
    finally:
        for v in vs:
            v.close()
        for e in engs:
            e.close()
    return general[0], accepted, W * sum(schedule)


@pytest.mark.parametrize('model', list(MODELS))
@pytest.mark.parametrize('n', [64, 63, 48, 33, 128, 66, 32, 130])
def test_lean_blocks_match_series_kernel(n, model):
    _, accepted, yields = run_pair(n, model, LONG)
    # moves were accepted and moves were rejected: both arms of a yield ran
    assert W * len(LONG) < accepted < yields


@pytest.mark.parametrize('schedule', [FIRST1, FIRST34], ids=['first1', 'first34'])
@pytest.mark.parametrize('n', [64, 48, 128])
def test_first_block_of_a_generator(n, schedule):
    run_pair(n, 'box', schedule)


@pytest.mark.parametrize('n', [64, 48])
def test_leaves_and_reenters_sorted_path(n):
    general, _, _ = run_pair(n, 'box', (16, 65, 16, 33), start=edge)
    # the general path did run, and not in every yield of the chains at the
    # edge (the lattice chains never take it)
    assert general > 0
    assert general < 130 * (W // 2)


@pytest.mark.parametrize('factor', [2 * (1 - 2.0 ** -10), 2 * (1 + 2.0 ** -10), 3.0],
                         ids=['below2L', 'above2L', '3L'])
@pytest.mark.parametrize('model', list(MODELS))
@pytest.mark.parametrize('n', [64, 66])
def test_move_spread_around_two_box_lengths(n, model, factor):
    run_pair(n, model, (16, 33, 2), spread=factor * n)


def test_single_particle():
    run_pair(1, 'free', (16, 1, 33, 65))
    run_pair(1, 'box', (16, 1, 33, 65))
