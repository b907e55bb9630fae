"""The fused steady VMC launch after its per-launch accept thresholds
(vmc_accept_thresholds in qmc_kernels.h: lane l of the wavefront draws and
takes the logarithm of the accept uniform of yield l, 64 yields at a time)
against the series kernel of the same stream, which draws and tests yield by
yield -- bit for bit: positions, log|psi|, carried energy, the three block sums
and the general-path counter.  Blocks long enough to refill the thresholds,
chains that leave and re-enter the sorted-row path inside a launch, models
whose pair sums or one-body factor take other branches, and the padded shape.
The move spread here is exactly 0.125 (a quarter of the well width), at which
the product vmc_move_unit * move_spread is exact; the spreads at which it
rounds are in tests/test_gpu_generic_steps.py."""

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu

# 200 chains: not a multiple of the 128-workgroup rounding of the grid
W = 200


def lattice(n, seed):
    # one particle per well, jittered: the sorted-row path
    rng = np.random.RandomState(seed)
    return np.arange(n)[None, :] + 0.25 + 0.3 * (rng.random_sample((W, n)) - 0.5)


def packed(n, npack, seed):
    """The first half of the chains with `npack` particles uniform in
    [0, 0.2 L) and the rest over the box, the second half on the lattice."""
    rng = np.random.RandomState(seed)
    pos = lattice(n, seed + 1)
    h = W // 2
    pos[:h, :npack] = 0.2 * n * rng.random_sample((h, npack))
    pos[:h, npack:] = n * rng.random_sample((h, n - npack))
    return pos


def lean_against_series(spec, pos, blocks, seed):
    """Runs `blocks` (yields per block) on a LEAN and on a series ensemble of
    the same seed and compares everything after every block; -> the counter of
    the general path per block."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spread = 0.25 * spec.well_width
    eng = ModelEngine(spec.cfc_spec, device=0)
    lean = VmcEnsemble(eng, W, spread, rng_seed=seed)
    full = VmcEnsemble(eng, W, spread, rng_seed=seed)
    general = []
    try:
        lean.set_state(pos)
        full.set_state(pos)
        for b in blocks:
            eng.general_path_walkers(reset=True)
            x = lean.run_block(b)
            g_lean = eng.general_path_walkers(reset=True)
            y = full.run_block(b, series=True)
            g_full = eng.general_path_walkers(reset=True)
            for k in ('sum_energy', 'sum_energy2', 'num_accepted'):
                assert np.array_equal(x[k], y[k]), (k, b)
            assert g_lean == g_full, b
            general.append(g_lean)
            pa, wa, ea = lean.get_state()
            pb, wb, eb = full.get_state()
            assert np.array_equal(pa, pb), b
            assert np.array_equal(wa, wb), b
            assert np.array_equal(ea, eb), b
            assert np.array_equal(wa, y['wf_abs_log'][-1]), b
            assert np.array_equal(ea, y['energy'][-1]), b
    finally:
        lean.close(); full.close(); eng.close()
    return general


# the steady launch of a block of b yields runs b - 1 of them: 65 -> the 64
# thresholds of one fill exactly, 66 -> one yield after the refill, 130 -> two
# refills.  Three blocks in a row: the first starts with the forced yield.
@pytest.mark.parametrize('n,b', [(64, 65), (64, 66), (64, 130), (128, 66)])
def test_threshold_refill(n, b):
    lean_against_series(box(n), lattice(n, 300 + n + b), [b] * 3, seed=51)


# Chains that leave the sorted-row path and come back inside a launch: a
# packed chain has its farthest partner beyond L - r_m (r_m = L / 4 here) and
# spreads out as it moves; the lattice chains never leave the path.  40 packed
# particles trip the counter at both sizes (measured, yields on the general
# path in each of the four blocks of 16: all 1600 of the 100 packed chains at
# N = 64, about 840 of them at N = 128, where the 40 are a smaller share of
# the row).
@pytest.mark.parametrize('n,npack', [(64, 40), (128, 40)])
@pytest.mark.parametrize('b', [16, 17])
def test_leaves_and_reenters_sorted_path(n, npack, b):
    g = lean_against_series(box(n), packed(n, npack, 700 + n + b), [b] * 4,
                            seed=52)
    assert g[0] > 0


# Models whose steps take other branches of the same kernel: no lattice (no
# one-body factor), no interaction (the general pair sums, never the sorted
# rows) and barriers of two heights (the one-body constants per particle).
@pytest.mark.parametrize('kw', [dict(lattice_depth=0),
                                dict(interaction_strength=0),
                                dict(num_defects=4, defect_magnitude=25)],
                         ids=['free', 'ideal', 'defects'])
def test_other_model_classes(kw):
    spec = box(64, **kw)
    lean_against_series(spec, lattice(64, 811), [17] * 2, seed=53)


@pytest.mark.parametrize('b', [2, 16, 66])
def test_padded_48(b):
    lean_against_series(box(48), lattice(48, 900 + b), [b] * 2, seed=54)
