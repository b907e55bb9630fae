"""The fused steady VMC launch (one launch runs every yield of a block after the
first, VmcFused in qmc_kernels.h) against the per-yield kernels, bit for bit:
LEAN blocks of several yields against the series kernel of the same stream
(one launch per yield) and against blocks of one yield each, right after
set_state and later; positions, labels (through the positions handed back in
particle order), log|psi|, carried energy, block sums and accept counts; the
general-path counter; and a DMC ensemble built from a fused block.  The move
spread here is exactly 0.125 (a quarter of the well width), at which the
product vmc_move_unit * move_spread is exact; the spreads at which it rounds
are in tests/test_gpu_generic_steps.py."""

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


def same_state(u, v):
    pa, wa, ea = u.get_state()
    pb, wb, eb = v.get_state()
    assert np.array_equal(pa, pb)
    assert np.array_equal(wa, wb)
    assert np.array_equal(ea, eb)


# N = 64: the headline shape; N = 48: padded; N = 128: two particles per
# lane; N = 99: two per lane, odd (the general pair sums inside the loop)
@pytest.mark.parametrize('n', [64, 48, 128, 99])
@pytest.mark.parametrize('b', [1, 2, 16, 17])
def test_fused_block_matches_series(n, b):
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n)
    spread = 0.25 * spec.well_width
    pos = lattice(n, 900 + n + b)
    eng = ModelEngine(spec.cfc_spec, device=0)
    lean = VmcEnsemble(eng, W, spread, rng_seed=33)
    full = VmcEnsemble(eng, W, spread, rng_seed=33)
    try:
        lean.set_state(pos)
        full.set_state(pos)
        # the first block starts with the forced initial yield, the later
        # ones with a real move
        for _ in range(3):
            eng.general_path_walkers(reset=True)
            x = lean.run_block(b)
            g_lean = eng.general_path_walkers(reset=True)
            y = full.run_block(b, series=True)
            g_full = eng.general_path_walkers(reset=True)
            for k in ('sum_energy', 'sum_energy2', 'num_accepted'):
                assert np.array_equal(x[k], y[k]), k
            assert g_lean == g_full
            same_state(lean, full)
            _, wf, ec = lean.get_state()
            assert np.array_equal(wf, y['wf_abs_log'][-1])
            assert np.array_equal(ec, y['energy'][-1])
    finally:
        lean.close(); full.close(); eng.close()


@pytest.mark.parametrize('n', [64, 48, 128])
@pytest.mark.parametrize('b', [2, 16, 17])
def test_fused_block_matches_single_yields(n, b):
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n)
    spread = 0.25 * spec.well_width
    pos = n * np.random.RandomState(40 + n + b).random_sample((W, n))
    eng = ModelEngine(spec.cfc_spec, device=0)
    fused = VmcEnsemble(eng, W, spread, rng_seed=8)
    single = VmcEnsemble(eng, W, spread, rng_seed=8)
    try:
        fused.set_state(pos)
        single.set_state(pos)
        for _ in range(2):
            x = fused.run_block(b)
            se = np.zeros(W)
            se2 = np.zeros(W)
            na = np.zeros(W, dtype=np.int64)
            for _ in range(b):
                r = single.run_block(1)
                se = se + r['sum_energy']
                se2 = se2 + r['sum_energy2']
                na = na + r['num_accepted']
            # (the block adds every yield's energy in yield order, as here;
            # its squares go through a fused multiply-add)
            assert np.array_equal(x['sum_energy'], se)
            assert np.allclose(x['sum_energy2'], se2, rtol=1e-13, atol=0)
            assert np.array_equal(x['num_accepted'], na)
            same_state(fused, single)
    finally:
        fused.close(); single.close(); eng.close()


def test_dmc_from_fused_block():
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    n = 64
    spec = box(n)
    spread = 0.25 * spec.well_width
    pos = lattice(n, 77)
    eng = ModelEngine(spec.cfc_spec, device=0)
    lean = VmcEnsemble(eng, W, spread, rng_seed=2)
    full = VmcEnsemble(eng, W, spread, rng_seed=2)
    ds = []
    try:
        lean.set_state(pos)
        full.set_state(pos)
        lean.run_block(16)
        full.run_block(16, series=True)
        lean.run_block(9)
        full.run_block(9, series=True)
        same_state(lean, full)
        sers = []
        for v in (lean, full):
            d = DmcEnsemble(eng, 6.25e-4, 512, 256, 0.5, rng_seed=3)
            ds.append(d)
            d.set_state_from_vmc(v, 256, replicate=True)
            sers.append(d.run_block(6))
        a, c = sers
        assert np.array_equal(a.energy, c.energy)
        assert np.array_equal(a.num_walkers, c.num_walkers)
        assert np.array_equal(a.weight, c.weight)
    finally:
        for d in ds:
            d.close()
        lean.close(); full.close(); eng.close()
