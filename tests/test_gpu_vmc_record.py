"""The per-chain record of the VMC step (log|psi|, carried energy, block sums
in one 64-byte word group per chain) against what the C ABI hands out: the
compact arrays of get_state / block_sums_dev and the sums of run_block, after
blocks of several yields -- the first yield of a block runs the general LEAN
kernel, the later ones its steady-state variant -- compared bit for bit with
the per-step series of the non-LEAN kernel on the same stream."""

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu


def device_sums(ens, W):
    import torch
    from phd_qmclib_amd.dist import _wrap_f64, _wrap_i64
    ens.engine.sync()
    dev = torch.device('cuda', 0)
    p_e, p_e2, p_acc = ens.block_sums_dev()
    return (_wrap_f64(p_e, W, dev).cpu().numpy().copy(),
            _wrap_f64(p_e2, W, dev).cpu().numpy().copy(),
            _wrap_i64(p_acc, W, dev).cpu().numpy().copy())


# N = 64: one chain per wavefront, the headline shape; N = 100: two particles
# per lane, padded; N = 16: four chains per wavefront
@pytest.mark.parametrize('n', [64, 100, 16])
def test_record_matches_series(n):
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n)
    spread = 0.25 * spec.well_width
    W, ny, blocks = 96, 6, 3
    pos = n * np.random.RandomState(500 + n).random_sample((W, n))
    eng = ModelEngine(spec.cfc_spec, device=0)
    lean = VmcEnsemble(eng, W, spread, rng_seed=21)
    full = VmcEnsemble(eng, W, spread, rng_seed=21)
    try:
        _compare_blocks(lean, full, pos, W, ny, blocks)
    finally:
        lean.close(); full.close(); eng.close()


def _compare_blocks(lean, full, pos, W, ny, blocks):
    lean.set_state(pos)
    full.set_state(pos)
    for _ in range(blocks):
        a = lean.run_block(ny)
        b = full.run_block(ny, series=True)
        for k in ('sum_energy', 'sum_energy2', 'num_accepted'):
            assert np.array_equal(a[k], b[k]), k
        # the sums of the block are those of its series, in yield order
        se = np.zeros(W)
        for y in range(ny):
            se = se + b['energy'][y]
        assert np.array_equal(a['sum_energy'], se)
        assert np.array_equal(a['num_accepted'], b['move_stat'].sum(axis=0))
        # the device copies of the C ABI hold the same sums
        d_e, d_e2, d_acc = device_sums(lean, W)
        assert np.array_equal(d_e, a['sum_energy'])
        assert np.array_equal(d_e2, a['sum_energy2'])
        assert np.array_equal(d_acc, a['num_accepted'])
        # log|psi| and the carried energy of the last yield
        pa, wa, ea = lean.get_state()
        pb, wb, eb = full.get_state()
        assert np.array_equal(pa, pb)
        assert np.array_equal(wa, b['wf_abs_log'][-1])
        assert np.array_equal(ea, b['energy'][-1])
        assert np.array_equal(wb, wa) and np.array_equal(eb, ea)
    # a block without sums read back leaves the same device sums
    lean.run_block(ny, sums=False)
    b = full.run_block(ny, series=True)
    d_e, d_e2, d_acc = device_sums(lean, W)
    assert np.array_equal(d_e, b['sum_energy'])
    assert np.array_equal(d_e2, b['sum_energy2'])
    assert np.array_equal(d_acc, b['num_accepted'])


@pytest.mark.parametrize('n', [64, 16])
def test_set_state_round_trip(n):
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n)
    spread = 0.25 * spec.well_width
    W = 64
    pos = n * np.random.RandomState(700 + n).random_sample((W, n))
    eng = ModelEngine(spec.cfc_spec, device=0)
    v = VmcEnsemble(eng, W, spread, rng_seed=5)
    u = VmcEnsemble(eng, W, spread, rng_seed=5)
    try:
        v.set_state(pos)
        p0, w0, e0 = v.get_state()
        assert np.array_equal(p0, pos)
        # (set_state evaluates the rows in position order: to rounding)
        assert np.allclose(w0, eng.evaluate(pos).wf_abs_log, rtol=1e-12,
                           atol=1e-12)
        assert not e0.any()
        v.run_block(7)
        p1, w1, e1 = v.get_state()
        # the state read back, set again: same configuration, log|psi| of it
        u.set_state(p1)
        p2, w2, e2 = u.get_state()
        assert np.array_equal(p2, p1)
        assert np.allclose(w2, w1, rtol=1e-12, atol=1e-12)
        # the first yield of the new ensemble is its initial state: that
        # state's log|psi| and energy
        r = u.run_block(1, series=True)
        assert np.allclose(r['wf_abs_log'][0], w1, rtol=1e-12, atol=1e-12)
        assert np.allclose(r['energy'][0], e1, rtol=1e-12, atol=1e-12)
        assert r['move_stat'][0].all()
    finally:
        # (ensembles before their engine, whatever failed)
        v.close(); u.close(); eng.close()
