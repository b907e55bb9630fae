"""Single-particle VMC sweeps, the parts that need no GPU: the move codes, the
acceptance rate of an `EnsembleBlock` of sweeps, and the restatement
(tests/_vmc_sweep_restatement.py) the GPU tests compare the device with --
its log-ratio against the oracle's full log|psi| and the margin condition of
every case of tests/_vmc_sweep_cases.py."""
import numpy as np
import pytest

from . import _vmc_sweep_cases as sc
from . import _vmc_sweep_restatement as rs

CASES = [(cid, sp) for cid in sc.IDS for sp in sc.SPREADS]


def test_vmc_move_code():
    from phd_qmclib_amd.engine import vmc_move_code
    assert vmc_move_code('all') == 0
    assert vmc_move_code('particle') == 2
    for bad in ('gaussian', 'sweep', '', None, 2, b'all'):
        with pytest.raises(ValueError):
            vmc_move_code(bad)


def test_ensemble_block_accept_rate():
    from phd_qmclib_amd.qmc_base.vmc import EnsembleBlock
    se, se2 = np.array([8.0, 12.0]), np.array([20.0, 40.0])
    na = np.array([2, 3])
    b3 = EnsembleBlock(se, se2, na, 4)
    assert b3.moves_per_step == 1
    assert np.array_equal(b3.accept_rate, [0.5, 0.75])
    assert np.array_equal(b3.energy, [2.0, 3.0])
    kw = EnsembleBlock(sum_energy=se, sum_energy2=se2, num_accepted=na,
                       num_steps=4)
    assert np.array_equal(kw.accept_rate, b3.accept_rate)
    sweeps = EnsembleBlock(se, se2, np.array([32, 48]), 4, 16)
    assert sweeps[-1] == 16 and sweeps.moves_per_step == 16
    assert np.array_equal(sweeps.accept_rate, [0.5, 0.75])
    assert np.array_equal(sweeps.energy, [2.0, 3.0])


@pytest.mark.parametrize('cid,spread', CASES)
def test_restated_ratio_is_the_difference_of_full_sums(oracle, cid, spread):
    """D of every move against oracle.wf_abs_log(R') - oracle.wf_abs_log(R):
    1e-9 covers the cancellation in the difference of two full sums."""
    _, m, _ = sc.model_of(oracle, cid)
    ref = sc.reference(oracle, cid, spread)
    worst = 0.0
    for c in range(sc.W):
        # yield y + 1 is the row after sweep y
        for y in range(sc.NYIELD - 1):
            row = ref['pos'][y, c].copy()
            wf = oracle.wf_abs_log(m, row)
            for k in range(row.size):
                trial = row.copy()
                trial[k] = ref['proposal'][y, c, k]
                wf_t = oracle.wf_abs_log(m, trial)
                worst = max(worst, abs(ref['delta'][y, c, k] - (wf_t - wf)))
                if ref['accepted'][y, c, k]:
                    row, wf = trial, wf_t
            assert np.array_equal(row, ref['pos'][y + 1, c])
    print(cid, spread, 'worst |D - (wf(R\') - wf(R))|', worst)
    assert worst <= 1e-9


@pytest.mark.parametrize('cid,spread', CASES)
def test_margins_allow_identical_decisions(oracle, cid, spread):
    ref = sc.preconditions(oracle, cid, spread)
    n = ref['pos'].shape[2]
    assert ref['margin'].shape == (sc.NYIELD - 1, sc.W, n)
    assert ref['margin'].size < 5000
    print(cid, spread, 'smallest |margin| %.2e' % np.abs(ref['margin']).min(),
          'accepted %.3f' % ref['accepted'].mean())
    # both outcomes occur, the yields say so, rejected moves leave the row
    assert ref['accepted'].any() and not ref['accepted'].all()
    assert np.array_equal(ref['move_stat'][1:], ref['accepted'].any(axis=2))
    moved = ref['pos'][1:] != ref['pos'][:-1]
    assert not np.any(moved & ~ref['accepted'])


def test_hard_moves_are_in_the_cases(oracle):
    """At spread 0.75 particles cross the box edge and pairs change class."""
    ref = sc.reference(oracle, 'box16', 0.75)
    L = 16.0
    jump = np.abs(ref['pos'][1:] - ref['pos'][:-1])
    assert np.any(jump > 0.5 * L)
    rows = sc.start_rows('box16')
    assert np.array_equal(ref['pos'][0], rows)


def test_restatement_is_keyed_by_slot(oracle):
    """Chain c of an ensemble at chain0 = 0 is chain 0 of one at chain0 = c."""
    cfc, m, p = sc.model_of(oracle, 'box9')
    rows = sc.start_rows('box9')
    a = rs.Chain(oracle, m, p, rows[3], 0.75, 5, 3).run(4)
    b = rs.run_ensemble(oracle, m, p, rows[3:4], 0.75, 5, 4, chain0=3)
    assert np.array_equal(a['pos'], b['pos'][:, 0])
    # ... and a block in two parts is the block
    ch = rs.Chain(oracle, m, p, rows[3], 0.75, 5, 3)
    two = np.concatenate([ch.run(1)['pos'], ch.run(3)['pos']])
    assert np.array_equal(a['pos'], two)
