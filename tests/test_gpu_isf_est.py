"""The DMC imaginary-time density correlation estimator F(k, tau) on the GPU,
against the NumPy restatement (tests/_isf_restatement.py) on the states of a
twin ensemble, against the S(k) slot of the same ensemble at lag 0, and against
its exact rule in the free ideal gas.

Ensemble A and ensemble B start from the same positions with the same seed, so
they follow the same trajectory (test_gpu_sampling.py::
test_dmc_split_step_equals_block).  A runs one time step at a time and hands
out its State after each; B runs one estimator block.

The rounding bound of the comparison is `tolerance` of the restatement,
derived in its docstring.  At the largest value an entry can take, |x| =
nw N^2 (nw N), the suite's usual 2e-11 max(1, |x|) is above it for every shape
below (asserted): the worst, m = 63 at N = 16, has Q_m / N^2 = 5.9e-13.
"""
import functools
from itertools import islice
from typing import NamedTuple

import numpy as np
import pytest

from . import _dmc_walks as walks
from . import _isf_restatement as isf
from ._dmc_walks import EST, G2, TIME_STEP, WALKS
from ._models import box

pytestmark = pytest.mark.gpu


class Shape(NamedTuple):
    walk: str                   # of _dmc_walks.WALKS
    steps: int


class Case(NamedTuple):
    shape: str
    K: int
    T: int
    q: int


# An odd N below a wavefront; N = 16; N = 64 with more walkers than one pass
# of a block's wavefronts; N = 100, two chunks of 32 particles and a ragged
# third plus a tail; a population that starts at its cap; more live walkers
# than the launch has wavefronts (N = 37: two chunks, the second ragged), so
# that every wavefront goes round its slot loop again and rewrites its tables,
# its rho rows and its running sums.
SHAPES = {
    'odd':         Shape('odd', 8),
    'mid':         Shape('many', 6),
    'wave':        Shape('wave', 10),
    'two_pass':    Shape('two_pass', 6),
    'cap':         Shape('cap', 8),
    'second_trip': Shape('second_trip', 4),
}
KTQ = (8, 4, 2)
# Beyond the six shapes: the row limit K (T + 2) = 1024 (sixteen indices per
# lane, all 64 modes); one mode, one lag (a row of three doubles); a block
# that ends before lags 2 and 3 are reached.
CASES = {tag: Case(tag, *KTQ) for tag in SHAPES}
CASES.update({
    'limit': Case('mid', 64, 14, 1),
    'one':   Case('mid', 1, 1, 1),
    'short': Case('mid', 8, 4, 3),
})


def walk_of(shape):
    return WALKS[SHAPES[shape].walk]


def reference(shape):
    """Ensemble A's states of the block (recorded once per walk) -> dict."""
    return walks.record(SHAPES[shape].walk, SHAPES[shape].steps)


@functools.lru_cache(maxsize=None)
def restated(shape, K, T, q):
    rows = isf.isf_rows(reference(shape)['steps'], float(walk_of(shape).n),
                        K, T, q)
    rows.setflags(write=False)
    return rows


def run_block_b(shape, ktq=KTQ, eval_estimators=True, others=None, est=EST):
    """Ensemble B: one estimator block -> (series, ssf, dens, g2 rows, cm
    rows, isf rows); ktq None leaves the F(k, tau) slot off; `others` sets the
    other four estimators as well, 'before' or 'after' it."""
    nts = SHAPES[shape].steps
    eng = walks.engine(walk_of(shape))
    b = walks.ensemble(eng, walk_of(shape))
    if others == 'before':
        walks.set_others(b, est=est, cm=True)
    if ktq is not None:
        b.set_isf_estimator(*ktq)
    if others == 'after':
        walks.set_others(b, est=est, cm=True, reverse=True)
    ser, ssf, dens = b.run_block_est(nts, eval_estimators)
    g2 = b.read_pair_dist(nts) if others else None
    cmd = b.read_cm_diffusion(nts) if others else None
    rows = b.read_isf(nts) if ktq is not None else None
    b.close()
    eng.close()
    return ser, ssf, dens, g2, cmd, rows


@pytest.mark.parametrize('case', list(CASES))
def test_rows_equal_the_restatement(case):
    c = CASES[case]
    shape, K, T, q = c.shape, c.K, c.T, c.q
    n, nts = walk_of(shape).n, SHAPES[shape].steps
    ref = reference(shape)
    walks.assert_transport_exercised(ref, walk_of(shape), shape)
    for confs, _, nw in ref['steps']:
        assert confs[:nw].min() >= 0.0 and confs[:nw].max() <= n
    ser, _, _, _, _, rows = run_block_b(shape, (K, T, q))
    assert np.array_equal(ser.num_walkers, ref['num_walkers'])
    assert np.array_equal(ser.energy, ref['energy'])
    want = restated(shape, K, T, q)
    assert rows.shape == (nts, K, T + 2)
    tol = isf.tolerance(n, K, T, ref['num_walkers'])
    nw = ref['num_walkers'].astype(np.float64)[:, None, None]
    # the derivation gets below the suite's usual bound at full scale
    assert (tol[:, :, :T] <= 2e-11 * nw * n * n).all()
    assert (tol[:, :, T:] <= 2e-11 * nw * n).all()
    err = np.abs(rows - want)
    print(case, 'walkers', ref['num_walkers'], 'max err / tol',
          (err / tol).max(), 'max err', err.max(), 'max |x|',
          np.abs(want).max())
    assert (err <= tol).all(), np.argwhere(err > tol)[:8]
    # what has not been measured yet is exactly zero, what has is not
    for t in range(nts):
        measured = min(t // q, T - 1) + 1
        assert not rows[t][:, measured:T].any()
        assert rows[t][:, :measured].all()
    if case == 'short':
        assert not rows[:, :, 2:T].any() and rows[-1][:, :2].all()
    # m = 0: rho_0 = N whatever the positions
    for t in range(nts):
        measured = min(t // q, T - 1) + 1
        assert np.array_equal(rows[t, 0, :measured],
                              np.full(measured, nw[t, 0, 0] * n * n))
        assert rows[t, 0, T] == nw[t, 0, 0] * n and rows[t, 0, T + 1] == 0.0


@pytest.mark.parametrize('shape', ['mid', 'two_pass'])
def test_lag_zero_columns_against_the_ssf_slot(shape):
    """Columns 0, T, T+1 are the pure S(k) parts with a forward-walking
    length of one step (tests/test_isf_est_host.py has the identity on the
    CPU).  The kernel forms rho with code of its own, in the same way as the
    S(k) kernel: the bound of the module docstring holds between the two, the
    restatement's share of it to spare; whether they are equal to the bit is
    printed."""
    n, nts = walk_of(shape).n, SHAPES[shape].steps
    K, T, q = KTQ
    est = dict(num_modes=K, ssf_pure=True, ssf_pfw=1, num_bins=0)
    run = run_block_b(shape, KTQ, others='before', est=est)
    ssf, rows = run[1], run[5]
    assert ssf.shape == (nts, K, 3)
    tol = isf.tolerance(n, K, T, reference(shape)['num_walkers'])
    got = rows[:, :, [0, T, T + 1]]
    err = np.abs(got - ssf)
    print(shape, 'equal to the bit:', np.array_equal(got, ssf),
          'max err / tol', (err / tol[:, :, [0, T, T + 1]]).max())
    assert (err <= tol[:, :, [0, T, T + 1]]).all()


def test_deterministic_and_burn_in():
    shape = 'wave'
    nts = SHAPES[shape].steps
    r1 = run_block_b(shape)
    r2 = run_block_b(shape)
    assert r1[5].tobytes() == r2[5].tobytes()
    assert r1[5][-1][1:].all()                # (Im rho_0 is zero)
    # a burn-in block propagates the same walkers and leaves the rows zero
    r0 = run_block_b(shape, eval_estimators=False)
    assert r0[5].shape == (nts,) + (KTQ[0], KTQ[1] + 2) and not r0[5].any()
    walks.assert_same_series(r0[0], r1[0])


def test_the_walk_and_the_other_estimators_do_not_notice():
    shape = 'mid'
    alone = run_block_b(shape)
    off = run_block_b(shape, ktq=None)
    before = run_block_b(shape, others='before')
    after = run_block_b(shape, others='after')
    without = run_block_b(shape, ktq=None, others='before')
    for both in (before, after):
        assert both[5].tobytes() == alone[5].tobytes()
        for k in (1, 2, 3, 4):
            assert both[k].any()
            assert both[k].tobytes() == without[k].tobytes()
    assert alone[5][-1][:, :3].all()
    # the walk itself does not know about the estimator
    ref = reference(shape)
    for run in (alone, off, before, after, without):
        assert run[0].energy.tobytes() == ref['energy'].tobytes()
        assert np.array_equal(run[0].num_walkers, ref['num_walkers'])
        walks.assert_same_series(run[0], off[0])


def test_resetting_a_live_ensemble_equals_a_fresh_one():
    """Ensemble R has every estimator set, then F(k, tau) switched off and on
    again with another shape and the others set to other sizes; ensemble F is
    set once, to R's last configuration.  Same seed, same state, one estimator
    block each: every buffer of R was dropped and sized anew, so its rows are
    F's byte for byte."""
    from phd_qmclib_amd.engine import DmcEnsemble
    shape = 'mid'
    walk, nts = walk_of(shape), SHAPES[shape].steps
    eng = walks.engine(walk)
    runs = []
    for again in (True, False):                      # R, then F
        d = DmcEnsemble(eng, TIME_STEP, walk.maxw, walk.nw0, 0.5,
                        rng_seed=walk.seed)
        if again:
            d.set_estimators(num_modes=5, num_bins=0)
            d.set_isf_estimator(64, 14, 1)
            d.set_pair_dist_estimator(7)
            d.set_isf_estimator(0)
            d.set_cm_diffusion_estimator()
            d.set_isf_estimator(3, 2, 5)
        d.set_estimators(**EST)
        d.set_isf_estimator(*KTQ)
        d.set_cm_diffusion_estimator()
        d.set_pair_dist_estimator(**G2)
        d.set_state(walks.start_positions(walk))
        ser, ssf, dens = d.run_block_est(nts)
        runs.append((ser, ssf, dens, d.read_pair_dist(nts),
                     d.read_cm_diffusion(nts), d.read_isf(nts)))
        d.close()
    eng.close()
    r, f = runs
    walks.assert_same_series(r[0], f[0])
    for k in (1, 2, 3, 4, 5):
        assert r[k].tobytes() == f[k].tobytes() and r[k].any()
    assert r[5].shape == (nts, KTQ[0], KTQ[1] + 2)
    assert r[5].tobytes() == run_block_b(shape)[5].tobytes()


def test_switching_off_and_errors():
    from phd_qmclib_amd._lib import QmcError
    shape = 'odd'
    nts = SHAPES[shape].steps
    eng = walks.engine(walk_of(shape))
    d = walks.ensemble(eng, walk_of(shape))
    with pytest.raises(QmcError):
        d.read_isf(1)                        # the estimator is off
    for bad, what in (((65, 1, 1), 'num_modes'), ((-1, 1, 1), 'num_modes'),
                      ((4, 0, 1), 'num_lags'), ((4, 65, 1), 'num_lags'),
                      ((4, 4, 0), 'lag_stride'), ((4, 4, 2 ** 31), 'lag_stride'),
                      ((64, 15, 1), '1024'), ((16, 63, 1), '1024')):
        with pytest.raises(QmcError, match=what):
            d.set_isf_estimator(*bad)
        assert d.isf_shape is None
    d.set_isf_estimator(*KTQ)
    assert d.isf_shape == (KTQ[0], KTQ[1] + 2)
    with pytest.raises(QmcError):
        d.read_isf(1)                        # no estimator block yet
    d.run_block_est(nts)
    full = d.read_isf(nts)
    assert full[-1][1:].all()                # (Im rho_0 is zero)
    assert np.array_equal(d.read_isf(2), full[:2])
    with pytest.raises(QmcError):
        d.read_isf(nts + 1)
    with pytest.raises(QmcError):
        d.read_isf(0)
    # a failed setter leaves the estimator as it was
    with pytest.raises(QmcError):
        d.set_isf_estimator(4, 0, 1)
    assert np.array_equal(d.read_isf(nts), full)
    d.set_isf_estimator(0)
    assert d.isf_shape is None
    ser, ssf, dens = d.run_block_est(2)      # falls through to run_block
    assert ssf is None and dens is None and len(ser.energy) == 2
    with pytest.raises(QmcError):
        d.read_isf(1)
    d.close()
    eng.close()


def test_distributed_dmc_refuses_the_estimator():
    walks.assert_refused_by_distributed(
        walk_of('mid'), lambda d: d.set_isf_estimator(*KTQ),
        lambda d: d.set_isf_estimator(0), r'F\(k, tau\)')


# ---- top level ------------------------------------------------------------
def test_sampling_blocks_fill_iter_isf():
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    confs = np.zeros((48, 2, 16))
    confs[:, 0, :] = walks.start_positions(walk_of('mid'))
    kw = dict(max_num_walkers=64, target_num_walkers=48, rng_seed=13)
    plain = mrbp_qmc.dmc.Sampling(spec, TIME_STEP, **kw)
    with_isf = mrbp_qmc.dmc.Sampling(
        spec, TIME_STEP, isf_est_spec=mrbp_qmc.dmc.ISFEstSpec(*KTQ), **kw)
    ini = plain.build_state(confs)
    b0 = list(islice(plain.blocks(ini, 6, 0), 2))
    b1 = list(islice(with_isf.blocks(ini, 6, 1), 2))
    for p, q in zip(b0, b1):
        assert p.iter_isf is None and p.iter_pair_dist is None
        assert q.iter_density is None and q.iter_ssf is None
        assert q.iter_pair_dist is None and q.iter_cm_diffusion is None
        assert q.iter_isf.shape == (6, KTQ[0], KTQ[1] + 2)
        assert p.iter_props.energy.tobytes() == q.iter_props.energy.tobytes()
    assert not b1[0].iter_isf.any()                  # the burn-in block
    kept = b1[1].iter_isf
    assert kept[0][:, [0, 4, 5]].any() and not kept[0][:, 1:4].any()
    assert kept[-1][:, :3].all() and not kept[-1][:, 3].any()
    # the first block of a run equals the twin's block
    first = list(islice(with_isf.blocks(ini, 6, 0), 1))[0].iter_isf
    assert first.tobytes() == run_block_b('mid')[5].tobytes()


def test_proc_exec_yields_isf_blocks():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.engine import intermediate_scattering
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    dx = mrbp_qmc.dmc_exec
    spec = box(16)
    np.random.seed(5)
    K, T, q = 6, 4, 4
    kw = dict(max_num_walkers=512, target_num_walkers=480, rng_seed=7,
              num_blocks=4, num_time_steps_block=16, burn_in_blocks=1)
    on = dx.Proc(spec, TIME_STEP, isf_spec=dx.ISFEstSpec(K, T, q), **kw)
    din = dx.ProcInput.from_model_sys_conf_spec(
        dx.ModelSysConfSpec('RANDOM'), on)
    res = on.exec(din)
    blocks = res.data.blocks.isf
    assert isinstance(blocks, dd.ISFBlocks)
    assert blocks.totals.shape == (4, K, T + 2) and res.data.series is None
    assert np.isfinite(blocks.totals).all()
    assert np.array_equal(blocks.totals[:, 0, :T], np.full((4, T), 256.0))
    tau, f, err, conn = blocks.scattering_function(spec, TIME_STEP, q)
    assert np.array_equal(tau, np.arange(T) * q * TIME_STEP)
    assert f.shape == err.shape == conn.shape == (T, K)
    assert np.isfinite(f).all() and np.isfinite(conn).all()
    assert (f[0] > 0).all()                          # lag 0 is S(k)
    kres = dx.Proc(spec, TIME_STEP, keep_iter_data=True,
                   isf_spec=dx.ISFEstSpec(K, T, q), **kw).exec(din)
    kept = kres.data.series.isf_blocks
    assert kept.shape == (4, 16, K, T + 2)
    nw = kres.data.series.iter_props_blocks.num_walkers
    assert np.array_equal(kres.data.blocks.isf.totals,
                          kept[:, -1] / nw[:, -1][:, None, None])
    assert np.array_equal(kres.data.blocks.isf.totals, blocks.totals)
    _, f0, rho0 = intermediate_scattering(kept[0], nw[0], 16, TIME_STEP, q)
    assert np.array_equal(f0, blocks.totals[0][:, :T].T / 16)
    assert np.array_equal(rho0.real, blocks.totals[0][:, T])
    # the walk is the same with and without the estimator
    off = dx.Proc(spec, TIME_STEP, **kw).exec(din)
    assert off.data.blocks.isf is None
    assert np.array_equal(off.data.blocks.energy.totals,
                          res.data.blocks.energy.totals)
    assert np.array_equal(off.data.blocks.energy.weight_totals,
                          res.data.blocks.energy.weight_totals)


# ---- the exact rule -------------------------------------------------------
def test_free_ideal_gas_decays_as_exp_minus_k_squared_tau():
    """lattice_depth = 0 and interaction_strength = 0: psi_T = 1, no drift,
    unit weights; every particle diffuses with variance 2 tau.  From a uniform
    random start E[iter[t][m][l]] / nw = N exp(-k_m^2 tau_l) for m >= 1 and
    N^2 for m = 0, at any time step.

    N = L = 8, dt = 1e-2, K = 4, T = 4, q = 8, target 2048 / cap 2560 walkers,
    seed 21, one burn-in block and 16 kept blocks of 32 steps, read at the
    last step of each.  The blocks restart the origin; the error of the mean
    is the scatter of the 16 values over sqrt(16).  Asserted for every
    (m >= 1, l >= 1): |mean - N exp(-k^2 tau)| <= 4 stderr and stderr <= 0.08,
    1 % of N.  The same workload through the CPU oracle's DMC and the
    restatement: stderr 0.013 - 0.036; F(k_1, 0.08) = 7.621 +- 0.015 against
    7.615, F(k_2, 0.16) = 5.385 +- 0.030 against 5.391, F(k_3, 0.24) =
    2.135 +- 0.031 against 2.111; largest deviation 1.6 stderr; the cloning
    table is the identity and the population 2048 throughout.
    """
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.engine import intermediate_scattering
    n, nts, nblocks, dt = 8, 32, 16, 1e-2
    K, T, q = 4, 4, 8
    spec = box(n, depth=0, gint=0)
    pos = n * np.random.RandomState(21).random_sample((2048, n))
    smp = mrbp_qmc.dmc.Sampling(
        spec, dt, max_num_walkers=2560, target_num_walkers=2048, rng_seed=21,
        isf_est_spec=mrbp_qmc.dmc.ISFEstSpec(K, T, q))
    confs = np.zeros((2048, 2, n))
    confs[:, 0, :] = pos
    blocks = list(islice(smp.blocks(smp.build_state(confs), nts, 1),
                         1 + nblocks))
    assert not blocks[0].iter_isf.any()
    curves = []
    for b in blocks[1:]:
        tau, f, rho = intermediate_scattering(
            b.iter_isf, b.iter_props.num_walkers, n, dt, q)
        curves.append(f * n)                        # F itself, [T, K]
    curves = np.array(curves)
    assert np.array_equal(tau, np.arange(T) * q * dt)
    mean = curves.mean(axis=0)
    stderr = curves.std(axis=0, ddof=1) / np.sqrt(nblocks)
    want = n * np.exp(-np.outer(tau, smp.isf_momenta ** 2))
    print('population', sorted({int(x) for b in blocks
                                for x in b.iter_props.num_walkers}))
    for arr in (mean, stderr, want):
        print(np.array2string(arr, precision=4, suppress_small=True))
    assert np.allclose(mean[:, 0], n * n, rtol=1e-13)
    assert (stderr[1:, 1:] <= 0.08).all()
    assert (np.abs(mean - want)[1:, 1:] <= 4 * stderr[1:, 1:]).all()
