"""The DMC centre-of-mass diffusion estimator (superfluid fraction) on the GPU,
against the NumPy restatement (tests/_cmdiff_restatement.py) on the states of a
twin ensemble, and against its exact rule in a translation invariant system.

Ensemble A and ensemble B start from the same positions with the same seed, so
they follow the same trajectory (test_gpu_sampling.py::
test_dmc_split_step_equals_block).  A runs one time step at a time and hands
out its State after each; B runs one estimator block.  The rounding bound of
the comparison is `tolerance` of the restatement, derived in its docstring;
nothing is fitted to what the kernel gives.
"""
import functools
from itertools import islice
from typing import NamedTuple

import numpy as np
import pytest

from . import _cmdiff_restatement as cm
from . import _dmc_walks as walks
from ._dmc_walks import EST, G2, TIME_STEP, WALKS
from ._models import box

pytestmark = pytest.mark.gpu


class Case(NamedTuple):
    walk: str                   # of _dmc_walks.WALKS
    steps: int


# An odd N below a wavefront; N = 16; N = 64, one index per lane, with more
# walkers than one pass of a block's wavefronts; N = 100, two passes over the
# indices; a population that starts at its cap; more live walkers than the
# launch has wavefronts, so that every wavefront goes round its slot loop
# again.
CASES = {
    'odd':         Case('odd', 8),
    'mid':         Case('many', 6),
    'wave':        Case('wave', 10),
    'two_pass':    Case('two_pass', 6),
    'cap':         Case('cap', 8),
    'second_trip': Case('second_trip', 4),
}


def walk_of(tag):
    return WALKS[CASES[tag].walk]


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Ensemble A's states of the block and the restatement's rows on them,
    computed once per case -> dict."""
    rec = walks.record(CASES[tag].walk, CASES[tag].steps)
    L = float(walk_of(tag).n)
    rows, wrapped, max_d = cm.cm_diffusion(rec['steps'], L)
    rows.setflags(write=False)
    return dict(rec, rows=rows, wrapped=wrapped, max_d=max_d,
                max_y=cm.largest_y(rec['steps'], L))


def run_block_b(tag, on=True, eval_estimators=True, others=None):
    """Ensemble B: one estimator block -> (series, ssf, dens, g2 rows, cm
    rows); `others` sets S(k), the density and g2 as well, 'before' or 'after'
    the centre-of-mass diffusion."""
    T = CASES[tag].steps
    eng = walks.engine(walk_of(tag))
    b = walks.ensemble(eng, walk_of(tag))
    if others == 'before':
        walks.set_others(b)
    if on:
        b.set_cm_diffusion_estimator()
    if others == 'after':
        walks.set_others(b, reverse=True)
    ser, ssf, dens = b.run_block_est(T, eval_estimators)
    g2 = b.read_pair_dist(T) if others else None
    rows = b.read_cm_diffusion(T) if on else None
    b.close()
    eng.close()
    return ser, ssf, dens, g2, rows


@pytest.mark.parametrize('tag', list(CASES))
def test_rows_equal_the_restatement(tag):
    n, T = walk_of(tag).n, CASES[tag].steps
    L = float(n)
    ref = reference(tag)
    # the transport is exercised, a walker is carried over the box edge, and
    # the minimum image is never in doubt
    walks.assert_transport_exercised(ref, walk_of(tag), tag)
    assert ref['wrapped'] > 0, 'no walker-step wrapped: choose another seed'
    assert ref['max_d'] < L / 4
    ser, _, _, _, rows = run_block_b(tag)
    assert np.array_equal(ser.num_walkers, ref['num_walkers'])
    assert np.array_equal(ser.energy, ref['energy'])
    want = ref['rows']
    assert rows.shape == (T, 2)
    tol = cm.tolerance(ref['steps'], n, L)     # (asserts its precondition)
    err = np.abs(rows - want)
    print(tag, 'walkers', ref['num_walkers'], 'wrapped', ref['wrapped'],
          'max|d|', ref['max_d'], 'max|Y|', ref['max_y'])
    print('rows', rows, 'max err / tol', (err[1:] / tol[1:]).max(axis=0))
    assert not rows[0].any()                  # the origin: exactly zero
    assert (rows[1:] != 0).all()
    assert (err <= tol).all(), np.argwhere(err > tol)[:8]


def test_deterministic_and_burn_in():
    tag = 'wave'
    T = CASES[tag].steps
    s1, _, _, _, r1 = run_block_b(tag)
    s2, _, _, _, r2 = run_block_b(tag)
    assert r1.tobytes() == r2.tobytes()
    assert r1[1:].all()
    # a burn-in block propagates the same walkers and leaves the rows zero
    s0, _, _, _, r0 = run_block_b(tag, eval_estimators=False)
    assert r0.shape == (T, 2) and not r0.any()
    walks.assert_same_series(s0, s1)


def test_the_walk_and_the_other_estimators_do_not_notice():
    tag = 'mid'
    alone = run_block_b(tag)
    off = run_block_b(tag, on=False)
    before = run_block_b(tag, others='before')
    after = run_block_b(tag, others='after')
    without = run_block_b(tag, on=False, others='before')
    for both in (before, after):
        assert both[4].tobytes() == alone[4].tobytes()
        for k in (1, 2, 3):
            assert both[k].any()
            assert both[k].tobytes() == without[k].tobytes()
    assert alone[4][1:].all()
    # the walk itself does not know about the estimator
    ref = reference(tag)
    for run in (alone, off, before, after, without):
        assert run[0].energy.tobytes() == ref['energy'].tobytes()
        assert np.array_equal(run[0].num_walkers, ref['num_walkers'])
        walks.assert_same_series(run[0], off[0])


def test_resetting_a_live_ensemble_equals_a_fresh_one():
    """Ensemble R has every estimator set, then the centre-of-mass diffusion
    switched off and on again and the others set to other sizes; ensemble F is
    set once, to R's last configuration.  Same seed, same state, one estimator
    block each: every buffer of R was dropped and sized anew, so its rows are
    F's byte for byte."""
    from phd_qmclib_amd.engine import DmcEnsemble
    tag = 'mid'
    walk, T = walk_of(tag), CASES[tag].steps
    eng = walks.engine(walk)
    runs = []
    for again in (True, False):                      # R, then F
        d = DmcEnsemble(eng, TIME_STEP, walk.maxw, walk.nw0, 0.5,
                        rng_seed=walk.seed)
        if again:
            d.set_estimators(num_modes=5, num_bins=0)
            d.set_cm_diffusion_estimator()
            d.set_pair_dist_estimator(7)
            d.set_cm_diffusion_estimator(False)
        d.set_estimators(**EST)
        d.set_cm_diffusion_estimator()
        d.set_pair_dist_estimator(**G2)
        d.set_state(walks.start_positions(walk))
        ser, ssf, dens = d.run_block_est(T)
        runs.append((ser, ssf, dens, d.read_pair_dist(T),
                     d.read_cm_diffusion(T)))
        d.close()
    eng.close()
    r, f = runs
    walks.assert_same_series(r[0], f[0])
    for k in (1, 2, 3, 4):
        assert r[k].tobytes() == f[k].tobytes() and r[k].any()
    assert r[4].shape == (T, 2)


def test_switching_off_and_errors():
    from phd_qmclib_amd._lib import QmcError
    tag = 'odd'
    T = CASES[tag].steps
    eng = walks.engine(walk_of(tag))
    d = walks.ensemble(eng, walk_of(tag))
    with pytest.raises(QmcError):
        d.read_cm_diffusion(1)               # the estimator is off
    d.set_cm_diffusion_estimator()
    assert d.cm_diffusion
    with pytest.raises(QmcError):
        d.read_cm_diffusion(1)               # no estimator block yet
    d.run_block_est(T)
    assert d.read_cm_diffusion(T)[1:].all()
    assert np.array_equal(d.read_cm_diffusion(2), d.read_cm_diffusion(T)[:2])
    with pytest.raises(QmcError):
        d.read_cm_diffusion(T + 1)
    with pytest.raises(QmcError):
        d.read_cm_diffusion(0)
    d.set_cm_diffusion_estimator(False)
    assert not d.cm_diffusion
    ser, ssf, dens = d.run_block_est(2)      # falls through to run_block
    assert ssf is None and dens is None and len(ser.energy) == 2
    with pytest.raises(QmcError):
        d.read_cm_diffusion(1)
    d.close()
    eng.close()


def test_distributed_dmc_refuses_the_estimator():
    walks.assert_refused_by_distributed(
        walk_of('mid'), lambda d: d.set_cm_diffusion_estimator(),
        lambda d: d.set_cm_diffusion_estimator(False),
        'centre-of-mass diffusion')


# ---- top level ------------------------------------------------------------
def test_sampling_blocks_fill_iter_cm_diffusion():
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    confs = np.zeros((48, 2, 16))
    confs[:, 0, :] = walks.start_positions(walk_of('mid'))
    kw = dict(max_num_walkers=64, target_num_walkers=48, rng_seed=13)
    plain = mrbp_qmc.dmc.Sampling(spec, TIME_STEP, **kw)
    with_cm = mrbp_qmc.dmc.Sampling(
        spec, TIME_STEP, superfluid_est_spec=mrbp_qmc.dmc.SuperfluidEstSpec(),
        **kw)
    ini = plain.build_state(confs)
    b0 = list(islice(plain.blocks(ini, 6, 0), 2))
    b1 = list(islice(with_cm.blocks(ini, 6, 1), 2))
    for p, q in zip(b0, b1):
        assert p.iter_cm_diffusion is None and p.iter_pair_dist is None
        assert q.iter_density is None and q.iter_ssf is None
        assert q.iter_pair_dist is None
        assert q.iter_cm_diffusion.shape == (6, 2)
        assert p.iter_props.energy.tobytes() == q.iter_props.energy.tobytes()
    assert not b1[0].iter_cm_diffusion.any()         # the burn-in block
    kept = b1[1].iter_cm_diffusion
    assert not kept[0].any() and kept[1:].all()      # the origin, then not


def test_proc_exec_yields_cm_diffusion_blocks():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    dx = mrbp_qmc.dmc_exec
    spec = box(16)
    np.random.seed(5)
    kw = dict(max_num_walkers=512, target_num_walkers=480, rng_seed=7,
              num_blocks=4, num_time_steps_block=16, burn_in_blocks=1)
    on = dx.Proc(spec, TIME_STEP, superfluid_spec=dx.SuperfluidEstSpec(), **kw)
    din = dx.ProcInput.from_model_sys_conf_spec(
        dx.ModelSysConfSpec('RANDOM'), on)
    res = on.exec(din)
    blocks = res.data.blocks.cm_diffusion
    assert isinstance(blocks, dd.CMDiffusionBlocks)
    assert blocks.totals.shape == (4, 16) and res.data.series is None
    assert np.isfinite(blocks.totals).all()
    assert not blocks.totals[:, 0].any() and (blocks.totals[:, 1:] > 0).all()
    tau, ratio, err = blocks.superfluid_fraction(spec, TIME_STEP)
    assert tau.shape == ratio.shape == err.shape == (15,)
    assert np.isfinite(ratio).all() and np.isfinite(err).all()
    assert (ratio > 0).all()
    kres = dx.Proc(spec, TIME_STEP, keep_iter_data=True,
                   superfluid_spec=dx.SuperfluidEstSpec(), **kw).exec(din)
    kept = kres.data.series.cm_diffusion_blocks
    assert kept.shape == (4, 16, 2)
    nw = kres.data.series.iter_props_blocks.num_walkers
    assert np.array_equal(kres.data.blocks.cm_diffusion.totals,
                          kept[:, :, 1] / nw)
    assert np.array_equal(kres.data.blocks.cm_diffusion.totals, blocks.totals)
    # the walk is the same with and without the estimator
    off = dx.Proc(spec, TIME_STEP, **kw).exec(din)
    assert off.data.blocks.cm_diffusion is None
    assert np.array_equal(off.data.blocks.energy.totals,
                          res.data.blocks.energy.totals)
    assert np.array_equal(off.data.blocks.energy.weight_totals,
                          res.data.blocks.energy.weight_totals)


# ---- the exact rule -------------------------------------------------------
def test_free_centre_of_mass_diffuses_at_the_bare_rate():
    """lattice_depth = 0: the trial function is translation invariant, the
    drifts of a configuration add up to zero and the branching weights do not
    depend on the centre of mass, whose noise is independent of the relative
    motion.  E[Y_t^2] = 2 N t dt exactly, at any time step and from any start:
    ratio[t] = 1 (rho_s / rho = 1, no lattice to pin the gas).

    N = L = 8, interaction strength 4, dt = 1e-3, target 2048 / cap 2560
    walkers, one burn-in block and 16 kept blocks of 32 steps.  The blocks are
    independent (the origin resets, the noise is fresh), so the error of the
    mean over blocks is the scatter of the 16 values over sqrt(16).  Asserted:
    |mean - 1| <= 4 stderr at t = 16 and t = 31, and stderr <= 0.02
    (independent walkers would give sqrt(2 / 2048) / 4 = 0.008; the cap allows
    2.5 times that for shared ancestry).  The same workload through the CPU
    oracle's DMC and the restatement gives 0.994 +- 0.008 and 0.986 +- 0.009.
    """
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.engine import ModelEngine, superfluid_ratio
    n, nts, nblocks, dt = 8, 32, 16, 1e-3
    spec = box(n, depth=0, gint=4)
    pos = n * np.random.RandomState(21).random_sample((2048, n))
    eng = ModelEngine(spec.cfc_spec, device=0)
    drift = eng.evaluate(pos).drift
    eng.close()
    assert np.abs(drift.sum(axis=1)).max() * 2 * dt < 1e-9
    smp = mrbp_qmc.dmc.Sampling(
        spec, dt, max_num_walkers=2560, target_num_walkers=2048, rng_seed=21,
        superfluid_est_spec=mrbp_qmc.dmc.SuperfluidEstSpec())
    confs = np.zeros((2048, 2, n))
    confs[:, 0, :] = pos
    blocks = list(islice(smp.blocks(smp.build_state(confs), nts, 1),
                         1 + nblocks))
    assert not blocks[0].iter_cm_diffusion.any()
    ratios = np.array([
        superfluid_ratio(b.iter_cm_diffusion, b.iter_props.num_walkers, n,
                         dt)[1] for b in blocks[1:]])
    assert ratios.shape == (nblocks, nts - 1)
    for t in (16, 31):
        col = ratios[:, t - 1]                       # ratio[t], t >= 1
        mean = col.mean()
        stderr = col.std(ddof=1) / np.sqrt(nblocks)
        print('t', t, 'ratio', mean, '+-', stderr)
        assert stderr <= 0.02
        assert abs(mean - 1.0) <= 4 * stderr
