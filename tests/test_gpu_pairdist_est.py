"""The DMC pair distribution estimator on the GPU, mixed and pure, against the
NumPy forward walking (tests/_pairdist_fw_restatement.py) on the states of a
twin ensemble.

Ensemble A and ensemble B start from the same positions with the same seed, so
they follow the same trajectory (test_gpu_sampling.py::
test_dmc_split_step_equals_block).  A runs one time step at a time and hands
out its State after each; B runs one estimator block.  Every device quantity is
an integer held in a double and the one division is of an integer by an
integer: the rows must be EQUAL to the restatement's, whatever the order of the
sums.  The only freedom is the rounding of r / delta at a bin edge; the seeds
below were picked so that no pair of any case sits within 1e-9 of one.
"""
import functools
from itertools import islice
from typing import NamedTuple

import numpy as np
import pytest

from . import _dmc_walks as walks
from . import _pairdist_fw_restatement as fw
from ._dmc_walks import EST, TIME_STEP, WALKS
from ._models import box

pytestmark = pytest.mark.gpu


class Case(NamedTuple):
    walk: str                   # of _dmc_walks.WALKS
    bins: int
    steps: int
    pfw: int


# The smallest shapes that still reach every path of the kernel: an odd N with
# fewer bins than lanes; a single bin; more than 64 bins (the lane = bin
# chunks); N = 64, one particle per lane, with pfw inside the block (both
# divisors); N = 100, two passes over the own particles, at the largest bin
# count; a population that starts at the cap; more live walkers than the
# launch has wavefronts (N = 37, bins in two lane chunks, pfw inside the block),
# so that every wavefront goes round its slot loop again and rewrites its
# positions and its histogram.
CASES = {
    'odd':         Case('odd', 7, 8, 3),
    'one_bin':     Case('one_bin', 1, 6, 3),
    'many':        Case('many', 200, 6, 3),
    'wave':        Case('wave', 64, 10, 4),
    'two_pass':    Case('two_pass', 256, 6, 3),
    'cap':         Case('cap', 16, 8, 3),
    'second_trip': Case('second_trip', 70, 4, 2),
}


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Ensemble A's states of the block and the restatement's rows on them,
    computed once per case -> dict."""
    case = CASES[tag]
    rec = walks.record(case.walk, case.steps)
    mixed, pure, amb = fw.forward_walk(
        rec['steps'], float(WALKS[case.walk].n), case.bins, case.pfw)
    for arr in (mixed, pure):
        arr.setflags(write=False)
    return dict(rec, mixed=mixed, pure=pure, ambiguous=amb)


def run_block_b(tag, pure, eval_estimators=True, others=False, order=0,
                with_g2=True):
    """Ensemble B: one estimator block -> (series, ssf, dens, g2 rows);
    `others` sets S(k) and the density as well, before (order 0) or after
    (order 1) the pair distribution."""
    case = CASES[tag]
    T, pfw = case.steps, case.pfw
    B = case.bins if with_g2 else 0
    eng = walks.engine(WALKS[case.walk])
    b = walks.ensemble(eng, WALKS[case.walk])
    est = dict(EST, ssf_pfw=pfw)
    if others and order == 0:
        b.set_estimators(**est)
    if B:
        b.set_pair_dist_estimator(B, pure=pure, pfw=pfw)
    if others and order == 1:
        b.set_estimators(**est)
    ser, ssf, dens = b.run_block_est(T, eval_estimators)
    rows = b.read_pair_dist(T) if B else None
    b.close()
    eng.close()
    return ser, ssf, dens, rows


@pytest.mark.parametrize('pure', [False, True], ids=['mixed', 'pure'])
@pytest.mark.parametrize('tag', list(CASES))
def test_rows_equal_the_forward_walking(tag, pure):
    case = CASES[tag]
    n, B, T, pfw = WALKS[case.walk].n, case.bins, case.steps, case.pfw
    ref = reference(tag)
    assert ref['ambiguous'] == [], \
        'a pair sits on a bin edge: choose another seed ' + \
        repr(ref['ambiguous'][:4])
    walks.assert_transport_exercised(ref, WALKS[case.walk], tag)
    if pure:
        assert 1 < pfw < T          # both divisors, min(t + 1, pfw)
    ser, _, _, rows = run_block_b(tag, pure)
    print(tag, 'pure' if pure else 'mixed', 'walkers', ref['num_walkers'])
    assert np.array_equal(ser.num_walkers, ref['num_walkers'])
    assert np.array_equal(ser.energy, ref['energy'])
    want = ref['pure'] if pure else ref['mixed']
    assert rows.shape == (T, B)
    assert np.array_equal(rows, want), np.argwhere(rows != want)[:8]
    # every walker holds N (N - 1) / 2 pairs, at every step, mixed and pure:
    # checked on the integer numerators
    counts, div = walks.numerators(rows, T, pfw, pure)
    assert np.array_equal(counts.sum(axis=1),
                          ref['num_walkers'] * div[:, 0] * (n * (n - 1) // 2))


@pytest.mark.parametrize('pure', [False, True], ids=['mixed', 'pure'])
def test_deterministic_and_burn_in(pure):
    tag = 'wave'
    B, T = CASES[tag].bins, CASES[tag].steps
    s1, _, _, r1 = run_block_b(tag, pure)
    s2, _, _, r2 = run_block_b(tag, pure)
    assert r1.tobytes() == r2.tobytes()
    assert r1.any()
    # a burn-in block propagates the same walkers and leaves the rows zero
    s0, _, _, r0 = run_block_b(tag, pure, eval_estimators=False)
    assert r0.shape == (T, B) and not r0.any()
    assert np.array_equal(s0.energy, s1.energy)
    assert np.array_equal(s0.num_walkers, s1.num_walkers)


@pytest.mark.parametrize('pure', [False, True], ids=['mixed', 'pure'])
def test_independent_of_the_other_estimators(pure):
    tag = 'many'
    alone = run_block_b(tag, pure)
    first = run_block_b(tag, pure, others=True, order=0)
    second = run_block_b(tag, pure, others=True, order=1)
    without = run_block_b(tag, pure, others=True, with_g2=False)
    for both in (first, second):
        assert np.array_equal(both[3], alone[3])
        assert both[1].any() and both[2].any()
        assert both[1].tobytes() == without[1].tobytes()
        assert both[2].tobytes() == without[2].tobytes()
    # the walk itself does not know about the estimator
    ref = reference(tag)
    for run in (alone, first, second, without):
        assert np.array_equal(run[0].energy, ref['energy'])
        assert np.array_equal(run[0].num_walkers, ref['num_walkers'])


@pytest.mark.parametrize('second_pure', [False, True],
                         ids=['wide_then_narrow', 'narrow_then_wide'])
def test_resetting_a_live_ensemble_equals_a_fresh_one(second_pure):
    """Estimators set again, to other sizes, on an ensemble that already has
    some: ensemble R is set twice, ensemble F only to the second configuration;
    same seed, same state, one estimator block each.  Every buffer of R was
    dropped and sized anew, so its rows are F's byte for byte.  The density is
    off in the narrow configuration (`dens is None` in R and in F); where the
    second configuration is the wide one it has 12 bins, and the density rows
    are compared like the others: equal byte for byte, none of them zero."""
    from phd_qmclib_amd.engine import DmcEnsemble
    tag = 'many'
    case, walk = CASES[tag], WALKS[CASES[tag].walk]
    n, nw0, maxw, seed = walk.n, walk.nw0, walk.maxw, walk.seed
    B, T, pfw = case.bins, case.steps, case.pfw
    B2 = B // 4          # its bin edges are edges of the B bins as well
    assert (n, nw0, maxw) == (16, 48, 64) and 0 < B2 < B
    wide = (dict(num_modes=8, ssf_pure=True, ssf_pfw=pfw, num_bins=12),
            dict(num_bins=B, pure=True, pfw=pfw))
    narrow = (dict(num_modes=5, num_bins=0), dict(num_bins=B2, pure=False))
    configs = [narrow, wide] if second_pure else [wide, narrow]
    eng = walks.engine(walk)
    runs = []
    for todo in (configs, configs[1:]):              # R, then F
        d = DmcEnsemble(eng, TIME_STEP, maxw, nw0, 0.5, rng_seed=seed)
        for est, g2 in todo:
            d.set_estimators(**est)
            d.set_pair_dist_estimator(**g2)
        d.set_state(walks.start_positions(walk))
        ser, ssf, dens = d.run_block_est(T)
        runs.append((ser, ssf, dens, d.read_pair_dist(T)))
        d.close()
    eng.close()
    (ser_r, ssf_r, dens_r, g2_r), (ser_f, ssf_f, dens_f, g2_f) = runs
    walks.assert_same_series(ser_r, ser_f)
    assert ssf_r.tobytes() == ssf_f.tobytes()
    assert g2_r.tobytes() == g2_f.tobytes()
    assert ssf_r.shape == (T, 8 if second_pure else 5, 3)
    assert g2_r.shape == (T, B if second_pure else B2)
    assert ssf_r.reshape(T, -1).any(axis=1).all() and g2_r.any(axis=1).all()
    if second_pure:
        assert dens_r.tobytes() == dens_f.tobytes()
        assert dens_r.shape == (T, 12, 1) and dens_r.any(axis=(1, 2)).all()
    else:
        assert dens_r is None and dens_f is None
    # F is not the only witness: the restatement on the twin's states
    ref = reference(tag)
    assert np.array_equal(ser_r.energy, ref['energy'])
    if second_pure:
        want = ref['pure']
    else:
        want, _, amb = fw.forward_walk(ref['steps'], float(n), B2, pfw)
        assert amb == []
    assert np.array_equal(g2_r, want), np.argwhere(g2_r != want)[:8]


def test_switching_off_and_errors():
    from phd_qmclib_amd._lib import QmcError
    case = CASES['odd']
    B, T, pfw = case.bins, case.steps, case.pfw
    eng = walks.engine(WALKS[case.walk])
    d = walks.ensemble(eng, WALKS[case.walk])
    with pytest.raises(QmcError):
        d.set_pair_dist_estimator(257)
    with pytest.raises(QmcError):
        d.set_pair_dist_estimator(-1)
    with pytest.raises(QmcError):
        d.set_pair_dist_estimator(8, pure=True, pfw=0)
    d.set_pair_dist_estimator(B, pure=True, pfw=pfw)
    with pytest.raises(QmcError):
        d.read_pair_dist(1)                  # no estimator block yet
    d.run_block_est(T)
    assert d.read_pair_dist(T).any()
    with pytest.raises(QmcError):
        d.read_pair_dist(T + 1)
    d.set_pair_dist_estimator(0)
    ser, ssf, dens = d.run_block_est(2)      # falls through to run_block
    assert ssf is None and dens is None and len(ser.energy) == 2
    with pytest.raises(QmcError):
        d.read_pair_dist(1)
    d.close()
    eng.close()


def test_distributed_dmc_refuses_the_estimator():
    walks.assert_refused_by_distributed(
        WALKS['many'], lambda d: d.set_pair_dist_estimator(16),
        lambda d: d.set_pair_dist_estimator(0), 'pair distribution',
        rng_seed=2)


# ---- top level ------------------------------------------------------------
def test_sampling_blocks_fill_iter_pair_dist():
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    confs = np.zeros((48, 2, 16))
    confs[:, 0, :] = walks.start_positions(WALKS['many'])
    kw = dict(max_num_walkers=64, target_num_walkers=48, rng_seed=13)
    plain = mrbp_qmc.dmc.Sampling(spec, TIME_STEP, **kw)
    with_pd = mrbp_qmc.dmc.Sampling(
        spec, TIME_STEP, pair_dist_est_spec=mrbp_qmc.dmc.PairDistEstSpec(
            20, as_pure_est=True, pfw_num_time_steps=3), **kw)
    assert with_pd.pair_dist_bins.shape == (20,)
    ini = plain.build_state(confs)
    b0 = list(islice(plain.blocks(ini, 6, 0), 2))
    b1 = list(islice(with_pd.blocks(ini, 6, 1), 2))
    for p, q in zip(b0, b1):
        assert p.iter_pair_dist is None and p.iter_density is None
        assert q.iter_density is None and q.iter_ssf is None
        assert q.iter_pair_dist.shape == (6, 20)
        assert np.array_equal(p.iter_props.energy, q.iter_props.energy)
    assert not b1[0].iter_pair_dist.any()            # the burn-in block
    nw = b1[1].iter_props.num_walkers.astype(np.int64)
    counts, div = walks.numerators(b1[1].iter_pair_dist, 6, 3, True)
    assert np.array_equal(counts.sum(axis=1), nw * div[:, 0] * 120)


def test_proc_exec_pure_and_mixed_kept():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    spec = box(16)
    B = 32
    np.random.seed(5)
    kw = dict(max_num_walkers=512, target_num_walkers=480, rng_seed=7,
              num_blocks=4, num_time_steps_block=16, burn_in_blocks=1)
    pure = mrbp_qmc.dmc_exec.Proc(
        spec, TIME_STEP, pair_dist_spec=mrbp_qmc.dmc_exec.PairDistEstSpec(B),
        **kw)
    din = mrbp_qmc.dmc_exec.ProcInput.from_model_sys_conf_spec(
        mrbp_qmc.dmc_exec.ModelSysConfSpec('RANDOM'), pure)
    res = pure.exec(din)
    pd = res.data.blocks.pair_dist
    assert isinstance(pd, dd.PairDistBlocks)
    assert pd.totals.shape == (4, B) and pd.weight_totals.shape == (4, 1)
    assert res.data.blocks.density is None and res.data.series is None
    # the last row of a block: every walker's pairs of the 16 steps, over 16
    nw_last = np.rint(pd.weight_totals[:, 0])
    assert np.allclose(pd.weight_totals[:, 0], nw_last, rtol=1e-14, atol=0)
    assert np.array_equal(pd.totals.sum(axis=1), nw_last * 120)
    r, g2, err = pd.pair_distribution(spec)
    assert r.shape == g2.shape == err.shape == (B,)
    assert np.isfinite(g2).all() and (g2 >= 0).all()
    # the histogram of a whole population averages to one
    assert abs(g2.mean() - 1.0) < 1e-12
    mixed = mrbp_qmc.dmc_exec.Proc(
        spec, TIME_STEP, keep_iter_data=True,
        pair_dist_spec=mrbp_qmc.dmc_exec.PairDistEstSpec(B, False), **kw)
    kres = mixed.exec(din)
    kept = kres.data.series.pair_dist_blocks
    assert kept.shape == (4, 16, B)
    nw = kres.data.series.iter_props_blocks.num_walkers.astype(np.int64)
    assert np.array_equal(kept.sum(axis=2), nw * 120)
    kpd = kres.data.blocks.pair_dist
    assert np.array_equal(kpd.totals, kept.sum(axis=1))
    assert np.isfinite(kpd.pair_distribution(spec)[1]).all()
    # the walk is the same with and without the estimator
    off = mrbp_qmc.dmc_exec.Proc(spec, TIME_STEP, **kw).exec(din)
    assert off.data.blocks.pair_dist is None
    assert np.array_equal(off.data.blocks.energy.totals,
                          res.data.blocks.energy.totals)
