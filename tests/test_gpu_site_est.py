"""The DMC site occupation estimator on the GPU, mixed and pure, against the
NumPy forward walking (tests/_site_restatement.py) on the states of a twin
ensemble, and against the exact multinomial law of free particles.

Ensemble A and ensemble B start from the same positions with the same seed, so
they follow the same trajectory (test_gpu_pairdist_est.py).  A runs one time
step at a time and hands out its State after each; B runs one estimator block.
Every device quantity is an integer held in a double and the one division is
of an integer by an integer: the rows must be EQUAL to the restatement's,
whatever the order of the sums.  The only freedom is a particle at a site
boundary; every case asserts that none of its particles sits within 1e-9 of
one.
"""
import functools
from itertools import islice
from math import comb
from typing import NamedTuple

import numpy as np
import pytest

from . import _dmc_walks as walks
from . import _site_restatement as sr
from ._dmc_walks import TIME_STEP, WALKS
from ._models import box

pytestmark = pytest.mark.gpu

RATIO = 1
HALF_ZB = sr.half_barrier(RATIO)


class Case(NamedTuple):
    walk: str                   # of _dmc_walks.WALKS
    P: int                      # occupation bins
    D: int                      # distances
    steps: int
    pfw: int


# `Spec` accepts every shape as the cases were set.
CASES = {
    'odd':         Case('site_odd', 3, 5, 8, 3),
    'occ_only':    Case('site_occ_only', 1, 0, 6, 3),
    'many':        Case('site_many', 17, 16, 6, 3),
    'dilute':      Case('site_dilute', 4, 17, 6, 3),
    'dense':       Case('site_dense', 4, 9, 6, 3),
    'wave':        Case('site_wave', 8, 33, 10, 4),
    'two_pass':    Case('site_two_pass', 56, 200, 6, 3),
    'cap':         Case('site_cap', 5, 9, 8, 3),
    'second_trip': Case('site_second_trip', 5, 19, 4, 2),
}


def walk_of(tag):
    return WALKS[CASES[tag].walk]


@functools.lru_cache(maxsize=None)
def reference(tag):
    """Ensemble A's states of the block and the restatement's rows on them,
    computed once per case -> dict."""
    case = CASES[tag]
    rec = walks.record(case.walk, case.steps)
    mixed, pure, amb = sr.forward_walk(
        rec['steps'], float(walk_of(tag).sites), HALF_ZB, case.P, case.D,
        case.pfw)
    for arr in (mixed, pure):
        arr.setflags(write=False)
    return dict(rec, mixed=mixed, pure=pure, ambiguous=amb)


def _read_others(b, T):
    return (b.read_pair_dist(T), b.read_cm_diffusion(T), b.read_isf(T),
            b.read_obdm(T))


def run_block_b(tag, pure, eval_estimators=True, others=False, order=0,
                with_site=True):
    """Ensemble B: one estimator block -> (series, site rows, rows of the
    other estimators); `others` sets all the other estimators as well, before
    (order 0) or after (order 1) the site estimator."""
    case = CASES[tag]
    P, D, T, pfw = case.P, case.D, case.steps, case.pfw
    eng = walks.engine(walk_of(tag))
    b = walks.ensemble(eng, walk_of(tag))
    if others and order == 0:
        walks.set_others(b, **walks.ALL_SLOTS)
    if with_site:
        b.set_site_estimator(P, D, pure=pure, pfw=pfw)
        assert b.site_shape == (P, D)
    if others and order == 1:
        walks.set_others(b, **walks.ALL_SLOTS)
    ser, ssf, dens = b.run_block_est(T, eval_estimators)
    rows = b.read_site(T) if with_site else None
    rest = (ssf, dens) + _read_others(b, T) if others else ()
    b.close()
    eng.close()
    return ser, rows, rest


@pytest.mark.parametrize('pure', [False, True], ids=['mixed', 'pure'])
@pytest.mark.parametrize('tag', list(CASES))
def test_rows_equal_the_forward_walking(tag, pure):
    case = CASES[tag]
    n, S = walk_of(tag).n, walk_of(tag).sites
    P, D, T, pfw = case.P, case.D, case.steps, case.pfw
    ref = reference(tag)
    assert ref['ambiguous'] == [], \
        'a particle sits on a site boundary: choose another seed ' + \
        repr(ref['ambiguous'][:4])
    walks.assert_transport_exercised(ref, walk_of(tag), tag)
    if tag == 'two_pass':
        assert P + D == 256 and n > 64 and S > 64 and D > 64
    if pure:
        assert 1 < pfw < T          # both divisors, min(t + 1, pfw)
    ser, rows, _ = run_block_b(tag, pure)
    print(tag, 'pure' if pure else 'mixed', 'walkers', ref['num_walkers'])
    assert np.array_equal(ser.num_walkers, ref['num_walkers'])
    assert np.array_equal(ser.energy, ref['energy'])
    want = ref['pure'] if pure else ref['mixed']
    assert rows.shape == (T, P + D)
    assert np.array_equal(rows, want), np.argwhere(rows != want)[:8]
    # the identities of a row, on the integer numerators
    counts, div = walks.numerators(rows, T, pfw, pure)
    # (the row of a pure walker holds the min(t + 1, pfw) steps of its
    # lineage, so the identities hold for both with the walkers times steps)
    steps_in = ref['num_walkers'] * div[:, 0]
    occ, corr = counts[:, :P], counts[:, P:]
    assert np.array_equal(occ.sum(axis=1), S * steps_in)
    max_occ = max(sr.site_counts(c[:nw], float(S), HALF_ZB).max()
                  for c, _, nw in ref['steps'])
    if tag == 'odd':
        assert max_occ >= P         # the last bin saturates
    if tag in ('many', 'two_pass'):
        assert max_occ < P - 1      # no bin saturates
    if P > max_occ and D > 0:
        assert np.array_equal(corr[:, 0], occ @ (np.arange(P) ** 2.0))
    if D == S:
        for d in range(1, S):
            assert np.array_equal(corr[:, d], corr[:, S - d])
        assert np.array_equal(corr.sum(axis=1), n * n * steps_in)


@pytest.mark.parametrize('pure', [False, True], ids=['mixed', 'pure'])
def test_deterministic_and_burn_in(pure):
    tag = 'wave'
    P, D, T = CASES[tag].P, CASES[tag].D, CASES[tag].steps
    s1, r1, _ = run_block_b(tag, pure)
    s2, r2, _ = run_block_b(tag, pure)
    assert r1.tobytes() == r2.tobytes()
    assert r1.any()
    # a burn-in block propagates the same walkers and leaves the rows zero
    s0, r0, _ = run_block_b(tag, pure, eval_estimators=False)
    assert r0.shape == (T, P + D) and not r0.any()
    assert np.array_equal(s0.energy, s1.energy)
    assert np.array_equal(s0.num_walkers, s1.num_walkers)


@pytest.mark.parametrize('pure', [False, True], ids=['mixed', 'pure'])
def test_independent_of_the_other_estimators(pure):
    tag = 'many'
    alone = run_block_b(tag, pure)
    first = run_block_b(tag, pure, others=True, order=0)
    second = run_block_b(tag, pure, others=True, order=1)
    without = run_block_b(tag, pure, others=True, with_site=False)
    assert len(without[2]) == 6
    for both in (first, second):
        assert np.array_equal(both[1], alone[1])
        for got, want in zip(both[2], without[2]):
            assert got.any()
            assert got.tobytes() == want.tobytes()
    # the walk itself does not know about the estimator
    ref = reference(tag)
    for run in (alone, first, second, without):
        walks.assert_same_series(run[0], alone[0])
        assert np.array_equal(run[0].energy, ref['energy'])
        assert np.array_equal(run[0].num_walkers, ref['num_walkers'])


@pytest.mark.parametrize('second_pure', [False, True],
                         ids=['wide_then_narrow', 'narrow_then_wide'])
def test_resetting_a_live_ensemble_equals_a_fresh_one(second_pure):
    """The estimator set again, to another shape, on an ensemble that already
    has it: ensemble R is set twice, ensemble F only to the second shape; same
    seed, same state, one estimator block each."""
    from phd_qmclib_amd.engine import DmcEnsemble
    tag = 'many'
    case, walk = CASES[tag], walk_of(tag)
    S, P, D, T, pfw = walk.sites, case.P, case.D, case.steps, case.pfw
    wide = dict(num_occ=P, num_dist=D, pure=True, pfw=pfw)
    narrow = dict(num_occ=3, num_dist=4, pure=False)
    configs = [narrow, wide] if second_pure else [wide, narrow]
    eng = walks.engine(walk)
    runs = []
    for todo in (configs, configs[1:]):              # R, then F
        d = DmcEnsemble(eng, TIME_STEP, walk.maxw, walk.nw0, 0.5,
                        rng_seed=walk.seed)
        for cfg in todo:
            d.set_site_estimator(**cfg)
        d.set_state(walks.start_positions(walk))
        ser, _, _ = d.run_block_est(T)
        runs.append((ser, d.read_site(T)))
        d.close()
    eng.close()
    (ser_r, rows_r), (ser_f, rows_f) = runs
    walks.assert_same_series(ser_r, ser_f)
    assert rows_r.tobytes() == rows_f.tobytes()
    assert rows_r.shape == (T, P + D if second_pure else 7)
    assert rows_r.any(axis=1).all()
    # F is not the only witness: the restatement on the twin's states
    ref = reference(tag)
    if second_pure:
        want = ref['pure']
    else:
        want, _, amb = sr.forward_walk(ref['steps'], float(S), HALF_ZB, 3, 4,
                                       pfw)
        assert amb == []
    assert np.array_equal(rows_r, want), np.argwhere(rows_r != want)[:8]


def test_switching_off_and_errors():
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    from phd_qmclib_amd._lib import QmcError
    tag = 'odd'
    case, S = CASES[tag], walk_of(tag).sites
    P, D, T, pfw = case.P, case.D, case.steps, case.pfw
    eng = walks.engine(walk_of(tag))
    d = walks.ensemble(eng, walk_of(tag))
    who = 'qmc_dmc_set_site_estimator'
    for bad in (dict(num_occ=-1), dict(num_occ=2, num_dist=-1),
                dict(num_occ=2, num_dist=S + 1), dict(num_occ=257),
                dict(num_occ=254, num_dist=3),
                dict(num_occ=3, num_dist=2, pure=True, pfw=0)):
        with pytest.raises(QmcError, match=who):
            d.set_site_estimator(**bad)
        assert d.site_shape is None
    with pytest.raises(QmcError, match='read_site'):
        d.read_site(1)                       # the estimator is off
    d.set_site_estimator(P, D, pure=True, pfw=pfw)
    with pytest.raises(QmcError, match='qmc_dmc_read_site'):
        d.read_site(1)                       # no estimator block yet
    d.run_block_est(T)
    assert d.read_site(T).any()
    with pytest.raises(QmcError, match='qmc_dmc_read_site'):
        d.read_site(T + 1)
    d.set_site_estimator(0)
    assert d.site_shape is None
    ser, ssf, dens = d.run_block_est(2)      # falls through to run_block
    assert ssf is None and dens is None and len(ser.energy) == 2
    with pytest.raises(QmcError, match='read_site'):
        d.read_site(1)
    d.close()
    eng.close()
    # the sites are the periods of the lattice: a supercell that does not
    # hold a whole number of them has none
    spec = box(5, supercell_size=5.5)
    eng = ModelEngine(spec.cfc_spec, device=0)
    d = DmcEnsemble(eng, TIME_STEP, 64, 40, 0.5, rng_seed=1)
    with pytest.raises(QmcError, match=who + '.*supercell_size'):
        d.set_site_estimator(3, 2)
    d.set_site_estimator(0)                  # off needs no sites
    d.close()
    eng.close()


def test_distributed_dmc_refuses_the_estimator():
    walks.assert_refused_by_distributed(
        walk_of('many'), lambda d: d.set_site_estimator(4, 3),
        lambda d: d.set_site_estimator(0), 'site occupation', rng_seed=2)


# ---- top level ------------------------------------------------------------
def test_sampling_blocks_fill_iter_site():
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    confs = np.zeros((48, 2, 16))
    confs[:, 0, :] = walks.start_positions(walk_of('many'))
    kw = dict(max_num_walkers=64, target_num_walkers=48, rng_seed=13)
    plain = mrbp_qmc.dmc.Sampling(spec, TIME_STEP, **kw)
    with_site = mrbp_qmc.dmc.Sampling(
        spec, TIME_STEP, site_est_spec=mrbp_qmc.dmc.SiteEstSpec(
            5, 9, as_pure_est=True, pfw_num_time_steps=3), **kw)
    ini = plain.build_state(confs)
    b0 = list(islice(plain.blocks(ini, 6, 0), 2))
    b1 = list(islice(with_site.blocks(ini, 6, 1), 2))
    for p, q in zip(b0, b1):
        assert p.iter_site is None and p.iter_density is None
        assert q.iter_density is None and q.iter_pair_dist is None
        assert q.iter_site.shape == (6, 14)
        assert np.array_equal(p.iter_props.energy, q.iter_props.energy)
    assert not b1[0].iter_site.any()                 # the burn-in block
    nw = b1[1].iter_props.num_walkers.astype(np.int64)
    counts, div = walks.numerators(b1[1].iter_site, 6, 3, True)
    assert np.array_equal(counts[:, :5].sum(axis=1), nw * div[:, 0] * 16)


def test_proc_exec_yields_site_blocks(tmp_path):
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.engine import site_statistics
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    dx = mrbp_qmc.dmc_exec
    spec = box(16)
    P, D = 6, 9
    np.random.seed(5)
    kw = dict(max_num_walkers=512, target_num_walkers=480, rng_seed=7,
              num_blocks=4, num_time_steps_block=16, burn_in_blocks=1)
    pure = dx.Proc(spec, TIME_STEP, site_spec=dx.SiteEstSpec(P, D), **kw)
    assert pure.sampling.site_est_spec == mrbp_qmc.dmc.SiteEstSpec(
        P, D, True, 16)                     # forward walking spans the block
    din = dx.ProcInput.from_model_sys_conf_spec(
        dx.ModelSysConfSpec('RANDOM'), pure)
    res = pure.exec(din)
    sb = res.data.blocks.site
    assert isinstance(sb, dd.SiteBlocks) and sb.num_occupations == P
    assert sb.totals.shape == (4, P + D) and sb.weight_totals.shape == (4, 1)
    assert res.data.blocks.density is None and res.data.series is None
    # the last row of a block: every walker's sites of the 16 steps, over 16
    nw_last = np.rint(sb.weight_totals[:, 0])
    assert np.allclose(sb.weight_totals[:, 0], nw_last, rtol=1e-14, atol=0)
    assert np.array_equal(sb.totals[:, :P].sum(axis=1), nw_last * 16)
    pn, pn_err = sb.occupation_distribution()
    assert pn.shape == pn_err.shape == (P,)
    assert abs(pn.sum() - 1.0) < 1e-14 and (pn >= 0).all()
    assert np.isfinite(pn_err).all()
    corr, corr_err = sb.site_correlation(spec)
    assert corr.shape == corr_err.shape == (D,)
    # the container's numbers are those of the helper on the mean row
    stats = site_statistics(sb.mean, 1.0, 16, 16, P)
    assert np.array_equal(corr, stats.correlation)
    ells, var, var_err = sb.number_variance(D, spec)
    assert np.array_equal(ells, np.arange(1, D + 1))
    assert var[0] == corr[0] and np.isfinite(var_err).all()
    assert np.allclose(var, [stats.number_variance(ell) for ell in ells],
                       rtol=1e-13, atol=1e-13)
    # the result file
    h = dx.HDF5FileHandler(str(tmp_path / 'site.h5'), 'run-A')
    h.dump(res)
    back = h.load()
    assert back.proc == res.proc and back.proc.site_spec == dx.SiteEstSpec(P, D)
    got = back.data.blocks.site
    assert isinstance(got, dd.SiteBlocks) and got.num_occupations == P
    assert np.array_equal(got.totals, sb.totals)
    assert np.array_equal(got.weight_totals, sb.weight_totals)
    assert back.data.blocks.pair_dist is None
    # the walk is the same with and without the estimator
    off = dx.Proc(spec, TIME_STEP, **kw).exec(din)
    assert off.data.blocks.site is None
    assert np.array_equal(off.data.blocks.energy.totals,
                          res.data.blocks.energy.totals)


# ---- the exact law ----------------------------------------------------------
def test_free_particles_follow_the_multinomial_law():
    """No lattice, no interaction: psi_T = 1, no drift, no branching, and the
    Gaussian step of the free diffusion is exact at any time step.  A uniform
    start stays independent and uniform, so the occupations of the S sites are
    multinomial: P(n) = Binom(N, 1/S), <n_c^2> = N (N - 1) / S^2 + N / S and
    <n_c n_{c+d}> = N (N - 1) / S^2 for d != 0.

    N = S = 8, P = 6 (the last bin collects n >= 5), D = 5, dt = 5e-2, 2048
    walkers, one burn-in block and 16 kept blocks of 64 steps, pure, read at
    the last step of a block.  Every one of the 11 columns must lie within 5
    standard errors of the exact value, the standard error being the scatter
    of the 16 block values over sqrt(16).  With these block lengths the exact
    process, simulated with NumPy, stays within 3.6 standard errors on 40
    seeds; with 32-step blocks at dt = 1e-2 the blocks are correlated and 30 %
    of the seeds exceed 4, so the blocks must not be shortened."""
    from phd_qmclib_amd.engine import (DmcEnsemble, ModelEngine,
                                       site_statistics)
    N = S = 8
    P, D, W, T, NB = 6, 5, 2048, 64, 16
    spec = box(N, depth=0, gint=0)
    eng = ModelEngine(spec.cfc_spec, device=0)
    d = DmcEnsemble(eng, 5e-2, 2560, W, 0.5, rng_seed=31)
    d.set_state(S * np.random.RandomState(32).random_sample((W, N)))
    d.set_site_estimator(P, D, pure=True, pfw=T)
    ser, _, _ = d.run_block_est(T, False)             # the burn-in block
    assert not d.read_site(T).any()
    walkers = [ser.num_walkers]
    blocks = np.zeros((NB, P + D))
    for b in range(NB):
        ser, _, _ = d.run_block_est(T)
        walkers.append(ser.num_walkers)
        last = d.read_site(T)[T - 1]
        assert last[:P].sum() == S * W                # sum_n P(n) = 1, exactly
        blocks[b] = last
    d.close()
    eng.close()
    assert (np.concatenate(walkers) == W).all()
    stats = site_statistics(blocks, float(W), N, S, P)
    assert np.array_equal(stats.occupation_dist.sum(axis=1), np.ones(NB))
    p = 1.0 / S
    binom = np.array([comb(N, n) * p ** n * (1 - p) ** (N - n)
                      for n in range(N + 1)])
    exact = np.concatenate([binom[:P - 1], [binom[P - 1:].sum()],
                            [N * (N - 1) / S ** 2 + N / S],
                            np.full(D - 1, N * (N - 1) / S ** 2)])
    # per site and walker: P(n) | <n_c n_{c+d}>
    values = blocks / (S * W)
    mean = values.mean(axis=0)
    stderr = values.std(axis=0, ddof=1) / np.sqrt(NB)
    dev = np.abs(mean - exact) / stderr
    print('mean', mean, 'exact', exact, 'stderr', stderr, 'dev', dev)
    assert (stderr > 0).all()
    assert (dev <= 5.0).all(), dev
