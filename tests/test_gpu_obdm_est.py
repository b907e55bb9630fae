"""The DMC one-body density matrix estimator on the GPU (`dmc_obdm_kernel`),
against the NumPy restatement of g1 (tests/_obdm_restatement.py) and against
the batch kernel (`ModelEngine.one_body_density`) on the states of a twin
ensemble.

Ensemble A and ensemble B start from the same positions with the same seed, so
they follow the same trajectory.  A runs one time step at a time and hands out
`(confs[:, 0, :], cloning_ref, num_walkers)` after each; B runs one estimator
block.  Row t of B is the sum over the walkers of step t of their g1.

Yardsticks, per step and shift:

* the definition: |row - sum_s ref_s| <= 2e-11 sum_s max(1, |ref_s|), the
  per-value tolerance of tests/test_gpu_obdm.py (RTOL) summed over the walkers;
* the batch kernel: |row - fsum_s x_s| <= nw 2^-52 sum_s |x_s|, the worst case
  of nw fp64 additions of values that are equal bit for bit, which the shared
  device code of the two kernels gives;
* with at most two walkers the row IS the float sum of the batch kernel's
  values (a sum of two does not depend on the order).
"""
import ctypes as C
import functools
import math
from itertools import islice
from math import pi
from typing import NamedTuple

import numpy as np
import pytest

from . import _dmc_walks as walks
from . import _obdm_restatement as restated
from ._dmc_walks import TIME_STEP, WALKS
from ._models import box, model_dict

pytestmark = pytest.mark.gpu

RTOL = 2e-11                    # of tests/test_gpu_obdm.py


class Case(NamedTuple):
    walk: str                   # of _dmc_walks.WALKS
    steps: int
    shifts: tuple               # as multiples of L


# The walks `odd` .. `second_trip` clone, change population and, for
# `second_trip`, stay above 4096 live walkers.
#   odd_k1:   N = 5, G = 8: eight shift groups per wave, a single one and a
#             single u-slot live
#   odd_k19:  more than one trip of 8 groups x 2 shifts, with a remainder
#   one_bin, many: N = 16, the maximum of 256 shifts: zero, negative, beyond L,
#             -0.37 L among them
#   wave:     N = 64, G = 64: one shift group; an odd count, the last u-slot idle
#   two_pass: N = 100, two passes over the own particles
#   cap:      the population starts at the cap
#   second_trip: more live walkers than wavefronts: every wavefront goes round
#             the slot loop again and rewrites its LDS region
#   n512:     the largest LDS request
#   free16 (no one-body factor), ideal16 (no pair factor), odd24 (non-integer
#             L: the one-body factor does not have the period L; a shift of
#             exactly L)
def _k256():
    grid = np.linspace(-0.5, 1.5, 252)
    return tuple(grid) + (0.0, -0.37, 1.25, -0.01)


CASES = {
    'odd_k1':      Case('odd', 8, (0.3,)),
    'odd_k19':     Case('odd', 8, tuple(np.linspace(0.0, 0.5, 19))),
    'one_bin':     Case('one_bin', 6, _k256()),
    'many':        Case('many', 6, _k256()),
    'wave':        Case('wave', 10, (0.0, 0.01, 0.03, -0.37, 0.5)),
    'two_pass':    Case('two_pass', 6, (0.0, 0.013)),
    'cap':         Case('cap', 8, (0.0, 0.1, -0.45)),
    'second_trip': Case('second_trip', 2, (0.0, 0.02)),
    'n512':        Case('n512', 2, (0.0, 0.002)),
    'free16':      Case('free16', 4, (0.0, 0.07, -0.37)),
    'ideal16':     Case('ideal16', 4, (0.0, 0.07, -0.37)),
    'odd24':       Case('odd24', 4, (0.0, 0.07, 1.0)),
}
PAIRDIST_WALKS = ('odd_k1', 'odd_k19', 'one_bin', 'many', 'wave', 'two_pass',
                  'cap', 'second_trip')


def walk_of(tag):
    return WALKS[CASES[tag].walk]


def spec_of(tag):
    return walks.spec(walk_of(tag))


def shifts_of(tag):
    L = float(spec_of(tag).supercell_size)
    return np.array(CASES[tag].shifts) * L


@functools.lru_cache(maxsize=None)
def walk(tag):
    """Ensemble A's states of the case's block, each step cut to its live
    walkers -> dict."""
    rec = walks.record(CASES[tag].walk, CASES[tag].steps)
    return dict(rec, steps=[(c[:nw], r[:nw], nw) for c, r, nw in rec['steps']])


@functools.lru_cache(maxsize=None)
def reference(tag):
    """The two yardsticks on ensemble A's configurations, once per case:
    defn[t], batch[t] = g1[nw_t, K] of the restatement (evaluated once per
    distinct configuration: clones repeat) and of the batch kernel."""
    w = walk(tag)
    cfc = spec_of(tag).cfc_spec
    p, sh = model_dict(cfc), shifts_of(tag)
    eng = walks.engine(walk_of(tag))
    defn, batch = [], []
    for pos, _, nw in w['steps']:
        uniq, inv = np.unique(pos, axis=0, return_inverse=True)
        g = restated.one_body_density(uniq, sh, p)[inv.reshape(-1)]
        b = eng.one_body_density(pos, sh)
        for arr in (g, b):
            arr.setflags(write=False)
        defn.append(g)
        batch.append(b)
    eng.close()
    return dict(w, defn=defn, batch=batch)


def run_block_b(tag, shifts=None, stride=1, steps=None, eval_estimators=True,
                others=0, with_g1=True, disturb=False, blocks=1):
    """Ensemble B: `blocks` estimator blocks -> list of (series, ssf, dens,
    g2 rows, isf rows, g1 rows).  `others`: S(k), the density, g2 and
    F(k, tau) are set as well, before (1) or after (2) g1.  `disturb`: the
    batch g1 entry point runs on the same engine, with another number of
    shifts, between the setter and the block and between the blocks."""
    T = CASES[tag].steps if steps is None else steps
    sh = shifts_of(tag) if shifts is None else np.asarray(shifts)
    eng = walks.engine(walk_of(tag))
    b = walks.ensemble(eng, walk_of(tag))

    def disturb_engine():
        other = walks.start_positions(walk_of(tag))[:5] * 0.9
        eng.one_body_density(other, np.linspace(-1.0, 2.0, 7))

    if others == 1:
        walks.set_others(b, isf=(4, 2, 2))
    if with_g1:
        b.set_obdm_estimator(sh, stride)
    if others == 2:
        walks.set_others(b, isf=(4, 2, 2))
    out = []
    for _ in range(blocks):
        if disturb:
            disturb_engine()
        ser, ssf, dens = b.run_block_est(T, eval_estimators)
        out.append((ser, ssf, dens,
                    b.read_pair_dist(T) if others else None,
                    b.read_isf(T) if others else None,
                    b.read_obdm(T) if with_g1 else None))
    b.close()
    eng.close()
    return out


@pytest.mark.parametrize('tag', list(CASES))
def test_rows_against_the_definition_and_the_batch_kernel(tag):
    T = CASES[tag].steps
    ref = reference(tag)
    sh = shifts_of(tag)
    K = sh.size
    if tag in PAIRDIST_WALKS:
        # the walk clones and the population changes
        walks.assert_transport_exercised(ref, walk_of(tag), tag)
    (ser, _, _, _, _, rows), = run_block_b(tag)
    print(tag, 'walkers', ref['num_walkers'])
    # the estimator does not touch the walk
    assert np.array_equal(ser.num_walkers, ref['num_walkers'])
    assert np.array_equal(ser.energy, ref['energy'])
    assert rows.shape == (T, K)
    worst_d = worst_b = 0.0
    for t in range(T):
        nw = int(ref['num_walkers'][t])
        g, x = ref['defn'][t], ref['batch'][t]
        assert g.shape == x.shape == (nw, K)
        want = g.sum(axis=0)
        bound = RTOL * np.maximum(1.0, np.abs(g)).sum(axis=0)
        err = np.abs(rows[t] - want)
        worst_d = max(worst_d, float((err / bound).max()))
        assert (err <= bound).all(), (t, np.argwhere(err > bound)[:4],
                                      err.max())
        exact = np.array([math.fsum(x[:, k]) for k in range(K)])
        bbound = nw * 2.0 ** -52 * np.abs(x).sum(axis=0)
        berr = np.abs(rows[t] - exact)
        with np.errstate(invalid='ignore', divide='ignore'):
            worst_b = max(worst_b, float(np.nanmax(
                np.where(bbound > 0, berr / bbound, 0.0))))
        assert (berr <= bbound).all(), (t, np.argwhere(berr > bbound)[:4],
                                        berr.max())
        # a zero shift: every walker contributes exactly 1
        for k in np.flatnonzero(sh == 0.0):
            assert rows[t, k] == nw
    print(tag, 'worst error / bound: definition %.3g, batch kernel %.3g'
          % (worst_d, worst_b))


@pytest.mark.parametrize('n', [5, 16, 64, 100])
def test_two_walkers_carry_the_batch_kernels_bits(n):
    """At most two walkers at the evaluated step: the row is the float sum of
    the batch kernel's g1 of the same configurations, bit for bit.

    "The same configuration" includes the order of its particles: g1 is a sum
    over the particles of products over the partners, and another order rounds
    differently (by an ulp: seen on the device at N = 5).  The ensemble keeps
    its rows sorted by position and `get_state` hands them out in the order of
    the start.  So the walkers start in ascending order, a fifth of the mean
    spacing apart at the least (17 diffusion lengths of a time step), and the
    test asserts that the configurations handed out are still ascending and
    inside the box: then both kernels see the same rows."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    seed = 31
    L = float(n)
    sh = np.array([0.0, 0.011, -0.37, 0.5, 1.2]) * L
    jitter = np.random.RandomState(seed).random_sample((2, n)) - 0.5
    pos0 = (np.arange(n) + 0.5 + 0.2 * jitter) * (L / n)
    eng = ModelEngine(box(n).cfc_spec, device=0)
    runs = []
    for with_g1 in (False, True):
        d = DmcEnsemble(eng, TIME_STEP, 4, 2, 0.5, rng_seed=seed)
        d.set_state(pos0)
        if with_g1:
            d.set_obdm_estimator(sh)
            ser, _, _ = d.run_block_est(1)
            runs.append((ser, d.read_obdm(1)))
        else:
            ser = d.run_block(1)
            s = d.get_state()
            runs.append((ser, s.confs[:int(s.num_walkers), 0, :].copy()))
        d.close()
    (ser_a, pos), (ser_b, rows) = runs
    nw = pos.shape[0]
    assert 1 <= nw <= 2, 'change the seed: the yardstick needs nw <= 2'
    assert int(ser_b.num_walkers[0]) == nw
    assert ser_a.energy.tobytes() == ser_b.energy.tobytes()
    assert (np.diff(pos, axis=1) > 0).all() and (pos > 0).all() and \
        (pos < L).all(), 'the rows were reordered: change the seed'
    x = eng.one_body_density(pos, sh)
    eng.close()
    want = x[0] + x[1] if nw == 2 else x[0]
    assert rows[0].tobytes() == want.tobytes(), (rows[0] - want)
    assert rows[0, 0] == nw


def test_stride_evaluates_every_third_step():
    tag, T = 'odd_k19', 7
    (s1, _, _, _, _, every), = run_block_b(tag, steps=T)
    (s3, _, _, _, _, third), = run_block_b(tag, steps=T, stride=3)
    assert every.shape == third.shape == (T, 19)
    assert every.any(axis=1).all()
    for t in (0, 3, 6):
        assert third[t].tobytes() == every[t].tobytes()
    for t in (1, 2, 4, 5):
        assert not third[t].any()
    assert s1.energy.tobytes() == s3.energy.tobytes()


def test_deterministic_and_burn_in():
    tag = 'wave'
    T, K = CASES[tag].steps, len(CASES[tag].shifts)
    (s1, _, _, _, _, r1), = run_block_b(tag)
    (s2, _, _, _, _, r2), = run_block_b(tag)
    assert r1.tobytes() == r2.tobytes()
    assert r1.all()
    # a burn-in block propagates the same walkers and leaves the rows zero
    (s0, _, _, _, _, r0), = run_block_b(tag, eval_estimators=False)
    assert r0.shape == (T, K) and not r0.any()
    assert np.array_equal(s0.energy, s1.energy)
    assert np.array_equal(s0.num_walkers, s1.num_walkers)


def test_independent_of_the_other_estimators():
    tag = 'odd_k19'
    alone, = run_block_b(tag)
    before, = run_block_b(tag, others=2)       # g1 set before the others
    after, = run_block_b(tag, others=1)        # g1 set after the others
    without, = run_block_b(tag, others=1, with_g1=False)
    assert alone[5].any()
    for both in (before, after):
        assert both[5].tobytes() == alone[5].tobytes()
        for k in (1, 2, 3, 4):
            assert both[k].any()
            assert both[k].tobytes() == without[k].tobytes()
    w = walk(tag)
    for run in (alone, before, after, without):
        assert np.array_equal(run[0].energy, w['energy'])
        assert np.array_equal(run[0].num_walkers, w['num_walkers'])


def test_shift_table_survives_other_calls_on_the_engine():
    tag = 'cap'
    quiet = run_block_b(tag, blocks=2)
    noisy = run_block_b(tag, blocks=2, disturb=True)
    for q, d in zip(quiet, noisy):
        assert q[5].all()
        assert q[5].tobytes() == d[5].tobytes()
    assert quiet[0][5].tobytes() != quiet[1][5].tobytes()
    # the first block is the twin's
    ref = reference(tag)
    assert np.array_equal(quiet[0][0].energy, ref['energy'])


def test_resetting_a_live_ensemble_equals_a_fresh_one():
    from phd_qmclib_amd.engine import DmcEnsemble
    from phd_qmclib_amd._lib import QmcError
    tag = 'many'
    w, T = walk_of(tag), CASES[tag].steps
    wide = shifts_of(tag)
    narrow = np.array([0.0, 1.7, -3.3])
    assert wide.size == 256
    eng = walks.engine(w)
    runs = []
    for todo in ([(wide, 2), (narrow, 1)], [(narrow, 1)]):   # R, then F
        d = DmcEnsemble(eng, TIME_STEP, w.maxw, w.nw0, 0.5, rng_seed=w.seed)
        for sh, q in todo:
            d.set_obdm_estimator(sh, q)
        assert np.array_equal(d.obdm_shifts, narrow)
        d.set_state(walks.start_positions(w))
        ser, _, _ = d.run_block_est(T)
        runs.append((ser, d.read_obdm(T)))
        if len(todo) == 2:
            d.set_obdm_estimator(None)
            assert d.obdm_shifts is None
            with pytest.raises(QmcError, match='one-body density'):
                d.read_obdm(1)
            # (the library says so too)
            out = np.zeros(3)
            assert d._lib.qmc_dmc_read_obdm(
                d._h, 1, out.ctypes.data_as(C.POINTER(C.c_double))) != 0
            assert b'one-body density' in d._lib.qmc_last_error()
            d.set_obdm_estimator(())
            assert d.obdm_shifts is None
        d.close()
    eng.close()
    (ser_r, g1_r), (ser_f, g1_f) = runs
    walks.assert_same_series(ser_r, ser_f)
    assert g1_r.shape == (T, 3) and g1_r.all()
    assert g1_r.tobytes() == g1_f.tobytes()
    assert np.array_equal(g1_r[:, 0], ser_r.num_walkers.astype(np.float64))


def test_bad_arguments_name_the_entry_point():
    tag = 'odd_k1'
    eng = walks.engine(walk_of(tag))
    d = walks.ensemble(eng, walk_of(tag))
    lib, dp = d._lib, C.POINTER(C.c_double)
    good = np.array([0.0, 0.5])

    def setter(nshift, arr, stride, handle=d._h):
        p = None if arr is None else arr.ctypes.data_as(dp)
        return lib.qmc_dmc_set_obdm_estimator(handle, nshift, p, stride)

    bad = [(-1, good, 1), (257, np.zeros(257), 1),
           (2, np.array([0.0, np.nan]), 1), (2, np.array([np.inf, 0.0]), 1),
           (2, good, 0), (2, good, 2 ** 31), (2, None, 1)]
    for nshift, arr, stride in bad:
        assert setter(nshift, arr, stride) != 0, (nshift, stride)
        assert b'qmc_dmc_set_obdm_estimator' in lib.qmc_last_error()
    assert setter(2, good, 1, handle=None) != 0
    assert b'qmc_dmc_set_obdm_estimator' in lib.qmc_last_error()
    # none of them left the estimator on, and the ensemble still steps
    out = np.zeros((8, 2))
    assert lib.qmc_dmc_read_obdm(d._h, 1, out.ctypes.data_as(dp)) != 0
    assert b'qmc_dmc_read_obdm' in lib.qmc_last_error()
    assert len(d.run_block(2).energy) == 2
    assert setter(2, good, 1) == 0
    d.obdm_shifts = good
    assert lib.qmc_dmc_read_obdm(d._h, 1, out.ctypes.data_as(dp)) != 0   # no block yet
    assert b'qmc_dmc_read_obdm' in lib.qmc_last_error()
    d.run_block_est(4)
    for nsteps in (0, -1, 5):
        assert lib.qmc_dmc_read_obdm(d._h, nsteps,
                                     out.ctypes.data_as(dp)) != 0
        assert b'qmc_dmc_read_obdm' in lib.qmc_last_error()
    assert lib.qmc_dmc_read_obdm(d._h, 4, None) != 0
    assert b'qmc_dmc_read_obdm' in lib.qmc_last_error()
    assert lib.qmc_dmc_read_obdm(None, 4, out.ctypes.data_as(dp)) != 0
    assert b'qmc_dmc_read_obdm' in lib.qmc_last_error()
    rows = d.read_obdm(4)
    assert rows.shape == (4, 2) and rows.all()
    assert len(d.run_block(2).energy) == 2
    d.close()
    eng.close()


def test_distributed_dmc_refuses_the_estimator():
    walks.assert_refused_by_distributed(
        WALKS['many'], lambda d: d.set_obdm_estimator([0.0, 1.0]),
        lambda d: d.set_obdm_estimator(None), 'one-body density', rng_seed=2)


# ---- top level ------------------------------------------------------------
def test_sampling_blocks_fill_iter_obdm():
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    confs = np.zeros((48, 2, 16))
    confs[:, 0, :] = walks.start_positions(WALKS['many'])
    kw = dict(max_num_walkers=64, target_num_walkers=48, rng_seed=13)
    sh = (0.0, 0.5, 2.0, 8.0)
    plain = mrbp_qmc.dmc.Sampling(spec, TIME_STEP, **kw)
    with_g1 = mrbp_qmc.dmc.Sampling(
        spec, TIME_STEP, obdm_est_spec=mrbp_qmc.dmc.OBDMEstSpec(sh, 2), **kw)
    assert np.array_equal(with_g1.obdm_shifts, sh)
    ini = plain.build_state(confs)
    b0 = list(islice(plain.blocks(ini, 6, 0), 2))
    b1 = list(islice(with_g1.blocks(ini, 6, 1), 2))
    for p, q in zip(b0, b1):
        assert p.iter_obdm is None and p.iter_pair_dist is None
        assert q.iter_density is None and q.iter_ssf is None
        assert q.iter_pair_dist is None and q.iter_isf is None
        assert q.iter_obdm.shape == (6, 4)
        assert p.iter_props.energy.tobytes() == q.iter_props.energy.tobytes()
    assert not b1[0].iter_obdm.any()                 # the burn-in block
    kept = b1[1].iter_obdm
    nw = b1[1].iter_props.num_walkers.astype(np.float64)
    assert np.array_equal(kept[::2, 0], nw[::2]) and kept[::2].all()
    assert not kept[1::2].any()


def test_proc_exec_yields_obdm_blocks(tmp_path):
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    dx = mrbp_qmc.dmc_exec
    spec = box(16)
    np.random.seed(5)
    K, q, nts = 4, 2, 8
    kw = dict(max_num_walkers=512, target_num_walkers=480, rng_seed=7,
              num_blocks=4, num_time_steps_block=nts, burn_in_blocks=1)
    on = dx.Proc(spec, TIME_STEP, obdm_spec=dx.OBDMEstSpec(K, None, q), **kw)
    din = dx.ProcInput.from_model_sys_conf_spec(
        dx.ModelSysConfSpec('RANDOM'), on)
    res = on.exec(din)
    blocks = res.data.blocks.obdm
    assert isinstance(blocks, dd.OBDMBlocks) and res.data.series is None
    assert blocks.totals.shape == (4, K)
    assert blocks.weight_totals.shape == (4, 1)
    assert np.array_equal(blocks.totals[:, 0], blocks.weight_totals[:, 0])
    g1, err = blocks.one_body_density()
    assert g1.shape == err.shape == (K,)
    assert g1[0] == 1.0 and err[0] == 0.0
    assert np.isfinite(g1).all() and np.isfinite(err).all()
    # (every term is an exponential; the walkers are a few steps from a
    # random start, far from psi_T phi_0, so nothing bounds g1 by 1 here)
    assert (g1[1:] > 0).all()
    shifts = on.obdm_spec.shifts(spec.supercell_size)
    assert np.array_equal(shifts, np.linspace(0, 8.0, K))
    nk, nk_err = blocks.momentum_distribution(
        shifts, 2 * pi * np.arange(3) / 16, spec)
    assert nk.shape == nk_err.shape == (3,) and np.isfinite(nk).all()
    # the kept series: totals and weights are sums over the evaluated steps
    kres = dx.Proc(spec, TIME_STEP, keep_iter_data=True,
                   obdm_spec=dx.OBDMEstSpec(K, None, q), **kw).exec(din)
    kept = kres.data.series.obdm_blocks
    assert kept.shape == (4, nts, K)
    nw = kres.data.series.iter_props_blocks.num_walkers.astype(np.float64)
    assert kept[:, ::q].all() and not kept[:, 1::q].any()
    kb = kres.data.blocks.obdm
    assert np.array_equal(kb.totals, kept[:, ::q].sum(axis=1))
    assert np.array_equal(kb.weight_totals[:, 0], nw[:, ::q].sum(axis=1))
    assert np.array_equal(kb.totals, blocks.totals)
    assert np.array_equal(kb.weight_totals, blocks.weight_totals)
    # HDF5 round trip
    path = tmp_path / 'dmc_obdm.h5'
    dx.HDF5FileHandler(str(path), 'run').dump(res)
    back = dx.HDF5FileHandler(str(path), 'run').load()
    assert back.proc.obdm_spec == on.obdm_spec
    assert np.array_equal(back.data.blocks.obdm.totals, blocks.totals)
    assert np.array_equal(back.data.blocks.obdm.weight_totals,
                          blocks.weight_totals)
    # the walk is the same with and without the estimator
    off = dx.Proc(spec, TIME_STEP, **kw).exec(din)
    assert off.data.blocks.obdm is None
    assert np.array_equal(off.data.blocks.energy.totals,
                          res.data.blocks.energy.totals)
