"""Host side of the DMC pair distribution estimator (no GPU): the forward
walking restatement against values written out by hand, the specs and the
configuration of a procedure, the block containers, the normalisation and the
result file."""
import numpy as np
import pytest

from phd_qmclib_amd.util import h5lite

from . import _pairdist_fw_restatement as fw

try:
    h5lite._load()
    HAVE_HDF5 = True
except h5lite.HDF5Unavailable:          # pragma: no cover
    try:
        import h5py  # noqa: F401
        HAVE_HDF5 = True
    except ImportError:
        HAVE_HDF5 = False

MODEL = dict(lattice_depth=24, lattice_ratio=1, interaction_strength=1.0,
             boson_number=16, supercell_size=16.0, tbf_contact_cutoff=4)


# ---- the restatement on a lineage small enough to follow by hand -----------
# N = 3, L = 8, B = 4: delta = 1, a pair with separation r counts in bin
# floor(r) (r <= 4); separations beyond L/2 = 4 fold back as 8 - r.
#
#   step 0   two walkers, no history          ref = [0, 1]
#            w0 (0, 0.5, 2.25)   r = 0.5, 2.25, 1.75          H = [1, 1, 1, 0]
#            w1 (0, 3.5, 7.25)   r = 3.5, 0.75 (7.25), 3.75   H = [1, 0, 0, 2]
#   step 1   walker 0 is cloned               ref = [0, 0, 1]
#            w0 = w1 (1, 1.5, 2.75)  r = 0.5, 1.75, 1.25      H = [1, 2, 0, 0]
#            w2 (0, 2.5, 5.25)   r = 2.5, 2.75 (5.25), 2.75   H = [0, 0, 3, 0]
#   step 2   walker 0 of step 1 dies          ref = [1, 2]
#            w0 (0, 0.25, 0.5)   r = 0.25, 0.5, 0.25          H = [3, 0, 0, 0]
#            w1 (0, 1.5, 3.25)   r = 1.5, 3.25, 1.75          H = [0, 2, 0, 1]
def _lineage():
    pad = [9.0, 9.1, 9.2]            # dead slots: must not count
    return [
        (np.array([[0, 0.5, 2.25], [0, 3.5, 7.25], pad, pad]),
         np.array([0, 1, 0, 0]), 2),
        (np.array([[1, 1.5, 2.75], [1, 1.5, 2.75], [0, 2.5, 5.25], pad]),
         np.array([0, 0, 1, 0]), 3),
        (np.array([[0, 0.25, 0.5], [0, 1.5, 3.25], pad, pad]),
         np.array([1, 2, 0, 0]), 2),
    ]


def test_forward_walking_by_hand():
    mixed, pure, amb = fw.forward_walk(_lineage(), 8.0, 4, pfw=2)
    assert amb == []
    assert np.array_equal(mixed, [[2, 1, 1, 2], [2, 4, 3, 0], [3, 2, 0, 1]])
    # pfw = 2 < 3 steps:
    #  t = 0  aux = H                                     / 1
    #  t = 1  aux[0] = aux[1] = [1,1,1,0] + [1,2,0,0] = [2,3,1,0],
    #         aux[2] = [1,0,0,2] + [0,0,3,0] = [1,0,3,2]  / 2
    #  t = 2  nothing is counted: aux[0] = old aux[1] = [2,3,1,0],
    #         aux[1] = old aux[2] = [1,0,3,2]             / 2
    assert np.array_equal(pure, [[2, 1, 1, 2], [2.5, 3, 2.5, 1],
                                 [1.5, 1.5, 2, 1]])
    # every walker holds N (N - 1) / 2 = 3 pairs per counted step
    nw = np.array([2, 3, 2])
    assert np.array_equal(mixed.sum(axis=1), 3 * nw)
    assert np.array_equal(pure.sum(axis=1), 3 * nw)
    # a long forward walk keeps counting: the last row over 3 steps
    _, pure3, _ = fw.forward_walk(_lineage(), 8.0, 4, pfw=99)
    assert np.array_equal(pure3[:2], pure[:2])
    #  aux[0] = [2,3,1,0] + [3,0,0,0], aux[1] = [1,0,3,2] + [0,2,0,1]
    assert np.array_equal(pure3[2], np.array([6., 5., 4., 3.]) / 3.0)


def test_forward_walking_accepts_state_confs_and_lists_edges():
    steps = _lineage()
    as_state = [(np.stack([c, np.zeros_like(c)], axis=1), r, n)
                for c, r, n in steps]
    a = fw.forward_walk(steps, 8.0, 4, pfw=2)
    b = fw.forward_walk(as_state, 8.0, 4, pfw=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a pair exactly on a bin edge is reported, with step and walker
    on_edge = [(np.array([[0.0, 1.0, 2.5]]), np.array([0]), 1)]
    _, _, amb = fw.forward_walk(on_edge, 8.0, 4, pfw=1)
    assert (0, 0, 0, 1, 1) in amb


# ---- specs and procedure ----------------------------------------------------
def test_spec_defaults():
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    s = dmc.PairDistEstSpec(32)
    assert (s.num_bins, s.as_pure_est, s.pfw_num_time_steps) == \
        (32, True, 99999999)
    assert dmc.PairDistEstSpec(8, False, 5).pfw_num_time_steps == 5
    e = dmc_exec.PairDistEstSpec(np.int64(12))
    assert (e.num_bins, e.as_pure_est) == (12, True)
    fields = [f.name for f in dmc.Sampling.__attrs_attrs__]
    assert fields[-1] == 'pair_dist_est_spec'
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    assert dmc_base.SamplingBlock._fields[-1] == 'iter_pair_dist'
    assert dmc_base.SamplingBlock._field_defaults['iter_pair_dist'] is None


def test_proc_from_config_and_sampling():
    from phd_qmclib_amd.mrbp_qmc import dmc_exec
    base = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                num_time_steps_block=8, max_num_walkers=12,
                target_num_walkers=10, rng_seed=5)
    proc = dmc_exec.Proc.from_config(dict(
        base, pair_dist_spec=dict(num_bins=24, as_pure_est=False)))
    assert proc.pair_dist_spec == dmc_exec.PairDistEstSpec(24, False)
    assert proc.should_eval_pair_dist
    cfg = proc.as_config()
    assert cfg['pair_dist_spec'] == dict(num_bins=24, as_pure_est=False)
    assert dmc_exec.Proc.from_config(cfg) == proc
    s = proc.sampling
    # the forward walking of a pure estimator spans one block
    assert s.pair_dist_est_spec.pfw_num_time_steps == 8
    assert s.pair_dist_est_spec.num_bins == 24
    assert not s.pair_dist_est_spec.as_pure_est
    assert np.allclose(s.pair_dist_bins, (np.arange(24) + 0.5) * 8.0 / 24)
    # without the spec nothing changes
    plain = dmc_exec.Proc.from_config(base)
    assert plain.pair_dist_spec is None and not plain.should_eval_pair_dist
    assert 'pair_dist_spec' not in plain.as_config()
    assert sorted(plain.as_config()) == sorted(
        ['model_spec', 'time_step', 'max_num_walkers', 'target_num_walkers',
         'num_walkers_control_factor', 'rng_seed', 'num_blocks',
         'num_time_steps_block', 'keep_iter_data', 'jit_parallel',
         'jit_fastmath', 'verbose'])
    assert plain.sampling.pair_dist_est_spec is None
    with pytest.raises(TypeError):
        plain.sampling.pair_dist_bins
    # the kernel-facing spec is as it was
    assert len(plain.sampling.cfc_spec) == 6


# ---- block containers ------------------------------------------------------
def _props(weight):
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    z = np.zeros_like(weight)
    return dmc_base.PropsData(z, weight, z.astype(np.uint64), z, z)


def test_pair_dist_blocks_from_data():
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    rng = np.random.RandomState(3)
    nb, nts, B = 5, 4, 6
    rows = rng.randint(0, 50, (nb, nts, B)).astype(np.float64)
    w = 1.0 + rng.rand(nb, nts)
    fac = 1.0 + rng.rand(nb)
    # kept per step (`reduce_data`: the container reduces the steps itself)
    mixed = dd.PairDistBlocks.from_data(nts, rows, _props(w), True, False)
    assert np.array_equal(mixed.totals, rows.sum(axis=1))
    assert np.array_equal(mixed.weight_totals, w.sum(axis=1)[:, None])
    pure = dd.PairDistBlocks.from_data(nts, rows, _props(w), True, True, fac)
    assert np.array_equal(pure.totals, rows[:, -1, :])
    assert np.array_equal(pure.weight_totals, w[:, -1][:, None])
    # already reduced by the block loop
    wb = w.sum(axis=1)
    mixed_r = dd.PairDistBlocks.from_data(nts, rows.sum(axis=1), _props(wb),
                                          False, False)
    assert np.array_equal(mixed_r.totals, mixed.totals)
    assert np.array_equal(mixed_r.weight_totals, mixed.weight_totals)
    pure_r = dd.PairDistBlocks.from_data(nts, rows[:, -1, :], _props(wb),
                                         False, True, fac)
    assert np.array_equal(pure_r.totals, pure.totals)
    assert np.array_equal(pure_r.weight_totals, (wb * fac)[:, None])
    assert isinstance(mixed, dd.SetPropBlocks)
    assert mixed.mean.shape == (B,) and len(mixed) == nb
    both = mixed + mixed_r
    assert isinstance(both, dd.PairDistBlocks) and len(both) == 2 * nb
    assert [f.name for f in dd.PropsDataBlocks.__attrs_attrs__][-1] == \
        'pair_dist'


def test_uniform_counts_normalise_to_one():
    """N (N - 1) / 2 pairs spread evenly over the bins: g2 = 1 in every bin."""
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    spec = mrbp_qmc.Spec(**MODEL)
    n, B, nb = 16, 8, 6
    per_bin = n * (n - 1) / 2 / B                   # 15 pairs
    nw = np.array([10., 12., 9., 11., 10., 12.])    # walkers of a block
    blocks = dd.PairDistBlocks(np.outer(nw, np.full(B, per_bin)),
                               np.tile(nw[:, None], (1, B)))
    r, g2, err = blocks.pair_distribution(spec)
    assert np.array_equal(r, (np.arange(B) + 0.5) * 1.0)
    assert np.allclose(g2, 1.0, rtol=0, atol=1e-14)
    assert err.shape == (B,)


@pytest.mark.skipif(not HAVE_HDF5, reason='no HDF5 library')
def test_result_file_roundtrip(tmp_path):
    from phd_qmclib_amd.mrbp_qmc import dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    proc = dmc_exec.Proc.from_config(dict(
        model_spec=MODEL, time_step=1e-3, num_blocks=6, num_time_steps_block=8,
        max_num_walkers=12, target_num_walkers=10, rng_seed=5,
        pair_dist_spec=dict(num_bins=7, as_pure_est=True)))
    rng = np.random.RandomState(0)
    props = dmc_base.StateProps(rng.rand(12), rng.rand(12),
                                np.arange(12) >= 10)
    state = dmc_base.State(
        confs=rng.rand(12, 2, 16), props=props, energy=3.5, weight=9.75,
        num_walkers=10, ref_energy=0.35, accum_energy=0.36, max_num_walkers=12,
        branching_spec=dmc_base.BranchingSpec(np.ones(12, np.int64),
                                              np.arange(12)[::-1].copy()))
    w = rng.rand(6)
    pd = dd.PairDistBlocks(rng.randint(0, 99, (6, 7)).astype(np.float64),
                           np.tile(w[:, None], (1, 7)))
    data = dd.SamplingData(dd.PropsDataBlocks(
        dd.EnergyBlocks(rng.rand(6), w), dd.WeightBlocks(w),
        dd.NumWalkersBlocks(rng.randint(8, 12, 6).astype(np.uint64)),
        pair_dist=pd))
    h = dmc_exec.HDF5FileHandler(str(tmp_path / 'r.h5'), 'run-A')
    h.dump(dmc_exec.ProcResult(state, proc, data))
    with h5lite.open_file(h.location, 'r') as f:
        q = f['run-A/dmc']
        assert sorted(q['proc_spec'].keys()) == ['model_spec',
                                                 'pair_dist_spec']
        assert q['proc_spec/pair_dist_spec'].attrs['num_bins'] == 7
        assert sorted(q['data/blocks'].keys()) == [
            'energy', 'num_walkers', 'pair_dist', 'weight']
        assert sorted(q['data/blocks/pair_dist'].keys()) == ['totals',
                                                             'weight_totals']
    back = h.load()
    assert back.proc == proc
    b = back.data.blocks
    assert isinstance(b.pair_dist, dd.PairDistBlocks)
    assert np.array_equal(b.pair_dist.totals, pd.totals)
    assert np.array_equal(b.pair_dist.weight_totals, pd.weight_totals)
    assert b.density is None and b.ss_factor is None
    r, g2, err = b.pair_dist.pair_distribution(back.proc.model_spec)
    assert r.shape == g2.shape == err.shape == (7,)
