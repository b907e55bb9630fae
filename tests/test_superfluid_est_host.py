"""Host side of the DMC centre-of-mass diffusion estimator (no GPU): the
restatement against values written out by hand, the normalisation, the block
container, the specs and the configuration of a procedure, the result file and
the signature table."""
import numpy as np
import pytest

from phd_qmclib_amd.util import h5lite

from . import _cmdiff_restatement as cm

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
# N = 2, L = 8; every number is a multiple of 1/4, so the arithmetic is exact.
#
#   step 0   two walkers, the origin                  ref = [0, 1]    Y = 0, 0
#            w0 (1, 2)  X = 3          w1 (7.5, 3)  X = 10.5
#   step 1   walker 0 is cloned                       ref = [0, 0, 1]
#            w0 (1.25, 2.25)  X = 3.5    raw = 0.5              Y = 0.5
#            w1 (0.75, 2)     X = 2.75   raw = -0.25            Y = -0.25
#            w2 (0.25, 3.25)  X = 3.5    raw = -7: its first particle went
#               from 7.5 over the edge to 8.25 = 0.25; d = -7 + 8 = 1, Y = 1
#   step 2   walker 0 of step 1 dies                  ref = [1, 2]
#            w0 (2.5, 0.5)  X = 3: the row is stored the other way round,
#               (0.5, 2.5) after (0.75, 2); raw = 0.25   Y = -0.25 + 0.25 = 0
#            w1 (7.75, 3.5) X = 11.25: back over the edge, 0.25 -> -0.25;
#               raw = 7.75, d = -0.25                    Y = 1 - 0.25 = 0.75
def _lineage():
    pad = [5.0, 5.5]                 # dead slots: must not count
    return [
        (np.array([[1, 2], [7.5, 3], pad, pad]), np.array([0, 1, 0, 0]), 2),
        (np.array([[1.25, 2.25], [0.75, 2], [0.25, 3.25], pad]),
         np.array([0, 0, 1, 0]), 3),
        (np.array([[2.5, 0.5], [7.75, 3.5], pad, pad]),
         np.array([1, 2, 0, 0]), 2),
    ]


def test_restatement_by_hand():
    rows, wrapped, max_d = cm.cm_diffusion(_lineage(), 8.0)
    #  t = 1   Y = (0.5, -0.25, 1)      t = 2   Y = (0, 0.75)
    assert np.array_equal(rows, [[0, 0], [1.25, 1.3125], [0.75, 0.5625]])
    assert wrapped == 2              # w2 at step 1, w1 at step 2
    assert max_d == 1.0
    assert cm.largest_y(_lineage(), 8.0) == 1.0


def test_restatement_lineage_properties():
    steps = _lineage()
    rows = cm.cm_diffusion(steps, 8.0)[0]
    # a clone inherits the Y of its parent: with the clone's own move undone
    # (w1 of step 1 a copy of w0) both carry the same Y
    same = [(c.copy(), r, n) for c, r, n in steps]
    same[1][0][1] = same[1][0][0]
    r2 = cm.cm_diffusion(same[:2], 8.0)[0]
    assert np.array_equal(r2[1], [0.5 + 0.5 + 1, 0.25 + 0.25 + 1])
    # a dead walker's history ends: whatever walker 0 of step 1 carried, it
    # does not reach step 2 (nobody descends from it)
    other = [(c.copy(), r, n) for c, r, n in steps]
    other[1][0][0] = [3.25, 2.25]             # Y = 2.5 instead of 0.5
    r3 = cm.cm_diffusion(other, 8.0)[0]
    assert np.array_equal(r3[1], [2.5 - 0.25 + 1, 6.25 + 0.0625 + 1])
    assert np.array_equal(r3[2], rows[2])
    # a permuted row, or a particle wrapped by L, gives the same answer
    perm = [(c[:, ::-1].copy(), r, n) for c, r, n in steps]
    assert np.array_equal(cm.cm_diffusion(perm, 8.0)[0], rows)
    moved = [(c.copy(), r, n) for c, r, n in steps]
    moved[2][0][1][1] += 8.0
    assert np.array_equal(cm.cm_diffusion(moved, 8.0)[0], rows)
    # State-shaped confs[W, 2, N] are accepted
    as_state = [(np.stack([c, np.zeros_like(c)], axis=1), r, n)
                for c, r, n in steps]
    assert np.array_equal(cm.cm_diffusion(as_state, 8.0)[0], rows)
    # the dead slots do not count
    junk = [(c.copy(), r, n) for c, r, n in steps]
    for c, _, n in junk:
        c[n:] += 1.75
    assert np.array_equal(cm.cm_diffusion(junk, 8.0)[0], rows)


# ---- normalisation ---------------------------------------------------------
def test_superfluid_ratio_normalisation():
    from phd_qmclib_amd.engine import superfluid_ratio
    n, dt, nts = 5, 0.25, 6
    nw = np.array([7, 8, 9, 8, 7, 10], dtype=np.uint64)
    t = np.arange(nts)
    # free diffusion of N particles: <Y^2> = 2 N t dt per walker
    iter_cm = np.stack([np.full(nts, 123.0), 2 * n * t * dt * nw], axis=1)
    tau, ratio = superfluid_ratio(iter_cm, nw, n, dt)
    assert np.array_equal(tau, [0.25, 0.5, 0.75, 1.0, 1.25])
    assert np.array_equal(ratio, np.ones(nts - 1))
    # one factor each: a third of the mean square, a third of the ratio
    _, third = superfluid_ratio(iter_cm / 3.0, nw, n, dt)
    assert np.allclose(third, 1.0 / 3.0, rtol=1e-15, atol=0)
    _, twice_n = superfluid_ratio(iter_cm, nw, 2 * n, dt)
    assert np.array_equal(twice_n, np.full(nts - 1, 0.5))
    _, twice_dt = superfluid_ratio(iter_cm, nw, n, 2 * dt)
    assert np.array_equal(twice_dt, np.full(nts - 1, 0.5))


# ---- block container -------------------------------------------------------
def test_cm_diffusion_blocks_on_synthetic_curves():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    from phd_qmclib_amd.stats import reblock
    spec = mrbp_qmc.Spec(**MODEL)
    n, dt, nb, nts = 16, 0.125, 8, 5
    t = np.arange(nts)
    rng = np.random.RandomState(4)
    # blocks scattered around a curve with rho_s / rho = 0.75
    curves = 0.75 * 2 * n * t * dt * (1 + 0.01 * rng.standard_normal((nb, 1)))
    blocks = dd.CMDiffusionBlocks(curves)
    assert isinstance(blocks, dd.UnWeightedPropBlocks) and len(blocks) == nb
    assert blocks.mean.shape == (nts,)
    tau, ratio, err = blocks.superfluid_fraction(spec, dt)
    assert np.array_equal(tau, t[1:] * dt)
    assert tau.shape == ratio.shape == err.shape == (nts - 1,)
    norm = 2 * n * tau
    assert np.allclose(ratio, curves.mean(axis=0)[1:] / norm, rtol=1e-14)
    assert np.allclose(ratio, 0.75, rtol=0.02)
    # the error per lag is the project's reblocking over the blocks
    want = reblock.OTFSet.from_non_obj_data(
        curves[:, 1:]).mean_eff_error / norm
    assert np.array_equal(err, want)
    assert (err > 0).all() and (err < 0.01 * 0.75).all()
    # exact curves (with one block off, so that there is a scatter to
    # reblock): the ratio follows the mean of the blocks
    flat = np.tile(2 * n * t * dt, (nb, 1))
    flat[0] *= 1.5
    exact = dd.CMDiffusionBlocks(flat)
    _, lifted, _ = exact.superfluid_fraction(spec, dt)
    assert np.allclose(lifted, 1 + 0.5 / nb, rtol=1e-14, atol=0)
    both = blocks + exact
    assert isinstance(both, dd.CMDiffusionBlocks) and len(both) == 2 * nb
    names = [f.name for f in dd.PropsDataBlocks.__attrs_attrs__]
    assert 'cm_diffusion' in names
    assert dd.PropsDataSeries(None).cm_diffusion_blocks is None


# ---- specs and procedure ----------------------------------------------------
def test_specs_and_block_field():
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    assert dmc.SuperfluidEstSpec() == dmc.SuperfluidEstSpec()
    assert dmc_exec.SuperfluidEstSpec() == dmc_exec.SuperfluidEstSpec()
    fields = {f.name: f for f in dmc.Sampling.__attrs_attrs__}
    assert fields['superfluid_est_spec'].default is None
    assert 'iter_cm_diffusion' in dmc_base.SamplingBlock._fields
    assert dmc_base.SamplingBlock._field_defaults['iter_cm_diffusion'] is None
    blk = dmc_base.SamplingBlock(None, None, iter_cm_diffusion=np.zeros((3, 2)))
    assert blk.iter_cm_diffusion.shape == (3, 2) and blk.iter_pair_dist is None


def test_proc_from_config_and_sampling():
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    base = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                num_time_steps_block=8, max_num_walkers=12,
                target_num_walkers=10, rng_seed=5)
    for given in ({}, True):
        proc = dmc_exec.Proc.from_config(dict(base, superfluid_spec=given))
        assert proc.superfluid_spec == dmc_exec.SuperfluidEstSpec()
        assert proc.should_eval_superfluid
    cfg = proc.as_config()
    assert cfg['superfluid_spec'] == {}
    assert dmc_exec.Proc.from_config(cfg) == proc
    s = proc.sampling
    assert s.superfluid_est_spec == dmc.SuperfluidEstSpec()
    assert s.pair_dist_est_spec is None and s.density_est_spec is None
    # without the spec nothing changes
    for absent in (base, dict(base, superfluid_spec=None),
                   dict(base, superfluid_spec=False)):
        plain = dmc_exec.Proc.from_config(absent)
        assert plain.superfluid_spec is None
        assert not plain.should_eval_superfluid
        assert 'superfluid_spec' not in plain.as_config()
        assert plain.sampling.superfluid_est_spec is None
    # the kernel-facing spec is as it was
    assert len(s.cfc_spec) == 6


@pytest.mark.skipif(not HAVE_HDF5, reason='no HDF5 library')
def test_result_file_roundtrip(tmp_path):
    from phd_qmclib_amd.mrbp_qmc import dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    rng = np.random.RandomState(0)
    props = dmc_base.StateProps(rng.rand(12), rng.rand(12),
                                np.arange(12) >= 10)
    state = dmc_base.State(
        confs=rng.rand(12, 2, 16), props=props, energy=3.5, weight=9.75,
        num_walkers=10, ref_energy=0.35, accum_energy=0.36, max_num_walkers=12,
        branching_spec=dmc_base.BranchingSpec(np.ones(12, np.int64),
                                              np.arange(12)[::-1].copy()))
    w = rng.rand(6)
    curves = rng.rand(6, 8)
    for on in (True, False):
        cfg = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                   num_time_steps_block=8, max_num_walkers=12,
                   target_num_walkers=10, rng_seed=5)
        if on:
            cfg['superfluid_spec'] = {}
        proc = dmc_exec.Proc.from_config(cfg)
        data = dd.SamplingData(dd.PropsDataBlocks(
            dd.EnergyBlocks(rng.rand(6), w), dd.WeightBlocks(w),
            dd.NumWalkersBlocks(rng.randint(8, 12, 6).astype(np.uint64)),
            cm_diffusion=dd.CMDiffusionBlocks(curves) if on else None))
        h = dmc_exec.HDF5FileHandler(str(tmp_path / f'r{int(on)}.h5'), 'run-A')
        h.dump(dmc_exec.ProcResult(state, proc, data))
        with h5lite.open_file(h.location, 'r') as f:
            q = f['run-A/dmc']
            extra = ['superfluid_spec'] if on else []
            assert sorted(q['proc_spec'].keys()) == ['model_spec'] + extra
            extra = ['cm_diffusion'] if on else []
            assert sorted(q['data/blocks'].keys()) == sorted(
                ['energy', 'num_walkers', 'weight'] + extra)
            if on:
                assert sorted(q['data/blocks/cm_diffusion'].keys()) == \
                    ['totals']
        back = h.load()
        assert back.proc == proc
        b = back.data.blocks
        assert b.density is None and b.pair_dist is None
        if on:
            assert isinstance(b.cm_diffusion, dd.CMDiffusionBlocks)
            assert np.array_equal(b.cm_diffusion.totals, curves)
            tau, ratio, err = b.cm_diffusion.superfluid_fraction(
                back.proc.model_spec, back.proc.time_step)
            assert tau.shape == ratio.shape == err.shape == (7,)
        else:
            assert b.cm_diffusion is None


# ---- the C interface --------------------------------------------------------
def test_signature_table_lists_the_entry_points():
    import ctypes as C
    from phd_qmclib_amd import _lib
    sig = _lib.SIGNATURES
    assert sig['qmc_dmc_set_cm_diffusion_estimator'] == \
        (C.c_int, [C.c_void_p, C.c_int32])
    res, args = sig['qmc_dmc_read_cm_diffusion']
    assert res is C.c_int and len(args) == 3
    assert args[:2] == [C.c_void_p, C.c_int64]
    assert args[2] == sig['qmc_dmc_read_pair_dist'][1][2]
