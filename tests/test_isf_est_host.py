"""Host side of the DMC imaginary-time density correlation estimator F(k, tau)
(no GPU): the restatement against values written out by hand, its lag-0
identity with the oracle's pure S(k) parts, the free-gas rule on Brownian
paths, the normalisation, the block container, the specs and the configuration
of a procedure, the result file and the signature table."""
from math import pi

import numpy as np
import pytest

from phd_qmclib_amd.util import h5lite

from . import _isf_restatement as isf

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
# N = 2, L = 8, K = 3 modes (k_1 = pi / 4, k_2 = pi / 2), T = 3 lags, q = 1;
# every position is even, so every exp(i k z) is a power of i.
#
#   step 0   two walkers, the origin                     ref = [0, 1]
#            w0 (0, 2)   rho_1 = 1 + i     rho_2 = 1 - 1 = 0
#            w1 (2, 2)   rho_1 = 2i        rho_2 = -2
#   step 1   walker 0 is cloned                          ref = [0, 0, 1]
#            w0 (0, 0)   rho_1 = 2         rho_2 = 2     origin: w0 of step 0
#            w1 (2, 4)   rho_1 = -1 + i    rho_2 = 0     origin: w0 of step 0
#            w2 (4, 4)   rho_1 = -2        rho_2 = 2     origin: w1 of step 0
#            lag 1, Re rho(1) conj rho(0):
#              m = 1: Re 2 (1 - i) = 2;  Re (-1 + i)(1 - i) = 0;  Re -2 (-2i) = 0
#              m = 2: 2 * 0 = 0;  0;  2 * (-2) = -4
#   step 2   walker 0 of step 1 dies                     ref = [1, 2]
#            w0 (2, 6)   rho_1 = i - i = 0   rho_2 = -2  origin: w0 of step 0
#            w1 (0, 2)   rho_1 = 1 + i       rho_2 = 0   origin: w1 of step 0
#            lag 2:  m = 1: 0;  Re (1 + i)(-2i) = 2      m = 2: -2 * 0;  0 * -2
# rho_0 = 2 for everybody: every measured column of m = 0 is 4 per walker.
def _lineage():
    pad = [5.0, 5.5]                 # dead slots: must not count
    return [
        (np.array([[0, 2], [2, 2], pad, pad]), np.array([0, 1, 0, 0]), 2),
        (np.array([[0, 0], [2, 4], [4, 4], pad]), np.array([0, 0, 1, 0]), 3),
        (np.array([[2, 6], [0, 2], pad, pad]), np.array([1, 2, 0, 0]), 2),
    ]


#                 lag 0  lag 1  lag 2  Re rho(0)  Im rho(0)
BY_HAND = np.array([
    [[8, 0, 0, 4, 0],            # step 0, m = 0
     [2 + 4, 0, 0, 1 + 0, 1 + 2],
     [0 + 4, 0, 0, 0 - 2, 0]],
    [[12, 12, 0, 6, 0],          # step 1: w0's row counts twice
     [2 + 2 + 4, 2 + 0 + 0, 0, 1 + 1 + 0, 1 + 1 + 2],
     [0 + 0 + 4, 0 + 0 - 4, 0, 0 + 0 - 2, 0]],
    [[8, 8, 8, 4, 0],            # step 2: the rows of w1 and w2 of step 1
     [2 + 4, 0 + 0, 0 + 2, 1 + 0, 1 + 2],
     [0 + 4, 0 - 4, 0 + 0, 0 - 2, 0]],
], dtype=np.float64)


def test_restatement_by_hand():
    rows = isf.isf_rows(_lineage(), 8.0, 3, 3, 1)
    assert rows.shape == (3, 3, 5)
    # (cos(pi / 2) is 6e-17 in floating point, not 0)
    assert np.abs(rows - BY_HAND).max() < 1e-14
    # a block shorter than the lags: what was not measured is exactly zero
    assert not rows[0][:, 1:3].any() and not rows[1][:, 2].any()


def test_restatement_lineage_properties():
    steps = _lineage()
    rows = isf.isf_rows(steps, 8.0, 3, 3, 1)
    # a dead walker's row ends: whatever walker 0 of step 1 carried, it does
    # not reach step 2
    other = [(c.copy(), r, n) for c, r, n in steps]
    other[1][0][0] = [1.0, 3.5]
    r2 = isf.isf_rows(other, 8.0, 3, 3, 1)
    assert not np.array_equal(r2[1], rows[1])
    assert np.array_equal(r2[2], rows[2])
    # State-shaped confs[W, 2, N] are accepted, the dead slots do not count
    as_state = [(np.stack([c, np.zeros_like(c)], axis=1), r, n)
                for c, r, n in steps]
    assert np.array_equal(isf.isf_rows(as_state, 8.0, 3, 3, 1), rows)
    junk = [(c.copy(), r, n) for c, r, n in steps]
    for c, _, n in junk:
        c[n:] += 1.75
    assert np.array_equal(isf.isf_rows(junk, 8.0, 3, 3, 1), rows)
    # lag stride 2: lag 1 is measured at step 2, with step 2's rho against
    # the origin; step 1 measures nothing and only transports
    q2 = isf.isf_rows(steps, 8.0, 3, 3, 2)
    assert np.array_equal(q2[0], rows[0])
    assert np.array_equal(q2[2][:, 1], rows[2][:, 2])
    assert not q2[1][:, 1:3].any() and not q2[2][:, 2].any()
    assert np.array_equal(q2[1][:, [0, 3, 4]], rows[1][:, [0, 3, 4]])
    # one lag only: the origin and lag 0, transported
    t1 = isf.isf_rows(steps, 8.0, 3, 1, 1)
    assert t1.shape == (3, 3, 3)
    assert np.array_equal(t1, rows[:, :, [0, 3, 4]])


def _random_block(num_steps, n=7, maxw=12, seed=3):
    """A made-up block with clones and deaths -> steps."""
    rng = np.random.RandomState(seed)
    steps, nw = [], 9
    for t in range(num_steps):
        new_nw = nw if t == 0 else int(rng.randint(6, maxw + 1))
        ref = np.zeros(maxw, dtype=np.int64)
        ref[:new_nw] = np.arange(new_nw) if t == 0 else \
            np.sort(rng.randint(0, nw, new_nw))
        steps.append((n * rng.random_sample((maxw, n)), ref, new_nw))
        nw = new_nw
    return steps


def test_mode_zero_is_n_squared_in_every_measured_column():
    n, K, T, q = 7, 4, 3, 2
    steps = _random_block(8, n=n)
    rows = isf.isf_rows(steps, float(n), K, T, q)
    for t, (_, _, nw) in enumerate(steps):
        measured = min(t // q, T - 1) + 1
        assert np.array_equal(rows[t, 0, :measured], np.full(measured, nw * n * n))
        assert not rows[t, :, measured:T].any()
        assert rows[t, 0, T] == nw * n and rows[t, 0, T + 1] == 0
    assert len({s[2] for s in steps}) > 1


# ---- lag-0 identity with the oracle's pure S(k) ------------------------------
def oracle_block(oracle, n=16, nw0=48, maxw=64, num_steps=10, seed=13):
    """One oracle population -> steps."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=n, supercell_size=n,
                tbf_contact_cutoff=0.25 * n)
    m = oracle.model_from_cfc(spec.cfc_spec)
    pos = n * np.random.RandomState(seed).random_sample((nw0, n))
    o = oracle.DmcEnsemble(m, pos, 1e-3, maxw, nw0, 0.5, seed=seed)
    steps = []
    for _ in range(num_steps):
        y = o.step()
        steps.append((o.confs.copy(), o.cloning_ref.copy(),
                      int(y.num_walkers)))
    return steps


def test_lag_zero_columns_equal_the_pure_ssf_parts(oracle):
    """Columns 0, T, T+1 of a row are |rho|^2, Re rho, Im rho of the origin,
    transported through the cloning table: what the pure S(k) estimator with a
    forward-walking length of one step carries."""
    n, maxw, nts, K, T = 16, 64, 10, 8, 4
    steps = oracle_block(oracle, n=n, maxw=maxw, num_steps=nts)
    est = oracle.DmcEstimators(float(n), n, maxw, nts, ssf=(K, True, 1))
    for t, (confs, ref, nw) in enumerate(steps):
        est.step(t, confs, nw, ref)
    moved = sum(not np.array_equal(r[:nw], np.arange(nw))
                for _, r, nw in steps)
    sizes = {nw for _, _, nw in steps}
    print('non-identity cloning tables', moved, 'population', sorted(sizes))
    assert moved >= 1 and len(sizes) > 1
    for q in (1, 2):
        rows = isf.isf_rows(steps, float(n), K, T, q)
        for t in range(nts):
            assert np.array_equal(rows[t][:, [0, T, T + 1]], est.iter_ssf[t])


# ---- the free-gas rule on Brownian paths ------------------------------------
def test_free_particles_decay_as_exp_minus_k_squared_tau():
    """Independent particles diffusing with variance 2 tau from a uniform
    start, unit weights, no branching: E[iter[t][m][l]] / nw =
    N exp(-k_m^2 tau_l).  4096 walkers: the deviation of one block is
    asserted within 5 standard errors of the walker average, and the standard
    error itself is below N / sqrt(nw) (|rho|^2 fluctuates by about N)."""
    n, nw, dt, K, T, q, nts = 8, 4096, 1e-2, 4, 4, 8, 32
    rng = np.random.RandomState(21)
    pos = n * rng.random_sample((nw, n))
    ident = np.arange(nw)
    steps = []
    for _ in range(nts):
        steps.append((pos.copy(), ident, nw))
        pos = pos + np.sqrt(2 * dt) * rng.standard_normal((nw, n))
    rows = isf.isf_rows(steps, float(n), K, T, q)
    k = isf.momenta(K, n)
    tau = np.arange(T) * q * dt
    want = n * np.exp(-np.outer(k ** 2, tau))
    got = rows[-1][:, :T] / nw
    assert np.allclose(got[0], n * n, rtol=1e-13)
    err = np.abs(got[1:] - want[1:])
    print(got[1:], want[1:])
    assert (err <= 5 * n / np.sqrt(nw)).all()


# ---- normalisation ---------------------------------------------------------
def test_intermediate_scattering_normalisation():
    from phd_qmclib_amd.engine import intermediate_scattering
    n, dt, K, T, q, nts = 5, 0.25, 3, 2, 3, 6
    nw = np.array([7, 8, 9, 8, 7, 10], dtype=np.uint64)
    rng = np.random.RandomState(2)
    iter_isf = rng.random_sample((nts, K, T + 2))
    tau, f, rho = intermediate_scattering(iter_isf, nw, n, dt, q)
    assert np.array_equal(tau, [0.0, 0.75])
    assert f.shape == (T, K) and rho.shape == (K,) and rho.dtype == complex
    # the last step over its own population, per particle
    assert np.array_equal(f, (iter_isf[-1][:, :T] / 10.0).T / n)
    assert np.array_equal(rho.real, iter_isf[-1][:, T] / 10.0)
    assert np.array_equal(rho.imag, iter_isf[-1][:, T + 1] / 10.0)
    # a crystal at rest, rho_m = N at every time: F / N = N, connected part 0
    still = np.zeros((nts, K, T + 2))
    still[..., :T] = (n * n * nw)[:, None, None]
    still[..., T] = (n * nw)[:, None]
    _, f, rho = intermediate_scattering(still, nw, n, dt, q)
    assert np.array_equal(f, np.full((T, K), float(n)))
    assert np.array_equal(f * n - np.abs(rho) ** 2, np.zeros((T, K)))


# ---- block container -------------------------------------------------------
def test_isf_blocks_on_synthetic_rows():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    from phd_qmclib_amd.stats import reblock
    spec = mrbp_qmc.Spec(**MODEL)
    n, dt, nb, K, T, q = 16, 0.125, 8, 3, 4, 2
    rng = np.random.RandomState(4)
    tau_want = np.arange(T) * q * dt
    gap = np.array([0.0, 1.0, 2.5])
    clean = np.zeros((K, T + 2))
    clean[:, :T] = n * np.exp(-np.outer(gap, tau_want))
    clean[0, :T] = n * n
    clean[:, T] = [n, 0.5, 0.125]
    clean[:, T + 1] = [0.25, -0.25, 0.5]
    rows = clean * (1 + 0.01 * rng.standard_normal((nb, 1, 1)))
    blocks = dd.ISFBlocks(rows)
    assert isinstance(blocks, dd.UnWeightedPropBlocks) and len(blocks) == nb
    tau, f, err, conn = blocks.scattering_function(spec, dt, lag_stride=q)
    assert np.array_equal(tau, tau_want)
    assert f.shape == err.shape == conn.shape == (T, K)
    mean = rows.mean(axis=0)
    assert np.allclose(f, mean[:, :T].T / n, rtol=1e-14)
    assert np.allclose(f, clean[:, :T].T / n, rtol=0.02)
    want = reblock.OTFSet.from_non_obj_data(
        rows.reshape(nb, -1)).mean_eff_error.reshape(K, T + 2)
    assert np.array_equal(err, want[:, :T].T / n)
    assert (err > 0).all()
    rho_sqr = mean[:, T] ** 2 + mean[:, T + 1] ** 2
    assert np.allclose(conn, (mean[:, :T] - rho_sqr[:, None]).T / n,
                       rtol=1e-13, atol=1e-13)
    # m = 0: rho_0 is N (almost, here), little is left of the connected
    # function
    assert np.abs(conn[:, 0]).max() < 1e-2 * n
    # the default stride is one time step per lag
    assert np.array_equal(blocks.scattering_function(spec, dt)[0],
                          np.arange(T) * dt)
    both = blocks + dd.ISFBlocks(rows[:3])
    assert isinstance(both, dd.ISFBlocks) and len(both) == nb + 3
    names = [f.name for f in dd.PropsDataBlocks.__attrs_attrs__]
    assert 'isf' in names and names[-1] == 'pair_dist'
    assert dd.PropsDataSeries(None).isf_blocks is None


# ---- specs and procedure ----------------------------------------------------
def test_specs_and_block_field():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    assert dmc.ISFEstSpec(8, 4) == dmc.ISFEstSpec(8, 4, 1)
    assert dmc.ISFEstSpec(8, 4, 2).lag_stride == 2
    assert dmc_exec.ISFEstSpec(np.int64(8), 4) == dmc_exec.ISFEstSpec(8, 4, 1)
    fields = [f.name for f in dmc.Sampling.__attrs_attrs__]
    assert 'isf_est_spec' in fields and fields[-1] == 'pair_dist_est_spec'
    by_name = {f.name: f for f in dmc.Sampling.__attrs_attrs__}
    assert by_name['isf_est_spec'].default is None
    assert by_name['isf_est_spec'].kw_only
    assert 'iter_isf' in dmc_base.SamplingBlock._fields
    assert dmc_base.SamplingBlock._fields[-1] == 'iter_pair_dist'
    assert dmc_base.SamplingBlock._field_defaults['iter_isf'] is None
    blk = dmc_base.SamplingBlock(None, None, iter_isf=np.zeros((3, 2, 4)))
    assert blk.iter_isf.shape == (3, 2, 4) and blk.iter_pair_dist is None
    assert blk.iter_cm_diffusion is None
    s = dmc.Sampling(mrbp_qmc.Spec(**MODEL), 1e-3, 12, 10, rng_seed=1,
                     isf_est_spec=dmc.ISFEstSpec(5, 3, 2))
    assert np.allclose(s.isf_momenta, np.arange(5) * 2 * pi / 16.0, rtol=1e-15)
    with pytest.raises(TypeError):
        dmc.Sampling(mrbp_qmc.Spec(**MODEL), 1e-3, 12, 10).isf_momenta
    assert len(s.cfc_spec) == 6


def test_proc_from_config_and_sampling():
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    base = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                num_time_steps_block=8, max_num_walkers=12,
                target_num_walkers=10, rng_seed=5)
    proc = dmc_exec.Proc.from_config(
        dict(base, isf_spec=dict(num_modes=8, num_lags=4, lag_stride=2)))
    assert proc.isf_spec == dmc_exec.ISFEstSpec(8, 4, 2)
    assert proc.should_eval_isf
    cfg = proc.as_config()
    assert cfg['isf_spec'] == dict(num_modes=8, num_lags=4, lag_stride=2)
    assert dmc_exec.Proc.from_config(cfg) == proc
    by_kw = dmc_exec.Proc(proc.model_spec, 1e-3, num_blocks=6,
                          num_time_steps_block=8, max_num_walkers=12,
                          target_num_walkers=10, rng_seed=5,
                          isf_spec=dmc_exec.ISFEstSpec(8, 4, 2))
    assert by_kw == proc
    s = proc.sampling
    assert s.isf_est_spec == dmc.ISFEstSpec(8, 4, 2)
    assert s.pair_dist_est_spec is None and s.superfluid_est_spec is None
    short = dmc_exec.Proc.from_config(
        dict(base, isf_spec=dict(num_modes=8, num_lags=4)))
    assert short.sampling.isf_est_spec == dmc.ISFEstSpec(8, 4, 1)
    # without the spec nothing changes
    for absent in (base, dict(base, isf_spec=None)):
        plain = dmc_exec.Proc.from_config(absent)
        assert plain.isf_spec is None and not plain.should_eval_isf
        assert 'isf_spec' not in plain.as_config()
        assert plain.sampling.isf_est_spec is None
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
    rows = rng.rand(6, 5, 6)
    for on in (True, False):
        cfg = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                   num_time_steps_block=8, max_num_walkers=12,
                   target_num_walkers=10, rng_seed=5)
        if on:
            cfg['isf_spec'] = dict(num_modes=5, num_lags=4, lag_stride=2)
        proc = dmc_exec.Proc.from_config(cfg)
        data = dd.SamplingData(dd.PropsDataBlocks(
            dd.EnergyBlocks(rng.rand(6), w), dd.WeightBlocks(w),
            dd.NumWalkersBlocks(rng.randint(8, 12, 6).astype(np.uint64)),
            isf=dd.ISFBlocks(rows) if on else None))
        h = dmc_exec.HDF5FileHandler(str(tmp_path / f'r{int(on)}.h5'), 'run-A')
        h.dump(dmc_exec.ProcResult(state, proc, data))
        with h5lite.open_file(h.location, 'r') as f:
            q = f['run-A/dmc']
            extra = ['isf_spec'] if on else []
            assert sorted(q['proc_spec'].keys()) == extra + ['model_spec']
            extra = ['isf'] if on else []
            assert sorted(q['data/blocks'].keys()) == sorted(
                ['energy', 'num_walkers', 'weight'] + extra)
            if on:
                assert sorted(q['data/blocks/isf'].keys()) == ['totals']
        back = h.load()
        assert back.proc == proc
        b = back.data.blocks
        assert b.density is None and b.pair_dist is None
        assert b.cm_diffusion is None
        if on:
            assert isinstance(b.isf, dd.ISFBlocks)
            assert np.array_equal(b.isf.totals, rows)
            tau, f, err, conn = b.isf.scattering_function(
                back.proc.model_spec, back.proc.time_step,
                back.proc.isf_spec.lag_stride)
            assert tau.shape == (4,) and tau[1] == 2e-3
            assert f.shape == err.shape == conn.shape == (4, 5)
        else:
            assert b.isf is None


# ---- the C interface --------------------------------------------------------
def test_signature_table_lists_the_entry_points():
    import ctypes as C
    from phd_qmclib_amd import _lib
    sig = _lib.SIGNATURES
    assert sig['qmc_dmc_set_isf_estimator'] == \
        (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64])
    res, args = sig['qmc_dmc_read_isf']
    assert res is C.c_int and len(args) == 3
    assert args[:2] == [C.c_void_p, C.c_int64]
    assert args[2] == sig['qmc_dmc_read_pair_dist'][1][2]
