"""The reference-shaped Python surface (Spec / Sampling / Proc) on the GPU:
the assertions the reference's own tests make (tests/mrbp_qmc/test_vmc.py:
62-125, test_dmc.py:56-71, test_model.py:60-91), the split-step multi-GPU path
at world size 1, and the 2-sigma statistical gate against block statistics the
reference produced with its own RNG (tests/golden/stats.npz)."""
from itertools import islice
from math import pi

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu


def test_core_funcs_surface():
    """tests/mrbp_qmc/test_model.py:60-91: drift keeps positions and fills the
    drift slot; ith_energy == ith_energy_and_drift[0]; energy == sum."""
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    cf, cfc = mrbp_qmc.core_funcs, spec.cfc_spec
    np.random.seed(3)
    sc = spec.init_get_sys_conf()
    out = cf.drift(sc, *cfc)
    assert np.array_equal(out[0], sc[0]) and np.all(out[1] != 0)
    e = cf.energy(sc, *cfc)
    parts = [cf.ith_energy_and_drift(i, sc, *cfc) for i in range(16)]
    assert np.isclose(sum(p[0] for p in parts), e, rtol=1e-12)
    assert parts[3][0] == cf.ith_energy(3, sc, *cfc)
    assert np.allclose([p[1] for p in parts], out[1], rtol=1e-13)
    assert np.isfinite(cf.wf_abs_log(sc, *cfc))


def test_vmc_generators_agree():
    """Same seed => `states`, `blocks` and `as_chain` walk the same chain
    (tests/mrbp_qmc/test_vmc.py:62-83, 95-125)."""
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16, lattice_depth=100, interaction_strength=1)
    smp = mrbp_qmc.vmc.Sampling(spec, 0.25 * spec.well_width, rng_seed=1)
    np.random.seed(1)
    ini = smp.build_state(spec.init_get_sys_conf())
    ns = 96
    chain = smp.as_chain(ns, ini)
    assert chain.confs.shape == (ns, 2, 16)
    acc_states = sum(s.move_stat for s in islice(smp.states(ini), ns)) / ns
    assert acc_states == chain.accept_rate
    b1, b2 = list(islice(smp.blocks(ns // 2, ini), 2))
    assert (b1.accept_rate + b2.accept_rate) / 2 == chain.accept_rate
    assert np.array_equal(np.r_[b1.iter_props.wf_abs_log,
                                b2.iter_props.wf_abs_log],
                          chain.props.wf_abs_log)
    assert np.array_equal(b2.last_state.sys_conf[0], chain.confs[-1, 0])
    # first yield is the initial state, flagged accepted
    assert chain.props.move_stat[0] and np.array_equal(chain.confs[0, 0],
                                                       ini.sys_conf[0])
    # (evaluated in lane = position order: summation order differs)
    assert chain.props.wf_abs_log[0] == pytest.approx(ini.wf_abs_log, rel=1e-13, abs=1e-13)
    with pytest.raises(mrbp_qmc.vmc.StateError):
        smp.build_state(np.zeros((2, 15)))
    with pytest.raises(ValueError):
        smp.as_chain(0, ini)


def test_vmc_ssf_blocks():
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    smp = mrbp_qmc.vmc.Sampling(spec, 0.125, rng_seed=2,
                                ssf_est_spec=mrbp_qmc.vmc.SSFEstSpec(16))
    np.random.seed(2)
    blk = next(smp.blocks(32, smp.build_state(spec.init_get_sys_conf())))
    assert blk.iter_ssf.shape == (32, 16, 3)
    assert np.allclose(blk.iter_ssf[:, 0, 0], 16.0 ** 2)   # k = 0 mode
    rej = ~blk.iter_props.move_stat
    assert np.array_equal(blk.iter_ssf[1:][rej[1:]], blk.iter_ssf[:-1][rej[1:]])


def test_dmc_build_state_and_blocks():
    """tests/mrbp_qmc/test_dmc.py:56-71 + a VMC -> DMC pipeline like :74-125."""
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16, lattice_depth=0, interaction_strength=4, num_defects=4,
               defect_magnitude=0)
    vs = mrbp_qmc.vmc.Sampling(spec, 0.125, rng_seed=1)
    np.random.seed(5)
    chain = vs.as_chain(300, vs.build_state(spec.init_get_sys_conf()))
    ds = mrbp_qmc.dmc.Sampling(spec, 1e-3, max_num_walkers=512,
                               target_num_walkers=480, rng_seed=3)
    ini_set = chain.confs[-128:]
    st = ds.build_state(ini_set)
    assert st.num_walkers == 128 and st.max_num_walkers == 512
    assert np.allclose(st.confs[:128, 0], ini_set[:, 0])
    assert np.all(st.props.weight[:128] == 1) and not st.props.mask[:128].any()
    assert st.props.mask[128:].all()
    assert np.isclose(st.ref_energy, st.props.energy[:128].mean())
    blocks = list(islice(ds.blocks(st, 16, 1), 3))
    for b in blocks:
        p = b.iter_props
        assert p.energy.shape == (16,) and p.num_walkers.dtype == np.uint64
        assert np.array_equal(p.weight, p.num_walkers.astype(float))
        assert np.all(p.num_walkers <= 512)
    # population is pulled towards the target by the E_ref feedback
    assert blocks[-1].iter_props.num_walkers[-1] > 128
    last = blocks[-1].last_state
    assert last.num_walkers == int(blocks[-1].iter_props.num_walkers[-1])
    # a generator restarted from a yielded state continues from it
    again = next(ds.blocks(last, 4, 0))
    assert again.iter_props.num_walkers[0] > 0
    states = list(islice(ds.states(st), 3))
    assert states[0].confs.shape == (512, 2, 16)
    with pytest.raises(mrbp_qmc.dmc.StateError):
        ds.build_state(np.zeros((10, 2, 15)))


def test_dmc_split_step_equals_block():
    """step_local + (identity all-reduce) + step_finish == run_block."""
    import torch
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    from phd_qmclib_amd.dist import DistributedDmc
    spec = box(16)
    eng = ModelEngine(spec.cfc_spec,
                      stream=torch.cuda.current_stream().cuda_stream)
    pos = 16 * np.random.RandomState(4).random_sample((300, 16))
    a = DmcEnsemble(eng, 1e-3, 512, 300, 0.5, rng_seed=8)
    b = DmcEnsemble(eng, 1e-3, 512, 300, 0.5, rng_seed=8, external_reduce=True)
    a.set_state(pos)
    b.set_state(pos)
    sa = a.run_block(10)
    dd = DistributedDmc(b, 16, 'cuda')
    sb = dd.run_block(10)
    assert np.array_equal(sa.num_walkers, sb.num_walkers)
    assert np.array_equal(sa.energy, sb.energy)
    assert np.array_equal(sa.ref_energy, sb.ref_energy)
    # export / truncate / import round trip keeps the walkers
    nw = b.num_walkers()
    st0 = b.get_state()
    buf = torch.zeros(20 * (3 * 16 + 2), dtype=torch.float64, device='cuda')
    b.export_walkers(nw - 20, 20, buf.data_ptr())
    b.truncate(nw - 20)
    assert b.num_walkers() == nw - 20
    b.import_walkers(20, buf.data_ptr())
    assert b.num_walkers() == nw
    with pytest.raises(Exception):
        b.run_block(1)        # external_reduce handles refuse run_block
    for h in (a, b):
        h.close()
    eng.close()


def _two_sigma(a_mean, a_err, b_mean, b_err):
    return abs(a_mean - b_mean) <= 2.0 * np.hypot(a_err, b_err)


def test_vmc_statistics_vs_reference(golden_stats):
    """Block-averaged energy, second moment and acceptance of the device
    chains against the reference's own runs (N=16 box, 4 seeds x 14 kept
    blocks of 512 steps; reference RNG = numpy MT19937, ours = Philox)."""
    from phd_qmclib_amd import mrbp_qmc
    g = golden_stats['vmc/block_stats']            # [seed, block, (E, E2, acc)]
    ns, nb, burn, spread = golden_stats['vmc/cfg']
    ns, nb, burn = int(ns), int(nb), int(burn)
    spec = box(16)
    W = 256
    ens = mrbp_qmc.vmc.EnsembleSampling(spec, float(spread), W, rng_seed=77)
    ens.init_random(seed=5)
    blocks = list(islice(ens.blocks(ns), nb))[burn:]
    ens.close()
    e = np.array([b.energy for b in blocks])             # [block, chain]
    e2 = np.array([b.sum_energy2 / b.num_steps for b in blocks])
    acc = np.array([b.accept_rate for b in blocks])
    # chains are independent: error of the mean from the chain-to-chain spread
    def stat(x):
        per_chain = x.mean(axis=0)
        return per_chain.mean(), per_chain.std(ddof=1) / np.sqrt(W)
    ref = g.mean(axis=1)                                 # per seed
    for col, ours in ((0, stat(e)), (1, stat(e2)), (2, stat(acc))):
        r_mean = ref[:, col].mean()
        r_err = ref[:, col].std(ddof=1) / np.sqrt(ref.shape[0])
        assert _two_sigma(ours[0], ours[1], r_mean, r_err), \
            (col, ours, r_mean, r_err)


def test_dmc_statistics_vs_reference(golden_stats):
    """DMC mixed-estimator energy E/N of the device run against the
    reference's runs (N=16 box, 3 seeds): within 2 sigma of the combined
    error."""
    from phd_qmclib_amd import mrbp_qmc
    g = golden_stats['dmc/block_totals']           # [seed, block, (E, W, nw)]
    dt, target, maxw, kappa, nts, nbd, burnd = golden_stats['dmc/cfg']
    target, maxw, nts, nbd, burnd = map(int, (target, maxw, nts, nbd, burnd))
    spec = box(16)
    ref = np.array([s[burnd:, 0].sum() / s[burnd:, 1].sum() for s in g]) / 16
    r_mean, r_err = ref.mean(), ref.std(ddof=1) / np.sqrt(len(ref))
    ours = []
    for seed in range(6):
        vs = mrbp_qmc.vmc.EnsembleSampling(spec, 0.125, target, rng_seed=seed)
        vs.init_random(seed=10 + seed)
        next(islice(vs.blocks(600), 1))
        confs = np.zeros((target, 2, 16))
        confs[:, 0] = vs.confs()
        vs.close()
        ds = mrbp_qmc.dmc.Sampling(spec, dt, maxw, target, kappa,
                                   rng_seed=seed)
        blocks = list(islice(ds.blocks(ds.build_state(confs), nts, burnd),
                             nbd))[burnd:]
        E = sum(b.iter_props.energy.sum() for b in blocks)
        Wt = sum(b.iter_props.weight.sum() for b in blocks)
        ours.append(E / Wt / 16)
    ours = np.array(ours)
    o_mean, o_err = ours.mean(), ours.std(ddof=1) / np.sqrt(len(ours))
    assert _two_sigma(o_mean, o_err, r_mean, r_err), (o_mean, o_err, r_mean,
                                                      r_err)


def test_proc_exec_end_to_end():
    """Proc.exec drivers: burn-in, block reductions, reblocked results
    (qmc_exec/vmc/proc.py:87-250, qmc_exec/dmc/proc.py:136-415)."""
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    np.random.seed(11)
    vp = mrbp_qmc.vmc_exec.Proc(spec, 0.125, rng_seed=4, num_blocks=16,
                                num_steps_block=64)
    vin = mrbp_qmc.vmc_exec.ProcInput.from_model_sys_conf_spec(
        mrbp_qmc.vmc_exec.ModelSysConfSpec('RANDOM'), vp)
    vres = vp.exec(vin)
    eb = vres.data.blocks.energy
    assert len(eb) == 16 and 12 < eb.mean / 16 < 20 and eb.mean_error > 0
    assert vres.state.sys_conf.shape == (2, 16)
    with pytest.raises(mrbp_qmc.vmc_exec.ProcInputError):
        vp.exec(object())
    dp = mrbp_qmc.dmc_exec.Proc(spec, 1e-3, max_num_walkers=128,
                                target_num_walkers=96, rng_seed=4,
                                num_blocks=16, num_time_steps_block=16)
    din = mrbp_qmc.dmc_exec.ProcInput.from_model_sys_conf_spec(
        mrbp_qmc.dmc_exec.ModelSysConfSpec('RANDOM'), dp)
    dres = dp.exec(din)
    blocks = dres.data.blocks
    assert len(blocks.energy) == 16
    assert 12 < blocks.energy.mean / 16 < 20 and blocks.energy.mean_error > 0
    assert np.array_equal(blocks.weight.totals, blocks.num_walkers.totals)
    # chaining: the result of one run is the input of the next
    d2 = dp.exec(mrbp_qmc.dmc_exec.ProcInput.from_result(dres, dp))
    assert d2.state.num_walkers > 0
    keep = mrbp_qmc.dmc_exec.Proc(spec, 1e-3, max_num_walkers=128,
                                  target_num_walkers=96, rng_seed=4,
                                  num_blocks=4, num_time_steps_block=8,
                                  keep_iter_data=True)
    kres = keep.exec(din)
    assert kres.data.series.iter_props_blocks.energy.shape == (4, 8)
    assert kres.data.series.props.energy.shape == (32,)


def test_dmc_estimators_through_sampling_and_proc():
    """S(k) / density through `dmc.Sampling.blocks` and `dmc_exec.Proc.exec`
    (qmc_exec/dmc/proc.py:203-250, 322-368): shapes, burn-in gating, the
    k = 0 mode (|rho_0|^2 = N^2 per walker), density normalisation."""
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    rng = np.random.RandomState(8)
    confs = np.zeros((96, 2, 16))
    confs[:, 0] = 16 * rng.random_sample((96, 16))
    ds = mrbp_qmc.dmc.Sampling(
        spec, 1e-3, 128, 96, 0.5, rng_seed=2,
        density_est_spec=mrbp_qmc.dmc.DensityEstSpec(32, False),
        ssf_est_spec=mrbp_qmc.dmc.SSFEstSpec(16, False))
    blocks = list(islice(ds.blocks(ds.build_state(confs), 8, 1), 3))
    assert blocks[0].iter_ssf.shape == (8, 16, 3)
    assert blocks[0].iter_density.shape == (8, 32, 1)
    assert not blocks[0].iter_ssf.any() and not blocks[0].iter_density.any()
    for b in blocks[1:]:
        nw = b.iter_props.num_walkers.astype(float)
        assert np.allclose(b.iter_ssf[:, 0, 0], 256.0 * nw)     # k = 0
        assert np.allclose(b.iter_ssf[:, 0, 1], 16.0 * nw)
        assert np.allclose(b.iter_ssf[:, 0, 2], 0.0)
    # mixed density of the first kept step counts every particle once
    assert blocks[1].iter_density[0].sum() == \
        16 * blocks[1].iter_props.num_walkers[0]
    proc = mrbp_qmc.dmc_exec.Proc(
        spec, 1e-3, max_num_walkers=128, target_num_walkers=96, rng_seed=3,
        num_blocks=8, num_time_steps_block=8, burn_in_blocks=1,
        density_spec=mrbp_qmc.dmc_exec.DensityEstSpec(32, True),
        ssf_spec=mrbp_qmc.dmc_exec.SSFEstSpec(16, True))
    res = proc.exec(mrbp_qmc.dmc_exec.ProcInput(ds.build_state(confs)))
    sk = res.data.blocks.ss_factor
    assert sk.mean.shape == (16,)
    # (k = 0: Im rho_0 is identically zero, its relative error is 0/0 in the
    # reference's formula too)
    assert np.all(np.isfinite(sk.mean_error[1:]))
    assert abs(sk.mean[0]) < 1e-6          # S(0) = N^2 - N^2 - 0 per walker
    assert np.all(sk.mean[1:] > 0) and np.all(sk.mean[1:] < 16 * 1.5)
    dn = res.data.blocks.density
    assert dn.mean.shape == (32,)
    # the reference transports the pure density by slot index (not along the
    # lineage), so slots that joined late dilute the normalisation slightly
    assert 14.0 < dn.mean.sum() <= 16.0 + 1e-9


def test_vmc_to_dmc_handoff_on_device(oracle):
    """VMC chains seed the DMC population without a host round trip
    (the pipeline of tests/mrbp_qmc/test_dmc.py:76-83); the population that
    results is the oracle's built from the same configurations."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    spec = box(16)
    eng = ModelEngine(spec.cfc_spec)
    rng = np.random.RandomState(4)
    v = VmcEnsemble(eng, 500, 0.125, rng_seed=6)
    v.set_state(16 * rng.random_sample((500, 16)))
    v.run_block(40, sums=False)
    pos = v.get_state()[0]
    a = DmcEnsemble(eng, 1e-3, 512, 480, 0.5, rng_seed=6)
    a.set_state_from_vmc(v, 480)
    b = DmcEnsemble(eng, 1e-3, 512, 480, 0.5, rng_seed=6)
    b.set_state(pos[:480])
    sa, sb = a.get_state(), b.get_state()
    # same configurations; the two populations differ in lane order only (a
    # keeps the VMC's nearly-sorted lanes, b sorts afresh), i.e. in summation order
    assert np.array_equal(sa.confs[:, 0], sb.confs[:, 0])
    assert np.allclose(sa.confs[:, 1], sb.confs[:, 1], rtol=1e-11, atol=1e-11)
    assert sa.ref_energy == pytest.approx(sb.ref_energy, rel=1e-13)
    ser_a, ser_b = a.run_block(5), b.run_block(5)
    assert np.allclose(ser_a.energy, ser_b.energy, rtol=1e-10)
    # ... and against the CPU oracle on the same Philox streams
    orc = oracle.DmcEnsemble(oracle.model_from_cfc(spec.cfc_spec), pos[:480],
                             1e-3, 512, 480, 0.5, seed=6)
    assert sa.ref_energy == pytest.approx(orc.st.ref_energy, rel=1e-10)
    for t in range(5):
        o = orc.step()
        assert int(ser_a.num_walkers[t]) == o.num_walkers, t
        assert ser_a.energy[t] == pytest.approx(o.energy, rel=1e-9), t
        assert ser_a.ref_energy[t] == pytest.approx(o.ref_energy, rel=1e-9), t
    for h in (a, b, v):
        h.close()
    eng.close()


def test_vmc_ndf_gaussian_proposal(oracle, golden_params):
    """mrbp_qmc/vmc_ndf.py:23-51: Gaussian proposal with sigma = sqrt(dt);
    device chain vs the oracle's Gaussian chain on the same Philox stream."""
    from phd_qmclib_amd import mrbp_qmc
    from .conftest import oracle_model
    spec = box(16)
    smp = mrbp_qmc.vmc.NDFSampling(spec, time_step=4e-3, rng_seed=21)
    assert abs(smp._proposal_width() - np.sqrt(4e-3)) < 1e-16
    np.random.seed(9)
    ini = smp.build_state(spec.init_get_sys_conf())
    blk = next(smp.blocks(40, ini))
    m = oracle_model(oracle, golden_params, 'box16')
    ch = oracle.VmcChain(m, ini.sys_conf[0], np.sqrt(4e-3), seed=21, chain=0,
                         gaussian=True)
    wf, en, st, acc = ch.run(40)
    assert np.array_equal(st, blk.iter_props.move_stat)
    assert np.allclose(en, blk.iter_props.energy, rtol=1e-9)
    assert np.allclose(wf, blk.iter_props.wf_abs_log, rtol=1e-9)
    assert 0.2 < blk.accept_rate <= 1.0


@pytest.mark.parametrize('n,modes', [(16, 8), (64, 64), (64, 130)])
def test_vmc_ensemble_ssf_on_device(n, modes):
    """f2: S(k) parts of a whole VMC ensemble in one launch (matrix-core
    kernel) against numpy on the ensemble's configurations."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n)
    eng = ModelEngine(spec.cfc_spec)
    W = 700
    v = VmcEnsemble(eng, W, 0.125, rng_seed=9)
    v.set_state(n * np.random.RandomState(n).random_sample((W, n)))
    v.run_block(20, sums=False)
    got = v.ssf_parts(modes)
    z = v.get_state()[0]
    k = 2 * pi * np.arange(modes) / n
    ph = np.exp(1j * k[None, :, None] * z[:, None, :]).sum(axis=2)
    ref = np.stack([(np.abs(ph) ** 2).mean(0), ph.real.mean(0),
                    ph.imag.mean(0)], axis=1)
    assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max()
    # S(k = 0) parts: N^2, N, 0
    assert got[0, 0] == pytest.approx(n * n) and got[0, 1] == pytest.approx(n)
    v.close(); eng.close()


def test_lieb_liniger_known_answer():
    """Independent physics check: without the lattice the model
    is the Lieb-Liniger gas, gamma = (L/N)^2 g / 2; for gamma = 2 the exact
    ground-state energy per particle is e(gamma) n^2 = 1.0504 n^2 in units
    hbar^2 / 2m (Lieb & Liniger 1963).  N = 32, n = 1, 4096 walkers, started
    from equilibrated VMC configurations (the variational energy is 1.0586):
    DMC with the parent's energy in the branching weight gives 1.048 +- 0.001
    (the finite ring sits slightly below the thermodynamic limit); with the
    reference's stale-slot-energy quirk D1 (the default, reproduced for
    parity) the estimate stays ~0.8 % higher."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    n = 32
    spec = box(n, lattice_depth=0.0, interaction_strength=4.0,
               tbf_contact_cutoff=0.25 * n)
    eng = ModelEngine(spec.cfc_spec)
    W = 4096
    v = VmcEnsemble(eng, W, 0.4, rng_seed=3)
    v.set_state(n * np.random.RandomState(2).random_sample((W, n)))
    v.run_block(800, sums=False)
    out = v.run_block(200)
    e_vmc = out['sum_energy'].sum() / (200 * W) / n
    assert 1.0504 < e_vmc < 1.075, e_vmc          # variational bound
    res = {}
    for fix in (True, False):
        d = DmcEnsemble(eng, 1e-3, 4608, W, 0.5, rng_seed=4,
                        fix_stale_energy=fix)
        d.set_state_from_vmc(v, W)
        d.run_block(1500, read=False)            # equilibrate
        ser = d.run_block(1500)
        res[fix] = ser.energy.sum() / ser.weight.sum() / n
        assert np.all(ser.num_walkers < 4608)
        d.close()
    assert abs(res[True] - 1.0504) < 0.008, res
    assert res[True] < e_vmc
    assert abs(res[False] - 1.0504) < 0.015, res
    v.close(); eng.close()


def test_ensemble_sampling_ssf():
    """EnsembleSampling.ssf: S(k) of the box from 2048 equilibrated chains is
    0 at k = 0, positive elsewhere and tends to 1 at large k."""
    from phd_qmclib_amd import mrbp_qmc
    spec = box(16)
    smp = mrbp_qmc.vmc.EnsembleSampling(spec, 0.125, 2048, rng_seed=5)
    smp.init_random(seed=1)
    next(smp.blocks(400))
    k, ssf = smp.ssf(48)
    assert k[1] == pytest.approx(2 * pi / 16)
    assert abs(ssf[0]) < 1e-9
    assert np.all(ssf[1:] > 0) and np.all(ssf[1:] < 3)
    # far beyond the lattice's Bragg peak (k = 2 pi) the gas looks uncorrelated
    assert abs(ssf[40:].mean() - 1.0) < 0.15
    smp.close()


def _z(a, b):
    """(mean a - mean b) in units of the combined standard error; a, b are
    independent samples (chains / runs)."""
    return (a.mean() - b.mean()) / np.sqrt(a.var(ddof=1) / len(a) +
                                           b.var(ddof=1) / len(b))


def test_vmc_n64_statistics_vs_oracle(oracle):
    """The north-star gate at the benchmarked size (N = 64, where the reference
    itself is too slow to sample): block-averaged energy, VARIANCE of the
    local energy and acceptance of the device ensemble against the pinned CPU
    oracle, independent chains, SIX seeds on each side.

    Gate (BASELINE.json north_star, SURVEY 8d "parity gate"): each quantity
    pooled over the seeds within 2 sigma of the combined Monte Carlo error,
    and every single seed-against-seed comparison within 3 sigma.  Nominal
    false-alarm probability: 4.6 % per pooled quantity (three quantities),
    0.27 % per single comparison; the seeds are fixed and both generators are
    counter-based, so a given build always reproduces the same z values --
    they are printed for the record (round 4, Philox2x32 move stream:
    z = -0.34, -1.20, -0.10 for E, var, acceptance; largest single 2.39).

    Why six seeds (round 4).  Rounds 2-3 pooled three.  With the new move
    stream the three-seed z of var(E_L) came out at -2.02 (E: -0.77,
    acceptance: +0.07): a 4 % event on one of three quantities, or a bias?  It
    cannot be a bias of the sampled law -- on equal seeds the device follows
    the oracle's chains decision for decision (tests/test_gpu_scale.py) -- and
    the data say chance: ten seeds on each side (the oracle's offline) give
    z = +0.84, -0.98, -0.51, the pooled z as a function of the number of seeds
    is -2.02, -2.03, -2.22, -1.20, ... -0.63, ... -0.98 (3, 4, 5, 6, 8, 10:
    oracle seeds 5 and 6 happen to be as low as 0-2 are high), and a bootstrap
    of samples of the two sizes from the device's 81 920 per-chain values of
    var(E_L) -- a heavy-tailed quantity: median 0.148, 99.9th percentile 0.87
    -- has P(|z| > 2) = 5.0 %: the statistic behaves as advertised.  A
    borderline gate is settled with more data, not with other seeds: six
    seeds (about 30 s of host time for the oracle side) is what fits the
    suite.

    Burn-in (round 4): from uniform random starts E/N of this box is still
    relaxing after thousands of steps (oracle, 512 chains: 15.75 over steps
    300-550, 15.69, 15.67, 15.65, 15.63 over the following windows of 250) --
    the long-wavelength modes move diffusively under moves of 0.06 lattice
    periods.  Both sides walk through the same transient, so the comparison is
    fair at any time, but with the 300 burn-in steps of rounds 2-3 the sample
    means still carried the memory of the 1536 initial configurations of the
    oracle side, the same in every build: z(E) was -1.6 with the Philox4x32
    move stream and -2.1 with the Philox2x32 one (round 4), i.e. correlated
    draws.  1200 steps of burn-in let most of that memory decay (the oracle
    side costs ~20 s of host time)."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(64)
    m = oracle.model_from_cfc(spec.cfc_spec)
    burn, ns = 1200, 500
    Wo, Wg = 512, 8192
    eng = ModelEngine(spec.cfc_spec)
    dev, orc = [], []
    for k in range(6):
        pos = 64 * np.random.RandomState(80 + k).random_sample((Wo, 64))
        wf = np.array([oracle.wf_abs_log(m, p) for p in pos])
        ec = np.zeros(Wo)
        oracle.vmc_ensemble(m, pos, wf, ec, 0.125, 770 + k, burn,
                            yield_initial=True)
        se, se2, na = oracle.vmc_ensemble(m, pos, wf, ec, 0.125, 770 + k, ns,
                                          step0=burn)
        orc.append(dict(e=se / ns / 64, acc=na / ns,
                        var=(se2 / ns - (se / ns) ** 2) / 64 ** 2))
        v = VmcEnsemble(eng, Wg, 0.125, rng_seed=1234 + k)
        v.set_state(64 * np.random.RandomState(90 + k)
                    .random_sample((Wg, 64)))
        v.run_block(burn, sums=False)
        out = v.run_block(ns)
        dev.append(dict(
            e=out['sum_energy'] / ns / 64, acc=out['num_accepted'] / ns,
            var=(out['sum_energy2'] / ns - (out['sum_energy'] / ns) ** 2)
            / 64 ** 2))
        v.close()
    eng.close()
    report = {}
    for q in ('e', 'var', 'acc'):
        pooled = _z(np.concatenate([d[q] for d in dev]),
                    np.concatenate([o[q] for o in orc]))
        single = [_z(d[q], o[q]) for d in dev for o in orc]
        report[q] = (float(pooled), [round(float(x), 2) for x in single])
    print('N=64 VMC z values (pooled, singles):', report)
    for q in ('e', 'var', 'acc'):
        d = np.concatenate([x[q] for x in dev])
        o = np.concatenate([x[q] for x in orc])
        print(f'  {q}: device {d.mean():.6f} +- {d.std(ddof=1) / len(d) ** 0.5:.6f}'
              f'  oracle {o.mean():.6f} +- {o.std(ddof=1) / len(o) ** 0.5:.6f}'
              f'  per oracle seed', [round(float(x[q].mean()), 6) for x in orc])
    for q, (pooled, single) in report.items():
        assert abs(pooled) < 2.0, (q, report)
        assert max(abs(x) for x in single) < 3.0, (q, report)
    # and the numbers are the physical ones (VMC energy of the trial state)
    assert 15.5 < np.concatenate([d['e'] for d in dev]).mean() < 15.95


def test_dmc_n64_statistics_vs_oracle(oracle):
    """Same gate for DMC at N = 64: independent ensembles of 128 walkers (same
    population, hence the same population-control bias) on the device (96
    seeds) and in the oracle (24 seeds), POOLED with the 16 + 8 seeds of the
    first version of this test (see below): 112 against 32 runs; time-averaged
    E/N and mean population within the 2-sigma-equivalent of Welch's t (the
    run-to-run spread is estimated from the runs themselves, so the critical
    value is Student's: same 4.6 % nominal false-alarm probability per
    quantity).

    Before that, the stronger statement the counter-based generator allows:
    on EQUAL seeds the device follows the oracle's trajectory, so both
    quantities agree to rounding run by run -- the two sides are the same
    process in law, and the independent-seed gate measures nothing but
    Monte-Carlo noise.  (For the record: the first choice of 16 + 8 seeds
    -- device 100..115, oracle 200..207 -- gave t = 2.8 for the mean
    population on its own, a 1 % event.  Round 2 replaced those seeds; a
    failing sample is not discarded, so they are pooled with the 96 + 24
    here and the t values of the pooled sample and of both parts are printed.)"""
    from scipy import stats
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    spec = box(64)
    m = oracle.model_from_cfc(spec.cfc_spec)
    eng = ModelEngine(spec.cfc_spec)
    dt, target, maxw, eq, ns = 1e-3, 128, 160, 200, 300
    start = 64 * np.random.RandomState(3).random_sample((target, 64))

    def dev_run(seed):
        d = DmcEnsemble(eng, dt, maxw, target, 0.5, rng_seed=seed)
        d.set_state(start)
        d.run_block(eq, read=False)
        s = d.run_block(ns)
        d.close()
        return s.energy.sum() / s.weight.sum() / 64, s.num_walkers.mean()

    def orc_run(seed):
        o = oracle.DmcEnsemble(m, start, dt, maxw, target, 0.5, seed=seed,
                               nthreads=oracle.max_threads())
        for _ in range(eq):
            o.step()
        e = w = nw = 0.0
        for _ in range(ns):
            y = o.step()
            e += y.energy; w += y.weight; nw += y.num_walkers
        return e / w / 64, nw / ns

    orc = np.array([orc_run(3000 + k) for k in range(24)] +
                   [orc_run(200 + k) for k in range(8)])
    # equal seeds: the same trajectories (500 steps of branching decisions)
    same = np.array([dev_run(3000 + k) for k in range(3)])
    assert np.array_equal(same[:, 1], orc[:3, 1])
    assert np.allclose(same[:, 0], orc[:3, 0], rtol=1e-9, atol=0)
    dev = np.array([dev_run(1000 + k) for k in range(96)] +
                   [dev_run(100 + k) for k in range(16)])

    def welch(a, b):
        va, vb = a.var(ddof=1) / len(a), b.var(ddof=1) / len(b)
        t = (a.mean() - b.mean()) / np.sqrt(va + vb)
        dof = (va + vb) ** 2 / (va ** 2 / (len(a) - 1) + vb ** 2 / (len(b) - 1))
        crit = stats.t.ppf(1 - 0.0455 / 2, dof)      # "2 sigma" for Student's t
        return float(t), float(crit)

    report = {}
    for col, name in ((0, 'E/N'), (1, '<nw>')):
        a, b = dev[:, col], orc[:, col]
        t, crit = welch(a, b)
        report[name] = dict(
            pooled=(t, crit, float(a.mean()), float(b.mean())),
            seeds_96_24=welch(a[:96], b[:24]),
            seeds_16_8_round1=welch(a[96:], b[24:]))
    print('N=64 DMC t values (t, 2-sigma critical value[, dev, oracle]):',
          report)
    for name, r in report.items():
        t, crit = r['pooled'][:2]
        assert abs(t) < crit, (name, report)
    assert 14.5 < dev[:, 0].mean() < 16.5
    eng.close()


@pytest.mark.parametrize('n', [100, 128])
def test_dmc_large_n_equal_seed_trajectories(oracle, n):
    """BASELINE configs[3] is DMC at N = 128 (two particles per lane: the
    sorted-row pair sum of csrc/qmc_sorted128.h with its cotangent / tangent
    tables, no cached second normal).  On EQUAL seeds the device must follow the
    oracle's ensemble through branching for many steps: population identical
    step by step, E_t and E_ref to rounding (qmc_base/dmc.py:739-785,
    jastrow/dmc.py:758-825); N = 100 is the padded ring of 50 lanes."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    spec = box(n)
    m = oracle.model_from_cfc(spec.cfc_spec)
    eng = ModelEngine(spec.cfc_spec)
    dt, target, maxw, steps = 1e-3, 96, 128, 120
    # spread like equilibrated walkers (the sorted-row path takes them all)
    rng = np.random.RandomState(1280 + n)
    start = (np.arange(n) + 0.5 + 0.5 * (rng.random_sample((target, n)) - 0.5))
    eng.general_path_walkers(reset=True)
    for seed in (41, 42):
        d = DmcEnsemble(eng, dt, maxw, target, 0.5, rng_seed=seed)
        d.set_state(start)
        ser = d.run_block(steps)
        d.close()
        o = oracle.DmcEnsemble(m, start, dt, maxw, target, 0.5, seed=seed,
                               nthreads=oracle.max_threads())
        for t in range(steps):
            y = o.step()
            assert int(ser.num_walkers[t]) == y.num_walkers, (seed, t)
            assert ser.energy[t] == pytest.approx(y.energy, rel=1e-9), (seed, t)
            assert ser.ref_energy[t] == pytest.approx(y.ref_energy, rel=1e-9)
    assert eng.general_path_walkers() == 0
    eng.close()
