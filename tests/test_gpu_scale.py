"""Size-independent properties at (or near) the BASELINE.json sizes, where the
CPU oracle is too slow to be the checker: determinism, independence of a
chain's trajectory from the ensemble size (counter RNG keyed by chain), exact
bookkeeping identities of the DMC step, and the symmetries of the model
(particle permutation, translation by a lattice period)."""

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng64():
    from phd_qmclib_amd.engine import ModelEngine
    e = ModelEngine(box(64).cfc_spec)
    yield e
    e.close()


@pytest.mark.parametrize('log2w', [16, 20])      # 20: BASELINE configs[1]
def test_vmc_chains_do_not_depend_on_ensemble_size(eng64, log2w):
    """Chain c follows the same trajectory in an ensemble of 2^16 (2^20: the
    benchmarked size) chains and in one of 300 (Philox stream = chain index),
    and a rerun is bit-identical."""
    from phd_qmclib_amd.engine import VmcEnsemble
    rng = np.random.RandomState(1)
    W = 1 << log2w
    pos = 64 * rng.random_sample((W, 64))
    big = VmcEnsemble(eng64, W, 0.125, rng_seed=5)
    big.set_state(pos)
    a = big.run_block(12)
    a2 = big.run_block(12)
    small = VmcEnsemble(eng64, 300, 0.125, rng_seed=5)
    small.set_state(pos[:300])
    b = small.run_block(12)
    b2 = small.run_block(12)
    for k in ('sum_energy', 'sum_energy2', 'num_accepted'):
        assert np.array_equal(a[k][:300], b[k]) and \
            np.array_equal(a2[k][:300], b2[k])
    again = VmcEnsemble(eng64, W, 0.125, rng_seed=5)
    again.set_state(pos)
    c = again.run_block(12)
    assert np.array_equal(a['sum_energy'], c['sum_energy'])
    # a rank shard with a chain offset reproduces the tail of the ensemble
    shard = VmcEnsemble(eng64, 256, 0.125, rng_seed=5, chain0=W - 256)
    shard.set_state(pos[-256:])
    d = shard.run_block(12)
    assert np.array_equal(d['sum_energy'], a['sum_energy'][-256:])
    # sanity of the physics at scale: E/N of the box and the acceptance
    e_per = (a2['sum_energy'].sum() / (12 * W)) / 64
    assert 12 < e_per < 25
    acc = a2['num_accepted'].sum() / (12 * W)
    assert 0.3 < acc < 0.8
    for h in (big, small, again, shard):
        h.close()


@pytest.mark.parametrize('n', [16, 64, 128])
def test_vmc_benchmarked_kernel_vs_series_kernel_and_oracle(oracle, n):
    """Trajectory-level pin of the instantiation bench.py times (VERDICT r2,
    missing 2): a block WITHOUT series runs the production kernel
    (`vmc_step_kernel<..., LEAN = true>`: Philox proposal, per-chain block sums
    only); every tape / series comparison of the suite runs the other
    instantiation.  Same ensemble, same seed:
      * both kernels: identical sum_energy, sum_energy2, num_accepted and final
        configurations, bit for bit;
      * the production kernel against `oracle.vmc_ensemble` on the same Philox
        stream (qmc_base/vmc.py:624-646, jastrow/vmc.py:253-262): per-chain
        block sums to rounding, except for the rare chain where a proposal
        falls within rounding of the Metropolis threshold and the two sides
        decide differently (that chain then follows another trajectory);
      * the device's counter of walkers that left the sorted-row pair sums
        (N = 64, 128) stays 0: the sums compared here came from them."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    from ._traj import explain_flips, first_difference
    spec = box(n)
    spread = 0.25 * spec.well_width
    W, steps = 192, 40
    pos = n * np.random.RandomState(300 + n).random_sample((W, n))
    eng = ModelEngine(spec.cfc_spec)
    eng.general_path_walkers(reset=True)
    lean = VmcEnsemble(eng, W, spread, rng_seed=11)
    lean.set_state(pos)
    a1 = lean.run_block(steps)                   # no series: the LEAN kernel
    a2 = lean.run_block(steps)
    full = VmcEnsemble(eng, W, spread, rng_seed=11)
    full.set_state(pos)
    b1 = full.run_block(steps, series=True)
    b2 = full.run_block(steps, series=True)
    for a, b in ((a1, b1), (a2, b2)):
        for k in ('sum_energy', 'sum_energy2', 'num_accepted'):
            assert np.array_equal(a[k], b[k]), k
    pa, wa, ea = lean.get_state()
    pb, wb, eb = full.get_state()
    assert np.array_equal(pa, pb) and np.array_equal(wa, wb) and \
        np.array_equal(ea, eb)
    # the series kernel's block sums are the sums of its own series
    assert np.allclose(b2['energy'].sum(axis=0), b2['sum_energy'], rtol=1e-13)
    assert np.array_equal(b2['move_stat'].sum(axis=0), b2['num_accepted'])
    gp_walkers = eng.general_path_walkers()
    lean.close(); full.close(); eng.close()
    # the oracle on the same stream (first yield = the initial state, ACCEPTED)
    m = oracle.model_from_cfc(spec.cfc_spec)
    opos = pos.copy()
    owf = np.array([oracle.wf_abs_log(m, p) for p in opos])
    oec = np.zeros(W)
    se1, se21, na1 = oracle.vmc_ensemble(m, opos, owf, oec, spread, 11, steps,
                                         yield_initial=True)
    se2, se22, na2 = oracle.vmc_ensemble(m, opos, owf, oec, spread, 11, steps,
                                         step0=steps - 1)
    same1 = (na1 == a1['num_accepted']) & \
        (np.abs(se1 - a1['sum_energy']) <= 1e-9 * np.abs(se1))
    same2 = same1 & (na2 == a2['num_accepted']) & \
        (np.abs(se2 - a2['sum_energy']) <= 1e-9 * np.abs(se2)) & \
        (np.abs(se22 - a2['sum_energy2']) <= 1e-9 * np.abs(se22))
    # A chain whose block sums differ must have left the oracle through a
    # Metropolis test with a rounding-level margin: located with the series
    # kernel's accept series (bit-identical to the production kernel's, above)
    # and checked, at most one per run (tests/_traj.py).  Observed: 0 chains
    # at N = 16, 64 and 128.
    stat_dev = np.r_[b1['move_stat'], b2['move_stat']]
    stat_orc = stat_dev.copy()
    for c in np.nonzero(~same2)[0]:
        ch = oracle.VmcChain(m, pos[c], spread, seed=11, chain=int(c))
        _, _, st_a, _ = ch.run(steps)
        _, _, st_b, _ = ch.run(steps)
        stat_orc[:, c] = np.r_[st_a, st_b]
        assert first_difference(stat_dev[:, c], stat_orc[:, c]) is not None, \
            (c, 'same accept series but different block sums')
    same = explain_flips(oracle, m, pos, spread, 11, stat_dev, stat_orc)
    assert np.array_equal(same, same2)
    assert np.abs(opos[same2] - pa[same2]).max() < 1e-9
    if n > 32:
        assert gp_walkers == 0, 'a walker left the sorted-row path'


@pytest.mark.parametrize('log2w', [16, 18])      # 18: BASELINE configs[2]
def test_dmc_step_identities_at_scale(eng64, log2w):
    """2^16 (2^18: the benchmarked size) walkers: unit weights after branching
    (W_t == n_w), E_t equals the sum of the yielded walkers' energies, the
    cloning table is non-decreasing and only references parents, population
    capped, rerun bit-identical."""
    from phd_qmclib_amd.engine import DmcEnsemble
    rng = np.random.RandomState(2)
    target = 1 << log2w
    maxw = target * 512 // 480
    pos = 64 * rng.random_sample((target, 64))

    def run():
        d = DmcEnsemble(eng64, 6.25e-4, maxw, target, 0.5, rng_seed=9)
        d.set_state(pos)
        ser = d.run_block(9)
        st = d.get_state()
        d.close()
        return ser, st
    ser, st = run()
    ser2, st2 = run()
    assert np.array_equal(ser.energy, ser2.energy)
    assert np.array_equal(st.cloning_ref, st2.cloning_ref)
    assert np.array_equal(ser.weight, ser.num_walkers.astype(float))
    assert np.all(ser.num_walkers <= maxw) and np.all(ser.num_walkers > 0)
    nw = st.num_walkers
    assert nw == int(ser.num_walkers[-1])
    assert np.isclose(st.energy[:nw].sum(), ser.energy[-1], rtol=1e-12)
    ref = st.cloning_ref[:nw]
    assert np.all(np.diff(ref) >= 0) and ref[0] >= 0
    assert ref[-1] < int(ser.num_walkers[-2])
    # accumulated energy is the running ratio of the series
    acc = np.cumsum(ser.energy) / np.cumsum(ser.weight)
    assert np.allclose(acc, ser.accum_energy, rtol=1e-12)
    # E_ref feedback formula (qmc_base/dmc.py:769-771)
    ref_e = ser.accum_energy - 0.5 * np.log(ser.weight / target) / 6.25e-4
    assert np.allclose(ref_e, ser.ref_energy, rtol=1e-12)


@pytest.mark.parametrize('n', [64, 128, 512])
def test_model_symmetries(n):
    """Bosonic symmetry and lattice periodicity at the large-N shapes:
    permuting particles permutes the drift and leaves E, log|psi| unchanged;
    shifting every particle by one lattice period (mod L) changes nothing."""
    from phd_qmclib_amd.engine import ModelEngine
    eng = ModelEngine(box(n).cfc_spec)
    rng = np.random.RandomState(n)
    pos = n * rng.random_sample((5, n))
    base = eng.evaluate(pos)
    perm = rng.permutation(n)
    p = eng.evaluate(pos[:, perm])
    tol = 5e-10
    assert np.allclose(p.energy, base.energy, rtol=tol)
    assert np.allclose(p.wf_abs_log, base.wf_abs_log, rtol=tol)
    assert np.allclose(p.drift, base.drift[:, perm], rtol=1e-8, atol=1e-8)
    sh = eng.evaluate((pos + 1.0) % n)
    assert np.allclose(sh.energy, base.energy, rtol=tol)
    assert np.allclose(sh.wf_abs_log, base.wf_abs_log, rtol=tol)
    assert np.allclose(sh.drift, base.drift, rtol=1e-8, atol=1e-8)
    assert np.allclose(base.ith_energy.sum(axis=1), base.energy, rtol=1e-12)
    eng.close()


def test_large_n_sampling_runs():
    """C4 / C5 shapes: DMC at N = 128 and VMC at N = 512 step and stay sane."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    eng = ModelEngine(box(128).cfc_spec)
    rng = np.random.RandomState(3)
    pos = 128 * rng.random_sample((4096, 128))
    v = VmcEnsemble(eng, 4096, 0.125, rng_seed=1)
    v.set_state(pos)
    v.run_block(30, sums=False)
    d = DmcEnsemble(eng, 6.25e-4, 4608, 4096, 0.5, rng_seed=1)
    d.set_state(v.get_state()[0])
    ser = d.run_block(10)
    assert np.all(ser.num_walkers > 3000)
    assert 10 < ser.energy[-1] / ser.weight[-1] / 128 < 30
    d.close(); v.close(); eng.close()
    eng = ModelEngine(box(512).cfc_spec)
    pos = 512 * rng.random_sample((64, 512))
    v = VmcEnsemble(eng, 64, 0.125, rng_seed=1)
    v.set_state(pos)
    out = v.run_block(6)
    assert np.all(np.isfinite(out['sum_energy']))
    v.close(); eng.close()


@pytest.mark.parametrize('n', [37, 48, 63, 66, 100, 101, 126, 128, 130, 256,
                               300, 512])
def test_large_shapes_trajectories_vs_oracle(oracle, n):
    """Every lane-group shape of one walker per wavefront -- (64,1) padded,
    (64,2), (64,4), (64,8), exact and padded -- through the VMC and DMC
    kernels, against the oracle on the same Philox streams.  The sorted-row
    paths (qmc_sorted64.h, qmc_sorted128.h) on rings shorter than the
    wavefront: N = 37, 63 (odd: no half step), 48; N = 66, 126 (an odd number
    of lanes in use), 100; N = 101 (odd: the general path); above 128 the
    single-copy LDS tables, the two-pass own-particle scheme and the masked
    variants."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    from ._traj import explain_flips
    spec = box(n)
    m = oracle.model_from_cfc(spec.cfc_spec)
    eng = ModelEngine(spec.cfc_spec)
    rng = np.random.RandomState(n)
    W, ns = 5, 5
    pos0 = n * rng.random_sample((W, n))
    v = VmcEnsemble(eng, W, 0.125, rng_seed=12)
    v.set_state(pos0)
    out = v.run_block(ns, series=True)
    st_o, en_o, wf_o = [np.zeros((ns, W)) for _ in range(3)]
    for c in range(W):
        wf_o[:, c], en_o[:, c], st_o[:, c], _ = oracle.VmcChain(
            m, pos0[c], 0.125, seed=12, chain=c).run(ns)
    # (tests/_traj.py: a differing chain must show a rounding-level Metropolis
    # margin; observed: none at any size)
    same = explain_flips(oracle, m, pos0, 0.125, 12, out['move_stat'], st_o)
    assert np.allclose(en_o[:, same], out['energy'][:, same], rtol=1e-9)
    assert np.allclose(wf_o[:, same], out['wf_abs_log'][:, same], rtol=1e-9)
    v.close()
    d = DmcEnsemble(eng, 5e-4, 16, 12, 0.5, rng_seed=3)
    d.set_state(np.vstack([pos0, pos0, pos0[:2]]))
    orc = oracle.DmcEnsemble(m, np.vstack([pos0, pos0, pos0[:2]]), 5e-4, 16,
                             12, 0.5, seed=3)
    ser = d.run_block(4)
    for t in range(4):
        o = orc.step()
        assert int(ser.num_walkers[t]) == o.num_walkers, t
        assert ser.energy[t] == pytest.approx(o.energy, rel=1e-9), t
        assert ser.ref_energy[t] == pytest.approx(o.ref_energy, rel=1e-9), t
    d.close()
    eng.close()


@pytest.mark.parametrize('n', [37, 48, 64, 66, 100, 101, 128, 300, 512])
def test_long_trajectories_across_the_box_boundary(oracle, n):
    """Lane order is kept ascending with the place where positions wrap from L
    to 0 anchored at the end of the row: whenever a particle crosses the box
    boundary the whole row moves by one slot.  Long chains with wide moves
    cross it many times; positions (handed back in particle order through the
    labels), log|psi| and the carried energy must still be the oracle's on the
    same Philox streams.

    Which code keeps the order at this cutoff (L / 4, pairs classified from
    the sines), by size:
      37, 48, 64    (64, 1): `sort_lanes64` -- odd-even passes until the lanes
                    ascend, `anchor_seam` as its first move when the inversion
                    sits at an end of the row -- then the sorted-row pair sum;
      66, 100, 128  (64, 2): `sort_rows128`, with `anchor_seam_rows<2>` in the
                    same role;
      101           (64, 2), odd N: no sorted rows exist, nothing reorders the
                    row and the general pair sum takes it in any order;
      300, 512      (64, 8): the `anchor_seam_rows` + `resort_linear_rows`
                    branch of `vmc_step_kernel` itself.
    The `anchor_seam` + `resort_linear<64>` branch of the stepping kernels and
    their `anchor_seam_rows` branch at (64, 2) are compiled only for models
    that classify pairs from the positions (cutoff above 0.45 L): they are
    pinned by tests/test_gpu_zclass_steps.py."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    from ._traj import explain_flips
    spec = box(n)
    m = oracle.model_from_cfc(spec.cfc_spec)
    eng = ModelEngine(spec.cfc_spec)
    rng = np.random.RandomState(1000 + n)
    W, ns, spread = 6, 60, 0.6
    L = float(n)
    pos0 = L * rng.random_sample((W, n))
    v = VmcEnsemble(eng, W, spread, rng_seed=21)
    v.set_state(pos0)
    out = v.run_block(ns, series=True)
    pos, wf, ec = v.get_state()
    crossings = 0
    stat_o = np.zeros((ns, W), dtype=bool)
    pos_o, wf_o = np.zeros((W, n)), np.zeros(W)
    for c in range(W):
        ch = oracle.VmcChain(m, pos0[c], spread, seed=21, chain=c)
        prev = np.mod(pos0[c], L)
        for t in range(ns):
            _, _, st, _ = ch.run(1)
            stat_o[t, c] = bool(st[0])
            cur = np.mod(ch.pos, L)
            crossings += int((np.abs(cur - prev) > 0.5 * L).sum())
            prev = cur
        pos_o[c], wf_o[c] = np.mod(ch.pos, L), float(ch.wf[0])
    # (tests/_traj.py: a differing chain must show a rounding-level Metropolis
    # margin, at most one; observed: none at any size)
    same = explain_flips(oracle, m, pos0, spread, 21, out['move_stat'], stat_o)
    assert np.allclose(np.mod(pos[same], L), pos_o[same], rtol=0, atol=1e-9)
    assert np.allclose(wf[same], wf_o[same], rtol=1e-9, atol=1e-8)
    assert crossings >= 3, 'the chains did cross the boundary'
    v.close()
    eng.close()


@pytest.mark.parametrize('n', [48, 64, 100, 128])
def test_clustered_walkers_take_the_general_path_vs_oracle(oracle, n):
    """The sorted-row pair sums (qmc_sorted64.h, qmc_sorted128.h) assume, per
    walker, that the farthest partner of the rotation is closer than L - rm;
    a walker with more than half of its particles inside L / 4 fails that check
    and is evaluated by `eval_walker` inside the same kernel.  Chains started
    from configurations squeezed into a fifth of the box (and, beside them,
    ordinary ones: the choice is per walker) must follow the oracle on the same
    Philox streams while they spread out again -- VMC and DMC."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    from ._traj import explain_flips
    spec = box(n)
    m = oracle.model_from_cfc(spec.cfc_spec)
    eng = ModelEngine(spec.cfc_spec)
    rng = np.random.RandomState(7000 + n)
    W, ns, spread = 8, 24, 0.125
    L = float(n)
    pos0 = L * rng.random_sample((W, n))
    pos0[::2] = 0.37 * L + 0.2 * L * rng.random_sample((W // 2, n))
    eng.general_path_walkers(reset=True)
    v = VmcEnsemble(eng, W, spread, rng_seed=33)
    v.set_state(pos0)
    out = v.run_block(ns, series=True)
    # the squeezed rows did take the general path (and the ordinary ones did
    # not: at most W / 2 walkers per yield)
    gp = eng.general_path_walkers()
    assert W // 2 <= gp <= (W // 2) * ns, gp
    st_o, en_o, wf_o = [np.zeros((ns, W)) for _ in range(3)]
    for c in range(W):
        wf_o[:, c], en_o[:, c], st_o[:, c], _ = oracle.VmcChain(
            m, pos0[c], spread, seed=33, chain=c).run(ns)
    same = explain_flips(oracle, m, pos0, spread, 33, out['move_stat'], st_o)
    assert np.allclose(en_o[:, same], out['energy'][:, same], rtol=1e-9)
    assert np.allclose(wf_o[:, same], out['wf_abs_log'][:, same], rtol=1e-9,
                       atol=1e-8)
    v.close()
    d = DmcEnsemble(eng, 5e-4, 16, 8, 0.5, rng_seed=5)
    d.set_state(pos0)
    orc = oracle.DmcEnsemble(m, pos0, 5e-4, 16, 8, 0.5, seed=5)
    ser = d.run_block(6)
    for t in range(6):
        o = orc.step()
        assert int(ser.num_walkers[t]) == o.num_walkers, t
        assert ser.energy[t] == pytest.approx(o.energy, rel=1e-9), t
    assert eng.general_path_walkers() >= W // 2     # the DMC kernel too
    d.close()
    eng.close()


def test_random_specs_all_shapes_vs_oracle(oracle):
    """Differential test over random models at random sizes up to 512 (every
    lane-group shape, exact and padded, both pair classifiers): evaluate on
    the device against the oracle, 2e-11 relative per configuration."""
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    rng = np.random.RandomState(424242)
    done = 0
    sizes = [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255,
             256, 257, 400, 511, 512]
    while done < 40:
        n = int(rng.choice(sizes)) if done < 30 else int(rng.randint(2, 513))
        L = float(np.round(n * rng.uniform(0.7, 1.8), 3))
        kw = dict(lattice_depth=float(rng.choice([0.0, rng.uniform(1, 120)])),
                  lattice_ratio=float(np.round(rng.uniform(0.2, 3.0), 3)),
                  interaction_strength=float(10 ** rng.uniform(-1, 1.5)),
                  boson_number=n, supercell_size=L,
                  tbf_contact_cutoff=float(L * rng.uniform(0.01, 0.494)))
        try:
            spec = Spec(**kw)
            cfc = spec.cfc_spec
        except ValueError:
            continue
        m = oracle.model_from_cfc(cfc)
        eng = ModelEngine(cfc)
        pos = L * rng.random_sample((3, n))
        pos[2] = np.sort(pos[2])            # an ordered configuration too
        out = eng.evaluate(pos)
        eng.close()
        wf, en, ie, fd = oracle.evaluate_set(m, pos)
        for name, got, ref in (('wf', out.wf_abs_log, wf), ('E', out.energy, en),
                               ('ith', out.ith_energy, ie),
                               ('drift', out.drift, fd)):
            scale = np.maximum(1.0, np.abs(ref).reshape(3, -1).max(1))
            if name in ('wf', 'E'):
                scale = np.maximum(scale, np.abs(ie).max(1))
            err = np.abs(got - ref).reshape(3, -1).max(1) / scale
            assert err.max() <= 2e-11, (kw, name, err)
        done += 1
