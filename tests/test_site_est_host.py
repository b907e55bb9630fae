"""The host side of the site occupation estimator (no GPU):
`engine.site_statistics`, the `SiteBlocks` reductions, the spec validators,
the configuration key and the record in `dmc_est.ESTIMATORS`."""
import textwrap

import numpy as np
import pytest

from phd_qmclib_amd.util import h5lite

from . import _site_restatement as sr

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


def _rows_of(n_sites, num_occ, num_dist):
    """The row [occ | corr] of site counts n[W, S], summed over the walkers,
    counted directly."""
    n_sites = np.asarray(n_sites)
    S = n_sites.shape[1]
    occ = [(np.minimum(n_sites, num_occ - 1) == k).sum()
           for k in range(num_occ)]
    corr = [sum(int(n[c]) * int(n[(c + d) % S]) for n in n_sites
                for c in range(S)) for d in range(num_dist)]
    return np.array(occ + corr, dtype=np.float64)


def test_site_statistics_of_one_particle_per_site():
    from phd_qmclib_amd.engine import site_statistics
    S, W, P = 8, 5, 3
    rows = _rows_of(np.ones((W, S), dtype=int), P, S)
    assert np.array_equal(rows[:P], [0, S * W, 0])
    assert np.array_equal(rows[P:], np.full(S, S * W))
    st = site_statistics(rows, W, S, S, P)
    assert np.array_equal(st.occupation_dist, [0.0, 1.0, 0.0])
    assert st.mean_occupation == 1.0
    assert st.variance == 0.0
    assert np.array_equal(st.correlation, np.zeros(S))
    for ell in range(1, S + 1):
        assert st.number_variance(ell) == 0.0
    for bad in (0, S + 1):
        with pytest.raises(ValueError):
            st.number_variance(bad)
    # without a correlation part there is no variance
    only = site_statistics(rows[:P], W, S, S, P)
    assert only.variance is None and only.correlation.shape == (0,)
    with pytest.raises(ValueError):
        site_statistics(rows, W, S, S, 0)
    with pytest.raises(ValueError):
        site_statistics(rows, W, S, S, len(rows) + 1)


def test_site_statistics_against_a_direct_count():
    from phd_qmclib_amd.engine import site_statistics
    rng = np.random.RandomState(3)
    S, N, W, P = 6, 9, 40, 5
    pos = S * rng.random_sample((W, N))
    n = sr.site_counts(pos, float(S), 0.25)
    assert (n.sum(axis=1) == N).all()
    rows = _rows_of(n, P, S)
    # the restatement the GPU test relies on counts the same
    assert np.array_equal(sr.site_rows(pos, float(S), 0.25, P, S).sum(axis=0),
                          rows)
    st = site_statistics(rows, W, N, S, P)
    assert abs(st.occupation_dist.sum() - 1.0) < 1e-15
    assert st.mean_occupation == N / S
    assert np.isclose(st.variance, (n ** 2).mean() - (N / S) ** 2,
                      rtol=1e-13)
    # the number variance of ell consecutive sites, counted window by window
    # (all S windows of every walker, periodic); N is conserved, so the
    # whole ring has none
    for ell in range(1, S + 1):
        win = np.array([[n[w, np.arange(c, c + ell) % S].sum()
                         for c in range(S)] for w in range(W)])
        direct = (win ** 2).mean() - (ell * N / S) ** 2
        assert np.isclose(st.number_variance(ell), direct, rtol=1e-12,
                          atol=1e-12), ell
    assert abs(st.number_variance(S)) < 1e-12
    # leading axes: one row per block, walkers per block
    stacked = site_statistics(np.stack([rows, 2 * rows]), [W, 2 * W], N, S, P)
    assert np.array_equal(stacked.correlation[0], stacked.correlation[1])
    assert np.array_equal(stacked.number_variance(3)[0], st.number_variance(3))


def test_restatement_sites_and_edges():
    # site c is [c - z_b/2, c + 1 - z_b/2): with z_b = 0.5 the boundary of
    # sites 0 and 1 sits at 0.75, and the last quarter belongs to site 0
    pos = np.array([[0.0, 0.7, 0.8, 3.7, 3.8]])
    assert sr.half_barrier(1) == 0.25
    assert np.array_equal(sr.site_counts(pos, 4.0, 0.25), [[3, 1, 0, 1]])
    assert sr.ambiguous_particles(pos, 4.0, 0.25) == []
    assert sr.ambiguous_particles(np.array([[0.75, 1.0]]), 4.0, 0.25) == [
        (0, 0)]
    assert sr.ambiguous_particles(np.array([[3.75]]), 4.0, 0.25) == [(0, 0)]
    rows = sr.site_rows(pos, 4.0, 0.25, 3, 4)
    assert np.array_equal(rows, [[1, 2, 1, 11, 6, 2, 6]])
    assert rows[0, 3:].sum() == 25
    # forward walking: a clone inherits the row of its parent
    steps = [(pos, np.array([0]), 1),
             (np.array([[0.1] * 5, [1.1] * 5]), np.array([0, 0]), 2)]
    mixed, pure, amb = sr.forward_walk(steps, 4.0, 0.25, 3, 1, 2)
    assert amb == []
    assert np.array_equal(mixed, [[1, 2, 1, 11], [6, 0, 2, 50]])
    assert np.array_equal(pure, [[1, 2, 1, 11], [4, 2, 2, 36]])


def test_spec_validators():
    import attr
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    s = dmc.SiteEstSpec(np.int64(4), 3)
    assert s == dmc.SiteEstSpec(4, 3, True, 99999999)
    assert dmc.SiteEstSpec(4).num_distances == 0
    assert dmc.SiteEstSpec(1, 255).num_distances == 255
    assert hash(s) == hash(dmc.SiteEstSpec(4, 3))
    for bad in (dict(num_occupations=0), dict(num_occupations=-1),
                dict(num_occupations=1.5), dict(num_occupations=True),
                dict(num_occupations=2, num_distances=-1),
                dict(num_occupations=2, num_distances=255),
                dict(num_occupations=257),
                dict(num_occupations=2, pfw_num_time_steps=0)):
        with pytest.raises(ValueError):
            dmc.SiteEstSpec(**bad)
    # keyword only on Sampling: the positional order stays
    by_name = {f.name: f for f in attr.fields(dmc.Sampling)}
    assert by_name['site_est_spec'].default is None
    assert by_name['site_est_spec'].kw_only
    smp = dmc.Sampling(mrbp_qmc.Spec(**MODEL), 1e-3, 12, 10, rng_seed=1,
                       site_est_spec=s)
    assert smp.site_est_spec is s and len(smp.cfc_spec) == 6
    assert dmc_base.SamplingBlock._field_defaults['iter_site'] is None
    blk = dmc_base.SamplingBlock(None, None, iter_site=np.zeros((3, 7)))
    assert blk.iter_site.shape == (3, 7) and blk.iter_pair_dist is None
    # the procedure's spec
    x = dmc_exec.SiteEstSpec(np.int64(4), 3)
    assert x == dmc_exec.SiteEstSpec(4, 3, True)
    assert dmc_exec.SiteEstSpec(4, as_pure_est=0).as_pure_est is False
    for bad in (dict(num_occupations=0), dict(num_occupations=2,
                                              num_distances=-1),
                dict(num_occupations=200, num_distances=57)):
        with pytest.raises(ValueError):
            dmc_exec.SiteEstSpec(**bad)
    with pytest.raises(TypeError):
        dmc_exec.SiteEstSpec(1.5)


def test_proc_from_config_and_sampling():
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    base = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                num_time_steps_block=8, max_num_walkers=12,
                target_num_walkers=10, rng_seed=5)
    # forward walking spans the block: a configured length is dropped
    proc = dmc_exec.Proc.from_config(dict(base, site_spec=dict(
        num_occupations=5, num_distances=9, pfw_num_time_steps=3)))
    assert proc.site_spec == dmc_exec.SiteEstSpec(5, 9, True)
    assert proc.should_eval_site
    cfg = proc.as_config()
    assert cfg['site_spec'] == dict(num_occupations=5, num_distances=9,
                                    as_pure_est=True)
    assert dmc_exec.Proc.from_config(cfg) == proc
    by_kw = dmc_exec.Proc(proc.model_spec, 1e-3, num_blocks=6,
                          num_time_steps_block=8, max_num_walkers=12,
                          target_num_walkers=10, rng_seed=5,
                          site_spec=dmc_exec.SiteEstSpec(5, 9))
    assert by_kw == proc
    s = proc.sampling
    assert s.site_est_spec == dmc.SiteEstSpec(5, 9, True, 8)
    assert s.obdm_est_spec is None and s.pair_dist_est_spec is None
    mixed = dmc_exec.Proc.from_config(dict(base, site_spec=dict(
        num_occupations=3, as_pure_est=False)))
    assert mixed.sampling.site_est_spec == dmc.SiteEstSpec(3, 0, False, 8)
    for absent in (base, dict(base, site_spec=None)):
        plain = dmc_exec.Proc.from_config(absent)
        assert plain.site_spec is None and not plain.should_eval_site
        assert 'site_spec' not in plain.as_config()
        assert plain.sampling.site_est_spec is None


def test_config_loader_accepts_site_spec(tmp_path):
    from phd_qmclib_amd.mrbp_qmc import dmc_exec
    text = textwrap.dedent('''\
        meta:
          name: "n"
          description: "d"
          author: "a"
          institution: "i"
          author_email: "e@x"
          category: "c"
          tags: ["qmc"]
        app_spec:
          - proc:
              model_spec:
                lattice_depth: 24
                lattice_ratio: 1
                interaction_strength: 1.0
                boson_number: 16
                supercell_size: 16.0
                tbf_contact_cutoff: 4
              time_step: 1e-3
              num_blocks: 4
              site_spec:
                num_occupations: 6
                num_distances: 9
            proc_input:
              type: "MODEL_SYS_CONF"
              dist_type: "RANDOM"
            proc_output:
              type: "HDF5_FILE"
              location: "out.h5"
              group: "dmc-proc-ID0"
            proc_id: 0
        ''')
    path = tmp_path / 'dmc-spec.yml'
    path.write_text(text)
    app = dmc_exec.CLIApp.from_config(dmc_exec.config_loader.load(path))
    proc = app.app_spec[0].proc
    assert proc.site_spec == dmc_exec.SiteEstSpec(6, 9, True)
    assert proc.sampling.site_est_spec.pfw_num_time_steps == 512


def test_estimators_record_resolves():
    from phd_qmclib_amd.dist import DistributedDmc  # noqa: F401
    from phd_qmclib_amd.engine import DmcEnsemble
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base, dmc_est
    from phd_qmclib_amd.qmc_exec import io
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    keys = [est.key for est in dmc_est.ESTIMATORS]
    assert keys[-1] == 'site' and keys.count('site') == 1
    est = dmc_est.ESTIMATORS[-1]
    assert hasattr(dmc_exec.Proc, 'should_eval_site')
    assert est.proc_field in [f.name for f in
                              dmc_exec.Proc.__attrs_attrs__]
    assert est.sampling_field in [f.name for f in
                                  dmc.Sampling.__attrs_attrs__]
    assert est.block_field in dmc_base.SamplingBlock._fields
    assert est.key in [f.name for f in dd.PropsDataBlocks.__attrs_attrs__]
    assert est.series_field is None     # (the rows are not kept as a series)
    assert getattr(dmc_exec, est.spec_class) is dmc_exec.SiteEstSpec
    assert getattr(dmc, est.spec_class) is dmc.SiteEstSpec
    assert getattr(dd, est.blocks_class) is dd.SiteBlocks
    assert est.proc_field in io.EST_SPEC_GROUPS
    assert callable(DmcEnsemble.set_site_estimator)
    assert callable(DmcEnsemble.read_site)
    assert est.ensemble_attr == 'site_shape'
    assert est.refusal.startswith(
        'the site occupation estimator is single-GPU only')
    # the record's functions on a procedure spec
    spec = dmc_exec.SiteEstSpec(5, 9, False)
    assert est.row_shape(spec) == (14,)
    assert est.sampling_args(spec, 8, None) == (5, 9, False, 8)
    assert est.config_kwargs(dict(num_occupations=5, pfw_num_time_steps=3)) \
        == dict(num_occupations=5)
    assert est.config_kwargs(None) is None

    class Ens:
        calls = []

        def set_site_estimator(self, *args):
            self.calls.append(args)

        def read_site(self, nts):
            return ('rows', nts)

    ens = Ens()
    est.enable(ens, dmc.SiteEstSpec(5, 9, False, 8))
    assert ens.calls == [(5, 9, False, 8)]
    assert est.read(ens, 6) == ('rows', 6)


def _blocks(pure, keep):
    """Hand-made rows of 3 blocks of 4 steps through the record's reduce and
    wrap -> (SiteBlocks, rows[3, 4, K], walkers[3, 4])."""
    from phd_qmclib_amd.mrbp_qmc import dmc_exec
    from phd_qmclib_amd.qmc_base import dmc as dmc_base, dmc_est
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    est = dmc_est.ESTIMATORS[-1]
    S, N, P, D = 6, 9, 5, 4
    rng = np.random.RandomState(7)
    nw = np.array([[10, 11, 12, 12], [12, 12, 11, 9], [9, 10, 10, 10]],
                  dtype=np.uint64)
    rows = np.zeros((3, 4, P + D))
    for b in range(3):
        for t in range(4):
            pos = S * rng.random_sample((int(nw[b, t]), N))
            rows[b, t] = sr.site_rows(pos, float(S), 0.25, P, D).sum(axis=0)
    spec = dmc_exec.SiteEstSpec(P, D, pure)
    w = nw.astype(np.float64)
    totals = np.zeros((3, P + D))
    pure_fac = np.ones(3)
    for b in range(3):
        props = dmc_base.PropsData(None, w[b], nw[b], None, None)
        if not keep:        # (the container reduces kept rows itself)
            totals[b], = est.reduce(rows[b], props, 4, keep, spec)
        else:
            assert est.reduce(rows[b], props, 4, keep, spec) == ()
        pure_fac[b] = nw[b, 3] / w[b].sum()
    if keep:
        props = dmc_base.PropsData(None, w, nw, None, None)
    else:
        props = dmc_base.PropsData(None, w.sum(axis=1), nw.sum(axis=1), None,
                                   None)
    got = est.wrap(dd.SiteBlocks, [totals], rows if keep else None, props, 4,
                   keep, spec, pure_fac)
    return got, rows, nw


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('pure', [False, True])
def test_site_blocks_reductions(pure, keep):
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.engine import site_statistics
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    S, N, P, D = 6, 9, 5, 4
    blocks, rows, nw = _blocks(pure, keep)
    assert type(blocks) is dd.SiteBlocks and blocks.num_occupations == P
    assert isinstance(blocks, dd.SetPropBlocks) and len(blocks) == 3
    # mixed: the steps of a block summed; pure: its last step
    if pure:
        want, weights = rows[:, 3], nw[:, 3].astype(np.float64)
    else:
        want, weights = rows.sum(axis=1), nw.sum(axis=1).astype(np.float64)
    assert np.array_equal(blocks.totals, want)
    assert np.allclose(blocks.weight_totals[:, 0], weights, rtol=1e-15)
    model = mrbp_qmc.Spec(**dict(MODEL, boson_number=N, supercell_size=S,
                                 tbf_contact_cutoff=1.5))
    row = want.sum(axis=0) / weights.sum()       # the row of one walker
    stats = site_statistics(row, 1.0, N, S, P)
    pn, pn_err = blocks.occupation_distribution()
    assert np.allclose(pn, stats.occupation_dist, rtol=1e-13)
    assert abs(pn.sum() - 1.0) < 1e-14
    corr, corr_err = blocks.site_correlation(model)
    assert np.allclose(corr, stats.correlation, rtol=1e-12, atol=1e-13)
    ells, var, var_err = blocks.number_variance(D, model)
    assert np.array_equal(ells, [1, 2, 3, 4])
    assert np.allclose(var, [stats.number_variance(e) for e in ells],
                       rtol=1e-12, atol=1e-13)
    for err in (pn_err, corr_err, var_err):
        assert np.isfinite(err).all() and (err >= 0).all()
    # reblocked errors, as the other containers: those of the columns
    assert np.allclose(corr_err, np.nan_to_num(blocks.mean_error)[P:] / S)
    # one distance with an error: the error of the window is |weight| times it
    assert np.isclose(var_err[0], corr_err[0])
    assert np.isclose(var_err[1], np.hypot(2 * corr_err[0], 2 * corr_err[1]))
    with pytest.raises(ValueError):
        blocks.number_variance(D + 1, model)
    both = blocks + dd.SiteBlocks(blocks.totals[:2], blocks.weight_totals[:2],
                                  P)
    assert type(both) is dd.SiteBlocks and len(both) == 5
    assert both.num_occupations == P
    with pytest.raises(TypeError):
        blocks + dd.SiteBlocks(blocks.totals, blocks.weight_totals, P - 1)


def test_site_blocks_of_one_particle_per_site():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.qmc_exec.data import dmc as dd
    S, P = 16, 3
    weights = np.full((4, 1), 8.0)
    totals = np.zeros((4, P + S))
    totals[:, 1] = S * weights[:, 0]
    totals[:, P:] = S * weights
    blocks = dd.SiteBlocks(totals, weights, P)
    pn, pn_err = blocks.occupation_distribution()
    assert np.array_equal(pn, [0.0, 1.0, 0.0])
    assert np.array_equal(pn_err, np.zeros(P))
    corr, corr_err = blocks.site_correlation(mrbp_qmc.Spec(**MODEL))
    assert np.array_equal(corr, np.zeros(S))
    assert np.array_equal(corr_err, np.zeros(S))
    _, var, var_err = blocks.number_variance(S, mrbp_qmc.Spec(**MODEL))
    assert np.array_equal(var, np.zeros(S))
    assert np.array_equal(var_err, np.zeros(S))


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
    totals, weights = rng.rand(6, 9), 10.0 + rng.rand(6, 1)
    for on in (True, False):
        cfg = dict(model_spec=MODEL, time_step=1e-3, num_blocks=6,
                   num_time_steps_block=8, max_num_walkers=12,
                   target_num_walkers=10, rng_seed=5)
        if on:
            cfg['site_spec'] = dict(num_occupations=4, num_distances=5)
        proc = dmc_exec.Proc.from_config(cfg)
        data = dd.SamplingData(dd.PropsDataBlocks(
            dd.EnergyBlocks(rng.rand(6), w), dd.WeightBlocks(w),
            dd.NumWalkersBlocks(rng.randint(8, 12, 6).astype(np.uint64)),
            site=dd.SiteBlocks(totals, weights, 4) if on else None))
        h = dmc_exec.HDF5FileHandler(str(tmp_path / f'r{int(on)}.h5'), 'run-A')
        h.dump(dmc_exec.ProcResult(state, proc, data))
        with h5lite.open_file(h.location, 'r') as f:
            q = f['run-A/dmc']
            extra = ['site_spec'] if on else []
            assert sorted(q['proc_spec'].keys()) == ['model_spec'] + extra
            extra = ['site'] if on else []
            assert sorted(q['data/blocks'].keys()) == sorted(
                ['energy', 'num_walkers', 'weight'] + extra)
            if on:
                assert sorted(q['data/blocks/site'].keys()) == [
                    'totals', 'weight_totals']
        back = h.load()
        assert back.proc == proc
        b = back.data.blocks
        assert b.obdm is None and b.pair_dist is None
        if on:
            assert type(b.site) is dd.SiteBlocks
            assert b.site.num_occupations == 4
            assert np.array_equal(b.site.totals, totals)
            assert np.array_equal(b.site.weight_totals, weights)
            assert back.proc.site_spec == dmc_exec.SiteEstSpec(4, 5, True)
        else:
            assert b.site is None
