"""Single-particle VMC sweeps (engine.VmcEnsemble(move='particle'),
csrc/qmc_vmc_sweep.h) against their restatement on the same Philox blocks
(tests/_vmc_sweep_restatement.py; cases and seeds: tests/_vmc_sweep_cases.py,
whose margin condition -- no |2 D - log u| below 1e-7 in the restatement,
checked without a GPU in tests/test_vmc_sweep_host.py -- lets every accept
decision be demanded identical).

Tolerances: positions 1e-10 modulo L; log|psi| and energy 2e-11 max(1, |x|),
the suite's (tests/_traj.py, tests/test_gpu_sorted_pins.py)."""
import numpy as np
import pytest

from . import _vmc_sweep_cases as sc

pytestmark = pytest.mark.gpu

RTOL = 2e-11
POS_TOL = 1e-10
CASES = [(cid, sp) for cid in sc.IDS for sp in sc.SPREADS]


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def ring(a, b, L):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return float(np.max(np.minimum(d, L - d)))


@pytest.fixture(scope='module')
def engines():
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = ModelEngine(sc.make_spec(cid).cfc_spec)
        return cache[cid]
    yield get
    for e in cache.values():
        e.close()


def ensemble(eng, cid, spread, rows=None, chain0=0, **kw):
    from phd_qmclib_amd.engine import VmcEnsemble
    rows = sc.start_rows(cid) if rows is None else rows
    v = VmcEnsemble(eng, len(rows), spread, rng_seed=sc.seed_of(cid, spread),
                    chain0=chain0, move='particle', **kw)
    v.set_state(rows)
    return v


_runs = {}


def device_run(engines, cid, spread):
    """The device's block of a case, run once and shared (not modified)."""
    key = (cid, spread)
    if key not in _runs:
        v = ensemble(engines(cid), cid, spread)
        out = v.run_block(sc.NYIELD, series=True, confs=True)
        out['state'] = v.get_state()
        v.close()
        _runs[key] = out
    return _runs[key]


@pytest.mark.parametrize('cid,spread', CASES)
def test_sweeps_against_restatement(engines, oracle, cid, spread):
    ref = sc.preconditions(oracle, cid, spread)
    out = device_run(engines, cid, spread)
    L = float(sc.make_spec(cid).supercell_size)
    n = ref['pos'].shape[2]
    pos = out['pos']
    assert pos.shape == ref['pos'].shape == (sc.NYIELD, sc.W, n)
    # the initial yield is the initial state as given
    assert np.array_equal(pos[0], sc.start_rows(cid))
    # every decision, read from the series: a particle moved or it did not
    moved = pos[1:] != pos[:-1]
    assert np.array_equal(moved, ref['accepted']), \
        int((moved != ref['accepted']).sum())
    figures = dict(pos=ring(pos, ref['pos'], L),
                   wf=rel(out['wf_abs_log'], ref['wf_abs_log']),
                   energy=rel(out['energy'], ref['energy']))
    print(cid, spread, figures, 'accepted %.3f' % ref['accepted'].mean())
    assert figures['pos'] <= POS_TOL
    assert figures['wf'] <= RTOL
    assert figures['energy'] <= RTOL
    assert np.array_equal(out['move_stat'], ref['move_stat'])
    # accepted particle moves, + N for the initial yield
    assert np.array_equal(out['num_accepted'],
                          ref['accepted'].sum(axis=(0, 2)) + n)
    # the block sums are the sums of the series, the state is the last yield
    assert rel(out['sum_energy'], out['energy'].sum(axis=0)) <= 1e-13
    assert rel(out['sum_energy2'], (out['energy'] ** 2).sum(axis=0)) <= 1e-13
    st_pos, st_wf, st_e = out['state']
    assert np.array_equal(st_pos, pos[-1])
    assert np.array_equal(st_wf, out['wf_abs_log'][-1])
    assert np.array_equal(st_e, out['energy'][-1])
    # a rejected sweep carries both values over
    for name in ('wf_abs_log', 'energy'):
        same = out[name][1:] == out[name][:-1]
        assert np.all(same[~ref['move_stat'][1:]])


@pytest.mark.parametrize('cid', sc.IDS)
def test_block_in_two_parts_is_the_block(engines, cid):
    """6 yields = 2 + 4 yields, bit for bit (series or not)."""
    spread = 0.75
    whole = ensemble(engines(cid), cid, spread)
    a = whole.run_block(6, series=True, confs=True)
    parts = ensemble(engines(cid), cid, spread)
    b1 = parts.run_block(2, series=True, confs=True)
    b2 = parts.run_block(4)                     # sums only
    for name in ('pos', 'wf_abs_log', 'energy', 'move_stat'):
        assert np.array_equal(a[name][:2], b1[name]), name
    for x, y in zip(whole.get_state(), parts.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a['num_accepted'],
                          b1['num_accepted'] + b2['num_accepted'])
    assert rel(b2['sum_energy'], a['energy'][2:].sum(axis=0)) <= 1e-13
    # ... and the chains go on alike
    ra, rb = whole.run_block(3, series=True), parts.run_block(3, series=True)
    for name in ('wf_abs_log', 'energy', 'move_stat', 'sum_energy',
                 'sum_energy2', 'num_accepted'):
        assert np.array_equal(ra[name], rb[name]), name
    whole.close(); parts.close()


@pytest.mark.parametrize('cid', sc.IDS)
def test_chain_is_keyed_by_its_global_index(engines, cid):
    """Chain c at chain0 = 0 is chain 0 at chain0 = c, bit for bit."""
    spread = 0.75
    out = device_run(engines, cid, spread)
    rows = sc.start_rows(cid)
    for c in (1, sc.W - 1):
        v = ensemble(engines(cid), cid, spread, rows=rows[c:c + 1], chain0=c)
        one = v.run_block(sc.NYIELD, series=True, confs=True)
        v.close()
        for name in ('pos', 'wf_abs_log', 'energy', 'move_stat'):
            assert np.array_equal(one[name][:, 0], out[name][:, c]), (name, c)
        assert one['num_accepted'][0] == out['num_accepted'][c]
        assert one['sum_energy'][0] == out['sum_energy'][c]


@pytest.mark.parametrize('cid', sc.IDS)
def test_label_order_is_what_counts(engines, oracle, cid):
    """Rows given in a shuffled particle order: the device keeps a row by
    position, so it holds the very row it holds for the unshuffled start, under
    other labels -- and the chain follows the labels: it is the restatement of
    the shuffled rows (identical decisions; the margin condition is checked
    here on the restatement, four yields)."""
    from . import _vmc_sweep_restatement as rs
    spread = 0.75
    _, m, p = sc.model_of(oracle, cid)
    rows = sc.start_rows(cid)
    perm = np.random.RandomState(77).permutation(rows.shape[1])
    ref = rs.run_ensemble(oracle, m, p, rows[:, perm], spread,
                          sc.seed_of(cid, spread), 4)
    assert np.min(np.abs(ref['margin'])) >= sc.MARGIN
    v = ensemble(engines(cid), cid, spread, rows=rows[:, perm])
    out = v.run_block(4, series=True, confs=True)
    v.close()
    L = float(sc.make_spec(cid).supercell_size)
    assert np.array_equal(out['pos'][0], rows[:, perm])
    assert np.array_equal(out['pos'][1:] != out['pos'][:-1], ref['accepted'])
    assert ring(out['pos'], ref['pos'], L) <= POS_TOL
    assert rel(out['wf_abs_log'], ref['wf_abs_log']) <= RTOL
    assert rel(out['energy'], ref['energy']) <= RTOL
    # the initial yield evaluates the same set of positions as the unshuffled
    # start: the same values to rounding
    base = device_run(engines, cid, spread)
    assert rel(out['wf_abs_log'][0], base['wf_abs_log'][0]) <= RTOL
    assert rel(out['energy'][0], base['energy'][0]) <= RTOL


def test_eight_particles_per_lane(oracle):
    """N = 260, the (64, 8) shape: two chains, the initial state and three
    sweeps against the restatement (its margins checked here)."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    from phd_qmclib_amd.mrbp_qmc import Spec
    from . import _vmc_sweep_restatement as rs
    n, L, spread, seed = 260, 260.0, 0.75, 1
    spec = Spec(boson_number=n, supercell_size=n, tbf_contact_cutoff=0.25 * n,
                **sc._BOX)
    cfc = spec.cfc_spec
    rows = L * np.random.RandomState(9100 + n).random_sample((2, n))
    ref = rs.run_ensemble(oracle, oracle.model_from_cfc(cfc),
                          rs.model_dicts(cfc), rows, spread, seed, 4)
    assert np.min(np.abs(ref['margin'])) >= sc.MARGIN
    eng = ModelEngine(cfc)
    v = VmcEnsemble(eng, 2, spread, rng_seed=seed, move='particle')
    v.set_state(rows)
    out = v.run_block(4, series=True, confs=True)
    v.close(); eng.close()
    assert np.array_equal(out['pos'][1:] != out['pos'][:-1], ref['accepted'])
    assert ring(out['pos'], ref['pos'], L) <= POS_TOL
    assert rel(out['wf_abs_log'], ref['wf_abs_log']) <= RTOL
    assert rel(out['energy'], ref['energy']) <= RTOL
    assert np.array_equal(out['num_accepted'],
                          ref['accepted'].sum(axis=(0, 2)) + n)


@pytest.mark.parametrize('cid', ['box16', 'box64', 'half100'])
def test_move_all_is_the_ensemble_without_the_keyword(engines, cid):
    from phd_qmclib_amd.engine import VmcEnsemble
    eng = engines(cid)
    rows = sc.start_rows(cid)
    a = VmcEnsemble(eng, len(rows), 0.125, rng_seed=3)
    b = VmcEnsemble(eng, len(rows), 0.125, rng_seed=3, move='all')
    assert a.move == b.move == 'all'
    for v in (a, b):
        v.set_state(rows)
    ra = a.run_block(9, series=True, confs=True)
    rb = b.run_block(9, series=True, confs=True)
    assert sorted(ra) == sorted(rb)
    for name in ra:
        assert np.array_equal(ra[name], rb[name]), name
    ra, rb = a.run_block(7), b.run_block(7)
    for name in ra:
        assert np.array_equal(ra[name], rb[name]), name
    a.close(); b.close()


def test_arguments(engines):
    from phd_qmclib_amd._lib import QmcError
    from phd_qmclib_amd.engine import VmcEnsemble
    eng = engines('box16')
    with pytest.raises(ValueError):
        VmcEnsemble(eng, 4, 0.5, rng_seed=1, move='particle', gaussian=True)
    with pytest.raises(ValueError):
        VmcEnsemble(eng, 4, 0.5, rng_seed=1, move='sweep')
    v = ensemble(eng, 'box16', 0.5)
    assert v.move == 'particle'
    with pytest.raises(QmcError):
        v.set_tape(np.full((sc.W, 3, 17), 0.5))
    with pytest.raises(QmcError):
        v.set_tape(None)
    v.close()


def test_create_refuses_unknown_codes(engines):
    import ctypes as C
    from phd_qmclib_amd import _lib
    eng = engines('box16')
    for code in (3, -1, 7):
        p = _lib.VmcParams(4, 0.5, 1, 0, code)
        h = C.c_void_p()
        assert eng._lib.qmc_vmc_create(eng._h, C.byref(p), C.byref(h)) != 0
        assert not h.value


@pytest.mark.parametrize('cid', ['box16', 'box37', 'box64', 'half100',
                                 'hard130'])
def test_estimators_on_a_swept_ensemble(engines, cid):
    """ssf_parts, obdm_parts and pair_dist_parts read the rows the sweeps
    leave: against the batch entry points on get_state() positions, at the
    tolerances of those entry points' own tests (test_gpu_sampling.py: 1e-11
    of the largest part; test_gpu_obdm.py: 1e-12 relative on the sums;
    test_gpu_pair_dist.py: the counts themselves)."""
    eng = engines(cid)
    spec = sc.make_spec(cid)
    n, L = spec.boson_number, float(spec.supercell_size)
    rng = np.random.RandomState(31)
    W = 40
    v = ensemble(eng, cid, 0.5, rows=L * rng.random_sample((W, n)))
    v.run_block(4, sums=False)
    z = v.get_state()[0]
    modes = 12
    k = 2 * np.pi * np.arange(modes) / L
    ph = np.exp(1j * k[None, :, None] * z[:, None, :]).sum(axis=2)
    want = np.stack([(np.abs(ph) ** 2).mean(0), ph.real.mean(0),
                     ph.imag.mean(0)], axis=1)
    got = v.ssf_parts(modes)
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
    shifts = np.array([0.0, 0.3, -1.7, 0.25 * L])
    g1 = eng.one_body_density(z, shifts)
    parts = v.obdm_parts(shifts)
    assert np.allclose(parts[:, 0], g1.sum(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(parts[:, 1], (g1 ** 2).sum(axis=0), rtol=1e-12, atol=0)
    B = 24
    H = eng.pair_distribution(z, B).astype(np.float64)
    parts = v.pair_dist_parts(B)
    assert np.array_equal(parts[:, 0], H.sum(axis=0))
    assert np.array_equal(parts[:, 1], (H ** 2).sum(axis=0))
    # state_dev: the resident rows are the state, row by row a permutation
    p_pos, p_wf = v.state_dev()
    wf, rows = np.zeros(W), np.zeros((W, n))
    eng.sync()
    assert eng._lib.qmc_buffer_download(wf.ctypes.data, p_wf, wf.nbytes) == 0
    assert eng._lib.qmc_buffer_download(rows.ctypes.data, p_pos,
                                        rows.nbytes) == 0
    assert np.array_equal(wf, v.get_state()[1])
    assert np.array_equal(np.sort(rows, axis=1), np.sort(z, axis=1))
    v.close()


@pytest.mark.parametrize('cid', ['box16', 'box64', 'half100', 'hard130'])
def test_dmc_hand_off(engines, cid):
    """After set_state_from_vmc the walkers carry the swept configurations
    and their energies."""
    from phd_qmclib_amd.engine import DmcEnsemble
    eng = engines(cid)
    v = ensemble(eng, cid, 0.5)
    v.run_block(5, sums=False)
    pos = v.get_state()[0]
    d = DmcEnsemble(eng, 1e-3, 8, sc.W, 0.5, rng_seed=2)
    d.set_state_from_vmc(v)
    st = d.get_state()
    assert st.num_walkers == sc.W
    assert np.array_equal(st.confs[:sc.W, 0], pos)
    want = eng.evaluate(pos)
    assert rel(st.energy[:sc.W], want.energy) <= RTOL
    assert rel(st.confs[:sc.W, 1], want.drift) <= 1e-10
    d.close(); v.close()


def test_hand_off_lands_on_the_sorted_rows(engines):
    """N = 64 on a jittered lattice: the rows leave the sweeps position-sorted
    with their labels, so the first DMC step takes the sorted-row sums."""
    from phd_qmclib_amd.engine import DmcEnsemble
    from ._steps import jittered_lattice
    eng = engines('box64')
    rng = np.random.RandomState(5)
    rows = np.array([rng.permutation(jittered_lattice(rng, 64, 64.0))
                     for _ in range(12)])
    v = ensemble(eng, 'box64', 0.5, rows=rows)
    eng.general_path_walkers(reset=True)
    out = v.run_block(4)
    assert np.all(out['num_accepted'] > 64)
    assert eng.general_path_walkers(reset=True) == 0
    d = DmcEnsemble(eng, 1e-3, 16, 12, 0.5, rng_seed=2)
    d.set_state_from_vmc(v)
    eng.general_path_walkers(reset=True)
    d.run_block(1)
    assert eng.general_path_walkers(reset=True) == 0
    d.close(); v.close()
