"""The float pair loop (`fast_math`, the reference's `jit_fastmath`) INSIDE the
VMC / DMC stepping kernels at 33 <= N <= 128: the sorted-row pair sums of
csrc/qmc_sorted64.h and qmc_sorted128.h instantiated with R = float -- the
clamped tangent / cotangent quotients of `sorted_particle_setup`, the exponent
folds (`q_fold`) of the running log-psi products, the two-wide LDS reads of
`SlotPair<float>`, the separate one-body logarithm, the rotations cast to R.
`tests/test_gpu_fastmath.py` reaches the float loop through `qmc_evaluate`
only, which takes the general pair sum, and through block-averaged energies;
`tests/test_gpu_sorted_pins.py` pins the sorted rows at 2e-11 with R = double
only.  Here the same single steps run in float, against the reference's
goldens and the fp64 oracle, at the tolerances of test_gpu_fastmath.py
(2e-5: energy and log|psi| of max(1, |ref|), drift of the largest |drift| of
the configuration):

1. the forced first VMC yield and the zero-move DMC step on the golden
   configurations of every sorted-row shape;
2. the same two steps over random models with particles on and next to the
   poles of tan(k2 z - phi), tan(k2 z) and at z = 1e-9;
3. real steps on Philox streams: VMC chains follow the oracle's accept /
   reject series wherever the oracle's own Metropolis margin is not marginal,
   a DMC population keeps the oracle's walker counts and cloning table;
4. the shapes where the variant does not exist (ideal gas, cutoff near L / 2:
   the double path, 2e-11) and N = 130 (the general pair sum in float inside
   the step kernels).

The achieved maxima go to the report file of test_gpu_fastmath.py
(fastmath_report.json: `steps_golden`, `steps_pole_rows`, `steps_real_step`)
and are quoted in DESIGN.md section 4.
"""
import os
from math import pi

import numpy as np
import pytest

from .test_gpu_fastmath import (TOL_DRIFT, TOL_ENERGY, TOL_WF, _report,
                                min_separation)
from ._models import spec_from_golden
from .test_gpu_parity import close, worst

pytestmark = pytest.mark.gpu

TAGS = ['box64', 'box128', 'deep100', 'box37', 'box48', 'box100', 'box126']
RTOL64 = 2e-11                  # the double path (test_gpu_parity.RTOL)
STREAM_DMC_BRANCH = 2           # oracle/qmc_oracle.h: ORC_STREAM_DMC_BRANCH

# what the tests of this module measured, by report key (the report file is
# rewritten with the whole record of a key every time one entry is added)
_RECORD = {'steps_golden': {}, 'steps_pole_rows': {}, 'steps_real_step': {}}


def _record(key, name, rows):
    _RECORD[key][name] = rows
    _report({key: dict(_RECORD[key])})


def errors(got, ref, drift=False):
    """Per configuration: max |got - ref| over the configuration, of
    max(1, |ref|) (energy, log|psi|) or of the largest |drift| -> [W]."""
    ref2 = np.asarray(ref, dtype=np.float64)
    ref2 = ref2.reshape(ref2.shape[0], -1)
    got2 = np.asarray(got, dtype=np.float64).reshape(ref2.shape)
    top = np.abs(ref2).max(1)
    scale = np.maximum(top, 1e-300) if drift else np.maximum(1.0, top)
    return np.abs(got2 - ref2).max(1) / scale


def jittered_rows(rng, W, n, L):
    """Particles spread like an equilibrated walker: a lattice of spacing
    L / n, every particle displaced by up to 0.3 spacings."""
    return (np.arange(n) + 0.5 + 0.6 * (rng.random_sample((W, n)) - 0.5)) \
        * (L / n)


@pytest.fixture(scope='module')
def fast_engines(golden_params):
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = ModelEngine(
                spec_from_golden(golden_params, tag).cfc_spec, fast_math=True)
        return cache[tag]
    yield get
    for e in cache.values():
        e.close()


def vmc_first_yield(eng, pos, series, spread=0.125):
    """The forced first yield of chains started at pos[W, N] -> (energy[W],
    log|psi|[W]); the exact asserts of the double test are made here."""
    from phd_qmclib_amd.engine import VmcEnsemble
    W = pos.shape[0]
    v = VmcEnsemble(eng, W, spread, rng_seed=1)
    v.set_state(pos)
    out = v.run_block(1, series=series)
    # (the block sums of a one-yield block ARE the first yield: the production
    # kernel has no series)
    en = out['energy'][0] if series else out['sum_energy']
    assert np.all(out['num_accepted'] == 1)
    p, wf, ec = v.get_state()
    if series:
        assert np.array_equal(out['wf_abs_log'][0], wf)
        assert out['move_stat'].all()
    assert np.array_equal(p, pos)           # the state is handed back as given
    assert close(ec, en, 1e-14)             # the carried energy IS that yield
    v.close()
    return np.array(en), wf


def dmc_zero_move_step(eng, pos):
    """Two steps of time_step = 1e-300 under a tape of zero normals -> (energy,
    drift) of the first step's children; the exact asserts are made here."""
    from phd_qmclib_amd.engine import DmcEnsemble
    W, n = pos.shape
    L = float(eng.cfc_spec.model_params.supercell_size)
    d = DmcEnsemble(eng, 1e-300, W, W, 0.5, rng_seed=1)
    d.set_state(pos)
    d.set_tape(np.zeros(2 * W), np.zeros(2 * W * n), [0, W], [0, W * n])
    ser = d.run_block(2)
    assert np.array_equal(ser.num_walkers, [W, W])
    st = d.get_state()
    assert st.num_walkers == W
    assert np.array_equal(st.cloning_ref[:W], np.arange(W))
    # positions: unchanged (a particle at exactly 0 may come back as 2 F dt, or
    # as L when its drift is negative, as in the double test)
    dz = np.abs(st.confs[:W, 0] - pos)
    assert np.all(np.minimum(dz, L - dz) <= 1e-250)
    assert np.array_equal(ser.weight, [W, W])
    # E_t of the second yield: the sum of those energies (unit weights)
    assert close(ser.energy[1], st.energy[:W].sum(), rtol=1e-13 * W)
    d.close()
    return st.energy[:W].copy(), st.confs[:W, 1].copy()


def check_float_rows(what, err, keep):
    """err: {quantity: [W]} -- TOL_* on the rows `keep`; on the others
    (near-contact) TOL_* for energy and log|psi|, half of the largest
    component for the drift."""
    for name, e in err.items():
        print(what, name, 'kept rows', e[keep], 'near contact', e[~keep])
    assert np.all(np.isfinite(np.concatenate(list(err.values()))))
    if 'energy' in err:
        assert err['energy'].max() <= TOL_ENERGY, (what, err['energy'])
    if 'wf_abs_log' in err:
        assert err['wf_abs_log'].max() <= TOL_WF, (what, err['wf_abs_log'])
    if 'drift' in err:
        assert err['drift'][keep].max() <= TOL_DRIFT, (what, err['drift'])
        if (~keep).any():
            assert err['drift'][~keep].max() <= 0.5, (what, err['drift'])


def summary(err, keep):
    rows = {}
    for name, e in err.items():
        rows[name] = dict(f32_max_rel=float(e[keep].max()),
                          f32_near_contact=float(e[~keep].max())
                          if (~keep).any() else None)
    return rows


# ---------------------------------------------------------------------------
# 1. the golden configurations
# ---------------------------------------------------------------------------

def golden_keep(golden_kernels, tag, L):
    """(verified from kernels.npz alone: 4-6 of the 8 rows of every tag are
    separated by more than 1e-3; the other rows hold a pair 1e-3 ... 1e-12
    apart)"""
    pos = golden_kernels[tag + '/pos']
    keep = np.array([min_separation(p, L) > 1e-3 for p in pos])
    assert keep.sum() >= 3, 'the fixtures hold well-separated configurations'
    return pos, keep


@pytest.mark.parametrize('tag', TAGS)
def test_vmc_first_yield_float_on_golden_configurations(fast_engines,
                                                        golden_kernels, tag):
    """log|psi| from the sorted float log-psi pass (folded products), energy
    from the sorted float energy pass of `vmc_step_kernel`, series and
    production kernel, against the reference's goldens."""
    eng = fast_engines(tag)
    assert eng.fast_math
    L = float(eng.cfc_spec.model_params.supercell_size)
    pos, keep = golden_keep(golden_kernels, tag, L)
    g = golden_kernels
    eng.general_path_walkers(reset=True)
    top = 0.0
    for series in (True, False):
        en, wf = vmc_first_yield(eng, pos, series)
        err = dict(energy=errors(en, g[tag + '/energy']),
                   wf_abs_log=errors(wf, g[tag + '/wf_abs_log']))
        _record('steps_golden', f'{tag}/vmc/{"series" if series else "lean"}',
                summary(err, keep))
        check_float_rows((tag, 'vmc', series), err, keep)
        top = max(top, max(e.max() for e in err.values()))
    assert eng.general_path_walkers() == 0, 'a golden row left the sorted path'
    # a different computation, not a relabelled double path
    assert top > 1e-10


@pytest.mark.parametrize('tag', TAGS)
def test_dmc_zero_move_step_float_on_golden_configurations(fast_engines,
                                                           golden_kernels,
                                                           tag):
    """Energy and drift from the sorted float energy + drift pass of
    `dmc_evolve_kernel` (cotangent / tangent quotients) against the goldens."""
    eng = fast_engines(tag)
    assert eng.fast_math
    L = float(eng.cfc_spec.model_params.supercell_size)
    pos, keep = golden_keep(golden_kernels, tag, L)
    g = golden_kernels
    eng.general_path_walkers(reset=True)
    en, dr = dmc_zero_move_step(eng, pos)
    assert eng.general_path_walkers() == 0, 'a golden row left the sorted path'
    err = dict(energy=errors(en, g[tag + '/energy']),
               drift=errors(dr, g[tag + '/ith_drift'], drift=True))
    _record('steps_golden', f'{tag}/dmc', summary(err, keep))
    check_float_rows((tag, 'dmc'), err, keep)
    assert max(e.max() for e in err.values()) > 1e-10


# ---------------------------------------------------------------------------
# 2. the poles, across random models
# ---------------------------------------------------------------------------

def test_sorted_float_paths_random_specs_vs_oracle(oracle):
    """The reduced float counterpart of
    `test_sorted_paths_random_specs_vs_oracle`: the same model generator and
    sizes, a seed of its own, rows 0-3 only -- two plain rows (a jittered
    lattice, one of them permuted) and two rows with particles ON and one ulp
    above the poles of tan(k2 z - phi), tan(k2 z) and at z = 1e-9, which is
    what the +-1e18 clamp of the quotients and the folded products exist for.
    VMC first yield and zero-move DMC step against the oracle; the plain rows
    at TOL_* for energy, log|psi| and drift, the pole rows at TOL_* for
    energy and log|psi| (their drift is recorded)."""
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    rng = np.random.RandomState(20261018)
    sizes = [33, 37, 48, 63, 64, 66, 100, 126, 128]
    count = int(os.environ.get('QMC_FUZZ_SPECS_F32', 18))
    done = tried = 0
    plain = np.array([True, True, False, False])
    top = dict(plain={}, pole={})
    while done < count:
        tried += 1
        assert tried < 20 * count
        n = sizes[done % len(sizes)]
        L = float(np.round(n * rng.uniform(0.6, 1.6), 3))
        kw = dict(lattice_depth=float(rng.choice([0.0, rng.uniform(1, 120)])),
                  lattice_ratio=float(np.round(rng.uniform(0.2, 3.0), 3)),
                  interaction_strength=float(10 ** rng.uniform(-1, 1.5)),
                  boson_number=n, supercell_size=L,
                  tbf_contact_cutoff=float(L * rng.uniform(0.02, 0.44)))
        try:
            spec = Spec(**kw)
            cfc = spec.cfc_spec
        except ValueError:
            continue
        m = oracle.model_from_cfc(cfc)
        eng = ModelEngine(cfc, fast_math=True)
        assert eng.fast_math, kw
        pos = jittered_rows(rng, 4, n, L)
        pos[0] = rng.permutation(pos[0])
        k2, phi = float(cfc.tbf_params.param_k2), \
            float(cfc.tbf_params.param_k2 * cfc.tbf_params.param_r_off)
        # (next to the pole of cot(pi z / L), not AT 0: see the double test)
        for i, zp in enumerate([(0.5 * pi + phi) / k2, 0.5 * pi / k2,
                                (0.5 * pi + phi) / k2 - L, 1e-9]):
            if 0.0 <= zp < L:
                pos[2, i] = zp
                pos[3, i] = np.nextafter(zp, L)
        wf, en, ie, fd = oracle.evaluate_set(m, pos)
        eng.general_path_walkers(reset=True)
        err = {}
        en_v, wf_v = vmc_first_yield(eng, pos, True, spread=0.1)
        err['vmc energy'] = errors(en_v, en)
        err['vmc wf'] = errors(wf_v, wf)
        en_d, dr_d = dmc_zero_move_step(eng, pos)
        err['dmc energy'] = errors(en_d, en)
        err['dmc drift'] = errors(dr_d, fd, drift=True)
        # (spread rows: the sorted-row path is certain to take them)
        assert eng.general_path_walkers() == 0, kw
        eng.close()
        for name, e in err.items():
            assert np.all(np.isfinite(e)), (kw, name, e)
            top['plain'][name] = max(top['plain'].get(name, 0.0),
                                     float(e[plain].max()))
            top['pole'][name] = max(top['pole'].get(name, 0.0),
                                    float(e[~plain].max()))
        _record('steps_pole_rows', 'worst_over_models',
                dict(models=done + 1, plain_rows=top['plain'],
                     pole_rows=top['pole']))
        print(n, {k: [f'{x:.1e}' for x in v] for k, v in err.items()})
        tol = {'vmc energy': TOL_ENERGY, 'vmc wf': TOL_WF,
               'dmc energy': TOL_ENERGY, 'dmc drift': TOL_DRIFT}
        for name, e in err.items():
            assert e[plain].max() <= tol[name], (kw, name, e)
            if name != 'dmc drift':
                assert e[~plain].max() <= tol[name], (kw, name, 'pole', e)
        done += 1
    print(f'{done} models ({tried} drawn); worst deviation / tolerance scale:',
          top)


# ---------------------------------------------------------------------------
# 3. real steps on Philox streams
# ---------------------------------------------------------------------------

# Philox seeds of the VMC chains, chosen with the oracle alone (see the test)
VMC_SEEDS = {'box64': 33, 'box100': 2738}
VMC_STEPS = 8


def oracle_chain_with_margins(oracle, m, pos0, spread, seed, chain, nsteps):
    """The oracle chain over its initial yield and `nsteps` Metropolis steps
    -> (wf, energy, move_stat, margin, scale) [nsteps + 1]: margin[t] =
    log u - 2 (log|psi'| - log|psi|) of the step that made yield t (inf for
    the initial yield), rebuilt from the shared move stream (word 0 of
    particle i's block moves it, the second words of particles 0 and 1 are
    the accept draw: tests/_traj.py), scale[t] = max(1, |log psi|) before
    that step."""
    n, L = int(m.boson_number), float(m.supercell_size)
    ch = oracle.VmcChain(m, pos0, spread, seed=seed, chain=chain)
    wf, en, st = [list(x) for x in ch.run(1)[:3]]
    margin, scale = [np.inf], [1.0]
    for _ in range(nsteps):
        step = int(ch.cfg.step0)
        w = [oracle.vmc_move_block(seed, chain, step, i) for i in range(n)]
        d = np.array([oracle.vmc_move_unit(w0) for w0, _ in w]) * spread
        wf_new = oracle.wf_abs_log(m, np.mod(ch.pos + d, L))
        ua = oracle.vmc_accept_uniform(w[0][1], w[min(1, n - 1)][1])
        margin.append(float(np.log(ua) - 2.0 * (wf_new - ch.wf[0])))
        scale.append(max(1.0, abs(float(ch.wf[0]))))
        a, b, c, _ = ch.run(1)
        assert bool(c[0]) == (margin[-1] < 0.0)     # the rebuilt test IS the
        wf.append(a[0]); en.append(b[0]); st.append(c[0])   # oracle's
    return (np.array(wf), np.array(en), np.array(st, dtype=bool),
            np.array(margin), np.array(scale))


@pytest.mark.parametrize('tag', ['box64', 'box100'])
def test_vmc_float_steps_follow_the_oracle(fast_engines, oracle, golden_params,
                                           tag):
    """64 chains from jittered-lattice rows, the initial yield and 8
    Metropolis steps in float against the fp64 oracle on the same Philox
    streams, step by step: equal move status, energy and log|psi| within
    TOL_*.  A float accept decision may differ only where the oracle's own
    margin |log u - 2 dlog psi| is below 2 TOL_WF max(1, |log psi|); a chain
    is dropped from its first such step on, and at most 5 % of the
    chain-steps may be dropped.  |log psi| is ~930 (N = 64) and ~2600
    (N = 100), so that window is 0.04 / 0.1 wide and an arbitrary seed drops
    more than that: measured with the oracle alone, 6.3 % on average over the
    Philox seeds 1-39 at N = 64 (1.4 % - 13.7 %; 12 of 39 seeds below 5 %)
    and 13.6 % over 1746 seeds at N = 100 (2.7 % - 26.8 %; 3 seeds below
    5 %).  The seeds used here (VMC_SEEDS, picked by that share, which no
    device result enters) drop 1.4 % (box64) and 2.7 % (box100); the test
    asserts the share from the oracle's numbers."""
    from phd_qmclib_amd.engine import VmcEnsemble
    from .conftest import oracle_model
    eng = fast_engines(tag)
    assert eng.fast_math
    m = oracle_model(oracle, golden_params, tag)
    n, L = int(m.boson_number), float(m.supercell_size)
    W, spread, seed = 64, 0.125, VMC_SEEDS[tag]
    ny = VMC_STEPS + 1
    pos0 = jittered_rows(np.random.RandomState(20261018), W, n, L)
    eng.general_path_walkers(reset=True)
    v = VmcEnsemble(eng, W, spread, rng_seed=seed)
    v.set_state(pos0)
    out = v.run_block(ny, series=True)
    v.close()
    left_sorted = eng.general_path_walkers()
    dropped = 0
    top = dict(energy=0.0, wf_abs_log=0.0)
    for c in range(W):
        wf, en, st, mg, sc = oracle_chain_with_margins(oracle, m, pos0[c],
                                                       spread, seed, c,
                                                       VMC_STEPS)
        marginal = np.nonzero(np.abs(mg) < 2.0 * TOL_WF * sc)[0]
        stop = int(marginal[0]) if marginal.size else ny
        dropped += ny - stop
        assert np.array_equal(out['move_stat'][:stop, c], st[:stop]), \
            (c, out['move_stat'][:, c], st, mg)
        e_en = errors(out['energy'][:stop, c], en[:stop])
        e_wf = errors(out['wf_abs_log'][:stop, c], wf[:stop])
        top['energy'] = max(top['energy'], float(e_en.max()))
        top['wf_abs_log'] = max(top['wf_abs_log'], float(e_wf.max()))
        assert e_en.max() <= TOL_ENERGY, (c, e_en)
        assert e_wf.max() <= TOL_WF, (c, e_wf)
    share = dropped / (W * VMC_STEPS)
    _record('steps_real_step', f'{tag}/vmc',
            dict(top, dropped_share=share, general_path_walkers=left_sorted,
                 note=f'{W} chains x {VMC_STEPS} steps, Philox seed {seed}'))
    assert share <= 0.05, share
    assert top['wf_abs_log'] > 1e-10       # the float loop was measured


# seeds of the DMC populations: on the oracle no branching draw of the two
# steps lies within 1e-4 of an integer boundary of its walker's weight
DMC_SEEDS = {'box64': 5, 'box100': 5}


@pytest.mark.parametrize('tag', ['box64', 'box100'])
def test_dmc_float_steps_follow_the_oracle(fast_engines, oracle, golden_params,
                                           tag):
    """64 walkers (max 96), time_step 1e-3, two real steps in float against
    the Philox oracle: walker counts and cloning table equal, the yielded
    positions within 2 dt TOL_DRIFT max|F| + 4 ulp of L (minimum image),
    energies within TOL_ENERGY.  Equal counts are a fair demand: the test
    first establishes from the oracle's weights and draws that no walker's
    int(w + u) is within 1e-4 of changing (a float energy moves w by
    dt TOL_ENERGY |E| ~ 4e-5 at most)."""
    from phd_qmclib_amd.engine import DmcEnsemble
    from .conftest import oracle_model
    eng = fast_engines(tag)
    assert eng.fast_math
    m = oracle_model(oracle, golden_params, tag)
    n, L = int(m.boson_number), float(m.supercell_size)
    W, maxw, dt, seed = 64, 96, 1e-3, DMC_SEEDS[tag]
    pos0 = jittered_rows(np.random.RandomState(20261019), W, n, L)
    orc = oracle.DmcEnsemble(m, pos0, dt, maxw, W, 0.5, seed=seed)
    fmax = np.abs(orc.ini_confs[:W, 1]).max(1)          # per initial walker
    ys, weights = [], [np.ones(W)]
    ys.append(orc.step())
    # (the weights the second branching reads: written by the first step into
    # the oracle's `next` buffers, which the C side then made its `prev`)
    weights.append(orc.bufs['next_weight'][:ys[0].num_walkers].copy())
    ys.append(orc.step())
    for t, w in enumerate(weights):
        u = np.array([oracle.philox_uniform2(seed, s, t, 0,
                                             STREAM_DMC_BRANCH)[0]
                      for s in range(len(w))])
        x = w + u
        assert np.abs(x - np.round(x)).min() > 1e-4, (t, 'a marginal draw')
        assert int(np.floor(x).sum()) == ys[t].num_walkers < maxw
    eng.general_path_walkers(reset=True)
    d = DmcEnsemble(eng, dt, maxw, W, 0.5, rng_seed=seed)
    d.set_state(pos0)
    ser = d.run_block(2)
    st = d.get_state()
    d.close()
    left_sorted = eng.general_path_walkers()
    for t in range(2):
        assert int(ser.num_walkers[t]) == ys[t].num_walkers, t
        assert close(ser.energy[t], ys[t].energy, TOL_ENERGY), t
    nw = ys[1].num_walkers
    assert st.num_walkers == nw
    assert np.array_equal(st.cloning_ref[:nw], orc.cloning_ref[:nw])
    # the yielded walkers: the children of the first step's walkers (moved
    # once, by the drift of the initial configurations), energy and drift from
    # the evolve kernel's float pass
    par = orc.cloning_ref[:nw]
    dz = np.abs(st.confs[:nw, 0] - orc.confs[:nw, 0])
    dz = np.minimum(dz, L - dz)
    bound = 2 * dt * TOL_DRIFT * fmax[par] + 4 * np.spacing(L)
    e_en = errors(st.energy[:nw], orc.energy[:nw])
    e_dr = errors(st.confs[:nw, 1], orc.confs[:nw, 1], drift=True)
    _record('steps_real_step', f'{tag}/dmc',
            dict(energy=float(e_en.max()), drift=float(e_dr.max()),
                 pos_abs=float(dz.max()),
                 pos_of_bound=float((dz.max(1) / bound).max()),
                 general_path_walkers=left_sorted,
                 note=f'{W} walkers, 2 steps of {dt}, seed {seed}'))
    assert np.all(dz.max(1) <= bound), (dz.max(1) / bound).max()
    assert e_en.max() <= TOL_ENERGY, e_en
    assert max(e_en.max(), e_dr.max()) > 1e-10     # the float loop was measured


# ---------------------------------------------------------------------------
# 4. where the variant does not exist
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['ideal', 'zclass'])
def test_fast_math_is_a_no_op_at_n64_where_the_variant_does_not_exist(oracle,
                                                                       kind):
    """N = 64, one wavefront per walker, but no float instantiation: an ideal
    gas, and a cutoff above 0.45 L (pairs classified from positions,
    `has_fast` / `qmc_engine_set_fast_math` in qmcwalk.hip).  The request is
    a no-op and the first yield is the double path's, 2e-11."""
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    n = 64
    kw = dict(lattice_depth=5 * pi ** 2, lattice_ratio=1, boson_number=n,
              supercell_size=n)
    if kind == 'ideal':
        spec = Spec(interaction_strength=0, tbf_contact_cutoff=0.25 * n, **kw)
    else:
        spec = Spec(interaction_strength=2, tbf_contact_cutoff=0.47 * n, **kw)
    cfc = spec.cfc_spec
    eng = ModelEngine(cfc, fast_math=True)
    assert not eng.fast_math
    m = oracle.model_from_cfc(cfc)
    pos = jittered_rows(np.random.RandomState(64), 6, n, float(n))
    wf, en, _, _ = oracle.evaluate_set(m, pos)
    for series in (True, False):
        en_v, wf_v = vmc_first_yield(eng, pos, series)
        assert close(en_v, en, RTOL64), (kind, series, worst(en_v, en))
        assert close(wf_v, wf, RTOL64), (kind, series, worst(wf_v, wf))
    eng.close()


def test_float_general_pair_sum_inside_the_steps_n130(oracle):
    """N = 130: four particles per lane, padded -- every walker takes the
    general pair sum, in float, inside the step kernels (no demand on the
    sorted-path counter).  First yield and zero-move step against the
    oracle."""
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    n = 130
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=n, supercell_size=n,
                tbf_contact_cutoff=0.25 * n)
    cfc = spec.cfc_spec
    eng = ModelEngine(cfc, fast_math=True)
    assert eng.fast_math
    m = oracle.model_from_cfc(cfc)
    pos = jittered_rows(np.random.RandomState(130), 6, n, float(n))
    keep = np.ones(6, dtype=bool)
    wf, en, _, fd = oracle.evaluate_set(m, pos)
    top = 0.0
    for series in (True, False):
        en_v, wf_v = vmc_first_yield(eng, pos, series)
        err = dict(energy=errors(en_v, en), wf_abs_log=errors(wf_v, wf))
        _record('steps_golden', f'n130/vmc/{"series" if series else "lean"}',
                summary(err, keep))
        check_float_rows(('n130', 'vmc', series), err, keep)
        top = max(top, max(e.max() for e in err.values()))
    en_d, dr_d = dmc_zero_move_step(eng, pos)
    err = dict(energy=errors(en_d, en), drift=errors(dr_d, fd, drift=True))
    _record('steps_golden', 'n130/dmc', summary(err, keep))
    check_float_rows(('n130', 'dmc'), err, keep)
    assert max(top, max(e.max() for e in err.values())) > 1e-10
    eng.close()
