"""The second-order DMC propagator on the device (`propagator='quadratic'`,
`dmc_evolve2_kernel`, csrc/qmc_evolve2.h) against its numpy restatement
(tests/_dmc2_restatement.py: the CPU oracle's energy, drift, normals and
branching draws under the new step), at one N per lane-group shape the
dispatch can pick (tests/_dmc2_cases.py says which N hits which shape), at the
case's own time step and at 8 x that -- larger moves force re-sorts and box
crossings at every one of the three stages.

1. Real steps: 12 walkers (cap 16) from `tests/_steps.dmc_start`, 8 steps;
   the tolerances of `test_dmc_real_steps_follow_the_oracle`: populations and
   cloning table exact, E_t / E_ref at 1e-9 relative, per-walker energy at
   2e-11, positions (minimum image) and drift at 1e-10.  The preconditions --
   no walker within 1e-9 of a decision, so none is left out -- are asserted
   on the restatement (tests/test_dmc2_host.py runs them without a GPU).
2. N = 64, 128 on jittered lattices: all three stages take the sorted rows
   (`general_path_walkers()` is 0 after the block); N = 101: none does.
3. `propagator='linear'` is the ensemble created without the keyword, bit for
   bit; `fix_stale_energy` changes nothing under 'quadratic'; a replay tape
   holds two rows of normals per walker; an unknown name or code is refused.
4. Estimators and distribution ride along: site and one-body density rows of
   a 'quadratic' block, and a world of one of `DistributedDmc`.

Without the feature everything under 'quadratic' fails (the keyword does not
exist).  Every test prints its worst deviation as a fraction of its tolerance
(`-s`).
"""
import numpy as np
import pytest

from . import _dmc2_cases as dc
from . import _generic_cases as gc
from . import _site_restatement as sr
from ._steps import DMC_KAPPA, DMC_MAXW, DMC_STEPS, DMC_W, report
from .test_gpu_parity import worst

pytestmark = pytest.mark.gpu

RTOL = 2e-11                    # the suite's double-path tolerance


def say(part, cid, figures):
    report(part, cid, figures, module='dmc2')


def make_engine(oracle, case, shape=None, monkeypatch=None):
    from phd_qmclib_amd.engine import ModelEngine
    cfc, _ = gc.oracle_model(oracle, case)
    if shape is not None:
        # (read when the engine picks its lane-group shape)
        monkeypatch.setenv('QMCWALK_SHAPE', shape)
    return ModelEngine(cfc)


def run_block(eng, pos0, dt, seed, steps=DMC_STEPS, maxw=DMC_MAXW, target=DMC_W,
              **kw):
    """-> (series, state, general-path counter of the block)."""
    from phd_qmclib_amd.engine import DmcEnsemble
    d = DmcEnsemble(eng, dt, maxw, target, DMC_KAPPA, rng_seed=seed, **kw)
    try:
        d.set_state(pos0)
        eng.general_path_walkers(reset=True)
        ser = d.run_block(steps)
        st = d.get_state()
        general = eng.general_path_walkers(reset=True)
    finally:
        d.close()
    return ser, st, general


# ---------------------------------------------------------------------------
# 1. real steps against the restatement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('mult', dc.MULTS)
@pytest.mark.parametrize('cid', dc.IDS)
def test_quadratic_steps_follow_the_restatement(oracle, monkeypatch, cid, mult):
    ref = dc.preconditions(oracle, cid, mult)
    case, L = ref.case, ref.case[2]
    n = case[1]
    eng = make_engine(oracle, case, ref.shape, monkeypatch)
    try:
        ser, st, general = run_block(eng, ref.pos0, ref.time_step, ref.seed,
                                     propagator='quadratic')
    finally:
        eng.close()
    ys, pop = ref.yields, ref.pop
    dev = dict(E_t=0.0, E_ref=0.0)
    for t, (nw, e_t, e_ref) in enumerate(ys):
        assert int(ser.num_walkers[t]) == nw, t
        dev['E_t'] = max(dev['E_t'], worst(ser.energy[t], e_t) / 1e-9)
        dev['E_ref'] = max(dev['E_ref'],
                           worst(ser.ref_energy[t], e_ref) / 1e-9)
    nw = ys[-1][0]
    z_o, f_o = pop.confs[:nw, 0], pop.confs[:nw, 1]
    dz = np.abs(st.confs[:nw, 0] - z_o)
    dz = np.minimum(dz, L - dz)
    dev['energy'] = worst(st.energy[:nw], pop.energy[:nw]) / RTOL
    dev['pos'] = float((dz / np.maximum(1.0, np.abs(z_o))).max()) / 1e-10
    dev['drift'] = worst(st.confs[:nw, 1], f_o) / 1e-10
    say('part1', f'{cid}x{mult}', dict(
        dev, dt=ref.time_step, crossed=pop.crossed, general=general,
        closest_pair=pop.min_pair_margin,
        populations='/'.join(str(y[0]) for y in ys)))
    for t, (nw_t, e_t, e_ref) in enumerate(ys):
        assert ser.energy[t] == pytest.approx(e_t, rel=1e-9), t
        assert ser.ref_energy[t] == pytest.approx(e_ref, rel=1e-9), t
    assert st.num_walkers == nw
    assert np.array_equal(st.cloning_ref[:nw], pop.cloning_ref[:nw])
    assert dev['energy'] <= 1.0 and dev['pos'] <= 1.0 and \
        dev['drift'] <= 1.0, dev
    if n > 64 and n % 2 and n <= 128:
        # no sorted rows at an odd N: three general sums per walker and step
        assert general == 3 * sum(y[0] for y in ys)


# ---------------------------------------------------------------------------
# 2. the three stages take the sorted rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [64, 128])
def test_all_three_stages_take_the_sorted_rows(oracle, n):
    """Jittered lattices on the box: no evaluation of the block leaves the
    sorted-row sums, and the population is the restatement's."""
    case = gc.lean_case('box', n)
    _, m = gc.oracle_model(oracle, case)
    L = case[2]
    pos0 = dc.lattice_rows(n, L, 9100 + n)
    dt = 8 * 5e-4
    from . import _dmc2_restatement as r2
    pop = r2.Population(oracle, m, pos0, dt, DMC_MAXW, DMC_W, DMC_KAPPA, seed=3)
    ys = [pop.step() for _ in range(4)]
    assert pop.branch_margin > dc.MARGIN and pop.min_pair_margin > dc.MARGIN
    eng = make_engine(oracle, case)
    try:
        ser, st, general = run_block(eng, pos0, dt, 3, steps=4,
                                     propagator='quadratic')
    finally:
        eng.close()
    assert general == 0
    nw = ys[-1][0]
    assert [int(x) for x in ser.num_walkers] == [y[0] for y in ys]
    dz = np.abs(st.confs[:nw, 0] - pop.confs[:nw, 0])
    assert np.minimum(dz, L - dz).max() <= 1e-10 * L
    assert worst(st.energy[:nw], pop.energy[:nw]) <= RTOL


# ---------------------------------------------------------------------------
# 3. the switch
# ---------------------------------------------------------------------------

def same_run(a, b):
    (sa, ta, ga), (sb, tb, gb) = a, b
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    assert ta.num_walkers == tb.num_walkers and ga == gb
    for f in ('confs', 'energy', 'weight', 'mask', 'cloning_ref'):
        assert np.array_equal(getattr(ta, f), getattr(tb, f)), f
    assert (ta.state_energy, ta.ref_energy, ta.accum_energy) == \
        (tb.state_energy, tb.ref_energy, tb.accum_energy)


@pytest.mark.parametrize('cid', ['dilute16', 'offlat64', 'hard100'])
def test_linear_is_the_default_and_stale_energy_is_ignored(oracle, cid):
    """'linear' = no keyword, bit for bit (series and state), with either
    `fix_stale_energy`; 'quadratic' does not depend on `fix_stale_energy`, and
    differs from 'linear'."""
    ref = dc.preconditions(oracle, cid, 1)
    eng = make_engine(oracle, ref.case)
    try:
        args = (eng, ref.pos0, ref.time_step, ref.seed)
        for fix in (False, True):
            same_run(run_block(*args, fix_stale_energy=fix),
                     run_block(*args, fix_stale_energy=fix,
                               propagator='linear'))
        quad = run_block(*args, propagator='quadratic')
        same_run(quad, run_block(*args, propagator='quadratic',
                                 fix_stale_energy=True))
        lin = run_block(*args)
        assert not np.array_equal(quad[1].confs, lin[1].confs)
    finally:
        eng.close()


def test_tape_holds_two_rows_of_normals_per_walker(oracle):
    """Tape mode: a step's normals are [slot][2][N], the xi1 row, then the
    xi2 row.  A tape of the restatement's draws (the oracle's normals and
    branching uniforms) under ANOTHER Philox seed on the device gives the
    restatement's population, at the tolerances of part 1."""
    from phd_qmclib_amd.engine import DmcEnsemble
    from . import _dmc2_restatement as r2
    cid = 'offlat37'
    ref = dc.preconditions(oracle, cid, 1)
    n, L = ref.case[1], ref.case[2]
    u, g, n_u, n_g = [], [], [], []
    parents = DMC_W
    for t, (nw, _, _) in enumerate(ref.yields):
        u += [oracle.philox_uniform2(ref.seed, s, t, 0, r2.STREAM_DMC_BRANCH)[0]
              for s in range(parents)]
        for s in range(nw):
            g += list(r2.normals(oracle, ref.seed, s, t, n))
        n_u.append(parents)
        n_g.append(2 * nw * n)
        parents = nw
    u, g = np.array(u), np.concatenate(g)
    u_off = np.concatenate([[0], np.cumsum(n_u)[:-1]])
    g_off = np.concatenate([[0], np.cumsum(n_g)[:-1]])
    eng = make_engine(oracle, ref.case)
    d = DmcEnsemble(eng, ref.time_step, DMC_MAXW, DMC_W, DMC_KAPPA,
                    rng_seed=ref.seed + 1000, propagator='quadratic')
    try:
        d.set_state(ref.pos0)
        d.set_tape(u, g, u_off, g_off)
        ser = d.run_block(DMC_STEPS)
        st = d.get_state()
    finally:
        d.close()
        eng.close()
    pop = ref.pop
    for t, (nw, e_t, e_ref) in enumerate(ref.yields):
        assert int(ser.num_walkers[t]) == nw, t
        assert ser.energy[t] == pytest.approx(e_t, rel=1e-9), t
        assert ser.ref_energy[t] == pytest.approx(e_ref, rel=1e-9), t
    nw = ref.yields[-1][0]
    assert np.array_equal(st.cloning_ref[:nw], pop.cloning_ref[:nw])
    dz = np.abs(st.confs[:nw, 0] - pop.confs[:nw, 0])
    assert np.minimum(dz, L - dz).max() <= 1e-10 * max(1.0, L)
    assert worst(st.energy[:nw], pop.energy[:nw]) <= RTOL
    assert worst(st.confs[:nw, 1], pop.confs[:nw, 1]) <= 1e-10


def test_unknown_propagators_are_refused(oracle):
    import ctypes as C
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import DmcParams, QmcError, check
    from phd_qmclib_amd.engine import DmcEnsemble
    ref = dc.preconditions(oracle, 'dilute16', 1)
    eng = make_engine(oracle, ref.case)
    try:
        for bad in ('cubic', 'Linear', None, 1):
            with pytest.raises(ValueError, match='propagator'):
                DmcEnsemble(eng, 1e-3, 16, 12, 0.5, rng_seed=1, propagator=bad)
        # the C ABI refuses a code it does not know, with a message
        for code in (2, -1):
            p = DmcParams(16, 12, 1e-3, 0.5, 1, 0, 0, 0, code)
            h = C.c_void_p()
            with pytest.raises(QmcError, match='propagator'):
                check(_lib.load().qmc_dmc_create(eng._h, C.byref(p),
                                                 C.byref(h)))
            assert not h.value
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# 4. estimators and distribution ride along
# ---------------------------------------------------------------------------

EST_N, EST_W, EST_MAXW, EST_T, EST_DT = 16, 64, 96, 16, 4e-3
SITE_P, SITE_D = 4, 9
SHIFTS = (0.0, 0.5, 1.0, 3.25)


def est_ensemble(eng, **kw):
    from phd_qmclib_amd.engine import DmcEnsemble
    d = DmcEnsemble(eng, EST_DT, EST_MAXW, EST_W, 0.5, rng_seed=11,
                    propagator='quadratic', **kw)
    L = float(EST_N)
    d.set_state(L * np.random.RandomState(77).random_sample((EST_W, EST_N)))
    return d


def test_site_and_obdm_rows_of_a_quadratic_block(oracle):
    """N = 16, 64 walkers, two blocks of 16 steps with the site and the
    one-body density estimators on: the zero-shift g1 row is num_walkers
    exactly, the occupation rows sum to sites x walkers, and the site rows
    are tests/_site_restatement.py on the configurations a second ensemble of
    the same seed yields step by step."""
    case = gc.lean_case('box', EST_N)
    S = case[2]
    half_zb = sr.half_barrier(1)
    eng = make_engine(oracle, case)
    a, b = est_ensemble(eng), est_ensemble(eng)
    try:
        b.set_site_estimator(SITE_P, SITE_D, pure=False)
        b.set_obdm_estimator(SHIFTS, 1)
        for blk in range(2):
            steps = []
            for _ in range(EST_T):
                a.run_block(1)
                s = a.get_state()
                steps.append((s.confs[:, 0, :].copy(), s.cloning_ref.copy(),
                              int(s.num_walkers)))
            ser, _, _ = b.run_block_est(EST_T)
            nws = np.array([s[2] for s in steps])
            assert np.array_equal(ser.num_walkers.astype(np.int64), nws)
            g1 = b.read_obdm(EST_T)
            assert np.array_equal(g1[:, 0], nws.astype(np.float64))
            assert np.all(g1[:, 1:] > 0)
            rows = b.read_site(EST_T)
            assert np.array_equal(rows[:, :SITE_P].sum(axis=1), S * nws)
            mixed, _, amb = sr.forward_walk(steps, S, half_zb, SITE_P, SITE_D,
                                            1)
            assert amb == []
            assert np.array_equal(rows, mixed), blk
        assert not np.array_equal(nws, np.full(EST_T, EST_W)), 'it branches'
    finally:
        a.close()
        b.close()
        eng.close()


def test_world_of_one_equals_the_plain_ensemble(oracle):
    """`DistributedDmc(..., block_estimators=True)` on one rank around an
    `external_reduce` ensemble with propagator='quadratic': series and
    estimator rows bit-equal to the plain ensemble's."""
    import torch
    from phd_qmclib_amd.dist import DistributedDmc
    from phd_qmclib_amd.engine import ModelEngine
    case = gc.lean_case('box', EST_N)
    cfc, _ = gc.oracle_model(oracle, case)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = ModelEngine(cfc, stream=side.cuda_stream)
        a = est_ensemble(eng)
        b = est_ensemble(eng, external_reduce=True)
        try:
            for h in (a, b):
                h.set_site_estimator(SITE_P, SITE_D, pure=True, pfw=EST_T)
                h.set_obdm_estimator(SHIFTS, 2)
            dd = DistributedDmc(b, EST_N, 'cuda', block_estimators=True)
            for blk in range(2):
                sa, _, _ = a.run_block_est(EST_T)
                sb, _, _ = dd.run_block(EST_T, estimators=True)
                for f in ('energy', 'num_walkers'):
                    assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
                for key, read in (('site', a.read_site), ('obdm', a.read_obdm)):
                    want = read(EST_T)
                    got = dd.read_estimator(key, EST_T)
                    assert got.tobytes() == want.tobytes(), key
                    assert np.abs(got[-2:]).max() > 0, key
            sa, sb = a.get_state(), b.get_state()
            assert np.array_equal(sa.confs, sb.confs)
            assert np.array_equal(sa.energy, sb.energy)
        finally:
            a.close()
            b.close()
            eng.close()
