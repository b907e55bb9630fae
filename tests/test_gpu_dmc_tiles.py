"""The DMC branching step beyond one tile of parents, against exact references.

Which branching kernels run is decided by max_num_walkers alone
(nblocks = ceil(max_num_walkers / 1024), `dmc_fused_branching()` in
csrc/qmcwalk.hip), not by the population:

    max_num_walkers   path
    <= 1024           branch_fused_kernel, one tile (the rest of the suite)
    1025 .. 2048      branch_fused_kernel, two tiles walked serially with
                      block_off
    > 2048            branch_count_kernel + branch_scatter_kernel (tile offsets
                      summed per workgroup, the cap owned by the last tile in
                      use), dmc_finish_kernel summing block_esum, and
                      dmc_local_sums_kernel in split-step runs

Here every row meets a reference of the branching itself:

1. equal-seed trajectories against the CPU oracle (same Philox streams)
   through every row, with populations that grow through the tile edges, sit
   on the cap, and have the benchmarked sizes;
2. single branching steps with constructed weights and taped uniforms at the
   tile edges, against the rule itself (tests/_branch_ref.py, pinned to the
   oracle in tests/test_branch_ref.py);
3. the split step (step_local + reduction + step_finish) on the multi-block
   path against the oracle;
4. the S(k) and density estimators, mixed and forward-walking, on a
   population whose cloning table spans tiles, against the oracle's
   estimators.

Discrete quantities (population, cloning table, mask, histogram counts) must
match exactly; energies to the tolerances the suite already uses for
equal-seed runs (1e-9 relative for the series, 2e-11 max(1, |x|) for walker
energies, 1e-10 for configurations).
"""

import numpy as np
import pytest

from . import _branch_ref as br
from ._models import box

pytestmark = pytest.mark.gpu

RTOL = 2e-11
SEED = 7
KAPPA = 0.5


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


def worst(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope='module')
def engines():
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = ModelEngine(box(n).cfc_spec)
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


# ---- 1. equal-seed trajectories ------------------------------------------
# name -> (N, start walkers, target, max_num_walkers, dt, steps, step by step,
#          path and edge)
CASES = {
    'two_fused_tiles_across_1024': (
        8, 900, 1200, 2048, 4e-3, 30, True,
        'nblocks = 2, fused: the population grows from one tile into the '
        'second (900 -> ~1385 -> ~1190), so block_off[1] is in use'),
    'multi_block_across_2048_and_3072': (
        8, 1800, 2600, 4096, 4e-3, 30, True,
        'nblocks = 4, multi-block: two, three and four tiles in use '
        '(1800 -> ~3160 -> ~2590)'),
    'multi_block_on_the_cap': (
        8, 1800, 2600, 3000, 4e-3, 14, True,
        'nblocks = 3, multi-block: the table is cut at max_num_walkers = 3000 '
        'inside the last tile on at least one step, and is below it again'),
    'multi_block_40000_n16': (
        16, 40000, 40000, 42000, 1e-3, 12, False,
        'nblocks = 42, multi-block, 40 tiles in use, N = 16'),
    'multi_block_2p18_n8': (
        8, 1 << 18, 1 << 18, (1 << 18) * 512 // 480, 1e-3, 6, False,
        'nblocks = 274, multi-block: the benchmarked population, 256 tiles '
        '(more tiles than one workgroup has threads)'),
    'multi_block_8192_n64': (
        64, 8192, 8192, 8738, 6.25e-4, 6, False,
        'nblocks = 9, multi-block: the benchmarked shape N = 64'),
    'multi_block_one_tile_of_five': (
        8, 100, 100, 5000, 4e-3, 12, True,
        'nblocks = 5, multi-block with one tile in use and four idle'),
}


def case_positions(n, start):
    return n * np.random.RandomState(SEED).random_sample((start, n))


def check_case_covers_its_edge(name, nw, maxw):
    """On the ORACLE's population series: the case still runs into the edge it
    is here for."""
    nw = np.asarray(nw)
    if name == 'two_fused_tiles_across_1024':
        assert nw.min() < 1024 < nw.max()
    elif name == 'multi_block_across_2048_and_3072':
        assert nw.min() < 2048 and nw.max() > 3072
    elif name == 'multi_block_on_the_cap':
        full = np.nonzero(nw == maxw)[0]
        assert full.size >= 1 and np.any(nw[full[-1] + 1:] < maxw)
    elif name == 'multi_block_one_tile_of_five':
        assert nw.max() <= 1024
    else:
        assert nw.min() > 2048          # three or more tiles in use throughout


def prev_weights(orc):
    """The weights the oracle's next branching step reads."""
    maxw = orc.cfg.max_num_walkers
    w = np.ctypeslib.as_array(orc.st.prev_weight, shape=(maxw,))
    return w[:orc.st.prev_num_walkers].copy()


def branching_margin(oracle, weights, step):
    """(parent, distance) of the oracle's w + u closest to an integer at time
    step `step`: two sides that evaluate the weights with rounding-level
    differences can take different clone counts only where this is at
    rounding level."""
    best = (-1, 1.0)
    for s, w in enumerate(weights):
        x = w + oracle.philox_uniform2(SEED, s, step, 0, 2)[0]
        d = abs(x - round(x))
        if d < best[1]:
            best = (s, d)
    return best


class OracleRun:
    """The oracle ensemble of a case and what it yielded."""

    def __init__(self, oracle, n, start, target, maxw, dt):
        self.oracle = oracle
        self.m = oracle.model_from_cfc(box(n).cfc_spec)
        self.orc = oracle.DmcEnsemble(self.m, case_positions(n, start), dt,
                                      maxw, target, KAPPA, seed=SEED,
                                      nthreads=oracle.max_threads())
        self.yields = []
        self.weights_before = []

    def step(self):
        self.weights_before.append(prev_weights(self.orc))
        o = self.orc.step()
        self.yields.append((o.energy, o.weight, int(o.num_walkers),
                            o.ref_energy, o.accum_energy))
        return self.yields[-1]

    def compare_series(self, ser, t0=0):
        """Device series `ser` against the yields t0, t0 + 1, ...: no step is
        left out."""
        for i in range(len(ser.energy)):
            t = t0 + i
            e, w, nw, ref, acc = self.yields[t]
            if int(ser.num_walkers[i]) != nw:
                s, d = branching_margin(self.oracle, self.weights_before[t], t)
                raise AssertionError(
                    f'step {t}: device population {int(ser.num_walkers[i])}, '
                    f'oracle {nw}; the oracle\'s w + u closest to an integer '
                    f'at this step: parent {s}, distance {d:.3e}')
            assert ser.weight[i] == w, t
            assert close(ser.energy[i], e, 1e-9), (t, ser.energy[i], e)
            assert close(ser.ref_energy[i], ref, 1e-9), (t, ser.ref_energy[i],
                                                         ref)
            assert close(ser.accum_energy[i], acc, 1e-9), t

    def compare_state(self, st, t):
        """The device's yielded state against the oracle's after step t: every
        walker."""
        nw = self.yields[t][2]
        orc = self.orc
        assert st.num_walkers == nw, t
        assert np.array_equal(st.cloning_ref[:nw], orc.cloning_ref[:nw]), \
            (t, int(np.nonzero(st.cloning_ref[:nw] !=
                               orc.cloning_ref[:nw])[0][0]))
        assert not st.mask[:nw].any() and st.mask[nw:].all(), t
        assert np.array_equal(st.weight[:nw], np.ones(nw)), t
        assert close(st.energy[:nw], orc.energy[:nw]), \
            (t, worst(st.energy[:nw], orc.energy[:nw]))
        assert close(st.confs[:nw], orc.confs[:nw], 1e-10), \
            (t, worst(st.confs[:nw], orc.confs[:nw]))


@pytest.mark.parametrize('name', list(CASES))
def test_equal_seed_trajectories_through_every_path(engines, oracle, name):
    """Device and oracle from the same start on the same Philox streams, per
    step: population and W_t exact, E_t / E_ref / accumulated energy to 1e-9;
    cloning table, mask, walker energies and configurations of the yielded
    state (after every step where the case is run step by step, after the
    last step of the one-block run otherwise).  The block of all steps in one
    call gives the series of the step-by-step run bit for bit.

    Path and edge of each case (CASES): two_fused_tiles_across_1024 is the
    only user of the second fused tile (nblocks = 2); every other case runs
    branch_count_kernel / branch_scatter_kernel / dmc_finish_kernel
    (nblocks >= 3) with 1, 2..4, 3 (capped), 9, 40 and 256 tiles in use.

    A clone count int(w + u) can differ between the two sides only where
    w + u is within rounding of an integer; a difference in population is
    reported with the oracle's smallest such distance at that step."""
    from phd_qmclib_amd.engine import DmcEnsemble
    n, start, target, maxw, dt, steps, stepwise, _ = CASES[name]
    assert (br.nblocks(maxw) == 2) == name.startswith('two_fused') and \
        (br.nblocks(maxw) >= 3) == name.startswith('multi_block')
    run = OracleRun(oracle, n, start, target, maxw, dt)
    pos = case_positions(n, start)
    eng = engines(n)
    one = DmcEnsemble(eng, dt, maxw, target, KAPPA, rng_seed=SEED)
    one.set_state(pos)
    if stepwise:
        ser_steps = []
        for t in range(steps):
            run.step()
            ser = one.run_block(1)
            run.compare_series(ser, t)
            run.compare_state(one.get_state(), t)
            ser_steps.append(ser)
        one.close()
    else:
        for t in range(steps):
            run.step()
    check_case_covers_its_edge(name, [y[2] for y in run.yields], maxw)
    blk = DmcEnsemble(eng, dt, maxw, target, KAPPA, rng_seed=SEED)
    blk.set_state(pos)
    ser = blk.run_block(steps)
    run.compare_series(ser)
    run.compare_state(blk.get_state(), steps - 1)
    blk.close()
    if stepwise:
        for k in ser._fields:
            joined = np.concatenate([getattr(s, k) for s in ser_steps])
            assert np.array_equal(getattr(ser, k), joined), k
    else:
        one.close()


# ---- 2. constructed branching edges ----------------------------------------
EDGE_CASES = [(m, p, name) for m, p in br.SHAPES
              for name in br.pattern_names(m, p)]


@pytest.fixture(scope='module')
def parents(engines):
    """Parent states (configurations with their drifts and energies as the
    device computes them) by parent count."""
    from phd_qmclib_amd.engine import DmcEnsemble
    cache = {}

    def get(P):
        if P not in cache:
            d = DmcEnsemble(engines(8), 1e-300, P, P, KAPPA, rng_seed=1)
            d.set_state(8 * np.random.RandomState(P).random_sample((P, 8)))
            cache[P] = d.get_state()
            d.close()
        return cache[P]
    return get


@pytest.mark.parametrize('maxw,nparents,name', EDGE_CASES)
def test_constructed_branching_edges(engines, parents, oracle, maxw, nparents,
                                     name):
    """One branching step (time step 1e-300, zero normals: the children stay
    where their parents are) with constructed weights and taped uniforms,
    against kids = min(floor(w + u), maxw), table = repeat(arange, kids)[:maxw]
    (tests/_branch_ref.py): cloning table and population exact, W_t == n_w,
    |E_t - fsum(E_parent(table))| <= 2 n_w 2^-53 sum |E_parent(table)| (the
    device adds at most maxw products in a fixed order), children at their
    parents' positions with their parents' energies, parents after the cap
    nowhere in the table.

    max_num_walkers 1024: fused, one tile (control: the path the rest of the
    suite covers); 2048: fused, two tiles; 2049: multi-block, 3 tiles; 5000:
    multi-block, 5 tiles.  Parent counts on both sides of the tile edges and
    not multiples of the four parents a thread owns.  Patterns: a tile's last
    parent rich and the next tile's first without children, and the reverse;
    a whole tile without children between productive ones; all children from
    the last parent; the cap inside one parent's children, on and one past
    the first child of a tile, and equal to the total; one parent with weight
    1e6 (compared with the oracle too).

    one_parent_1e300 is DEVICE-DEFINED behaviour: the device clamps a clone
    count to the cap before the conversion (fmin(exp(log w) + u, maxw)), where
    the reference's int() and the oracle's cast overflow (the oracle returns a
    negative population); it is compared with the clamped numpy rule only."""
    from phd_qmclib_amd.engine import DmcEnsemble
    st = parents(nparents)
    P, n = nparents, 8
    w, u = br.pattern(maxw, P, name)
    kids, table = br.branch_reference(w, u, maxw)
    nw = len(table)
    d = DmcEnsemble(engines(n), 1e-300, maxw, P, KAPPA, rng_seed=1)
    d.set_full_state(st.confs[:P], st.energy[:P], w, st.ref_energy)
    d.set_tape(u, np.zeros(nw * n), [0], [0])
    ser = d.run_block(1)
    st2 = d.get_state()
    d.close()
    assert int(ser.num_walkers[0]) == nw and st2.num_walkers == nw
    got = st2.cloning_ref[:nw]
    assert np.array_equal(got, table), \
        ('first difference at slot', int(np.nonzero(got != table)[0][0]))
    assert ser.weight[0] == nw
    assert not st2.mask[:nw].any() and st2.mask[nw:].all()
    e_t, bound = br.energy_sum_and_bound(st.energy, table)
    assert abs(ser.energy[0] - e_t) <= bound, (ser.energy[0] - e_t, bound)
    assert np.abs(st2.confs[:nw, 0] - st.confs[table, 0]).max() <= 1e-250
    assert close(st2.energy[:nw], st.energy[table])
    assert np.array_equal(st2.weight[:nw], np.ones(nw))
    if name == 'one_parent_1e6':
        m = oracle.model_from_cfc(box(n).cfc_spec)
        orc = oracle.DmcEnsemble(m, st.confs[:P, 0], 1e-300, maxw, P, KAPPA,
                                 seed=1, nthreads=oracle.max_threads())
        orc.bufs['prev_weight'][:P] = w
        out = orc.step(np.r_[u, np.zeros(8)], np.zeros(maxw * n))
        assert out.num_walkers == nw
        assert np.array_equal(orc.cloning_ref[:nw], got)
        assert close(ser.energy[0], out.energy, 1e-9)


# ---- 3. split step on the multi-block path ---------------------------------
def test_split_step_on_the_multi_block_path_vs_oracle(oracle):
    """step_local + (identity reduction) + step_finish at max_num_walkers 4096
    (nblocks = 4, multi-block: the one caller of dmc_local_sums_kernel, and
    dmc_finish_kernel fed with the reduced totals) against the oracle, case
    multi_block_across_2048_and_3072; bit-equal to the block run of the same
    case."""
    import torch
    from phd_qmclib_amd.dist import DistributedDmc
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    name = 'multi_block_across_2048_and_3072'
    n, start, target, maxw, dt, steps, _, _ = CASES[name]
    run = OracleRun(oracle, n, start, target, maxw, dt)
    for t in range(steps):
        run.step()
    check_case_covers_its_edge(name, [y[2] for y in run.yields], maxw)
    pos = case_positions(n, start)
    eng = ModelEngine(box(n).cfc_spec,
                      stream=torch.cuda.current_stream().cuda_stream)
    a = DmcEnsemble(eng, dt, maxw, target, KAPPA, rng_seed=SEED)
    b = DmcEnsemble(eng, dt, maxw, target, KAPPA, rng_seed=SEED,
                    external_reduce=True)
    a.set_state(pos)
    b.set_state(pos)
    sa = a.run_block(steps)
    sb = DistributedDmc(b, n, 'cuda').run_block(steps)
    run.compare_series(sb)
    run.compare_state(b.get_state(), steps - 1)
    for k in sa._fields:
        assert np.array_equal(getattr(sa, k), getattr(sb, k)), k
    a.close(); b.close(); eng.close()


# ---- 4. estimators across tiles --------------------------------------------
@pytest.mark.parametrize('kind,pure', [('ssf', False), ('ssf', True),
                                       ('dens', False), ('dens', True)])
def test_estimators_across_tiles_vs_oracle(engines, oracle, kind, pure):
    """S(k) (20 modes) and density (24 bins), mixed and pure with a
    forward-walking length of 3, on the population of case
    multi_block_across_2048_and_3072 (max_num_walkers 4096, nblocks = 4,
    multi-block; 1800 -> ~3160 -> ~2590 walkers: a cloning table that spans
    tiles, and more walkers than the 1024 workgroups of dmc_ssf_mfma_kernel /
    dmc_density_kernel, so several wavefronts of a workgroup have work).
    One burned block and two evaluated blocks of 6 steps.  Reference:
    `oracle.DmcEstimators.step` on the equal-seed oracle ensemble's yielded
    configurations, populations and cloning tables.  S(k) within
    1e-11 max |ref| per step; density equal exactly."""
    from phd_qmclib_amd.engine import DmcEnsemble
    n, start, target, maxw, dt, _, _, _ = \
        CASES['multi_block_across_2048_and_3072']
    nts, nblocks, burn, pfw = 6, 3, 1, 3
    run = OracleRun(oracle, n, start, target, maxw, dt)
    cfg = (20 if kind == 'ssf' else 24, pure, pfw)
    est = oracle.DmcEstimators(float(n), n, maxw, nts,
                               **{kind: cfg})
    ens = DmcEnsemble(engines(n), dt, maxw, target, KAPPA, rng_seed=SEED)
    ens.set_state(case_positions(n, start))
    if kind == 'ssf':
        ens.set_estimators(num_modes=cfg[0], ssf_pure=pure, ssf_pfw=pfw)
    else:
        ens.set_estimators(num_bins=cfg[0], dens_pure=pure, dens_pfw=pfw)
    seen = []
    for b in range(nblocks):
        est.reset_block()
        for t in range(nts):
            _, _, nw, _, _ = run.step()
            if b >= burn:
                est.step(t, run.orc.confs, nw, run.orc.cloning_ref)
        ser, ssf, dens = ens.run_block_est(nts, b >= burn)
        run.compare_series(ser, b * nts)
        seen += [y[2] for y in run.yields[b * nts:]]
        if b < burn:
            continue
        if kind == 'ssf':
            assert dens is None and ssf.shape == est.iter_ssf.shape
            for t in range(nts):
                ref = est.iter_ssf[t]
                err = np.abs(ssf[t] - ref).max() / np.abs(ref).max()
                assert err <= 1e-11, (b, t, err)
        else:
            assert ssf is None and dens.shape == est.iter_density.shape
            for t in range(nts):
                bad = np.nonzero(dens[t] != est.iter_density[t])[0]
                assert bad.size == 0, (b, t, 'bins', bad.tolist(),
                                       dens[t][bad].ravel().tolist(),
                                       est.iter_density[t][bad].ravel()
                                       .tolist())
    ens.close()
    # the evaluated blocks did see a table spanning three tiles
    assert max(seen[burn * nts:]) > 2048
