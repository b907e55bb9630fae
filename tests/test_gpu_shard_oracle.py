"""Sharded DMC against the CPU oracle: the split step (step_local, the global
sum, step_finish), the Philox slot offset of a rank and the walker records the
population rebalance moves between ranks, at the shapes the multi-GPU run
uses.

Two `DmcEnsemble` handles on ONE engine are driven as two ranks of one
population (slot0 = 0 and slot0 = max_num_walkers, one global target, the sum
of the two (E_t, W_t) pairs between step_local and step_finish).  Beside them
run two `OracleShard`s (tests/_dist_worker.py) with the same model, start,
seed, slot offsets, caps, target and initial E_ref.  The oracle's normals and
branching uniforms are pure functions of (seed, slot0 + slot, step, particle
label), so both sides are the same process: populations and W_t must agree
exactly, energies to the 1e-9 relative bound the suite uses for equal-seed
trajectories (test_dmc_large_n_equal_seed_trajectories).

A schedule of transfers (step, source, destination, k) is applied to both
sides: the tail k walkers of the source are exported, the source truncated
(set_num_walkers) and the records imported at the destination's count.  After
the step that follows every import, and at the end, the whole population of
either device shard is exported and compared record by record with the
oracle's: labels a permutation, positions, drift, energy and the weight.  The
weight is what sees the slot energy of the reference's quirk D1
(`eslot`, csrc/qmc_kernels_misc.h unpack_walkers_kernel): with
fix_stale_energy = 0 the step after an import weighs the children that land
in the imported slots with the energy the import left there.  The oracle
stand-in restates that rule (`import_sets_slot_energy`); without it the weight
comparison fails in the D1 parametrisation (see `run_oracle`).

Every schedule moves walkers a -> b before an EVEN step (b's count then
exceeds every count it has had: slots that never held a walker), b -> a
before an ODD step (one particle per lane: the step that consumes the cached
second normal) and a -> b again before an odd step.  The oracle side asserts
that the case fits: no count reaches its cap or drops to zero, every k is at
most the source's count.
"""

import numpy as np
import pytest

from ._dist_worker import OracleShard
from ._models import box

pytestmark = pytest.mark.gpu

DT, KAPPA, SEED = 1e-3, 0.5, 21
RTOL = 1e-9                      # equal-seed trajectories (project bound)
A, B = 0, 1

# name -> N, walkers of shard a / b at the start, local cap, steps, transfers
# (before step, source, destination, k), time step if not DT
CASES = {
    # P = 1 with spare normals, four walkers per wavefront
    'n16_16x1': dict(n=16, start=(150, 60), maxw=256, steps=16,
                     moves=((4, A, B, 50), (9, B, A, 30), (13, A, B, 25))),
    # sorted lanes, spare cache, padded ring
    'n37_64x1_ring': dict(n=37, start=(96, 40), maxw=192, steps=16,
                          moves=((4, A, B, 36), (9, B, A, 21), (13, A, B, 17))),
    'n64_64x1': dict(n=64, start=(96, 40), maxw=192, steps=16,
                     moves=((4, A, B, 36), (9, B, A, 21), (13, A, B, 17))),
    # two particles per lane: no cached normal, sorted rows
    'n100_64x2_ring': dict(n=100, start=(96, 40), maxw=192, steps=16,
                           moves=((4, A, B, 36), (9, B, A, 21),
                                  (13, A, B, 17))),
    'n128_64x2': dict(n=128, start=(96, 40), maxw=192, steps=16,
                      moves=((4, A, B, 36), (9, B, A, 21), (13, A, B, 17))),
    # eight particles per lane, masked.  (dt: in the D1 mode a child in a
    # slot that never held a walker is weighed with a slot energy of zero,
    # exp(dt E / 2) = 9.5 at E = 4500 and dt = 1e-3: the population would run
    # into the cap within two steps)
    'n300_64x8': dict(n=300, start=(24, 12), maxw=64, steps=8, dt=5e-4,
                      moves=((2, A, B, 9), (5, B, A, 6), (7, A, B, 4))),
    # cap > 2048: branch_count / branch_scatter / dmc_local_sums kernels; the
    # moved ranges cross the 1024-walker tile edges (a: 2048, b: 1024)
    'n16_multi_tile': dict(n=16, start=(2600, 900), maxw=4096, steps=10,
                           moves=((4, A, B, 700), (7, B, A, 300),
                                  (9, A, B, 80))),
}
SORTED_ROW_CASES = ('n37_64x1_ring', 'n64_64x1', 'n100_64x2_ring',
                    'n128_64x2')


def start_positions(name):
    """-> positions of shard a, shard b.  N >= 33: spread like equilibrated
    walkers, so that the sorted-row kernels (33 <= N <= 128) take them all
    and the branching weights stay near one."""
    c = CASES[name]
    n = c['n']
    out = []
    for k, nw in enumerate(c['start']):
        rng = np.random.RandomState(1000 * n + k)
        if n >= 33:
            out.append(np.arange(n) + 0.5 +
                       0.5 * (rng.random_sample((nw, n)) - 0.5))
        else:
            out.append(n * rng.random_sample((nw, n)))
    return out


class Trace:
    """What the oracle pair did: series[shard] rows (E_t, W_t, local walkers,
    E_ref, accumulated energy), counts[t] before step t's transfers, and
    snaps[t][shard] = (confs[nw, 2, N], energy[nw], weight[nw]) of the
    population after step t."""

    def __init__(self):
        self.series, self.counts, self.snaps, self.ref0 = None, [], {}, None


_TRACES = {}


def run_oracle(oracle, name, fix, slot_rule=True):
    """The two-shard oracle run of a case (computed once per case and mode).
    `slot_rule=False` leaves the slot energies of imported walkers as they
    were -- NOT what the device does; with fix = False the record weights then
    differ at O(dt) and test_two_shards_follow_the_oracle fails (checked once
    when this module was written, by flipping the default)."""
    key = (name, fix, slot_rule)
    if key in _TRACES:
        return _TRACES[key]
    c = CASES[name]
    n, maxw, steps, dt = c['n'], c['maxw'], c['steps'], c.get('dt', DT)
    m = oracle.model_from_cfc(box(n).cfc_spec)
    pos = start_positions(name)
    target = sum(c['start'])
    nth = min(16, oracle.max_threads())

    def shards(ref):
        return [OracleShard(oracle, m, pos[r], dt, maxw, target, KAPPA,
                            seed=SEED, slot0=r * maxw, ref_energy=ref,
                            fix_stale_energy=fix, nthreads=nth,
                            import_sets_slot_energy=slot_rule)
                for r in (A, B)]

    # one E_ref for all four handles: the mean energy of the union
    e0 = np.concatenate([s.ens.ini_energy[:nw]
                         for s, nw in zip(shards(None), c['start'])])
    tr = Trace()
    tr.ref0 = float(e0.mean())
    sh = shards(tr.ref0)
    part = [np.zeros(2), np.zeros(2)]
    tot = np.zeros(2)
    rec = 3 * n + 2
    grew = False
    seen_b = c['start'][B]
    for t in range(steps):
        cnt = [s.num_walkers() for s in sh]
        tr.counts.append(tuple(cnt))
        moved = False
        for (when, src, dst, k) in c['moves']:
            if when != t:
                continue
            assert 0 < k <= cnt[src], (name, t, 'k exceeds the source', cnt)
            assert cnt[dst] + k < maxw, (name, t, 'import reaches the cap')
            buf = np.zeros((k, rec))
            sh[src].export_walkers(cnt[src] - k, k, buf.ctypes.data)
            sh[src].set_num_walkers(cnt[src] - k)
            sh[dst].import_walkers_at(cnt[dst], k, buf.ctypes.data)
            cnt[src] -= k
            cnt[dst] += k
            if dst == B and cnt[B] > seen_b:
                grew = True
            moved = True
        assert min(cnt) > 0, (name, t, cnt)
        for r in (A, B):
            sh[r].step_local(part[r].ctypes.data)
        tot[:] = part[A] + part[B]
        for r in (A, B):
            sh[r].step_finish(tot.ctypes.data)
        now = [s.num_walkers() for s in sh]
        assert 0 < min(now) and max(now) < maxw, (name, t, now)
        seen_b = max(seen_b, now[B])
        if moved or t == steps - 1:
            snap = []
            for r in (A, B):
                confs, en, wt = sh[r]._pop()
                snap.append((confs[:now[r]].copy(), en[:now[r]].copy(),
                             wt[:now[r]].copy()))
            tr.snaps[t] = snap
    assert grew, (name, 'no import into slots that never held a walker')
    tr.series = [np.array(s.series) for s in sh]
    _TRACES[key] = tr
    return tr


def unpermute(rec, n):
    """Records [count, >= 3N + 2] -> pos[count, N], drift[count, N] in the
    original particle order, energy, log-weight.  The label row of every
    record must be a permutation of 0..N-1."""
    lab = rec[:, 2 * n:3 * n]
    assert np.array_equal(lab, np.rint(lab))
    lab = lab.astype(np.int64)
    assert np.array_equal(np.sort(lab, axis=1),
                          np.broadcast_to(np.arange(n), lab.shape)), \
        'a record label row is not a permutation'
    pos, drift = np.empty_like(rec[:, :n]), np.empty_like(rec[:, :n])
    np.put_along_axis(pos, lab, rec[:, :n], axis=1)
    np.put_along_axis(drift, lab, rec[:, n:2 * n], axis=1)
    return pos, drift, rec[:, 3 * n], rec[:, 3 * n + 1]


def export_all(h, count):
    import torch
    rec = h.walker_record_size()
    buf = torch.zeros(count * rec, dtype=torch.float64, device='cuda')
    h.export_walkers(0, count, buf.data_ptr())
    h.engine.sync()
    return buf.cpu().numpy().reshape(count, rec)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def check_population(h, snap, n, L, where):
    confs, en, wt = snap
    rec = export_all(h, len(en))
    pos, drift, e, logw = unpermute(rec, n)
    d_pos = float(np.abs(pos - confs[:, 0]).max())
    scale = np.abs(confs[:, 1]).max(axis=1, keepdims=True)
    d_drift = float((np.abs(drift - confs[:, 1]) / scale).max())
    d_e, d_w = rel(e, en), rel(np.exp(logw), wt)
    print(where, 'pos %.2e drift %.2e energy %.2e weight %.2e'
          % (d_pos / L, d_drift, d_e, d_w))
    assert d_pos <= RTOL * L, where
    assert d_drift <= RTOL, where
    assert d_e <= RTOL, where
    assert d_w <= RTOL, where


@pytest.mark.parametrize('fix', [False, True], ids=['d1', 'fix_stale'])
@pytest.mark.parametrize('name', list(CASES))
def test_two_shards_follow_the_oracle(oracle, name, fix):
    import torch
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    c = CASES[name]
    n, maxw, steps, dt = c['n'], c['maxw'], c['steps'], c.get('dt', DT)
    tr = run_oracle(oracle, name, fix)
    pos = start_positions(name)
    target = sum(c['start'])
    eng = ModelEngine(box(n).cfc_spec,
                      stream=torch.cuda.current_stream().cuda_stream)
    eng.general_path_walkers(reset=True)
    sh = []
    for r in (A, B):
        d = DmcEnsemble(eng, dt, maxw, target, KAPPA, rng_seed=SEED,
                        slot0=r * maxw, fix_stale_energy=fix,
                        external_reduce=True)
        d.set_state(pos[r], ref_energy=tr.ref0)
        sh.append(d)
    rec = sh[A].walker_record_size()
    assert rec == 3 * n + 2
    part = [torch.zeros(2, dtype=torch.float64, device='cuda')
            for _ in (A, B)]
    tot = torch.zeros(2, dtype=torch.float64, device='cuda')
    keep = []                    # record buffers: alive until the stream is past
    for t in range(steps):
        cnt = list(tr.counts[t])
        assert [d.num_walkers() for d in sh] == cnt, (name, t)
        for (when, src, dst, k) in c['moves']:
            if when != t:
                continue
            buf = torch.zeros(k * rec, dtype=torch.float64, device='cuda')
            keep.append(buf)
            sh[src].export_walkers(cnt[src] - k, k, buf.data_ptr())
            sh[src].set_num_walkers(cnt[src] - k)
            sh[dst].import_walkers_at(cnt[dst], k, buf.data_ptr())
            cnt[src] -= k
            cnt[dst] += k
        for r in (A, B):
            sh[r].step_local(part[r].data_ptr())
        torch.add(part[A], part[B], out=tot)
        for r in (A, B):
            sh[r].step_finish(tot.data_ptr())
        if t in tr.snaps:
            for r in (A, B):
                assert sh[r].num_walkers() == len(tr.snaps[t][r][1]), (name, t)
                check_population(sh[r], tr.snaps[t][r], n, float(n),
                                 '%s step %d shard %d:' % (name, t, r))
    ser = [d.read_series(steps) for d in sh]
    for r in (A, B):
        s, o = ser[r], tr.series[r]
        assert np.array_equal(s.num_walkers.astype(np.int64),
                              o[:, 2].astype(np.int64)), (name, r)
        assert np.array_equal(s.weight, o[:, 1]), (name, r)
        d_e, d_ref, d_acc = (rel(s.energy, o[:, 0]), rel(s.ref_energy, o[:, 3]),
                             rel(s.accum_energy, o[:, 4]))
        print('%s shard %d: E_t %.2e E_ref %.2e accum %.2e'
              % (name, r, d_e, d_ref, d_acc))
        assert d_e <= RTOL and d_ref <= RTOL and d_acc <= RTOL, (name, r)
    assert np.array_equal(ser[A].ref_energy, ser[B].ref_energy)
    assert np.array_equal(ser[A].energy, ser[B].energy)
    if name in SORTED_ROW_CASES:
        assert eng.general_path_walkers() == 0, 'left the sorted-row kernels'
    for h in sh + [eng]:
        h.close()


EST = dict(num_modes=12, ssf_pure=True, ssf_pfw=24, num_bins=16,
           dens_pure=True, dens_pfw=24)


@pytest.mark.parametrize('n', [24, 16])
def test_transit_through_the_other_shard_is_an_identity(n):
    """N = 24 (four walkers per wavefront, two particles per lane) and N = 16
    (one per lane: the returned slots regenerate the second normal the odd
    step would have read from the cache) with PURE S(k) and density rows:
    before an odd and before an even step the tail of shard a travels to
    shard b and straight back, so that every walker is in its original slot
    again before the step.  The free slots of b the guests
    passed through are saved and put back the same way (a pure density row is
    carried by its SLOT, dead or alive), so nothing a later step reads has
    changed: the per-step series, the estimator rows and the final records of
    both shards must be bit-identical to an undisturbed pair.

    This needs fix_stale_energy = True.  In the default (D1) mode an import
    sets the slot energy of the imported slots to the newcomers' own energies
    while an undisturbed slot holds the energy of its previous parent, so the
    round trip changes the next weights at O(dt) and is no identity."""
    import torch
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    maxw, steps, k = 256, 12, 37
    start = (150, 60)
    pos = [n * np.random.RandomState(70 + r).random_sample((start[r], n))
           for r in (A, B)]
    res = []
    for disturb in (False, True):
        eng = ModelEngine(box(n).cfc_spec,
                          stream=torch.cuda.current_stream().cuda_stream)
        sh = []
        for r in (A, B):
            d = DmcEnsemble(eng, DT, maxw, sum(start), KAPPA, rng_seed=SEED,
                            slot0=r * maxw, fix_stale_energy=True,
                            external_reduce=True)
            d.set_estimators(**EST)
            d.set_state(pos[r], ref_energy=14.8 * n)
            d.est_begin_block(steps)
            sh.append(d)
        rec = sh[A].walker_record_size()
        assert rec == 3 * n + 2 + 3 * 12 + 16
        part = [torch.zeros(2, dtype=torch.float64, device='cuda')
                for _ in (A, B)]
        tot = torch.zeros(2, dtype=torch.float64, device='cuda')
        keep = []
        for t in range(steps):
            if disturb and t in (5, 8):
                na, nb = sh[A].num_walkers(), sh[B].num_walkers()
                assert k <= na and nb + k <= maxw
                guests, free, back = (torch.zeros(k * rec, dtype=torch.float64,
                                                  device='cuda')
                                      for _ in range(3))
                keep += [guests, free, back]
                sh[B].export_walkers(nb, k, free.data_ptr())
                sh[A].export_walkers(na - k, k, guests.data_ptr())
                sh[A].set_num_walkers(na - k)
                sh[B].import_walkers_at(nb, k, guests.data_ptr())
                assert (sh[A].num_walkers(), sh[B].num_walkers()) == \
                    (na - k, nb + k)
                sh[B].export_walkers(nb, k, back.data_ptr())
                sh[B].import_walkers_at(nb, k, free.data_ptr())
                sh[B].set_num_walkers(nb)
                sh[A].import_walkers_at(na - k, k, back.data_ptr())
                assert (sh[A].num_walkers(), sh[B].num_walkers()) == (na, nb)
            for r in (A, B):
                sh[r].step_local(part[r].data_ptr())
            torch.add(part[A], part[B], out=tot)
            for r in (A, B):
                sh[r].step_finish(tot.data_ptr())
                sh[r].step_estimators(t)
        out = []
        from phd_qmclib_amd.dist import _wrap_f64
        dev = torch.device('cuda')
        for d in sh:
            ssf_p, dens_p = d.est_iter_dev()
            ser = d.read_series(steps)
            ssf = _wrap_f64(ssf_p, steps * 12 * 3, dev).cpu().numpy().copy()
            dens = _wrap_f64(dens_p, steps * 16, dev).cpu().numpy().copy()
            out.append((ser, ssf, dens, export_all(d, d.num_walkers())))
        res.append(out)
        for h in sh + [eng]:
            h.close()
    for (s0, ssf0, den0, rec0), (s1, ssf1, den1, rec1) in zip(*res):
        for f0, f1 in zip(s0, s1):
            assert np.array_equal(f0, f1)
        assert np.array_equal(ssf0, ssf1)
        assert np.array_equal(den0, den1)
        assert np.array_equal(rec0, rec1)
        assert np.abs(ssf0).max() > 0 and den0.sum() > 0
        unpermute(rec0, n)


def test_walker_record_calls_reject_what_does_not_fit():
    import torch
    from phd_qmclib_amd._lib import QmcError
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine
    n, maxw, nw = 16, 64, 40
    eng = ModelEngine(box(n).cfc_spec,
                      stream=torch.cuda.current_stream().cuda_stream)
    d = DmcEnsemble(eng, DT, maxw, nw, KAPPA, rng_seed=SEED,
                    external_reduce=True)
    assert d.walker_record_size() == 3 * n + 2
    d.set_state(n * np.random.RandomState(5).random_sample((nw, n)))
    before = export_all(d, maxw)
    rec = d.walker_record_size()
    assert rec == 3 * n + 2
    buf = torch.full((maxw * rec,), 7.0, dtype=torch.float64, device='cuda')
    for first, count in ((maxw - 3, 4), (maxw, 1), (-1, 2), (0, maxw + 1)):
        with pytest.raises(QmcError, match='slot range'):
            d.export_walkers(first, count, buf.data_ptr())
        with pytest.raises(QmcError, match='max_num_walkers'):
            d.import_walkers_at(first, count, buf.data_ptr())
    with pytest.raises(QmcError, match='max_num_walkers'):
        d.import_walkers(maxw - nw + 1, buf.data_ptr())
    with pytest.raises(QmcError, match='bad population size'):
        d.truncate(nw + 1)
    with pytest.raises(QmcError, match='bad population size'):
        d.set_num_walkers(maxw + 1)
    eng.sync()
    assert float(buf.min()) == 7.0 == float(buf.max())     # nothing exported
    assert d.num_walkers() == nw
    assert np.array_equal(export_all(d, maxw), before)
    one = torch.zeros(rec, dtype=torch.float64, device='cuda')
    d.export_walkers(nw - 1, 1, one.data_ptr())            # and what does fit
    d.truncate(nw - 1)
    assert d.num_walkers() == nw - 1
    d.import_walkers(1, one.data_ptr())
    assert d.num_walkers() == nw
    assert np.array_equal(export_all(d, maxw), before)
    d.set_estimators(**EST)
    assert d.walker_record_size() == 3 * n + 2 + 3 * 12 + 16
    d.close()
    eng.close()
