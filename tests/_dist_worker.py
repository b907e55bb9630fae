"""Worker processes of the world_size-2 gloo tests (CPU).  The population
handle is an ORACLE-backed stand-in with the method set of
`engine.DmcEnsemble` -- test infrastructure, never the product path."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class OracleShard:
    """engine.DmcEnsemble look-alike over oracle/qmc_oracle.c."""

    def __init__(self, orc, model, pos, dt, local_max, global_target, kappa,
                 seed, slot0, ref_energy=None, fix_stale_energy=False,
                 nthreads=1, import_sets_slot_energy=False):
        self.orc = orc
        self.n = model.boson_number
        self.maxw = local_max
        self.ens = orc.DmcEnsemble(model, pos, dt, local_max, global_target,
                                   kappa, seed=seed, ref_energy=ref_energy,
                                   slot0=slot0,
                                   fix_stale_energy=fix_stale_energy,
                                   nthreads=nthreads)
        # the device's rule for the slot ("stale") energy of an imported
        # walker (csrc/qmc_kernels_misc.h, unpack_walkers_kernel): off by
        # default, the gloo workers run as they always did
        self.import_sets_slot_energy = import_sets_slot_energy
        # ref_energy=None: build_state used the local mean as E_ref; keep it
        self.dt, self.kappa, self.target = dt, kappa, float(global_target)
        self.series = []
        self._saved = None

    def _view(self, ptr, shape):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(
            C.cast(ptr, C.POINTER(C.c_double)), shape=(n,)).reshape(shape)

    def step_local(self, partial_ptr):
        st = self.ens.st
        self._saved = (st.total_energy, st.total_weight)
        out = self.ens.step()
        self._last = out
        buf = (C.c_double * 2).from_address(partial_ptr)
        buf[0], buf[1] = out.energy, float(out.num_walkers)

    def step_finish(self, total_ptr):
        from math import log
        buf = (C.c_double * 2).from_address(total_ptr)
        e_t, w_t = buf[0], buf[1]
        st = self.ens.st
        st.total_energy = self._saved[0] + e_t
        st.total_weight = self._saved[1] + w_t
        accum = st.total_energy / st.total_weight
        st.ref_energy = accum - self.kappa * log(w_t / self.target) / self.dt
        self.series.append((e_t, w_t, self._last.num_walkers, st.ref_energy,
                            accum))

    def read_series(self, nsteps):
        rows = self.series[:nsteps]
        self.series = self.series[nsteps:]
        return np.array(rows)

    def num_walkers(self):
        return int(self.ens.st.prev_num_walkers)

    def _pop(self):
        st = self.ens.st
        return (self._view(st.prev_confs, (self.maxw, 2, self.n)),
                self._view(st.prev_energy, (self.maxw,)),
                self._view(st.prev_weight, (self.maxw,)))

    def export_walkers(self, first, count, buf_ptr):
        confs, en, wt = self._pop()
        rec = 3 * self.n + 2
        out = self._view(buf_ptr, (count, rec))
        out[:, :self.n] = confs[first:first + count, 0]
        out[:, self.n:2 * self.n] = confs[first:first + count, 1]
        out[:, 2 * self.n:3 * self.n] = np.arange(self.n)     # lane labels
        out[:, 3 * self.n] = en[first:first + count]
        out[:, 3 * self.n + 1] = wt[first:first + count]

    def walker_record_size(self):
        return 3 * self.n + 2

    def import_walkers_at(self, first, count, buf_ptr):
        confs, en, wt = self._pop()
        rec = 3 * self.n + 2
        src = self._view(buf_ptr, (count, rec))
        assert first + count <= self.maxw
        confs[first:first + count, 0] = src[:, :self.n]
        confs[first:first + count, 1] = src[:, self.n:2 * self.n]
        en[first:first + count] = src[:, 3 * self.n]
        wt[first:first + count] = src[:, 3 * self.n + 1]
        if self.import_sets_slot_energy:
            # the slot's previous occupant is gone: the energy quirk D1 reads
            # for this slot becomes the newcomer's own
            self.ens.bufs['actual_energy'][first:first + count] = \
                src[:, 3 * self.n]
        self.ens.st.prev_num_walkers = first + count

    def import_walkers(self, count, buf_ptr):
        self.import_walkers_at(self.num_walkers(), count, buf_ptr)

    def set_num_walkers(self, new_nw):
        assert 0 <= new_nw <= self.maxw
        self.ens.st.prev_num_walkers = new_nw

    def truncate(self, new_nw):
        assert 0 <= new_nw <= self.num_walkers()
        self.set_num_walkers(new_nw)

    def fingerprint(self):
        confs, en, wt = self._pop()
        nw = self.num_walkers()
        return sorted(float(x) for x in en[:nw])


class OracleVmcShard:
    """`vmc.EnsembleSampling` look-alike (attribute `.ensemble` with
    `run_block`) over the oracle's chain ensemble."""

    def __init__(self, orc, model, pos, move_spread, seed, first_chain):
        self.orc, self.model = orc, model
        self.pos = np.array(pos, dtype=np.float64, order='C')     # own copy
        self.wf = np.array([orc.wf_abs_log(model, p) for p in self.pos])
        self.ec = np.zeros(len(self.pos))
        self.spread, self.seed, self.chain0 = move_spread, seed, first_chain
        self.step = 0
        self.ensemble = self

    def run_block(self, ns):
        se, se2, na = self.orc.vmc_ensemble(
            self.model, self.pos, self.wf, self.ec, self.spread, self.seed,
            ns, step0=self.step, yield_initial=self.step == 0,
            chain0=self.chain0, nthreads=1)
        self.step += ns - (1 if self.step == 0 else 0)
        return dict(sum_energy=se, sum_energy2=se2, num_accepted=na)


def main():
    rank, world, port, out_dir = (int(sys.argv[1]), int(sys.argv[2]),
                                  sys.argv[3], sys.argv[4])
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=port,
                      RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from oracle import qmc_oracle as orc
    from phd_qmclib_amd.dist import DistributedDmc
    params = json.load(open(os.path.join(ROOT, 'tests', 'golden',
                                         'params.json')))['box8']
    m = orc.model_from_params(params['params'], params['obf_params'],
                              params['tbf_params'])
    n = m.boson_number
    rng = np.random.RandomState(100 + rank)
    # deliberately unbalanced start: rank 0 gets 3x the walkers of rank 1
    n0 = 36 if rank == 0 else 12
    pos = n * rng.random_sample((n0, n))
    shard = OracleShard(orc, m, pos, 1e-3, 64, 48, 0.5, seed=9,
                        slot0=rank * 64)
    dd = DistributedDmc(shard, n, 'cpu', rebalance_every=4,
                        imbalance_tol=0.0)
    res = dict(rank=rank)
    before = dd.global_counts()
    fp_before = shard.fingerprint()
    moved = dd.rebalance(force=True)
    after = dd.global_counts()
    res.update(counts_before=before, counts_after=after, moved=moved,
               fp_before=fp_before, fp_after=shard.fingerprint())
    ser = dd.run_block(10)
    res.update(series=ser.tolist(), counts_end=dd.global_counts(),
               walkers_moved=dd.walkers_moved)
    # VMC: chains sharded by global index; the global block statistics must
    # not depend on how many ranks hold them
    from phd_qmclib_amd.dist import DistributedVmc
    all_pos = n * np.random.RandomState(55).random_sample((12, n))
    per = 12 // world
    dv = DistributedVmc(
        lambda first: OracleVmcShard(orc, m, all_pos[first:first + per],
                                     0.125, 21, first), per, device='cpu')
    res['vmc'] = [dv.run_block(16), dv.run_block(16)]
    if rank == 0:
        whole = OracleVmcShard(orc, m, all_pos, 0.125, 21, 0)
        tot = []
        for _ in range(2):
            o = whole.run_block(16)
            tot.append(dict(
                energy_mean=float(o['sum_energy'].sum() / (12 * 16)),
                accept_rate=float(o['num_accepted'].sum() / (12 * 16))))
        res['vmc_single'] = tot
    with open(os.path.join(out_dir, f'rank{rank}.json'), 'w') as fp:
        json.dump(res, fp)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
