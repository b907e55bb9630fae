"""Host side of the block estimators of a sharded DMC population: the opt-in
of `DistributedDmc`, `read_estimator` on a stand-in ensemble whose rows live in
host memory, `global_props`, and the slot numbers of the descriptor table
against the names of include/qmcwalk.h.  No GPU."""
import os
import re

import numpy as np
import pytest

from .conftest import ROOT

HEADER_NAMES = {'ss_factor': 'SSF', 'density': 'DENSITY',
                'pair_dist': 'PAIR_DIST', 'cm_diffusion': 'CM_DIFFUSION',
                'isf': 'ISF', 'obdm': 'OBDM', 'site': 'SITE'}


class Standin:
    """What `DistributedDmc` asks of an ensemble, rows in host memory."""

    def __init__(self, nts=4):
        self.obdm_shifts = np.array([0.0, 1.0])
        self.isf_shape = (2, 3)
        self.record_rows = False
        self.begun = []
        self.steps = 0
        self.rows = {5: np.arange(nts * 2, dtype=np.float64) + 1.0,
                     4: np.arange(nts * 6, dtype=np.float64) - 3.0}

    def set_record_rows(self, on):
        self.record_rows = bool(on)

    def est_begin_block(self, nts):
        self.begun.append(nts)

    def step_local(self, ptr):
        pass

    def step_finish(self, ptr):
        self.steps += 1

    def step_estimators(self, t):
        pass

    def est_iter_dev(self):
        return None, None

    def est_rows_dev(self, slot):
        if slot not in self.rows:
            return None, 0
        rows = self.rows[slot]
        return rows.ctypes.data, {5: 2, 4: 6}[slot]

    def read_series(self, nts):
        from phd_qmclib_amd.engine import DmcSeries
        return DmcSeries(np.zeros(nts), np.full(nts, 7.0),
                         np.full(nts, 3, dtype=np.uint64), np.zeros(nts),
                         np.zeros(nts))


def test_an_estimator_is_refused_by_default_and_accepted_with_the_keyword():
    from phd_qmclib_amd.dist import DistributedDmc
    ens = Standin()
    ens.isf_shape = None                # g1 alone
    with pytest.raises(NotImplementedError, match='one-body density') as exc:
        DistributedDmc(ens, 16, 'cpu', solo=True)
    assert 'block_estimators=True' in str(exc.value)
    assert not ens.record_rows
    dd = DistributedDmc(ens, 16, 'cpu', solo=True, block_estimators=True)
    assert dd.block_estimators and ens.record_rows

    class Bare:                         # no set_record_rows: accepted as it is
        obdm_shifts = np.array([0.5])

    DistributedDmc(Bare(), 16, 'cpu', solo=True, block_estimators=True)


def test_every_refusal_names_the_keyword():
    from phd_qmclib_amd.qmc_base import dmc_est
    told = [e for e in dmc_est.ESTIMATORS if e.refusal]
    assert [e.key for e in told] == ['pair_dist', 'cm_diffusion', 'isf',
                                     'obdm', 'site']
    for est in told:
        assert 'single-GPU only' in est.refusal
        assert 'block_estimators=True' in est.refusal


def test_read_estimator_returns_the_rows_of_the_block_just_run():
    from phd_qmclib_amd.dist import DistributedDmc
    ens = Standin()
    dd = DistributedDmc(ens, 16, 'cpu', solo=True, block_estimators=True)
    with pytest.raises(RuntimeError, match='no estimator block has run'):
        dd.read_estimator('obdm', 4)
    with pytest.raises(KeyError, match='no block estimator .*isf.*obdm'):
        dd.read_estimator('g3', 4)
    with pytest.raises(KeyError, match='no block estimator'):
        dd.read_estimator('density', 4)     # (comes back from run_block)
    series, ssf, dens = dd.run_block(4, estimators=True)
    assert ens.begun == [4] and ens.steps == 4 and ssf is None and dens is None
    g1 = dd.read_estimator('obdm', 4)
    assert g1.shape == (4, 2)
    assert np.array_equal(g1.reshape(-1), ens.rows[5])
    f = dd.read_estimator('isf', 3)
    assert f.shape == (3, 2, 3)
    assert np.array_equal(f.reshape(-1), ens.rows[4][:18])
    g1[:] = 0.0                             # a copy, not a view
    assert ens.rows[5][0] == 1.0
    with pytest.raises(ValueError, match='had 4 steps, 5 were asked for'):
        dd.read_estimator('obdm', 5)
    with pytest.raises(RuntimeError, match="'site' estimator is not set"):
        dd.read_estimator('site', 4)
    # a block without estimators leaves nothing to read
    dd.run_block(2)
    with pytest.raises(RuntimeError, match='no estimator block has run'):
        dd.read_estimator('obdm', 2)


def test_global_props_counts_the_walkers_of_all_ranks():
    from phd_qmclib_amd.dist import DistributedDmc
    from phd_qmclib_amd.qmc_base import dmc_est
    series = Standin().read_series(4)
    props = DistributedDmc.global_props(series)
    assert props.num_walkers.dtype == np.uint64
    assert np.array_equal(props.num_walkers, [7, 7, 7, 7])
    assert np.array_equal(series.num_walkers, [3, 3, 3, 3])     # untouched
    assert props.weight is series.weight and props.energy is series.energy
    # the reductions of the table then normalise by the global count
    rows = np.full((4, 2, 3), 14.0)
    assert np.array_equal(dmc_est._isf_reduce(rows, props, 4, False, None)[0],
                          np.full((2, 3), 2.0))


def test_slot_numbers_are_unique_and_those_of_the_header():
    from phd_qmclib_amd.qmc_base import dmc_est
    with open(os.path.join(ROOT, 'include', 'qmcwalk.h')) as f:
        text = f.read()
    ids = dict(re.findall(r'\bQMC_EST_([A-Z_]+)\s*=\s*(\d+)', text))
    count = int(ids.pop('SLOTS'))
    assert sorted(int(v) for v in ids.values()) == list(range(count))
    slots = {e.key: e.slot for e in dmc_est.ESTIMATORS}
    assert set(slots) == set(HEADER_NAMES)
    assert sorted(slots.values()) == list(range(count))
    for key, slot in slots.items():
        assert int(ids[HEADER_NAMES[key]]) == slot, key
    # every estimator read through `read_estimator` knows its row shape
    for est in dmc_est.ESTIMATORS:
        assert (est.enable is None) == (est.ensemble_row_shape is None)
    # the internal enum is held to the header's names at compile time
    with open(os.path.join(ROOT, 'phd_qmclib_amd', 'csrc',
                           'qmcwalk.hip')) as f:
        src = f.read()
    enum = re.search(r'enum \{ (EST_SSF.*?)\s*EST_SLOTS \};', src, re.S)
    assert [s.strip() for s in enum.group(1).split(',') if s.strip()] == \
        ['EST_SSF', 'EST_DENS', 'EST_PD', 'EST_CM', 'EST_ISF', 'EST_OBDM',
         'EST_SITE']
    assert 'EST_SITE == QMC_EST_SITE && EST_SLOTS == QMC_EST_SLOTS' in src
