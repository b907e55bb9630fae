"""The table of walks and the shared checks of tests/_dmc_walks.py, without a
GPU."""
import numpy as np
import pytest

from . import _dmc_walks as walks
from . import (test_gpu_dist_estimators, test_gpu_isf_est, test_gpu_obdm_est,
               test_gpu_pairdist_est, test_gpu_site_est,
               test_gpu_superfluid_est)


def test_every_walk_a_module_refers_to_exists():
    named = set(test_gpu_dist_estimators.SHAPES)
    named |= {s.walk for s in test_gpu_isf_est.SHAPES.values()}
    assert {c.shape for c in test_gpu_isf_est.CASES.values()} <= \
        set(test_gpu_isf_est.SHAPES)
    for mod in (test_gpu_obdm_est, test_gpu_pairdist_est, test_gpu_site_est,
                test_gpu_superfluid_est):
        named |= {case.walk for case in mod.CASES.values()}
    # and the table holds no walk that nobody takes
    assert named == set(walks.WALKS), named ^ set(walks.WALKS)


@pytest.mark.parametrize('name', list(walks.WALKS))
def test_start_positions_fill_the_box(name):
    walk = walks.WALKS[name]
    spec = walks.spec(walk)
    L = float(spec.supercell_size)
    assert spec.boson_number == walk.n
    if walk.golden is None:
        assert L == (walk.n if walk.sites is None else walk.sites)
        assert spec.tbf_contact_cutoff == walk.cut * L
    pos = walks.start_positions(walk)
    assert pos.shape == (walk.nw0, walk.n)
    assert pos.min() >= 0.0 and pos.max() < L
    assert walk.nw0 <= walk.maxw


def test_numerators_give_back_integers_and_refuse_anything_else():
    T, pfw = 6, 3
    ints = np.arange(T * 4, dtype=np.float64).reshape(T, 4)
    for pure in (False, True):
        div = np.minimum(np.arange(T) + 1, pfw if pure else 1)[:, None]
        counts, got_div = walks.numerators(ints / div, T, pfw, pure)
        assert np.array_equal(counts, ints) and np.array_equal(got_div, div)
    rows = ints / np.minimum(np.arange(T) + 1, pfw)[:, None]
    rows[4, 1] += 0.25                          # numerator 17.75
    with pytest.raises(AssertionError):
        walks.numerators(rows, T, pfw, True)
    with pytest.raises(AssertionError):         # thirds are no mixed rows
        walks.numerators(ints / 3.0, T, pfw, False)
