"""Renyi-2 entanglement entropy by replica swap: what can be held without a GPU.

* the restatement (tests/_renyi_restatement.py): the cross-pair form the
  kernel evaluates, in NumPy with f2 written out from `tbf_params`, against
  the definition (explicitly swapped configurations through the C oracle's
  wf_abs_log), on box8, box16 and box37;
* the preconditions of the inputs of tests/test_gpu_renyi.py: no particle on a
  cut to within rounding, at least 8 matched and one unmatched (pair, length)
  entry in every pool;
* `engine.renyi_entropy` on hand-made sums, the argument checks that need no
  device, the binding of the four entry points, and the DMC slot table, which
  the estimator leaves alone.
"""
import numpy as np
import pytest

from . import _renyi_restatement as rs
from .conftest import oracle_model


# ---- the restatement ---------------------------------------------------------
def test_membership_by_hand():
    L = 8.0
    pos = np.array([[0.5, 1.5, 7.75, 3.0],
                    [8.5, -6.5, -0.25, 19.0]])       # the same, periods away
    lengths = [1.0, 2.0, 7.5]
    in_a, n_a = rs.membership(pos, L, lengths, 0.0)
    assert in_a.shape == (2, 4, 3) and n_a.dtype == np.int32
    assert n_a.tolist() == [[1, 2, 3], [1, 2, 3]]
    assert in_a[0].tolist() == [[True, True, True], [False, True, True],
                                [False, False, False], [False, False, True]]
    # A = [7.5, 8.75) wraps over the end of the box
    _, n_a = rs.membership(pos, L, [1.25], 7.5)
    assert n_a.tolist() == [[2], [2]]
    _, n_a = rs.membership(pos, L, [1.25], -0.5 - 3 * L)
    assert n_a.tolist() == [[2], [2]]
    # a particle at the origin is inside, one at origin + l is outside
    _, n_a = rs.membership(np.array([[2.0, 3.0]]), L, [1.0], 2.0)
    assert n_a.tolist() == [[1]]
    assert rs.matched(np.array([[1, 2], [1, 3]])).tolist() == [[True, False]]


def test_ambiguous_particles_are_found():
    L = 16.0
    pos = np.array([[1.0, 5.0 + 1e-10, 9.0],
                    [3.0 - 1e-12, 7.5, 12.0]])
    assert rs.ambiguous(pos, L, [2.0], 3.0).tolist() == [[0, 1], [1, 0]]
    assert rs.ambiguous(pos, L, [2.5], 3.5).tolist() == []
    assert rs.ambiguous(pos, L, [4.0, 8.0], 0.0).tolist() == []
    assert rs.ambiguous(pos + 1.0, L, [4.0, 9.5], 0.5).tolist() == [[0, 2]]


def test_swapped_configurations():
    r1, r2 = np.array([0.5, 2.5, 5.0]), np.array([1.0, 6.0, 7.0])
    in1, in2 = r1 < 3.0, r2 < 3.0
    with pytest.raises(AssertionError):
        rs.swapped(r1, r2, in1, in2)
    in1 = r1 < 2.0
    s1, s2 = rs.swapped(r1, r2, in1, in2)
    assert sorted(s1) == [1.0, 2.5, 5.0] and sorted(s2) == [0.5, 6.0, 7.0]
    lr, scale = rs.explicit_log_ratio(lambda z: float(np.sum(z)), r1, r2,
                                      in1, in2)
    assert lr == 0.0 and scale == 2 * (8.0 + 14.0)


@pytest.mark.parametrize('tag', ['box8', 'box16', 'box37'])
def test_cross_pair_form_equals_definition(oracle, golden_params, tag):
    """The two routes agree to 1e-14 of the sum of the |four ln psi terms|
    the explicit one cancels against (measured: 6e-16)."""
    rec = golden_params[tag]
    n = rec['spec']['boson_number']
    L = float(rec['spec']['supercell_size'])
    model = oracle_model(oracle, golden_params, tag)

    def wf(z):
        return oracle.wf_abs_log(model, z)
    worst, entries = 0.0, 0
    for K, origin, lengths, pos in rs.parity_cases(n):
        z = rs.wrap(pos, L)
        in_a, n_a = rs.membership(pos, L, lengths, origin)
        n_ref, lr, scale = rs.reference(wf, pos, L, lengths, origin)
        assert np.array_equal(n_ref, n_a)
        ok = rs.matched(n_a)
        assert np.array_equal(np.isneginf(lr), ~ok)
        for p, k in np.argwhere(ok):
            cross = rs.cross_log_ratio(rec['tbf_params'], L, z[2 * p],
                                       z[2 * p + 1], in_a[2 * p, :, k],
                                       in_a[2 * p + 1, :, k])
            worst = max(worst, abs(cross - lr[p, k]) / scale[p, k])
            entries += 1
    print('%s: %d entries, worst |cross - explicit| / scale = %.2e'
          % (tag, entries, worst))
    assert entries >= 32
    assert worst <= 1e-14


def test_no_interaction_gives_zero():
    """f2 = 1: every cross sum vanishes."""
    tbf = dict(param_am=1.0, param_beta=0.0, param_k2=0.0, param_r_off=8.0,
               tbf_contact_cutoff=4.0)
    rng = np.random.RandomState(3)
    r1, r2 = 16.0 * rng.random_sample((2, 16))
    in1 = r1 < np.sort(r1)[5] + 1e-3
    in2 = r2 < np.sort(r2)[5] + 1e-3
    assert rs.cross_log_ratio(tbf, 16.0, r1, r2, in1, in2) == 0.0


# ---- the inputs of the GPU tests ------------------------------------------------
@pytest.mark.parametrize('n', rs.PARITY_SIZES)
def test_parity_pools_meet_their_conditions(n):
    for K, origin, lengths, pos in rs.parity_cases(n):
        assert len(lengths) == K and pos.shape[0] % 2 == 0
        assert np.any(pos < 0) and np.any(pos >= n)
        assert np.all((lengths > 0) & (lengths < n))
        rs.assert_pool_conditions(pos, float(n), lengths, origin)
    assert min(rs.parity_origins(n)) < 0


def test_other_pools_meet_their_conditions():
    K, origin, lengths, pos = rs.many_lengths_case()
    assert K == len(lengths) == 130 > 64
    rs.assert_pool_conditions(pos, 16.0, lengths, origin)
    K, origin, lengths, pos = rs.large_case()
    assert pos.shape == (8, 512) and K == len(lengths) == 3
    rs.assert_pool_conditions(pos, 512.0, lengths, origin)
    # the run of 2 pairs x 3 lengths has entries of either kind
    _, n_a = rs.membership(rs.large_rows(pos), 512.0, lengths, origin)
    ok = rs.matched(n_a)
    assert ok.shape == (2, 3) and ok[0].all() and not ok[1].all()


def test_known_answer_on_the_restatement():
    """Free particles: swap is the indicator of a match, and its mean the
    probability that two binomial counts agree; the bound of 4 standard
    errors of the GPU test holds on the restatement alone (max |z| = 1.90 on
    the eight cases)."""
    pos = rs.known_answer_inputs()
    k = rs.KNOWN
    want, err = rs.known_answer_expected()
    assert np.all((want > 0.19) & (want < 0.33))
    worst = 0.0
    for origin in k['origins']:
        assert len(rs.ambiguous(pos, k['sc_size'], k['lengths'], origin)) == 0
        _, n_a = rs.membership(pos, k['sc_size'], k['lengths'], origin)
        z = (rs.matched(n_a).mean(axis=0) - want) / err
        worst = max(worst, np.abs(z).max())
    print('known answer on the restatement: max |z| = %.2f' % worst)
    assert worst <= 4.0


# ---- the Python surface -------------------------------------------------------
def test_renyi_entropy_on_hand_made_sums():
    from phd_qmclib_amd import engine
    # four pairs: swap = (1, 0.5, 0, 0.5), three of them matched; and a
    # length nobody matched at
    sums = np.array([[2.0, 1.5, 3.0], [4.0, 4.0, 4.0], [0.0, 0.0, 0.0]])
    s2, err, pm = engine.renyi_entropy(sums, 4)
    assert s2[0] == -np.log(0.5)
    x = np.array([1.0, 0.5, 0.0, 0.5])
    assert np.isclose(err[0], x.std(ddof=1) / 2.0 / x.mean(), rtol=1e-15)
    assert s2[1] == 0.0 and err[1] == 0.0
    assert np.isposinf(s2[2]) and np.isnan(err[2])
    assert pm.tolist() == [0.75, 1.0, 0.0]
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError):
            engine.renyi_entropy(bad, 4)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            engine.renyi_entropy(sums, bad)
    # one pair: no spread to estimate, no division by zero
    s2, err, pm = engine.renyi_entropy(np.array([[1.0, 1.0, 1.0]]), 1)
    assert s2[0] == 0.0 and err[0] == 0.0 and pm[0] == 1.0


def test_argument_errors():
    from phd_qmclib_amd import engine
    L = 16.0
    assert engine.MAX_RENYI_LENGTHS == 4096
    ok = engine.renyi_lengths(L, [1, 2.5, 15.999])
    assert ok.dtype == np.float64 and ok.flags.c_contiguous
    assert ok.tolist() == [1.0, 2.5, 15.999]
    assert engine.renyi_lengths(L, np.full(4096, 1.0)).size == 4096
    assert engine.renyi_lengths(L, 3.0).tolist() == [3.0]     # one length
    for bad in ([], [[1.0, 2.0]], np.full(4097, 1.0), [0.0], [-1.0],
                [16.0], [17.0], [1.0, float('nan')], [float('inf')]):
        with pytest.raises(ValueError):
            engine.renyi_lengths(L, bad)
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError):
            engine._renyi_origin(bad)
    assert engine._renyi_origin(-3) == -3.0
    for bad in (0, 1, 7, -2):
        with pytest.raises(ValueError):
            engine.ModelEngine._num_replicas(bad)
    assert engine.ModelEngine._num_replicas(8) == 8


def test_surface_binding_and_slot_table_unchanged():
    import ctypes as C
    from phd_qmclib_amd import _lib, engine, mrbp_qmc
    from phd_qmclib_amd.qmc_base import dmc_est
    sig = _lib.SIGNATURES
    vp, dp, i32, dbl = _lib._vp, _lib._dp, C.c_int32, C.c_double
    assert sig['qmc_renyi_swap'] == (
        C.c_int, [vp, C.c_int64, dp, i32, dp, dbl, _lib._i32p, dp])
    assert sig['qmc_renyi_swap_dev'] == (
        C.c_int, [vp, C.c_int64, vp, i32, vp, dbl, vp, vp])
    assert sig['qmc_renyi_swap_reduce_dev'] == (
        C.c_int, [vp, C.c_int64, vp, i32, vp, dbl, vp])
    assert sig['qmc_vmc_renyi_swap'] == (C.c_int, [vp, i32, dp, dbl, dp])
    for name in ('renyi_swap', 'renyi_swap_dev', 'renyi_swap_reduce_dev'):
        assert hasattr(engine.ModelEngine, name)
    assert hasattr(engine.VmcEnsemble, 'renyi_parts')
    assert hasattr(mrbp_qmc.vmc.EnsembleSampling, 'renyi_entropy')
    assert hasattr(mrbp_qmc.PhysicalFuncs, 'renyi_swap')
    # no block estimator: the slot table keeps its seven records
    assert len(dmc_est.ESTIMATORS) == 7
    assert all('renyi' not in str(e.key) and 'swap' not in str(e.key)
               for e in dmc_est.ESTIMATORS)
    assert not hasattr(mrbp_qmc.dmc.Sampling, 'renyi_entropy')
