"""One-particle replica swap (purity of the one-body density matrix): what can
be held without a GPU.

* the restatement (tests/_partent_restatement.py): the factorised form the
  kernel evaluates, in NumPy with f2 written out from `tbf_params`, against
  the definition (explicitly swapped configurations through the C oracle's
  wf_abs_log), on box8, box16 and box37;
* the exact cases, and the N = 2 known answer on the restatement alone;
* `engine.particle_entropy` on hand-made sums, the argument checks that need
  no device, the binding of the four entry points, and the DMC slot table,
  which the estimator leaves alone.
"""
import numpy as np
import pytest

from . import _partent_restatement as pe
from .conftest import oracle_model

IDEAL_TBF = dict(param_am=1.0, param_beta=0.0, param_k2=0.0, param_r_off=8.0,
                 tbf_contact_cutoff=4.0)


@pytest.mark.parametrize('tag', ['box8', 'box16', 'box37'])
def test_factorised_form_equals_definition(oracle, golden_params, tag):
    """Element by element within RTOL max(1, scale), scale the sum of the
    |four ln psi terms| the explicit route cancels against."""
    rec = golden_params[tag]
    n = rec['spec']['boson_number']
    L = float(rec['spec']['supercell_size'])
    model = oracle_model(oracle, golden_params, tag)
    pos = pe.pool(n)
    assert pos.shape == (12, n) and np.any(pos < 0) and np.any(pos >= L)
    lr, scale, mean = pe.reference(lambda z: oracle.wf_abs_log(model, z),
                                   pos, L)
    fac = pe.factorised(rec['tbf_params'], L, pos)
    assert fac.shape == lr.shape == (6, n, n)
    ok, worst = pe.within_tolerance(fac, lr, scale)
    print('%s: worst |factorised - explicit| / bound = %.3g' % (tag, worst))
    assert ok
    ok, worst = pe.mean_within_tolerance(pe.mean_of(fac), mean, scale)
    assert ok
    # the scale of the factorised form's own terms never exceeds the explicit
    # one by more than rounding: it is the tighter yardstick
    _, own = pe.factorised(rec['tbf_params'], L, pos, with_scale=True)
    assert np.all(np.abs(fac - lr) <= pe.RTOL * np.maximum(1.0, own))


def test_definition_by_hand():
    r1, r2 = np.array([0.5, 2.5, 5.0]), np.array([1.0, 6.0, 7.0])
    s1, s2 = pe.swapped(r1, r2, 1, 2)
    assert s1.tolist() == [0.5, 7.0, 5.0] and s2.tolist() == [1.0, 6.0, 2.5]
    assert r1.tolist() == [0.5, 2.5, 5.0]
    # a wave function that is a product of one-body factors cancels
    lr, scale = pe.explicit(lambda z: float(np.sum(z)), r1, r2)
    assert lr.shape == (3, 3) and np.all(lr == 0.0)
    assert np.all(scale == 2 * (8.0 + 14.0))
    lr, scale = pe.explicit(lambda z: float(np.sum(z)), r1, r2,
                            elements=[(0, 1), (2, 2)])
    assert lr.tolist() == [0.0, 0.0] and len(scale) == 2


def test_no_interaction_gives_zero_and_one():
    """f2 = 1: every element is exactly 0 and m exactly 1."""
    pos = pe.pool(16)
    lr = pe.factorised(IDEAL_TBF, 16.0, pos)
    assert lr.shape == (6, 16, 16) and np.all(lr == 0.0)
    assert np.all(pe.mean_of(lr) == 1.0)


def test_reorderings_permute_the_matrix(golden_params):
    rec = golden_params['box16']
    pos = pe.pool(16)
    lr = pe.factorised(rec['tbf_params'], 16.0, pos)
    srt, ps, shf, pr = pe.reorderings(pos, 16)
    assert np.all(np.diff(pe.wrap(srt, 16.0), axis=1) >= 0)
    assert not np.array_equal(pr[0], pr[1])
    for rows, perm in ((srt, ps), (shf, pr)):
        got = pe.factorised(rec['tbf_params'], 16.0, rows)
        assert np.allclose(got, pe.permuted(lr, perm), rtol=0, atol=1e-12)
    # the two rows of a pair exchanged: the transpose
    flipped = pos.reshape(-1, 2, 16)[:, ::-1].reshape(-1, 16)
    assert np.allclose(pe.factorised(rec['tbf_params'], 16.0, flipped),
                       lr.transpose(0, 2, 1), rtol=0, atol=1e-12)


def known_model():
    from phd_qmclib_amd.mrbp_qmc import Spec
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), 'golden',
                           'params.json')) as fp:
        args = dict(json.load(fp)['free16']['spec'])
    args['boson_number'] = 2
    return Spec(**args)


def test_known_answer_on_the_restatement():
    """N = 2 without a lattice on a 24 x 24 grid: the mean of m over the 8192
    drawn pairs lies within 4.5 sigma of the exact grid sum, on the
    restatement alone (the drawn sample is inside the bound)."""
    spec = known_model()
    L = float(spec.supercell_size)
    assert spec.is_free and not spec.is_ideal
    em, em2, pos = pe.known_answer(spec.tbf_params, L)
    assert pos.shape == (2 * pe.KNOWN['npair'], 2)
    assert 0.0 < em < 1.0 + 1e-12 and em2 > em * em
    m = pe.mean_of(pe.factorised(spec.tbf_params, L, pos))
    z = pe.known_answer_z(m, em, em2)
    print('known answer on the restatement: E m = %.6f, sigma = %.3g, '
          'z = %.2f' % (em, np.sqrt((em2 - em * em) / pe.KNOWN['npair']), z))
    assert abs(z) <= pe.KNOWN['sigmas'] == 4.5


# ---- the Python surface ------------------------------------------------------
def test_particle_entropy_on_hand_made_sums():
    from phd_qmclib_amd import engine
    m = np.array([1.0, 0.5, 0.25, 0.25])
    sums = np.array([m.sum(), (m ** 2).sum(), 4.0])
    s2, s2_err, purity, purity_err = engine.particle_entropy(sums, 4)
    assert purity == 0.5 and s2 == -np.log(0.5)
    assert np.isclose(purity_err, m.std(ddof=1) / 2.0, rtol=1e-15)
    assert np.isclose(s2_err, purity_err / purity, rtol=1e-15)
    # one pair: no spread to estimate, no division by zero
    assert engine.particle_entropy([1.0, 1.0, 1.0], 1) == (0.0, 0.0, 1.0, 0.0)
    for bad in (np.zeros(2), np.zeros((1, 3)), np.zeros(4)):
        with pytest.raises(ValueError):
            engine.particle_entropy(bad, 4)
    for bad in (0, -2, 1.5, 3):
        with pytest.raises(ValueError):
            engine.particle_entropy(sums, bad)


def test_argument_errors():
    from phd_qmclib_amd import engine, mrbp_qmc
    for bad in (0, 1, 7, -2):
        with pytest.raises(ValueError):
            engine.ModelEngine._num_replicas(bad)
    # (the engine is made on the first device call: none happens here)
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(known_model())
    for bad in (np.zeros((2, 8)), np.zeros((3, 2, 8)), np.zeros((4, 1, 2, 8))):
        with pytest.raises(ValueError):
            pf.particle_swap(bad)


def test_surface_binding_and_slot_table_unchanged():
    import ctypes as C
    from phd_qmclib_amd import _lib, engine, mrbp_qmc
    from phd_qmclib_amd.qmc_base import dmc_est
    sig = _lib.SIGNATURES
    vp, dp = _lib._vp, _lib._dp
    assert sig['qmc_particle_swap'] == (C.c_int, [vp, C.c_int64, dp, dp, dp])
    assert sig['qmc_particle_swap_dev'] == (
        C.c_int, [vp, C.c_int64, vp, vp, vp])
    assert sig['qmc_particle_swap_reduce_dev'] == (
        C.c_int, [vp, C.c_int64, vp, vp])
    assert sig['qmc_vmc_particle_swap'] == (C.c_int, [vp, dp])
    for name in ('particle_swap', 'particle_swap_dev',
                 'particle_swap_reduce_dev'):
        assert hasattr(engine.ModelEngine, name)
    assert hasattr(engine.VmcEnsemble, 'particle_swap_parts')
    assert hasattr(mrbp_qmc.vmc.EnsembleSampling, 'particle_entropy')
    assert hasattr(mrbp_qmc.PhysicalFuncs, 'particle_swap')
    # no block estimator: the slot table keeps its seven records
    assert len(dmc_est.ESTIMATORS) == 7
    assert all('particle_swap' not in str(e.key) and 'purity' not in str(e.key)
               for e in dmc_est.ESTIMATORS)
    assert not hasattr(mrbp_qmc.dmc.Sampling, 'particle_entropy')
