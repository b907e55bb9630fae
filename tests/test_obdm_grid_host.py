"""One-body density matrix on a grid (natural orbitals, condensate fraction):
what can be held without a GPU.

* the restatement (tests/_obdm_grid_restatement.py) against
  `ith_one_body_density` of tests/_obdm_restatement.py (itself anchored on the
  reference's goldens) at the shifts x_c - z_i, element by element;
* the N = 2 known answer on the restatement alone: exact grid sums of E R and
  E R^2, their identities, and the drawn sample inside 4.5 sigma;
* `engine.natural_orbitals` and `engine.momentum_from_matrix` on hand-made
  matrices;
* the argument checks that need no device, the binding of the three entry
  points, and the DMC slot table, which the estimator leaves alone.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from . import _obdm_grid_restatement as og
from . import _partent_restatement as pe
from ._obdm_restatement import ith_one_body_density
from .conftest import GOLDEN, ROOT

RTOL = og.RTOL


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


# ---- 1. the restatement against g1's -------------------------------------------
@pytest.mark.parametrize('tag', ['box8', 'box37'])
@pytest.mark.parametrize('num_points', [5, 16])
def test_restatement_equals_shifted_g1(golden_params, golden_kernels, tag,
                                       num_points):
    p = golden_params[tag]
    L = float(p['params']['supercell_size'])
    pos = np.array(golden_kernels[tag + '/pos'][:3])
    pos[1] += 2.0 * L                        # a row whole periods outside
    nconf, n = pos.shape
    M = num_points
    _, x = og.points(L, M)
    ratio, scale = og.ratios(pos, M, p)
    assert ratio.shape == scale.shape == (nconf, n, M)
    z = og.wrap(pos, L)
    for c in range(nconf):
        shifts = (x[:, None] - z[c][None, :]).reshape(-1)      # [c * n + i]
        ith = ith_one_body_density(z[c:c + 1], shifts, p)[0]
        ref = np.array([[ith[k * n + i, i] for k in range(M)]
                        for i in range(n)])
        assert close(ratio[c], ref), (tag, c)
    # the matrix is the ratios dropped into the particles' rows
    mats, bound = og.conf_matrices(pos, M, p)
    a = og.row_bins(pos, L, M)
    for c in range(nconf):
        want = np.zeros((M, M))
        for i in range(n):
            want[a[c, i]] += ratio[c, i]
        assert np.allclose(mats[c], want, rtol=1e-14, atol=0)
    assert np.all(bound >= 0) and np.all((bound > 0) == (mats > 0))
    # every particle counts once
    assert np.all(np.bincount(a[0], minlength=M) >= 0) and a.max() < M


def test_bins_by_hand():
    L, M = 16.0, 8
    delta, x = og.points(L, M)
    assert delta == 2.0 and x.tolist() == [1, 3, 5, 7, 9, 11, 13, 15]
    pos = np.array([[0.0, 2.0, 3.999, np.nextafter(16.0, 0.0), -0.5, 16.0,
                     33.0]])
    assert og.row_bins(pos, L, M).tolist() == [[0, 1, 1, 7, 7, 0, 0]]
    sums, wsum, bound = og.group_sums(np.arange(5.0)[:, None, None]
                                      * np.ones((5, 2, 2)),
                                      np.ones((5, 2, 2)), 2,
                                      weights=[1, 2, 3, 4, 5])
    assert sums[0, 0, 0] == 0 * 1 + 2 * 3 + 4 * 5 and sums[1, 1, 1] == 2 + 12
    assert wsum.tolist() == [9.0, 6.0] and bound[0, 0, 0] == 9.0


# ---- 2. the known answer: N = 2 without a lattice ---------------------------------
def known_spec():
    from phd_qmclib_amd.mrbp_qmc import Spec
    with open(os.path.join(GOLDEN, 'params.json')) as fp:
        args = dict(json.load(fp)['free16']['spec'])
    args['boson_number'] = 2
    return Spec(**args)


@pytest.fixture(scope='module')
def known():
    from ._models import model_dict
    spec = known_spec()
    L = float(spec.supercell_size)
    assert spec.is_free and not spec.is_ideal
    p = model_dict(spec.cfc_spec)
    em, em2, pos = pe.known_answer(spec.tbf_params, L)
    conf, w = og.known_grid(spec.tbf_params, L)
    return p, L, em, pos, conf, w


def test_known_answer_on_the_restatement(known):
    p, L, em, pos, conf, w = known
    assert pos.shape == (16384, 2) and conf.shape == (576, 2)
    # the drawn configurations come from this very law
    draw = np.random.RandomState(pe.KNOWN['seed']).choice(
        len(conf), size=len(pos), p=w)
    assert np.array_equal(conf[draw], pos)
    for M in (8, 24):
        er, er2 = og.known_moments(conf, w, M, p)
        assert np.abs(er - er.T).max() <= 1e-14
        if M == 24:
            # every particle sits on a cell centre
            assert abs(np.trace(er) - 2.0) <= 1e-14
            k = 0.5 * (er + er.T)
            assert abs(np.sum(k ** 2) / 4.0 - em) <= 1e-12
            lam = np.linalg.eigvalsh(k)
            print('N = 2: Tr rho1^2 = %.14f (swap: %.14f), lambda_max / N = '
                  '%.5f' % (np.sum(k ** 2) / 4.0, em, lam[-1] / 2.0))
            assert em <= lam[-1] / 2.0 <= np.sqrt(em)
        else:
            mats, _ = og.conf_matrices(pos, M, p)
            z = og.known_z(mats.mean(axis=0), er, er2, len(pos))
            print('M = 8: largest |z| of a cell = %.2f' % np.abs(z).max())
            assert np.abs(z).max() <= 4.5


# ---- 3. natural orbitals and n(k) on hand-made matrices ---------------------------
def test_natural_orbitals_rank_one_and_uniform():
    from phd_qmclib_amd import engine
    M, N, L = 12, 5.0, 6.0
    phi = np.cos(np.arange(M) * 0.3) + 1.5
    phi /= np.sqrt(np.sum(phi ** 2))
    k = N * np.outer(phi, phi)
    # one group of weight 3: sums = 3 K
    r = engine.natural_orbitals(3.0 * k[None], [3.0], N, supercell_size=L)
    assert np.allclose(r.matrix, k, rtol=1e-15, atol=0)
    assert abs(r.condensate_fraction - 1.0) <= 1e-14
    assert abs(r.purity - 1.0) <= 1e-14 and abs(r.trace - N) <= 1e-13
    assert np.all(np.diff(r.occupations) <= 1e-14)
    assert np.abs(r.occupations[1:]).max() <= 1e-14
    # G = 1: no errors to estimate
    assert r.purity_err == 0.0 and r.condensate_fraction_err == 0.0
    assert not r.occupations_err.any() and r.occupations_err.shape == (M,)
    # the orbitals: unit norm on the grid, the first one is phi
    delta = L / M
    assert np.allclose(np.sum(r.orbitals ** 2, axis=0) * delta, 1.0,
                       rtol=1e-13)
    assert np.allclose(np.abs(r.orbitals[:, 0]) * np.sqrt(delta), phi,
                       rtol=1e-12)
    unit = engine.natural_orbitals(k, 1.0, N)
    assert np.allclose(np.sum(unit.orbitals ** 2, axis=0), 1.0, rtol=1e-13)
    # K = (N / M) 1: every orbital holds N / M, purity 1 / M
    r = engine.natural_orbitals((N / M) * np.eye(M)[None], [1.0], N)
    assert abs(r.purity - 1.0 / M) <= 1e-15
    assert abs(r.condensate_fraction - 1.0 / M) <= 1e-15
    # a non-symmetric estimate is symmetrised
    a = np.array([[1.0, 0.5], [0.0, 2.0]])
    assert engine.natural_orbitals(a, 1.0, 3).matrix.tolist() == [
        [1.0, 0.25], [0.25, 2.0]]


def test_cross_group_purity_ignores_opposite_noise():
    from phd_qmclib_amd import engine
    M, N = 6, 3.0
    rng = np.random.RandomState(5)
    k = (N / M) * np.eye(M) + 0.01 * np.ones((M, M))
    e = rng.standard_normal((M, M))
    e = 0.05 * (e + e.T)
    sums = np.stack([2.0 * (k + e), 2.0 * (k - e)])
    r = engine.natural_orbitals(sums, [2.0, 2.0], N)
    assert np.allclose(r.matrix, k, rtol=1e-14)
    # <K + E, K - E> = |K|^2 - |E|^2, the same for (h, g): the mean of the
    # two ordered pairs; the Frobenius norm of either group alone is larger
    want = (np.sum(k ** 2) - np.sum(e ** 2)) / N ** 2
    assert abs(r.purity - want) <= 1e-15
    assert r.purity < np.sum((k + e) ** 2) / N ** 2
    assert r.purity != np.sum(k ** 2) / N ** 2
    assert r.purity_err > 0.0 and np.all(r.occupations_err >= 0.0)
    assert r.occupations_err.any() and r.condensate_fraction_err > 0.0
    # three equal groups: no spread, the cross estimate is the plain one
    r = engine.natural_orbitals(np.stack([k, k, k]), np.ones(3), N)
    assert abs(r.purity - np.sum(k ** 2) / N ** 2) <= 1e-15
    assert r.purity_err <= 1e-15 and np.all(r.occupations_err <= 1e-14)
    # the jackknife of the trace of a diagonal matrix, by hand: groups of
    # weight 1 with K_g = t_g, one cell
    t = np.array([1.0, 2.0, 4.0, 5.0])
    r = engine.natural_orbitals(t[:, None, None], np.ones(4), 1.0)
    assert r.occupations[0] == 3.0
    assert np.isclose(r.occupations_err[0], t.std(ddof=1) / 2.0, rtol=1e-14)
    for bad in ((np.zeros((2, 3, 4)), np.ones(2)), (np.zeros((2, 3, 3)),
                                                    np.ones(3)),
                (np.ones((2, 3, 3)), [1.0, 0.0])):
        with pytest.raises(ValueError):
            engine.natural_orbitals(bad[0], bad[1], 2)


def test_momentum_from_matrix_sums_to_the_trace():
    from phd_qmclib_amd import engine
    M, L = 9, 4.5
    rng = np.random.RandomState(3)
    a = rng.standard_normal((M, M))
    k = a @ a.T
    q = 2.0 * np.pi * np.arange(M) / L
    nk = engine.momentum_from_matrix(k, q, L)
    assert nk.shape == (M,) and np.all(nk >= -1e-12)
    assert abs(nk.sum() - np.trace(k)) <= 1e-12 * np.trace(k)
    # a uniform orbital holds everything at k = 0
    nk = engine.momentum_from_matrix(np.full((M, M), 2.0 / M), q, L)
    assert abs(nk[0] - 2.0) <= 1e-14 and np.abs(nk[1:]).max() <= 1e-14
    x = engine.one_body_matrix_points(L, M)
    assert np.array_equal(x, og.points(L, M)[1])
    with pytest.raises(ValueError):
        engine.momentum_from_matrix(np.zeros((2, 3)), q, L)


# ---- 4. the surface ----------------------------------------------------------------
def test_argument_errors():
    from phd_qmclib_amd import engine
    assert engine._obdm_grid_args(64, 32, 32) == (64, 32)
    assert engine._obdm_grid_args(512, 1024, 1024) == (512, 1024)
    for m, g, nc in ((0, 1, 4), (513, 1, 4), (2.5, 1, 4), (8, 0, 4),
                     (8, 5, 4), (8, 1025, 4096), (8, 1.5, 4), (8, 1, 0)):
        with pytest.raises(ValueError):
            engine._obdm_grid_args(m, g, nc)
    for bad in (0, 513, 1.5):
        with pytest.raises(ValueError):
            engine.one_body_matrix_points(16.0, bad)


_CTYPES = {'qmc_engine*': C.c_void_p, 'qmc_vmc*': C.c_void_p,
           'int64_t': C.c_int64, 'int32_t': C.c_int32}


def test_surface_binding_and_slot_table_unchanged():
    from phd_qmclib_amd import _lib, engine, mrbp_qmc
    from phd_qmclib_amd.qmc_base import dmc_est
    sig = _lib.SIGNATURES
    vp, dp = _lib._vp, _lib._dp
    i64, i32 = C.c_int64, C.c_int32
    assert sig['qmc_obdm_grid'] == (C.c_int, [vp, i64, dp, dp, i32, i32, dp,
                                              dp])
    assert sig['qmc_obdm_grid_dev'] == (C.c_int, [vp, i64, vp, vp, i32, i32,
                                                  vp, vp])
    assert sig['qmc_vmc_obdm_grid'] == (C.c_int, [vp, i32, i32, dp])
    # declared in the header with as many arguments
    text = open(os.path.join(ROOT, 'include', 'qmcwalk.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    assert 'QMCWALK_ABI_VERSION 1' in ' '.join(text.split())
    for name in ('qmc_obdm_grid', 'qmc_obdm_grid_dev', 'qmc_vmc_obdm_grid'):
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
        assert m, name + ' is not declared in include/qmcwalk.h'
        assert len(m.group(1).split(',')) == len(sig[name][1])
    for name in ('one_body_matrix', 'one_body_matrix_dev'):
        assert hasattr(engine.ModelEngine, name)
    assert hasattr(engine.VmcEnsemble, 'obdm_grid_parts')
    assert hasattr(mrbp_qmc.vmc.EnsembleSampling, 'one_body_matrix')
    assert hasattr(mrbp_qmc.dmc.Sampling, 'one_body_matrix')
    assert hasattr(mrbp_qmc.PhysicalFuncs, 'one_body_matrix')
    assert 'one_body_matrix(num_points, sys_conf)' in \
        mrbp_qmc.PhysicalFuncs.__doc__
    # no block estimator: the slot table keeps its seven records
    assert len(dmc_est.ESTIMATORS) == 7
    assert all('grid' not in str(e.key) and 'matrix' not in str(e.key)
               for e in dmc_est.ESTIMATORS)
