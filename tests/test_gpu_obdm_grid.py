"""One-body density matrix on a grid on the GPU (csrc/qmc_obdm_grid.h) against
the NumPy restatement of its definition (tests/_obdm_grid_restatement.py).
All tests need a GPU.

A group sum is compared cell by cell with

    |dev - ref| <= 2e-11 sum_terms |w| ratio_ref max(1, scale),

the sum over the terms of that cell, `scale` the sum of the magnitudes of the
logarithms in the exponent of a term and 2e-11 the RTOL of the suite; a cell
without a term must be exactly 0.  Integer-valued cases are compared exactly.
"""
from itertools import islice

import numpy as np
import pytest

from . import _obdm_grid_restatement as og
from . import _partent_restatement as pe
from ._models import _dev, model_dict

pytestmark = pytest.mark.gpu

RTOL = og.RTOL


def spec_for(golden_params, key):
    """The golden model of that tag, the golden 'box' model of n particles
    where there is one, the same family otherwise (L = n)."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    if isinstance(key, str):
        if key == 'ideal_free16':      # no interaction and no lattice
            args = dict(golden_params['free16']['spec'])
            args['interaction_strength'] = 0
            return Spec(**args)
        if key == 'known2':            # free16 with two particles
            args = dict(golden_params['free16']['spec'])
            args['boson_number'] = 2
            return Spec(**args)
        return Spec(**golden_params[key]['spec'])
    if key in og.GOLDEN_SIZES:
        return Spec(**golden_params[og.GOLDEN_SIZES[key]]['spec'])
    return Spec(**og.model_spec_args(key))


@pytest.fixture(scope='module')
def models(golden_params):
    """key -> (engine, restatement's model dict, N, L, spec), built once."""
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(key):
        if key not in cache:
            spec = spec_for(golden_params, key)
            cache[key] = (ModelEngine(spec.cfc_spec),
                          model_dict(spec.cfc_spec), spec.boson_number,
                          float(spec.supercell_size), spec)
        return cache[key]
    yield get
    for rec in cache.values():
        rec[0].close()


def check(got, want, label):
    sums, wsum = got
    ref, wref, bound = want
    assert sums.dtype == np.float64 and sums.shape == ref.shape
    assert wsum.shape == wref.shape
    ok, worst = og.within(sums, ref, bound)
    print('%s: worst error / bound = %.3g' % (label, worst))
    assert ok
    assert np.all(np.abs(wsum - wref) <= RTOL * np.maximum(1.0, np.abs(wref)))


# ---- 1. parity with the definition ---------------------------------------------
@pytest.mark.parametrize('num_points', og.PARITY_POINTS)
@pytest.mark.parametrize('n', og.PARITY_SIZES)
def test_parity(models, n, num_points):
    eng, p, nn, L, _ = models(n)
    assert nn == n and L == float(n)
    pos = og.pool(n)
    assert pos.shape == (og.PARITY_CONFS, n)
    assert np.any(pos < 0) and np.any(pos >= L)
    mats, bound = og.conf_matrices(pos, num_points, p)
    for G in og.PARITY_GROUPS:
        got = eng.one_body_matrix(pos, num_points, G)
        assert got[0].shape == (G, num_points, num_points)
        check(got, og.group_sums(mats, bound, G),
              'N=%d M=%d G=%d' % (n, num_points, G))
        # every particle of the group lands in one row
        assert np.array_equal(got[1], np.bincount(
            np.arange(len(pos)) % G, minlength=G).astype(float))


def test_parity_n512(models):
    eng, p, n, L, _ = models(512)
    pos = og.pool(512, nconf=4)
    assert pos.shape == (4, 512)
    for G in (1, 4):
        check(eng.one_body_matrix(pos, 8, G), og.reference(pos, 8, G, p),
              'N=512 M=8 G=%d' % G)


@pytest.mark.parametrize('tag', ['free16', 'defect24'])
def test_parity_other_models(models, tag):
    eng, p, n, L, _ = models(tag)
    rng = np.random.RandomState(len(tag))
    pos = L * (3.0 * rng.random_sample((og.PARITY_CONFS, n)) - 1.0)
    for M, G in ((7, 1), (24, 5), (65, 1)):
        check(eng.one_body_matrix(pos, M, G), og.reference(pos, M, G, p),
              '%s M=%d G=%d' % (tag, M, G))


# ---- 2. the order of a row does not matter -------------------------------------
@pytest.mark.parametrize('n', og.ORDER_SIZES)
def test_order_independence(models, n):
    eng, p, _, L, _ = models(n)
    pos = og.pool(n)
    srt, shf = og.reorderings(pos, L, n)
    assert np.all(np.diff(og.wrap(srt, L), axis=1) >= 0)
    for M, G in ((7, 5), (64, 1)):
        want = og.reference(pos, M, G, p)
        for rows, name in ((pos, 'as drawn'), (srt, 'sorted'),
                           (shf, 'shuffled')):
            check(eng.one_body_matrix(rows, M, G), want,
                  'N=%d M=%d %s' % (n, M, name))


# ---- 3. exact cases --------------------------------------------------------------
def test_constant_wave_function_counts_particles(models):
    """psi constant: sums[g][a][c] is the number of particles of group g in
    bin a, the same for every c, exactly."""
    eng, p, n, L, _ = models('ideal_free16')
    assert p['params']['is_free'] and p['params']['is_ideal']
    pos = og.pool(16, nconf=40)
    for M, G in ((7, 1), (64, 3), (130, 40)):
        sums, wsum = eng.one_body_matrix(pos, M, G)
        a = og.row_bins(pos, L, M)
        want = np.zeros((G, M))
        for c in range(len(pos)):
            want[c % G] += np.bincount(a[c], minlength=M)
        assert np.array_equal(sums, np.repeat(want[:, :, None], M, axis=2))
        assert np.array_equal(wsum, np.bincount(np.arange(40) % G,
                                                minlength=G).astype(float))


def test_cell_edges(models):
    """A particle exactly on the edge a delta counts in bin a, one at the
    largest double below L in bin M - 1 (psi constant: exact counts)."""
    eng, _, n, L, _ = models('ideal_free16')
    for M in (7, 16, 64):
        delta, _ = og.points(L, M)
        edges = np.arange(M) * delta
        pos = np.resize(edges, (3, n))
        pos[1] = np.resize(edges[::-1], n)
        pos[2] = np.nextafter(L, 0.0)
        pos[2, 0] = 0.0
        a = og.row_bins(pos, L, M)
        assert np.all(a[2, 1:] == M - 1) and a[2, 0] == 0
        if M in (16, 64):                  # delta a power of two: no rounding
            assert np.array_equal(a[0], np.resize(np.arange(M), n))
        sums, _ = eng.one_body_matrix(pos, M, 3)
        for c in range(3):
            want = np.bincount(a[c], minlength=M).astype(float)
            assert np.array_equal(sums[c], np.repeat(want[:, None], M, axis=1))


def test_no_interaction_is_an_outer_product(models):
    """ideal16 (lattice, no interaction): the matrix of every configuration is
    sum_{i in a} 1 / f1(z_i) times f1(x_c)."""
    from ._obdm_restatement import _log_f1
    eng, p, n, L, _ = models('ideal16')
    assert p['params']['is_ideal'] and not p['params']['is_free']
    pos = og.pool(16)
    for M in (7, 64):
        _, x = og.points(L, M)
        a = og.row_bins(pos, L, M)
        inv = np.exp(-_log_f1(og.wrap(pos, L), p))
        fx = np.exp(_log_f1(x, p))
        want = np.zeros((len(pos), M, M))
        for c in range(len(pos)):
            rows = np.zeros(M)
            np.add.at(rows, a[c], inv[c])
            want[c] = np.outer(rows, fx)
        _, bound = og.conf_matrices(pos, M, p)
        sums, _ = eng.one_body_matrix(pos, M, len(pos))
        ok, worst = og.within(sums, want, bound)
        print('ideal16 M=%d: worst error / bound = %.3g' % (M, worst))
        assert ok


@pytest.mark.parametrize('n', [16, 64])
def test_particle_on_a_cell_centre_gives_exactly_one(models, n):
    """Particles exactly on distinct cell centres: the diagonal cell of each
    is exactly 1, as g1(0) is."""
    eng, p, _, L, _ = models(n)
    M = 4 * n if n == 16 else 130
    _, x = og.points(L, M)
    rng = np.random.RandomState(n)
    cols = np.stack([rng.permutation(M)[:n] for _ in range(6)])
    pos = x[cols]
    sums, _ = eng.one_body_matrix(pos, M, len(pos))
    for c in range(len(pos)):
        assert np.array_equal(og.row_bins(pos[c], L, M), cols[c])
        assert np.all(sums[c][cols[c], cols[c]] == 1.0)
    check((sums, np.ones(6)), og.reference(pos, M, 6, p), 'N=%d centres' % n)


# ---- 4. groups, weights, sizes -----------------------------------------------------
@pytest.fixture(scope='module')
def many(models):
    """N = 8, M = 8, 4097 configurations: more work than one pass of the
    grid; the per-configuration reference, computed once."""
    eng, p, n, L, _ = models(8)
    rng = np.random.RandomState(4097)
    pos = L * (2.0 * rng.random_sample((4097, n)) - 0.5)
    mats, bound = og.conf_matrices(pos, 8, p)
    w = rng.random_sample(4097) + 0.1
    w[11] = 0.0
    for a in (pos, mats, bound, w):
        a.setflags(write=False)
    return eng, pos, mats, bound, w


@pytest.mark.parametrize('G', [1, 3, 32])
def test_groups_and_weights(many, G):
    eng, pos, mats, bound, w = many
    got = eng.one_body_matrix(pos, 8, G)
    check(got, og.group_sums(mats, bound, G), '4097 confs G=%d' % G)
    assert np.array_equal(got[1], np.bincount(np.arange(4097) % G,
                                              minlength=G).astype(float))
    # unit weights are the absent weights, bit for bit; two calls agree
    ones = eng.one_body_matrix(pos, 8, G, weights=np.ones(4097))
    again = eng.one_body_matrix(pos, 8, G)
    for a, b, c in zip(got, ones, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # random positive weights, one of them zero
    gw = eng.one_body_matrix(pos, 8, G, weights=w)
    check(gw, og.group_sums(mats, bound, G, w), '4097 confs G=%d weighted' % G)
    assert np.array_equal(eng.one_body_matrix(pos, 8, G, weights=w)[0], gw[0])


def test_groups_add_up(many):
    eng, pos, mats, bound, w = many
    s1, w1 = eng.one_body_matrix(pos, 8, 1, weights=w)
    s32, w32 = eng.one_body_matrix(pos, 8, 32, weights=w)
    _, _, b1 = og.group_sums(mats, bound, 1, w)
    assert np.all(np.abs(s32.sum(axis=0) - s1[0]) <= 2.0 * b1[0])
    assert abs(w32.sum() - w1[0]) <= RTOL * w1[0]


# ---- 5. one path, many doors -------------------------------------------------------
@pytest.mark.parametrize('n', [3, 37])
def test_entry_points_agree(models, golden_params, n):
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.engine import DeviceBuffer
    eng, p, _, L, _ = models(n)
    pos = og.pool(n)
    W, M, G = len(pos), 9, 4
    rng = np.random.RandomState(n)
    w = rng.random_sample(W) + 0.5
    sums, wsum = eng.one_body_matrix(pos, M, G, weights=w)
    dpos, dw = _dev(eng, pos), _dev(eng, w)
    ds, dws = DeviceBuffer((G, M, M), eng.device), DeviceBuffer((G,),
                                                                eng.device)
    eng.one_body_matrix_dev(W, dpos.ptr, dw.ptr, M, G, ds.ptr, dws.ptr)
    eng.sync()
    assert np.array_equal(ds.download(), sums)
    assert np.array_equal(dws.download(), wsum)
    # no weights, no wsum
    ds.upload(np.full((G, M, M), 7.0))
    eng.one_body_matrix_dev(W, dpos.ptr, None, M, G, ds.ptr, None)
    eng.sync()
    assert np.array_equal(ds.download(), eng.one_body_matrix(pos, M, G)[0])
    for b in (dpos, dw, ds, dws):
        b.close()
    # PhysicalFuncs: one configuration per group, broadcast loop dimensions
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec_for(golden_params, n))
    want = eng.one_body_matrix(pos, M, W)[0]
    check((want, np.ones(W)), og.reference(pos, M, W, p), 'N=%d per conf' % n)
    confs = np.zeros((W, 2, n))
    confs[:, 0, :] = pos
    out = pf.one_body_matrix(M, confs)
    assert out.shape == (W, M, M) and np.array_equal(out, want)
    out = pf.one_body_matrix(M, confs.reshape(3, 4, 2, n))
    assert np.array_equal(out, want.reshape(3, 4, M, M))
    one = pf.one_body_matrix(M, confs[5])
    assert one.shape == (M, M) and np.array_equal(one, want[5])


@pytest.mark.parametrize('move', ['all', 'particle'])
def test_vmc_resident_rows(golden_params, models, move):
    from phd_qmclib_amd import engine
    from phd_qmclib_amd.mrbp_qmc import vmc
    n, W, M, G = 16, 64, 24, 8
    spec = spec_for(golden_params, n)
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21,
                             move=move)
    s.init_random(seed=3)
    for _ in islice(s.blocks(4), 2):
        pass
    before = s.ensemble.get_state()
    x, res = s.one_body_matrix(M, G)
    parts = s.ensemble.obdm_grid_parts(M, G)
    after = s.ensemble.get_state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    confs = s.confs()
    with pytest.raises(ValueError):
        s.ensemble.obdm_grid_parts(M, W + 1)
    s.close()
    eng, p, _, L, _ = models(n)
    want = og.reference(confs, M, G, p)
    check((parts, np.full(G, W / G)), want, 'vmc %s' % move)
    check(eng.one_body_matrix(confs, M, G), want, 'vmc %s batch' % move)
    assert np.array_equal(x, og.points(L, M)[1])
    same = engine.natural_orbitals(parts, np.full(G, W / G), n, L)
    assert np.array_equal(res.matrix, same.matrix)
    assert np.array_equal(res.occupations, same.occupations)
    assert res.purity == same.purity and res.purity_err == same.purity_err
    assert res.matrix.shape == (M, M) and res.occupations.shape == (M,)
    assert abs(res.trace - res.occupations.sum()) <= 1e-10 * n
    assert res.condensate_fraction_err > 0.0 and res.purity_err > 0.0


def test_dmc_mixed_estimate(golden_params, golden_kernels, models):
    from phd_qmclib_amd import engine
    from phd_qmclib_amd.mrbp_qmc import dmc
    n, M, G = 16, 12, 4
    spec = spec_for(golden_params, n)
    rng = np.random.RandomState(9)
    pos = np.concatenate([golden_kernels['box16/pos'],
                          16.0 * rng.random_sample((40, 16))])
    nw0 = len(pos)
    s = dmc.Sampling(spec, 1e-3, 96, nw0, rng_seed=1)
    confs = np.zeros((nw0, 2, n))
    confs[:, 0, :] = pos
    state = next(s.blocks(s.build_state(confs), 8, 0)).last_state
    nw = int(state.num_walkers)
    assert 0 < nw < len(np.asarray(state.confs))
    weight = state.props.weight.copy()
    weight[nw:] = 1e9               # dead slots must not count
    live = np.asarray(state.confs)[:nw, 0, :].copy()
    garbage = np.asarray(state.confs).copy()
    garbage[nw:] = 0.123
    state = state._replace(confs=garbage,
                           props=state.props._replace(weight=weight))
    x, res = s.one_body_matrix(state, M, G)
    _, p, _, L, _ = models(n)
    sums, wsum, bound = og.reference(live, M, G, p, weight[:nw])
    k = sums.sum(axis=0) / wsum.sum()
    b = bound.sum(axis=0) / wsum.sum()
    b = 0.5 * (b + b.T) + 4e-16 * np.abs(k)
    assert np.array_equal(x, og.points(L, M)[1])
    assert np.all(np.abs(res.matrix - 0.5 * (k + k.T)) <= b)
    want = engine.natural_orbitals(sums, wsum, n, L)
    assert abs(res.condensate_fraction - want.condensate_fraction) <= 1e-9
    assert abs(res.purity - want.purity) <= 1e-9 and res.purity_err > 0.0


# ---- 6. the known answer: N = 2 without a lattice -----------------------------------
def test_known_answer(models):
    """The 16384 grid configurations drawn from psi^2 of two interacting
    particles on a ring: the per-cell mean of the device lies within 4.5 sigma
    of the exact E R, sigma from the exact E R^2; with M = 24 every particle
    sits on a cell centre and the trace of every configuration's matrix is
    exactly 2."""
    eng, p, n, L, spec = models('known2')
    assert n == 2 and spec.is_free and not spec.is_ideal
    _, _, pos = pe.known_answer(spec.tbf_params, L)
    conf, w = og.known_grid(spec.tbf_params, L)
    assert pos.shape == (16384, 2)
    for M in (8, 24):
        er, er2 = og.known_moments(conf, w, M, p)
        sums, wsum = eng.one_body_matrix(pos, M, 32)
        assert wsum.sum() == len(pos)
        z = og.known_z(sums.sum(axis=0) / len(pos), er, er2, len(pos))
        print('known answer M=%d: largest |z| of a cell = %.2f'
              % (M, np.abs(z).max()))
        assert np.abs(z).max() <= 4.5
    per = eng.one_body_matrix(pos[:1024], 24, 1024)[0]
    assert np.all(np.trace(per, axis1=1, axis2=2) == 2.0)


# ---- 7. errors -----------------------------------------------------------------------
def test_errors(models):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    n = 16
    eng, p, _, L, _ = models(n)
    pos = np.ascontiguousarray(og.pool(n))
    W = len(pos)
    for bad in (dict(num_points=0), dict(num_points=513),
                dict(num_points=8, num_groups=0),
                dict(num_points=8, num_groups=W + 1)):
        with pytest.raises(ValueError):
            eng.one_body_matrix(pos, **bad)
    for bad in (pos[:0], pos[:, :15], pos[0]):
        with pytest.raises(ValueError):
            eng.one_body_matrix(bad, 8)
    with pytest.raises(ValueError):
        eng.one_body_matrix(pos, 8, weights=np.ones(W - 1))
    lib = _lib.load()
    M, G = 8, 4
    sums, wsum = np.full((G, M, M), 7.0), np.full(G, 7.0)
    big = np.zeros((2000, n))

    def call(nconf=W, pos_=ptr(pos), m=M, g=G, out=ptr(sums)):
        return lib.qmc_obdm_grid(eng._h, nconf, pos_, None, m, g, out,
                                 ptr(wsum))
    for kwargs in (dict(m=0), dict(m=-3), dict(m=513), dict(g=0),
                   dict(g=W + 1), dict(nconf=0), dict(nconf=-2),
                   dict(pos_=None), dict(out=None),
                   dict(nconf=2000, g=1025, pos_=ptr(big))):
        assert call(**kwargs) != 0, kwargs
        assert b'qmc_obdm_grid' in lib.qmc_last_error()
        assert b'qmc_obdm_grid_dev' not in lib.qmc_last_error()
    assert np.all(sums == 7.0) and np.all(wsum == 7.0)
    assert lib.qmc_obdm_grid_dev(eng._h, W, None, None, M, G, None, None) != 0
    assert b'qmc_obdm_grid_dev' in lib.qmc_last_error()
    assert lib.qmc_obdm_grid_dev(eng._h, W, ptr(pos), None, 0, G,
                                 ptr(sums), None) != 0
    assert b'qmc_obdm_grid_dev' in lib.qmc_last_error()
    assert lib.qmc_vmc_obdm_grid(None, M, G, ptr(sums)) != 0
    assert b'qmc_vmc_obdm_grid' in lib.qmc_last_error()
    assert np.all(sums == 7.0)
    # wsum may be absent, and the engine still works afterwards
    assert lib.qmc_obdm_grid(eng._h, W, ptr(pos), None, M, G, ptr(sums),
                             None) == 0
    check((sums, np.full(G, W / G)), og.reference(pos, M, G, p),
          'after the errors')
