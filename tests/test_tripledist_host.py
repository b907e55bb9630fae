"""Three-body distribution g3(d): what can be held without a GPU.

* the restatement (tests/_tripledist_restatement.py): every row adds up to
  C(N,3); the ordered pair walk the kernel uses equals the brute force over
  all triples, ties and all-equal rows included; the closed form of the
  perfect lattice; the law of uniform particles E T[b] =
  C(N,3) 3 (delta/L)^2 (2 b + 1);
* the preconditions of the inputs of tests/test_gpu_triple_dist.py: no
  non-grid input has an edge-ambiguous triple, so every comparison of counts
  there is plain equality;
* the Python surface: bin centres, normalisation, argument errors, and the
  binding of the new entry points.
"""
from math import comb

import numpy as np
import pytest

from . import _pairdist_restatement as pd
from . import _tripledist_restatement as rs


def test_row_sums_and_wrap():
    rng = np.random.RandomState(1)
    for n in (3, 4, 5, 16, 37):
        L = float(n)
        pos = L * rng.random_sample((5, n))
        for B, D in ((1, None), (7, 0.3 * L), (64, L / 8)):
            T = rs.triple_counts(pos, L, B, D)
            assert T.shape == (5, B + 1)
            assert np.all(T.sum(axis=1) == comb(n, 3))
    # whole periods on a binary grid are exact
    grid = rs.grid_pool()
    T = rs.triple_counts(grid, 64.0, 16)
    for shift in (64.0, -64.0, 192.0):
        assert np.array_equal(rs.triple_counts(grid + shift, 64.0, 16), T)
    # a triple of span exactly D is overflow; below it counts in the last bin
    L = 16.0
    T = rs.triple_counts(np.array([[0.0, 3.0, 8.0]]), L, 4)
    assert T.tolist() == [[0, 0, 0, 0, 1]]
    T = rs.triple_counts(np.array([[1.0, 15.0, 16.5]]), L, 4)   # span 2.5
    assert T.tolist() == [[0, 1, 0, 0, 0]]
    T = rs.triple_counts(np.array([[0.0, 5.0, 11.0]]), L, 4)    # span 11
    assert T.tolist() == [[0, 0, 0, 0, 1]]
    for n in (1, 2):
        assert not rs.triple_counts(np.zeros((3, n)), 8.0, 5).any()
        assert not rs.rank_counts(np.zeros((3, n)), 8.0, 5).any()


@pytest.mark.parametrize('n', [3, 4, 7, 16, 37, 64, 65, 130])
def test_rank_form_equals_brute_force(n):
    L = float(n)
    rng = np.random.RandomState(40 + n)
    rows = [L * rng.random_sample((3, n)),
            rng.randint(0, 8 * n, size=(3, n)) / 8.0,        # ties on a grid
            rng.randint(0, 4, size=(2, n)) * (L / 4),        # heavy ties
            np.full((1, n), 0.375 * L),                      # all at one point
            np.zeros((1, n))]
    pos = np.concatenate(rows)
    for B, D in ((1, None), (8, None), (16, L / 4), (64, L / 8), (5, 0.3 * L)):
        brute = rs.triple_counts(pos, L, B, D)
        assert np.array_equal(rs.rank_counts(pos, L, B, D), brute), (B, D)
        # all particles at one point: every triple in bin 0
        assert brute[-1, 0] == brute[-2, 0] == comb(n, 3)
        perm = rng.permutation(n)
        assert np.array_equal(rs.rank_counts(pos[:, perm], L, B, D), brute)


def test_exact_lattice_closed_form():
    for n in (64, 512):
        L = float(n)
        pos = np.arange(n, dtype=np.float64)[None, :]
        for B in (1, 2, 16, 256, 4096):
            for D in (L / 2, L / 4):
                want = rs.lattice_counts(n, L, B, D)
                assert want.sum() == comb(n, 3)
                assert np.array_equal(rs.rank_counts(pos, L, B, D)[0], want)
                if n == 64:
                    assert np.array_equal(
                        rs.triple_counts(pos, L, B, D)[0], want)
    # delta = 1 at N = L = 64, D = 32: spans m = 2 ... 31, 64 (m - 1) each
    T = rs.lattice_counts(64, 64.0, 32)
    assert T[0] == T[1] == 0
    assert np.array_equal(T[2:32], 64 * (np.arange(2, 32) - 1))


def test_uniform_law():
    """|z| <= 4 on all 32 bins, the bound of the GPU test, on the restatement
    alone (max |z| = 1.9 on these inputs).  The 4096 rows go through the
    ordered pair walk; the brute force takes the first 64 of them."""
    u = pd.UNIFORM_LAW
    pos = pd.uniform_law_inputs()
    T = rs.rank_counts(pos, u['sc_size'], u['num_bins'])
    assert np.array_equal(
        T[:64], rs.triple_counts(pos[:64], u['sc_size'], u['num_bins']))
    assert np.all(T.sum(axis=1) == comb(u['n'], 3))
    z = rs.uniform_law_z(T, u['n'], u['sc_size'], u['num_bins'])
    print('uniform law: max |z| = %.2f' % np.abs(z).max())
    assert np.all(np.abs(z) <= 4.0)
    # and the normalisation is 1 on average
    g3 = rs.normalise(T.mean(axis=0), u['n'], u['sc_size'])
    assert abs(g3[-1] - 1.0) < 0.01


def test_ambiguous_triples_are_found():
    L, B = 16.0, 4                                  # delta = 2
    pos = np.array([[0.3, 1.1, 4.3, 9.45],          # span 4: on edge 2
                    [0.0, 1.0, 3.7, 9.1]])
    amb = rs.ambiguous_triples(pos, L, B)
    assert amb[0].tolist() == [[0, 1, 2]]
    assert len(amb[1]) == 0
    on_span = np.array([[0.5, 1.0, 8.5]])           # span 8 = D
    assert rs.ambiguous_triples(on_span, L, B)[0].tolist() == [[0, 1, 2]]
    assert rs.num_ambiguous(on_span + 1e-12, L, B) == 1
    assert rs.num_ambiguous(pos, L, B) == 1
    assert rs.num_ambiguous(pos, L, 3) == 0         # delta = 8/3
    assert rs.num_ambiguous(np.zeros((2, 2)), L, B) == 0


@pytest.mark.parametrize('n', rs.PARITY_SIZES)
def test_gpu_parity_inputs_have_no_ambiguous_triple(n):
    L = float(n)
    pool = rs.parity_pool(n)
    d = rs.triple_spans(pool, L)
    assert np.any(pool < 0) and np.any(pool >= L)
    for B in rs.PARITY_BINS:
        for D in rs.parity_spans(L):
            assert rs.num_ambiguous(pool, L, B, D, d=d) == 0, (B, D)


def test_other_gpu_inputs_have_no_ambiguous_triple():
    for n in (16, 37, 64, 128):
        pool, L = rs.nesting_pool(n), float(n)
        d = rs.triple_spans(pool, L)
        for B in (1, 5, 32):
            assert rs.num_ambiguous(pool, L, B, L / 4, d=d) == 0
            assert rs.num_ambiguous(pool, L, 2 * B, L / 2, d=d) == 0
    for n, B, frac in rs.ENTRY_CASES:
        pool, _ = rs.entry_pool(n)
        assert rs.num_ambiguous(pool, float(n), B, frac * n) == 0, (n, B)
    pool, _ = rs.entry_pool(16)
    for B, frac in ((33, 0.5), (4096, 0.125)):
        assert rs.num_ambiguous(pool, 16.0, B, frac * 16) == 0
    u = pd.UNIFORM_LAW
    pos = pd.uniform_law_inputs()[:64]
    assert rs.num_ambiguous(pos, u['sc_size'], u['num_bins']) == 0
    # the grid rows are exact instead: on the 1/8 grid with coincident rows
    grid = rs.grid_pool()
    assert np.array_equal(grid * 8, np.rint(grid * 8))
    assert np.all(grid[:, 0] == grid[:, 1]) and np.all(grid[:, 2] == grid[:, 5])


def test_normalisation_and_bin_centres(golden_params):
    from phd_qmclib_amd import engine, mrbp_qmc
    from phd_qmclib_amd.mrbp_qmc import Spec
    assert engine.MAX_TRIPLE_DIST_BINS == 4096
    spec = Spec(**golden_params['box37']['spec'])
    L, n = 37.0, 37
    for B, D in ((1, None), (16, None), (7, 0.3 * L), (64, L / 8)):
        want = rs.bin_centres(L, B, D)
        assert np.array_equal(engine.triple_distribution_bins(L, B, D), want)
        assert np.array_equal(mrbp_qmc.triple_distribution_bins(spec, B, D),
                              want)
        assert np.array_equal(
            mrbp_qmc.triple_distribution_bins(spec.cfc_spec, B, D), want)
        T = rs.triple_counts(rs.parity_pool(n), L, B, D)
        g3 = engine.triple_distribution_norm(T, n, L, D)
        assert g3.shape == (len(T), B)
        assert np.allclose(g3, rs.normalise(T, n, L, D), rtol=1e-14, atol=0)
        # the expectation of uniform particles normalises to 1
        e = np.append(rs.expected_uniform(n, L, B, D), 0.0)
        assert np.allclose(engine.triple_distribution_norm(e, n, L, D), 1.0,
                           rtol=1e-14, atol=0)
    # sum_b E T[b] = C(N,3) 3 (D/L)^2: the probability of a span below D
    assert np.isclose(rs.expected_uniform(n, L, 16).sum(),
                      comb(n, 3) * 0.75, rtol=1e-14)
    assert 'triple_distribution_bins' in mrbp_qmc.model.__all__
    assert hasattr(mrbp_qmc.PhysicalFuncs, 'triple_distribution')
    assert hasattr(mrbp_qmc.vmc.EnsembleSampling, 'triple_distribution')
    assert hasattr(mrbp_qmc.dmc.Sampling, 'triple_distribution')
    assert hasattr(engine.VmcEnsemble, 'triple_dist_parts')
    for name in ('triple_distribution', 'triple_distribution_dev',
                 'triple_distribution_reduce_dev',
                 'triple_distribution_weighted'):
        assert hasattr(engine.ModelEngine, name)


def test_argument_errors():
    from phd_qmclib_amd import engine
    L = 16.0
    for bad in (0.0, -1.0, 8.0 + 1e-9, 16.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            engine.triple_distribution_bins(L, 8, bad)
        with pytest.raises(ValueError):
            engine.triple_distribution_norm(np.zeros(9), 16, L, bad)
    for bad in (0, -3, 4097, 2.5):
        with pytest.raises(ValueError):
            engine.triple_distribution_bins(L, bad)
    with pytest.raises(ValueError):
        engine.triple_distribution_norm(np.zeros(1), 16, L)   # no bin left
    with pytest.raises(ValueError):
        engine.triple_distribution_norm(np.zeros(9), 2, L)    # no triple
    assert engine.triple_distribution_bins(L, 8, 8.0)[-1] == 7.5
    assert engine.triple_distribution_bins(L, 8, None)[-1] == 7.5


def test_binding_and_slot_table_unchanged():
    """The entry points are bound with max_span as a double after num_bins;
    no block-estimator slot was added for g3."""
    import ctypes as C
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd.qmc_base import dmc_est
    sig = _lib.SIGNATURES
    for name, pair in (('qmc_triple_dist', 'qmc_pair_dist'),
                       ('qmc_triple_dist_dev', 'qmc_pair_dist_dev'),
                       ('qmc_triple_dist_reduce_dev',
                        'qmc_pair_dist_reduce_dev'),
                       ('qmc_vmc_triple_dist', 'qmc_vmc_pair_dist')):
        res, args = sig[name]
        pres, pargs = sig[pair]
        k = pargs.index(C.c_int32) + 1
        assert res is pres
        assert args == pargs[:k] + [C.c_double] + pargs[k:]
    assert all('g3' not in str(e.key) and 'triple' not in str(e.key)
               for e in dmc_est.ESTIMATORS)
