"""Pair distribution function g2(r): the checks that need no GPU.

* the NumPy restatement of the definition (tests/_pairdist_restatement.py),
  which the GPU tests compare the device counts with, against the reference's
  own `real_distance` values (tests/golden/pair_dist.npz, written by
  tools/gen_pairdist_golden.py): the distances bit for bit, the histograms
  against a brute-force double loop over the stored distances and against the
  stored histograms, exactly;
* every row adds up to N (N - 1) / 2; the normalisation gives 1 for the
  uniform expectation; the bin centres;
* the uniform law: pooled counts of iid uniform configurations lie within
  five standard deviations of n P / B in every bin (bound fixed in advance;
  the GPU test demands these very counts);
* the ctypes binding declares the four entry points with the argument types
  of include/qmcwalk.h, and the Python surface is importable without a GPU.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import _pairdist_restatement as rs
from .conftest import GOLDEN, ROOT

BINS = (1, 7, 64, 1000)
PD_ENTRIES = ('qmc_pair_dist', 'qmc_pair_dist_dev', 'qmc_pair_dist_reduce_dev',
              'qmc_vmc_pair_dist')


@pytest.fixture(scope='module')
def golden_pd():
    return np.load(os.path.join(GOLDEN, 'pair_dist.npz'), allow_pickle=False)


def stored_counts(golden_pd, tag, num_bins):
    off = sum(b for b in BINS[:BINS.index(num_bins)])
    return golden_pd[tag + '/counts'][:, off:off + num_bins].astype(np.int64)


def test_golden_covers_every_spec(golden_params, golden_pd, golden_kernels):
    tags = {k.split('/')[0] for k in golden_pd.files}
    assert tags == set(golden_params) and len(tags) == 15
    for tag in tags:
        n = golden_params[tag]['params']['boson_number']
        pos = golden_kernels[tag + '/pos']
        dist, counts = golden_pd[tag + '/dist'], golden_pd[tag + '/counts']
        assert pos.shape[1] == n
        assert counts.shape == (len(pos), sum(BINS))
        assert dist.shape == (len(pos) if n <= 64 else 2 if n <= 128 else 0,
                              n * (n - 1) // 2)
        assert np.all(np.isfinite(dist))


def test_restatement_matches_reference_distances(golden_params, golden_pd,
                                                 golden_kernels):
    """The restated min_distance reproduces the reference's real_distance bit
    for bit, and binning the reference's values in a plain double loop gives
    the restatement's histograms."""
    pairs = 0
    for tag in sorted(golden_params):
        L = float(golden_params[tag]['params']['supercell_size'])
        dist = golden_pd[tag + '/dist']
        pos = golden_kernels[tag + '/pos'][:len(dist)]
        if not len(dist):
            continue
        n = pos.shape[1]
        i, j = rs.pair_index(n)
        d = rs.min_distance(pos[:, i], pos[:, j], L)
        assert np.array_equal(d, dist), tag
        assert np.array_equal(rs.pair_separations(pos, L), np.abs(dist)), tag
        for nb in BINS:
            H = rs.pair_counts(pos, L, nb)
            brute = np.zeros_like(H)
            bin_size = (0.5 * L) / nb
            for c in range(len(dist)):
                k = 0
                for a in range(n):
                    for b in range(a + 1, n):
                        q = min(int(abs(float(dist[c, k])) // bin_size), nb - 1)
                        brute[c, q] += 1
                        k += 1
            assert np.array_equal(H, brute), (tag, nb)
        pairs += dist.size
    print('pairs held against the reference distances:', pairs)
    assert pairs > 60000


def test_restatement_matches_reference_histograms(golden_params, golden_pd,
                                                  golden_kernels):
    """Every configuration of every tag (N = 512 included), B = 1, 7, 64,
    1000: the histograms derived from the reference's distances."""
    for tag in sorted(golden_params):
        L = float(golden_params[tag]['params']['supercell_size'])
        pos = golden_kernels[tag + '/pos']
        n = pos.shape[1]
        for nb in BINS:
            H = rs.pair_counts(pos, L, nb)
            assert np.array_equal(H, stored_counts(golden_pd, tag, nb)), \
                (tag, nb)
            assert np.all(H.sum(axis=1) == n * (n - 1) // 2)


def test_row_sum_and_wrap():
    rng = np.random.RandomState(7)
    for n, L in ((8, 8.0), (37, 37.0), (100, 17.5)):
        pos = L * (5.0 * rng.random_sample((6, n)) - 2.5)   # outside the box too
        for nb in (1, 3, 65, 4096):
            H = rs.pair_counts(pos, L, nb)
            assert H.shape == (6, nb)
            assert np.all(H.sum(axis=1) == n * (n - 1) // 2)
        # a pair at exactly L/2 counts in the last bin, one at 0 in the first
        two = np.zeros((1, n))
        two[0] = np.linspace(0.0, 0.4 * L, n)
        two[0, -1] = two[0, 0] + 0.5 * L
        r = rs.pair_separations(two, L)
        assert r[0, n - 2] == 0.5 * L
        assert rs.bin_index(r, L, 16)[0, n - 2] == 15


def test_normalisation_and_bin_centres(golden_params):
    from phd_qmclib_amd import engine, mrbp_qmc
    for n, L, nb in ((64, 64.0, 32), (24, 17.5, 7), (512, 512.0, 4096)):
        uniform = np.full(nb, n * (n - 1) / 2 / nb)
        assert np.allclose(rs.normalise(uniform, n, L), 1.0, rtol=1e-14, atol=0)
        assert np.allclose(engine.pair_distribution_norm(uniform, n, L), 1.0,
                           rtol=1e-14, atol=0)
        r = rs.bin_centres(L, nb)
        assert np.array_equal(engine.pair_distribution_bins(L, nb), r)
        assert r[0] == 0.25 * L / nb and np.all(np.diff(r) > 0)
        assert np.isclose(r[-1] + 0.25 * L / nb, 0.5 * L, rtol=1e-14)
    spec = mrbp_qmc.Spec(**golden_params['odd24']['spec'])
    assert np.array_equal(mrbp_qmc.pair_distribution_bins(spec, 7),
                          rs.bin_centres(17.5, 7))
    assert np.array_equal(mrbp_qmc.pair_distribution_bins(spec.cfc_spec, 7),
                          rs.bin_centres(17.5, 7))
    for bad in (0, -1, 4097, 2.5):
        with pytest.raises(ValueError):
            engine.pair_distribution_bins(64.0, bad)


def test_uniform_law():
    """|z| <= 5 was fixed before the first run; seed as written."""
    u = rs.UNIFORM_LAW
    pos = rs.uniform_law_inputs()
    amb = rs.ambiguous_pairs(pos, u['sc_size'], u['num_bins'])
    assert sum(len(a) for a in amb) == 0
    H = rs.pair_counts(pos, u['sc_size'], u['num_bins'])
    z = rs.uniform_law_z(H.sum(axis=0), u['nconf'], u['n'], u['num_bins'])
    print('uniform law z per bin:', np.round(z, 2))
    assert np.all(np.abs(z) <= 5.0)
    g2 = rs.normalise(H.mean(axis=0), u['n'], u['sc_size'])
    assert np.all(np.abs(g2 - 1.0) < 0.01)


def test_ambiguous_pairs_are_found():
    L, nb = 16.0, 8                        # delta = 1
    pos = np.array([[0.0, 3.0, 8.0, 10.5 + 1e-12, 1.3, 2.0 - 1e-10]])
    amb = rs.ambiguous_pairs(pos, L, nb)[0]
    found = {(int(i), int(j)): int(e) for i, j, e in amb}
    assert found[(0, 1)] == 3              # r = 3 on the edge of bins 2 | 3
    assert found[(0, 2)] == nb             # r = L/2
    assert found[(0, 5)] == 2              # r = 2 - 1e-10
    assert (0, 4) not in found
    slack = rs.edge_slack(amb, nb)
    assert slack[2] >= 1 and slack[3] >= 1 and slack[7] >= 1
    assert len(rs.ambiguous_pairs(np.array([[0.1, 0.45, 5.77]]), L, nb)[0]) == 0


_CTYPES = {'qmc_engine*': C.c_void_p, 'qmc_vmc*': C.c_void_p,
           'int64_t': C.c_int64, 'int32_t': C.c_int32}


def test_binding_matches_header():
    from phd_qmclib_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'qmcwalk.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    host = ('qmc_pair_dist', 'qmc_vmc_pair_dist')
    for name in PD_ENTRIES:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, text)
        assert m, name + ' is not declared in include/qmcwalk.h'
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        params = [' '.join(p.split()) for p in m.group(1).split(',')]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            typ = (p[:p.rindex('*') + 1] if '*' in p else p.rsplit(' ', 1)[0])
            typ = re.sub(r'\s*\*', '*', typ).replace('const ', '')
            if typ in ('double*', 'uint32_t*'):
                # host arrays are typed pointers, device addresses void*
                typed = _lib._dp if typ == 'double*' else _lib._u32p
                assert a is (typed if name in host else C.c_void_p), (name, p)
            else:
                assert a is _CTYPES[typ], (name, p)


def test_surface_importable_without_gpu(golden_params, monkeypatch, tmp_path):
    from phd_qmclib_amd import _lib, engine, mrbp_qmc
    spec = mrbp_qmc.Spec(**golden_params['box16']['spec'])
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec)
    assert callable(pf.pair_distribution)
    for cls, name in ((engine.ModelEngine, 'pair_distribution'),
                      (engine.ModelEngine, 'pair_distribution_dev'),
                      (engine.ModelEngine, 'pair_distribution_reduce_dev'),
                      (engine.ModelEngine, 'pair_distribution_weighted'),
                      (engine.VmcEnsemble, 'pair_dist_parts'),
                      (mrbp_qmc.vmc.EnsembleSampling, 'pair_distribution'),
                      (mrbp_qmc.dmc.Sampling, 'pair_distribution')):
        assert callable(getattr(cls, name)), name
    # a device member raises the loader's usual error only when called
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'libqmcwalk.so'))
    monkeypatch.setattr(mrbp_qmc.core_funcs, '_engines', {})
    conf = np.zeros((2, 16))
    conf[0] = np.arange(16) + 0.25
    with pytest.raises(_lib.QmcError, match='has not been built'):
        pf.pair_distribution(8, conf)
