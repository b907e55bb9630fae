"""Pair distribution function g2(r) on the GPU (csrc/qmc_pairdist.h) against the
NumPy restatement of its definition (tests/_pairdist_restatement.py, itself
held against the reference's own distances by tests/test_pairdist_host.py).
All tests need a GPU.

The per-configuration result is a vector of integers, so the comparison is
EQUALITY, in every test that compares counts (`check_counts`):

* device counts equal restatement counts exactly wherever the restatement
  reports no edge-ambiguous pair (a pair whose r / delta lies within 1e-9 of an
  integer, or whose |z_i - z_j| lies within 1e-9 L of L/2: the only pairs that
  rounding can move between neighbouring bins);
* where it reports some, bin b may differ by at most the number of ambiguous
  pairs that touch edge b or b + 1, and the row must still add up to
  N (N - 1) / 2.  Only the golden configurations (which hold particles at
  0, at L - 1e-12 and in contact on purpose) may use this rule; every randomly
  drawn input set asserts that it has NO ambiguous pair, so that plain
  equality is what is demanded there.

Weighted sums in floating point use the suite's own criterion,
|delta| <= 2e-11 max(1, |x|) (tests/test_gpu_parity.py).
"""
import os
import sys
from itertools import islice
from math import pi

import numpy as np
import pytest

from . import _pairdist_restatement as rs
from .conftest import ROOT
from ._models import _dev, spec_from_golden

pytestmark = pytest.mark.gpu

RTOL = 2e-11
BINS = (1, 7, 64, 1000)
ALL_TAGS = ['box8', 'box16', 'box64', 'box128', 'box512', 'free16', 'deep100',
            'deep16', 'ideal16', 'defect24', 'odd24', 'box37', 'box48',
            'box100', 'box126']


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


@pytest.fixture(scope='module')
def engines(golden_params):
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = ModelEngine(
                spec_from_golden(golden_params, tag).cfc_spec)
        return cache[tag]
    yield get
    for e in cache.values():
        e.close()


def check_counts(dev, ref, amb, n, widened=False):
    """The comparison rule of the module docstring.  dev[W, B] device counts,
    ref[W, B] restatement counts, amb: ambiguous pairs per configuration.
    -> number of ambiguous pairs."""
    dev = np.asarray(dev)
    assert dev.dtype == np.uint32 and dev.shape == ref.shape
    dev = dev.astype(np.int64)
    namb = sum(len(a) for a in amb)
    if not widened:
        assert namb == 0, 'a drawn input set must have no ambiguous pair'
    assert np.all(dev.sum(axis=1) == n * (n - 1) // 2)
    for c in range(len(ref)):
        if len(amb[c]) == 0:
            assert np.array_equal(dev[c], ref[c]), c
        else:
            slack = rs.edge_slack(amb[c], ref.shape[1])
            assert np.all(np.abs(dev[c] - ref[c]) <= slack), c
    return namb


def counts_dev(eng, dpos, W, B):
    """qmc_pair_dist_dev on a resident position buffer -> counts[W, B]."""
    from phd_qmclib_amd.engine import DeviceBuffer
    buf = DeviceBuffer(((W * B + 1) // 2,), eng.device)     # uint32 pairs
    eng.pair_distribution_dev(W, dpos.ptr, B, buf.ptr)
    eng.sync()
    out = buf.download().view(np.uint32)[:W * B].reshape(W, B).copy()
    buf.close()
    return out


# ---- 1. the golden configurations ----------------------------------------
@pytest.mark.parametrize('tag', ALL_TAGS)
def test_pair_dist_golden(engines, golden_params, golden_kernels, tag):
    L = float(golden_params[tag]['params']['supercell_size'])
    pos = golden_kernels[tag + '/pos']
    n = pos.shape[1]
    pairs = amb_total = 0
    for B in BINS:
        dev = engines(tag).pair_distribution(pos, B)
        amb = rs.ambiguous_pairs(pos, L, B)
        amb_total += check_counts(dev, rs.pair_counts(pos, L, B), amb, n,
                                  widened=True)
        pairs += len(pos) * n * (n - 1) // 2
    print(tag, 'pairs covered', pairs, 'of them edge-ambiguous', amb_total)


# ---- 2. the exact lattice case --------------------------------------------
def lattice_confs():
    """L = 64, positions multiples of 1/8: every operation is exact."""
    rng = np.random.RandomState(64)
    pos = rng.randint(0, 512, size=(40, 64)) / 8.0
    pos[:, 0] = 0.0
    pos[:, 1] = 32.0              # r = L/2 exactly
    pos[:, 2] = 4.0               # on a bin edge for every B >= 8
    pos[:, 3] = 63.875            # r = 1/8 through the boundary
    pos[0] = np.arange(64)        # the perfect lattice
    return pos


LATTICE_BINS = (1, 2, 16, 256, 4096)


def test_pair_dist_exact_lattice(engines):
    eng = engines('box64')
    pos = lattice_confs()
    for B in LATTICE_BINS:
        ref = rs.pair_counts(pos, 64.0, B)
        dev = eng.pair_distribution(pos, B)
        assert dev.dtype == np.uint32
        assert np.array_equal(dev.astype(np.int64), ref), B
        # the tie rule: r = L/2 in the last bin, r = k delta in bin k
        assert np.all(ref[:, -1] >= 1)
        for shift in (64.0, -64.0, 192.0, -192.0):
            assert np.array_equal(eng.pair_distribution(pos + shift, B), dev), \
                (B, shift)
    # the perfect lattice at delta = 1: 64 pairs per distance, 32 at L/2
    H = eng.pair_distribution(pos[:1], 32)[0]
    assert H[0] == 0 and np.all(H[1:31] == 64) and H[31] == 64 + 32


# ---- 3. identities ---------------------------------------------------------
def identity_pool(n, L):
    rng = np.random.RandomState(300 + n)
    return L * rng.random_sample((12, n))


@pytest.mark.parametrize('tag', ['box8', 'box37', 'box64', 'odd24', 'box100',
                                 'box128', 'box512'])
def test_pair_dist_identities(engines, golden_params, tag):
    p = golden_params[tag]['params']
    n, L = p['boson_number'], float(p['supercell_size'])
    pos = identity_pool(n, L)
    eng = engines(tag)
    rng = np.random.RandomState(11)
    perm = rng.permutation(n)
    for B in (1, 5, 64, 1000):
        H = eng.pair_distribution(pos, B)
        assert np.all(H.sum(axis=1, dtype=np.int64) == n * (n - 1) // 2)
        assert np.array_equal(eng.pair_distribution(pos[:, perm], B), H)
        check_counts(H, rs.pair_counts(pos, L, B),
                     rs.ambiguous_pairs(pos, L, B), n)
    one = eng.pair_distribution(pos, 1)
    assert np.array_equal(one, np.full((len(pos), 1), n * (n - 1) // 2))


def test_pair_dist_uniform_law(engines):
    """The pooled counts the host test holds against the uniform law
    (tests/test_pairdist_host.py::test_uniform_law), reproduced exactly."""
    u = rs.UNIFORM_LAW
    pos = rs.uniform_law_inputs()
    ref = rs.pair_counts(pos, u['sc_size'], u['num_bins'])
    dev = engines('box64').pair_distribution(pos, u['num_bins'])
    check_counts(dev, ref, rs.ambiguous_pairs(pos, u['sc_size'], u['num_bins']),
                 u['n'])
    z = rs.uniform_law_z(dev.sum(axis=0, dtype=np.int64), u['nconf'], u['n'],
                         u['num_bins'])
    assert np.all(np.abs(z) <= 5.0)


# ---- 4. every shape ----------------------------------------------------------
SHAPE_TAGS = {8: 'box8', 37: 'box37', 64: 'box64', 100: 'box100',
              128: 'box128', 512: 'box512'}
SHAPE_BINS = (1, 65, 4096)


def shape_pool(n, L):
    rng = np.random.RandomState(100 + n)
    pool = L * rng.random_sample((24 if n <= 128 else 8, n))
    pool[1] -= 0.75 * L            # positions outside [0, L) are legal
    pool[2] += 1.5 * L
    pool[3] -= 7.25 * L
    return pool, rng


@pytest.mark.parametrize('n', sorted(SHAPE_TAGS))
def test_pair_dist_batch_shapes(engines, golden_params, n):
    tag = SHAPE_TAGS[n]
    L = float(golden_params[tag]['params']['supercell_size'])
    pool, rng = shape_pool(n, L)
    eng = engines(tag)
    for B in SHAPE_BINS:
        ref = rs.pair_counts(pool, L, B)
        amb = rs.ambiguous_pairs(pool, L, B)
        assert sum(len(a) for a in amb) == 0
        for nconf in (1, 63, 64, 65, 4097):
            idx = rng.randint(0, len(pool), size=nconf)
            dev = eng.pair_distribution(pool[idx], B)
            assert dev.shape == (nconf, B) and dev.dtype == np.uint32
            assert np.array_equal(dev.astype(np.int64), ref[idx]), \
                (n, B, nconf)


# ---- 5. one path, many doors ---------------------------------------------
def entry_pool(n, L):
    rng = np.random.RandomState(500 + n)
    return L * rng.random_sample((70, n)), rng


@pytest.mark.parametrize('tag', ['box16', 'box37', 'box64', 'box100',
                                 'box128'])
def test_pair_dist_entry_points_agree(engines, golden_params, tag):
    from phd_qmclib_amd.engine import DeviceBuffer, VmcEnsemble
    eng = engines(tag)
    p = golden_params[tag]['params']
    n, L = p['boson_number'], float(p['supercell_size'])
    pos, rng = entry_pool(n, L)
    W = len(pos)
    for B in (7, 64):
        H = eng.pair_distribution(pos, B)
        check_counts(H, rs.pair_counts(pos, L, B),
                     rs.ambiguous_pairs(pos, L, B), n)
        Hi = H.astype(np.int64)
        # device buffers: bit for bit
        dpos = _dev(eng, pos)
        assert np.array_equal(counts_dev(eng, dpos, W, B), H)
        # the reduction, unit weights: exact integers, the same bits twice
        dsums = DeviceBuffer((B, 2), eng.device)
        dws = DeviceBuffer((1,), eng.device)
        eng.pair_distribution_reduce_dev(W, dpos.ptr, None, B, dsums.ptr,
                                         dws.ptr)
        eng.sync()
        s1, w1 = dsums.download(), dws.download()
        assert w1[0] == W
        assert np.array_equal(s1[:, 0], Hi.sum(axis=0))
        assert np.array_equal(s1[:, 1], (Hi ** 2).sum(axis=0))
        # random positive weights
        w = 0.25 + rng.random_sample(W)
        dw = _dev(eng, w)
        eng.pair_distribution_reduce_dev(W, dpos.ptr, dw.ptr, B, dsums.ptr,
                                         dws.ptr)
        eng.sync()
        sw, ww = dsums.download(), dws.download()
        eng.pair_distribution_reduce_dev(W, dpos.ptr, dw.ptr, B, dsums.ptr,
                                         dws.ptr)
        eng.sync()
        assert np.array_equal(dsums.download(), sw)
        assert np.array_equal(dws.download(), ww)
        assert close(ww[0], w.sum())
        assert close(sw[:, 0], (w[:, None] * Hi).sum(axis=0))
        assert close(sw[:, 1], (w[:, None] * Hi ** 2).sum(axis=0))
        mean = eng.pair_distribution_weighted(pos, w, B)
        assert np.array_equal(mean, sw[:, 0] / ww[0])
        # the VMC ensemble's resident, position-sorted rows
        v = VmcEnsemble(eng, W, 0.125, rng_seed=1)
        v.set_state(pos)
        parts = v.pair_dist_parts(B)
        v.close()
        assert np.array_equal(parts[:, 0], Hi.sum(axis=0))
        assert np.array_equal(parts[:, 1], (Hi ** 2).sum(axis=0))
        for b in (dpos, dsums, dws, dw):
            b.close()


def test_pair_dist_reduce_spans_tiles(engines, golden_params):
    """More than one tile of 2^16 configurations; at B = 4096 the tile is
    2^12, so 4097 configurations span two as well."""
    from phd_qmclib_amd.engine import DeviceBuffer
    eng = engines('box16')
    n, L = 16, 16.0
    pool, rng = entry_pool(n, L)
    for W, B in (((1 << 16) + 4097, 33), (4097, 4096)):
        assert sum(len(a) for a in rs.ambiguous_pairs(pool, L, B)) == 0
        ref = rs.pair_counts(pool, L, B)
        idx = rng.randint(0, len(pool), size=W)
        pos = pool[idx]
        w = 0.25 + rng.random_sample(W)
        dpos, dw = _dev(eng, pos), _dev(eng, w)
        dsums = DeviceBuffer((B, 2), eng.device)
        dws = DeviceBuffer((1,), eng.device)
        eng.pair_distribution_reduce_dev(W, dpos.ptr, None, B, dsums.ptr,
                                         dws.ptr)
        eng.sync()
        s1 = dsums.download()
        assert dws.download()[0] == W
        assert np.array_equal(s1[:, 0], ref[idx].sum(axis=0))
        assert np.array_equal(s1[:, 1], (ref[idx] ** 2).sum(axis=0))
        eng.pair_distribution_reduce_dev(W, dpos.ptr, dw.ptr, B, dsums.ptr,
                                         dws.ptr)
        eng.sync()
        sw = dsums.download()
        assert close(dws.download()[0], w.sum())
        assert close(sw[:, 0], (w[:, None] * ref[idx]).sum(axis=0))
        assert close(sw[:, 1], (w[:, None] * ref[idx] ** 2).sum(axis=0))
        for b in (dpos, dw, dsums, dws):
            b.close()


# ---- 6. the resident rows of a VMC ensemble ----------------------------------
@pytest.mark.parametrize('tag', ['box16', 'box64', 'box100'])
def test_vmc_resident_rows(golden_params, tag):
    from phd_qmclib_amd.mrbp_qmc import vmc
    spec = spec_from_golden(golden_params, tag)
    n, L = spec.boson_number, float(spec.supercell_size)
    W, B = 256, 32
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21)
    twin = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21)
    for e in (s, twin):
        e.init_random(seed=3)
        for _ in islice(e.blocks(16), 3):
            pass
    before = s.ensemble.get_state()
    r, mean, err = s.pair_distribution(B)
    parts = s.ensemble.pair_dist_parts(B)
    after = s.ensemble.get_state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    confs = s.confs()
    assert sum(len(a) for a in rs.ambiguous_pairs(confs, L, B)) == 0
    H = rs.pair_counts(confs, L, B)
    assert np.array_equal(parts[:, 0], H.sum(axis=0))
    assert np.array_equal(parts[:, 1], (H ** 2).sum(axis=0))
    assert np.array_equal(r, rs.bin_centres(L, B))
    assert np.allclose(mean, rs.normalise(H.mean(axis=0), n, L), rtol=1e-13,
                       atol=0)
    want_err = rs.normalise(np.sqrt(H.var(axis=0) / (W - 1)), n, L)
    assert np.allclose(err, want_err, rtol=1e-9, atol=1e-12)
    # the chains go on as those of a twin that was never asked
    blk, blk_twin = next(s.blocks(16)), next(twin.blocks(16))
    assert np.array_equal(blk.energy, blk_twin.energy)
    assert np.array_equal(blk.accept_rate, blk_twin.accept_rate)
    for a, b in zip(s.ensemble.get_state(), twin.ensemble.get_state()):
        assert np.array_equal(a, b)
    s.close()
    twin.close()


# ---- 7. DMC mixed estimate -------------------------------------------------
def test_dmc_mixed_estimate(golden_params, golden_kernels):
    from phd_qmclib_amd.mrbp_qmc import dmc
    tag, B = 'box16', 24
    spec = spec_from_golden(golden_params, tag)
    pos = golden_kernels[tag + '/pos']
    rng = np.random.RandomState(9)
    pos = np.concatenate([pos, 16.0 * rng.random_sample((40, 16))])
    nw0, n = pos.shape
    s = dmc.Sampling(spec, 1e-3, 96, nw0, rng_seed=1)
    confs = np.zeros((nw0, 2, n))
    confs[:, 0, :] = pos
    state = next(s.blocks(s.build_state(confs), 8, 0)).last_state
    nw = int(state.num_walkers)
    assert 0 < nw < 96
    weight = state.props.weight.copy()
    weight[nw:] = 1e9               # dead slots must not count
    live = np.asarray(state.confs)[:nw, 0, :]
    garbage = np.asarray(state.confs).copy()
    garbage[nw:] = 0.123
    state = state._replace(confs=garbage,
                           props=state.props._replace(weight=weight))
    r, g2 = s.pair_distribution(state, B)
    assert sum(len(a) for a in rs.ambiguous_pairs(live, 16.0, B)) == 0
    H = rs.pair_counts(live, 16.0, B)
    want = rs.normalise((weight[:nw, None] * H).sum(axis=0)
                        / weight[:nw].sum(), n, 16.0)
    assert r.shape == g2.shape == (B,)
    assert np.array_equal(r, rs.bin_centres(16.0, B))
    assert close(g2, want)
    assert close(g2.sum() * (r[1] - r[0]) / 16.0 * 2, 1.0)


# ---- 8. Python surface ---------------------------------------------------
def test_physical_funcs_and_errors(engines, golden_params, golden_kernels):
    from phd_qmclib_amd import _lib, mrbp_qmc
    from phd_qmclib_amd._lib import ptr
    tag, B = 'box37', 16
    spec = spec_from_golden(golden_params, tag)
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec)
    pos = identity_pool(37, 37.0)[:8]
    confs = np.zeros((8, 2, 37))
    confs[:, 0, :] = pos
    assert sum(len(a) for a in rs.ambiguous_pairs(pos, 37.0, B)) == 0
    want = rs.normalise(rs.pair_counts(pos, 37.0, B), 37, 37.0)
    out = pf.pair_distribution(B, confs)
    assert out.shape == (8, B)
    assert np.allclose(out, want, rtol=1e-14, atol=0)
    assert np.array_equal(pf.pair_distribution(B, confs.reshape(2, 4, 2, 37)),
                          out.reshape(2, 4, B))
    one = pf.pair_distribution(B, confs[3])
    assert one.shape == (B,) and np.array_equal(one, out[3])
    assert np.array_equal(mrbp_qmc.pair_distribution_bins(spec, B),
                          rs.bin_centres(37.0, B))
    # bad arguments
    eng = engines(tag)
    for bad in (0, -3, 4097):
        with pytest.raises(ValueError):
            eng.pair_distribution(pos, bad)
        with pytest.raises(ValueError):
            pf.pair_distribution(bad, confs)
    with pytest.raises(ValueError):
        eng.pair_distribution(pos[:, :36], B)
    with pytest.raises(ValueError):
        eng.pair_distribution(pos[0], B)
    with pytest.raises(ValueError):
        eng.pair_distribution_weighted(pos, np.ones(7), B)
    with pytest.raises(ValueError):
        pf.pair_distribution(B, pos[0])
    lib = _lib.load()
    p = np.ascontiguousarray(pos)
    cnt = np.zeros((8, B), dtype=np.uint32)
    for args in ((ptr(p), 0, ptr(cnt, _lib._u32p)),
                 (ptr(p), 4097, ptr(cnt, _lib._u32p)),
                 (None, B, ptr(cnt, _lib._u32p)),
                 (ptr(p), B, None)):
        assert lib.qmc_pair_dist(eng._h, 8, *args) != 0
        assert b'qmc_pair_dist' in lib.qmc_last_error()
    assert lib.qmc_pair_dist_dev(eng._h, 1, None, B, None) != 0
    assert lib.qmc_pair_dist_reduce_dev(eng._h, 1, None, None, 0, None,
                                        None) != 0
    with pytest.raises(_lib.QmcError):
        eng.pair_distribution_dev(1, None, 5000, None)
    # the engine still works afterwards
    assert np.all(eng.pair_distribution(pos, 1) == 37 * 36 // 2)


# ---- 9. physics: the correlation hole -------------------------------------
def hole_z(r, mean, err, L):
    """(mean of the bins around L/4 - first bin) in standard errors of the
    first bin."""
    k = int(np.argmin(np.abs(r - 0.25 * L)))
    around = mean[k - 2:k + 2].mean()
    return (around - mean[0]) / err[0], around


def test_correlation_hole():
    """5 standard errors was fixed before the first run; seeds as written."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from _stationary import seed_configurations
    from phd_qmclib_amd.mrbp_qmc import Spec, vmc
    W, B, L = 1 << 12, 32, 64.0
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=64, supercell_size=64,
                tbf_contact_cutoff=16)
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=17)
    s.set_confs(seed_configurations(s.engine, spec, 64, seeds=W, steps=20000))
    r, mean, err = s.pair_distribution(B)
    s.close()
    z, around = hole_z(r, mean, err, L)
    print('interacting: g2(first bin) = %.5f +- %.5f, around L/4 %.5f, z = %.1f'
          % (mean[0], err[0], around, z))
    assert np.all(np.isfinite(mean)) and err[0] > 0
    assert np.isclose(mean.sum() * (r[1] - r[0]) * 2 / L, 1.0, rtol=1e-12)
    assert z > 5.0
    free = Spec(lattice_depth=0.0, lattice_ratio=1, interaction_strength=0.0,
                boson_number=64, supercell_size=64, tbf_contact_cutoff=16)
    assert free.is_free and free.is_ideal
    f = vmc.EnsembleSampling(free, 0.25, W, rng_seed=18)
    f.init_random(seed=5)
    for _ in islice(f.blocks(64), 2):
        pass
    r, mean, err = f.pair_distribution(B)
    f.close()
    z, around = hole_z(r, mean, err, L)
    print('free ideal:  g2(first bin) = %.5f +- %.5f, around L/4 %.5f, z = %.1f'
          % (mean[0], err[0], around, z))
    assert abs(z) <= 5.0
