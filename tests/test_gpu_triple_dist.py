"""Three-body distribution g3(d) on the GPU (csrc/qmc_tripledist.h) against the
NumPy restatement of its definition (tests/_tripledist_restatement.py: brute
force over all triples).  All tests need a GPU.

The per-configuration result is a vector of integers and the comparison is
EQUALITY, with no slack: every input is either on a binary grid (every
operation exact) or has no edge-ambiguous triple (a span within 1e-9 delta of a
bin edge or within 1e-9 L of max_span: the only triples rounding can move),
which tests/test_tripledist_host.py asserts without a GPU and the tests here
assert again wherever the rows come from the device.

Weighted sums in floating point use |delta| <= 2e-11 max(1, |x|), the RTOL of
tests/test_gpu_pair_dist.py.
"""
from itertools import islice
from math import comb

import numpy as np
import pytest

from . import _pairdist_restatement as pd
from . import _tripledist_restatement as rs
from ._models import _dev

pytestmark = pytest.mark.gpu

RTOL = 2e-11


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


def spec_for(golden_params, n):
    """The golden 'box' model of n particles where there is one, the same
    family otherwise; L = n either way."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    if n in rs.GOLDEN_SIZES:
        spec = Spec(**golden_params[rs.GOLDEN_SIZES[n]]['spec'])
    else:
        spec = Spec(**rs.model_spec_args(n))
    assert spec.boson_number == n and float(spec.supercell_size) == float(n)
    return spec


@pytest.fixture(scope='module')
def engines(golden_params):
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = ModelEngine(spec_for(golden_params, n).cfc_spec)
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


def check_counts(dev, ref, n):
    dev = np.asarray(dev)
    assert dev.dtype == np.uint32 and dev.shape == ref.shape
    assert np.all(dev.sum(axis=1, dtype=np.int64) == (comb(n, 3) if n >= 3
                                                      else 0))
    assert np.array_equal(dev.astype(np.int64), ref)


def counts_dev(eng, dpos, W, B, D):
    """qmc_triple_dist_dev on a resident position buffer -> counts[W, B + 1]."""
    from phd_qmclib_amd.engine import DeviceBuffer
    K = B + 1
    buf = DeviceBuffer(((W * K + 1) // 2,), eng.device)     # uint32 pairs
    eng.triple_distribution_dev(W, dpos.ptr, B, D, buf.ptr)
    eng.sync()
    out = buf.download().view(np.uint32)[:W * K].reshape(W, K).copy()
    buf.close()
    return out


# ---- 1. restatement parity, bit for bit -----------------------------------
@pytest.mark.parametrize('n', rs.PARITY_SIZES)
def test_restatement_parity(engines, n):
    L = float(n)
    pool = rs.parity_pool(n)
    assert np.any(pool < 0) and np.any(pool >= L)
    d = rs.triple_spans(pool, L)
    eng = engines(n)
    for B in rs.PARITY_BINS:
        for D in rs.parity_spans(L):
            assert rs.num_ambiguous(pool, L, B, D, d=d) == 0
            ref = rs.counts_from_spans(d, L, B, D)
            check_counts(eng.triple_distribution(pool, B, D), ref, n)
    # max_span=None is L/2
    assert np.array_equal(eng.triple_distribution(pool, 7),
                          eng.triple_distribution(pool, 7, 0.5 * L))


@pytest.mark.parametrize('n', [1, 2])
def test_fewer_than_three_particles(engines, n):
    rng = np.random.RandomState(n)
    pos = 3.0 * n * rng.random_sample((5, n)) - n
    for B, D in ((1, None), (64, 0.125 * n)):
        T = engines(n).triple_distribution(pos, B, D)
        assert T.shape == (5, B + 1) and T.dtype == np.uint32
        assert not T.any()


# ---- 2. the exact lattice ---------------------------------------------------
@pytest.mark.parametrize('n', [64, 512])
def test_exact_lattice(engines, n):
    L = float(n)
    rng = np.random.RandomState(n)
    pos = np.stack([np.arange(n, dtype=np.float64),
                    rng.permutation(n).astype(np.float64),
                    np.arange(n, dtype=np.float64) - 3 * L])
    eng = engines(n)
    for B in (1, 2, 16, 256, 4096):
        for D in (L / 2, L / 4):
            want = rs.lattice_counts(n, L, B, D)
            T = eng.triple_distribution(pos, B, D)
            check_counts(T, np.broadcast_to(want, T.shape), n)


# ---- 3. ties ------------------------------------------------------------------
def test_ties(engines):
    n, L = 64, 64.0
    eng = engines(n)
    rng = np.random.RandomState(5)
    # all particles at one point: everything in bin 0
    for at in (0.0, 23.375, 63.999, -1.0):
        for B, D in ((1, None), (32, None), (4096, L / 8)):
            T = eng.triple_distribution(np.full((3, n), at), B, D)
            assert np.all(T[:, 0] == comb(n, 3)) and not T[:, 1:].any()
    # coincident particles on the 1/8 grid: exact, and index ties all round
    grid = rs.grid_pool()
    for B in (1, 16, 256, 4096):
        for D in (L / 2, L / 4):
            ref = rs.triple_counts(grid, L, B, D)
            T = eng.triple_distribution(grid, B, D)
            check_counts(T, ref, n)
            for shift in (64.0, -192.0):
                assert np.array_equal(
                    eng.triple_distribution(grid + shift, B, D), T)
    # the order of the particles is irrelevant
    pool = np.concatenate([grid, rs.nesting_pool(n)])
    for B, D in ((16, None), (33, 0.3 * L)):
        T = eng.triple_distribution(pool, B, D)
        for _ in range(3):
            perm = rng.permutation(n)
            assert np.array_equal(eng.triple_distribution(pool[:, perm], B, D),
                                  T)
    # N = 3 and 4 at one point and in coincident pairs (lane groups of 8)
    for k in (3, 4):
        e = engines(k)
        T = e.triple_distribution(np.full((9, k), 0.25 * k), 8)
        assert np.all(T[:, 0] == comb(k, 3)) and not T[:, 1:].any()
        pairs = np.array([[0.5, 0.5, 1.0, 1.0][:k]] * 2)
        check_counts(e.triple_distribution(pairs, 8),
                     rs.triple_counts(pairs, float(k), 8), k)


# ---- 4. nesting ---------------------------------------------------------------
@pytest.mark.parametrize('n', [16, 37, 64, 128])
def test_nesting(engines, n):
    L = float(n)
    pool = rs.nesting_pool(n)
    eng = engines(n)
    for B in (1, 5, 32):
        assert rs.num_ambiguous(pool, L, B, L / 4) == 0
        assert rs.num_ambiguous(pool, L, 2 * B, L / 2) == 0
        inner = eng.triple_distribution(pool, B, L / 4).astype(np.int64)
        outer = eng.triple_distribution(pool, 2 * B, L / 2).astype(np.int64)
        assert np.array_equal(inner[:, :B], outer[:, :B])
        assert np.array_equal(inner[:, B], outer[:, B:].sum(axis=1))
        check_counts(inner.astype(np.uint32),
                     rs.triple_counts(pool, L, B, L / 4), n)


# ---- 5. one path, many doors ------------------------------------------------
@pytest.mark.parametrize('n,B,frac', rs.ENTRY_CASES)
def test_entry_points_agree(engines, n, B, frac):
    from phd_qmclib_amd.engine import DeviceBuffer, VmcEnsemble
    eng = engines(n)
    L, D, K = float(n), frac * n, B + 1
    pos, rng = rs.entry_pool(n)
    W = len(pos)                  # 70: no multiple of the rows of a wavefront
    T = eng.triple_distribution(pos, B, D)
    check_counts(T, rs.triple_counts(pos, L, B, D), n)
    Ti = T.astype(np.int64)
    dpos = _dev(eng, pos)
    assert np.array_equal(counts_dev(eng, dpos, W, B, D), T)
    # the reduction, unit weights: the first column exact
    dsums = DeviceBuffer((K, 2), eng.device)
    dws = DeviceBuffer((1,), eng.device)
    eng.triple_distribution_reduce_dev(W, dpos.ptr, None, B, D, dsums.ptr,
                                       dws.ptr)
    eng.sync()
    s1, w1 = dsums.download(), dws.download()
    assert w1[0] == W
    assert np.array_equal(s1[:, 0], Ti.sum(axis=0))
    assert close(s1[:, 1], (Ti ** 2).sum(axis=0))
    # random positive weights; the same bits twice
    w = 0.25 + rng.random_sample(W)
    dw = _dev(eng, w)
    eng.triple_distribution_reduce_dev(W, dpos.ptr, dw.ptr, B, D, dsums.ptr,
                                       dws.ptr)
    eng.sync()
    sw, ww = dsums.download(), dws.download()
    eng.triple_distribution_reduce_dev(W, dpos.ptr, dw.ptr, B, D, dsums.ptr,
                                       dws.ptr)
    eng.sync()
    assert np.array_equal(dsums.download(), sw)
    assert close(ww[0], w.sum())
    assert close(sw[:, 0], (w[:, None] * Ti).sum(axis=0))
    assert close(sw[:, 1], (w[:, None] * Ti ** 2).sum(axis=0))
    mean = eng.triple_distribution_weighted(pos, w, B, D)
    assert mean.shape == (K,)
    assert close(mean, (w[:, None] * Ti).sum(axis=0) / w.sum())
    # the VMC ensemble's resident rows, as uploaded
    v = VmcEnsemble(eng, W, 0.125, rng_seed=1)
    v.set_state(pos)
    parts = v.triple_dist_parts(B, D)
    v.close()
    assert np.array_equal(parts[:, 0], Ti.sum(axis=0))
    assert close(parts[:, 1], (Ti ** 2).sum(axis=0))
    for b in (dpos, dsums, dws, dw):
        b.close()


def test_reduce_spans_tiles(engines):
    """More than one tile of 2^16 configurations; at B = 4096 the tile is
    2^24 // 4097 = 4095, so 4097 configurations span two as well.  Neither
    count is a multiple of the 4 (G = 16) configurations of a wavefront."""
    from phd_qmclib_amd.engine import DeviceBuffer
    n, L = 16, 16.0
    eng = engines(n)
    pool, rng = rs.entry_pool(n)
    for W, B, D in (((1 << 16) + 4097, 33, 0.5 * L), (4097, 4096, 0.125 * L)):
        assert rs.num_ambiguous(pool, L, B, D) == 0
        ref = rs.triple_counts(pool, L, B, D)
        idx = rng.randint(0, len(pool), size=W)
        pos = pool[idx]
        w = 0.25 + rng.random_sample(W)
        dpos, dw = _dev(eng, pos), _dev(eng, w)
        dsums = DeviceBuffer((B + 1, 2), eng.device)
        dws = DeviceBuffer((1,), eng.device)
        eng.triple_distribution_reduce_dev(W, dpos.ptr, None, B, D, dsums.ptr,
                                           dws.ptr)
        eng.sync()
        s1 = dsums.download()
        assert dws.download()[0] == W
        assert np.array_equal(s1[:, 0], ref[idx].sum(axis=0))
        assert close(s1[:, 1], (ref[idx] ** 2).sum(axis=0))
        eng.triple_distribution_reduce_dev(W, dpos.ptr, dw.ptr, B, D,
                                           dsums.ptr, dws.ptr)
        eng.sync()
        sw = dsums.download()
        assert close(dws.download()[0], w.sum())
        assert close(sw[:, 0], (w[:, None] * ref[idx]).sum(axis=0))
        assert close(sw[:, 1], (w[:, None] * ref[idx] ** 2).sum(axis=0))
        # the host entry point on the same rows
        if W == 4097:
            assert np.array_equal(
                eng.triple_distribution(pos, B, D).astype(np.int64), ref[idx])
        for b in (dpos, dw, dsums, dws):
            b.close()


# ---- 6. the resident rows of a VMC ensemble ----------------------------------
@pytest.mark.parametrize('move', ['all', 'particle'])
@pytest.mark.parametrize('n', [16, 64])
def test_vmc_resident_rows(golden_params, n, move):
    from phd_qmclib_amd.mrbp_qmc import vmc
    spec = spec_for(golden_params, n)
    L, W, B, D = float(n), 64, 16, 0.25 * n
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21,
                             move=move)
    s.init_random(seed=3)
    for _ in islice(s.blocks(4), 2):
        pass
    before = s.ensemble.get_state()
    d, mean, err = s.triple_distribution(B, D)
    parts = s.ensemble.triple_dist_parts(B, D)
    after = s.ensemble.get_state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    confs = s.confs()
    s.close()
    assert rs.num_ambiguous(confs, L, B, D) == 0
    T = rs.triple_counts(confs, L, B, D)
    assert parts.shape == (B + 1, 2)
    assert np.array_equal(parts[:, 0], T.sum(axis=0))
    assert close(parts[:, 1], (T ** 2).sum(axis=0))
    assert np.array_equal(d, rs.bin_centres(L, B, D))
    assert mean.shape == err.shape == (B,)
    assert np.allclose(mean, rs.normalise(T.mean(axis=0), n, L, D),
                       rtol=1e-13, atol=0)
    want_err = rs.normalise(np.sqrt(T.var(axis=0) / (W - 1)), n, L, D)
    assert np.allclose(err, want_err, rtol=1e-9, atol=1e-12)


# ---- 7. DMC mixed estimate -------------------------------------------------
def test_dmc_mixed_estimate(golden_params, golden_kernels):
    from phd_qmclib_amd.mrbp_qmc import dmc
    n, B, D = 16, 12, 4.0
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
    assert 0 < nw < 96
    weight = state.props.weight.copy()
    weight[nw:] = 1e9               # dead slots must not count
    live = np.asarray(state.confs)[:nw, 0, :]
    garbage = np.asarray(state.confs).copy()
    garbage[nw:] = 0.123
    state = state._replace(confs=garbage,
                           props=state.props._replace(weight=weight))
    d, g3 = s.triple_distribution(state, B, D)
    assert rs.num_ambiguous(live, 16.0, B, D) == 0
    T = rs.triple_counts(live, 16.0, B, D)
    want = rs.normalise((weight[:nw, None] * T).sum(axis=0)
                        / weight[:nw].sum(), n, 16.0, D)
    assert d.shape == g3.shape == (B,)
    assert np.array_equal(d, rs.bin_centres(16.0, B, D))
    assert close(g3, want)
    d2, g3_half = s.triple_distribution(state, B)
    assert np.array_equal(d2, rs.bin_centres(16.0, B))


# ---- 8. Python surface and the C-level errors ---------------------------------
def test_physical_funcs_and_errors(engines, golden_params):
    from phd_qmclib_amd import _lib, mrbp_qmc
    from phd_qmclib_amd._lib import ptr
    n, L, B, D = 37, 37.0, 16, 0.3 * 37
    spec = spec_for(golden_params, n)
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec)
    pos = rs.entry_pool(n)[0][:8]
    confs = np.zeros((8, 2, n))
    confs[:, 0, :] = pos
    assert rs.num_ambiguous(pos, L, B, D) == 0
    want = rs.normalise(rs.triple_counts(pos, L, B, D), n, L, D)
    out = pf.triple_distribution(B, confs, D)
    assert out.shape == (8, B)
    assert np.allclose(out, want, rtol=1e-14, atol=0)
    assert np.array_equal(
        pf.triple_distribution(B, confs.reshape(2, 4, 2, n), max_span=D),
        out.reshape(2, 4, B))
    one = pf.triple_distribution(B, confs[3], D)
    assert one.shape == (B,) and np.array_equal(one, out[3])
    # bad arguments
    eng = engines(n)
    for bad in (0, -3, 4097):
        with pytest.raises(ValueError):
            eng.triple_distribution(pos, bad)
        with pytest.raises(ValueError):
            pf.triple_distribution(bad, confs)
    for bad in (0.0, -1.0, 0.5 * L + 1e-9, L):
        with pytest.raises(ValueError):
            eng.triple_distribution(pos, B, bad)
        with pytest.raises(ValueError):
            eng.triple_distribution_weighted(pos, np.ones(8), B, bad)
    with pytest.raises(ValueError):
        eng.triple_distribution(pos[:, :36], B)
    with pytest.raises(ValueError):
        eng.triple_distribution_weighted(pos, np.ones(7), B)
    lib = _lib.load()
    p = np.ascontiguousarray(pos)
    cnt = np.zeros((8, B + 1), dtype=np.uint32)
    cp = ptr(cnt, _lib._u32p)
    for args in ((ptr(p), 0, D, cp), (ptr(p), 4097, D, cp),
                 (ptr(p), B, 0.0, cp), (ptr(p), B, -1.0, cp),
                 (ptr(p), B, 0.5 * L + 1e-9, cp),
                 (ptr(p), B, float('nan'), cp),
                 (None, B, D, cp), (ptr(p), B, D, None)):
        assert lib.qmc_triple_dist(eng._h, 8, *args) != 0
        assert b'qmc_triple_dist' in lib.qmc_last_error()
    assert lib.qmc_triple_dist(eng._h, 8, ptr(p), B, L, cp) != 0
    assert b'max_span' in lib.qmc_last_error()
    assert lib.qmc_triple_dist(eng._h, -1, ptr(p), B, D, cp) != 0
    assert lib.qmc_triple_dist_dev(eng._h, 1, None, B, D, None) != 0
    assert lib.qmc_triple_dist_reduce_dev(eng._h, 1, None, None, 0, D, None,
                                          None) != 0
    assert lib.qmc_vmc_triple_dist(None, B, D, None) != 0
    assert not cnt.any()
    # max_span = L/2 exactly is legal; the engine still works afterwards
    T = eng.triple_distribution(pos, 1, 0.5 * L)
    assert np.all(T.sum(axis=1) == comb(n, 3))


# ---- 9. the law of uniform particles ----------------------------------------
def test_uniform_law(engines):
    """|z| <= 4 on all 32 bins, z from the sample standard deviation over the
    4096 configurations (the restatement alone gives max |z| = 1.9)."""
    u = pd.UNIFORM_LAW
    n, L, B = u['n'], u['sc_size'], u['num_bins']
    pos = pd.uniform_law_inputs()
    T = engines(n).triple_distribution(pos, B)
    assert T.shape == (u['nconf'], B + 1)
    assert np.all(T.sum(axis=1, dtype=np.int64) == comb(n, 3))
    assert rs.num_ambiguous(pos[:64], L, B) == 0
    assert np.array_equal(T[:64].astype(np.int64),
                          rs.triple_counts(pos[:64], L, B))
    z = rs.uniform_law_z(T, n, L, B)
    print('uniform law on the device: max |z| = %.2f' % np.abs(z).max())
    assert np.all(np.abs(z) <= 4.0)
