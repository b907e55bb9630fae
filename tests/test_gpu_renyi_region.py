"""Replica swap of regions made of up to two segments, and the charge-resolved
reduction, on the GPU (csrc/qmc_renyi_region.h) against the NumPy restatement
of the definition (tests/_renyi_region_restatement.py) with the C oracle's
wf_abs_log on explicitly swapped configurations.  All tests need a GPU.

The occupations n_x are integers and compared for EQUALITY: no input has a
particle on a mark to within rounding (tests/test_renyi_region_host.py asserts
that without a GPU, the tests here assert it again).  log_ratio is compared
as tests/test_gpu_renyi.py does,

    |dev - ref| <= 2e-11 max(1, sum of the |four ln psi terms|),

and unmatched entries are -inf exactly.  The reduction is held against NumPy
sums of the per-pair rows: the integer columns exactly, the swap columns to
rtol 1e-11 (the figure of tests/test_gpu_energy_parts.py for its reduction).
"""
from itertools import islice

import numpy as np
import pytest

from . import _renyi_region_restatement as rr
from . import _renyi_restatement as rs
from ._models import _dev
from .test_gpu_renyi import models, spec_for, swap_of        # noqa: F401

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-11


@pytest.fixture(scope='module')
def references(models):
    """(key, case name) -> (n_x, log_ratio, scale) of the explicit route,
    computed once and shared; nobody writes into them."""
    cache = {}

    def get(key, name, pos, regions, origin):
        if (key, name) not in cache:
            _, wf, _, L = models(key)
            out = rr.reference(wf, pos, L, regions, origin)
            for a in out:
                a.setflags(write=False)
            cache[(key, name)] = out
        return cache[(key, name)]
    return get


def check_parity(eng, ref, pos, regions, origin, label):
    n_ref, lr_ref, scale = ref
    n_x, lr = eng.renyi_region_swap(pos, regions, origin)
    assert n_x.dtype == np.int32 and n_x.shape == n_ref.shape
    assert lr.dtype == np.float64 and lr.shape == lr_ref.shape
    assert np.array_equal(n_x, n_ref)
    ok, worst = rr.within_tolerance(lr, lr_ref, scale)
    print('%s: %d matched entries, worst error / bound = %.3g'
          % (label, int(np.isfinite(lr_ref).sum()), worst))
    assert ok
    return n_x, lr


def numpy_sums(n_x, lr, num_charges):
    """sums[K, 3 + 2Q] of the per-pair rows, as the definition has them."""
    swap = swap_of(lr)
    K = lr.shape[1]
    out = np.zeros((K, 3 + 2 * num_charges))
    out[:, 0] = swap.sum(axis=0)
    out[:, 1] = (swap ** 2).sum(axis=0)
    out[:, 2] = np.isfinite(lr).sum(axis=0)
    for c in range(num_charges):
        out[:, 3 + 2 * c] = (swap * (n_x[0::2] == c)).sum(axis=0)
        out[:, 4 + 2 * c] = (n_x == c).sum(axis=0)
    return out


def assert_sums(got, want):
    """The integer columns exactly, the swap columns to SUM_RTOL."""
    assert got.shape == want.shape
    assert np.array_equal(got[:, 2], want[:, 2])
    assert np.array_equal(got[:, 4::2], want[:, 4::2])
    for cols in (slice(0, 2), slice(3, None, 2)):
        assert np.allclose(got[:, cols], want[:, cols], rtol=SUM_RTOL, atol=0)


def reduce_dev(eng, dpos, W, dreg, K, origin, Q):
    from phd_qmclib_amd.engine import DeviceBuffer
    dsums = DeviceBuffer((K, 3 + 2 * Q), eng.device)
    eng.renyi_region_swap_reduce_dev(W, dpos.ptr, K, dreg.ptr, origin, Q,
                                     dsums.ptr)
    eng.sync()
    out = dsums.download()
    dsums.close()
    return out


# ---- 1. parity with the definition --------------------------------------------
@pytest.mark.parametrize('n', rr.PARITY_SIZES)
def test_parity(models, references, n):
    eng, _, nn, L = models(n)
    assert nn == n and L == float(n)
    for origin, regions, pos in rr.parity_cases(n):
        rr.assert_pool_conditions(pos, L, regions, origin)
        ref = references(n, origin, pos, regions, origin)
        _, lr = check_parity(eng, ref, pos, regions, origin,
                             'N=%d origin=%g' % (n, origin))
        # the entries a prefix cannot represent are among those compared
        assert np.all(np.isfinite(
            lr[rr.split_differently(pos, L, regions, origin)]))


def test_parity_many_regions(models, references):
    """130 regions: more than the wavefront has lanes."""
    origin, regions, pos = rr.many_regions_case()
    eng, _, n, L = models(16)
    rr.assert_pool_conditions(pos, L, regions, origin)
    ref = references(16, 'many', pos, regions, origin)
    check_parity(eng, ref, pos, regions, origin, 'N=16 K=130')


def test_parity_n512(models, references):
    """N = 512: the four rows of the one-segment test's large case."""
    origin, regions, pos = rr.large_case()
    eng, _, n, L = models(512)
    amb, hit, miss, split = rr.pool_conditions(pos, L, regions, origin)
    assert amb == 0 and hit >= 4 and miss >= 1 and split >= 1
    ref = references(512, 'large', pos, regions, origin)
    check_parity(eng, ref, pos, regions, origin, 'N=512, 2 pairs')


def test_n512_with_4096_regions(models, references):
    """The largest LDS footprint (88 KB): N = 512, the largest N of an engine,
    with 4096 regions, whose last five are those of the parity case.  An
    entry's result does not depend on the other entries of the call, so those
    five columns carry the bits of the call with 5 regions; the occupations
    are exact at every entry, and a sample of the other matched entries is
    held against the explicit route."""
    origin, regions, pos = rr.large_case()
    eng, wf, n, L = models(512)
    many = np.concatenate([rr.many_regions(512, 4091), regions])
    assert len(many) == 4096
    assert len(rr.ambiguous(pos, L, many, origin)) == 0
    n5, lr5 = eng.renyi_region_swap(pos, regions, origin)
    n_x, lr = eng.renyi_region_swap(pos, many, origin)
    in_x, n_ref = rr.membership(pos, L, many, origin)
    assert np.array_equal(n_x, n_ref)
    ok = rr.matched(n_x)
    assert np.array_equal(np.isneginf(lr), ~ok)
    assert np.array_equal(n_x[:, -5:], n5)
    assert np.array_equal(lr[:, -5:], lr5)
    split = rr.split_differently(pos, L, many, origin)
    sample = ([(0, k) for k in np.flatnonzero(ok[0, :4091])[::100][:3]]
              + [(1, k) for k in np.flatnonzero(split[1, :4091])[::30][:3]])
    assert len(sample) == 6
    z = rs.wrap(pos, L)
    for p, k in sample:
        want, scale = rr.explicit_log_ratio(
            wf, z[2 * p], z[2 * p + 1], in_x[2 * p, :, k],
            in_x[2 * p + 1, :, k])
        assert abs(lr[p, k] - want) <= rr.RTOL * max(1.0, scale), (p, k)


def test_parity_without_lattice(models, references):
    """free16: interacting particles and no one-body factor."""
    eng, _, n, L = models('free16')
    origin, regions, pos = rr.parity_cases(16)[1]
    ref = references('free16', 'free', pos, regions, origin)
    check_parity(eng, ref, pos, regions, origin, 'free16')


# ---- 2. exact cases ---------------------------------------------------------------
def test_no_interaction_is_exactly_zero(models):
    """ideal16: every matched entry is exactly 0.0 and the swap sums are the
    match counts, charge by charge."""
    eng, _, n, L = models('ideal16')
    assert n == 16 and L == 16.0
    for origin, regions, pos in rr.parity_cases(16):
        _, n_ref = rr.membership(pos, L, regions, origin)
        ok = rr.matched(n_ref)
        n_x, lr = eng.renyi_region_swap(pos, regions, origin)
        assert np.array_equal(n_x, n_ref)
        assert np.array_equal(np.isneginf(lr), ~ok)
        assert np.all(lr[ok] == 0.0)
        dpos, dreg = _dev(eng, pos), _dev(eng, regions)
        sums = reduce_dev(eng, dpos, len(pos), dreg, 5, origin, n + 1)
        assert np.array_equal(sums, numpy_sums(n_x, lr, n + 1))
        assert np.array_equal(sums[:, 0], ok.sum(axis=0))
        dpos.close()
        dreg.close()


@pytest.mark.parametrize('n', [16, 64, 100])
def test_everything_inside_or_outside_is_exactly_zero(models, n):
    """Regions that hold every particle of both replicas, in one window and in
    two, and one that holds none: no pair crosses the cut."""
    eng, _, _, L = models(n)
    rng = np.random.RandomState(n)
    pos = 0.05 * L + 0.85 * L * rng.random_sample((6, n))
    pos[1] += 2 * L
    regions = L * np.array([[0.97, 0.0, 0.0], [0.5, 0.0, 0.47],
                            [0.04, 0.87, 0.05], [0.3, 0.1, 0.2]])
    assert len(rr.ambiguous(pos, L, regions, 0.0)) == 0
    n_x, lr = eng.renyi_region_swap(pos, regions, 0.0)
    assert np.all(n_x[:, :2] == n) and not n_x[:, 2].any()
    assert np.all(lr[:, :3] == 0.0)
    assert np.all((n_x[:, 3] > 0) & (n_x[:, 3] < n))


# ---- 3. the one-segment kernel -------------------------------------------------------
@pytest.mark.parametrize('n', [16, 64, 100, 128])
def test_single_segments_agree_with_renyi_swap(models, n):
    """l2 = 0 entries against `ModelEngine.renyi_swap` on the same input."""
    eng, wf, _, L = models(n)
    K, origin, lengths, pos = rs.parity_cases(n)[3]
    regions = np.stack([lengths, 0.01 * L * np.arange(K), np.zeros(K)],
                       axis=1)
    assert len(rr.ambiguous(pos, L, regions, origin)) == 0
    n_a, lr_a = eng.renyi_swap(pos, lengths, origin)
    n_x, lr_x = eng.renyi_region_swap(pos, regions, origin)
    assert np.array_equal(n_x, n_a)
    assert np.isfinite(lr_a).sum() >= 8
    _, _, scale = rs.reference(wf, pos, L, lengths, origin)
    ok, worst = rr.within_tolerance(lr_x, lr_a, scale)
    print('N=%d: new against old, worst difference / bound = %.3g'
          % (n, worst))
    assert ok


# ---- 4. one path, many doors --------------------------------------------------------
@pytest.mark.parametrize('n', [16, 37, 64, 100])
def test_entry_points_agree(models, n):
    from phd_qmclib_amd.engine import DeviceBuffer
    eng, _, _, L = models(n)
    origin, regions, pos = rr.parity_cases(n)[1]
    K, W, P = len(regions), len(pos), len(pos) // 2
    n_x, lr = eng.renyi_region_swap(pos, regions, origin)
    dpos, dreg = _dev(eng, pos), _dev(eng, regions)
    # the device entry point: the same bits, and either output alone
    dnx = DeviceBuffer(((W * K + 1) // 2,), eng.device)       # int32 pairs
    dlr = DeviceBuffer((P, K), eng.device)
    eng.renyi_region_swap_dev(W, dpos.ptr, K, dreg.ptr, origin, dnx.ptr,
                              dlr.ptr)
    eng.sync()
    got_n = dnx.download().view(np.int32)[:W * K].reshape(W, K)
    assert np.array_equal(got_n, n_x)
    assert np.array_equal(dlr.download(), lr)
    dlr.upload(np.full((P, K), 7.0))
    eng.renyi_region_swap_dev(W, dpos.ptr, K, dreg.ptr, origin, None, dlr.ptr)
    eng.sync()
    assert np.array_equal(dlr.download(), lr)
    dnx.upload(np.zeros(dnx.shape))
    eng.renyi_region_swap_dev(W, dpos.ptr, K, dreg.ptr, origin, dnx.ptr, None)
    eng.sync()
    assert np.array_equal(
        dnx.download().view(np.int32)[:W * K].reshape(W, K), n_x)
    # the reduction: NumPy sums of the per-pair rows, every charge, a few,
    # none; the same bits twice
    full = reduce_dev(eng, dpos, W, dreg, K, origin, n + 1)
    assert_sums(full, numpy_sums(n_x, lr, n + 1))
    assert np.array_equal(reduce_dev(eng, dpos, W, dreg, K, origin, n + 1),
                          full)
    assert np.array_equal(full[:, 4::2].sum(axis=1), np.full(K, float(W)))
    assert np.allclose(full[:, 3::2].sum(axis=1), full[:, 0], rtol=SUM_RTOL,
                       atol=0)
    some = reduce_dev(eng, dpos, W, dreg, K, origin, 3)
    assert np.array_equal(some, full[:, :9])
    none = reduce_dev(eng, dpos, W, dreg, K, origin, 0)
    assert np.array_equal(none, full[:, :3])
    for b in (dpos, dreg, dnx, dlr):
        b.close()


def test_reduce_spans_tiles(models):
    """More than 2^16 pairs at N = 2: the reduction works in two tiles and
    adds them up in order."""
    n, P = 2, (1 << 16) + 3
    eng, _, _, L = models(n)
    rng = np.random.RandomState(65536)
    pos = L * rng.random_sample((2 * P, n))
    regions = L * np.array([[0.3, 0.2, 0.25], [0.45, 0.0, 0.0],
                            [0.1, 0.0, 0.6]])
    origin = 0.125
    n_x, lr = eng.renyi_region_swap(pos, regions, origin)
    assert np.array_equal(n_x, rr.membership(pos, L, regions, origin)[1])
    ok = np.isfinite(lr)
    assert np.array_equal(ok, rr.matched(n_x)) and np.any(~ok)
    # the last pairs, in the second tile, as a batch of their own
    n_last, lr_last = eng.renyi_region_swap(pos[-6:], regions, origin)
    assert np.array_equal(n_last, n_x[-6:])
    assert np.array_equal(lr_last, lr[-3:])
    dpos, dreg = _dev(eng, pos), _dev(eng, regions)
    sums = reduce_dev(eng, dpos, 2 * P, dreg, 3, origin, n + 1)
    assert_sums(sums, numpy_sums(n_x, lr, n + 1))
    assert np.array_equal(sums[:, 4::2].sum(axis=1), np.full(3, 2.0 * P))
    assert np.array_equal(reduce_dev(eng, dpos, 2 * P, dreg, 3, origin, n + 1),
                          sums)
    dpos.close()
    dreg.close()


def test_physical_funcs_broadcast(models, golden_params):
    from phd_qmclib_amd import mrbp_qmc
    n = 37
    eng, _, _, L = models(n)
    origin, regions, pos = rr.parity_cases(n)[1]
    K = len(regions)
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec_for(golden_params, n))
    _, lr = eng.renyi_region_swap(pos, regions, origin)
    want = swap_of(lr)
    P = len(pos) // 2
    assert P == 12 and np.any(want == 0.0) and np.any(want > 0.0)
    confs = np.zeros((P, 2, 2, n))
    confs[:, :, 0, :] = pos.reshape(P, 2, n)
    out = pf.renyi_region_swap(regions, confs, origin)
    assert out.shape == (P, K) and np.array_equal(out, want)
    out = pf.renyi_region_swap(regions, confs.reshape(3, 4, 2, 2, n),
                               origin=origin)
    assert np.array_equal(out, want.reshape(3, 4, K))
    one = pf.renyi_region_swap(regions, confs[5], origin)
    assert one.shape == (K,) and np.array_equal(one, want[5])
    for bad in (confs[0, 0], confs[:, :1], np.zeros((P, 3, 2, n))):
        with pytest.raises(ValueError):
            pf.renyi_region_swap(regions, bad, origin)


# ---- 5. the resident rows of a VMC ensemble ------------------------------------------
@pytest.mark.parametrize('move', ['all', 'particle'])
def test_vmc_resident_rows(golden_params, models, move):
    from phd_qmclib_amd import engine
    from phd_qmclib_amd.mrbp_qmc import vmc
    n, W = 16, 64
    spec = spec_for(golden_params, n)
    L, P = float(n), W // 2
    lengths, origin = rs.parity_lengths(n, 5), -0.5 * spec.barrier_width
    length, second = 3.0, 2.0
    separations = np.array([1.0, 4.0, 1.0, 7.5])        # one of them twice
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21,
                             move=move)
    s.init_random(seed=3)
    for _ in islice(s.blocks(4), 2):
        pass
    before = s.ensemble.get_state()
    res = s.renyi_entropy_resolved(lengths, origin)
    few = s.renyi_entropy_resolved(lengths, origin, num_charges=4)
    calls = []
    parts_of = s.ensemble.renyi_region_parts
    s.ensemble.renyi_region_parts = lambda *a: (calls.append(a),
                                                parts_of(*a))[1]
    mi = s.renyi_mutual_information(length, separations, origin, second)
    del s.ensemble.renyi_region_parts
    after = s.ensemble.get_state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    confs = s.confs()
    s.close()
    eng = models(n)[0]

    # the charge-resolved entropies of single segments
    single = np.stack([lengths, np.zeros(5), np.zeros(5)], axis=1)
    assert len(rr.ambiguous(confs, L, single, origin)) == 0
    n_x, lr = eng.renyi_region_swap(confs, single, origin)
    assert np.array_equal(n_x, rr.membership(confs, L, single, origin)[1])
    want = engine.renyi_resolved(numpy_sums(n_x, lr, n + 1), P, n + 1)
    assert isinstance(res, engine.ResolvedRenyi)
    assert res.charge_prob.shape == (5, n + 1)
    assert np.array_equal(res.p_match, want.p_match) and res.p_match.sum() > 0
    assert np.array_equal(res.charge_prob, want.charge_prob)
    assert np.array_equal(res.charge_prob.sum(axis=1), np.ones(5))
    for got, ref in ((res.entropy, want.entropy),
                     (res.charge_swap, want.charge_swap),
                     (res.charge_entropy, want.charge_entropy)):
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        fin = np.isfinite(ref)
        assert np.allclose(got[fin], ref[fin], rtol=SUM_RTOL, atol=SUM_RTOL)
    assert np.allclose(res.charge_swap.sum(axis=1), np.exp(-res.entropy),
                       rtol=SUM_RTOL, atol=0)
    assert np.array_equal(few.entropy, res.entropy)
    assert np.array_equal(few.charge_swap, res.charge_swap[:, :4])
    assert np.array_equal(few.charge_prob, res.charge_prob[:, :4])

    # the mutual information: one call at the origin, one per distinct
    # separation
    assert len(calls) == 1 + 3
    sep, i2, i2_err, s_a, s_c, s_ac = mi
    assert np.array_equal(sep, separations)
    union = np.concatenate(
        [[[length, 0.0, 0.0]],
         [[length, g, second] for g in separations]])
    assert len(rr.ambiguous(confs, L, union, origin)) == 0
    n_u, lr_u = eng.renyi_region_swap(confs, union, origin)
    s2_u, err_u, _ = engine.renyi_entropy(numpy_sums(n_u, lr_u, 0), P)
    s2_c, err_c = np.empty(4), np.empty(4)
    for i, g in enumerate(separations):
        a0 = origin + length + g
        assert len(rr.ambiguous(confs, L, [[second, 0.0, 0.0]], a0)) == 0
        n_c, lr_c = eng.renyi_region_swap(confs, [[second, 0.0, 0.0]], a0)
        out = engine.renyi_entropy(numpy_sums(n_c, lr_c, 0), P)
        s2_c[i], err_c[i] = out[0][0], out[1][0]
    want_i2, want_err = engine.renyi_mutual_information(
        s2_u[0], s2_c, s2_u[1:], err_u[0], err_c, err_u[1:])
    assert np.isfinite(s_a) and np.all(np.isfinite(s_c))
    for got, ref in ((s_a, s2_u[0]), (s_c, s2_c), (s_ac, s2_u[1:]),
                     (i2, want_i2), (i2_err, want_err)):
        got, ref = np.asarray(got), np.asarray(ref)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin)
        assert np.allclose(got[fin], ref[fin], rtol=1e-9, atol=1e-9)
    assert s_c[0] == s_c[2] and i2[0] == i2[2]


def test_vmc_odd_number_of_chains(golden_params):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    from phd_qmclib_amd.mrbp_qmc import vmc
    spec = spec_for(golden_params, 16)
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, 63, rng_seed=2)
    s.init_random(seed=1)
    with pytest.raises(ValueError):
        s.renyi_entropy_resolved([4.0])
    with pytest.raises(ValueError):
        s.renyi_mutual_information(2.0, [1.0, 3.0])
    with pytest.raises(ValueError):
        s.ensemble.renyi_region_parts([[4.0, 1.0, 2.0]])
    lib = _lib.load()
    rg, out = np.array([[4.0, 1.0, 2.0]]), np.zeros((1, 3))
    assert lib.qmc_vmc_renyi_region_swap(s.ensemble._h, 1, ptr(rg), 0.0, 0,
                                         ptr(out)) != 0
    assert b'qmc_vmc_renyi_region_swap' in lib.qmc_last_error()
    assert not out.any()
    s.close()


# ---- 6. the known answer of free particles ---------------------------------------------
def test_known_answer():
    """N = L = 8 without interactions, 4096 pairs of uniform rows: the count
    of a row in X is binomial with x = (l1 + l2) / L, so <swap> = sum_n
    pmf(n)^2, charge_prob[n] = pmf(n) and charge_swap[n] = pmf(n)^2, each
    within 4 binomial standard errors, the number that
    tests/test_gpu_renyi.py::test_known_answer allows (the restatement alone:
    max |z| = 2.61)."""
    from phd_qmclib_amd import engine
    from phd_qmclib_amd.mrbp_qmc import Spec
    k = rs.KNOWN
    n, P = k['n'], k['nconf'] // 2
    args = rs.model_spec_args(n)
    args['interaction_strength'] = 0
    eng = engine.ModelEngine(Spec(**args).cfc_spec)
    pos = rs.known_answer_inputs()
    regions = np.array(rr.KNOWN_REGIONS)
    dpos, dreg = _dev(eng, pos), _dev(eng, regions)
    for origin in k['origins']:
        assert len(rr.ambiguous(pos, k['sc_size'], regions, origin)) == 0
        sums = reduce_dev(eng, dpos, len(pos), dreg, 3, origin, n + 1)
        _, n_ref = rr.membership(pos, k['sc_size'], regions, origin)
        assert np.array_equal(sums[:, 2], rr.matched(n_ref).sum(axis=0))
        res = engine.renyi_resolved(sums, P, n + 1)
        zs = rr.known_z(res.charge_swap * P, res.charge_prob * 2 * P,
                        np.exp(-res.entropy) * P, P)
        for name, z in zip(('swap', 'charge_prob', 'charge_swap'), zs):
            print('known answer, origin %g, %s: max |z| = %.2f'
                  % (origin, name, np.abs(z).max()))
            assert np.all(np.abs(z) <= 4.0)
    dpos.close()
    dreg.close()
    eng.close()


# ---- 7. errors ----------------------------------------------------------------------------
def test_errors(models):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    from phd_qmclib_amd.engine import DeviceBuffer
    n = 16
    eng, _, _, L = models(n)
    origin, regions, pos = rr.parity_cases(n)[0]
    K = len(regions)
    for bad in (pos[:5], pos[:1], pos[:0], pos[:, :15]):
        with pytest.raises(ValueError):
            eng.renyi_region_swap(bad, regions, origin)
    for bad in ([[0.0, 1.0, 1.0]], [[1.0, -1.0, 1.0]], [[L, 0.0, 0.0]],
                [[1.0, 2.0, L]], [[float('nan'), 0.0, 0.0]], [], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            eng.renyi_region_swap(pos, bad, origin)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            eng.renyi_region_swap(pos, regions, bad)
    lib = _lib.load()
    p = np.ascontiguousarray(pos)
    rg = np.ascontiguousarray(regions)
    W = len(p)
    n_x = np.zeros((W, K), dtype=np.int32)
    lr = np.zeros((W // 2, K))
    np_, lp = ptr(n_x, _lib._i32p), ptr(lr)

    def call(nconf=W, pos_=ptr(p), nreg=K, reg_=ptr(rg), a0=origin, nx=np_,
             out=lp):
        return lib.qmc_renyi_region_swap(eng._h, nconf, pos_, nreg, reg_, a0,
                                         nx, out)
    nan, inf = float('nan'), float('inf')
    bad_reg = [np.array([v] + [[1.0, 1.0, 1.0]] * (K - 1)) for v in
               ([0.0, 1.0, 1.0], [-2.0, 1.0, 1.0], [1.0, -1.0, 1.0],
                [1.0, 1.0, -1.0], [L, 0.0, 0.0], [1.0, L, 0.0],
                [6.0, 5.0, 5.0], [nan, 0.0, 0.0], [1.0, nan, 0.0],
                [1.0, 0.0, nan], [inf, 0.0, 0.0], [1.0, 0.0, inf])]
    for kwargs in ([dict(nconf=W - 1), dict(nconf=1), dict(nconf=0),
                    dict(nconf=-2), dict(nreg=0), dict(nreg=4097),
                    dict(a0=nan), dict(a0=inf), dict(pos_=None),
                    dict(reg_=None), dict(nx=None, out=None)]
                   + [dict(reg_=ptr(b)) for b in bad_reg]):
        assert call(**kwargs) != 0, kwargs
        assert b'qmc_renyi_region_swap' in lib.qmc_last_error()
    assert not n_x.any() and not lr.any()
    assert lib.qmc_renyi_region_swap_dev(eng._h, W - 1, None, K, None, origin,
                                         None, None) != 0
    assert b'qmc_renyi_region_swap_dev' in lib.qmc_last_error()
    assert lib.qmc_renyi_region_swap_reduce_dev(eng._h, W, None, K, None,
                                                origin, 0, None) != 0
    assert b'qmc_renyi_region_swap_reduce_dev' in lib.qmc_last_error()
    assert lib.qmc_vmc_renyi_region_swap(None, K, ptr(rg), origin, 0,
                                         None) != 0
    # the number of charges, on live device buffers
    dpos, dreg = _dev(eng, p), _dev(eng, rg)
    dsums = DeviceBuffer((K, 3 + 2 * (n + 1)), eng.device)
    for q in (-1, n + 2):
        assert lib.qmc_renyi_region_swap_reduce_dev(
            eng._h, W, dpos.ptr, K, dreg.ptr, origin, q, dsums.ptr) != 0
        assert b'num_charges' in lib.qmc_last_error()
        with pytest.raises(Exception):
            eng.renyi_region_swap_reduce_dev(W, dpos.ptr, K, dreg.ptr, origin,
                                             q, dsums.ptr)
    for nconf, nreg in ((W - 1, K), (0, K), (W, 0), (W, 4097)):
        assert lib.qmc_renyi_region_swap_reduce_dev(
            eng._h, nconf, dpos.ptr, nreg, dreg.ptr, origin, 0,
            dsums.ptr) != 0
    # either output alone is legal, and the engine still works afterwards
    assert call(nx=None) == 0 and call(out=None) == 0
    want_n, want_lr = eng.renyi_region_swap(pos, regions, origin)
    assert np.array_equal(n_x, want_n) and np.array_equal(lr, want_lr)
    full = reduce_dev(eng, dpos, W, dreg, K, origin, n + 1)
    assert_sums(full, numpy_sums(want_n, want_lr, n + 1))
    for b in (dpos, dreg, dsums):
        b.close()


def test_sums_size_limit(models):
    """nreg (3 + 2 Q) > 2^20 is refused; the largest that fits at N = 512 and
    4096 regions (Q = 126) runs."""
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd.engine import DeviceBuffer
    origin, regions, pos = rr.large_case()
    eng, _, n, L = models(512)
    many = np.concatenate([rr.many_regions(512, 4091), regions])
    lib = _lib.load()
    dpos, dreg = _dev(eng, pos), _dev(eng, many)
    dsums = DeviceBuffer((4096, 3 + 2 * 126), eng.device)
    assert lib.qmc_renyi_region_swap_reduce_dev(
        eng._h, 4, dpos.ptr, 4096, dreg.ptr, origin, 127, dsums.ptr) != 0
    assert b'2^20' in lib.qmc_last_error()
    sums = reduce_dev(eng, dpos, 4, dreg, 4096, origin, 126)
    n_x, lr = eng.renyi_region_swap(pos, many, origin)
    assert_sums(sums, numpy_sums(n_x, lr, 126))
    for b in (dpos, dreg, dsums):
        b.close()
