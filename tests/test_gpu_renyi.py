"""Renyi-2 entanglement entropy by replica swap on the GPU (csrc/qmc_renyi.h)
against the NumPy restatement of its definition (tests/_renyi_restatement.py)
with the C oracle's wf_abs_log on explicitly swapped configurations.  All
tests need a GPU.

The occupations n_a are integers and compared for EQUALITY: no input has a
particle on a cut to within rounding (tests/test_renyi_host.py asserts that
without a GPU, the tests here assert it again).  log_ratio is compared with

    |dev - ref| <= 2e-11 max(1, sum of the |four ln psi terms|),

the 2e-11 being the RTOL of tests/test_gpu_pair_dist.py and the scale what
the explicit route cancels against; the cross-pair form and the explicit route
agree to 6e-16 of that scale on the CPU, which leaves the margin to the
device's pair arithmetic.  Unmatched entries are -inf exactly.  Sums in
floating point use |delta| <= 2e-11 max(1, |x|).
"""
from itertools import islice

import numpy as np
import pytest

from . import _renyi_restatement as rs
from ._models import _dev

pytestmark = pytest.mark.gpu

RTOL = rs.RTOL


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


def spec_for(golden_params, key):
    """The golden model of that tag, the golden 'box' model of n particles
    where there is one, the same family otherwise (L = n)."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    if isinstance(key, str):
        if key == 'ideal_free16':      # no interaction and no lattice
            args = dict(golden_params['free16']['spec'])
            args['interaction_strength'] = 0
            return Spec(**args)
        return Spec(**golden_params[key]['spec'])
    if key in rs.GOLDEN_SIZES:
        return Spec(**golden_params[rs.GOLDEN_SIZES[key]]['spec'])
    return Spec(**rs.model_spec_args(key))


@pytest.fixture(scope='module')
def models(golden_params, oracle):
    """key -> (engine, wf_abs_log of the oracle, N, L), built once."""
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(key):
        if key not in cache:
            spec = spec_for(golden_params, key)
            eng = ModelEngine(spec.cfc_spec)
            om = oracle.model_from_cfc(spec.cfc_spec)
            cache[key] = (eng, lambda z: oracle.wf_abs_log(om, z),
                          spec.boson_number, float(spec.supercell_size))
        return cache[key]
    yield get
    for rec in cache.values():
        rec[0].close()


@pytest.fixture(scope='module')
def references(models):
    """(key, case name) -> (n_a, log_ratio, scale) of the explicit route,
    computed once and shared; nobody writes into them."""
    cache = {}

    def get(key, name, pos, lengths, origin):
        if (key, name) not in cache:
            _, wf, _, L = models(key)
            out = rs.reference(wf, pos, L, lengths, origin)
            for a in out:
                a.setflags(write=False)
            cache[(key, name)] = out
        return cache[(key, name)]
    return get


def check_parity(eng, ref, pos, lengths, origin, label):
    n_ref, lr_ref, scale = ref
    n_a, lr = eng.renyi_swap(pos, lengths, origin)
    assert n_a.dtype == np.int32 and n_a.shape == n_ref.shape
    assert lr.dtype == np.float64 and lr.shape == lr_ref.shape
    assert np.array_equal(n_a, n_ref)
    ok, worst = rs.within_tolerance(lr, lr_ref, scale)
    print('%s: %d matched entries, worst error / bound = %.3g'
          % (label, int(np.isfinite(lr_ref).sum()), worst))
    assert ok
    return n_a, lr


def swap_of(log_ratio):
    swap = np.exp(np.clip(log_ratio, -700.0, 700.0))
    swap[np.isneginf(log_ratio)] = 0.0
    return swap


def reduce_dev(eng, dpos, W, dlen, K, origin):
    from phd_qmclib_amd.engine import DeviceBuffer
    dsums = DeviceBuffer((K, 3), eng.device)
    eng.renyi_swap_reduce_dev(W, dpos.ptr, K, dlen.ptr, origin, dsums.ptr)
    eng.sync()
    out = dsums.download()
    dsums.close()
    return out


# ---- 1. parity with the definition --------------------------------------------
@pytest.mark.parametrize('n', rs.PARITY_SIZES)
def test_parity(models, references, n):
    eng, _, nn, L = models(n)
    assert nn == n and L == float(n)
    for K, origin, lengths, pos in rs.parity_cases(n):
        rs.assert_pool_conditions(pos, L, lengths, origin)
        ref = references(n, (K, origin), pos, lengths, origin)
        check_parity(eng, ref, pos, lengths, origin,
                     'N=%d K=%d origin=%g' % (n, K, origin))


def test_parity_many_lengths(models, references):
    """K = 130: more lengths than the wavefront has lanes."""
    K, origin, lengths, pos = rs.many_lengths_case()
    eng, _, n, L = models(16)
    rs.assert_pool_conditions(pos, L, lengths, origin)
    ref = references(16, 'many', pos, lengths, origin)
    check_parity(eng, ref, pos, lengths, origin, 'N=16 K=130')


def test_parity_n512(models, references):
    """N = 512: 2 pairs x 3 lengths (a pair that matches everywhere and a
    random one), and the pool of 4 pairs they come from, which meets the
    conditions of every pool."""
    K, origin, lengths, pos = rs.large_case()
    eng, wf, n, L = models(512)
    rs.assert_pool_conditions(pos, L, lengths, origin)
    ref = references(512, 'large', pos, lengths, origin)
    _, lr = check_parity(eng, ref, pos, lengths, origin, 'N=512, 4 pairs')
    two = rs.large_rows(pos)
    assert two.shape == (4, 512) and K == 3
    ref2 = tuple(a[[0, 1, 6, 7]] if a.shape[0] == 8 else a[[0, 3]]
                 for a in ref)
    _, lr2 = check_parity(eng, ref2, two, lengths, origin, 'N=512, 2 pairs')
    assert np.array_equal(lr2, lr[[0, 3]])


def test_n512_with_4096_lengths(models):
    """The largest LDS footprint (56 KB, beyond the default limit of a
    launch): the run of 2 pairs at N = 512 with 4096 lengths, whose last three
    are those of the parity case.  A length's result does not depend on the
    other lengths of the call, so those three columns carry the bits of the
    call with 3 lengths; the occupations are exact at every length."""
    K, origin, lengths, pos = rs.large_case()
    eng, _, n, L = models(512)
    two = rs.large_rows(pos)
    many = np.concatenate([L * (np.arange(4093) + 0.5) / 4094, lengths])
    assert len(many) == 4096
    assert len(rs.ambiguous(two, L, many, origin)) == 0
    n3, lr3 = eng.renyi_swap(two, lengths, origin)
    n_a, lr = eng.renyi_swap(two, many, origin)
    assert np.array_equal(n_a, rs.membership(two, L, many, origin)[1])
    ok = rs.matched(n_a)
    assert np.array_equal(np.isneginf(lr), ~ok)
    assert ok[0].sum() >= 8 and np.any(~ok[1])
    assert np.array_equal(n_a[:, -3:], n3)
    assert np.array_equal(lr[:, -3:], lr3)


def test_parity_without_lattice(models, references):
    """free16: interacting particles and no one-body factor."""
    eng, _, n, L = models('free16')
    K, origin, lengths, pos = rs.parity_cases(16)[3]
    rs.assert_pool_conditions(pos, L, lengths, origin)
    ref = references('free16', 'free', pos, lengths, origin)
    check_parity(eng, ref, pos, lengths, origin, 'free16')


# ---- 2. exact cases ---------------------------------------------------------------
@pytest.mark.parametrize('tag', ['ideal16', 'ideal_free16'])
def test_no_interaction_is_exactly_zero(models, tag):
    """g = 0, with a lattice and without: every matched entry is exactly 0.0
    and the swap sums are the match counts."""
    eng, _, n, L = models(tag)
    assert n == 16 and L == 16.0
    for K, origin, lengths, pos in rs.parity_cases(16):
        rs.assert_pool_conditions(pos, L, lengths, origin)
        _, n_ref = rs.membership(pos, L, lengths, origin)
        ok = rs.matched(n_ref)
        n_a, lr = eng.renyi_swap(pos, lengths, origin)
        assert np.array_equal(n_a, n_ref)
        assert np.array_equal(np.isneginf(lr), ~ok)
        assert np.all(lr[ok] == 0.0)
        dpos, dlen = _dev(eng, pos), _dev(eng, lengths)
        sums = reduce_dev(eng, dpos, len(pos), dlen, K, origin)
        count = ok.sum(axis=0).astype(np.float64)
        for col in range(3):
            assert np.array_equal(sums[:, col], count)
        dpos.close()
        dlen.close()


@pytest.mark.parametrize('n', [16, 64, 100])
def test_everything_inside_is_exactly_zero(models, n):
    """A length that puts every particle of both replicas in A: no pair
    crosses the cut."""
    eng, _, _, L = models(n)
    rng = np.random.RandomState(n)
    pos = 0.05 * L + 0.85 * L * rng.random_sample((6, n))
    pos[1] += 2 * L
    lengths = np.array([0.5 * L, 0.97 * L])
    assert len(rs.ambiguous(pos, L, lengths, 0.0)) == 0
    n_a, lr = eng.renyi_swap(pos, lengths, 0.0)
    assert np.all(n_a[:, 1] == n)
    assert np.all(lr[:, 1] == 0.0)
    # and every particle outside A
    n_a, lr = eng.renyi_swap(pos, [0.04 * L], 0.0)
    assert not n_a.any() and np.all(lr == 0.0)


# ---- 3. symmetries ----------------------------------------------------------------
@pytest.mark.parametrize('n', [16, 37, 128])
def test_symmetries(models, references, n):
    eng, wf, _, L = models(n)
    K, origin, lengths, pos = rs.parity_cases(n)[3]
    assert K == 5 and origin < 0
    n_ref, lr_ref, scale = references(n, (K, origin), pos, lengths, origin)
    fin = np.isfinite(lr_ref)
    bound = RTOL * np.maximum(1.0, scale)

    def same(lr):
        assert np.array_equal(np.isneginf(lr), ~fin)
        assert np.all(np.abs(lr[fin] - lr_ref[fin]) <= bound[fin])

    # the two rows of every pair exchanged
    flipped = pos.reshape(-1, 2, n)[:, ::-1].reshape(-1, n)
    n_a, lr = eng.renyi_swap(flipped, lengths, origin)
    assert np.array_equal(n_a.reshape(-1, 2, K)[:, ::-1].reshape(-1, K), n_ref)
    same(lr)
    # the complement of every segment
    for k in range(K):
        a0, ell = origin + lengths[k], L - lengths[k]
        assert len(rs.ambiguous(pos, L, [ell], a0)) == 0
        n_a, lr = eng.renyi_swap(pos, [ell], a0)
        assert np.array_equal(n_a[:, 0], n - n_ref[:, k])
        assert np.array_equal(np.isneginf(lr[:, 0]), ~fin[:, k])
        at = fin[:, k]
        assert np.all(np.abs(lr[at, 0] - lr_ref[at, k]) <= bound[at, k])
    # the particles of every row permuted
    rng = np.random.RandomState(n)
    perm = np.stack([row[rng.permutation(n)] for row in pos])
    n_a, lr = eng.renyi_swap(perm, lengths, origin)
    assert np.array_equal(n_a, n_ref)
    same(lr)
    # rows moved by whole periods
    moved = pos.copy()
    moved[0::3] += 2.0 * L
    moved[1::3] -= 5.0 * L
    assert len(rs.ambiguous(moved, L, lengths, origin)) == 0
    n_a, lr = eng.renyi_swap(moved, lengths, origin)
    assert np.array_equal(n_a, n_ref)
    same(lr)
    # R2 = R1: matched at every length, and the swap changes nothing
    twice = np.repeat(pos[0::2], 2, axis=0)
    n_a, lr = eng.renyi_swap(twice, lengths, origin)
    assert np.array_equal(n_a[0::2], n_a[1::2])
    z = rs.wrap(twice[0::2], L)
    own = 4.0 * np.abs([wf(row) for row in z])
    assert np.all(np.abs(lr) <= RTOL * np.maximum(1.0, own)[:, None])


# ---- 4. one path, many doors --------------------------------------------------------
@pytest.mark.parametrize('n,K', [(16, 5), (37, 1), (64, 5), (100, 5)])
def test_entry_points_agree(models, n, K):
    from phd_qmclib_amd.engine import DeviceBuffer
    eng, _, _, L = models(n)
    _, origin, lengths, pos = [c for c in rs.parity_cases(n) if c[0] == K][1]
    W, P = len(pos), len(pos) // 2
    n_a, lr = eng.renyi_swap(pos, lengths, origin)
    dpos, dlen = _dev(eng, pos), _dev(eng, lengths)
    # the device entry point: the same bits, and either output alone
    dna = DeviceBuffer(((W * K + 1) // 2,), eng.device)       # int32 pairs
    dlr = DeviceBuffer((P, K), eng.device)
    eng.renyi_swap_dev(W, dpos.ptr, K, dlen.ptr, origin, dna.ptr, dlr.ptr)
    eng.sync()
    got_n = dna.download().view(np.int32)[:W * K].reshape(W, K)
    assert np.array_equal(got_n, n_a)
    assert np.array_equal(dlr.download(), lr)
    dlr.upload(np.full((P, K), 7.0))
    eng.renyi_swap_dev(W, dpos.ptr, K, dlen.ptr, origin, None, dlr.ptr)
    eng.sync()
    assert np.array_equal(dlr.download(), lr)
    dna.upload(np.zeros(dna.shape))
    eng.renyi_swap_dev(W, dpos.ptr, K, dlen.ptr, origin, dna.ptr, None)
    eng.sync()
    assert np.array_equal(
        dna.download().view(np.int32)[:W * K].reshape(W, K), n_a)
    # the reduction: NumPy sums of the per-pair rows, the match column exact,
    # the same bits twice
    swap = swap_of(lr)
    sums = reduce_dev(eng, dpos, W, dlen, K, origin)
    assert sums.shape == (K, 3)
    assert close(sums[:, 0], swap.sum(axis=0))
    assert close(sums[:, 1], (swap ** 2).sum(axis=0))
    assert np.array_equal(sums[:, 2], np.isfinite(lr).sum(axis=0))
    assert np.array_equal(reduce_dev(eng, dpos, W, dlen, K, origin), sums)
    for b in (dpos, dlen, dna, dlr):
        b.close()


def test_reduce_spans_tiles(models):
    """K = 4096 lengths: the tile of the reduction is 2^24 // 8192 = 2048
    pairs and that of the host entry point 4096 configurations, so 2051 pairs
    span two of either."""
    n, K, P = 8, 4096, 2051
    eng, _, _, L = models(n)
    rng = np.random.RandomState(4096)
    made = L * rng.random_sample((P, n))
    pos = np.empty((2 * P, n))
    pos[0::2] = made
    pos[1::2] = made
    pos[1::2, 0] = L * rng.random_sample(P)       # one particle elsewhere
    lengths = L * (np.arange(K) + 0.5) / (K + 1)
    n_a, lr = eng.renyi_swap(pos, lengths, 0.25)
    assert np.array_equal(n_a, rs.membership(pos, L, lengths, 0.25)[1])
    ok = np.isfinite(lr)
    assert np.array_equal(ok, rs.matched(n_a)) and np.any(ok) and np.any(~ok)
    # the last pair, in the second tile, as a batch of its own
    n_last, lr_last = eng.renyi_swap(pos[-2:], lengths, 0.25)
    assert np.array_equal(n_last, n_a[-2:]) and np.array_equal(lr_last, lr[-1:])
    swap = swap_of(lr)
    dpos, dlen = _dev(eng, pos), _dev(eng, lengths)
    sums = reduce_dev(eng, dpos, 2 * P, dlen, K, 0.25)
    assert close(sums[:, 0], swap.sum(axis=0))
    assert close(sums[:, 1], (swap ** 2).sum(axis=0))
    assert np.array_equal(sums[:, 2], ok.sum(axis=0))
    assert np.array_equal(reduce_dev(eng, dpos, 2 * P, dlen, K, 0.25), sums)
    dpos.close()
    dlen.close()


def test_physical_funcs_broadcast(models, golden_params):
    from phd_qmclib_amd import mrbp_qmc
    n = 37
    eng, _, _, L = models(n)
    K, origin, lengths, pos = rs.parity_cases(n)[3]
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec_for(golden_params, n))
    _, lr = eng.renyi_swap(pos, lengths, origin)
    want = swap_of(lr)
    P = len(pos) // 2
    assert P == 12 and np.any(want == 0.0) and np.any(want > 0.0)
    confs = np.zeros((P, 2, 2, n))
    confs[:, :, 0, :] = pos.reshape(P, 2, n)
    out = pf.renyi_swap(lengths, confs, origin)
    assert out.shape == (P, K) and np.array_equal(out, want)
    out = pf.renyi_swap(lengths, confs.reshape(3, 4, 2, 2, n), origin=origin)
    assert np.array_equal(out, want.reshape(3, 4, K))
    one = pf.renyi_swap(lengths, confs[5], origin)
    assert one.shape == (K,) and np.array_equal(one, want[5])
    for bad in (confs[0, 0], confs[:, :1], np.zeros((P, 3, 2, n))):
        with pytest.raises(ValueError):
            pf.renyi_swap(lengths, bad, origin)


# ---- 5. the resident rows of a VMC ensemble ------------------------------------------
@pytest.mark.parametrize('move', ['all', 'particle'])
def test_vmc_resident_rows(golden_params, models, move):
    from phd_qmclib_amd import engine
    from phd_qmclib_amd.mrbp_qmc import vmc
    n, W = 16, 64
    spec = spec_for(golden_params, n)
    L = float(n)
    lengths, origin = rs.parity_lengths(n, 5), -0.5 * spec.barrier_width
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21,
                             move=move)
    s.init_random(seed=3)
    for _ in islice(s.blocks(4), 2):
        pass
    before = s.ensemble.get_state()
    ln, s2, s2_err, p_match = s.renyi_entropy(lengths, origin)
    parts = s.ensemble.renyi_parts(lengths, origin)
    after = s.ensemble.get_state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    confs = s.confs()
    s.close()
    assert len(rs.ambiguous(confs, L, lengths, origin)) == 0
    eng = models(n)[0]
    n_a, lr = eng.renyi_swap(confs, lengths, origin)
    assert np.array_equal(n_a, rs.membership(confs, L, lengths, origin)[1])
    swap = swap_of(lr)
    assert parts.shape == (5, 3)
    assert np.array_equal(parts[:, 2], np.isfinite(lr).sum(axis=0))
    assert parts[:, 2].sum() > 0
    assert close(parts[:, 0], swap.sum(axis=0))
    assert close(parts[:, 1], (swap ** 2).sum(axis=0))
    want = engine.renyi_entropy(parts, W // 2)
    assert np.array_equal(ln, lengths)
    for got, ref in zip((s2, s2_err, p_match), want):
        assert np.array_equal(got, ref, equal_nan=True)
    assert np.array_equal(p_match, parts[:, 2] / (W // 2))


def test_vmc_odd_number_of_chains(golden_params):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    from phd_qmclib_amd.mrbp_qmc import vmc
    spec = spec_for(golden_params, 16)
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, 63, rng_seed=2)
    s.init_random(seed=1)
    with pytest.raises(ValueError):
        s.renyi_entropy([4.0])
    with pytest.raises(ValueError):
        s.ensemble.renyi_parts([4.0])
    lib = _lib.load()
    ln, out = np.array([4.0]), np.zeros((1, 3))
    assert lib.qmc_vmc_renyi_swap(s.ensemble._h, 1, ptr(ln), 0.0,
                                  ptr(out)) != 0
    assert b'qmc_vmc_renyi_swap' in lib.qmc_last_error()
    assert not out.any()
    s.close()


# ---- 6. the known answer of free particles ---------------------------------------------
def test_known_answer():
    """N = L = 8 without interactions, 4096 pairs of uniform rows: mean(swap)
    is the probability that two binomial counts agree, within 4 binomial
    standard errors (the restatement alone: max |z| = 1.90)."""
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    k = rs.KNOWN
    args = rs.model_spec_args(k['n'])
    args['interaction_strength'] = 0
    eng = ModelEngine(Spec(**args).cfc_spec)
    pos = rs.known_answer_inputs()
    want, err = rs.known_answer_expected()
    P = k['nconf'] // 2
    for origin in k['origins']:
        assert len(rs.ambiguous(pos, k['sc_size'], k['lengths'], origin)) == 0
        n_a, lr = eng.renyi_swap(pos, k['lengths'], origin)
        assert np.array_equal(
            n_a, rs.membership(pos, k['sc_size'], k['lengths'], origin)[1])
        mean = swap_of(lr).mean(axis=0)
        z = (mean - want) / err
        print('known answer, origin %g: z = %s' % (origin, np.round(z, 2)))
        assert np.all(np.abs(z) <= 4.0)
        dpos, dlen = _dev(eng, pos), _dev(eng, np.array(k['lengths']))
        sums = reduce_dev(eng, dpos, len(pos), dlen, 4, origin)
        assert np.array_equal(sums[:, 0] / P, mean)
        dpos.close()
        dlen.close()
    eng.close()


# ---- 7. errors ----------------------------------------------------------------------------
def test_errors(models):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    n = 16
    eng, _, _, L = models(n)
    K, origin, lengths, pos = rs.parity_cases(n)[2]
    for bad in (pos[:5], pos[:1], pos[:0], pos[:, :15]):
        with pytest.raises(ValueError):
            eng.renyi_swap(bad, lengths, origin)
    for bad in ([0.0], [-1.0], [L], [1.0, L + 1.0], [float('nan')], []):
        with pytest.raises(ValueError):
            eng.renyi_swap(pos, bad, origin)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            eng.renyi_swap(pos, lengths, bad)
    lib = _lib.load()
    p = np.ascontiguousarray(pos)
    ln = np.ascontiguousarray(lengths)
    W = len(p)
    n_a = np.zeros((W, K), dtype=np.int32)
    lr = np.zeros((W // 2, K))
    np_, lp = ptr(n_a, _lib._i32p), ptr(lr)

    def call(nconf=W, pos_=ptr(p), nlen=K, len_=ptr(ln), a0=origin, na=np_,
             out=lp):
        return lib.qmc_renyi_swap(eng._h, nconf, pos_, nlen, len_, a0, na,
                                  out)
    bad_len = [np.array(v + [1.0] * (K - len(v))) for v in
               ([0.0], [-2.0], [L], [1.0, 2.0 * L], [float('nan')],
                [float('inf')])]
    for kwargs in ([dict(nconf=W - 1), dict(nconf=1), dict(nconf=0),
                    dict(nconf=-2), dict(nlen=0), dict(nlen=4097),
                    dict(a0=float('nan')), dict(a0=float('inf')),
                    dict(pos_=None), dict(len_=None), dict(na=None, out=None)]
                   + [dict(len_=ptr(b)) for b in bad_len]):
        assert call(**kwargs) != 0, kwargs
        assert b'qmc_renyi_swap' in lib.qmc_last_error()
    assert not n_a.any() and not lr.any()
    assert lib.qmc_renyi_swap_dev(eng._h, W - 1, None, K, None, origin, None,
                                  None) != 0
    assert lib.qmc_renyi_swap_reduce_dev(eng._h, W, None, K, None, origin,
                                         None) != 0
    assert lib.qmc_vmc_renyi_swap(None, K, ptr(ln), origin, None) != 0
    # either output alone is legal, and the engine still works afterwards
    assert call(na=None) == 0 and call(out=None) == 0
    want_n, want_lr = eng.renyi_swap(pos, lengths, origin)
    assert np.array_equal(n_a, want_n) and np.array_equal(lr, want_lr)
