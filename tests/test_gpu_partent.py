"""One-particle replica swap on the GPU (csrc/qmc_partent.h) against the NumPy
restatement of its definition (tests/_partent_restatement.py) with the C
oracle's wf_abs_log on explicitly swapped configurations.  All tests need a
GPU.

log_ratio is compared element by element with

    |dev - ref| <= 2e-11 max(1, sum of the |four ln psi terms|),

the 2e-11 being the RTOL of the suite and the scale what the explicit route
cancels against; the per-pair mean with 2e-11 max(1, largest scale of the
pair) mean_ref.  Where the reference is the factorised restatement (N = 512),
the scale is the sum of the magnitudes of the terms of that form, which is the
smaller of the two.  Sums in floating point use |delta| <= 2e-11 max(1, |x|).
"""
from itertools import islice

import numpy as np
import pytest

from . import _partent_restatement as pe
from ._models import _dev

pytestmark = pytest.mark.gpu

RTOL = pe.RTOL


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
    if key in pe.GOLDEN_SIZES:
        return Spec(**golden_params[pe.GOLDEN_SIZES[key]]['spec'])
    return Spec(**pe.model_spec_args(key))


@pytest.fixture(scope='module')
def models(golden_params, oracle):
    """key -> (engine, wf_abs_log of the oracle, N, L, spec), built once."""
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(key):
        if key not in cache:
            spec = spec_for(golden_params, key)
            eng = ModelEngine(spec.cfc_spec)
            om = oracle.model_from_cfc(spec.cfc_spec)
            cache[key] = (eng, lambda z: oracle.wf_abs_log(om, z),
                          spec.boson_number, float(spec.supercell_size), spec)
        return cache[key]
    yield get
    for rec in cache.values():
        rec[0].close()


@pytest.fixture(scope='module')
def references(models):
    """n -> (pos, log_ratio, scale, mean) of the explicit route on the pool of
    that size, computed once and shared; nobody writes into them."""
    cache = {}

    def get(n):
        if n not in cache:
            _, wf, _, L, _ = models(n)
            pos = pe.pool(n)
            out = (pos,) + pe.reference(wf, pos, L)
            for a in out:
                a.setflags(write=False)
            cache[n] = out
        return cache[n]
    return get


def reduce_dev(eng, dpos, W):
    from phd_qmclib_amd.engine import DeviceBuffer
    dsums = DeviceBuffer((3,), eng.device)
    eng.particle_swap_reduce_dev(W, dpos.ptr, dsums.ptr)
    eng.sync()
    out = dsums.download()
    dsums.close()
    return out


def check(mean, lr, lr_ref, scale, mean_ref, label):
    assert lr.dtype == np.float64 and lr.shape == lr_ref.shape
    assert mean.dtype == np.float64 and mean.shape == mean_ref.shape
    ok, worst = pe.within_tolerance(lr, lr_ref, scale)
    okm, worstm = pe.mean_within_tolerance(mean, mean_ref, scale)
    print('%s: worst error / bound = %.3g (log_ratio), %.3g (mean)'
          % (label, worst, worstm))
    assert ok and okm


# ---- 1. parity with the definition ----------------------------------------------
@pytest.mark.parametrize('n', pe.PARITY_SIZES)
def test_parity(models, references, n):
    eng, _, nn, L, _ = models(n)
    assert nn == n and L == float(n)
    pos, lr_ref, scale, mean_ref = references(n)
    assert pos.shape == (2 * pe.PARITY_PAIRS, n)
    assert np.any(pos < 0) and np.any(pos >= L)
    mean, lr = eng.particle_swap(pos, matrix=True)
    check(mean, lr, lr_ref, scale, mean_ref, 'N=%d' % n)
    assert np.array_equal(eng.particle_swap(pos), mean)


def test_parity_n512(models, golden_params):
    """N = 512, 2 pairs: the whole matrix against the factorised restatement,
    64 drawn elements against the definition through the oracle."""
    eng, wf, n, L, _ = models(512)
    pos, drawn = pe.large_case()
    assert pos.shape == (4, 512) and drawn.shape == (64, 3)
    tbf = golden_params['box512']['tbf_params']
    lr_ref, scale = pe.factorised(tbf, L, pos, with_scale=True)
    mean, lr = eng.particle_swap(pos, matrix=True)
    check(mean, lr, lr_ref, scale, pe.mean_of(lr_ref), 'N=512 factorised')
    z = pe.wrap(pos, L)
    worst = 0.0
    for p in (0, 1):
        el = [(i, j) for q, i, j in drawn if q == p]
        assert el
        ref, sc = pe.explicit(wf, z[2 * p], z[2 * p + 1], elements=el)
        got = np.array([lr[p, i, j] for i, j in el])
        ok, w = pe.within_tolerance(got, ref, sc)
        worst = max(worst, w)
        assert ok
    print('N=512, 64 elements through the oracle: worst error / bound = %.3g'
          % worst)


def test_parity_without_lattice(models, oracle):
    """free16: interacting particles and no one-body factor."""
    eng, wf, n, L, _ = models('free16')
    pos = pe.pool(16, seed=77)
    lr_ref, scale, mean_ref = pe.reference(wf, pos, L)
    mean, lr = eng.particle_swap(pos, matrix=True)
    check(mean, lr, lr_ref, scale, mean_ref, 'free16')


# ---- 2. the order of a row does not matter ----------------------------------------
@pytest.mark.parametrize('n', pe.ORDER_SIZES)
def test_order_independence(models, references, n):
    """Rows sorted ascending, rows shuffled one by one and rows as drawn: the
    same mean, and log_ratio permuted with the rows."""
    eng, _, _, L, _ = models(n)
    pos, lr_ref, scale, mean_ref = references(n)
    srt, ps, shf, pr = pe.reorderings(pos, n)
    assert np.all(np.diff(pe.wrap(srt, L), axis=1) >= 0)
    for rows, perm, name in ((srt, ps, 'sorted'), (shf, pr, 'shuffled')):
        mean, lr = eng.particle_swap(rows, matrix=True)
        check(mean, lr, pe.permuted(lr_ref, perm), pe.permuted(scale, perm),
              mean_ref, 'N=%d %s' % (n, name))


# ---- 3. symmetries and exact cases ------------------------------------------------
@pytest.mark.parametrize('n', [16, 37, 128])
def test_symmetries(models, references, n):
    eng, wf, _, L, _ = models(n)
    pos, lr_ref, scale, mean_ref = references(n)
    # the two rows of every pair exchanged: the transpose, the same mean
    flipped = pos.reshape(-1, 2, n)[:, ::-1].reshape(-1, n)
    mean, lr = eng.particle_swap(flipped, matrix=True)
    check(mean, lr, lr_ref.transpose(0, 2, 1), scale.transpose(0, 2, 1),
          mean_ref, 'N=%d flipped' % n)
    # rows moved by whole periods
    moved = pos.copy()
    moved[0::3] += 2.0 * L
    moved[1::3] -= 5.0 * L
    mean, lr = eng.particle_swap(moved, matrix=True)
    check(mean, lr, lr_ref, scale, mean_ref, 'N=%d moved' % n)
    # R2 = R1: exchanging particle i with its copy changes nothing
    twice = np.repeat(pos[0::2], 2, axis=0)
    _, lr = eng.particle_swap(twice, matrix=True)
    own = 4.0 * np.abs([wf(row) for row in pe.wrap(twice[0::2], L)])
    diag = np.diagonal(lr, axis1=1, axis2=2)
    assert np.all(np.abs(diag) <= RTOL * np.maximum(1.0, own)[:, None])


@pytest.mark.parametrize('tag', ['ideal16', 'ideal_free16'])
def test_no_interaction_is_exactly_zero_and_one(models, tag):
    eng, _, n, L, _ = models(tag)
    assert n == 16 and L == 16.0
    pos = pe.pool(16)
    mean, lr = eng.particle_swap(pos, matrix=True)
    assert np.all(lr == 0.0) and np.all(mean == 1.0)
    dpos = _dev(eng, pos)
    assert reduce_dev(eng, dpos, len(pos)).tolist() == [6.0, 6.0, 6.0]
    dpos.close()


# ---- 4. one path, many doors ------------------------------------------------------
@pytest.mark.parametrize('n', [3, 16, 37, 100])
def test_entry_points_agree(models, n):
    from phd_qmclib_amd.engine import DeviceBuffer
    eng, _, _, L, _ = models(n)
    pos = pe.pool(n)
    W, P = len(pos), len(pos) // 2
    mean, lr = eng.particle_swap(pos, matrix=True)
    dpos = _dev(eng, pos)
    # the device entry point: the same bits, and either output alone
    dm, dlr = DeviceBuffer((P,), eng.device), DeviceBuffer((P, n, n),
                                                           eng.device)
    eng.particle_swap_dev(W, dpos.ptr, dm.ptr, dlr.ptr)
    eng.sync()
    assert np.array_equal(dm.download(), mean)
    assert np.array_equal(dlr.download(), lr)
    dlr.upload(np.full((P, n, n), 7.0))
    eng.particle_swap_dev(W, dpos.ptr, None, dlr.ptr)
    eng.sync()
    assert np.array_equal(dlr.download(), lr)
    dm.upload(np.full(P, 7.0))
    eng.particle_swap_dev(W, dpos.ptr, dm.ptr, None)
    eng.sync()
    assert np.array_equal(dm.download(), mean)
    # the reduction: NumPy sums of the per-pair means, the count exact, the
    # same bits twice
    sums = reduce_dev(eng, dpos, W)
    assert sums.shape == (3,)
    assert close(sums[0], mean.sum()) and close(sums[1], (mean ** 2).sum())
    assert sums[2] == P
    assert np.array_equal(reduce_dev(eng, dpos, W), sums)
    for b in (dpos, dm, dlr):
        b.close()


def test_reduce_spans_tiles(models):
    """N = 2: 2^16 + 3 pairs span two scratch tiles of 2^16 pairs."""
    n, P = 2, (1 << 16) + 3
    eng, _, _, L, _ = models(n)
    pos = L * np.random.RandomState(65536).random_sample((2 * P, n))
    mean = eng.particle_swap(pos)
    # the last pair, in the second tile, as a batch of its own
    assert np.array_equal(eng.particle_swap(pos[-2:]), mean[-1:])
    dpos = _dev(eng, pos)
    sums = reduce_dev(eng, dpos, 2 * P)
    assert close(sums[0], mean.sum()) and close(sums[1], (mean ** 2).sum())
    assert sums[2] == P
    assert np.array_equal(reduce_dev(eng, dpos, 2 * P), sums)
    dpos.close()


def test_physical_funcs_broadcast(models, golden_params):
    from phd_qmclib_amd import mrbp_qmc
    n = 37
    eng, _, _, L, _ = models(n)
    pos = pe.pool(n)
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec_for(golden_params, n))
    want = eng.particle_swap(pos)
    P = len(pos) // 2
    confs = np.zeros((P, 2, 2, n))
    confs[:, :, 0, :] = pos.reshape(P, 2, n)
    out = pf.particle_swap(confs)
    assert out.shape == (P,) and np.array_equal(out, want)
    out = pf.particle_swap(confs.reshape(2, 3, 2, 2, n))
    assert np.array_equal(out, want.reshape(2, 3))
    one = pf.particle_swap(confs[5])
    assert np.shape(one) == () and one == want[5]
    for bad in (confs[0, 0], confs[:, :1], np.zeros((P, 3, 2, n))):
        with pytest.raises(ValueError):
            pf.particle_swap(bad)


# ---- 5. the resident rows of a VMC ensemble ----------------------------------------
@pytest.mark.parametrize('move', ['all', 'particle'])
def test_vmc_resident_rows(golden_params, models, move):
    from phd_qmclib_amd import engine
    from phd_qmclib_amd.mrbp_qmc import vmc
    n, W = 16, 64
    spec = spec_for(golden_params, n)
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=21,
                             move=move)
    s.init_random(seed=3)
    for _ in islice(s.blocks(4), 2):
        pass
    before = s.ensemble.get_state()
    got = s.particle_entropy()
    parts = s.ensemble.particle_swap_parts()
    after = s.ensemble.get_state()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    confs = s.confs()
    s.close()
    mean = models(n)[0].particle_swap(confs)
    assert parts.shape == (3,) and parts[2] == W // 2
    assert close(parts[0], mean.sum()) and close(parts[1], (mean ** 2).sum())
    assert got == engine.particle_entropy(parts, W // 2)
    s2, s2_err, purity, purity_err = got
    # (a few yields from a random start: the 32 pairs are not a sample of
    # |psi|^2, so their mean need not stay below 1)
    assert purity == parts[0] / (W // 2) > 0.0 and s2 == -np.log(purity)
    assert purity_err > 0.0 and s2_err == purity_err / purity


def test_vmc_odd_number_of_chains(golden_params):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    from phd_qmclib_amd.mrbp_qmc import vmc
    spec = spec_for(golden_params, 16)
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, 63, rng_seed=2)
    s.init_random(seed=1)
    with pytest.raises(ValueError):
        s.particle_entropy()
    with pytest.raises(ValueError):
        s.ensemble.particle_swap_parts()
    lib = _lib.load()
    out = np.zeros(3)
    assert lib.qmc_vmc_particle_swap(s.ensemble._h, ptr(out)) != 0
    assert b'qmc_vmc_particle_swap' in lib.qmc_last_error()
    assert not out.any()
    s.close()


# ---- 6. the known answer: N = 2 without a lattice -----------------------------------
def test_known_answer(golden_params):
    """Two interacting particles on a ring, 8192 pairs of grid configurations
    drawn from psi^2 on a 24 x 24 grid: the device mean of m lies within
    4.5 sigma of the exact grid sum E m, sigma from the exact E m^2
    (the restatement alone: tests/test_partent_host.py)."""
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    args = dict(golden_params['free16']['spec'])
    args['boson_number'] = 2
    spec = Spec(**args)
    L = float(spec.supercell_size)
    em, em2, pos = pe.known_answer(spec.tbf_params, L)
    eng = ModelEngine(spec.cfc_spec)
    mean = eng.particle_swap(pos)
    dpos = _dev(eng, pos)
    sums = reduce_dev(eng, dpos, len(pos))
    dpos.close()
    eng.close()
    assert mean.shape == (pe.KNOWN['npair'],)
    z = pe.known_answer_z(mean, em, em2)
    print('known answer: E m = %.6f, device mean = %.6f, z = %.2f'
          % (em, mean.mean(), z))
    assert abs(z) <= pe.KNOWN['sigmas'] == 4.5
    assert sums[2] == pe.KNOWN['npair'] and close(sums[0], mean.sum())


# ---- 7. errors -------------------------------------------------------------------------
def test_errors(models):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import QmcError, ptr
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    n = 16
    eng, _, _, L, _ = models(n)
    pos = np.ascontiguousarray(pe.pool(n))
    for bad in (pos[:5], pos[:1], pos[:0], pos[:, :15]):
        with pytest.raises(ValueError):
            eng.particle_swap(bad)
    lib = _lib.load()
    W = len(pos)
    mean, lr = np.zeros(W // 2), np.zeros((W // 2, n, n))

    def call(nconf=W, pos_=ptr(pos), m=ptr(mean), out=ptr(lr)):
        return lib.qmc_particle_swap(eng._h, nconf, pos_, m, out)
    for kwargs in (dict(nconf=W - 1), dict(nconf=1), dict(nconf=0),
                   dict(nconf=-2), dict(pos_=None), dict(m=None, out=None)):
        assert call(**kwargs) != 0, kwargs
        assert b'qmc_particle_swap' in lib.qmc_last_error()
    assert not mean.any() and not lr.any()
    assert lib.qmc_particle_swap_dev(eng._h, W - 1, None, None, None) != 0
    assert lib.qmc_particle_swap_reduce_dev(eng._h, W, None, None) != 0
    assert lib.qmc_particle_swap_reduce_dev(eng._h, 0, None, None) != 0
    assert lib.qmc_vmc_particle_swap(None, None) != 0
    # either output alone is legal, and the engine still works afterwards
    assert call(m=None) == 0 and call(out=None) == 0
    want_m, want_lr = eng.particle_swap(pos, matrix=True)
    assert np.array_equal(mean, want_m) and np.array_equal(lr, want_lr)
    # N above 512: no engine holds such a model, and a row of another
    # length is refused
    with pytest.raises(QmcError, match='512'):
        ModelEngine(Spec(**pe.model_spec_args(513)).cfc_spec)
    with pytest.raises(ValueError):
        models(512)[0].particle_swap(np.zeros((2, 513)))
