"""One-body density matrix g1(s) on the GPU (csrc/qmc_obdm.h) against the
reference's golden values (tests/golden/obdm.npz), exact identities, every
entry point against the others, batch shapes against the NumPy restatement of
the definition (tests/_obdm_restatement.py, itself anchored on the golden
values by tests/test_obdm_host.py), the Python surface and the statistics of
an equilibrated ensemble.  All tests need a GPU.

Tolerance: the suite's own, |delta| <= 2e-11 max(1, |x|)
(tests/test_gpu_parity.py).

Two statements of the specification are narrowed here, with the reason:

* g1(L) = 1 and g1(s + L) = g1(s) hold where the one-body factor (period 1,
  the lattice) has the period L of the supercell too, i.e. for an integer L
  or a free model.  `odd24` has L = 17.5 and a lattice: the reference's own
  golden value there is g1(L) = 0.46 .. 1.54.  The identities are asserted
  for the fourteen other specs; for odd24 the golden parity covers g1(L).
* batch shapes: every batch size (1, 63, 64, 65, 4097), every nshift
  (1, 2, 65) and every N (8, 37, 64, 100, 128, 512) run in every combination
  on the device, and every value is compared.  The NumPy yardstick costs
  O(N^2) per value, so the rows of a batch are drawn (with repetition, in
  random order) from a pool of distinct random configurations per N (24; 8
  at N = 512) whose g1 the restatement computes once for the 65 shifts.
"""
import ctypes as C
import os
import sys
from math import pi

import numpy as np
import pytest

from ._obdm_restatement import ith_one_body_density
from .conftest import GOLDEN, ROOT
from ._models import _dev, spec_from_golden

pytestmark = pytest.mark.gpu

RTOL = 2e-11
ALL_TAGS = ['box8', 'box16', 'box64', 'box128', 'box512', 'free16', 'deep100',
            'deep16', 'ideal16', 'defect24', 'odd24', 'box37', 'box48',
            'box100', 'box126']


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


def worst(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope='module')
def golden_obdm():
    return np.load(os.path.join(GOLDEN, 'obdm.npz'), allow_pickle=False)


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


def golden_case(golden_kernels, golden_obdm, tag):
    g1 = golden_obdm[tag + '/g1']
    pos = golden_kernels[tag + '/pos'][:len(g1)]
    return pos, golden_obdm[tag + '/shifts'], g1


# ---- 1. parity with the reference ---------------------------------------
@pytest.mark.parametrize('tag', ALL_TAGS)
def test_obdm_vs_reference_golden(engines, golden_kernels, golden_obdm, tag):
    pos, shifts, ref = golden_case(golden_kernels, golden_obdm, tag)
    assert np.all(np.isfinite(ref))
    has_ith = tag + '/ith' in golden_obdm.files
    out = engines(tag).one_body_density(pos, shifts, ith=has_ith)
    g1 = out[0] if has_ith else out
    print(tag, 'g1 worst', worst(g1, ref))
    assert g1.shape == ref.shape
    assert close(g1, ref)
    if has_ith:
        ref_ith = golden_obdm[tag + '/ith']
        assert np.all(np.isfinite(ref_ith))
        print(tag, 'ith worst', worst(out[1], ref_ith))
        assert out[1].shape == ref_ith.shape
        assert close(out[1], ref_ith)


# ---- 2. exact identities -------------------------------------------------
@pytest.mark.parametrize('tag', ALL_TAGS)
def test_obdm_identities(engines, golden_params, golden_kernels, tag):
    eng = engines(tag)
    pos = golden_kernels[tag + '/pos']
    L = float(golden_params[tag]['params']['supercell_size'])
    base = np.array([0.0, 0.37, -1.21, 0.25 * L, -0.431 * L])
    g = eng.one_body_density(pos, base)
    print(tag, 'max |g1(0) - 1|', np.max(np.abs(g[:, 0] - 1.0)))
    assert np.all(np.abs(g[:, 0] - 1.0) <= 1e-14)
    periodic = L == int(L) or golden_params[tag]['params']['is_free']
    if periodic:
        gl = eng.one_body_density(pos, base + L)
        print(tag, 'g1(s + L) worst', worst(gl, g))
        assert close(gl[:, 0], np.ones(len(pos)))
        assert close(gl, g)
    else:
        assert tag == 'odd24'


def test_obdm_free_ideal_is_one(golden_params):
    from phd_qmclib_amd.engine import ModelEngine
    from phd_qmclib_amd.mrbp_qmc import Spec
    spec = Spec(**dict(golden_params['box16']['spec'], lattice_depth=0.0,
                       interaction_strength=0.0))
    assert spec.is_free and spec.is_ideal
    eng = ModelEngine(spec.cfc_spec)
    rng = np.random.RandomState(5)
    pos = 16.0 * rng.random_sample((9, 16))
    shifts = np.array([0.0, 0.3, -7.7, 16.0, 40.1])
    g1, ith = eng.one_body_density(pos, shifts, ith=True)
    eng.close()
    assert np.array_equal(g1, np.ones((9, 5)))
    assert np.array_equal(ith, np.ones((9, 5, 16)))


# ---- 3. order independence -----------------------------------------------
@pytest.mark.parametrize('tag', ['box16', 'box37', 'box64', 'defect24',
                                 'box100', 'box128'])
def test_obdm_order_independent(engines, golden_kernels, golden_obdm, tag):
    pos, shifts, _ = golden_case(golden_kernels, golden_obdm, tag)
    rng = np.random.RandomState(11)
    perm = rng.permutation(pos.shape[1])
    eng = engines(tag)
    g1, ith = eng.one_body_density(pos, shifts, ith=True)
    g1p, ithp = eng.one_body_density(pos[:, perm], shifts, ith=True)
    assert close(g1p, g1)
    assert close(ithp, ith[:, :, perm])


# ---- 4. one path, many doors ---------------------------------------------
@pytest.mark.parametrize('tag', ['box16', 'box37', 'box64', 'box100',
                                 'box128'])
def test_obdm_entry_points_agree(engines, golden_params, golden_kernels,
                                 golden_obdm, tag):
    from phd_qmclib_amd.engine import DeviceBuffer, VmcEnsemble
    eng = engines(tag)
    pos, shifts, _ = golden_case(golden_kernels, golden_obdm, tag)
    rng = np.random.RandomState(3)
    L = float(golden_params[tag]['params']['supercell_size'])
    pos = np.concatenate([pos, L * rng.random_sample((70 - len(pos),
                                                      pos.shape[1]))])
    W, n = pos.shape
    M = len(shifts)
    g1, ith = eng.one_body_density(pos, shifts, ith=True)
    # device buffers: bit for bit
    dpos, dsh = _dev(eng, pos), _dev(eng, shifts)
    dg1, dith = DeviceBuffer((W, M), eng.device), \
        DeviceBuffer((W, M, n), eng.device)
    eng.one_body_density_dev(W, dpos.ptr, M, dsh.ptr, dg1.ptr, dith.ptr)
    eng.sync()
    assert np.array_equal(dg1.download(), g1)
    assert np.array_equal(dith.download(), ith)
    # the reduction, unit weights: the NumPy sums, and the same bits twice
    dsums, dws = DeviceBuffer((M, 2), eng.device), DeviceBuffer((1,),
                                                                eng.device)
    eng.one_body_density_reduce_dev(W, dpos.ptr, None, M, dsh.ptr, dsums.ptr,
                                    dws.ptr)
    eng.sync()
    s1, w1 = dsums.download(), dws.download()
    eng.one_body_density_reduce_dev(W, dpos.ptr, None, M, dsh.ptr, dsums.ptr,
                                    dws.ptr)
    eng.sync()
    assert np.array_equal(dsums.download(), s1)
    assert w1[0] == W
    assert np.allclose(s1[:, 0], g1.sum(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(s1[:, 1], (g1 ** 2).sum(axis=0), rtol=1e-12, atol=0)
    # random positive weights
    w = 0.25 + rng.random_sample(W)
    dw = _dev(eng, w)
    eng.one_body_density_reduce_dev(W, dpos.ptr, dw.ptr, M, dsh.ptr,
                                    dsums.ptr, dws.ptr)
    eng.sync()
    sw, ww = dsums.download(), dws.download()
    assert np.allclose(ww[0], w.sum(), rtol=1e-12, atol=0)
    assert np.allclose(sw[:, 0], (w[:, None] * g1).sum(axis=0), rtol=1e-12,
                       atol=0)
    assert np.allclose(sw[:, 1], (w[:, None] * g1 ** 2).sum(axis=0),
                       rtol=1e-12, atol=0)
    # the VMC ensemble's resident, position-sorted rows
    v = VmcEnsemble(eng, W, 0.125, rng_seed=1)
    v.set_state(pos)
    parts = v.obdm_parts(shifts)
    v.close()
    assert np.allclose(parts[:, 0], g1.sum(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(parts[:, 1], (g1 ** 2).sum(axis=0), rtol=1e-12, atol=0)
    for b in (dpos, dsh, dg1, dith, dsums, dws, dw):
        b.close()


# ---- 5. every shape --------------------------------------------------------
SHAPE_TAGS = {8: 'box8', 37: 'box37', 64: 'box64', 100: 'box100',
              128: 'box128', 512: 'box512'}


@pytest.mark.parametrize('n', sorted(SHAPE_TAGS))
def test_obdm_batch_shapes(engines, golden_params, n):
    tag = SHAPE_TAGS[n]
    p = golden_params[tag]
    L = float(p['params']['supercell_size'])
    rng = np.random.RandomState(100 + n)
    pool = L * rng.random_sample((24 if n <= 128 else 8, n))
    pool[1] -= 0.75 * L            # positions outside [0, L) are legal
    pool[2] += 1.5 * L
    shifts = np.concatenate([[0.4321, -0.37 * L],
                             L * (3.0 * rng.random_sample(63) - 1.5)])
    ref = ith_one_body_density(pool, shifts, p)        # [pool, 65, n]
    ref_g1 = ref.mean(axis=2)
    eng = engines(tag)
    for nconf in (1, 63, 64, 65, 4097):
        idx = rng.randint(0, len(pool), size=nconf)
        pos = pool[idx]
        for nshift in (1, 2, 65):
            want_ith = nconf <= 65 and n <= 128
            out = eng.one_body_density(pos, shifts[:nshift], ith=want_ith)
            g1 = out[0] if want_ith else out
            assert g1.shape == (nconf, nshift)
            w = worst(g1, ref_g1[idx, :nshift])
            assert w <= RTOL, (n, nconf, nshift, w)
            if want_ith:
                assert close(out[1], ref[idx, :nshift]), (n, nconf, nshift)


# ---- 6. Python surface ---------------------------------------------------
def test_core_funcs_scalars(golden_params, golden_kernels, golden_obdm):
    from phd_qmclib_amd import mrbp_qmc
    for tag in ('box16', 'free16', 'defect24'):
        cfc = spec_from_golden(golden_params, tag).cfc_spec
        pos, shifts, g1 = golden_case(golden_kernels, golden_obdm, tag)
        ith = golden_obdm[tag + '/ith']
        conf = np.zeros((2, pos.shape[1]))
        conf[0] = pos[3]
        for k in (1, 5, 14):
            v = mrbp_qmc.core_funcs.one_body_density(shifts[k], conf, *cfc)
            assert type(v) is float and close(v, g1[3, k])
            for i in (0, pos.shape[1] - 1):
                u = mrbp_qmc.core_funcs.ith_one_body_density(
                    i, shifts[k], conf, *cfc)
                assert type(u) is float and close(u, ith[3, k, i])


def test_physical_funcs(golden_params, golden_kernels, golden_obdm):
    from phd_qmclib_amd import mrbp_qmc
    tag = 'box37'
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(
        spec_from_golden(golden_params, tag))
    pos, shifts, g1 = golden_case(golden_kernels, golden_obdm, tag)
    confs = np.zeros((len(pos), 2, pos.shape[1]))
    confs[:, 0, :] = pos
    out = pf.one_body_density(shifts[:, None], confs[None])
    assert out.shape == (len(shifts), len(pos))
    assert close(out, g1.T)
    one = pf.one_body_density(shifts[2], confs[1])
    assert np.ndim(one) == 0 and close(one, g1[1, 2])
    assert close(pf.one_body_density(shifts[4], confs), g1[:, 4])
    assert close(pf.wf_abs_log(confs), golden_kernels[tag + '/wf_abs_log'])
    assert close(pf.energy(confs), golden_kernels[tag + '/energy'])
    assert close(pf.energy(confs.reshape(2, 4, 2, -1)),
                 golden_kernels[tag + '/energy'].reshape(2, 4))
    kz = 2 * pi / 37.0 * np.arange(5)
    fd = pf.fourier_density(kz, confs)
    assert fd.shape == (len(pos), 5) and np.iscomplexobj(fd)
    want = np.exp(1j * kz[None, :, None] * pos[:, None, :]).sum(axis=2)
    assert np.allclose(fd, want, rtol=0, atol=1e-11)


# ---- 7. statistics on an equilibrated ensemble ----------------------------
def test_ensemble_statistics():
    """5 sigma and the other bounds were fixed before the first run; seeds as
    written."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from _stationary import seed_configurations
    from phd_qmclib_amd.mrbp_qmc import Spec, vmc
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=64, supercell_size=64,
                tbf_contact_cutoff=16)
    W = 1 << 14
    s = vmc.EnsembleSampling(spec, 0.25 * spec.well_width, W, rng_seed=17)
    s.set_confs(seed_configurations(s.engine, spec, 64, seeds=W, steps=30000))
    L = 64.0
    pos_shifts = L / 2 * np.arange(1, 9) / 8.0          # eight in (0, L/2]
    shifts = np.concatenate([[0.0], pos_shifts, -pos_shifts])
    sh, mean, err = s.one_body_density(shifts)
    s.close()
    for row in zip(sh, mean, err):
        print('g1(%8.3f) = %.6e +- %.3e' % row)
    assert np.array_equal(sh, shifts)
    assert abs(mean[0] - 1.0) <= 1e-14 and err[0] < 1e-14
    assert np.all(np.isfinite(mean)) and np.all(mean[1:] > 0.0)
    gp, gm = mean[1:9], mean[9:]
    comb = np.sqrt(err[1:9] ** 2 + err[9:] ** 2)
    print('|g1(s) - g1(-s)| / combined stderr:', np.abs(gp - gm) / comb)
    assert np.all(np.abs(gp - gm) <= 5.0 * comb)


# ---- 8. bad arguments ------------------------------------------------------
def test_bad_arguments(engines, golden_kernels):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd._lib import ptr
    lib = _lib.load()
    eng = engines('box16')
    pos = np.ascontiguousarray(golden_kernels['box16/pos'])
    sh = np.array([0.5, 1.0])
    g1 = np.zeros((len(pos), 2))
    for args in ((0, ptr(sh), ptr(g1)),
                 (2, ptr(np.array([0.5, np.nan])), ptr(g1)),
                 (2, ptr(np.array([np.inf, 0.5])), ptr(g1)),
                 (2, None, ptr(g1)),
                 (2, ptr(sh), None)):
        rc = lib.qmc_obdm(eng._h, len(pos), ptr(pos), args[0], args[1],
                          args[2], None)
        assert rc != 0
        assert b'qmc_obdm' in lib.qmc_last_error()
    assert lib.qmc_obdm_dev(eng._h, 1, None, 1, None, None, None) != 0
    assert lib.qmc_obdm_reduce_dev(eng._h, 1, None, None, 0, None, None,
                                   None) != 0
    with pytest.raises(_lib.QmcError):
        eng.one_body_density(pos, [0.1, float('nan')])
    # the engine still evaluates afterwards
    assert np.all(np.abs(eng.one_body_density(pos, [0.0]) - 1.0) <= 1e-14)
    assert close(eng.evaluate(pos).energy, golden_kernels['box16/energy'])


# ---- 9. DMC mixed estimate -------------------------------------------------
def test_dmc_mixed_estimate(golden_params, golden_kernels, golden_obdm):
    from phd_qmclib_amd.mrbp_qmc import dmc
    tag = 'box16'
    pos, shifts, g1 = golden_case(golden_kernels, golden_obdm, tag)
    nw, n = pos.shape
    s = dmc.Sampling(spec_from_golden(golden_params, tag), 1e-3, 32, nw,
                     rng_seed=1)
    confs = np.zeros((nw, 2, n))
    confs[:, 0, :] = pos
    state = s.build_state(confs)
    weight = state.props.weight.copy()
    weight[:nw] = 0.5 + np.arange(nw) / 3.0
    weight[nw:] = 1e9               # dead slots must not count
    state = state._replace(props=state.props._replace(weight=weight))
    est = s.one_body_density(state, shifts)
    want = (weight[:nw, None] * g1).sum(axis=0) / weight[:nw].sum()
    assert est.shape == (len(shifts),)
    assert close(est, want)
