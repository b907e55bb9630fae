"""Energy components and Tan's contact on the GPU (csrc/qmc_energy_parts.h)
against the NumPy restatement of the row (tests/_energy_parts_restatement.py,
anchored on the reference's golden values by tests/test_energy_parts_host.py).
All tests need a GPU.

Tolerance: |delta| <= 2e-11 max(1, |x|) on every column, the RTOL of
tests/test_gpu_parity.py.  It is enough for the window sums because every
input is edge free (no pair distance within 1e-9 of a window: the only pairs
rounding can move), which tests/test_energy_parts_host.py asserts without a GPU
and the tests here assert again.

The two statistical tests hold a mean to +-4.5 standard errors (a condition,
not a tuned number: 7e-6 of a normal law lies outside).  For the model with
interactions the bias of the window r_c = 0.05 against 0.02 was -0.19 +- 0.2 on
the CPU oracle and the standard error of the paired difference at 2^14 chains
is about 0.4, so the bias is inside the bound; a wrong factor in T or V moves
the difference by tens.
"""
from math import pi

import numpy as np
import pytest

from . import _energy_parts_restatement as rs
from ._models import _dev, box, model_dict

pytestmark = pytest.mark.gpu

RTOL = 2e-11


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


def worst(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def spec_for(golden_params, key):
    """The golden model `key` (a tag), the golden 'box' model of `key`
    particles where there is one, the same family otherwise."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    if isinstance(key, str):
        return Spec(**golden_params[key]['spec'])
    if key in rs.GOLDEN_SIZES:
        return Spec(**golden_params[rs.GOLDEN_SIZES[key]]['spec'])
    return Spec(**rs.model_spec_args(key))


@pytest.fixture(scope='module')
def engines(golden_params):
    from phd_qmclib_amd.engine import ModelEngine
    cache = {}

    def get(key):
        if key not in cache:
            spec = spec_for(golden_params, key)
            cache[key] = (ModelEngine(spec.cfc_spec), spec,
                          model_dict(spec.cfc_spec))
        return cache[key]
    yield get
    for e, _, _ in cache.values():
        e.close()


@pytest.fixture(scope='module')
def reference_rows(engines):
    """The restatement's rows of the parity pool of a model, for the three
    window sets of `parity_windows`: computed once, shared, left unchanged."""
    cache = {}

    def get(key):
        if key not in cache:
            _, spec, p = engines(key)
            L, rm = float(spec.supercell_size), spec.tbf_contact_cutoff
            pool = rs.parity_pool(spec.boson_number, L, rm)
            rows = []
            for ranges in rs.parity_windows(rm):
                assert rs.edge_free(pool, ranges, L)
                r = rs.energy_parts(pool, ranges, p)
                r.setflags(write=False)
                rows.append((ranges, r))
            pool.setflags(write=False)
            cache[key] = (pool, rows)
        return cache[key]
    return get


# ---- 1. restatement parity ---------------------------------------------------
@pytest.mark.parametrize('key', rs.PARITY_SIZES + rs.EXTRA_MODELS)
def test_restatement_parity(engines, reference_rows, key):
    eng, spec, p = engines(key)
    n, L = spec.boson_number, float(spec.supercell_size)
    pool, rows = reference_rows(key)
    assert pool.shape == ((6 if n < 260 else 3), n)
    assert np.any(pool < 0) and np.any(pool >= L)
    for ranges, ref in rows:
        got = eng.energy_parts(pool, ranges)
        assert got.shape == ref.shape == (pool.shape[0], 4 + len(ranges))
        print(key, len(ranges), 'worst relative deviation per column',
              [worst(got[:, c], ref[:, c]) for c in range(got.shape[1])])
        assert close(got, ref)
        if n == 1:
            assert not got[:, 4:].any()
        elif n >= 6 and len(ranges):
            assert np.all(got[:, 4] > 0)      # the planted pairs count
    if p['params']['is_ideal']:
        # weight 1: the plain coincidence count
        ranges, ref = rows[0]
        got = eng.energy_parts(pool, ranges)
        counts = got[:, 4:] * (2.0 * np.asarray(ranges))
        assert np.allclose(counts, np.rint(counts), atol=1e-9)


# ---- 2. consistency with the steppers' code ------------------------------------
@pytest.mark.parametrize('key', (8, 16, 24, 37, 64, 100, 128, 260, 512,
                                 'defect24', 'ideal16'))
def test_matches_evaluate(engines, reference_rows, key):
    eng, spec, _ = engines(key)
    pool, _ = reference_rows(key)
    ev = eng.evaluate(pool)
    got = eng.energy_parts(pool)
    assert got.shape == (pool.shape[0], 4)
    assert close(got[:, 0], ev.energy)
    assert close(got[:, 1], (ev.drift ** 2).sum(axis=1))
    # (the remainder inherits the absolute error of its three terms)
    T = (ev.drift ** 2).sum(axis=1)
    scale = np.maximum(1.0, np.abs(ev.energy) + T + got[:, 2])
    assert np.all(np.abs(got[:, 3] - ((ev.energy - T) - got[:, 2]))
                  <= RTOL * scale)


# ---- 3. call-form agreement -------------------------------------------------
@pytest.mark.parametrize('key', (16, 37, 100, 'defect24'))
def test_call_forms_agree(engines, key):
    from phd_qmclib_amd.engine import DeviceBuffer
    eng, spec, p = engines(key)
    n, L = spec.boson_number, float(spec.supercell_size)
    rng = np.random.RandomState(700 + n)
    W = 70
    pos = L * (3.0 * rng.random_sample((W, n)) - 1.0)
    ranges = rs.parity_windows(spec.tbf_contact_cutoff)[0]
    K = len(ranges)
    host = eng.energy_parts(pos, ranges)
    assert np.array_equal(host, eng.energy_parts(pos, ranges))    # same bits
    dpos = _dev(eng, pos)
    dparts = DeviceBuffer((W, 4 + K), eng.device)
    eng.energy_parts_dev(W, dpos.ptr, ranges, dparts.ptr)
    eng.sync()
    assert np.array_equal(dparts.download(), host)
    # K = 0 through the device call: the four leading columns, same bits
    d4 = DeviceBuffer((W, 4), eng.device)
    eng.energy_parts_dev(W, dpos.ptr, (), d4.ptr)
    eng.sync()
    assert np.array_equal(d4.download(), host[:, :4])
    # weighted sums; a zero weight removes a row
    w = rng.random_sample(W) + 0.25
    w[5] = 0.0
    w[W - 1] = 0.0
    dw = _dev(eng, w)
    dsums = DeviceBuffer((4 + K, 2), eng.device)
    dwsum = DeviceBuffer((1,), eng.device)
    for weights, wptr in ((np.ones(W), 0), (w, dw.ptr)):
        eng.energy_parts_reduce_dev(W, dpos.ptr, wptr, ranges, dsums.ptr,
                                    dwsum.ptr)
        eng.sync()
        sums, wsum = dsums.download(), dwsum.download()
        assert close(sums[:, 0], (weights[:, None] * host).sum(axis=0))
        assert close(sums[:, 1], (weights[:, None] * host ** 2).sum(axis=0))
        assert close(wsum[0], weights.sum())
        eng.energy_parts_reduce_dev(W, dpos.ptr, wptr, ranges, dsums.ptr,
                                    dwsum.ptr)
        eng.sync()
        assert np.array_equal(dsums.download(), sums)             # same bits
    keep = w > 0
    s2, ws2 = eng.energy_parts_weighted(pos[keep], w[keep], ranges)
    assert close(s2, sums) and close(ws2, wsum[0])
    for b in (dpos, dparts, d4, dw, dsums, dwsum):
        b.close()


def test_physical_funcs_broadcast(engines, golden_params):
    from phd_qmclib_amd import mrbp_qmc
    eng, spec, _ = engines(16)
    rng = np.random.RandomState(12)
    conf = np.zeros((2, 3, 2, 16))
    conf[:, :, 0, :] = 16.0 * rng.random_sample((2, 3, 16))
    pf = mrbp_qmc.PhysicalFuncs.from_model_spec(spec)
    out = pf.energy_parts(conf, (0.3, 0.9))
    assert out.shape == (2, 3, 6)
    want = eng.energy_parts(conf[:, :, 0, :].reshape(6, 16), (0.3, 0.9))
    assert np.array_equal(out.reshape(6, 6), want)
    assert pf.energy_parts(conf[0, 0]).shape == (4,)
    with pytest.raises(ValueError):
        pf.energy_parts(conf, (5.0,))


# ---- 4. argument errors at the C level ----------------------------------------
def test_c_level_argument_errors(engines):
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd.engine import DeviceBuffer
    lib = _lib.load()
    eng, spec, _ = engines(16)             # L = 16, |rm| = 4
    ideal, _, _ = engines('ideal16')
    pos = 16.0 * np.random.RandomState(2).random_sample((4, 16))
    out = np.zeros((4, 4 + 17))
    dpos = _dev(eng, pos)
    dout = DeviceBuffer(out.shape, eng.device)

    def dp(a):
        return None if a is None else a.ctypes.data_as(_lib._dp)

    def refused(rc):
        assert rc != 0
        assert lib.qmc_last_error().decode().startswith('qmc_')

    def host(e, ranges, k=None, p=pos, o=out):
        rg = None if ranges is None else np.asarray(ranges, dtype=np.float64)
        k = (0 if rg is None else rg.size) if k is None else k
        return lib.qmc_energy_parts(e._h, 4, dp(p), k, dp(rg), dp(o))

    assert host(eng, (0.5, 4.0)) == 0 and host(ideal, (8.0,)) == 0
    assert host(eng, None, 0) == 0
    bad = (np.full(17, 0.1), (0.0,), (-0.5,), (np.nan,), (np.inf,), (8.5,),
           (0.5, 4.5))
    for ranges in bad:
        refused(host(eng, ranges))
        rg = np.asarray(ranges, dtype=np.float64)
        refused(lib.qmc_energy_parts_dev(eng._h, 4, dpos.ptr, rg.size, dp(rg),
                                         dout.ptr))
        refused(lib.qmc_energy_parts_reduce_dev(eng._h, 4, dpos.ptr, None,
                                                rg.size, dp(rg), dout.ptr,
                                                None))
    refused(host(ideal, (8.5,)))           # beyond L/2 on an ideal model too
    refused(host(eng, (0.5,), k=-1))
    refused(host(eng, None, k=1))          # NULL pointers
    refused(host(eng, (0.5,), p=None))
    refused(host(eng, (0.5,), o=None))
    refused(lib.qmc_energy_parts(None, 4, dp(pos), 0, None, dp(out)))
    refused(lib.qmc_energy_parts_dev(eng._h, 4, None, 0, None, dout.ptr))
    refused(lib.qmc_energy_parts_dev(eng._h, 4, dpos.ptr, 0, None, None))
    refused(lib.qmc_energy_parts_reduce_dev(eng._h, 4, dpos.ptr, None, 0,
                                            None, None, None))
    refused(lib.qmc_vmc_energy_parts(None, 0, None, dp(out)))
    dpos.close()
    dout.close()


# ---- 5. VMC statistics ----------------------------------------------------------
def vmc_rows(spec, ranges, seed):
    """2^14 chains of single-particle sweeps -> (rows of the chains, the
    ensemble's EnergyComponents with and without windows)."""
    from phd_qmclib_amd.mrbp_qmc import vmc
    s = vmc.EnsembleSampling(spec, 1.0, 1 << 14, rng_seed=seed,
                             move='particle')
    s.init_random(seed)
    next(s.blocks(200))
    before = s.confs()
    rows = s.engine.energy_parts(before, ranges)
    ec = s.energy_components(ranges)
    ec0 = s.energy_components()
    assert np.array_equal(s.confs(), before)        # the chains: only read
    s.close()
    return rows, ec, ec0


def mean_err(x):
    return x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(x.shape[0])


def check_components(ec, rows, ranges):
    mean, err = mean_err(rows)
    got = np.array([ec.total, ec.kinetic, ec.lattice, ec.interaction,
                    *ec.contact])
    got_err = np.array([ec.total_err, ec.kinetic_err, ec.lattice_err,
                        ec.interaction_err, *ec.contact_err])
    assert got.shape == mean.shape == (4 + len(ranges),)
    assert np.allclose(got, mean, rtol=1e-11, atol=1e-11)
    assert np.allclose(got_err, err, rtol=1e-6,
                       atol=1e-7 * np.max(np.abs(mean)))
    assert np.array_equal(ec.contact_ranges, np.asarray(ranges, dtype=float))


def test_vmc_ideal_gas():
    n = 8
    spec = box(n=n, gint=0)
    rows, ec, ec0 = vmc_rows(spec, (), 11)
    e0 = spec.obf_params.param_e0
    assert np.all(np.abs(rows[:, 0] - n * e0) <= 1e-10 * n * e0)
    mean, err = mean_err(rows)
    z = mean[3] / err[3]
    print('ideal gas: <T> =', mean[1], '<V> =', mean[2], '<I> =', mean[3],
          '+-', err[3], ' z =', z)
    assert -4.5 <= z <= 4.5
    check_components(ec, rows, ())
    check_components(ec0, rows, ())
    assert ec.coupling == 0.0 and ec.contact.shape == (0,)


def test_vmc_interaction_energy_two_routes():
    n = 8
    spec = box(n=n, gint=20, depth=2 * pi ** 2)
    ranges = (0.02, 0.05)
    rows, ec, ec0 = vmc_rows(spec, ranges, 12)
    assert abs(ec.coupling - 20.0) <= 1e-12 * 20.0
    diff = rows[:, 3] - ec.coupling * rows[:, 5]
    dm, de = diff.mean(), diff.std(ddof=1) / np.sqrt(diff.size)
    mean, err = mean_err(rows)
    print('gint = 20: <I> =', mean[3], '+-', err[3],
          ' g C(0.02) =', 20 * mean[4], '+-', 20 * err[4],
          ' g C(0.05) =', 20 * mean[5], '+-', 20 * err[5],
          ' D =', dm, '+-', de, ' z =', dm / de)
    assert -4.5 <= dm / de <= 4.5
    check_components(ec, rows, ranges)
    check_components(ec0, rows[:, :4], ())
    assert ec0.coupling == ec.coupling


# ---- 6. DMC mixed estimate -------------------------------------------------------
def test_dmc_mixed_estimate(engines):
    from phd_qmclib_amd.mrbp_qmc import dmc
    from phd_qmclib_amd.qmc_base import dmc as dmc_base
    n, slots, nw = 16, 12, 9
    _, spec, p = engines(16)
    rng = np.random.RandomState(21)
    pos = 16.0 * rng.random_sample((slots, n))
    pos[:, 1] = np.mod(pos[:, 0] + 0.04, 16.0)       # a pair inside 0.1
    pos[nw:] = 0.123                                 # garbage in the dead slots
    confs = np.zeros((slots, 2, n))
    confs[:, 0, :] = pos
    confs[:, 1, :] = 77.0
    weight = rng.random_sample(slots) * 2.0 + 0.1
    weight[nw:] = 1e9                                # dead slots must not count
    props = dmc_base.StateProps(np.zeros(slots), weight,
                                np.arange(slots) >= nw)
    state = dmc_base.State(confs, props, 0.0, float(weight[:nw].sum()), nw,
                           0.0, 0.0, slots)
    ranges = (0.1, 0.5)
    live = pos[:nw]
    assert rs.edge_free(live, ranges, 16.0)
    rows = rs.energy_parts(live, ranges, p)
    w = weight[:nw]
    want = (w[:, None] * rows).sum(axis=0) / w.sum()
    s = dmc.Sampling(spec, 1e-3, slots, nw, rng_seed=1)
    ec = s.energy_components(state, ranges)
    got = np.array([ec.total, ec.kinetic, ec.lattice, ec.interaction,
                    *ec.contact])
    print('DMC mixed: worst relative deviation', worst(got, want))
    assert close(got, want)
    assert np.all(ec.contact > 0)
    var = (w[:, None] * (rows - want) ** 2).sum(axis=0) / w.sum()
    got_err = np.array([ec.total_err, ec.kinetic_err, ec.lattice_err,
                        ec.interaction_err, *ec.contact_err])
    assert np.allclose(got_err, np.sqrt(var / (nw - 1)), rtol=1e-6)
    assert abs(ec.coupling - 2.0) <= 2e-12
    ec0 = s.energy_components(state)
    assert ec0.contact.shape == (0,) and close(ec0.total, want[0])
