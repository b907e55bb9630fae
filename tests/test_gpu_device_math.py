"""The device primitives of the stepping kernels (csrc/qmc_math.h,
csrc/qmc_device.h) run on the GPU through `qmc_engine_probe` -- the
`__device__` functions themselves, with an engine's model constants and
device tables -- against mpmath at 40 digits, at the inputs their callers
produce and densely at the edges where such code goes wrong (row edges,
quadrant boundaries, the closing row of a table, z_a +- ulp, k L +- ulp).

The parity suite compares energies, drifts and log psi at 2e-11 max(1, |x|);
each bound here is the one the code states, five orders of magnitude tighter,
so a primitive that lost digits, or went wrong in a narrow band of inputs, is
caught here even where the parity tests still pass.

Measured worst cases on the MI355X are quoted in each test (and in DESIGN.md
section 2); set QMC_PROBE_REPORT=1 to print them.
"""
import math
import os

import numpy as np
import pytest

from ._models import spec_from_golden
from .test_gpu_parity import RTOL, close, worst

mpmath = pytest.importorskip('mpmath')
mp = mpmath.mp

pytestmark = pytest.mark.gpu

GOLDEN_TAGS = ['box8', 'box16', 'box37', 'box48', 'box64', 'box100', 'box126',
               'box128', 'box512', 'deep16', 'deep100', 'defect24', 'odd24']
ULP_BOUND = 2.0


def _report(name, value, at):
    if os.environ.get('QMC_PROBE_REPORT'):
        print(f'\nWORST {name}: {value!r} at {at!r}')


def _mpf(x):
    return mpmath.mpf(float(x))


def _ulps(got, ref):
    """|got - ref| in units of the last place of the double nearest ref."""
    got = np.asarray(got, dtype=np.float64).ravel()
    out = np.empty(got.size)
    for k, (g, r) in enumerate(zip(got, ref)):
        sp = np.spacing(abs(float(r))) if float(r) != 0.0 else 5e-324
        out[k] = float(abs(_mpf(g) - r)) / sp
    return out


def _around(xs, k=3):
    """every x and its k neighbours below and above (doubles)."""
    out = []
    for x in xs:
        x = float(x)
        lo = hi = x
        out.append(x)
        for _ in range(k):
            lo = math.nextafter(lo, -math.inf)
            hi = math.nextafter(hi, math.inf)
            out += [lo, hi]
    return np.array(out)


@pytest.fixture(scope='module')
def dps():
    with mp.workdps(40):
        yield


@pytest.fixture(scope='module')
def eng(golden_params):
    """an engine of the benchmarked model (the model-free primitives)"""
    from phd_qmclib_amd.engine import ModelEngine
    e = ModelEngine(spec_from_golden(golden_params, 'box64').cfc_spec)
    yield e
    e.close()


def _sweep_specs():
    import json
    from phd_qmclib_amd.mrbp_qmc import Spec
    from .conftest import GOLDEN
    with open(os.path.join(GOLDEN, 'sweep.json')) as fp:
        recs = json.load(fp)
    return [(r['tag'], Spec(**r['spec'])) for r in recs]


@pytest.fixture(scope='module')
def model_engines(golden_params):
    """(tag, engine) of the golden models and 20 sweep models (non-integer
    box lengths, depths 0-250, ratios 0.15-4)."""
    from phd_qmclib_amd.engine import ModelEngine
    out = [(t, ModelEngine(spec_from_golden(golden_params, t).cfc_spec))
           for t in GOLDEN_TAGS]
    out += [(t, ModelEngine(s.cfc_spec)) for t, s in _sweep_specs()[:20]]
    yield out
    for _, e in out:
        e.close()


def _mparams(e):
    return e._params


# ------------------------------------------------------------ sin / cos ----
def test_sincos_halfpi_within_2ulp(eng, golden_params, dps):
    """sincos_halfpi(u) = (sin, cos)(pi u / 2), |u| < 2^20: quadrant split by
    rint and the sin/cos kernels.  Edges: u = k/2 +- 1..3 ulp for k = -16..16
    (both sides of every quadrant boundary and of every rounding tie of rint),
    u = 2 z / L over [0, L) for the golden box lengths.
    Measured: 1.60 ulp at u = 0.4947337289966274."""
    rng = np.random.default_rng(11)
    u = [_around(np.arange(-16, 17) / 2.0, 3),
         rng.uniform(-4, 4, 4000), rng.uniform(-2.0 ** 20, 2.0 ** 20, 2000),
         np.array([0.0, -0.0, 1e-300, -1e-300, 2.0 ** 20 - 0.5,
                   -(2.0 ** 20 - 0.5)])]
    for tag in ('box37', 'box64', 'box100', 'box128'):
        L = float(golden_params[tag]['params']['supercell_size'])
        z = np.concatenate([rng.uniform(0, L, 500),
                            _around(np.arange(0, 9) * L / 8.0, 2)])
        z = z[(z >= 0) & (z < L)]
        u.append(z * (2.0 / L))
    u = np.concatenate(u)
    out = eng.probe('sincos_halfpi', u)
    ref_s = [mpmath.sinpi(_mpf(x) / 2) for x in u]
    ref_c = [mpmath.cospi(_mpf(x) / 2) for x in u]
    es, ec = _ulps(out[:, 0], ref_s), _ulps(out[:, 1], ref_c)
    k = int(np.argmax(np.maximum(es, ec)))
    _report('sincos_halfpi ulp', float(max(es.max(), ec.max())), u[k])
    assert es.max() <= ULP_BOUND, (u[np.argmax(es)], es.max())
    assert ec.max() <= ULP_BOUND, (u[np.argmax(ec)], ec.max())


def test_sincos_kernel_within_2ulp(eng, dps):
    """sincos_kernel(x), |x| <= pi/4 (fdlibm's minimax coefficients).
    Edges: +-pi/4, 0, +-tiny.  Measured: 1.16 ulp at x = -0.774418822960846."""
    q = float(mpmath.pi / 4)
    rng = np.random.default_rng(12)
    x = np.concatenate([_around([q, -q], 4)[np.abs(_around([q, -q], 4)) <=
                                            q],
                        [0.0, -0.0, 1e-300, -1e-300, 2.0 ** -30, -2.0 ** -30],
                        rng.uniform(-q, q, 6000)])
    out = eng.probe('sincos_kernel', x)
    es = _ulps(out[:, 0], [mpmath.sin(_mpf(v)) for v in x])
    ec = _ulps(out[:, 1], [mpmath.cos(_mpf(v)) for v in x])
    k = int(np.argmax(np.maximum(es, ec)))
    _report('sincos_kernel ulp', float(max(es.max(), ec.max())), x[k])
    assert es.max() <= ULP_BOUND and ec.max() <= ULP_BOUND, (x[k], es.max(),
                                                             ec.max())


# --------------------------------------------------------------- exp / log ----
def test_exp_bounded_ulp(eng, model_engines, dps):
    """exp_bounded(x), |x| < 700.  Edges: n ln 2 +- ulp (the reduction's
    rounding ties), +-699.9, and the barrier arguments 2 x of every golden and
    sweep model (x = kp1 (z_cell - 1 + z_b / 2) over the barrier).
    Bound 2.5 ulp: the "<= 2 ulp" qmc_math.h used to state does not hold for
    the degree-12 Taylor sum (its remainder alone is ~0.8 ulp); measured
    2.25 ulp at x = -298.39986123105643."""
    rng = np.random.default_rng(13)
    ln2 = float(mpmath.log(2))
    xs = [_around(np.arange(-1000, 1001) * ln2 / 1.0, 1),
          _around((np.arange(-1000, 1000) + 0.5) * ln2, 1),
          [699.9, -699.9, 0.0, -0.0, 1e-300, -1e-300],
          rng.uniform(-699.9, 699.9, 4000), rng.uniform(-40, 40, 4000)]
    for _, e in model_engines:
        p = _mparams(e)
        if p.is_free:
            continue
        zb = p.lattice_ratio / (1.0 + p.lattice_ratio)
        xs.append(2.0 * p.param_kp1 * zb * rng.uniform(-0.5, 0.5, 200))
    x = np.concatenate(xs)
    x = x[np.abs(x) < 700.0]
    out = eng.probe('exp_bounded', x)[:, 0]
    err = _ulps(out, [mpmath.exp(_mpf(v)) for v in x])
    k = int(np.argmax(err))
    _report('exp_bounded ulp', float(err[k]), x[k])
    assert err.max() <= 2.5, (x[k], err[k])


def _log_err(got, x):
    ref = [mpmath.log(_mpf(v)) for v in x]
    return np.array([float(abs(_mpf(g) - r) / (1 + abs(r)))
                     for g, r in zip(got, ref)])


def test_log_pos_absolute_bound(eng, dps):
    """log_pos(x), positive normal x: |error| <= 1.25e-16 (1 + |log x|)
    (qmc_math.h).  Edges: every row edge of the 256-row table +- 1..2 ulp,
    [1 - 2^-20, 1 + 2^-20] densely, 1 +- 2^-33, 10^-300 .. 10^300, the
    smallest normal.  Measured: 1.10e-16 (1 + |log x|) at x = 2.42e111."""
    rng = np.random.default_rng(14)
    edges = 0.5 + np.arange(0, 257) / 512.0
    xs = [_around(edges, 2), _around(edges * 2.0, 2),
          _around(edges * 2.0 ** -700, 1), _around(edges * 2.0 ** 700, 1),
          1.0 + np.linspace(-2.0 ** -20, 2.0 ** -20, 4001),
          _around([1.0 - 2.0 ** -33, 1.0 + 2.0 ** -33, 1.0, 2.0 ** -33], 2),
          10.0 ** rng.uniform(-300, 300, 4000), rng.uniform(0, 1, 3000),
          [2.2250738585072014e-308, 1.7976931348623157e308]]
    x = np.concatenate(xs)
    x = x[x >= 2.2250738585072014e-308]
    out = eng.probe('log_pos', x)[:, 0]
    err = _log_err(out, x)
    k = int(np.argmax(err))
    _report('log_pos err/(1+|log x|)', float(err[k]), x[k])
    assert err.max() <= 1.25e-16, (x[k], err[k])


def test_log_pos_device_no_worse_than_host_copy(eng, dps):
    """The sweep of qmc_log_table_info (its LCG, 2 x 10^5 arguments of every
    size, near 1 and in (0, 1), and the row edges) through the DEVICE's
    log_pos: its worst deviation is no larger than what the host copy
    reports for itself."""
    import ctypes as C
    from phd_qmclib_amd import _lib
    lib = _lib.load()
    rows, host_err = C.c_int32(0), C.c_double(0)
    assert lib.qmc_log_table_info(C.byref(rows), C.byref(host_err)) == 0
    M = (1 << 64) - 1
    state = 0x9E3779B97F4A7C15
    xs = []
    for i in range(200000):
        state = (state * 6364136223846793005 + 1442695040888963407) & M
        u = float(state >> 11) * (1.0 / 9007199254740992.0)
        if i < 100000:
            x = math.pow(10.0, -300.0 + 600.0 * u)
        elif i < 150000:
            x = 1.0 + (u - 0.5) * 1e-3 * (i % 1000)
        else:
            x = u + 1e-17
        xs.append(x)
    for r in range(rows.value + 1):
        x = 0.5 + r / (2.0 * rows.value)
        xs += [math.nextafter(x, 0.0), x, math.nextafter(x, 2.0)]
    x = np.array(xs)
    out = eng.probe('log_pos', x)[:, 0]
    err = _log_err(out, x)
    _report('log_pos on the host sweep', float(err.max()), host_err.value)
    assert err.max() <= host_err.value * (1 + 1e-6), (err.max(),
                                                       host_err.value)


# ---------------------------------------------------- division / sqrt ----
def _pow2_edges(lo, hi):
    return _around(2.0 ** np.arange(lo, hi + 1), 1)


def _signed_pairs(rng, n, emax):
    a = rng.uniform(1, 2, n) * 2.0 ** rng.integers(-emax, emax, n)
    return a * rng.choice([-1.0, 1.0], n)


def test_divisions_and_sqrt(eng, dps):
    """fast_div, fast_rcp, fast_sqrt <= 2 ulp; pair_div relative 2.5e-15;
    |x|, |y| in 2^+-500 with y at powers of two +- ulp.  (qmc_math.h stated
    8e-16 for pair_div from eps_rcp = 2^-25; the hardware estimate is
    coarser: measured 1.86e-15 at x = 1.7767074890743405e+143,
    y = -1.5979141888958425e+147.)  Measured: fast_div, fast_rcp and
    fast_sqrt 0.5 ulp."""
    rng = np.random.default_rng(15)
    y = np.concatenate([_pow2_edges(-500, 500), -_pow2_edges(-60, 60),
                        _signed_pairs(rng, 6000, 500)])
    x = np.concatenate([_signed_pairs(rng, y.size - 2000, 500),
                        rng.uniform(-2, 2, 2000)])
    rng.shuffle(x)
    xy = np.stack([x, y], 1)
    ref = [_mpf(a) / _mpf(b) for a, b in xy]
    for fn in ('fast_div', 'pair_div'):
        got = eng.probe(fn, xy)[:, 0]
        if fn == 'fast_div':
            err = _ulps(got, ref)
            k = int(np.argmax(err))
            _report('fast_div ulp', float(err[k]), tuple(xy[k]))
            assert err[k] <= ULP_BOUND, (xy[k], err[k])
        else:
            rel = np.array([float(abs(_mpf(g) - r) / abs(r))
                            for g, r in zip(got, ref)])
            k = int(np.argmax(rel))
            _report('pair_div rel', float(rel[k]), tuple(xy[k]))
            assert rel[k] <= 2.5e-15, (xy[k], rel[k])
    got = eng.probe('fast_rcp', y)[:, 0]
    err = _ulps(got, [1 / _mpf(b) for b in y])
    _report('fast_rcp ulp', float(err.max()), y[int(np.argmax(err))])
    assert err.max() <= ULP_BOUND, (y[int(np.argmax(err))], err.max())
    s = np.abs(np.concatenate([y, _pow2_edges(-500, 500) * 1.5]))
    got = eng.probe('fast_sqrt', s)[:, 0]
    err = _ulps(got, [mpmath.sqrt(_mpf(v)) for v in s])
    _report('fast_sqrt ulp', float(err.max()), s[int(np.argmax(err))])
    assert err.max() <= ULP_BOUND, (s[int(np.argmax(err))], err.max())


def test_pair_div_float_within_2_float_ulp(eng, dps):
    """float pair_div (reduced-precision pair loop): x * rcp(y) within 2
    float ulp of the exact quotient, |x|, |y| in 2^+-60.  Measured: 1.74
    float ulp at x = -61273.28125, y = 2.1803181482482614e-10."""
    rng = np.random.default_rng(16)
    y = np.concatenate([_pow2_edges(-60, 60), _signed_pairs(rng, 6000, 60)])
    x = _signed_pairs(rng, y.size, 60)
    xy = np.stack([x, y], 1).astype(np.float32).astype(np.float64)
    got = eng.probe('pair_div_f32', xy)[:, 0]
    assert np.all(got.astype(np.float32) == got)
    err = np.array([float(abs(_mpf(g) - _mpf(a) / _mpf(b))) /
                    float(np.spacing(np.float32(abs(a / b))))
                    for g, (a, b) in zip(got, xy)])
    k = int(np.argmax(err))
    _report('pair_div f32 ulp', float(err[k]), tuple(xy[k]))
    assert err[k] <= ULP_BOUND, (xy[k], err[k])


# ------------------------------------------------------ trig row table ----
def _trig_rows(e):
    import ctypes as C
    rows, err = C.c_int32(0), C.c_double(0)
    assert e._lib.qmc_model_trig_table_info(C.byref(e._params), C.byref(rows),
                                            C.byref(err)) == 0
    return rows.value


def test_trig_table_absolute_bound(model_engines, dps):
    """trig_tab_load + trig_tab_finish: sin / cos of pi z / L and of k2 z from
    the row table within 3.5e-16 absolute, z in [0, L) for the golden and 20
    sweep models.  Edges: every row edge +- 1 ulp, z = 0, L - ulp.
    Measured: 1.59e-16 (box64, z = 33.929)."""
    rng = np.random.default_rng(17)
    overall = (0.0, None)
    for tag, e in model_engines:
        rows = _trig_rows(e)
        if not rows:
            continue
        p = _mparams(e)
        L, k2 = p.supercell_size, p.param_k2
        h = L / rows
        edges = np.unique(np.r_[0, 1, rows - 1, rows,
                                rng.integers(0, rows + 1, 200)])
        z = np.concatenate([_around(edges * h, 1),
                            rng.uniform(0, L, 400),
                            [0.0, math.nextafter(L, 0.0)]])
        # (z just below L can round to row index `rows`: that position takes
        # the direct evaluation, test_trig_table_fallback_is_wave_wide)
        inv_h = rows / L
        z = z[(z >= 0) & (z < L) & (np.floor(z * inv_h) < rows)]
        # whole wavefronts of valid positions: the table path for all
        out = e.probe('trig_tab', z)
        assert np.all(out[:, 4] == 1.0), tag
        piL = mp.pi / _mpf(L)
        worst_err = 0.0
        for zi, o in zip(z, out):
            a1, a2 = piL * _mpf(zi), _mpf(k2) * _mpf(zi)
            ref = (mpmath.sin(a1), mpmath.cos(a1), mpmath.sin(a2),
                   mpmath.cos(a2))
            err = max(float(abs(_mpf(g) - r)) for g, r in zip(o[:4], ref))
            if err > worst_err:
                worst_err, at = err, zi
        if worst_err > overall[0]:
            overall = (worst_err, (tag, at))
        assert worst_err <= 3.5e-16, (tag, rows, at, worst_err)
    _report('trig_tab abs', overall[0], overall[1])


def test_trig_table_fallback_is_wave_wide(model_engines):
    """trig_tab_load returns false for the whole wavefront exactly when some
    lane's row index (int)(z rows / L) is outside the table -- z = L, z < 0,
    z just below L, one such lane in an otherwise valid wavefront -- and
    true otherwise (the caller then evaluates directly)."""
    rng = np.random.default_rng(18)
    for tag, e in model_engines[:6] + model_engines[-4:]:
        rows = _trig_rows(e)
        if not rows:
            continue
        L = _mparams(e).supercell_size
        inv_h = rows / L
        specials = [L, math.nextafter(L, 0.0), math.nextafter(L, 8 * L),
                    -0.0, -1e-300, -2.0 ** -60, math.nextafter(0.0, -1.0),
                    -L / rows, -L / (2 * rows), -0.5 * L, 1.5 * L, 2 * L,
                    math.nextafter(L, 0.0) * (1 - 2.0 ** -52)]
        waves = []
        for s in specials:
            w = rng.uniform(0, L, 64)
            w[rng.integers(64)] = s
            waves.append(w)
        waves.append(rng.uniform(0, L, 64))
        z = np.concatenate(waves)
        out = e.probe('trig_tab', z)
        for wi in range(len(waves)):
            sl = slice(64 * wi, 64 * wi + 64)
            ok = out[sl, 4]
            assert np.all(ok == ok[0]), (tag, wi, 'not wave-uniform')
            idx = [int(v * inv_h) if abs(v * inv_h) < 2 ** 31 else -1
                   for v in z[sl]]
            want = all(0 <= r < rows for r in idx)
            assert bool(ok[0]) == want, (tag, z[sl][np.argmin(ok)], idx)


# ------------------------------------------------------- one-body factor ----
def _ob_rows(e):
    import ctypes as C
    m1, m2, err = C.c_int32(0), C.c_int32(0), C.c_double(0)
    assert e._lib.qmc_model_one_body_table_info(
        C.byref(e._params), C.byref(m1), C.byref(m2), C.byref(err)) == 0
    return m1.value, m2.value


def _ob_ref(p, zc, barrier):
    """f1'/f1 and log f1 of mrbp_qmc/model.py:404-464 at cell position zc
    (mpf), restated: the well's cos(k1 (zc - z_a/2)) scaled by cf, the
    barrier's cosh(kp1 (zc - 1 + z_b/2))."""
    za = _mpf(1.0 / (1.0 + p.lattice_ratio))
    zb = _mpf(p.lattice_ratio / (1.0 + p.lattice_ratio))
    if barrier:
        kp1 = _mpf(p.param_kp1)
        x = kp1 * (zc - 1 + zb / 2)
        return (kp1 * mpmath.tanh(x), mpmath.log(mpmath.cosh(x)),
                kp1 ** 2 / mpmath.cosh(x) ** 2)
    v0, e0 = _mpf(p.lattice_depth), _mpf(p.param_e0)
    cf = mpmath.sqrt(1 + v0 / e0 * mpmath.sinh(mpmath.sqrt(v0 - e0) * zb / 2)
                     ** 2)
    k1 = _mpf(p.param_k1)
    x = k1 * (zc - za / 2)
    return (-k1 * mpmath.tan(x), mpmath.log(cf * mpmath.cos(x)),
            -k1 ** 2 / mpmath.cos(x) ** 2)


def _device_frac(z):
    """v_fract_f64: z - floor(z), below 1"""
    f = z % 1.0
    return f if f < 1.0 else 1.0 - 2.0 ** -53


def _ob_positions(rng, L, za, m1, m2, nedge=150):
    """row edges (a random subset of each region's, with the first and the
    last) +- ulp, z_a +- 3 ulp, cell position -> 1, each in a random cell of
    [-2L, 3L); integer z; random z; z just below 0"""
    e1 = np.unique(np.r_[0, m1, rng.integers(0, m1 + 1, nedge)])
    e2 = np.unique(np.r_[0, m2, rng.integers(0, m2 + 1, nedge)])
    zc = np.concatenate([e1 * (za / m1), za + e2 * ((1 - za) / m2)])
    zc = np.concatenate([_around(zc, 1), _around([za], 3),
                         1.0 - np.arange(1, 9) * 2.0 ** -53,
                         rng.uniform(0, 1, 200)])
    zc = zc[(zc >= 0) & (zc < 1)]
    cells = np.floor(np.array([-2 * L, -L, -1, 0, 1, 3, L - 1, 2 * L]))
    z = zc + rng.choice(cells, zc.size)
    ints = np.arange(-2 * int(L), 3 * int(L)).astype(float)
    z = np.concatenate([z, rng.choice(ints, min(ints.size, 200)),
                        rng.uniform(-2 * L, 3 * L, 600),
                        -rng.uniform(0, 1e-12, 20)])
    return z[(z >= -2 * L) & (z < 3 * L)]


def _ob_errors(p, z, ldz, logf, near, rtol, slope_ulps=0.0):
    """worst err / tol of ldz and log f1, tol = rtol max(1, |f|) + slope_ulps
    ulp(1) |df/dz| (a position off by that many ulp of the cell position);
    near a joint of the piecewise closed form (z_a, the cell edge) either
    side's form is the reference (they agree there only to the precision of
    the matching)."""
    za = 1.0 / (1.0 + p.lattice_ratio)
    dz = slope_ulps * 2.0 ** -52
    worst_r, at = 0.0, None
    for zi, g1, g2 in zip(z, ldz, logf):
        zc = _mpf(zi) - mpmath.floor(_mpf(zi))
        cands = [(zc, zc > za)]
        if abs(float(zc) - za) < near:
            cands.append((zc, not (zc > za)))
        if float(zc) < near:
            cands.append((zc + 1, True))
        if float(zc) > 1 - near:
            cands.append((zc - 1, False))
        best = math.inf
        for r1, r2, d1 in (_ob_ref(p, c, b) for c, b in cands):
            t1 = rtol * max(1, abs(float(r1))) + dz * abs(float(d1))
            t2 = rtol * max(1, abs(float(r2))) + dz * abs(float(r1))
            best = min(best, max(float(abs(_mpf(g1) - r1)) / t1,
                                 float(abs(_mpf(g2) - r2)) / t2))
        if best > worst_r:
            worst_r, at = best, zi
    return worst_r, at


def test_one_body_table_against_closed_forms(model_engines, dps):
    """one_body_tab<true, true>: f1'/f1 and log f1 from the polynomial rows
    within OB_TOL = 2e-15 max(1, |f|) (qmcwalk.hip, the builder's claim,
    which it checks only at its own sample points and not through the
    device's row map fmax(...) / fract) for z in [-2L, 3L): row edges,
    z_a +- ulp, cell position -> 1 (the closing row), integer and negative
    z.  The barrier flag exactly as z_a < frac(z).  Bound 2 OB_TOL
    max(1, |f|) + 2 ulp(1) |df/dz|: between the builder's sample points the
    fit is worse than OB_TOL (3.2e-15 for defect24 at z = 0.83077), and the
    row map u = (frac(z) + shift2) invh2 rounds the cell position by up to
    an ulp, which a steep factor turns into more (sweep06 at z = 1.79605:
    2.4e-14 where d(f1'/f1)/dz = 212; the closed form, below, stays at
    9e-16)."""
    rng = np.random.default_rng(19)
    overall = (0.0, None)
    ran = 0
    for tag, e in model_engines:
        p = _mparams(e)
        m1, m2 = _ob_rows(e)
        if not m1:
            continue
        ran += 1
        za = 1.0 / (1.0 + p.lattice_ratio)
        z = _ob_positions(rng, p.supercell_size, za, m1, m2)
        out = e.probe('one_body_tab', z)
        want = np.array([za < _device_frac(v) for v in z])
        assert np.array_equal(out[:, 2] == 1.0, want), tag
        w, at = _ob_errors(p, z, out[:, 0], out[:, 1], 1e-12, 4e-15, 2.0)
        if w > overall[0]:
            overall = (w, (tag, at))
        assert w <= 1.0, (tag, at, w)
    assert ran >= 20
    _report('one_body_tab err / tol', overall[0], overall[1])


def test_one_body_closed_form(model_engines, dps):
    """one_body (the direct evaluation): f1'/f1 and log f1 - xoff within
    1e-14 max(1, |f|) of the same reference.  Measured: 9.1e-16 (deep100,
    z = -99.2305)."""
    rng = np.random.default_rng(20)
    overall = (0.0, None)
    for tag, e in model_engines:
        p = _mparams(e)
        if p.is_free:
            continue
        za = 1.0 / (1.0 + p.lattice_ratio)
        z = _ob_positions(rng, p.supercell_size, za, 16, 16)[::3]
        out = e.probe('one_body', z)
        logf = np.log(out[:, 2]) - out[:, 3]
        w, at = _ob_errors(p, z, out[:, 0], logf, 1e-12, 1e-14)
        if w > overall[0]:
            overall = (w, (tag, at))
        assert w <= 1.0, (tag, at, w)
    _report('one_body err / 1e-14 max(1, |f|)', overall[0], overall[1])


# ------------------------------------------------------------- wrap_box ----
def test_wrap_box_is_the_reference_floor_mod(golden_params):
    """wrap_box(z, L) bit for bit against the reference's recast, Python's
    float floor-mod (py_mod, oracle/qmc_oracle.c), z in (-3L, 4L), for the
    golden box lengths and non-integer ones (2.1, 17.5, 0.3 * 7, the sweep's
    25.266): k L +- ulp, -2^-60, -L, 2L, random, in wavefronts that take the
    far branch and wavefronts that do not.  The one expected exception: -0.0,
    which wrap_box returns as -0.0 where py_mod gives +0.0; zeros are
    compared by value.  (The far branch gave -4.4e-16 for z = -6.3 - ulp at
    L = 2.1 before the fix in qmc_device.h.)"""
    import ctypes as C
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd.engine import ModelEngine, model_params_struct
    rng = np.random.default_rng(21)
    Ls = [64.0, 128.0, 37.0, 100.0, 2.1, 17.5, 0.3 * 7, 25.266]
    lib = _lib.load()
    mism = 0
    for L in Ls:
        # the golden N = 16 model with another box length (the probe's
        # wrap_box reads the engine's L; nothing else of the model is used)
        p = model_params_struct(spec_from_golden(golden_params,
                                                 'box16').cfc_spec)
        p.supercell_size = L
        h = C.c_void_p()
        _lib.check(lib.qmc_engine_create(C.byref(p), 0, None, C.byref(h)))
        e = ModelEngine.__new__(ModelEngine)
        e._lib, e._h, e._params = lib, h, p
        e.num_particles = int(p.boson_number)
        near = np.concatenate([_around(np.arange(-1, 3) * L, 3),
                               rng.uniform(-L, 2 * L, 640),
                               [-2.0 ** -60, -0.0, 0.0]])
        near = near[(near >= -L) & (near < 2 * L)]
        far = np.concatenate([_around(np.arange(-3, 5) * L, 3),
                              rng.uniform(-3 * L, 4 * L, 1280)])
        far = far[(far > -3 * L) & (far < 4 * L)]
        # near-only wavefronts, then mixed ones
        pad = (-len(near)) % 64
        near = np.concatenate([near, np.full(pad, 0.5 * L)])
        z = np.concatenate([near, far])
        got = e.probe('wrap_box', z)[:, 0]
        want = np.array([v % L for v in z])
        bad = ~((got == want) & ((got != 0) | (want == 0)))
        mism += int(bad.sum())
        assert not bad.any(), (L, z[bad][:5], got[bad][:5], want[bad][:5])
        assert np.all((got >= 0) & (got <= L)), L
        e.close()
    assert mism == 0


# ------------------------------------------------------------ RNG maps ----
def test_vmc_move_unit_exact(eng):
    """vmc_move_unit(w) = (w + 1/2) 2^-32 - 1/2 exactly, every word class:
    0, 2^31 - 1, 2^31, 2^32 - 1 and random words."""
    from fractions import Fraction
    rng = np.random.default_rng(22)
    w = np.concatenate([[0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1],
                        rng.integers(0, 2 ** 32, 4000)]).astype(np.float64)
    got = eng.probe('vmc_move_unit', w)[:, 0]
    want = [float((Fraction(int(v)) + Fraction(1, 2)) / 2 ** 32 -
                  Fraction(1, 2)) for v in w]
    assert np.array_equal(got, want)
    assert got[0] == 2.0 ** -33 - 0.5 and got[5] == 0.5 - 2.0 ** -33


def _normal_bound(u0, r):
    """log_pos's 1.25e-16 (1 + |log u0|) carried to r = sqrt(-2 log u0)
    (dr = dlog / r), plus 4 ulp of r (fast_sqrt, sincos_halfpi, products)"""
    return (1.25e-16 * (1 + abs(math.log(u0))) / r +
            4 * float(np.spacing(r)))


def test_normal_from_words(eng, dps):
    """dmc_normal2 after Philox: (w0, w1) -> u = (w + 1/2) 2^-32 ->
    r = sqrt(-2 log u0), (g0, g1) = r (cos, sin)(2 pi u1), against mpmath
    Box-Muller on the same uniforms within the bound propagated from the
    parts.  Near u0 -> 1 (r ~ 1.5e-5) that allows ~1e-11: log_pos cancels
    there by design (an absolute, not relative, bound).  The law: w0 = 0 is
    the cut-off radius sqrt(66 ln 2) = 6.76 sigma, carrying tail mass
    exp(-r^2 / 2) = 2^-33; consecutive w1 turn the angle by 2 pi 2^-32."""
    rng = np.random.default_rng(23)
    ext = [0, 1, 2, 2 ** 30, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 3 * 2 ** 30,
           2 ** 32 - 2, 2 ** 32 - 1]
    w0 = np.concatenate([np.repeat(ext, len(ext)),
                         rng.integers(0, 2 ** 32, 3000)])
    w1 = np.concatenate([np.tile(ext, len(ext)),
                         rng.integers(0, 2 ** 32, 3000)])
    ww = np.stack([w0, w1], 1).astype(np.float64)
    got = eng.probe('normal2_words', ww)
    worst_ratio, at = 0.0, None
    for (a, b), (g0, g1) in zip(ww, got):
        u0 = (mpmath.mpf(int(a)) + 0.5) / 2 ** 32
        u1 = (mpmath.mpf(int(b)) + 0.5) / 2 ** 32
        r = mpmath.sqrt(-2 * mpmath.log(u0))
        c, s = mpmath.cospi(2 * u1), mpmath.sinpi(2 * u1)
        bound = _normal_bound(float(u0), float(r))
        err = max(float(abs(_mpf(g0) - r * c)), float(abs(_mpf(g1) - r * s)))
        if err / bound > worst_ratio:
            worst_ratio, at = err / bound, (int(a), int(b), err)
    _report('normal2_words err / bound', worst_ratio, at)
    assert worst_ratio <= 1.0, at
    # the cut-off radius and its tail mass
    g = eng.probe('normal2_words', [[0, 0]])[0]
    rmax = math.hypot(g[0], g[1])
    rref = mpmath.sqrt(66 * mpmath.log(2))
    assert abs(rmax - float(rref)) <= 1e-15 * float(rref)
    assert mpmath.almosteq(mpmath.exp(-rref ** 2 / 2), mpmath.mpf(2) ** -33,
                           1e-35)
    # the angle step: w1 -> w1 + 1 turns (g0, g1) by 2 pi 2^-32
    ww = np.array([[2 ** 31, k] for k in (0, 1, 2 ** 30, 2 ** 30 + 1)],
                  dtype=np.float64)
    g = eng.probe('normal2_words', ww)
    for j in (0, 2):
        d = math.atan2(g[j + 1][1], g[j + 1][0]) - math.atan2(g[j][1],
                                                              g[j][0])
        assert abs(d - 2 * math.pi * 2.0 ** -32) <= 1e-6 * 2 * math.pi * \
            2.0 ** -32, d


def test_normal_from_uniforms(eng, dps):
    """philox_normal2 after Philox (the Gaussian VMC proposal): 53-bit
    uniforms u0, u1 in [0, 1) -> r = sqrt(max(-2 log(1 - u0), 1e-300)),
    (g0, g1) = r (cos, sin)(2 pi u1), same bound.  u0 = 0 gives r = 1e-150."""
    rng = np.random.default_rng(24)
    ext = [0.0, 2.0 ** -53, 0.25, 0.5, 0.75, 1 - 2.0 ** -33, 1 - 2.0 ** -53]
    u0 = np.concatenate([np.repeat(ext, len(ext)),
                         np.floor(rng.uniform(0, 1, 3000) * 2 ** 53) /
                         2.0 ** 53])
    u1 = np.concatenate([np.tile(ext, len(ext)),
                         np.floor(rng.uniform(0, 1, 3000) * 2 ** 53) /
                         2.0 ** 53])
    uu = np.stack([u0, u1], 1)
    got = eng.probe('normal2_uniforms', uu)
    worst_ratio, at = 0.0, None
    for (a, b), (g0, g1) in zip(uu, got):
        v = 1 - _mpf(a)
        if a == 0.0:
            r = mpmath.sqrt(mpmath.mpf(1e-300))
            bound = 4 * float(np.spacing(1e-150))
        else:
            r = mpmath.sqrt(-2 * mpmath.log(v))
            bound = _normal_bound(float(v), float(r))
        c, s = mpmath.cospi(2 * _mpf(b)), mpmath.sinpi(2 * _mpf(b))
        err = max(float(abs(_mpf(g0) - r * c)), float(abs(_mpf(g1) - r * s)))
        if err / bound > worst_ratio:
            worst_ratio, at = err / bound, (a, b, err)
    _report('normal2_uniforms err / bound', worst_ratio, at)
    assert worst_ratio <= 1.0, at


def test_philox_known_answers(eng, oracle):
    """Philox2x32-10 / 4x32-10 on the device: the Random123 known-answer
    vectors (the ones tests/test_oracle_golden.py pins the oracle with), and
    agreement with the oracle's block function on random counters / keys."""
    kat2 = [((0, 0, 0), (0xff1dae59, 0x6cd10df2)),
            ((0xffffffff, 0xffffffff, 0xffffffff), (0x2c3f628b, 0xab4fd7ad)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e), (0xdd7ce038, 0xf62a4c12))]
    got = eng.probe('philox2x32', [k for k, _ in kat2])
    assert [tuple(int(v) for v in g) for g in got] == [w for _, w in kat2]
    kat4 = [((0, 0, 0, 0, 0, 0),
             (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 6,
             (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd))]
    got = eng.probe('philox4x32', [k for k, _ in kat4])
    assert [tuple(int(v) for v in g) for g in got] == [w for _, w in kat4]
    rng = np.random.default_rng(25)
    c = rng.integers(0, 2 ** 32, (500, 3))
    got = eng.probe('philox2x32', c.astype(np.float64))
    for (c0, c1, k), g in zip(c, got):
        assert oracle.philox2x32(int(c0), int(c1), int(k)) == \
            (int(g[0]), int(g[1]))


def test_probe_refuses_inputs_no_caller_produces(model_engines):
    """The probe never feeds a table an input its production callers cannot
    produce: non-finite inputs, log_pos of x <= 0 or subnormal, table
    positions outside (-4 L, 4 L) are errors."""
    from phd_qmclib_amd.engine import QmcError
    tag, e = model_engines[4]
    L = _mparams(e).supercell_size
    for fn, x in (('log_pos', [0.0]), ('log_pos', [-1.0]),
                  ('log_pos', [1e-310]), ('log_pos', [math.nan]),
                  ('exp_bounded', [math.inf]), ('trig_tab', [math.nan]),
                  ('trig_tab', [4 * L]), ('one_body_tab', [-4 * L]),
                  ('wrap_box', [math.inf])):
        with pytest.raises(QmcError):
            e.probe(fn, x)


# ------------------------------------ edges through the stepping kernels ----
def _regular(rng, W, n, L):
    base = (np.arange(n) + 0.5) * (L / n)
    return (base[None, :] + rng.uniform(-0.2, 0.2, (W, n)) * (L / n)) % L


@pytest.mark.parametrize('tag', ['box64', 'box128'])
def test_vmc_proposal_that_wraps_to_exactly_L(golden_params, oracle, tag):
    """A proposal landing in (-ulp(L)/2, 0) wraps to exactly L (z + L rounds
    up; the reference's floor-mod gives L too).  That position reaches the
    trig-table load (which falls back for the whole wavefront), the sorted
    row and the one-body table.  Tape: particle 0 at 2^-40 moves by
    -(2^-40 + 2^-54) and is accepted; move status, log psi and energy of
    that step and the next ones against the oracle on the same tape, and a
    seeded DMC block from the resulting configuration."""
    from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine, VmcEnsemble
    from .conftest import oracle_model
    rng = np.random.default_rng(26)
    spec = spec_from_golden(golden_params, tag)
    eng = ModelEngine(spec.cfc_spec)
    m = oracle_model(oracle, golden_params, tag)
    n = eng.num_particles
    L = float(spec.cfc_spec.model_params.supercell_size)
    W, K = 4, 6
    pos = _regular(rng, W, n, L)
    pos[:, 0] = 2.0 ** -40
    tape = np.empty((W, K, n + 1))
    tape[:, :, :n] = 0.5 + rng.uniform(-0.5, 0.5, (W, K, n)) * 0.1
    tape[:, :, n] = rng.uniform(0, 1, (W, K))
    tape[:, 0, :n] = 0.5
    tape[:, 0, 0] = 0.5 - (2.0 ** -40 + 2.0 ** -54)
    tape[:, 0, n] = 1e-300                 # accept
    assert 0.5 - tape[0, 0, 0] == 2.0 ** -40 + 2.0 ** -54
    v = VmcEnsemble(eng, W, 1.0, rng_seed=3)
    v.set_state(pos)
    v.set_tape(tape)
    out = v.run_block(1 + K, series=True, confs=True)
    assert np.all(out['move_stat'][1])
    assert np.any(out['pos'][1] == L), 'the proposal did not wrap to L'
    for w in range(W):
        ch = oracle.VmcChain(m, pos[w], 1.0, seed=3, chain=w)
        owf, oen, ost, _ = ch.run(1 + K, tape=tape[w])
        assert np.array_equal(ost, out['move_stat'][:, w]), w
        assert close(out['wf_abs_log'][:, w], owf), \
            (w, worst(out['wf_abs_log'][:, w], owf))
        assert close(out['energy'][:, w], oen), (w, worst(out['energy'][:, w],
                                                         oen))
    # DMC from a configuration with a particle at exactly L
    cur = out['pos'][1]
    assert np.any(cur == L)
    d = DmcEnsemble(eng, 1e-3, 16, W, 0.5, rng_seed=5)
    d.set_state(cur)
    ser = d.run_block(4)
    o = oracle.DmcEnsemble(m, cur, 1e-3, 16, W, 0.5, seed=5)
    for t in range(4):
        y = o.step()
        assert int(ser.num_walkers[t]) == y.num_walkers
        assert abs(ser.energy[t] - y.energy) <= RTOL * max(1.0, abs(y.energy))
    d.close()
    v.close()
    eng.close()


def test_nonideal_model_with_zero_beta_is_refused(golden_params):
    """param_beta = 0 on a non-ideal model (never produced by the reference's
    matching conditions): the sorted-row pair sums count the pair quotients
    in units of a_long = (pi / L) beta and would drop every short-range
    term without an error, so qmc_engine_create refuses the model."""
    import ctypes as C
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd.engine import model_params_struct
    lib = _lib.load()
    for tag in ('box16', 'box64', 'box128'):
        p = model_params_struct(spec_from_golden(golden_params, tag).cfc_spec)
        p.param_beta = 0.0
        h = C.c_void_p()
        assert lib.qmc_engine_create(C.byref(p), 0, None, C.byref(h)) != 0
        assert b'param_beta' in lib.qmc_last_error()
        assert not h.value


def test_out_of_box_configuration_at_non_integer_L(oracle):
    """The far branch of wrap_box at a non-integer box length, through
    qmc_evaluate: positions several box lengths out, including ones where
    the uncorrected floor-mod was negative, against the oracle."""
    import json
    from phd_qmclib_amd.engine import ModelEngine
    from .conftest import GOLDEN
    with open(os.path.join(GOLDEN, 'sweep.json')) as fp:
        rec = next(r for r in json.load(fp)
                   if float(r['params']['supercell_size']) % 1.0 != 0.0 and
                   r['params']['boson_number'] >= 32)
    from phd_qmclib_amd.mrbp_qmc import Spec
    spec = Spec(**rec['spec'])
    eng = ModelEngine(spec.cfc_spec)
    m = oracle.model_from_params(rec['params'], rec['obf_params'],
                                 rec['tbf_params'])
    n, L = eng.num_particles, float(rec['params']['supercell_size'])
    rng = np.random.default_rng(27)
    pos = _regular(rng, 8, n, L)
    shift = rng.integers(-3, 4, pos.shape) * L
    pos = pos + shift
    # multiples of L just below an integer quotient (the overshooting case)
    pos[:, 0] = [math.nextafter(k * L, -math.inf) for k in
                 (-3, -2, 2, 3, -3, -2, 2, 3)]
    out = eng.evaluate(pos)
    wf, en, ith, dr = oracle.evaluate_set(m, pos)
    assert close(out.wf_abs_log, wf), worst(out.wf_abs_log, wf)
    assert close(out.energy, en), worst(out.energy, en)
    assert close(out.drift, dr), worst(out.drift, dr)
    eng.close()
