"""Host side of the energy components (no GPU): the NumPy restatement of the
per-configuration row (tests/_energy_parts_restatement.py) against the
reference's golden values, the lattice potential on hand-placed particles, the
inputs of the GPU parity test, and the post-processing of phd_qmclib_amd.engine
(`energy_components`, `contact_extrapolate`, the argument checks) on synthetic
sums with known answers."""
from math import pi

import numpy as np
import pytest

from . import _energy_parts_restatement as rs
from ._models import box, model_dict

RTOL = 2e-11          # the tolerance of tests/golden/kernels.npz's own tests


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.maximum(1.0, np.abs(b)))


# ---- 1. the restatement against the reference ------------------------------
def golden_tags(golden_kernels):
    return sorted({name.split('/')[0] for name in golden_kernels.files})


def test_restatement_matches_golden(golden_params, golden_kernels):
    tags = golden_tags(golden_kernels)
    assert len(tags) == 15 and set(tags) <= set(golden_params)
    for tag in tags:
        p = golden_params[tag]
        pos = golden_kernels[tag + '/pos']
        F, e = rs.drift_energy(pos, p)
        assert close(F, golden_kernels[tag + '/ith_drift']), tag
        assert close(e, golden_kernels[tag + '/ith_energy']), tag
        assert close(e.sum(axis=1), golden_kernels[tag + '/energy']), tag
        rows = rs.energy_parts(pos, (), p)
        assert rows.shape == (pos.shape[0], 4)
        assert close(rows[:, 0], golden_kernels[tag + '/energy']), tag


# ---- 2. the lattice potential, by hand -------------------------------------
def test_potential_hand_placed(golden_params):
    p = golden_params['defect24']
    mp = p['params']
    v0, v0d = mp['lattice_depth'], mp['defect_magnitude']
    za = mp['well_width']
    assert mp['defects_sep'] == 6 and v0d < v0 and za == 1.0 / 1.5
    z = np.array([1.25,              # well
                  1.9,               # barrier of an ordinary cell
                  1.0 + za,          # exactly at z_a: z_a < zc is false
                  np.nextafter(1.0 + za, 2.0),      # the next double: barrier
                  6.9, 0.8, 12.75,   # defect cells 6, 0, 12
                  6.3,               # well of a defect cell
                  -0.1,              # cell -1, zc = 0.9: ordinary barrier
                  -5.2,              # cell -6 (a defect), zc = 0.8
                  -5.9,              # cell -6, zc = 0.1: well
                  24.0 + 0.8])       # beyond the box: cell 24, a defect
    want = np.array([0.0, v0, 0.0, v0, v0d, v0d, v0d, 0.0, v0, v0d, 0.0, v0d])
    assert np.array_equal(rs.potential(z, p), want)
    # every barrier alike without defects; nothing on a free model
    q = golden_params['box16']
    assert np.array_equal(rs.potential(np.array([0.2, 0.7, -0.4, 15.5]), q),
                          q['params']['lattice_depth'] *
                          np.array([0.0, 1.0, 1.0, 0.0]))
    assert not rs.potential(np.array([0.2, 0.7]), golden_params['free16']).any()


def test_window_sums_by_hand():
    # two particles d = 0.03 apart across the seam of an ideal box: weight 1
    p = model_dict(box(4, gint=0).cfc_spec)
    pos = np.array([[3.99, 0.02, 1.5, 2.5]])
    C = rs.window_sums(pos, (0.02, 0.05, 1.5), p)
    # (within 1.5: 0.03, 1.48, 1.0 and 1.49; 1.51 and 1.52 are not)
    assert np.allclose(C[0], [0.0, 1.0 / 0.1, 4.0 / 3.0], rtol=1e-12)
    # the cusp weight on a model with interactions
    spec = box(4)
    p = model_dict(spec.cfc_spec)
    tb = p['tbf_params']
    k2, r_off = tb['param_k2'], tb['param_r_off']
    pos = np.array([[1.0, 1.25, 3.0, 7.0]])         # 7.0 is 3.0 in the box
    w = lambda d: (np.cos(k2 * r_off) / np.cos(k2 * (d - r_off))) ** 2
    C = rs.window_sums(pos, (0.1, 0.5), p)
    assert np.allclose(C[0], [w(0.0) / 0.2, (w(0.0) + w(0.25)) / 1.0],
                       rtol=1e-12)
    assert w(0.0) == 1.0 and w(0.25) < 1.0


# ---- 3. the inputs of the GPU parity test ----------------------------------
def parity_cases(golden_params):
    for n in rs.PARITY_SIZES:
        yield n, float(n), 0.25 * n, None
    for tag in rs.EXTRA_MODELS:
        mp = golden_params[tag]['params']
        yield (mp['boson_number'], mp['supercell_size'],
               mp['tbf_contact_cutoff'], tag)


def test_parity_pools_are_edge_free(golden_params):
    for n, L, rm, tag in parity_cases(golden_params):
        pool = rs.parity_pool(n, L, rm)
        assert pool.shape == ((6 if n < 260 else 3), n)
        assert np.any(pool < 0) and np.any(pool >= L)
        for ranges in rs.parity_windows(rm):
            assert len(ranges) in (0, 3, 16)
            assert all(0 < r <= min(0.5 * L, abs(rm)) for r in ranges)
            assert rs.edge_free(pool, ranges, L), (n, tag)
        if n >= 6:
            # the planted pairs make the smallest window count
            p = (golden_params[tag] if tag else
                 model_dict(box(n).cfc_spec))
            assert np.all(rs.window_sums(pool, rs.parity_windows(rm)[0], p)
                          [:, 0] > 0)
    assert not rs.edge_free(np.array([[0.0, 0.25, 1.0]]), (0.25,), 3.0)
    assert rs.edge_free(np.array([[0.0, 0.25, 1.0]]), (0.2501,), 3.0)


# ---- 4. post-processing on synthetic sums ----------------------------------
def test_energy_components_known_answers():
    from phd_qmclib_amd.engine import (EnergyComponents, contact_coupling,
                                       energy_components)
    cfc = box(8, gint=20, depth=2 * pi ** 2).cfc_spec
    rng = np.random.RandomState(3)
    rows = rng.normal(size=(1000, 6)) * [3, 2, 1, 4, 0.5, 0.25] + \
        [40, 30, 5, 5, 0.3, 0.29]
    sums = np.stack([rows.sum(axis=0), (rows ** 2).sum(axis=0)], axis=1)
    ec = energy_components(sums, 1000, cfc, (0.02, 0.05))
    assert isinstance(ec, EnergyComponents)
    mean = rows.mean(axis=0)
    err = rows.std(axis=0, ddof=1) / np.sqrt(1000)
    got = [ec.total, ec.kinetic, ec.lattice, ec.interaction, *ec.contact]
    got_err = [ec.total_err, ec.kinetic_err, ec.lattice_err,
               ec.interaction_err, *ec.contact_err]
    assert np.allclose(got, mean, rtol=1e-13)
    assert np.allclose(got_err, err, rtol=1e-9)
    assert np.array_equal(ec.contact_ranges, [0.02, 0.05])
    # g = 4 kappa from the two-body parameters: interaction_strength at L = N
    tb = cfc.tbf_params
    assert ec.coupling == contact_coupling(cfc)
    assert ec.coupling == 4 * tb.param_k2 * np.tan(tb.param_k2 *
                                                   tb.param_r_off)
    assert abs(ec.coupling - 20.0) <= 1e-12 * 20.0
    assert abs(contact_coupling(box(8).cfc_spec) - 2.0) <= 2e-12
    assert contact_coupling(box(8, gint=0).cfc_spec) == 0.0
    # weights: the means of the weighted sums, the errors with n = num_confs
    w = rng.random_sample(1000) + 0.5
    sums = np.stack([(w[:, None] * rows).sum(axis=0),
                     (w[:, None] * rows ** 2).sum(axis=0)], axis=1)
    ec = energy_components(sums, w.sum(), cfc, (0.02, 0.05), num_confs=1000)
    wm = (w[:, None] * rows).sum(axis=0) / w.sum()
    wv = (w[:, None] * (rows - wm) ** 2).sum(axis=0) / w.sum()
    assert np.allclose([ec.total, ec.kinetic, ec.lattice, ec.interaction],
                       wm[:4], rtol=1e-13)
    assert np.allclose(ec.contact_err, np.sqrt(wv[4:] / 999), rtol=1e-9)
    # K = 0
    ec = energy_components(sums[:4], w.sum(), cfc)
    assert ec.contact.shape == (0,) and ec.contact_ranges.shape == (0,)


def test_contact_extrapolate_known_answers():
    from phd_qmclib_amd.engine import contact_extrapolate
    r = np.array([0.02, 0.05, 0.1, 0.2])
    # an exact parabola in r: the intercept, whatever the errors
    c0, err = contact_extrapolate(r, 0.31 - 1.7 * r ** 2, [0.01, 0.02, 0.01, 0.03])
    assert abs(c0 - 0.31) < 1e-13 and err > 0
    # two windows: the line through both points, errors propagated
    c0, err = contact_extrapolate([0.1, 0.2], [1.0, 0.7], [0.03, 0.04])
    assert abs(c0 - 1.1) < 1e-13
    assert abs(err - np.sqrt((4 * 0.03) ** 2 + 0.04 ** 2) / 3) < 1e-13
    # equal errors: ordinary least squares on (r^2, y)
    y = np.array([0.30, 0.31, 0.27, 0.25])
    c0, err = contact_extrapolate(r, y, np.full(4, 0.01))
    slope, icpt = np.polyfit(r ** 2, y, 1)
    assert abs(c0 - icpt) < 1e-12
    x2 = r ** 2
    assert abs(err - 0.01 * np.sqrt(np.sum(x2 ** 2) /
                                    (4 * np.sum(x2 ** 2) - x2.sum() ** 2))) < 1e-12
    for bad in (([0.1], [1.0], [0.1]), ([0.1, 0.1], [1.0, 1.1], [0.1, 0.1]),
                ([0.1, 0.2], [1.0, 1.1], [0.1, 0.0]),
                ([0.1, 0.2], [1.0], [0.1, 0.1])):
        with pytest.raises(ValueError):
            contact_extrapolate(*bad)


# ---- 5. Spec-level argument errors -----------------------------------------
def test_argument_errors():
    from phd_qmclib_amd.engine import (contact_ranges_array,
                                       energy_components)
    cfc = box(8).cfc_spec                      # L = 8, |rm| = 2
    ideal = box(8, gint=0).cfc_spec
    assert contact_ranges_array(cfc, None).shape == (0,)
    assert contact_ranges_array(cfc, ()).shape == (0,)
    assert np.array_equal(contact_ranges_array(cfc, (0.5, 2.0)), [0.5, 2.0])
    assert np.array_equal(contact_ranges_array(ideal, (3.0, 4.0)), [3.0, 4.0])
    assert contact_ranges_array(cfc, np.full(16, 0.1)).shape == (16,)
    for bad in (np.full(17, 0.1), (0.0,), (-0.1,), (np.nan,), (np.inf,),
                (4.5,), (2.5,), ((0.1, 0.2),)):
        with pytest.raises(ValueError):
            contact_ranges_array(cfc, bad)
    with pytest.raises(ValueError):
        contact_ranges_array(ideal, (4.5,))
    sums = np.ones((5, 2))
    with pytest.raises(ValueError):
        energy_components(sums, 10.0, cfc, (0.1, 0.2))     # 6 rows expected
    with pytest.raises(ValueError):
        energy_components(sums, 0.0, cfc, (0.1,))
    with pytest.raises(ValueError):
        energy_components(sums, 10.0, cfc, (2.5,))
