"""NumPy restatement of the energy-parts row (csrc/qmc_energy_parts.h), written
from the formulas (nothing is imported from the package):

    f1(z)   Kronig-Penney one-body factor of zc = z mod 1: barrier where
            z_a < zc, z_a = 1 / (1 + ratio), z_b = ratio / (1 + ratio)
              f1'/f1  =  kp1 tanh(kp1 (zc - 1 + z_b / 2))       barrier
                      = -k1 tan(k1 (zc - z_a / 2))              well
              f1''/f1 =  V0 - e0  |  -e0
    f2(r)   two-body factor of the minimum-image distance r:
              f2'/f2  = -k2 tan(k2 (r - r_off))                 r < |rm|
                      = (pi/L) beta / tan(pi r / L)             else
              f2''/f2 = -k2^2  |  (pi/L)^2 beta ((beta - 1) / tan^2 - 1)
    V(z)    barrier height where z_a < zc: defect_magnitude in the cells with
            floor(z) % defects_sep == 0, lattice_depth elsewhere; 0 in a well
    F_i     = f1'/f1 (z_i) + sum_{j != i} sign(d_ij) f2'/f2 (|d_ij|)
    e_i     = -f1''/f1 + (f1'/f1)^2 + sum_{j != i} [-f2''/f2 + (f2'/f2)^2]
              - F_i^2 + V(z_i)

    row     E = sum_i e_i,  T = sum_i F_i^2,  V = sum_i V(z_i),
            I = (E - T) - V,
            C_k = 1 / (2 r_k) sum_{i<j, |d_ij| < r_k}
                  [cos(k2 r_off) / cos(k2 (|d_ij| - r_off))]^2

The one-body terms and V take the position as given; the pairs take the images
inside the box (z mod L).  A model is the dict of tests/_models.model_dict (or
an entry of tests/golden/params.json): 'params', 'obf_params', 'tbf_params'.
tests/test_energy_parts_host.py anchors E and F on the reference's golden
values.

Rounding can move a pair across a window edge only where its distance sits on
the edge to within rounding: `edge_free` is true when no pair distance lies
within EDGE_EPS = 1e-9 of a window.
"""
import numpy as np

EDGE_EPS = 1e-9
COLS = 4


def _regions(z, ob):
    r = ob['lattice_ratio']
    za, zb = 1.0 / (1.0 + r), r / (1.0 + r)
    zc = np.mod(z, 1.0)
    return zc, za, zb, za < zc


def one_body_log_dz(z, p):
    ob = p['obf_params']
    k1, kp1 = ob['param_k1'], ob['param_kp1']
    zc, za, zb, barrier = _regions(z, ob)
    return np.where(barrier, kp1 * np.tanh(kp1 * (zc - 1.0 + 0.5 * zb)),
                    -k1 * np.tan(k1 * (zc - 0.5 * za)))


def one_body_log_dz2(z, p):
    ob = p['obf_params']
    v0, e0 = ob['lattice_depth'], ob['param_e0']
    return np.where(_regions(z, ob)[3], v0 - e0, -e0)


def potential(z, p):
    """V(z) of every position in z, as given (no wrapping)."""
    mp = p['params']
    z = np.asarray(z, dtype=np.float64)
    if mp['is_free']:
        return np.zeros_like(z)
    barrier = _regions(z, p['obf_params'])[3]
    defect = np.mod(np.floor(z), mp['defects_sep']) == 0
    height = np.where(defect, mp['defect_magnitude'], mp['lattice_depth'])
    return np.where(barrier, height, 0.0)


def two_body_log_dz(r, p):
    tb = p['tbf_params']
    L, rm = tb['supercell_size'], abs(tb['tbf_contact_cutoff'])
    k2, beta, r_off = tb['param_k2'], tb['param_beta'], tb['param_r_off']
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(r < rm, -k2 * np.tan(k2 * (r - r_off)),
                        (np.pi / L) * beta / np.tan(np.pi * r / L))


def two_body_log_dz2(r, p):
    tb = p['tbf_params']
    L, rm = tb['supercell_size'], abs(tb['tbf_contact_cutoff'])
    k2, beta = tb['param_k2'], tb['param_beta']
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.tan(np.pi * r / L)
        return np.where(r < rm, -k2 * k2,
                        (np.pi / L) ** 2 * beta * ((beta - 1.0) / t ** 2 - 1.0))


def min_image(d, L):
    half = 0.5 * L
    return np.where(np.abs(d) > half, -half + np.mod(d + half, L), d)


def separations(pos, L):
    """pos[W, N] -> signed minimum-image d[W, N, N], d[w, i, j] = z_i - z_j of
    the images inside the box."""
    z = np.mod(np.asarray(pos, dtype=np.float64), L)
    return min_image(z[:, :, None] - z[:, None, :], L)


def drift_energy(pos, p):
    """pos[W, N] -> (F[W, N], e[W, N]): the drift and the per-particle local
    energy."""
    pos = np.asarray(pos, dtype=np.float64)
    mp = p['params']
    W, n = pos.shape
    F, kin = np.zeros((W, n)), np.zeros((W, n))
    if not mp['is_free']:
        ldz = one_body_log_dz(pos, p)
        F += ldz
        kin += -one_body_log_dz2(pos, p) + ldz ** 2
    if not mp['is_ideal'] and n > 1:
        d = separations(pos, mp['supercell_size'])
        off = ~np.eye(n, dtype=bool)
        r = np.abs(d)
        r[:, ~off] = 0.25 * mp['supercell_size']     # (unused: the diagonal)
        q = two_body_log_dz(r, p)
        q2 = two_body_log_dz2(r, p)
        F += np.where(off, np.sign(d) * q, 0.0).sum(axis=2)
        kin += np.where(off, -q2 + q ** 2, 0.0).sum(axis=2)
    if mp['is_free'] and mp['is_ideal']:
        return F, np.zeros((W, n))
    return F, kin - F ** 2 + potential(pos, p)


def window_sums(pos, ranges, p):
    """pos[W, N], ranges[K] -> C[W, K], by brute force over all pairs."""
    pos = np.asarray(pos, dtype=np.float64)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1)
    mp, tb = p['params'], p['tbf_params']
    W, n = pos.shape
    out = np.zeros((W, ranges.size))
    if n < 2 or ranges.size == 0:
        return out
    i, j = np.triu_indices(n, 1)
    d = np.abs(separations(pos, mp['supercell_size'])[:, i, j])
    if mp['is_ideal']:
        wgt = np.ones_like(d)
    else:
        k2, r_off = tb['param_k2'], tb['param_r_off']
        wgt = (np.cos(k2 * r_off) / np.cos(k2 * (d - r_off))) ** 2
    for k, rk in enumerate(ranges):
        out[:, k] = np.where(d < rk, wgt, 0.0).sum(axis=1) / (2.0 * rk)
    return out


def energy_parts(pos, ranges, p):
    """pos[W, N], ranges[K] -> rows[W, 4 + K]."""
    F, e = drift_energy(pos, p)
    E, T = e.sum(axis=1), (F ** 2).sum(axis=1)
    V = potential(pos, p).sum(axis=1)
    head = np.stack([E, T, V, (E - T) - V], axis=1)
    return np.concatenate([head, window_sums(pos, ranges, p)], axis=1)


def edge_free(pos, ranges, L):
    """No pair distance of pos[W, N] within EDGE_EPS of a window edge."""
    pos = np.asarray(pos, dtype=np.float64)
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1)
    n = pos.shape[1]
    if n < 2 or ranges.size == 0:
        return True
    i, j = np.triu_indices(n, 1)
    d = np.abs(separations(pos, L)[:, i, j])
    return bool(np.all(np.abs(d[..., None] - ranges) > EDGE_EPS))


# ---- inputs shared by the host and the GPU tests ---------------------------
#: every lane-group shape, padded and full
PARITY_SIZES = (1, 2, 8, 16, 24, 32, 37, 64, 100, 128, 130, 260, 512)
GOLDEN_SIZES = {8: 'box8', 16: 'box16', 37: 'box37', 64: 'box64',
                100: 'box100', 128: 'box128', 512: 'box512'}
#: golden models beside the box family: one with defects, one ideal
EXTRA_MODELS = ('defect24', 'ideal16')


def model_spec_args(n):
    """Keyword arguments of a model Spec of n particles in a box of L = n
    (the 'box' family of tests/golden/params.json)."""
    return dict(boson_number=n, interaction_strength=2,
                lattice_depth=5 * np.pi ** 2, lattice_ratio=1,
                supercell_size=n, tbf_contact_cutoff=0.25 * n)


def window_unit(rm):
    return min(1.0, abs(float(rm)))


def parity_windows(rm):
    """The window sets of the parity test: three windows, none, sixteen."""
    u = window_unit(rm)
    return ((0.05 * u, 0.25 * u, 1.0 * u), (),
            tuple(u * np.linspace(0.04, 1.0, 16)))


def parity_pool(n, L=None, rm=None, seed=None):
    """Random rows in the box of length L (default n), some of them below 0
    and at or above L: 6 configurations, 3 from N = 260 on.  Every row holds a
    few planted close pairs (one across the seam of the box) so that the
    small windows are not empty."""
    L = float(n) if L is None else float(L)
    u = window_unit(0.25 * L if rm is None else rm)
    rng = np.random.RandomState(9100 + n if seed is None else seed)
    nconf = 6 if n < 260 else 3
    pool = L * rng.random_sample((nconf, n))
    if n >= 2:
        pool[:, 1] = np.mod(pool[:, 0] + 0.031 * u, L)
    if n >= 4:
        pool[:, 3] = np.mod(pool[:, 2] - 0.19 * u, L)
    if n >= 6:
        pool[:, n - 1] = L - 0.011 * u
        pool[:, n - 2] = 0.017 * u
    pool[0, ::3] += 2.0 * L
    pool[1] -= 0.75 * L
    pool[2] += 1.5 * L
    if nconf > 3:
        pool[3, ::2] -= 7.0 * L
    return pool
