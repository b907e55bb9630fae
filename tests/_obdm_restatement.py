"""NumPy restatement of the one-body density matrix, written from its
definition (no reference text):

    ith(i, s) = exp( [log f1(z_i + s) - log f1(z_i)]              (not is_free)
                   + sum_{j != i} [log f2(|d(z_i + s, z_j)|)
                                   - log f2(|d(z_i, z_j)|)] )      (not is_ideal)
    g1(s)     = (1/N) sum_i ith(i, s)

f1 is the Kronig-Penney one-body factor of the position modulo the lattice
period 1, f2 the two-body factor of the minimum-image distance in the
supercell of length L; z_i + s is not wrapped.  tests/test_obdm_host.py anchors
it on the reference's golden values; the GPU tests use it for batch shapes the
pure-Python reference is too slow for.
"""
import numpy as np


def _log_f1(z, p):
    ob, mp = p['obf_params'], p['params']
    v0, r = ob['lattice_depth'], ob['lattice_ratio']
    e0, k1, kp1 = ob['param_e0'], ob['param_k1'], ob['param_kp1']
    zc = np.mod(z, 1.0)
    za, zb = 1.0 / (1.0 + r), r / (1.0 + r)
    cf = np.sqrt(1.0 + v0 / e0 * np.sinh(0.5 * np.sqrt(v0 - e0) * zb) ** 2)
    barrier = np.cosh(kp1 * (zc - 1.0 + 0.5 * zb))
    well = cf * np.cos(k1 * (zc - 0.5 * za))
    return np.log(np.where(za < zc, barrier, well))


def _min_image(d, sc):
    half = 0.5 * sc
    return np.where(np.abs(d) > half, -half + np.mod(d + half, sc), d)


def _log_f2(rz, p):
    tb = p['tbf_params']
    sc, rm = tb['supercell_size'], abs(tb['tbf_contact_cutoff'])
    k2, beta = tb['param_k2'], tb['param_beta']
    r_off, am = tb['param_r_off'], tb['param_am']
    short = am * np.cos(k2 * (rz - r_off))
    with np.errstate(divide='ignore', invalid='ignore'):
        long_ = np.sin(np.pi * rz / sc) ** beta
        return np.log(np.where(rz < rm, short, long_))


def ith_one_body_density(pos, shifts, p):
    """pos[nconf, N], shifts[nshift] -> ith[nconf, nshift, N]."""
    pos = np.asarray(pos, dtype=np.float64)
    shifts = np.asarray(shifts, dtype=np.float64)
    mp = p['params']
    nconf, n = pos.shape
    sc = mp['supercell_size']
    out = np.zeros((nconf, len(shifts), n))
    if mp['is_free'] and mp['is_ideal']:
        return out + 1.0
    off = ~np.eye(n, dtype=bool)
    for c in range(nconf):
        z = pos[c]
        den = np.zeros(n)
        if not mp['is_free']:
            den += _log_f1(z, p)
        if not mp['is_ideal']:
            d0 = np.abs(_min_image(z[:, None] - z[None, :], sc))
            den += np.where(off, _log_f2(d0, p), 0.0).sum(axis=1)
        for k, s in enumerate(shifts):
            zs = z + s
            num = np.zeros(n)
            if not mp['is_free']:
                num += _log_f1(zs, p)
            if not mp['is_ideal']:
                d = np.abs(_min_image(zs[:, None] - z[None, :], sc))
                num += np.where(off, _log_f2(d, p), 0.0).sum(axis=1)
            out[c, k] = np.exp(num - den)
    return out


def one_body_density(pos, shifts, p):
    """pos[nconf, N], shifts[nshift] -> g1[nconf, nshift]."""
    return ith_one_body_density(pos, shifts, p).mean(axis=2)
