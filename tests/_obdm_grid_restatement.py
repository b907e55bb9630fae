"""NumPy restatement of the one-body density matrix on a grid
(csrc/qmc_obdm_grid.h), written from its definition:

    delta = L / M,  x_c = (c + 1/2) L / M                     (M cells of [0, L))
    z_i   the position of particle i brought into [0, L)
    a(i)  min(floor(z_i / delta), M - 1)
    ratio[i, c] = psi(z_1 .. z_i -> x_c .. z_N) / psi(R)
                = exp( [log f1(x_c) - log f1(z_i)]                 (not is_free)
                     + sum_{j != i} [log f2(|d(x_c, z_j)|)
                                     - log f2(|d(z_i, z_j)|)] )    (not is_ideal)
    R_conf[a, c]  = sum_{i : a(i) = a} ratio[i, c]
    sums[g, a, c] = sum_{conf = g (mod G)} w_conf R_conf[a, c]
    wsum[g]       = sum_{conf = g (mod G)} w_conf

with `_log_f1`, `_log_f2` and `_min_image` of tests/_obdm_restatement.py.
tests/test_obdm_grid_host.py anchors it on that file's `ith_one_body_density`
at the shifts x_c - z_i.

The yardstick of a comparison is, per cell,

    bound = RTOL sum_terms |w| ratio max(1, scale),

`scale` being the sum of the magnitudes of the logarithms in the exponent of
the term (as tests/_partent_restatement.py) and RTOL = 2e-11 the suite's.
"""
import numpy as np

from ._obdm_restatement import _log_f1, _log_f2, _min_image
from ._renyi_restatement import GOLDEN_SIZES, RTOL, model_spec_args

__all__ = ['GOLDEN_SIZES', 'RTOL', 'model_spec_args']

PARITY_SIZES = (1, 2, 3, 8, 37, 64, 100, 128)
PARITY_POINTS = (1, 7, 64, 65, 130)
PARITY_CONFS = 12
PARITY_GROUPS = (1, 5)
ORDER_SIZES = (16, 37, 128)
CHUNK_ELEMS = 1 << 22       # elements of the largest temporary


def points(sc_size, num_points):
    """-> (delta, x[M])."""
    delta = float(sc_size) / int(num_points)
    return delta, ((np.arange(int(num_points)) + 0.5) * float(sc_size)
                   / int(num_points))


def wrap(pos, sc_size):
    return np.mod(np.asarray(pos, dtype=np.float64), float(sc_size))


def row_bins(pos, sc_size, num_points):
    """a[..., N] of pos[..., N]."""
    delta, _ = points(sc_size, num_points)
    a = np.floor(wrap(pos, sc_size) / delta).astype(np.int64)
    return np.minimum(a, int(num_points) - 1)


def ratios(pos, num_points, p):
    """pos[nconf, N] -> (ratio[nconf, N, M], scale[nconf, N, M])."""
    pos = np.asarray(pos, dtype=np.float64)
    mp = p['params']
    sc = float(mp['supercell_size'])
    nconf, n = pos.shape
    m = int(num_points)
    _, x = points(sc, m)
    z = wrap(pos, sc)
    expo = np.zeros((nconf, n, m))
    scale = np.zeros((nconf, n, m))
    if not mp['is_free']:
        fx, fz = _log_f1(x, p), _log_f1(z, p)
        expo += fx[None, None, :] - fz[:, :, None]
        scale += np.abs(fx)[None, None, :] + np.abs(fz)[:, :, None]
    if not mp['is_ideal']:
        off = ~np.eye(n, dtype=bool)
        step = max(1, CHUNK_ELEMS // max(1, n * m * n))
        for c0 in range(0, nconf, step):
            zc = z[c0:c0 + step]
            # the moved particle at x_c against every z_j: [conf, c, j]
            num = _log_f2(np.abs(_min_image(x[None, :, None] - zc[:, None, :],
                                            sc)), p)
            own = np.where(off, _log_f2(np.abs(_min_image(
                zc[:, :, None] - zc[:, None, :], sc)), p), 0.0)   # [conf, i, j]
            sel = off[None, :, None, :]                            # j != i
            expo[c0:c0 + step] += (
                np.where(sel, num[:, None, :, :], 0.0).sum(axis=3)
                - own.sum(axis=2)[:, :, None])
            scale[c0:c0 + step] += (
                np.where(sel, np.abs(num)[:, None, :, :], 0.0).sum(axis=3)
                + np.abs(own).sum(axis=2)[:, :, None])
    return np.exp(np.clip(expo, -700.0, 700.0)), scale


def conf_matrices(pos, num_points, p):
    """pos[nconf, N] -> (R[nconf, M, M], bound[nconf, M, M] at unit weight)."""
    pos = np.asarray(pos, dtype=np.float64)
    m = int(num_points)
    sc = float(p['params']['supercell_size'])
    ratio, scale = ratios(pos, m, p)
    a = row_bins(pos, sc, m)
    nconf = len(pos)
    out = np.zeros((nconf, m, m))
    bound = np.zeros((nconf, m, m))
    conf = np.repeat(np.arange(nconf), pos.shape[1])
    np.add.at(out, (conf, a.reshape(-1)), ratio.reshape(-1, m))
    np.add.at(bound, (conf, a.reshape(-1)),
              (RTOL * ratio * np.maximum(1.0, scale)).reshape(-1, m))
    return out, bound


def group_sums(mats, bound, num_groups, weights=None):
    """Per-configuration matrices and bounds -> (sums[G, M, M], wsum[G],
    bound[G, M, M]): configuration c in group c mod G."""
    g = int(num_groups)
    nconf = len(mats)
    w = np.ones(nconf) if weights is None else np.asarray(weights, np.float64)
    sums = np.zeros((g,) + mats.shape[1:])
    bnd = np.zeros_like(sums)
    wsum = np.zeros(g)
    for c in range(nconf):
        sums[c % g] += w[c] * mats[c]
        bnd[c % g] += abs(w[c]) * bound[c]
        wsum[c % g] += w[c]
    return sums, wsum, bnd


def reference(pos, num_points, num_groups, p, weights=None):
    """-> (sums, wsum, bound) of the batch."""
    mats, bound = conf_matrices(pos, num_points, p)
    return group_sums(mats, bound, num_groups, weights)


def within(dev, ref, bound):
    """|dev - ref| <= bound in every cell -> (ok, worst error / bound); a cell
    of bound 0 (no term) must be equal."""
    err = np.abs(np.asarray(dev) - ref)
    ok = np.all(err <= bound)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0))
    return bool(ok), float(ratio.max()) if ratio.size else 0.0


def pool(n, nconf=PARITY_CONFS, seed=None):
    """pos[nconf, N] of random rows in the box L = n, some particles whole
    periods outside [0, L)."""
    L = float(n)
    rng = np.random.RandomState(7300 + n if seed is None else seed)
    rows = L * rng.random_sample((nconf, n))
    rows[0, ::3] += 2.0 * L
    rows[1] -= 3.0 * L
    rows[2 % nconf, ::2] -= 1.0 * L
    rows[-1] += 5.0 * L
    return rows


def reorderings(pos, sc_size, seed):
    """-> (rows sorted by their image in the box, rows shuffled one by one)."""
    rng = np.random.RandomState(seed)
    ps = np.argsort(wrap(pos, sc_size), axis=1, kind='stable')
    pr = np.stack([rng.permutation(pos.shape[1]) for _ in pos])
    take = np.take_along_axis
    return take(pos, ps, axis=1), take(pos, pr, axis=1)


# ---- the known answer: N = 2 without a lattice ------------------------------
def known_grid(tbf, sc_size):
    """The discrete ensemble of `_partent_restatement.known_answer`: the
    24 x 24 grid configurations conf[576, 2] and their probabilities w ~ psi^2
    (that function draws its 16384 configurations from exactly this law)."""
    from . import _partent_restatement as pe
    G = pe.KNOWN['grid']
    x = (np.arange(G) + 0.5) * sc_size / G
    conf = np.stack(np.meshgrid(x, x, indexing='ij'), axis=-1).reshape(-1, 2)
    lw = 2.0 * pe.log_f2(np.abs(pe.min_distance(conf[:, 0], conf[:, 1],
                                                sc_size)), tbf, sc_size)
    w = np.exp(lw - lw.max())
    return conf, w / w.sum()


def known_moments(conf, w, num_points, p):
    """Exact E R[M, M] and E R^2[M, M] (cell by cell) over the grid law."""
    mats, _ = conf_matrices(conf, num_points, p)
    return (np.einsum('c,cab->ab', w, mats),
            np.einsum('c,cab->ab', w, mats ** 2))


def known_z(mean, er, er2, nconf):
    """(mean - E R) / sigma per cell, sigma = sqrt((E R^2 - (E R)^2) / nconf);
    cells without variance count as 0 where mean equals E R within RTOL."""
    var = np.maximum(er2 - er * er, 0.0)
    sigma = np.sqrt(var / nconf)
    z = np.zeros_like(er)
    ok = sigma > 1e-13 * np.maximum(1.0, np.abs(er))
    z[ok] = (mean[ok] - er[ok]) / sigma[ok]
    flat = ~ok & (np.abs(mean - er) > RTOL * np.maximum(1.0, np.abs(er)))
    z[flat] = np.inf
    return z
