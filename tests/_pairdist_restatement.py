"""NumPy restatement of the pair-distance histogram behind g2(r), written from
its definition (no reference text):

    z_i    position brought into [0, L)                 (z mod L)
    d_ij   = z_i - z_j, or, where |z_i - z_j| > L/2, its image
             -L/2 + ((z_i - z_j) + L/2) mod L           (floored modulo)
    r_ij   = |d_ij|                                     in [0, L/2]
    b_ij   = min(r_ij // delta, B - 1),  delta = (L/2) / B
    H[b]   = number of unordered pairs i < j with b_ij = b
    g2(r_b) = H[b] L / (N (N - 1) delta)  at  r_b = (b + 1/2) delta

The image is formed with the reference's operations in the reference's order
(qmc_base/utils.py:35-51), so that the distances reproduce the reference's
`real_distance` bit for bit; tests/test_pairdist_host.py holds them against the
reference's own values in tests/golden/pair_dist.npz.

Rounding can move a pair between neighbouring bins only where it sits on a bin
edge or on the image switch to within rounding.  `ambiguous_pairs` lists such
pairs with a margin wide enough for any fp64 evaluation order: r / delta within
1e-9 (absolute) of an integer, or |z_i - z_j| within 1e-9 L of L/2.
"""
import numpy as np

EDGE_EPS = 1e-9


def wrap(pos, sc_size):
    """Positions brought into [0, L)."""
    return np.mod(np.asarray(pos, dtype=np.float64), sc_size)


def min_distance(z_i, z_j, sc_size):
    sc_half = 0.5 * sc_size
    z_ij = z_i - z_j
    image = -sc_half + np.mod(z_ij + sc_half, sc_size)
    return np.where(np.abs(z_ij) > sc_half, image, z_ij)


def pair_index(n):
    """The unordered pairs (i < j) in row-major order."""
    return np.triu_indices(n, 1)


def pair_separations(pos, sc_size):
    """pos[nconf, N] -> r[nconf, N (N - 1) / 2] over `pair_index(N)`."""
    z = wrap(pos, sc_size)
    i, j = pair_index(z.shape[1])
    return np.abs(min_distance(z[:, i], z[:, j], sc_size))


def bin_index(r, sc_size, num_bins):
    delta = (0.5 * sc_size) / num_bins
    b = np.floor_divide(r, delta).astype(np.int64)
    return np.minimum(b, num_bins - 1)


def counts_from_separations(r, sc_size, num_bins):
    """r[nconf, npairs] -> H[nconf, num_bins] (int64)."""
    b = bin_index(np.asarray(r, dtype=np.float64), sc_size, num_bins)
    out = np.zeros((b.shape[0], num_bins), dtype=np.int64)
    for c in range(b.shape[0]):
        out[c] = np.bincount(b[c], minlength=num_bins)
    return out


def pair_counts(pos, sc_size, num_bins):
    """pos[nconf, N] -> H[nconf, num_bins] (int64)."""
    return counts_from_separations(pair_separations(pos, sc_size), sc_size,
                                   num_bins)


def bin_centres(sc_size, num_bins):
    delta = (0.5 * sc_size) / num_bins
    return (np.arange(num_bins) + 0.5) * delta


def normalise(counts, n, sc_size):
    """H[..., B] -> g2[..., B]."""
    counts = np.asarray(counts, dtype=np.float64)
    delta = (0.5 * sc_size) / counts.shape[-1]
    return counts * sc_size / (n * (n - 1) * delta)


def ambiguous_pairs(pos, sc_size, num_bins):
    """Per configuration, the edge-ambiguous pairs: a list (one entry per
    configuration) of arrays [k, 3] of rows (i, j, e), e the bin edge the pair
    sits on (the boundary between the bins e - 1 and e; e = 0 and e = B are the
    ends of the range).  A pair at the image switch, |z_i - z_j| = L/2 to
    within 1e-9 L, is listed with e = B."""
    z = wrap(pos, sc_size)
    i, j = pair_index(z.shape[1])
    delta = (0.5 * sc_size) / num_bins
    zij = z[:, i] - z[:, j]
    r = np.abs(min_distance(z[:, i], z[:, j], sc_size))
    q = r / delta
    e = np.rint(q)
    on_edge = np.abs(q - e) <= EDGE_EPS
    on_switch = np.abs(np.abs(zij) - 0.5 * sc_size) <= EDGE_EPS * sc_size
    out = []
    for c in range(z.shape[0]):
        rows = []
        for k in np.nonzero(on_edge[c] | on_switch[c])[0]:
            edge = num_bins if on_switch[c, k] else int(e[c, k])
            rows.append((int(i[k]), int(j[k]), edge))
        out.append(np.array(rows, dtype=np.int64).reshape(-1, 3))
    return out


def edge_slack(amb, num_bins):
    """How far bin b of a histogram may differ from the restatement, given the
    ambiguous pairs of ONE configuration: the number of pairs that touch edge b
    or b + 1 -> slack[num_bins]."""
    slack = np.zeros(num_bins, dtype=np.int64)
    for e in amb[:, 2]:
        for b in (e - 1, e):
            if 0 <= b < num_bins:
                slack[b] += 1
    return slack


# ---- inputs shared by the host and the GPU tests ---------------------------
UNIFORM_LAW = dict(seed=20261, nconf=4096, n=64, sc_size=64.0, num_bins=32)


def uniform_law_inputs():
    """4096 configurations of 64 iid uniform positions in [0, 64)."""
    u = UNIFORM_LAW
    rng = np.random.RandomState(u['seed'])
    return u['sc_size'] * rng.random_sample((u['nconf'], u['n']))


def uniform_law_z(pooled, nconf, n, num_bins):
    """z-score per bin of pooled counts against the law of iid uniform points
    on a ring: the pair separations are uniform on [0, L/2] and pairwise
    independent, so a bin's pooled count has mean n_c P / B and variance
    n_c P (1/B)(1 - 1/B), P = N (N - 1) / 2."""
    total = nconf * (n * (n - 1) // 2)
    mean = total / num_bins
    var = total * (1.0 / num_bins) * (1.0 - 1.0 / num_bins)
    return (np.asarray(pooled, dtype=np.float64) - mean) / np.sqrt(var)
