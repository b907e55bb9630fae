"""NumPy restatement of the triple-span histogram behind g3(d), written from
its definition:

    z_i     position brought into [0, L)                  (z mod L)
    triple  {i, j, k}, i < j < k; a <= b <= c its three wrapped positions
    gaps    b - a,  c - b,  L - (c - a)
    span    d_ijk = L - (largest gap)      the shortest arc that holds all three
    delta   = D / B,  0 < D <= L/2
    bin     d_ijk <  D :  min(d_ijk // delta, B - 1)
            d_ijk >= D :  B                                (overflow bin)
    T[b]    = number of triples in bin b,  b = 0 ... B
    g3(d_b) = T[b] / (C(N,3) 3 (delta/L)^2 (2 b + 1))  at  d_b = (b + 1/2) delta

`triple_counts` is the brute force over all C(N,3) triples.  `rank_counts` is
the equivalent O(N^2) form the kernel uses (order by (position, index), walk
the forward arcs, multiplicity m - 1); tests/test_tripledist_host.py holds the
two against each other.

Rounding can move a triple between neighbouring bins only where its span sits
on a bin edge or on D to within rounding.  `ambiguous_triples` lists such
triples with the margin of tests/_pairdist_restatement.py (EDGE_EPS): d / delta
within 1e-9 (absolute) of an integer, or d within 1e-9 L of D.
"""
from math import comb

import numpy as np

from ._pairdist_restatement import EDGE_EPS, wrap

GOLDEN_SIZES = {8: 'box8', 16: 'box16', 37: 'box37', 64: 'box64',
                100: 'box100', 128: 'box128', 512: 'box512'}


def triple_index(n):
    """The unordered triples (i < j < k) in lexicographic order."""
    i, j = np.triu_indices(n, 1)
    k = np.arange(n)
    keep = k[None, :] > j[:, None]
    rows, kk = np.nonzero(keep)
    return i[rows], j[rows], kk


def triple_spans(pos, sc_size):
    """pos[nconf, N] -> d[nconf, C(N,3)] over `triple_index(N)`."""
    z = wrap(pos, sc_size)
    i, j, k = triple_index(z.shape[1])
    x, y, w = z[:, i], z[:, j], z[:, k]
    lo_xy, hi_xy = np.minimum(x, y), np.maximum(x, y)
    a = np.minimum(lo_xy, w)                      # sort three
    c = np.maximum(hi_xy, w)
    b = np.maximum(lo_xy, np.minimum(hi_xy, w))
    gap = np.maximum(np.maximum(b - a, c - b), sc_size - (c - a))
    return sc_size - gap


def span_of(sc_size, max_span=None):
    return 0.5 * sc_size if max_span is None else float(max_span)


def bin_index(d, sc_size, num_bins, max_span=None):
    D = span_of(sc_size, max_span)
    delta = D / num_bins
    b = np.minimum(np.floor_divide(d, delta).astype(np.int64), num_bins - 1)
    return np.where(d < D, b, num_bins)


def counts_from_spans(d, sc_size, num_bins, max_span=None):
    """d[nconf, ntriples] -> T[nconf, num_bins + 1] (int64)."""
    d = np.asarray(d, dtype=np.float64)
    b = bin_index(d, sc_size, num_bins, max_span)
    nconf, K = d.shape[0], num_bins + 1
    flat = b + K * np.arange(nconf, dtype=np.int64)[:, None]
    return np.bincount(flat.reshape(-1), minlength=nconf * K).reshape(nconf, K)


def triple_counts(pos, sc_size, num_bins, max_span=None, chunk=1 << 22):
    """pos[nconf, N] -> T[nconf, num_bins + 1] (int64), brute force."""
    pos = np.asarray(pos, dtype=np.float64)
    nconf, n = pos.shape
    if n < 3:
        return np.zeros((nconf, num_bins + 1), dtype=np.int64)
    step = max(1, chunk // comb(n, 3))
    return np.concatenate([
        counts_from_spans(triple_spans(pos[c:c + step], sc_size), sc_size,
                          num_bins, max_span)
        for c in range(0, nconf, step)])


def rank_counts(pos, sc_size, num_bins, max_span=None):
    """The same histogram by the ordered pair walk (module docstring)."""
    pos = np.asarray(pos, dtype=np.float64)
    nconf, n = pos.shape
    D = span_of(sc_size, max_span)
    delta = D / num_bins
    out = np.zeros((nconf, num_bins + 1), dtype=np.int64)
    if n < 3:
        return out
    z = wrap(pos, sc_size)
    for c in range(nconf):
        zs = z[c][np.argsort(z[c], kind='stable')]      # ties by index
        a = np.arange(n)[:, None]
        m = np.arange(1, n)[None, :]
        r = a + m
        arc = np.where(r < n, zs[r % n], zs[r % n] + sc_size) - zs[a]
        # the arc grows with m: `arc < D` is the prefix the walk visits
        ok = (arc < D) & (m >= 2)
        b = np.minimum(np.floor_divide(arc[ok], delta).astype(np.int64),
                       num_bins - 1)
        mult = np.broadcast_to(m - 1, arc.shape)[ok]
        out[c, :num_bins] = np.bincount(b, weights=mult,
                                        minlength=num_bins).astype(np.int64)
        out[c, num_bins] = comb(n, 3) - out[c, :num_bins].sum()
    return out


def lattice_counts(n, sc_size, num_bins, max_span=None):
    """Closed form for z_i = i L / N -> T[num_bins + 1]."""
    D = span_of(sc_size, max_span)
    delta = D / num_bins
    out = np.zeros(num_bins + 1, dtype=np.int64)
    for m in range(2, n):
        arc = m * sc_size / n
        if not arc < D:
            break
        out[min(int(arc // delta), num_bins - 1)] += n * (m - 1)
    out[num_bins] = comb(n, 3) - out.sum()
    return out


def bin_centres(sc_size, num_bins, max_span=None):
    delta = span_of(sc_size, max_span) / num_bins
    return (np.arange(num_bins) + 0.5) * delta


def expected_uniform(n, sc_size, num_bins, max_span=None):
    """E T[b], b < B, for iid uniform particles."""
    delta = span_of(sc_size, max_span) / num_bins
    return (comb(n, 3) * 3.0 * (delta / sc_size) ** 2
            * (2.0 * np.arange(num_bins) + 1.0))


def normalise(counts, n, sc_size, max_span=None):
    """T[..., B + 1] -> g3[..., B]."""
    counts = np.asarray(counts, dtype=np.float64)
    nb = counts.shape[-1] - 1
    return counts[..., :nb] / expected_uniform(n, sc_size, nb, max_span)


def ambiguous_triples(pos, sc_size, num_bins, max_span=None, d=None):
    """Per configuration the edge-ambiguous triples: a list (one entry per
    configuration) of arrays [k, 3] of rows (i, j, k).  `d`: the spans of
    `triple_spans(pos, sc_size)` where the caller has them."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[1]
    if n < 3:
        return [np.zeros((0, 3), dtype=np.int64) for _ in pos]
    D = span_of(sc_size, max_span)
    delta = D / num_bins
    if d is None:
        d = triple_spans(pos, sc_size)
    q = d / delta
    on_edge = (np.abs(q - np.rint(q)) <= EDGE_EPS) & (q <= num_bins + 0.5)
    on_span = np.abs(d - D) <= EDGE_EPS * sc_size
    i, j, k = triple_index(n)
    out = []
    for c in range(len(pos)):
        t = np.nonzero(on_edge[c] | on_span[c])[0]
        out.append(np.stack([i[t], j[t], k[t]], axis=1).astype(np.int64))
    return out


def num_ambiguous(pos, sc_size, num_bins, max_span=None, d=None):
    return sum(len(a) for a in
               ambiguous_triples(pos, sc_size, num_bins, max_span, d))


def uniform_law_z(counts, n, sc_size, num_bins, max_span=None):
    """counts[nconf, B + 1] -> z[B]: (mean - expectation) over the standard
    error of the mean, from the sample standard deviation over the
    configurations (triples share particles, so the pooled count is not
    binomial)."""
    x = np.asarray(counts, dtype=np.float64)[:, :num_bins]
    sem = x.std(axis=0, ddof=1) / np.sqrt(len(x))
    return (x.mean(axis=0) - expected_uniform(n, sc_size, num_bins,
                                              max_span)) / sem


# ---- inputs shared by the host and the GPU tests ---------------------------
PARITY_SIZES = (3, 4, 8, 16, 37, 64, 65, 100, 128, 130, 260)
PARITY_BINS = (1, 7, 64, 4096)


# (a seed whose rows had an edge-ambiguous triple was replaced)
PARITY_SEEDS = {260: 8260}


def parity_spans(sc_size):
    """D in {L/2, L/8, 0.3 L}."""
    return (0.5 * sc_size, 0.125 * sc_size, 0.3 * sc_size)


def model_spec_args(n):
    """Keyword arguments of a model Spec of n particles in a box of L = n
    (the 'box' family of tests/golden/params.json)."""
    return dict(boson_number=n, interaction_strength=2,
                lattice_depth=5 * np.pi ** 2, lattice_ratio=1,
                supercell_size=n, tbf_contact_cutoff=0.25 * n)


def parity_pool(n):
    """Random rows in the box L = n, some of them outside [0, L):
    8 configurations up to N = 64, 4 up to 130, 2 above."""
    L = float(n)
    rng = np.random.RandomState(PARITY_SEEDS.get(n, 7000 + n))
    nconf = 8 if n <= 64 else 4 if n <= 130 else 2
    pool = L * rng.random_sample((nconf, n))
    pool[0, ::3] += 2.0 * L
    pool[1] -= 0.75 * L
    if nconf > 2:
        pool[2] += 1.5 * L
        pool[3, ::2] -= 7.25 * L
    return pool


def grid_pool(n=64, sc_size=64.0, nconf=6, seed=64):
    """Positions on the 1/8 grid with coincident particles: every operation
    is exact for power-of-two bin counts."""
    rng = np.random.RandomState(seed)
    pos = rng.randint(0, int(8 * sc_size), size=(nconf, n)) / 8.0
    pos[1, :] = np.repeat(pos[1, :n // 2], 2)[:n]      # every particle paired
    pos[:, 1] = pos[:, 0]                   # a coincident pair and a quadruple
    pos[:, 3] = pos[:, 2]
    pos[:, 5] = pos[:, 4] = pos[:, 2]
    return pos


def nesting_pool(n):
    rng = np.random.RandomState(900 + n)
    return float(n) * rng.random_sample((4, n))


def entry_pool(n, nconf=70):
    rng = np.random.RandomState(500 + n)
    return float(n) * rng.random_sample((nconf, n)), rng


# (N, B, D / L) of tests/test_gpu_triple_dist.py::test_entry_points_agree
ENTRY_CASES = ((16, 7, 0.5), (16, 64, 0.125), (37, 7, 0.3), (64, 64, 0.5),
               (100, 7, 0.125), (128, 64, 0.5))
