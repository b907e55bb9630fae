"""NumPy restatement of the replica swap of regions made of up to two segments
(csrc/qmc_renyi_region.h), written from its definition:

    pair p    the rows (2p, 2p + 1) = (R1, R2) of pos[nconf, N], nconf even
    X_k       regions[k] = (l1, g, l2) with l1 > 0, g >= 0, l2 >= 0, m2 < L,
              m1 = l1 + g and m2 = m1 + l2 formed in fp64 in this order
    t         as tests/_renyi_restatement.py: zw - a0w, plus L where negative
    inX_k(i)  t_i < l1  or  (m1 <= t_i and t_i < m2)
    n_x[c,k]  number of particles of configuration c in X_k
    matched   n_x[2p, k] == n_x[2p + 1, k]   (the TOTALS, not the windows)
    R1', R2'  X(R2) u Y(R1),  X(R1) u Y(R2),   Y the complement
    log_ratio ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|
              where matched, -inf otherwise

`swapped`, `explicit_log_ratio` and `cross_log_ratio` of the one-segment
restatement take arbitrary boolean masks and are used as they stand; only the
membership is new.  A membership can change by rounding only where t sits on a
mark to within rounding: `ambiguous` lists the particles with t within
EDGE_EPS L of 0, L, l1, m1 or m2.
"""
import numpy as np

from ._pairdist_restatement import EDGE_EPS, wrap                 # noqa: F401
from ._renyi_restatement import (GOLDEN_SIZES, RTOL,              # noqa: F401
                                 cross_log_ratio, explicit_log_ratio,
                                 model_spec_args, within_tolerance)
from . import _renyi_restatement as rs


def marks(regions):
    """regions[K, 3] -> (l1[K], m1[K], m2[K]), in the stated order."""
    rg = np.asarray(regions, dtype=np.float64).reshape(-1, 3)
    l1 = rg[:, 0]
    m1 = l1 + rg[:, 1]
    m2 = m1 + rg[:, 2]
    return l1, m1, m2


def windows(pos, sc_size, regions, origin):
    """pos[nconf, N] -> (in1[nconf, N, K], in2[nconf, N, K]): the particles of
    the first and of the second window of every region."""
    t = rs.offsets(pos, sc_size, origin)[:, :, None]
    l1, m1, m2 = (a[None, None, :] for a in marks(regions))
    return t < l1, (m1 <= t) & (t < m2)


def membership(pos, sc_size, regions, origin):
    """pos[nconf, N] -> (inX[nconf, N, K] bool, n_x[nconf, K] int32)."""
    in1, in2 = windows(pos, sc_size, regions, origin)
    in_x = in1 | in2
    return in_x, in_x.sum(axis=1).astype(np.int32)


matched = rs.matched


def all_marks(regions):
    return np.concatenate(marks(regions))


def ambiguous(pos, sc_size, regions, origin):
    """Rows (c, i) of the particles whose t is within EDGE_EPS L of 0, L, l1,
    m1 or m2 of some region -> int64[k, 2]."""
    return rs.ambiguous(pos, sc_size, all_marks(regions), origin)


def split_differently(pos, sc_size, regions, origin):
    """-> bool[P, K]: matched entries whose two replicas divide their count
    differently between the two windows (what a prefix cannot represent)."""
    in1, in2 = windows(pos, sc_size, regions, origin)
    c1, c2 = in1.sum(axis=1), in2.sum(axis=1)
    same_total = (c1 + c2)[0::2] == (c1 + c2)[1::2]
    return same_total & (c1[0::2] != c1[1::2])


def reference(wf_abs_log, pos, sc_size, regions, origin):
    """pos[nconf, N] -> (n_x[nconf, K], log_ratio[P, K], scale[P, K]) by the
    explicit route on the positions brought into the box; scale is 0 where the
    pair is not matched."""
    z = wrap(pos, sc_size)
    in_x, n_x = membership(pos, sc_size, regions, origin)
    ok = matched(n_x)
    lr = np.full(ok.shape, -np.inf)
    scale = np.zeros(ok.shape)
    for p, k in np.argwhere(ok):
        lr[p, k], scale[p, k] = explicit_log_ratio(
            wf_abs_log, z[2 * p], z[2 * p + 1], in_x[2 * p, :, k],
            in_x[2 * p + 1, :, k])
    return n_x, lr, scale


# ---- inputs shared by the host and the GPU tests ---------------------------
PARITY_SIZES = rs.PARITY_SIZES
# (l1, g, l2) / L: two windows that touch, a single segment, the generic case,
# a second window that ends near L, and a wide gap
PARITY_FRACTIONS = ((0.11, 0.0, 0.2), (0.27, 0.13, 0.0), (0.2, 0.15, 0.25),
                    (0.3, 0.25, 0.44), (0.07, 0.5, 0.1))
MANY_REGIONS = 130           # more regions than one pass of lanes


def parity_regions(n):
    return float(n) * np.array(PARITY_FRACTIONS)


def many_regions(n, num):
    """`num` regions of a box of L = n: l1, g and l2 sweep through it, every
    third one a single segment, every fifth with g = 0."""
    k = np.arange(num)
    l1 = (0.05 + 0.4 * (k + 0.5) / num)
    g = np.where(k % 5 == 0, 0.0, 0.02 + 0.2 * ((7 * k) % num + 0.25) / num)
    l2 = np.where(k % 3 == 0, 0.0, 0.03 + 0.25 * ((11 * k) % num + 0.75) / num)
    return float(n) * np.stack([l1, g, l2], axis=1)


# (N, origin index) or a case name -> a seed under which the pool meets the
# three conditions on the restatement alone (found by trying 0, 1, 2, ...)
POOL_SEEDS = {(2, 0): 0, (8, 0): 0, (100, 0): 1, (100, 1): 2}


def pool(n, regions, origin, seed=None, **kw):
    """The pool of tests/_renyi_restatement.py with every mark of every region
    a cut: the made pairs match at every region, window by window; the random
    pairs bring the unmatched entries and the different splits."""
    return rs.pool(n, all_marks(regions), origin, seed=seed, **kw)


def parity_cases(n):
    """(origin, regions, pos) of the parity test of size n, one per origin."""
    regions = parity_regions(n)
    return [(origin, regions,
             pool(n, regions, origin, seed=POOL_SEEDS.get((n, io))))
            for io, origin in enumerate(rs.parity_origins(n))]


def many_regions_case(n=16):
    regions = many_regions(n, MANY_REGIONS)
    origin = rs.parity_origins(n)[1]
    return origin, regions, pool(n, regions, origin,
                                 seed=POOL_SEEDS.get('many'))


def large_case(n=512):
    """N = 512: the four rows of `large_case` of the one-segment tests (a made
    pair and a random one) with five regions; the first three have their marks
    on the cuts that pool was made for, so the made pair matches there, and
    the last is one at which the random pair holds the same total, divided
    differently between the windows (found by a scan of g and l2)."""
    _, origin, _, rows = rs.large_case(n)
    regions = float(n) * np.array([[0.2, 0.3, 0.21], [0.2, 0.0, 0.3],
                                   [0.5, 0.21, 0.0], [0.2, 0.51, 0.28],
                                   [0.2, 0.1125, 0.2625]])
    return origin, regions, rs.large_rows(rows)


def pool_conditions(pos, sc_size, regions, origin):
    """-> (ambiguous particles, matched entries, unmatched entries, matched
    entries split differently between the windows)."""
    _, n_x = membership(pos, sc_size, regions, origin)
    ok = matched(n_x)
    return (len(ambiguous(pos, sc_size, regions, origin)), int(ok.sum()),
            int((~ok).sum()),
            int(split_differently(pos, sc_size, regions, origin).sum()))


def assert_pool_conditions(pos, sc_size, regions, origin):
    amb, hit, miss, split = pool_conditions(pos, sc_size, regions, origin)
    assert amb == 0
    assert hit >= 8
    assert miss >= 1
    assert split >= 1


# ---- the known answer of free particles --------------------------------------
KNOWN_REGIONS = ((1.0, 1.0, 1.0), (2.0, 0.5, 2.0), (4.0, 0.0, 0.0))


def known_answer_expected():
    """Free uniform particles, x = (l1 + l2) / L: the count of a row in X is
    binomial -> (pmf[K, N + 1], E swap[K] = sum_n pmf^2)."""
    from math import comb
    n = rs.KNOWN['n']
    rg = np.array(KNOWN_REGIONS)
    x = (rg[:, 0] + rg[:, 2]) / rs.KNOWN['sc_size']
    k = np.arange(n + 1)
    c = np.array([comb(n, int(i)) for i in k], dtype=np.float64)
    pmf = c[None, :] * x[:, None] ** k * (1.0 - x[:, None]) ** (n - k)
    return pmf, (pmf ** 2).sum(axis=1)


def known_z(counts_swap, counts_conf, match, P):
    """z scores of <swap>, p(n) and <swap delta_n> against the binomial law
    and its standard errors over P pairs (2P rows), from the sums: swap
    resolved by charge [K, N + 1], rows per charge [K, N + 1], matched [K]."""
    pmf, want = known_answer_expected()
    z_swap = (match / P - want) / np.sqrt(want * (1 - want) / P)
    z_prob = ((counts_conf / (2.0 * P) - pmf)
              / np.sqrt(pmf * (1 - pmf) / (2 * P)))
    p2 = pmf ** 2
    z_cs = (counts_swap / P - p2) / np.sqrt(p2 * (1 - p2) / P)
    return z_swap, z_prob, z_cs
