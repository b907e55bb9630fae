"""NumPy restatement of the replica-swap estimator of the Renyi-2 entanglement
entropy (csrc/qmc_renyi.h), written from its definition:

    pair p    the rows (2p, 2p + 1) = (R1, R2) of pos[nconf, N], nconf even
    A_k       [a0, a0 + l_k) on the ring of length L, 0 < l_k < L; B_k the rest
    zw, a0w   z and a0 brought into [0, L)
    t         zw - a0w, plus L where negative
    inA_k(i)  t_i < l_k
    n_A[c,k]  number of particles of configuration c in A_k
    matched   n_A[2p, k] == n_A[2p + 1, k]
    R1', R2'  A(R2) u B(R1),  A(R1) u B(R2)            (N particles each)
    log_ratio ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|
              where matched, -inf otherwise
    swap      exp(log_ratio);  S2(l_k) = -ln(sum_p swap[p, k] / P)

`explicit_log_ratio` is that definition with a supplied `wf_abs_log`;
`cross_log_ratio` is the cross-pair form the kernel evaluates,

    S(A2, B1) + S(A1, B2) - S(A1, B1) - S(A2, B2),
    S(X, Y) = sum_{x in X, y in Y} ln f2(|min-image(x - y)|),

with f2 written out from the model's `tbf_params`;
tests/test_renyi_host.py holds the two against each other.

Rounding can change a membership only where t sits on a cut to within
rounding.  `ambiguous` lists such particles with the margin of
tests/_pairdist_restatement.py: t within EDGE_EPS L of 0, of L or of some l_k.
"""
from math import comb

import numpy as np

from ._pairdist_restatement import EDGE_EPS, min_distance, wrap

RTOL = 2e-11         # of tests/test_gpu_pair_dist.py

GOLDEN_SIZES = {8: 'box8', 16: 'box16', 37: 'box37', 64: 'box64',
                100: 'box100', 128: 'box128', 512: 'box512'}


def model_spec_args(n):
    """Keyword arguments of a model Spec of n particles in a box of L = n
    (the 'box' family of tests/golden/params.json)."""
    return dict(boson_number=n, interaction_strength=2,
                lattice_depth=5 * np.pi ** 2, lattice_ratio=1,
                supercell_size=n, tbf_contact_cutoff=0.25 * n)


def offsets(pos, sc_size, origin):
    """t[nconf, N] in [0, L]."""
    z = wrap(pos, sc_size)
    t = z - wrap(origin, sc_size)
    return np.where(t < 0, t + sc_size, t)


def membership(pos, sc_size, lengths, origin):
    """pos[nconf, N] -> (inA[nconf, N, K] bool, n_a[nconf, K] int32)."""
    t = offsets(pos, sc_size, origin)
    in_a = t[:, :, None] < np.asarray(lengths, dtype=np.float64)[None, None, :]
    return in_a, in_a.sum(axis=1).astype(np.int32)


def matched(n_a):
    """n_a[nconf, K] -> matched[nconf / 2, K]."""
    return n_a[0::2] == n_a[1::2]


def ambiguous(pos, sc_size, lengths, origin):
    """Rows (c, i) of the particles whose t is within EDGE_EPS L of 0, of L or
    of some length -> int64[k, 2]."""
    t = offsets(pos, sc_size, origin)
    marks = np.concatenate([[0.0, sc_size],
                            np.asarray(lengths, dtype=np.float64)])
    near = np.abs(t[:, :, None] - marks[None, None, :]) <= EDGE_EPS * sc_size
    return np.argwhere(near.any(axis=2)).astype(np.int64)


def swapped(r1, r2, in1, in2):
    """The swapped configurations (R1', R2') of a matched pair at one length:
    positions r1, r2 (N each) and the memberships in1, in2 (bool, N each)."""
    assert in1.sum() == in2.sum()
    return (np.concatenate([r2[in2], r1[~in1]]),
            np.concatenate([r1[in1], r2[~in2]]))


def explicit_log_ratio(wf_abs_log, r1, r2, in1, in2):
    """-> (log_ratio, scale): the definition with the supplied
    wf_abs_log(pos[N]) -> float, and scale = sum of the |four ln psi terms| it
    cancels against."""
    s1, s2 = swapped(r1, r2, in1, in2)
    terms = [wf_abs_log(s1), wf_abs_log(s2), wf_abs_log(r1), wf_abs_log(r2)]
    return (terms[0] + terms[1] - terms[2] - terms[3],
            float(np.sum(np.abs(terms))))


def log_f2(r, tbf, sc_size):
    """ln|f2(r)| of the model's two-body factor, from its tbf_params (a dict
    or a named tuple): |a_m cos(k2 (r - r_off))| below the contact cutoff,
    sin(pi r / L)^beta from there on."""
    def g(k):
        return float(tbf[k] if isinstance(tbf, dict) else getattr(tbf, k))
    r = np.asarray(r, dtype=np.float64)
    short = np.abs(g('param_am') * np.cos(g('param_k2')
                                          * (r - g('param_r_off'))))
    with np.errstate(divide='ignore'):
        long_ = g('param_beta') * np.log(np.sin(np.pi * r / sc_size))
        return np.where(r < abs(g('tbf_contact_cutoff')), np.log(short), long_)


def cross_sum(x, y, tbf, sc_size):
    """S(X, Y)."""
    if len(x) == 0 or len(y) == 0:
        return 0.0
    r = np.abs(min_distance(x[:, None], y[None, :], sc_size))
    return float(log_f2(r, tbf, sc_size).sum())


def cross_log_ratio(tbf, sc_size, r1, r2, in1, in2):
    """The cross-pair form on positions inside the box."""
    a1, b1, a2, b2 = r1[in1], r1[~in1], r2[in2], r2[~in2]
    return (cross_sum(a2, b1, tbf, sc_size) + cross_sum(a1, b2, tbf, sc_size)
            - cross_sum(a1, b1, tbf, sc_size)
            - cross_sum(a2, b2, tbf, sc_size))


def reference(wf_abs_log, pos, sc_size, lengths, origin):
    """pos[nconf, N] -> (n_a[nconf, K], log_ratio[P, K], scale[P, K]) by the
    explicit route on the positions brought into the box; scale is 0 where the
    pair is not matched."""
    z = wrap(pos, sc_size)
    in_a, n_a = membership(pos, sc_size, lengths, origin)
    ok = matched(n_a)
    lr = np.full(ok.shape, -np.inf)
    scale = np.zeros(ok.shape)
    for p, k in np.argwhere(ok):
        lr[p, k], scale[p, k] = explicit_log_ratio(
            wf_abs_log, z[2 * p], z[2 * p + 1], in_a[2 * p, :, k],
            in_a[2 * p + 1, :, k])
    return n_a, lr, scale


def within_tolerance(dev, ref, scale):
    """|dev - ref| <= RTOL max(1, scale) on the matched entries, -inf exactly
    on the others -> (ok, worst ratio of the error to its bound)."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    fin = np.isfinite(ref)
    same_inf = np.array_equal(np.isneginf(dev), ~fin)
    if not fin.any():
        return same_inf, 0.0
    if not same_inf:
        return False, np.inf
    ratio = np.abs(dev[fin] - ref[fin]) / (RTOL * np.maximum(1.0, scale[fin]))
    return bool(np.all(ratio <= 1.0)), float(ratio.max())


# ---- inputs shared by the host and the GPU tests ---------------------------
PARITY_SIZES = (1, 2, 8, 16, 37, 64, 100, 128)
PARITY_FRACTIONS = {1: (0.37,), 5: (0.11, 0.27, 0.5, 0.63, 0.93)}
MANY_LENGTHS = 130           # more lengths than one pass of lanes


def parity_lengths(n, num_lengths):
    if num_lengths in PARITY_FRACTIONS:
        return float(n) * np.array(PARITY_FRACTIONS[num_lengths])
    return float(n) * (np.arange(num_lengths) + 0.5) / (num_lengths + 1)


def parity_origins(n):
    """Two origins, one of them negative (and outside the box)."""
    return (0.3 * n + 0.0625, -1.7 * n - 0.21)


# (N, K, origin index) -> a seed, where the default gave an ambiguous particle
# or missed a pool condition
POOL_SEEDS = {}


def pool(n, lengths, origin, npair_made=8, npair_random=4, seed=None):
    """pos[2 (npair_made + npair_random), N] in the box L = n, some of it
    outside [0, L): pairs of a random configuration and a copy whose particles
    are each moved by less than half their distance to the nearest cut (such
    a pair matches at every length), then pairs of two random
    configurations."""
    L = float(n)
    rng = np.random.RandomState(9000 + n if seed is None else seed)
    lengths = np.asarray(lengths, dtype=np.float64)
    cuts = np.mod(np.concatenate([[origin], origin + lengths]), L)
    made = L * rng.random_sample((npair_made, n))
    d = np.abs(made[:, :, None] - cuts[None, None, :])
    d = np.minimum(d, L - d).min(axis=2)          # to the nearest cut
    moved = made + d * rng.uniform(-0.5, 0.5, size=made.shape)
    rows = np.empty((2 * (npair_made + npair_random), n))
    rows[0:2 * npair_made:2] = made
    rows[1:2 * npair_made:2] = moved
    rows[2 * npair_made:] = L * rng.random_sample((2 * npair_random, n))
    # whole periods away, in both replicas of a pair and in one alone
    rows[0, ::3] += 2.0 * L
    rows[1] -= 3.0 * L
    rows[2, ::2] -= 1.0 * L
    rows[-1] += 5.0 * L
    rows[-2, 1::2] -= 2.0 * L
    return rows


def parity_cases(n):
    """(K, origin, lengths, pos) of the parity test of size n."""
    out = []
    for K in (1, 5):
        for io, origin in enumerate(parity_origins(n)):
            lengths = parity_lengths(n, K)
            out.append((K, origin, lengths,
                        pool(n, lengths, origin,
                             seed=POOL_SEEDS.get((n, K, io)))))
    return out


def many_lengths_case(n=16):
    lengths = parity_lengths(n, MANY_LENGTHS)
    origin = parity_origins(n)[1]
    return (MANY_LENGTHS, origin, lengths,
            pool(n, lengths, origin, seed=POOL_SEEDS.get((n, MANY_LENGTHS, 1))))


def large_case(n=512):
    """N = 512, 3 lengths: a pool of 4 pairs (3 made, 1 random), so that it
    can meet the conditions of every pool (8 matched entries need more than
    2 pairs x 3 lengths); `large_rows` takes the run of 2 pairs out of it."""
    lengths = float(n) * np.array([0.2, 0.5, 0.71])
    origin = parity_origins(n)[1]
    rows = pool(n, lengths, origin, npair_made=3, npair_random=1)
    return 3, origin, lengths, rows


def large_rows(rows):
    """The 2 pairs x 3 lengths run of N = 512: one made pair and the random
    pair of `large_case`."""
    return np.concatenate([rows[0:2], rows[6:8]])


def pool_conditions(pos, sc_size, lengths, origin):
    """-> (ambiguous particles, matched entries, unmatched entries)."""
    _, n_a = membership(pos, sc_size, lengths, origin)
    ok = matched(n_a)
    return (len(ambiguous(pos, sc_size, lengths, origin)), int(ok.sum()),
            int((~ok).sum()))


def assert_pool_conditions(pos, sc_size, lengths, origin):
    amb, hit, miss = pool_conditions(pos, sc_size, lengths, origin)
    assert amb == 0
    assert hit >= 8
    assert miss >= 1


# ---- the known answer of free particles --------------------------------------
KNOWN = dict(n=8, sc_size=8.0, nconf=8192, origins=(0.0, -0.25),
             lengths=(1.0, 2.0, 4.0, 6.5))


def known_answer_inputs():
    return KNOWN['sc_size'] * np.random.RandomState(0).random_sample(
        (KNOWN['nconf'], KNOWN['n']))


def known_answer_expected():
    """E swap = sum_n [C(N,n) x^n (1 - x)^(N - n)]^2, x = l / L: the
    probability that two independent rows of N uniform particles hold the
    same number in A (swap is 1 there and 0 elsewhere without interactions)
    -> (p[K], binomial standard error of the mean over the P pairs)."""
    n = KNOWN['n']
    x = np.array(KNOWN['lengths']) / KNOWN['sc_size']
    k = np.arange(n + 1)
    c = np.array([comb(n, int(i)) for i in k], dtype=np.float64)
    pmf = c[None, :] * x[:, None] ** k * (1.0 - x[:, None]) ** (n - k)
    p = (pmf ** 2).sum(axis=1)
    return p, np.sqrt(p * (1.0 - p) / (KNOWN['nconf'] // 2))
