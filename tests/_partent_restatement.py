"""NumPy restatement of the one-particle replica swap (csrc/qmc_partent.h),
written from its definition:

    pair p     the rows (2p, 2p + 1) = (R1, R2) = (x1, x2) of pos[nconf, N]
    R1'(i, j)  R1 with its particle i replaced by particle j of R2
    R2'(i, j)  R2 with its particle j replaced by particle i of R1
    log_ratio[i, j] = ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|
    m          N^-2 sum_ij exp(log_ratio[i, j])
    purity     mean of m over independent pairs of |psi|^2;  S2 = -ln purity

`explicit` is that definition with a supplied `wf_abs_log`; `factorised` is
the form the kernel evaluates,

    F[i, j] = lf(x1_i, x2_j),            lf(x, y) = ln f2(|min-image(x - y)|)
    a_i = sum_k F[i, k] - sum_{k != i} lf(x1_i, x1_k)
    b_j = sum_k F[k, j] - sum_{k != j} lf(x2_j, x2_k)
    log_ratio[i, j] = a_i + b_j - 2 F[i, j],

with f2 written out from the model's `tbf_params`;
tests/test_partent_host.py holds the two against each other.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._renyi_restatement import (GOLDEN_SIZES, RTOL, log_f2, min_distance,
                                 model_spec_args, wrap)

__all__ = ['GOLDEN_SIZES', 'RTOL', 'model_spec_args', 'wrap']

PARITY_SIZES = (1, 2, 3, 8, 16, 37, 64, 100, 128)
PARITY_PAIRS = 6
ORDER_SIZES = (16, 37, 128)
THREADS = 16        # the oracle's wf_abs_log releases the interpreter lock


# ---- the definition ----------------------------------------------------------
def swapped(r1, r2, i, j):
    """(R1', R2') of the exchange x1_i <-> x2_j."""
    s1, s2 = r1.copy(), r2.copy()
    s1[i], s2[j] = r2[j], r1[i]
    return s1, s2


def explicit(wf_abs_log, r1, r2, elements=None):
    """-> (log_ratio, scale) of the exchanges `elements` (a list of (i, j);
    all N^2, as [N, N] arrays, when None) with the supplied
    wf_abs_log(pos[N]) -> float; scale = sum of the |four ln psi terms| the
    definition cancels against."""
    n = len(r1)
    todo = ([(i, j) for i in range(n) for j in range(n)]
            if elements is None else list(elements))
    rows = []
    for i, j in todo:
        rows.extend(swapped(r1, r2, i, j))
    rows = np.array(rows)
    w = np.empty(len(rows))

    def work(k):                 # every THREADS-th row: one task per thread
        w[k::THREADS] = [wf_abs_log(z) for z in rows[k::THREADS]]
    if len(rows) > 256:
        with ThreadPoolExecutor(THREADS) as ex:
            list(ex.map(work, range(THREADS)))
    else:
        for k in range(THREADS):
            work(k)
    w1, w2 = w[0::2], w[1::2]
    l1, l2 = wf_abs_log(r1), wf_abs_log(r2)
    lr = w1 + w2 - l1 - l2
    scale = np.abs(w1) + np.abs(w2) + abs(l1) + abs(l2)
    if elements is None:
        return lr.reshape(n, n), scale.reshape(n, n)
    return lr, scale


def mean_of(log_ratio):
    """m of log_ratio[..., N, N], the argument of exp clamped to +-700."""
    return np.exp(np.clip(log_ratio, -700.0, 700.0)).mean(axis=(-2, -1))


def reference(wf_abs_log, pos, sc_size):
    """pos[2 P, N] -> (log_ratio[P, N, N], scale[P, N, N], mean[P]) by the
    explicit route on the positions brought into the box."""
    z = wrap(pos, sc_size)
    out = [explicit(wf_abs_log, z[2 * p], z[2 * p + 1])
           for p in range(len(z) // 2)]
    lr = np.stack([o[0] for o in out])
    return lr, np.stack([o[1] for o in out]), mean_of(lr)


# ---- the factorised form -----------------------------------------------------
def _lf(x, y, tbf, sc_size):
    r = np.abs(min_distance(x[..., :, None], y[..., None, :], sc_size))
    with np.errstate(invalid='ignore'):     # beta = 0 at r = 0 (masked later)
        return log_f2(r, tbf, sc_size)


def factorised(tbf, sc_size, pos, with_scale=False):
    """pos[2 P, N] (any images) -> log_ratio[P, N, N]; with_scale adds
    scale[P, N, N], the sum of the magnitudes of the terms of an element."""
    z = wrap(np.asarray(pos, dtype=np.float64), sc_size)
    x1, x2 = z[0::2], z[1::2]
    n = z.shape[1]
    off = ~np.eye(n, dtype=bool)
    F = _lf(x1, x2, tbf, sc_size)                       # [P, i, j]
    own1 = np.where(off, _lf(x1, x1, tbf, sc_size), 0.0)
    own2 = np.where(off, _lf(x2, x2, tbf, sc_size), 0.0)
    a = F.sum(axis=2) - own1.sum(axis=2)                # [P, i]
    b = F.sum(axis=1) - own2.sum(axis=2)                # [P, j]
    lr = a[:, :, None] + b[:, None, :] - 2.0 * F
    if not with_scale:
        return lr
    sa = np.abs(F).sum(axis=2) + np.abs(own1).sum(axis=2)
    sb = np.abs(F).sum(axis=1) + np.abs(own2).sum(axis=2)
    return lr, sa[:, :, None] + sb[:, None, :] + 2.0 * np.abs(F)


def within_tolerance(dev, ref, scale):
    """|dev - ref| <= RTOL max(1, scale) -> (ok, worst error / bound)."""
    ratio = np.abs(np.asarray(dev) - ref) / (RTOL * np.maximum(1.0, scale))
    return bool(np.all(ratio <= 1.0)), float(ratio.max())


def mean_within_tolerance(dev, ref, scale):
    """|dev - ref| <= RTOL max(1, max scale of the pair) ref."""
    top = np.maximum(1.0, scale.reshape(len(ref), -1).max(axis=1))
    ratio = np.abs(np.asarray(dev) - ref) / (RTOL * top * ref)
    return bool(np.all(ratio <= 1.0)), float(ratio.max())


# ---- inputs shared by the host and the GPU tests -------------------------------
def pool(n, npair=PARITY_PAIRS, seed=None):
    """pos[2 npair, N] of random rows in the box L = n, some particles whole
    periods outside [0, L), in both replicas of a pair and in one alone."""
    L = float(n)
    rng = np.random.RandomState(9100 + n if seed is None else seed)
    rows = L * rng.random_sample((2 * npair, n))
    rows[0, ::3] += 2.0 * L
    rows[1] -= 3.0 * L
    rows[2, ::2] -= 1.0 * L
    rows[-1] += 5.0 * L
    rows[-2, 1::2] -= 2.0 * L
    return rows


def large_case(n=512):
    """N = 512: 2 pairs, and 64 drawn elements (pair, i, j) for the oracle."""
    rows = pool(n, npair=2)
    rng = np.random.RandomState(512)
    return rows, np.stack([rng.randint(0, 2, 64), rng.randint(0, n, 64),
                           rng.randint(0, n, 64)], axis=1)


def reorderings(pos, seed):
    """-> (sorted rows, perm_sorted, shuffled rows, perm_shuffled): every row
    sorted ascending by its image in the box, and every row shuffled on its
    own; row c of the reordered batch is pos[c, perm[c]]."""
    n = pos.shape[1]
    rng = np.random.RandomState(seed)
    ps = np.argsort(wrap(pos, float(n)), axis=1, kind='stable')
    pr = np.stack([rng.permutation(n) for _ in pos])
    take = np.take_along_axis
    return take(pos, ps, axis=1), ps, take(pos, pr, axis=1), pr


def permuted(log_ratio, perm):
    """log_ratio[P, N, N] of the rows as given -> that of the rows reordered
    by perm[2 P, N]."""
    out = np.empty_like(log_ratio)
    for p in range(len(log_ratio)):
        out[p] = log_ratio[p][np.ix_(perm[2 * p], perm[2 * p + 1])]
    return out


# ---- the known answer: N = 2 without a lattice ---------------------------------
KNOWN = dict(grid=24, npair=8192, seed=2024, sigmas=4.5)


def known_answer(tbf, sc_size):
    """Two particles on a ring without a lattice, psi = f2(x1 - x2), on the
    G x G grid x = (k + 1/2) L / G with weights w ~ psi^2.
    -> (E m, E m^2, pos[2 npair, 2]): the exact 4-fold grid sums of the
    factorised restatement over two independent grid configurations, and
    2 npair configurations drawn from that discrete law with a fixed seed."""
    G = KNOWN['grid']
    x = (np.arange(G) + 0.5) * sc_size / G
    conf = np.stack(np.meshgrid(x, x, indexing='ij'), axis=-1).reshape(-1, 2)
    lw = 2.0 * log_f2(np.abs(min_distance(conf[:, 0], conf[:, 1], sc_size)),
                      tbf, sc_size)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    S = len(conf)
    em = em2 = 0.0
    for c in range(S):                       # R1 = conf[c], every R2
        rows = np.empty((2 * S, 2))
        rows[0::2] = conf[c]
        rows[1::2] = conf
        m = mean_of(factorised(tbf, sc_size, rows))
        em += w[c] * np.dot(w, m)
        em2 += w[c] * np.dot(w, m * m)
    rng = np.random.RandomState(KNOWN['seed'])
    draw = rng.choice(S, size=2 * KNOWN['npair'], p=w)
    return em, em2, conf[draw]


def known_answer_z(mean, em, em2):
    """(mean of the per-pair m - E m) in units of sigma =
    sqrt((E m^2 - (E m)^2) / npair)."""
    sigma = np.sqrt((em2 - em * em) / KNOWN['npair'])
    return float((np.mean(mean) - em) / sigma)
