"""NumPy restatement of the centre-of-mass diffusion estimator of a DMC block
(the winding-number estimator of the superfluid fraction), from its definition
and in terms of the yielded states alone.

A block is a list of time steps; step t is `(confs, cloning_ref, num_walkers)`:
the positions `confs[s]` that walker s carries (the yielded configuration), the
cloning table `cloning_ref[s]` (the slot of its parent in the population of
step t - 1) and the number of live walkers nw_t.  Walker s is live if s < nw_t.
With X_t[s] = sum_i confs_t[s][i] and r = cloning_ref_t[s],

    raw     = X_t[s] - X_{t-1}[r]
    d       = raw - L rint(raw / L)                   (minimum image)
    Y_t[s]  = Y_{t-1}[r] + d,          Y_0 = 0
    iter[t] = (sum_{s live} Y_t[s], sum_{s live} Y_t[s]^2)

Y_t[s] is N times the unwrapped displacement of the centre of mass of walker s
since the first step of the block: a clone inherits the Y of its parent, a dead
walker's history ends.  X does not change under a permutation of a row, and a
wrap of one particle by L moves raw by L, which the minimum image takes out.

Rounding bound of a comparison with the kernel (`tolerance`).  The kernel sums
the N differences c_i - p_i of two rows, the restatement subtracts the sums of
two yielded rows; every term is below L in magnitude and every partial sum
below N L, so any order of either sum errs by at most g = 4 N^2 L 2^-53 (N
additions, each off by at most half an ulp of N L, on both sides, with a factor
two to spare), and as long as both pick the same image (the callers assert
max |d| < L / 4) the minimum image step does not add to it.  Y_t is a sum of at
most T such steps: |Y - Y'| <= T g.  Hence, per row,

    |sum_s Y   - sum_s Y'  | <= nw T g
    |sum_s Y^2 - sum_s Y'^2| <= nw 2 max|Y| T g

(the second to first order in T g, which is below 1e-9 in the suite).  The sums
over the walkers themselves, in whatever order, err by at most nw 2^-53 times
their largest partial sum, nw max|Y| or nw max|Y|^2: that fits into the factor
two spared above as long as nw max|Y| <= 2 T N^2 L, which `tolerance` asserts.
"""
import numpy as np


def step_positions(confs):
    """confs[W, N] or a State's confs[W, 2, N] -> pos[W, N]."""
    confs = np.asarray(confs, dtype=np.float64)
    return confs[:, 0, :] if confs.ndim == 3 else confs


def _walk(steps, sc_size):
    """-> (rows, num_wrapped, max_abs_d, max_abs_y)"""
    L = float(sc_size)
    rows = np.zeros((len(steps), 2))
    num_wrapped, max_abs_d, max_abs_y = 0, 0.0, 0.0
    x_prev = y_prev = None
    for t, (confs, ref, nw) in enumerate(steps):
        nw = int(nw)
        x = step_positions(confs)[:nw].sum(axis=1)
        ref = np.asarray(ref, dtype=np.int64)[:nw]
        y = np.zeros(nw)
        if t > 0:
            assert ref.max(initial=-1) < len(y_prev), \
                'a walker descends from a slot that was not live'
            raw = x - x_prev[ref]
            d = raw - L * np.rint(raw / L)
            num_wrapped += int(np.count_nonzero(np.abs(raw) > 0.5 * L))
            max_abs_d = max(max_abs_d, float(np.abs(d).max(initial=0.0)))
            y = y_prev[ref] + d
        max_abs_y = max(max_abs_y, float(np.abs(y).max(initial=0.0)))
        rows[t] = y.sum(), (y * y).sum()
        x_prev, y_prev = x, y
    return rows, num_wrapped, max_abs_d, max_abs_y


def cm_diffusion(steps, sc_size):
    """-> (rows[T, 2], num_wrapped, max_abs_d): the per-step sums, the number
    of walker-steps whose raw difference exceeded L/2 in magnitude (a wrap
    happened) and the largest |d| met."""
    return _walk(steps, sc_size)[:3]


def largest_y(steps, sc_size):
    """The largest |Y_t[s]| of the block (for rounding bounds)."""
    return _walk(steps, sc_size)[3]


def tolerance(steps, n, sc_size):
    """tol[T, 2] of the module docstring, for the rows of a block of T =
    len(steps) steps of N = n particles."""
    L, T = float(sc_size), len(steps)
    g = 4.0 * n * n * L * 2.0 ** -53
    nw = np.array([s[2] for s in steps], dtype=np.float64)
    max_y = largest_y(steps, L)
    assert nw.max() * max_y <= 2.0 * T * n * n * L
    return np.stack([nw * T * g, nw * 2.0 * max_y * T * g], axis=1)
