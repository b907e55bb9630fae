"""NumPy restatement of the imaginary-time density correlation estimator
F(k, tau) of a DMC block, from its definition and in terms of the yielded
states alone.

A block is a list of time steps; step t is `(confs, cloning_ref, num_walkers)`:
the positions `confs[s]` that walker s carries (the yielded configuration), the
cloning table `cloning_ref[s]` (the slot of its parent in the population of
step t - 1) and the number of live walkers nw_t.  Walker s is live if s < nw_t.

Parameters: K modes k_m = 2 pi m / L, m = 0 .. K-1; T lags; lag stride q; lag l
is tau_l = l q dt.  C = T + 2 and a walker's row is row[m][c].  With
rho_m = sum_i exp(i k_m confs_t[s][i]) and r = cloning_ref_t[s],

    t = 0:  row = 0;  row[m][T] = Re rho_m,  row[m][T+1] = Im rho_m,
            row[m][0] = (Re rho_m)^2 + (Im rho_m)^2
    t > 0:  row = rows_{t-1}[r];  if t % q == 0 and l = t / q < T:
            row[m][l] = Re rho_m row[m][T] + Im rho_m row[m][T+1]
    iter[t] = sum_{s live} row                        [K, C]

A clone inherits the row of its parent, a dead walker's row ends.
"""
import numpy as np


def step_positions(confs):
    """confs[W, N] or a State's confs[W, 2, N] -> pos[W, N]."""
    confs = np.asarray(confs, dtype=np.float64)
    return confs[:, 0, :] if confs.ndim == 3 else confs


def momenta(num_modes, sc_size):
    return np.arange(num_modes) * 2 * np.pi / float(sc_size)


def fourier_density(pos, num_modes, sc_size):
    """pos[W, N] -> (Re rho[W, K], Im rho[W, K])."""
    ph = pos[:, np.newaxis, :] * momenta(num_modes, sc_size)[:, np.newaxis]
    return np.cos(ph).sum(axis=2), np.sin(ph).sum(axis=2)


def isf_rows(steps, sc_size, num_modes, num_lags, lag_stride=1):
    """-> iter[len(steps), K, T + 2]: the per-step sums of the rows."""
    K, T, q = int(num_modes), int(num_lags), int(lag_stride)
    out = np.zeros((len(steps), K, T + 2))
    prev = None
    for t, (confs, ref, nw) in enumerate(steps):
        nw = int(nw)
        pos = step_positions(confs)[:nw]
        ref = np.asarray(ref, dtype=np.int64)[:nw]
        measures = t == 0 or (t % q == 0 and t // q < T)
        if measures:
            re, im = fourier_density(pos, K, sc_size)
        if t == 0:
            rows = np.zeros((nw, K, T + 2))
            rows[:, :, T] = re
            rows[:, :, T + 1] = im
            rows[:, :, 0] = re * re + im * im
        else:
            assert ref.max(initial=-1) < len(prev), \
                'a walker descends from a slot that was not live'
            rows = prev[ref].copy()
            if measures:
                rows[:, :, t // q] = re * rows[:, :, T] + im * rows[:, :, T + 1]
        out[t] = rows.sum(axis=0)
        prev = rows
    return out
