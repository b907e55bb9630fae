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

Rounding bound of a comparison with the kernel (`tolerance`), e = 2^-53,
positions in [0, L] (the callers assert it).

Per term exp(i k_m z), kernel against restatement, as a complex magnitude:
  * argument.  The kernel forms u = fl(fl(4 / L) z), relative error 2 e, the
    angle of mode 1 being (pi / 2) u <= 2 pi: 4 pi e; mode m = 8 a + b is the
    product of table entries with angles b and 8 a times that (8 u is exact),
    so its angle is off by m 4 pi e.  The restatement forms
    fl(fl(fl(2 m fl(pi)) / L) z), relative error 4 e of an angle <= 2 pi m:
    8 pi m e.  Together 12 pi m e.
  * sincos_halfpi: 2 ulp of a value <= 1, 4 e per
    component, 4 sqrt(2) e for the pair; the b-th power of the pair carries b
    times that, b <= 7: 28 sqrt(2) e per table.
  * growth of the recurrence.  Every rotation of a table (two products and a
    sum per component, terms <= 1) adds at most 8 e per component, 8 sqrt(2) e
    for the pair, seven times: 56 sqrt(2) e per table.
  * the product of the two table entries inherits the sum of both tables'
    errors: 2 (28 + 56) sqrt(2) e < 240 e.
  * NumPy's cos and sin: 1 ulp each, 2 sqrt(2) e < 3 e for the pair.
  delta_m = (12 pi m + 243) e.

rho_m is a sum of N such terms, each <= 1: N delta_m, plus the roundings of the
sums.  The j-th addition of any order rounds a partial sum <= j: N^2 e / 2 per
sum; the kernel's real and imaginary parts are differences of two accumulator
tiles (N^2 e + N e), the restatement's are one sum each (N^2 e / 2): below
2 N^2 e per component, 3 N^2 e for the pair.
  D_m = N delta_m + 3 N^2 e.

Row entries of one walker, |rho| <= N: columns T and T+1 (the origin) are off
by at most D_m; column 0, |rho|^2, and column l, Re rho conj(rho_0), by
2 N D_m + D_m^2 plus three roundings of values <= N^2 on each side:
  Q_m = 2 N D_m (1 + 1e-6) + 6 N^2 e.
The transport copies.  Sums over nw walkers of entries <= N^2 (N for the
origin), any order, both sides: nw^2 N^2 e (nw^2 N e).
  tol[t][m][c] = nw_t Q_m + nw_t^2 N^2 e   (c < T)
  tol[t][m][c] = nw_t D_m + nw_t^2 N e     (c = T, T+1)
Nothing is fitted to what the kernel gives.
"""
from math import pi

import numpy as np

EPS = 2.0 ** -53


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


def tolerance(n, K, T, num_walkers):
    """tol[nts, K, T + 2] of the module docstring."""
    m = np.arange(K, dtype=np.float64)
    delta = (12.0 * pi * m + 243.0) * EPS
    d = n * delta + 3.0 * n * n * EPS
    qd = 2.0 * n * d * (1.0 + 1e-6) + 6.0 * n * n * EPS
    nw = np.asarray(num_walkers, dtype=np.float64)[:, None]
    tol = np.empty((len(nw), K, T + 2))
    tol[:, :, :T] = (nw * qd + nw * nw * n * n * EPS)[:, :, None]
    tol[:, :, T:] = (nw * d + nw * nw * n * EPS)[:, :, None]
    return tol
