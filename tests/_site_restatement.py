"""NumPy forward walking of the site occupation rows: the DMC block estimator
of P(n) and <n_c n_{c+d}>, restated from its definition (csrc/qmc_site.h).

The lattice period is 1 and the supercell holds S = L sites; site c is well c
with half a barrier on each side.  Per configuration

    u_i     = (z_i + z_b / 2) brought into [0, L)
    c_i     = min(int(u_i), S - 1)
    n_c     = number of particles with c_i = c
    occ[n]  = number of sites with min(n_c, P - 1) = n,   n = 0 .. P-1
    corr[d] = sum_c n_c n_{(c + d) mod S},                 d = 0 .. D-1

and the row is R = [occ | corr].  A block is a list of time steps; step t is
`(confs, cloning_ref, num_walkers)` as in tests/_pairdist_fw_restatement.py:

    mixed   iter[t][j] = sum_{s live} R_s[j]
    pure    aux_t[s][j] = aux_{t-1}[cloning_ref_t[s]][j] + (t < pfw ? R_s[j] : 0)
            iter[t][j] = sum_{s live} aux_t[s][j] / min(t + 1, pfw)

with aux = 0 before the first step of the block.  Everything is an integer
until the one division, so the rows do not depend on the order of the sums.
The only freedom is a particle at a site boundary: u within 1e-9 of an integer
(0 and L included) is listed as ambiguous.
"""
import numpy as np

EDGE = 1e-9


def half_barrier(lattice_ratio):
    """z_b / 2 with z_b = 1 - z_a, z_a = 1 / (1 + ratio), formed as the
    library forms it."""
    return 0.5 * (1.0 - 1.0 / (1.0 + float(lattice_ratio)))


def step_positions(confs):
    """confs[W, N] or a State's confs[W, 2, N] -> pos[W, N]."""
    confs = np.asarray(confs, dtype=np.float64)
    return confs[:, 0, :] if confs.ndim == 3 else confs


def shifted(pos, sc_size, half_zb):
    """u[W, N] in [0, L] (L itself where a tiny negative value rounds up)."""
    return np.mod(np.asarray(pos, dtype=np.float64) + half_zb, float(sc_size))


def site_counts(pos, sc_size, half_zb):
    """n[W, S], int64."""
    S = int(sc_size)
    assert S == sc_size, 'the supercell must hold a whole number of sites'
    sites = np.minimum(shifted(pos, sc_size, half_zb).astype(np.int64), S - 1)
    n = np.zeros((len(sites), S), dtype=np.int64)
    for w, row in enumerate(sites):
        n[w] = np.bincount(row, minlength=S)
    return n


def site_rows(pos, sc_size, half_zb, num_occ, num_dist):
    """R[W, P + D], int64."""
    P, D = int(num_occ), int(num_dist)
    n = site_counts(pos, sc_size, half_zb)
    rows = np.zeros((len(n), P + D), dtype=np.int64)
    capped = np.minimum(n, P - 1)
    for k in range(P):
        rows[:, k] = (capped == k).sum(axis=1)
    for d in range(D):
        rows[:, P + d] = (n * np.roll(n, -d, axis=1)).sum(axis=1)
    return rows


def ambiguous_particles(pos, sc_size, half_zb):
    """-> [(walker, particle)] with u within EDGE of an integer."""
    u = shifted(pos, sc_size, half_zb)
    return [(int(w), int(i)) for w, i in
            np.argwhere(np.abs(u - np.rint(u)) < EDGE)]


def forward_walk(steps, sc_size, half_zb, num_occ, num_dist, pfw):
    """-> (mixed[T, K], pure[T, K], ambiguous): the per-step rows of both
    estimators and the particles met at a site boundary, a list of
    (t, walker, particle)."""
    T, K = len(steps), int(num_occ) + int(num_dist)
    mixed, pure = np.zeros((T, K)), np.zeros((T, K))
    ambiguous = []
    aux_prev = None
    for t, (confs, ref, nw) in enumerate(steps):
        nw = int(nw)
        pos = step_positions(confs)[:nw]
        ref = np.asarray(ref, dtype=np.int64)[:nw]
        R = site_rows(pos, sc_size, half_zb, num_occ, num_dist)
        ambiguous += [(t, w, i) for w, i in
                      ambiguous_particles(pos, sc_size, half_zb)]
        mixed[t] = R.sum(axis=0)
        aux = np.zeros((nw, K), dtype=np.int64)
        if aux_prev is not None:
            assert ref.max(initial=-1) < len(aux_prev), \
                'a walker descends from a slot that was not live'
            aux = aux_prev[ref].copy()
        if t < pfw:
            aux += R
        pure[t] = aux.sum(axis=0) / float(min(t + 1, pfw))
        aux_prev = aux
    return mixed, pure, ambiguous
