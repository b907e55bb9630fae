"""NumPy forward walking of the pair-distance histogram: the DMC block
estimator of g2(r), restated from its definition.

A block is a list of time steps; step t is `(confs, cloning_ref, num_walkers)`:
the positions `confs[s]` that walker s carries (the configuration of its
parent), the cloning table `cloning_ref[s]` (the slot of that parent in the
population of step t - 1) and the number of live walkers nw_t.  Walker s is
live if s < nw_t.  With H_s the histogram of tests/_pairdist_restatement.py,

    mixed   iter[t][b] = sum_{s live} H_s[b]
    pure    aux_t[s][b] = aux_{t-1}[cloning_ref_t[s]][b] + (t < pfw ? H_s[b] : 0)
            iter[t][b] = sum_{s live} aux_t[s][b] / min(t + 1, pfw)

with aux = 0 before the first step of the block.  Everything is an integer
until the one division, so the rows do not depend on the order of the sums.
"""
import numpy as np

from . import _pairdist_restatement as pdr


def step_positions(confs):
    """confs[W, N] or a State's confs[W, 2, N] -> pos[W, N]."""
    confs = np.asarray(confs, dtype=np.float64)
    return confs[:, 0, :] if confs.ndim == 3 else confs


def forward_walk(steps, sc_size, num_bins, pfw):
    """-> (mixed[T, B], pure[T, B], ambiguous): the per-step rows of both
    estimators and the edge-ambiguous pairs met, a list of (t, s, i, j, edge)
    (r / delta within 1e-9 of an integer, or a pair at the image switch)."""
    T, B = len(steps), int(num_bins)
    mixed, pure = np.zeros((T, B)), np.zeros((T, B))
    ambiguous = []
    aux_prev = None
    for t, (confs, ref, nw) in enumerate(steps):
        nw = int(nw)
        pos = step_positions(confs)[:nw]
        ref = np.asarray(ref, dtype=np.int64)[:nw]
        H = pdr.pair_counts(pos, sc_size, B)                  # int64 [nw, B]
        for s, amb in enumerate(pdr.ambiguous_pairs(pos, sc_size, B)):
            ambiguous += [(t, s, int(i), int(j), int(e)) for i, j, e in amb]
        mixed[t] = H.sum(axis=0)
        aux = np.zeros((nw, B), dtype=np.int64)
        if aux_prev is not None:
            assert ref.max(initial=-1) < len(aux_prev), \
                'a walker descends from a slot that was not live'
            aux = aux_prev[ref].copy()
        if t < pfw:
            aux += H
        pure[t] = aux.sum(axis=0) / float(min(t + 1, pfw))
        aux_prev = aux
    return mixed, pure, ambiguous
