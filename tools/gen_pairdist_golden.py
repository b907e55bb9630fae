#!/usr/bin/env python3
"""Generate tests/golden/pair_dist.npz: the reference's pair distances on the
golden configurations.

TEST INFRASTRUCTURE ONLY.  It runs only where the reference (PhD-QMCLib) is
installed, under the interpreter and the import harness that
oracle/refgen/gen_golden.py uses (the harness is imported unchanged):

    MPLBACKEND=Agg python3.9 tools/gen_pairdist_golden.py

Inputs: the positions committed in tests/golden/kernels.npz and the specs in
tests/golden/params.json.  The reference has no pair distribution function; what
it owns is the distance, `core_funcs.real_distance(z_i, z_j, model_params)`
(mrbp_qmc/model.py:555-562 -> qmc_base/utils.py:35-51).  Output, per tag:

  `dist`    [conf][N (N - 1) / 2]  real_distance(z_i, z_j) of the pairs i < j in
            the row-major order of numpy.triu_indices(N, 1): the upper triangle
            of the distance matrix (the lower one is its mirror image and the
            diagonal is zero; the whole matrices of the fifteen tags would be
            16 MB).  Every configuration up to N = 64; the first two for
            100 <= N <= 128, where more would push the file past the size
            limit for a committed file; none at N = 512.
  `counts`  [conf][1 + 7 + 64 + 1000]  for EVERY configuration the histograms
            min(int(|d| // bin_size), B - 1), bin_size = (L/2) / B, for
            B = 1, 7, 64, 1000 one after the other, derived from those
            reference distances in plain Python.

Only data is stored.
"""
import json
import os
import sys
from math import fabs

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                     '..'))
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refgen'))

import harness  # noqa: F401,E402  (must precede phd_qmclib imports)
import numpy as np  # noqa: E402

from phd_qmclib import mrbp_qmc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
core = mrbp_qmc.model.core_funcs
BINS = (1, 7, 64, 1000)


def stored_confs(n, nconf):
    if n <= 64:
        return nconf
    return 2 if n <= 128 else 0


def main():
    with open(os.path.join(GOLDEN, 'params.json')) as fp:
        params = json.load(fp)
    kernels = np.load(os.path.join(GOLDEN, 'kernels.npz'))
    out = {}
    for tag in sorted(params):
        spec = mrbp_qmc.Spec(**params[tag]['spec'])
        model_params = spec.cfc_spec.model_params
        n = spec.boson_number
        sc_size = float(spec.supercell_size)
        pos = kernels[tag + '/pos']
        iu, ju = np.triu_indices(n, 1)
        keep = stored_confs(n, len(pos))
        dist = np.zeros((keep, len(iu)))
        counts = np.zeros((len(pos), sum(BINS)), dtype=np.uint32)
        for c, row in enumerate(pos):
            d = np.array([core.real_distance(float(row[i]), float(row[j]),
                                             model_params)
                          for i, j in zip(iu, ju)])
            if c < keep:
                dist[c] = d
            off = 0
            for nb in BINS:
                bin_size = (0.5 * sc_size) / nb
                for v in d:
                    b = min(int(fabs(v) // bin_size), nb - 1)
                    counts[c, off + b] += 1
                off += nb
        assert np.all(np.isfinite(dist))
        assert np.all(np.abs(dist) <= 0.5 * sc_size)
        out[tag + '/dist'] = dist
        out[tag + '/counts'] = counts
        print('pair_dist', tag, dist.shape, counts.shape, flush=True)
    np.savez_compressed(os.path.join(GOLDEN, 'pair_dist.npz'), **out)


if __name__ == '__main__':
    main()
