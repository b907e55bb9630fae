#!/usr/bin/env python3
"""Generate tests/golden/obdm.npz: the reference's one-body density matrix on
the golden configurations.

TEST INFRASTRUCTURE ONLY.  It runs only where the reference (PhD-QMCLib) is
installed, under the interpreter and the import harness that
oracle/refgen/gen_golden.py uses (the harness is imported unchanged):

    MPLBACKEND=Agg python3.9 tools/gen_obdm_golden.py

Inputs: the positions committed in tests/golden/kernels.npz and the specs in
tests/golden/params.json.  Output, per tag: `shifts`, `g1[conf][shift]`
(core_funcs.one_body_density) and, for N <= 64, `ith[conf][shift][N]`
(core_funcs.ith_one_body_density).  Only data is stored.

Shift set per tag (L the supercell size), 14 values:
    0, +0.013, -0.013, 1, -L/2 ... L/2 in nine steps, L, 1.37 L
The reference runs as plain Python and costs O(N^2) per value: every
configuration up to N = 128; two configurations and the first six shifts at
N = 512.
"""
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                     '..'))
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refgen'))

import harness  # noqa: F401,E402  (must precede phd_qmclib imports)
import numpy as np  # noqa: E402

from phd_qmclib import mrbp_qmc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
core = mrbp_qmc.model.core_funcs


def shift_set(sc_size):
    return np.concatenate([[0.0, 0.013, -0.013, 1.0],
                           np.linspace(-0.5 * sc_size, 0.5 * sc_size, 9),
                           [sc_size, 1.37 * sc_size]])


def main():
    with open(os.path.join(GOLDEN, 'params.json')) as fp:
        params = json.load(fp)
    kernels = np.load(os.path.join(GOLDEN, 'kernels.npz'))
    out = {}
    for tag in sorted(params):
        spec = mrbp_qmc.Spec(**params[tag]['spec'])
        cfc = spec.cfc_spec
        n = spec.boson_number
        pos = kernels[tag + '/pos']
        shifts = shift_set(float(spec.supercell_size))
        if n >= 512:
            pos, shifts = pos[:2], shifts[:6]
        g1 = np.zeros((len(pos), len(shifts)))
        ith = np.zeros((len(pos), len(shifts), n)) if n <= 64 else None
        for c, row in enumerate(pos):
            sys_conf = np.zeros((2, n))
            sys_conf[0] = row
            for k, sz in enumerate(shifts):
                g1[c, k] = core.one_body_density(float(sz), sys_conf, *cfc)
                if ith is not None:
                    for i in range(n):
                        ith[c, k, i] = core.ith_one_body_density(
                            i, float(sz), sys_conf, *cfc)
        assert np.all(np.isfinite(g1))
        out[tag + '/shifts'] = shifts
        out[tag + '/g1'] = g1
        if ith is not None:
            assert np.all(np.isfinite(ith))
            assert np.allclose(ith.mean(axis=2), g1, rtol=1e-12, atol=0)
            out[tag + '/ith'] = ith
        print('obdm', tag, g1.shape, g1[0, :4], flush=True)
    np.savez_compressed(os.path.join(GOLDEN, 'obdm.npz'), **out)


if __name__ == '__main__':
    main()
