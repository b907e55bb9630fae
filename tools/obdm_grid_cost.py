"""Cost of the one-body density matrix on a grid (natural orbitals, condensate
fraction) next to g1(s), on the same resident chains in one process, and the
cross-check of its purity against the one-particle replica swap on a model
without a lattice (development tool).
usage: obdm_grid_cost.py [--shapes 64:65536,128:65536] [--points 64,256]
                         [--groups 32] [--shifts 16] [--reps 5] [--warm 1]
                         [--inner 2] [--check 16:8192] [--check-points 64]
                         [--snaps 8] [--out FILE]

Cost.  The ensemble is in the stationary state of the VMC chain
(tools/_stationary.py).  Per shape and per M of --points, the engine timer
(events on the stream) around `inner` back-to-back calls of
  qmc_vmc_obdm       (g1 at K shifts s_k = (L/2) (k + 1) / K)
  qmc_vmc_obdm_grid  (M x M cells, G groups)
alternating the two, `warm` untimed calls of each first, median of `reps`
windows: milliseconds per call, the spread (max - min) / median, the ratio
grid / g1 next to the arithmetic ratio M / K, and the time per pair factor of
both kernels, ms / (W M N (N - 1)) and ms / (W K N (N - 1)).  The grid call
includes the download of its G M^2 sums, the g1 call that of its 2 K.  No
ratio is asserted; g1(s) > 0 and Tr K > 0 are.

Cross-check.  N:W names a model of the free family (no lattice, g = 4, L = N)
and W chains started independently, the model of line 3 of
profiles/particle_entropy_cost.txt.  Over `snaps` snapshots 400 steps apart
the tool adds up the grid sums (M = --check-points, G = --groups) and the
one-particle swap sums of the same chains and prints n0 / N, the cross-group
purity of K and the swap purity with their errors, the difference of the two
purities in units of the combined error, and the bracket
[purity, sqrt(purity)] of the swap with n0 / N next to it.  Both errors treat
the snapshots as independent."""
import argparse
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _stationary import replicate, seed_configurations  # noqa: E402
from phd_qmclib_amd.engine import (ModelEngine, VmcEnsemble,  # noqa: E402
                                   natural_orbitals, particle_entropy)
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='64:65536,128:65536')
ap.add_argument('--points', default='64,256')
ap.add_argument('--groups', type=int, default=32)
ap.add_argument('--shifts', type=int, default=16)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--warm', type=int, default=1)
ap.add_argument('--inner', type=int, default=2)
ap.add_argument('--check', default='16:8192')
ap.add_argument('--check-points', type=int, default=64)
ap.add_argument('--snaps', type=int, default=8)
ap.add_argument('--out', default=None)
a = ap.parse_args()
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def timed(eng, call):
    eng.timer_start()
    for _ in range(a.inner):
        call()
    return eng.timer_stop() / a.inner


def stat(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


K, G = a.shifts, a.groups
for shape in [s for s in a.shapes.split(',') if s]:
    n, W = (int(x) for x in shape.split(':'))
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=n, supercell_size=n,
                tbf_contact_cutoff=0.25 * n)
    eng = ModelEngine(spec.cfc_spec, device=0)
    pos = replicate(seed_configurations(eng, spec, n, seeds=2048, steps=20000),
                    W)
    v = VmcEnsemble(eng, W, 0.25 * spec.well_width, rng_seed=1)
    v.set_state(pos)
    v.run_block(100, sums=False)
    eng.sync()
    shifts = 0.5 * n * (np.arange(K) + 1.0) / K
    for M in [int(x) for x in a.points.split(',') if x]:
        out = {}

        def g1():
            out['g1'] = v.obdm_parts(shifts)

        def grid():
            out['grid'] = v.obdm_grid_parts(M, G)

        for _ in range(a.warm):
            g1()
            grid()
        t1, t2 = [], []
        for _ in range(a.reps):
            t1.append(timed(eng, g1))
            t2.append(timed(eng, grid))
        assert np.all(out['g1'][:, 0] > 0)
        trace = float(np.trace(out['grid'].sum(axis=0))) / W
        assert trace > 0.0
        m1, sp1 = stat(t1)
        m2, sp2 = stat(t2)
        pairs = float(W) * n * (n - 1)
        say(f'N={n} W={W} K={K} M={M} G={G}: g1 {m1:8.3f} ms (spread '
            f'{sp1:.3f})  grid {m2:9.3f} ms (spread {sp2:.3f})  grid/g1 '
            f'{m2 / m1:6.2f} (M/K = {M / K:.0f})  per pair factor: g1 '
            f'{1e9 * m1 / (pairs * K):.4f} ps  grid '
            f'{1e9 * m2 / (pairs * M):.4f} ps  Tr K = {trace:.3f}')
    v.close()
    eng.close()

if a.check:
    n, W = (int(x) for x in a.check.split(':'))
    M = a.check_points
    spec = Spec(lattice_depth=0, lattice_ratio=1, interaction_strength=4,
                boson_number=n, supercell_size=n, tbf_contact_cutoff=0.25 * n)
    eng = ModelEngine(spec.cfc_spec, device=0)
    spread = 0.5
    pos = seed_configurations(eng, spec, n, seeds=W, steps=20000,
                              spread=spread)
    v = VmcEnsemble(eng, W, spread, rng_seed=1)
    v.set_state(pos)
    sw, sums = np.zeros(3), np.zeros((G, M, M))
    for _ in range(a.snaps):
        for _ in range(4):
            v.run_block(100, sums=False)
        sw += v.particle_swap_parts()
        sums += v.obdm_grid_parts(M, G)
    wsum = a.snaps * np.array([len(range(g, W, G)) for g in range(G)],
                              dtype=np.float64)
    res = natural_orbitals(sums, wsum, n, float(n))
    _, _, purity, purity_err = particle_entropy(sw, int(sw[2]))
    comb = float(np.hypot(purity_err, res.purity_err))
    lo, hi = purity, float(np.sqrt(purity))
    inside = lo <= res.condensate_fraction <= hi
    say(f'cross-check, no lattice, N={n} L={n} g=4, {W} chains x '
        f'{a.snaps} snapshots, M={M} G={G}: n0/N {res.condensate_fraction:.5f}'
        f' +- {res.condensate_fraction_err:.5f}  purity of K '
        f'{res.purity:.6f} +- {res.purity_err:.6f}  swap purity '
        f'{purity:.6f} +- {purity_err:.6f}  difference '
        f'{(res.purity - purity) / comb:+.2f} combined errors;  Tr K = '
        f'{res.trace:.4f};  bracket [{lo:.4f}, {hi:.4f}], n0/N '
        f'{"inside" if inside else "OUTSIDE"}')
    v.close()
    eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
