"""Cost of the DMC site occupation estimator at the DMC benchmark shape, next
to the same block without it and to the g2(r) estimator, in one process
(development tool).
usage: site_est_bench.py [--bosons N] [--walkers W] [--steps K] [--occ P]
                         [--dist D] [--pair-bins B] [--reps R] [--relax S]
                         [--out FILE]

One population of W walkers is relaxed for S time steps.  Then estimator
blocks of K steps are timed with the engine's event pair, each configuration
after a warm-up block of its own, the configurations taking turns R times:
  off        no estimator (the plain block)
  site       the site estimator, pure over the block, P occupation bins and
             D distances
  site_mixed the same, mixed
  g2         the pair distribution at B bins, pure over the block
The median per configuration and (max - min) / median are printed, and the
ratios to `off`."""
import argparse
import json
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--bosons', type=int, default=64)
ap.add_argument('--walkers', type=int, default=1 << 18)
ap.add_argument('--steps', type=int, default=128)
ap.add_argument('--occ', type=int, default=8)
ap.add_argument('--dist', type=int, default=33)
ap.add_argument('--pair-bins', type=int, default=64)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--relax', type=int, default=128)
ap.add_argument('--out', default=None)
a = ap.parse_args()
n, W, K = a.bosons, a.walkers, a.steps
spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1, interaction_strength=2,
            boson_number=n, supercell_size=n, tbf_contact_cutoff=0.25 * n)
eng = ModelEngine(spec.cfc_spec, device=0)
maxw = ((W * 512 // 480) + 255) // 256 * 256
d = DmcEnsemble(eng, 6.25e-4, maxw, W, 0.5, rng_seed=1)
d.set_state(n * np.random.RandomState(1).random_sample((W, n)))
d.run_block(a.relax, read=False)
eng.sync()


def configure(name):
    d.set_site_estimator(0)
    d.set_pair_dist_estimator(0)
    if name == 'site':
        d.set_site_estimator(a.occ, a.dist, pure=True, pfw=K)
    elif name == 'site_mixed':
        d.set_site_estimator(a.occ, a.dist)
    elif name == 'g2':
        d.set_pair_dist_estimator(a.pair_bins, pure=True, pfw=K)


names = ('off', 'site', 'site_mixed', 'g2')
ms = {name: [] for name in names}
for _ in range(a.reps):
    for name in names:
        configure(name)
        d.run_block_est(K)              # warm-up (and the buffers' first use)
        eng.sync()
        eng.timer_start()
        d.run_block_est(K)
        ms[name].append(eng.timer_stop())
res = dict(bosons=n, walkers=d.num_walkers(), steps=K, occ=a.occ, dist=a.dist,
           pair_bins=a.pair_bins)
for name in names:
    med = float(np.median(ms[name]))
    res[name] = dict(median_ms=med, ms=ms[name],
                     spread=(max(ms[name]) - min(ms[name])) / med)
    print(f'N={n} W={W} {K} steps {name:10s} {med:9.3f} ms  spread '
          f'{res[name]["spread"]:.3f}  over off '
          f'{med / float(np.median(ms["off"])):.4f}', flush=True)
if a.out:
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
d.close()
eng.close()
