"""Cost of the DMC estimators next to the plain time step (development tool).
usage: est_bench.py [--bosons N] [--walkers W] [--steps K] [--modes M] [--bins B]
                    [--pair-bins P] [--repeats R] [--relax S] [--isf K,T,q]
                    [--only plain,g2]
(groups: plain, ssf, density, g2 = g2mixed + g2pure, cm, isf)
Every line is the median over R timed blocks of K steps (after a warm-up
block and, with --relax, S more untimed steps that bring the population from
its random start to the stationary state), with the shortest and the longest
next to it."""
import argparse
import os
import sys
import time
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine  # noqa
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa

ap = argparse.ArgumentParser()
ap.add_argument('--bosons', type=int, default=64)
ap.add_argument('--walkers', type=int, default=1 << 17)
ap.add_argument('--steps', type=int, default=16)
ap.add_argument('--modes', type=int, default=64)
ap.add_argument('--bins', type=int, default=128)
ap.add_argument('--pair-bins', type=int, default=64)
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--relax', type=int, default=0)
ap.add_argument('--isf', default='16,16,8',
                help='modes, lags, lag stride of the F(k, tau) estimator')
ap.add_argument('--only', default='plain,ssf,density,g2',
                help='comma-separated groups to time')
a = ap.parse_args()
n = a.bosons
spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1, interaction_strength=2,
            boson_number=n, supercell_size=n, tbf_contact_cutoff=0.25 * n)
eng = ModelEngine(spec.cfc_spec, device=0)
pos = n * np.random.RandomState(1).random_sample((a.walkers, n))
maxw = ((a.walkers * 512 // 480) + 255) // 256 * 256


def timed(tag, pair=None, cm=False, isf=None, **est):
    d = DmcEnsemble(eng, 6.25e-4, maxw, a.walkers, 0.5, rng_seed=1)
    d.set_state(pos)
    if est:
        d.set_estimators(**est)
    if pair:
        d.set_pair_dist_estimator(**pair)
    if cm:
        d.set_cm_diffusion_estimator()
    if isf:
        d.set_isf_estimator(*isf)
    if est or pair or cm or isf:
        run = lambda k: d.run_block_est(k, True)
    else:
        run = lambda k: d.run_block(k)
    run(a.steps)
    if a.relax:
        run(a.relax)
    eng.sync()
    ts = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        run(a.steps)
        eng.sync()
        ts.append((time.perf_counter() - t0) / a.steps * 1e3)
    print(f'{tag:28s} {np.median(ts):8.3f} ms/step  (min {min(ts):.3f}, '
          f'max {max(ts):.3f}, {a.repeats} x {a.steps} steps)', flush=True)
    d.close()
    return float(np.median(ts))


only = a.only.split(',')
if 'plain' in only:
    timed('plain')
if 'ssf' in only:
    timed(f'ssf mixed M={a.modes}', num_modes=a.modes)
    timed(f'ssf pure  M={a.modes}', num_modes=a.modes, ssf_pure=True,
          ssf_pfw=8)
if 'density' in only:
    timed(f'density mixed B={a.bins}', num_bins=a.bins)
    timed(f'density pure  B={a.bins}', num_bins=a.bins, dens_pure=True,
          dens_pfw=8)
if 'g2' in only or 'g2mixed' in only:
    timed(f'g2 mixed B={a.pair_bins}', pair=dict(num_bins=a.pair_bins))
if 'g2' in only or 'g2pure' in only:
    timed(f'g2 pure  B={a.pair_bins}',
          pair=dict(num_bins=a.pair_bins, pure=True, pfw=a.steps))
if 'cm' in only:
    timed('centre-of-mass diffusion', cm=True)
if 'isf' in only:
    timed(f'F(k, tau) K,T,q={a.isf}', isf=[int(v) for v in a.isf.split(',')])
if 'plain' in only:
    timed('plain (again)')
