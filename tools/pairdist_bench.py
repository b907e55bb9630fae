"""Throughput of the pair distribution kernel next to the log|psi|-only
evaluation, on the same resident rows in one process (development tool).
usage: pairdist_bench.py [--shapes 64:1048576,128:262144] [--bins 64,1024]
                         [--reps R] [--warm K]

The ensemble is in the stationary state of the VMC chain (tools/_stationary.py).
Reported per shape, median of R timed calls that follow K warm-up calls with no
idle gap (the chip runs slower for the first launches after an upload; the timed
calls are enqueued back to back and each is bracketed by events on the stream):
  qmc_pair_dist_reduce_dev  W N (N - 1) / 2 pairs per second per bin count
  qmc_evaluate_dev          W N (N - 1) / 2 pairs per second, log|psi| alone
and the ratio of the two rates."""
import argparse
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _stationary import replicate, seed_configurations  # noqa: E402
from phd_qmclib_amd.engine import DeviceBuffer, ModelEngine, VmcEnsemble  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='64:1048576,128:262144')
ap.add_argument('--bins', default='64,1024')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--warm', type=int, default=3)
a = ap.parse_args()


def median_ms(eng, call):
    for _ in range(a.warm):
        call()
    ts = []
    for _ in range(a.reps):
        eng.timer_start()
        call()
        ts.append(eng.timer_stop())
    return float(np.median(ts)), (max(ts) - min(ts)) / float(np.median(ts))


for shape in a.shapes.split(','):
    n, W = (int(x) for x in shape.split(':'))
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=n, supercell_size=n,
                tbf_contact_cutoff=0.25 * n)
    eng = ModelEngine(spec.cfc_spec, device=0)
    pos = replicate(seed_configurations(eng, spec, n, seeds=2048, steps=20000),
                    W)
    v = VmcEnsemble(eng, W, 0.25 * spec.well_width, rng_seed=1)
    v.set_state(pos)
    v.run_block(300, sums=False)
    eng.sync()
    pos_dev, _ = v.state_dev()
    wf = DeviceBuffer((W,), eng.device)
    pairs = W * n * (n - 1) / 2
    ms, spread = median_ms(eng, lambda: eng.evaluate_dev(W, pos_dev, wf.ptr))
    rate_wf = pairs / (ms * 1e-3)
    print(f'N={n} W={W} log|psi| only      {ms:9.3f} ms  {rate_wf:.3e} pairs/s  '
          f'spread {spread:.3f}', flush=True)
    for B in [int(x) for x in a.bins.split(',')]:
        sums = DeviceBuffer((B, 2), eng.device)
        ms, spread = median_ms(eng, lambda: eng.pair_distribution_reduce_dev(
            W, pos_dev, None, B, sums.ptr))
        rate = pairs / (ms * 1e-3)
        total = sums.download()[:, 0].sum()
        assert total == pairs, (total, pairs)
        print(f'N={n} W={W} pair_dist B={B:4d}   {ms:9.3f} ms  {rate:.3e} '
              f'pairs/s  spread {spread:.3f}  ratio to log|psi| '
              f'{rate / rate_wf:.3f}', flush=True)
        sums.close()
    wf.close()
    v.close()
    eng.close()
