"""Throughput of the one-body density matrix kernel next to the log|psi|-only
evaluation, on the same resident rows in one process (development tool).
usage: obdm_bench.py [--bosons N] [--chains W] [--shifts 16,64] [--reps R]

The ensemble is in the stationary state of the VMC chain (tools/_stationary.py).
Reported per case, median of R timed calls after warm-up calls (the chip runs
slower for the first launches after an upload):
  qmc_vmc_obdm      W M N (N - 1) shifted pair factors per second
  qmc_evaluate_dev  W N (N - 1) / 2 pair factors per second, log|psi| alone
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
ap.add_argument('--bosons', type=int, default=64)
ap.add_argument('--chains', type=int, default=1 << 18)
ap.add_argument('--shifts', default='16,64')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--warm', type=int, default=3)
a = ap.parse_args()
n, W = a.bosons, a.chains
spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1, interaction_strength=2,
            boson_number=n, supercell_size=n, tbf_contact_cutoff=0.25 * n)
eng = ModelEngine(spec.cfc_spec, device=0)
pos = replicate(seed_configurations(eng, spec, n, seeds=2048, steps=20000), W)
v = VmcEnsemble(eng, W, 0.25 * spec.well_width, rng_seed=1)
v.set_state(pos)
v.run_block(300, sums=False)
eng.sync()


def median_ms(call):
    for _ in range(a.warm):
        call()
    eng.sync()
    ts = []
    for _ in range(a.reps):
        eng.timer_start()
        call()
        ts.append(eng.timer_stop())
    return float(np.median(ts)), (max(ts) - min(ts)) / float(np.median(ts))


pos_dev, _ = v.state_dev()
wf = DeviceBuffer((W,), eng.device)
ms, spread = median_ms(lambda: eng.evaluate_dev(W, pos_dev, wf.ptr))
rate_wf = W * n * (n - 1) / 2 / (ms * 1e-3)
print(f'N={n} W={W} log|psi| only   {ms:9.3f} ms  {rate_wf:.3e} pairs/s  '
      f'spread {spread:.3f}', flush=True)
for M in [int(x) for x in a.shifts.split(',')]:
    shifts = 0.5 * n * (np.arange(M) + 0.5) / M
    ms, spread = median_ms(lambda: v.obdm_parts(shifts))
    rate = W * M * n * (n - 1) / (ms * 1e-3)
    print(f'N={n} W={W} obdm M={M:3d}      {ms:9.3f} ms  {rate:.3e} pair '
          f'factors/s  spread {spread:.3f}  ratio to log|psi| '
          f'{rate / rate_wf:.3f}', flush=True)
wf.close()
v.close()
eng.close()
