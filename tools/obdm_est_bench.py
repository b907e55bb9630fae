"""Cost of the DMC g1(s) estimator launch next to the batch g1 path on the same
walkers, in one process (development tool).
usage: obdm_est_bench.py [--bosons N] [--walkers W] [--shifts K] [--reps R]
                         [--relax S] [--out FILE]

A population of W walkers is relaxed for S time steps.  Then, on the yielded
walkers of the last step:
  estimator  one `qmc_dmc_step_estimators` call with only g1 set: the
             dmc_obdm_kernel launch over the nw walkers and its block
             reduction (est_reduce_kernel)
  batch      `one_body_density_dev` on a device buffer holding the same nw
             configurations and the same K shifts (shift table + obdm_kernel)
  step       a plain DMC time step (run_block of `--block` steps over their
             number), for scale
Each is timed R times with the engine's event pair after warm-up calls; the
median and (max - min) / median are printed, and the ratio estimator / batch."""
import argparse
import json
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phd_qmclib_amd.engine import DeviceBuffer, DmcEnsemble, ModelEngine  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--bosons', type=int, default=64)
ap.add_argument('--walkers', type=int, default=1 << 16)
ap.add_argument('--shifts', type=int, default=16)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--warm', type=int, default=3)
ap.add_argument('--relax', type=int, default=64)
ap.add_argument('--block', type=int, default=16)
ap.add_argument('--out', default=None)
a = ap.parse_args()
n, W, K = a.bosons, a.walkers, a.shifts
spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1, interaction_strength=2,
            boson_number=n, supercell_size=n, tbf_contact_cutoff=0.25 * n)
eng = ModelEngine(spec.cfc_spec, device=0)
shifts = 0.5 * n * np.arange(K) / K
d = DmcEnsemble(eng, 1e-3, W + W // 4, W, 0.5, rng_seed=3)
d.set_state(n * np.random.RandomState(3).random_sample((W, n)))
d.run_block(a.relax)


def timed(call):
    for _ in range(a.warm):
        call()
    eng.sync()
    ts = []
    for _ in range(a.reps):
        eng.timer_start()
        call()
        ts.append(eng.timer_stop())
    med = float(np.median(ts))
    return dict(median_ms=med, spread=(max(ts) - min(ts)) / med, ms=ts)


step = timed(lambda: d.run_block(a.block, read=False))
for key in ('median_ms',):
    step[key] /= a.block
step['ms'] = [x / a.block for x in step['ms']]

state = d.get_state()
nw = int(state.num_walkers)
d.set_obdm_estimator(shifts)
d.est_begin_block(a.warm + a.reps)
calls = iter(range(a.warm + a.reps))
est = timed(lambda: d.step_estimators(next(calls)))
rows = d.read_obdm(a.warm + a.reps)

pos = DeviceBuffer((nw, n), eng.device).upload(state.confs[:nw, 0, :])
sh = DeviceBuffer((K,), eng.device).upload(shifts)
g1 = DeviceBuffer((nw, K), eng.device)
batch = timed(lambda: eng.one_body_density_dev(nw, pos.ptr, K, sh.ptr, g1.ptr))
# the two paths agree on what they computed
total = g1.download().sum(axis=0)
assert np.allclose(rows[-1], total, rtol=1e-12), (rows[-1], total)
assert rows[-1][0] == nw

res = dict(bosons=n, walkers=nw, shifts=K, estimator=est, batch=batch,
           step=step, ratio=est['median_ms'] / batch['median_ms'])
for name in ('estimator', 'batch', 'step'):
    r = res[name]
    print(f'N={n} nw={nw} K={K} {name:9s} {r["median_ms"]:9.3f} ms  '
          f'spread {r["spread"]:.3f}', flush=True)
print(f'estimator / batch = {res["ratio"]:.3f}', flush=True)
if a.out:
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
for b in (pos, sh, g1):
    b.close()
d.close()
eng.close()
