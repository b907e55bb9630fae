"""Cost of the three-body distribution next to the pair distribution, on the
same resident rows in one process (development tool).
usage: triple_dist_cost.py [--shapes 64:65536,128:65536] [--bins 64]
                           [--reps 5] [--warm 1] [--inner 4] [--out FILE]

The ensemble is in the stationary state of the VMC chain (tools/_stationary.py).
Per shape and per max_span in (L/2, L/8), the engine timer (events on the
stream) around `inner` back-to-back calls of
  qmc_pair_dist_reduce_dev    (g2, num_bins bins)
  qmc_triple_dist_reduce_dev  (g3, num_bins bins + overflow)
alternating the two, `warm` untimed calls of each first, median of `reps`:
milliseconds per call, the spread (max - min) / median, and the ratio g3 / g2.
No ratio is asserted; the row sums are (N (N - 1) / 2 and C(N,3) per row)."""
import argparse
import os
import sys
from math import comb, pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _stationary import replicate, seed_configurations  # noqa: E402
from phd_qmclib_amd.engine import DeviceBuffer, ModelEngine, VmcEnsemble  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='64:65536,128:65536')
ap.add_argument('--bins', type=int, default=64)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--warm', type=int, default=1)
ap.add_argument('--inner', type=int, default=4)
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


B = a.bins
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
    v.run_block(100, sums=False)
    eng.sync()
    pos_dev, _ = v.state_dev()
    s2 = DeviceBuffer((B, 2), eng.device)
    s3 = DeviceBuffer((B + 1, 2), eng.device)
    for frac in (0.5, 0.125):
        D = frac * n

        def g2():
            eng.pair_distribution_reduce_dev(W, pos_dev, None, B, s2.ptr)

        def g3():
            eng.triple_distribution_reduce_dev(W, pos_dev, None, B, D, s3.ptr)

        for _ in range(a.warm):
            g2()
            g3()
        t2, t3 = [], []
        for _ in range(a.reps):
            t2.append(timed(eng, g2))
            t3.append(timed(eng, g3))
        assert s2.download()[:, 0].sum() == W * (n * (n - 1) // 2)
        assert s3.download()[:, 0].sum() == W * comb(n, 3)
        m2, sp2 = stat(t2)
        m3, sp3 = stat(t3)
        say(f'N={n} W={W} B={B} max_span=L*{frac}: g2 {m2:8.3f} ms (spread '
            f'{sp2:.3f})  g3 {m3:8.3f} ms (spread {sp3:.3f})  g3/g2 '
            f'{m3 / m2:.2f}')
    for b in (s2, s3):
        b.close()
    v.close()
    eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
