"""Cost of the two-segment replica-swap estimator and its charge-resolved
reduction next to the one-segment kernel, on the same resident chains in one
process (development tool).
usage: renyi_region_cost.py [--shapes 64:65536,128:65536] [--regions 16]
                            [--reps 5] [--warm 1] [--inner 4] [--out FILE]

The ensemble is in the stationary state of the VMC chain (tools/_stationary.py).
Per shape, the engine timer (events on the stream) around `inner` back-to-back
calls of
  old      qmc_vmc_renyi_swap at the K lengths l_k = L (k + 1) / (K + 1)
  single   qmc_vmc_renyi_region_swap at the regions (l_k, 0, 0), no charges
  two      the same at the regions (l_k / 2, L / (2 K + 2), l_k / 2): the same
           total length in two windows
  charges  `two` with every charge collected (Q = N + 1)
with the cut in mid-barrier, the four alternating, `warm` untimed calls of
each first, median of `reps`: milliseconds per call, the spread
(max - min) / median, the ratios to `old`, and the fraction of matched
entries of `single` and `two` (only those reach the pair loop).  No ratio is
asserted; that `single` matches where `old` does and that the resolved sums
add up are."""
import argparse
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _stationary import replicate, seed_configurations  # noqa: E402
from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='64:65536,128:65536')
ap.add_argument('--regions', type=int, default=16)
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


K = a.regions
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
    lengths = float(n) * (np.arange(K) + 1.0) / (K + 1)
    zero = np.zeros(K)
    single = np.stack([lengths, zero, zero], axis=1)
    two = np.stack([0.5 * lengths, zero + 0.5 * n / (K + 1), 0.5 * lengths],
                   axis=1)
    origin = -0.5 * spec.barrier_width
    out = {}
    calls = {
        'old': lambda: v.renyi_parts(lengths, origin),
        'single': lambda: v.renyi_region_parts(single, origin, 0),
        'two': lambda: v.renyi_region_parts(two, origin, 0),
        'charges': lambda: v.renyi_region_parts(two, origin, n + 1),
    }
    for _ in range(a.warm):
        for name, call in calls.items():
            out[name] = call()
    times = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, call in calls.items():
            times[name].append(timed(eng, call))
    assert np.array_equal(out['single'][:, 2], out['old'][:, 2])
    assert np.allclose(out['single'][:, :2], out['old'][:, :2], rtol=1e-11,
                       atol=0)
    assert np.array_equal(out['charges'][:, :3], out['two'])
    assert np.array_equal(out['charges'][:, 4::2].sum(axis=1),
                          np.full(K, float(W)))
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    spread = {name: (max(ts) - min(ts)) / med[name]
              for name, ts in times.items()}
    pairs = K * (W // 2)
    say(f'N={n} W={W} K={K}: '
        + '  '.join(f'{name} {med[name]:8.3f} ms (spread {spread[name]:.3f})'
                    for name in calls))
    say(f'N={n} W={W} K={K}: '
        + '  '.join(f'{name}/old {med[name] / med["old"]:.2f}'
                    for name in ('single', 'two', 'charges'))
        + f'  matched single {out["single"][:, 2].sum() / pairs:.3f}'
        + f' two {out["two"][:, 2].sum() / pairs:.3f}')
    v.close()
    eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
