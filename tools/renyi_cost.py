"""Cost of the replica-swap estimator of the Renyi-2 entropy next to the
one-body density matrix, on the same resident chains in one process
(development tool).
usage: renyi_cost.py [--shapes 64:65536,128:65536] [--lengths 16]
                     [--reps 5] [--warm 1] [--inner 4] [--out FILE]

The ensemble is in the stationary state of the VMC chain (tools/_stationary.py).
Per shape, the engine timer (events on the stream) around `inner` back-to-back
calls of
  qmc_vmc_obdm        (g1 at K shifts s_k = (L/2) (k + 1) / K)
  qmc_vmc_renyi_swap  (K segments l_k = L (k + 1) / (K + 1), the cut in
                       mid-barrier)
alternating the two, `warm` untimed calls of each first, median of `reps`:
milliseconds per call, the spread (max - min) / median, the ratio swap / g1,
and the fraction of the (pair, length) entries that matched (only those reach
the pair loop).  No ratio is asserted; g1(s) > 0 and the match counts are."""
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
ap.add_argument('--lengths', type=int, default=16)
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


K = a.lengths
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
    shifts = 0.5 * n * (np.arange(K) + 1.0) / K
    lengths = float(n) * (np.arange(K) + 1.0) / (K + 1)
    origin = -0.5 * spec.barrier_width
    out = {}

    def g1():
        out['g1'] = v.obdm_parts(shifts)

    def swap():
        out['swap'] = v.renyi_parts(lengths, origin)

    for _ in range(a.warm):
        g1()
        swap()
    t1, t2 = [], []
    for _ in range(a.reps):
        t1.append(timed(eng, g1))
        t2.append(timed(eng, swap))
    matched = out['swap'][:, 2]
    assert np.all(out['g1'][:, 0] > 0)
    assert np.all((matched >= 0) & (matched <= W // 2))
    assert np.all(out['swap'][:, 0] > 0)
    frac = matched.sum() / (K * (W // 2))
    m1, sp1 = stat(t1)
    m2, sp2 = stat(t2)
    say(f'N={n} W={W} K={K}: g1 {m1:8.3f} ms (spread {sp1:.3f})  swap '
        f'{m2:8.3f} ms (spread {sp2:.3f})  swap/g1 {m2 / m1:.2f}  matched '
        f'{frac:.3f}')
    v.close()
    eng.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
