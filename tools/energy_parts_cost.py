"""Cost of the energy components next to g1(s) at 16 shifts and to one
evaluation pass, on the same resident rows in one process, and the two routes
to the interaction energy at full statistics (development tool).
usage: energy_parts_cost.py [--shapes 64:65536,128:65536] [--reps 5]
                            [--warm 2] [--inner 100] [--chains 262144]
                            [--sweeps 300] [--out FILE]

Timing.  The ensemble is in the stationary state of the VMC chain
(tools/_stationary.py).  Per shape, the engine timer (events on the stream)
around `inner` back-to-back calls of
  qmc_energy_parts_reduce_dev, no window      (energy_components, K = 0)
  qmc_energy_parts_reduce_dev, four windows   (energy_components, K = 4)
  qmc_obdm_reduce_dev, 16 shifts              (g1, the usual yardstick)
  qmc_evaluate_dev, energy and drift          (one evaluation pass)
taking turns, `warm` untimed calls of each first, median of `reps` windows:
milliseconds per call, the spread (max - min) / median, and the ratios.  No
ratio is asserted.

Physics.  N = 8 in the box of tests/_models.box, `chains` independent chains
of single-particle sweeps (move_spread 1) from a uniform start, `sweeps` sweeps,
one snapshot: the remainder <E_L - T - V>, g <C> at the windows 0.02, 0.05
and 0.2, its extrapolation to zero range from the first two, and the plain
coincidence count at 0.1 (from the pair histogram, no cusp weight) times g.
The errors are those of the mean over the chains."""
import argparse
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _stationary import replicate, seed_configurations  # noqa: E402
from phd_qmclib_amd.engine import (DeviceBuffer, ModelEngine,  # noqa: E402
                                   VmcEnsemble, contact_extrapolate)
from phd_qmclib_amd.mrbp_qmc import Spec, vmc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='64:65536,128:65536')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--warm', type=int, default=2)
ap.add_argument('--inner', type=int, default=100)
ap.add_argument('--chains', type=int, default=1 << 18)
ap.add_argument('--sweeps', type=int, default=300)
ap.add_argument('--out', default=None)
a = ap.parse_args()
lines = []
WINDOWS = (0.02, 0.05, 0.1, 0.2)
NSHIFT = 16


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


# ---- timing ----------------------------------------------------------------
for shape in (s for s in a.shapes.split(',') if s):
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
    shifts = 0.5 * n * (np.arange(NSHIFT) + 1.0) / NSHIFT
    dsh = DeviceBuffer((NSHIFT,), eng.device).upload(shifts)
    s0 = DeviceBuffer((4, 2), eng.device)
    s4 = DeviceBuffer((4 + len(WINDOWS), 2), eng.device)
    sg = DeviceBuffer((NSHIFT, 2), eng.device)
    den = DeviceBuffer((W,), eng.device)
    ddr = DeviceBuffer((W, n), eng.device)
    calls = {
        'parts K=0': lambda: eng.energy_parts_reduce_dev(W, pos_dev, None, (),
                                                         s0.ptr),
        'parts K=4': lambda: eng.energy_parts_reduce_dev(W, pos_dev, None,
                                                         WINDOWS, s4.ptr),
        'g1 16 shifts': lambda: eng.one_body_density_reduce_dev(
            W, pos_dev, None, NSHIFT, dsh.ptr, sg.ptr),
        'evaluate': lambda: eng.evaluate_dev(W, pos_dev, 0, den.ptr, 0,
                                             ddr.ptr),
    }
    for _ in range(a.warm):
        for call in calls.values():
            call()
    eng.sync()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, call in calls.items():
            times[k].append(timed(eng, call))
    med = {k: stat(ts) for k, ts in times.items()}
    # (the sums of the two calls agree on the four leading columns)
    assert np.array_equal(s0.download(), s4.download()[:4])
    say(f'N={n} W={W}: ' + '  '.join(
        f'{k} {m:8.3f} ms (spread {sp:.3f})' for k, (m, sp) in med.items()))
    g1 = med['g1 16 shifts'][0]
    ev = med['evaluate'][0]
    say(f'N={n} W={W}: ratios to g1 at 16 shifts: K=0 '
        f'{med["parts K=0"][0] / g1:.2f}  K=4 {med["parts K=4"][0] / g1:.2f}'
        f'   to one evaluate pass: K=0 {med["parts K=0"][0] / ev:.2f}  '
        f'K=4 {med["parts K=4"][0] / ev:.2f}')
    for b in (dsh, s0, s4, sg, den, ddr):
        b.close()
    v.close()
    eng.close()

# ---- the two routes to the interaction energy ------------------------------
say('')
for name, args in (('gint=2', dict(gint=2.0, depth=5 * pi ** 2)),
                   ('gint=20, depth=2pi^2', dict(gint=20.0,
                                                 depth=2 * pi ** 2))):
    if a.chains <= 0:
        break
    n = 8
    spec = Spec(lattice_depth=args['depth'], lattice_ratio=1,
                interaction_strength=args['gint'], boson_number=n,
                supercell_size=n, tbf_contact_cutoff=0.25 * n)
    s = vmc.EnsembleSampling(spec, 1.0, a.chains, rng_seed=5, move='particle')
    s.init_random(5)
    next(s.blocks(a.sweeps))
    ec = s.energy_components(WINDOWS)
    g = ec.coupling
    # the plain window at 0.1: the first bin of the pair histogram, 40 bins
    # of 0.1 over [0, L/2]
    hist = s.ensemble.pair_dist_parts(40)[:, 0] / a.chains
    plain = g * hist[0] / (2.0 * 0.1)
    c0, c0_err = contact_extrapolate(WINDOWS[:2], ec.contact[:2],
                                     ec.contact_err[:2])
    say(f'{name} (N=8, {a.chains} chains, {a.sweeps} sweeps, g = {g:.6f}): '
        f'E {ec.total:.3f} +- {ec.total_err:.3f}  T {ec.kinetic:.3f} +- '
        f'{ec.kinetic_err:.3f}  V {ec.lattice:.3f} +- {ec.lattice_err:.3f}')
    say(f'{name}: remainder <E_L - T - V> {ec.interaction:.3f} +- '
        f'{ec.interaction_err:.3f}  ' + '  '.join(
            f'g C({r}) {g * c:.3f} +- {g * e:.3f}'
            for r, c, e in zip(WINDOWS, ec.contact, ec.contact_err)) +
        f'  r -> 0 from (0.02, 0.05): {g * c0:.3f} +- {g * c0_err:.3f}  '
        f'plain window 0.1: {plain:.3f}')
    s.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
