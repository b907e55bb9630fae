"""Independent samples per second of the two VMC move types: the all-particle
step at the benchmark's move spread against single-particle sweeps
(`VmcEnsemble(move='particle')`) at several spreads, on stationary ensembles of
the standard box (development tool, needs the GPU).

usage: vmc_sweep_efficiency.py [N:chains ...] [--out FILE]
       (default: 64:65536 128:65536)

Per ensemble (depth 5 pi^2, ratio 1, coupling 2, L = N, cutoff N / 4): the
chains start from copies of 4096 configurations in the stationary state of the
all-particle chain (tools/_stationary.py) and every sampler takes the copies
apart with `--decorrelate` yields of its own (`--decorrelate-all` for the
all-particle chain).  Then, per sampler:

  acceptance   accepted moves / proposed moves of the timed blocks
  ms/yield     engine timer around blocks of `--steps` yields: one warm-up
               block each, then `--repeats` timed blocks, the samplers
               alternating on one engine; the median block
  rho(l)       correlation coefficient over the chains between E_L at yields
               `stride` l apart, l <= 64 (the all-particle chain moves slowly:
               its lags are taken `--stride-all` yields apart)
  tau          1/2 + stride * sum_l rho(l), in yields, the sum cut at the
               first rho < 2 / sqrt(chains); '>=' where no lag got there
  samples/s    chains / (2 tau ms/yield) * 1000
"""
import argparse
import os
import sys
from math import pi, sqrt

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from _stationary import replicate, seed_configurations  # noqa: E402
from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402

LAGS = 64


def advance(v, steps):
    done = 0
    while done < steps:
        b = min(256, steps - done)
        v.run_block(b, sums=False)
        done += b


def energy_series(v, stride):
    """E_L of every chain at LAGS + 1 yields `stride` apart."""
    if stride == 1:
        return v.run_block(LAGS + 1, series=True)['energy']
    rows = []
    for _ in range(LAGS + 1):
        v.run_block(stride, sums=False)
        rows.append(v.get_state()[2])
    return np.array(rows)


def autocorrelation(e):
    x = e - e.mean(axis=1, keepdims=True)
    s = x.std(axis=1)
    return np.array([np.mean(np.mean(x[:LAGS + 1 - k] * x[k:], axis=1) /
                             (s[:LAGS + 1 - k] * s[k:]))
                     for k in range(LAGS + 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('cases', nargs='*', default=['64:65536', '128:65536'])
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--decorrelate', type=int, default=400)
    ap.add_argument('--decorrelate-all', type=int, default=4000)
    ap.add_argument('--stride-all', type=int, default=64)
    ap.add_argument('--spreads', default='0.25,0.5,1.0')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def emit(s=''):
        print(s, flush=True)
        lines.append(s)

    for case in args.cases:
        n, chains = (int(x) for x in case.split(':'))
        spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                    interaction_strength=2, boson_number=n, supercell_size=n,
                    tbf_contact_cutoff=0.25 * n)
        eng = ModelEngine(spec.cfc_spec)
        start = replicate(seed_configurations(eng, spec, n), chains)
        all_spread = 0.25 * spec.well_width
        samplers = [('all', all_spread, 1, args.stride_all)] + \
            [('particle', float(s), n, 1) for s in args.spreads.split(',')]
        ens = []
        for i, (move, spread, moves, stride) in enumerate(samplers):
            v = VmcEnsemble(eng, chains, spread, rng_seed=31 + i, move=move)
            v.set_state(start)
            advance(v, args.decorrelate_all if move == 'all'
                    else args.decorrelate)
            ens.append(v)
        ms = [[] for _ in ens]
        acc = [[] for _ in ens]
        for rep in range(args.repeats + 1):
            for i, v in enumerate(ens):
                eng.timer_start()
                out = v.run_block(args.steps)
                t = eng.timer_stop() / args.steps
                if rep:                 # (the first block warms up)
                    ms[i].append(t)
                    acc[i].append(out['num_accepted'].mean() /
                                  (args.steps * samplers[i][2]))
        cut = 2.0 / sqrt(chains)
        emit(f'N = {n}, {chains} chains, stationary ensemble; blocks of '
             f'{args.steps} yields, median of {args.repeats}; '
             f'rho cut {cut:.4f}')
        emit('move      spread  accept  ms/yield  rho(1)   rho(8)   tau/yields'
             '  samples/s   vs all')
        base = None
        for i, (move, spread, moves, stride) in enumerate(samplers):
            rho = autocorrelation(energy_series(ens[i], stride))
            below = np.nonzero(rho[1:] < cut)[0]
            last = int(below[0]) if below.size else LAGS
            tau = 0.5 + stride * float(rho[1:1 + last].sum())
            t = float(np.median(ms[i]))
            rate = chains / (2.0 * tau * t) * 1000.0
            base = rate if base is None else base
            emit('%-9s %-7.4g %-7.3f %-9.4f %-8.4f %-8.4f %s%-10.1f %-11.3e '
                 '%.2f' % (move, spread, float(np.mean(acc[i])), t,
                           rho[1], rho[8], '  ' if below.size else '>=',
                           tau, rate, rate / base))
            if stride != 1:
                emit(f'          (lags of {stride} yields: rho(1), rho(8) are '
                     f'rho({stride}), rho({8 * stride}))')
        emit(f'general_path_walkers {eng.general_path_walkers()}')
        emit()
        for v in ens:
            v.close()
        eng.close()
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
