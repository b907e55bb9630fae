"""Cost of the second-order DMC propagator against the linear one: engine-timer
milliseconds per time step of `propagator='quadratic'` and 'linear' on the
same box and the same ensemble (development tool, needs the GPU).

usage: dmc2_cost.py [N:walkers ...]     (default: 64:262144 128:1048576)

The standard box (depth 5 pi^2, ratio 1, coupling 2, L = N, cutoff N / 4),
walkers on jittered lattices, cap = walkers, kappa 0.5, dt 1e-3 for both (the
work of a step does not depend on dt).  Per propagator: a warm-up block (code
objects, the first sorts), then REPEATS timed blocks, the two propagators
alternating; the figure is the median block.  Prints one JSON line per
ensemble: ms per step of each, their ratio, and the steps per unit of
imaginary time at the time step given for each (--dt-linear, --dt-quadratic).
"""
import argparse
import json
import os
import sys
from math import pi

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from phd_qmclib_amd.engine import DmcEnsemble, ModelEngine  # noqa: E402
from phd_qmclib_amd.mrbp_qmc import Spec  # noqa: E402


def ensemble(eng, n, walkers, propagator):
    d = DmcEnsemble(eng, 1e-3, walkers, walkers, 0.5, rng_seed=1,
                    propagator=propagator)
    rng = np.random.RandomState(n)
    d.set_state((np.arange(n) + 0.5 +
                 0.6 * (rng.random_sample((walkers, n)) - 0.5)))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('cases', nargs='*', default=['64:262144', '128:1048576'])
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--dt-linear', type=float, default=2.5e-4)
    ap.add_argument('--dt-quadratic', type=float, default=4e-3)
    args = ap.parse_args()
    for case in args.cases:
        n, walkers = (int(x) for x in case.split(':'))
        eng = ModelEngine(Spec(
            lattice_depth=5 * pi ** 2, lattice_ratio=1, interaction_strength=2,
            boson_number=n, supercell_size=n,
            tbf_contact_cutoff=0.25 * n).cfc_spec)
        ens = {p: ensemble(eng, n, walkers, p)
               for p in ('linear', 'quadratic')}
        ms = {p: [] for p in ens}
        for rep in range(args.repeats + 1):
            for p, d in ens.items():
                eng.timer_start()
                d.run_block(args.steps, read=False)
                t = eng.timer_stop() / args.steps
                if rep:                 # (the first block warms up)
                    ms[p].append(t)
        general = eng.general_path_walkers()
        for d in ens.values():
            d.close()
        eng.close()
        lin, quad = (float(np.median(ms[p])) for p in ('linear', 'quadratic'))
        print(json.dumps(dict(
            n=n, walkers=walkers, steps=args.steps, repeats=args.repeats,
            ms_per_step_linear=lin, ms_per_step_quadratic=quad,
            spread_linear=[min(ms['linear']), max(ms['linear'])],
            spread_quadratic=[min(ms['quadratic']), max(ms['quadratic'])],
            ratio=quad / lin, general_path_walkers=general,
            ms_per_unit_time_linear=lin / args.dt_linear,
            ms_per_unit_time_quadratic=quad / args.dt_quadratic,
            dt_linear=args.dt_linear, dt_quadratic=args.dt_quadratic)),
            flush=True)


if __name__ == '__main__':
    main()
