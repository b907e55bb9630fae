"""Time-step dependence of the DMC energy with both propagators, on the
ensemble of tests/test_gpu_dmc2_timestep.py (development tool, needs the GPU):
the pooled mean E / N and its error of the linear propagator at 5e-4, 1e-3,
2e-3 and of the quadratic one at 2e-3, 4e-3, 8e-3, the linear extrapolation E0
and every difference in units of its combined error.  DESIGN.md quotes a run.

usage: dmc2_timestep.py [--tau T] [--linear-only]
`--linear-only`: the runs from which the imaginary time of the test is chosen.
"""
import argparse
import os
import sys
import time
from math import sqrt

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_dmc2_timestep as ts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tau', type=float, default=ts.TAU)
    ap.add_argument('--linear-only', action='store_true')
    args = ap.parse_args()
    from phd_qmclib_amd.engine import ModelEngine
    eng = ModelEngine(ts.box(ts.N).cfc_spec)
    runs = [('linear', 5e-4), ('linear', 1e-3), ('linear', 2e-3)]
    if not args.linear_only:
        runs += [('quadratic', 2e-3), ('quadratic', 4e-3), ('quadratic', 8e-3)]
    got = {}
    for prop, dt in runs:
        t0 = time.perf_counter()
        got[prop, dt] = ts.pooled(eng, prop, dt, tau=args.tau)
        m, s = got[prop, dt]
        print(f'tau {args.tau:g} {prop:9s} dt {dt:g}: E/N = {m:.5f} +- {s:.5f}'
              f'   ({time.perf_counter() - t0:.2f} s for {len(ts.SEEDS)} '
              f'seeds)', flush=True)
    eng.close()
    (a, sa), (b, sb) = got['linear', 5e-4], got['linear', 1e-3]
    e0, s0 = 2 * a - b, sqrt(4 * sa * sa + sb * sb)
    print(f'E0 = {e0:.5f} +- {s0:.5f}')
    for key, (m, s) in got.items():
        if key[1] >= 2e-3:
            c = sqrt(s0 * s0 + s * s)
            print(f'{key[0]:9s} dt {key[1]:g}: E - E0 = {m - e0:+.5f} = '
                  f'{(m - e0) / c:+.2f} sigma_comb ({c:.5f})')


if __name__ == '__main__':
    main()
