"""The order of the second-order DMC propagator, statistically: on the
standard box (depth 5 pi^2, ratio 1, coupling 2, L = N, cutoff N / 4) at
N = 8 the mixed energy per particle of `propagator='quadratic'` at dt = 2e-3
sits on the dt -> 0 limit of the LINEAR propagator, where the linear one at
the same dt is visibly off.

Setup: target 4096 walkers, cap 4608, kappa 0.5, `fix_stale_energy=True` for
the linear runs, seeds 1, 2, 3 pooled (fixed before any run).  Every run
covers the same imaginary time TAU, its first sixth discarded; the rest is
cut into blocks of BLOCK_TAU, a block's energy is its sum of E_t over its sum
of W_t (per particle), and the error of a run's mean comes from
`stats.reblock` on these block values; the three seeds are independent, so
the pooled mean is their average and its variance the sum of theirs over 9.

Reference, from the linear propagator alone (its bias is linear in dt):
E0 = 2 E_lin(5e-4) - E_lin(1e-3), sigma0^2 = 4 sigma^2(5e-4) + sigma^2(1e-3).

Asserted, with sigma_comb^2 = sigma0^2 + sigma^2 of the run compared:
    |E_quad(2e-3) - E0| <= 3.5 sigma_comb
    E_lin(2e-3) - E0   <= -4  sigma_comb     (the test can see a first-order
                                              bias of this size at all)

TAU was chosen from the linear runs alone, so that the second assertion holds
with room to spare; DESIGN.md quotes the measured figures, E_quad(4e-3) and
E_quad(8e-3) (reported by tools/dmc2_timestep.py, not asserted) included.
"""
from math import sqrt

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu

N = 8
TARGET, MAXW, KAPPA = 4096, 4608, 0.5
SEEDS = (1, 2, 3)
TAU = 24.0                      # imaginary time of every run
BLOCK_TAU = 0.032               # ... of a block: 64 steps of 5e-4, 4 of 8e-3
DISCARD = 1.0 / 6.0


def start(seed, walkers=TARGET, n=N):
    """One particle per well, each up to 0.3 of the spacing off its centre."""
    rng = np.random.RandomState(1000 + seed)
    return (np.arange(n) + 0.5 + 0.6 * (rng.random_sample((walkers, n)) - 0.5))


def run(eng, propagator, dt, seed, tau=TAU, target=TARGET, maxw=MAXW):
    """-> (mean E / N, its error) of one run."""
    from phd_qmclib_amd.engine import DmcEnsemble
    from phd_qmclib_amd.stats.reblock import OTFObject
    per_block = int(round(BLOCK_TAU / dt))
    nblocks = int(round(tau / BLOCK_TAU))
    d = DmcEnsemble(eng, dt, maxw, target, KAPPA, rng_seed=seed,
                    fix_stale_energy=True, propagator=propagator)
    try:
        d.set_state(start(seed, target))
        ser = d.run_block(per_block * nblocks)
    finally:
        d.close()
    e = ser.energy.reshape(nblocks, per_block).sum(axis=1)
    w = ser.weight.reshape(nblocks, per_block).sum(axis=1)
    blocks = (e / w / N)[int(round(DISCARD * nblocks)):]
    otf = OTFObject.from_non_obj_data(blocks)
    return float(otf.mean), float(otf.mean_eff_error)


def pooled(eng, propagator, dt, **kw):
    """-> (mean, error) over the seeds."""
    runs = [run(eng, propagator, dt, seed, **kw) for seed in SEEDS]
    mean = sum(m for m, _ in runs) / len(runs)
    err = sqrt(sum(s * s for _, s in runs)) / len(runs)
    return mean, err


def reference(eng, **kw):
    """E0 and sigma0 from the linear runs at 5e-4 and 1e-3."""
    (a, sa), (b, sb) = (pooled(eng, 'linear', dt, **kw) for dt in (5e-4, 1e-3))
    return 2 * a - b, sqrt(4 * sa * sa + sb * sb), (a, sa), (b, sb)


def test_quadratic_energy_sits_on_the_linear_extrapolation():
    from phd_qmclib_amd.engine import ModelEngine
    eng = ModelEngine(box(N).cfc_spec)
    try:
        e0, s0, half, one = reference(eng)
        lin, s_lin = pooled(eng, 'linear', 2e-3)
        quad, s_quad = pooled(eng, 'quadratic', 2e-3)
    finally:
        eng.close()
    for name, (m, s) in (('E_lin(5e-4)', half), ('E_lin(1e-3)', one),
                         ('E0', (e0, s0)), ('E_lin(2e-3)', (lin, s_lin)),
                         ('E_quad(2e-3)', (quad, s_quad))):
        print(f'dmc2 timestep {name} = {m:.5f} +- {s:.5f}')
    c_quad = sqrt(s0 * s0 + s_quad * s_quad)
    c_lin = sqrt(s0 * s0 + s_lin * s_lin)
    print(f'dmc2 timestep quad - E0 = {(quad - e0) / c_quad:+.2f} sigma, '
          f'lin - E0 = {(lin - e0) / c_lin:+.2f} sigma')
    assert abs(quad - e0) <= 3.5 * c_quad
    assert lin - e0 <= -4.0 * c_lin
