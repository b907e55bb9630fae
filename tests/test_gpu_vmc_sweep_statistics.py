"""Single-particle VMC sweeps sample |psi|^2 and decorrelate the local energy
faster per yield than the all-particle step: the N = 16 box (V0 = 5 pi^2,
r = 1, g = 2, L = 16, cutoff 4), 4096 independent chains.  The yardstick is
the all-particle sampler, which the suite pins against the oracle.

Every number below was fixed before the first run:

* start: one particle per well plus jitter, both samplers the same rows;
* 'all' at spread 0.125 is given EQUIL_ALL = 20000 steps (tools/_stationary.py
  records ~20000 for the N = 64 box from the same start) and the choice is
  checked on the 'all' run alone: two successive blocks of it agree;
* 'particle' at spread 0.5 is given EQUIL_ALL / 8 sweeps: a sweep offers every
  particle a displacement four times as wide, sixteen times the diffusion
  per yield at equal acceptance, and half of that is kept in hand;
* blocks of 2000 steps / 250 sweeps; the standard error of a mean over the
  chains is the spread of the per-chain block means over sqrt(W);
* |z| <= 4 on <E> and on <E_L^2>; rho_particle(1) < rho_all(1) - 0.1, six
  standard errors of a correlation coefficient over 4096 chains."""
from math import pi

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, N, L = 4096, 16, 16.0
SEED_ROWS, SEED_ALL, SEED_PARTICLE = 20161, 11, 12
EQUIL_ALL, BLOCK_ALL = 20000, 2000
EQUIL_PARTICLE, BLOCK_PARTICLE = EQUIL_ALL // 8, BLOCK_ALL // 8


def advance(v, steps):
    done = 0
    while done < steps:
        b = min(500, steps - done)
        v.run_block(b, sums=False)
        done += b


def block_means(v, steps):
    out = v.run_block(steps)
    return out['sum_energy'] / steps, out['sum_energy2'] / steps, \
        out['num_accepted']


def mean_se(x):
    return float(np.mean(x)), float(np.std(x, ddof=1) / np.sqrt(len(x)))


def zscore(a, b):
    (ma, sa), (mb, sb) = mean_se(a), mean_se(b)
    return (ma - mb) / np.hypot(sa, sb)


def rho1(v):
    e = v.run_block(2, series=True)['energy']
    return float(np.corrcoef(e[0], e[1])[0, 1])


@pytest.fixture(scope='module')
def samplers():
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    from phd_qmclib_amd.mrbp_qmc import Spec
    spec = Spec(lattice_depth=5 * pi ** 2, lattice_ratio=1,
                interaction_strength=2, boson_number=N, supercell_size=N,
                tbf_contact_cutoff=4)
    eng = ModelEngine(spec.cfc_spec)
    rng = np.random.RandomState(SEED_ROWS)
    ww = spec.well_width
    rows = (np.arange(N)[None, :] + 0.5 * ww +
            0.6 * ww * (rng.random_sample((W, N)) - 0.5))
    va = VmcEnsemble(eng, W, 0.125, rng_seed=SEED_ALL)
    vp = VmcEnsemble(eng, W, 0.5, rng_seed=SEED_PARTICLE, move='particle')
    res = {}
    for name, v, equil, block in (('all', va, EQUIL_ALL, BLOCK_ALL),
                                  ('particle', vp, EQUIL_PARTICLE,
                                   BLOCK_PARTICLE)):
        v.set_state(rows)
        advance(v, equil)
        first = block_means(v, block)
        second = block_means(v, block)
        res[name] = dict(first=first, second=second, rho1=rho1(v),
                         block=block)
    va.close(); vp.close(); eng.close()
    return res


def test_all_particle_run_is_stationary(samplers):
    """The equilibration is sized on the yardstick alone."""
    a = samplers['all']
    z = zscore(a['first'][0], a['second'][0])
    print('all: successive blocks, z = %.2f' % z)
    assert abs(z) <= 4.0


def test_both_samplers_sample_the_same_distribution(samplers):
    a, p = samplers['all'], samplers['particle']
    for k, name in ((0, 'E'), (1, 'E_L^2')):
        for blk in ('first', 'second'):
            z = zscore(p[blk][k], a[blk][k])
            print('%s %s: all %.6f +- %.6f, particle %.6f +- %.6f, z = %.2f'
                  % ((name, blk) + mean_se(a[blk][k]) + mean_se(p[blk][k]) +
                     (z,)))
            assert abs(z) <= 4.0
    acc_a = a['second'][2].mean() / a['block']
    acc_p = p['second'][2].mean() / (p['block'] * N)
    print('acceptance per move: all %.3f, particle %.3f' % (acc_a, acc_p))
    assert 0.0 < acc_a < 1.0 and 0.0 < acc_p < 1.0


def test_sweeps_decorrelate_the_local_energy(samplers):
    ra, rp = samplers['all']['rho1'], samplers['particle']['rho1']
    print('rho(1) of E_L across %d chains: all %.4f, particle %.4f'
          % (W, ra, rp))
    assert rp < ra - 0.1
