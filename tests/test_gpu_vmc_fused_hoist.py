"""What the fused steady VMC launch of the one-particle-per-lane shape keeps
in registers across its yields (values derived from the lane index: the sort's
partner addresses and flip masks, the LDS row pointers of both pair passes,
the parity and half-wave flags, the ring source of the padded shape) against
the per-yield LEAN kernel, which derives them once per launch and is not
touched by how the yield loop is compiled.

One steady launch of K yields against K blocks of one yield each, bit for
bit: positions and labels (the positions come back in particle order, through
the labels), log|psi|, the carried energy, the three block sums and the
general-path counter.  N = 64 (unpadded), 63 and 33 (padded, odd ring: no half
step, idle lanes), 48 (padded, even); 130 chains (the grid is rounded up to
128 workgroups: inactive wavefronts); K = 1, 2, 65 and 130 (the accept
thresholds refill at yields 64 and 128 of a launch); the benchmark box and the
free model; and chains at the edge of the sorted-row path, which take the
general path in some yields of a launch and the sorted rows in the others.

A block of K + 1 yields is the per-yield kernel once and then ONE steady
launch of K yields (qmc_vmc_run_block).  Every ensemble first runs a block of
one yield, the forced initial yield, so that the compared blocks hold real
moves only.  The reference of a (model, start) pair is computed once, for 131
yields, and shared by the four launch lengths.

The block sums of the reference are rebuilt on the host exactly as the kernel
forms them: sum_e = sum_e + e and sum_e2 = fma(e, e, sum_e2), yield by yield.
A block of one yield returns e itself as its sum_energy (lanes 1, 2 and 3,
which give the carried energy, e for sum_e and e for sum_e2, sit in one 4x4
block of the matrix-core wave sum and hold the same bits), and the fused
multiply-add is evaluated in rational arithmetic and rounded once.  The move
spread is exactly 0.125, at which vmc_move_unit * move_spread is exact."""

from fractions import Fraction

import numpy as np
import pytest

from ._models import box

pytestmark = pytest.mark.gpu

W = 130
KS = (1, 2, 65, 130)
SEED = 61

MODELS = {'box': {}, 'free': dict(lattice_depth=0)}


def lattice(n, seed):
    # one particle per well, jittered: the sorted-row path
    rng = np.random.RandomState(seed)
    return np.arange(n)[None, :] + 0.25 + 0.3 * (rng.random_sample((W, n)) - 0.5)


def edge(n, seed):
    """Even chains: more than half of the particles (n // 2 + 1, evenly spaced)
    on an arc a little shorter or longer than r_m = L / 4 and the others evenly
    over the rest of the box -- the farthest partner of the rotation sits at
    L - r_m, give or take less than a move, so the once-per-walker test of the
    sorted-row path fails in some yields and holds in others.  Odd chains: the
    lattice."""
    rng = np.random.RandomState(seed)
    pos = lattice(n, seed + 1)
    m = n // 2 + 1
    for w in range(0, W, 2):
        arc = 0.25 * n + 0.08 * (rng.random_sample() - 0.5)
        z0 = 0.75 * n * rng.random_sample()
        pos[w, :m] = z0 + arc * np.arange(m) / (m - 1)
        pos[w, m:] = z0 + arc + (n - arc) * np.arange(1, n - m + 1) / (n - m + 1)
    return pos % n


STARTS = {'lattice': lattice, 'edge': edge}


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


_reference = {}


def reference(n, model, start):
    """Per K: the state and the block sums after a block of one yield (the
    forced one) and K + 1 more blocks of one yield each."""
    key = (n, model, start)
    if key in _reference:
        return _reference[key]
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n, **MODELS[model])
    eng = ModelEngine(spec.cfc_spec, device=0)
    v = VmcEnsemble(eng, W, 0.25 * spec.well_width, rng_seed=SEED)
    out = {}
    try:
        v.set_state(STARTS[start](n, 500 + n))
        v.run_block(1)
        eng.general_path_walkers(reset=True)
        se, se2 = np.zeros(W), np.zeros(W)
        na = np.zeros(W, dtype=np.int64)
        for y in range(1, max(KS) + 2):
            r = v.run_block(1)
            e = r['sum_energy']
            se = se + e
            se2 = np.array([fma(a, a, b) for a, b in zip(e, se2)])
            na = na + r['num_accepted']
            if y - 1 in KS:
                out[y - 1] = dict(
                    state=v.get_state(), sum_energy=se, sum_energy2=se2,
                    num_accepted=na,
                    general=eng.general_path_walkers(reset=False))
    finally:
        v.close(); eng.close()
    _reference[key] = out
    return out


def fused_block(n, model, start, k):
    """-> the sums, the state and the general-path count of a block of k + 1
    yields (one steady launch of k) after the forced yield."""
    from phd_qmclib_amd.engine import ModelEngine, VmcEnsemble
    spec = box(n, **MODELS[model])
    eng = ModelEngine(spec.cfc_spec, device=0)
    v = VmcEnsemble(eng, W, 0.25 * spec.well_width, rng_seed=SEED)
    try:
        v.set_state(STARTS[start](n, 500 + n))
        v.run_block(1)
        eng.general_path_walkers(reset=True)
        x = v.run_block(k + 1)
        x['general'] = eng.general_path_walkers(reset=True)
        x['state'] = v.get_state()
    finally:
        v.close(); eng.close()
    return x


def assert_same(x, ref):
    for name, a, b in zip(('pos', 'wf', 'ecarry'), x['state'], ref['state']):
        assert np.array_equal(a, b), name
    for name in ('sum_energy', 'sum_energy2', 'num_accepted'):
        assert np.array_equal(x[name], ref[name]), name
    assert x['general'] == ref['general']


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('model', list(MODELS))
@pytest.mark.parametrize('n', [64, 63, 33, 48])
def test_steady_launch_matches_single_yields(n, model, k):
    ref = reference(n, model, 'lattice')[k]
    x = fused_block(n, model, 'lattice', k)
    assert_same(x, ref)
    # (moves were accepted and moves were rejected: both arms of the yield ran
    # -- over the ensemble; the free model accepts nine moves in ten)
    if k > 2:
        assert 0 < x['num_accepted'].sum() < W * (k + 1)


# Leaving and re-entering the sorted-row path inside one launch: whatever the
# general path clobbers has to be there again in the next sorted yield.  The
# unpadded and the even padded shape; 65 yields, one refill.
@pytest.mark.parametrize('n', [64, 48])
def test_leaves_and_reenters_sorted_path(n):
    k = 65
    ref = reference(n, 'box', 'edge')[k]
    x = fused_block(n, 'box', 'edge', k)
    assert_same(x, ref)
    # the general path did run, and not in every yield of the chains at the
    # edge (the lattice chains never take it)
    assert 0 < x['general'] < (k + 1) * (W // 2)
