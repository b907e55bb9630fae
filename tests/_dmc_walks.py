"""The walks of the DMC block estimator tests, and the twin-ensemble harness
they share (tests/test_gpu_{pairdist,superfluid,isf,obdm,site}_est.py and
tests/test_gpu_dist_estimators.py).

Ensemble A and ensemble B start from the same positions with the same seed, so
they follow the same trajectory (test_gpu_sampling.py::
test_dmc_split_step_equals_block).  A runs one time step at a time and hands
out its state after each (`record`); B runs one estimator block, in the module
of its estimator; a NumPy restatement of the estimator on A's states is the
yardstick for B's rows.  A walk is recorded once per pytest process, however
many modules compare against it.
"""
import functools
import json
import os
from typing import NamedTuple, Optional

import numpy as np

from ._models import box, spec_from_golden

TIME_STEP = 1e-3
CONTROL = 0.5                   # the population control factor
WAVEFRONTS = 4096               # of an estimator launch: 1024 blocks of 4


class Walk(NamedTuple):
    n: int                      # bosons
    cut: Optional[float]        # contact cutoff / L
    nw0: int                    # start walkers
    maxw: int                   # the cap
    seed: int                   # of the start positions and of the ensemble
    sites: Optional[int] = None     # supercell size L; None: L = N
    ratio: int = 1
    golden: Optional[str] = None    # the model is tests/golden/params.json's


# The first seven are the smallest populations that still reach every path of
# an estimator kernel (each module says which): an odd N below a wavefront;
# N = 16, twice; N = 64, one particle per lane, with more walkers than one pass
# of a block's wavefronts; N = 100, two passes over the particles; a population
# that starts at its cap; more live walkers than an estimator launch has
# wavefronts, so that every wavefront goes round its slot loop again.
WALKS = {
    'odd':         Walk(5, 0.25, 40, 64, 1100),
    'one_bin':     Walk(16, 0.25, 48, 64, 12),
    'many':        Walk(16, 0.25, 48, 64, 13),
    'wave':        Walk(64, 0.25, 300, 512, 14),
    'two_pass':    Walk(100, 0.1, 64, 96, 15),
    'cap':         Walk(16, 0.25, 64, 64, 1600),
    'second_trip': Walk(37, 0.25, 4500, 5120, 1700),
    # g1(s) alone: the largest LDS request; no one-body factor; no pair factor;
    # a non-integer L, which is not a period of the one-body factor
    'n512':        Walk(512, 0.25, 12, 16, 18),
    'free16':      Walk(16, None, 24, 32, 19, golden='free16'),
    'ideal16':     Walk(16, None, 24, 32, 20, golden='ideal16'),
    'odd24':       Walk(24, None, 24, 32, 21, golden='odd24'),
    # the site statistics have walks of their own: other seeds, and supercells
    # with fewer or more sites than bosons
    'site_odd':         Walk(5, 0.25, 40, 64, 2100, sites=5),
    'site_occ_only':    Walk(16, 0.25, 48, 64, 22, sites=16),
    'site_many':        Walk(16, 0.25, 48, 64, 23, sites=16),
    'site_dilute':      Walk(8, 0.25, 48, 64, 24, sites=32),
    'site_dense':       Walk(64, 0.25, 100, 160, 25, sites=16),
    'site_wave':        Walk(64, 0.25, 300, 512, 26, sites=64),
    'site_two_pass':    Walk(100, 0.1, 64, 96, 27, sites=200),
    'site_cap':         Walk(16, 0.25, 64, 64, 2600, sites=16),
    'site_second_trip': Walk(37, 0.25, 4500, 5120, 2700, sites=37),
    # the sharded population.  `wide`: two label passes per wavefront, N no
    # multiple of 64
    'small':       Walk(16, 0.25, 250, 512, 41, sites=16),
    'wide':        Walk(100, 0.1, 64, 96, 42, sites=200),
}


@functools.lru_cache(maxsize=None)
def _golden_params():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, 'golden', 'params.json')) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def spec(walk):
    if walk.golden is not None:
        return spec_from_golden(_golden_params(), walk.golden)
    return box(walk.n, walk.cut, sites=walk.sites, ratio=walk.ratio)


def start_positions(walk):
    """Uniform in [0, L) -> pos[nw0, N]."""
    L = float(spec(walk).supercell_size)
    return L * np.random.RandomState(walk.seed).random_sample(
        (walk.nw0, walk.n))


def engine(walk, stream=None):
    """An engine of the walk's model on device 0, or on the caller's stream."""
    from phd_qmclib_amd.engine import ModelEngine
    if stream is None:
        return ModelEngine(spec(walk).cfc_spec, device=0)
    return ModelEngine(spec(walk).cfc_spec, stream=stream)


def ensemble(eng, walk, **kw):
    """The walk's population at its start."""
    from phd_qmclib_amd.engine import DmcEnsemble
    kw.setdefault('rng_seed', walk.seed)
    d = DmcEnsemble(eng, TIME_STEP, walk.maxw, walk.nw0, CONTROL, **kw)
    d.set_state(start_positions(walk))
    return d


def state_of(d):
    """-> (confs[W, N], cloning_ref, num_walkers): a step as the restatements
    take it."""
    s = d.get_state()
    return (s.confs[:, 0, :].copy(), s.cloning_ref.copy(), int(s.num_walkers))


@functools.lru_cache(maxsize=None)
def record(name, steps):
    """Ensemble A: the states after each of `steps` single-step blocks of
    WALKS[name] -> dict(steps, energy, num_walkers), every array read-only.
    The rows of a step are the full slot arrays: slice them with its
    num_walkers."""
    walk = WALKS[name]
    eng = engine(walk)
    a = ensemble(eng, walk)
    out, energy = [], []
    for _ in range(steps):
        ser = a.run_block(1)
        out.append(state_of(a))
        energy.append(ser.energy[0])
    a.close()
    eng.close()
    energy = np.array(energy)
    num_walkers = np.array([s[2] for s in out])
    for arr in [energy, num_walkers] + [x for s in out for x in s[:2]]:
        arr.setflags(write=False)
    return dict(steps=tuple(out), energy=energy, num_walkers=num_walkers)


# ---- the checks every module makes -------------------------------------------
def assert_transport_exercised(rec, walk, tag):
    """A step whose cloning table is not the identity, and a population that
    changes; what the walks `cap` and `second_trip` are there for."""
    assert any(not np.array_equal(r[:nw], np.arange(nw))
               for _, r, nw in rec['steps'])
    assert len(set(rec['num_walkers']) | {walk.nw0}) > 1
    if tag == 'cap':
        assert walk.nw0 == walk.maxw
    if tag == 'second_trip':
        assert walk.maxw >= 5120 and (rec['num_walkers'] > WAVEFRONTS).all()


def numerators(rows, T, pfw, pure):
    """The integers behind forward-walking rows: a pure entry is the rounded
    quotient of an integer by min(t + 1, pfw) (thirds, say), and a float sum
    of such quotients is not exact.  Row identities are checked on the
    numerators, which each entry must give back bit for bit
    -> (counts[T, K], div[T, 1])."""
    div = np.minimum(np.arange(T) + 1, pfw if pure else 1)[:, None]
    counts = np.rint(rows * div)
    assert np.array_equal(counts / div, rows)
    return counts, div


def assert_same_series(a, b):
    """Two `DmcSeries`, byte for byte."""
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def assert_refused_by_distributed(walk, switch_on, switch_off, match, **kw):
    """`DistributedDmc` without `block_estimators` refuses an ensemble whose
    estimator `switch_on(d)` set, and takes it after `switch_off(d)`."""
    import pytest
    import torch
    from phd_qmclib_amd.dist import DistributedDmc
    eng = engine(walk, stream=torch.cuda.current_stream().cuda_stream)
    d = ensemble(eng, walk, external_reduce=True, **kw)
    switch_on(d)
    with pytest.raises(NotImplementedError, match=match):
        DistributedDmc(d, walk.n, 'cuda', solo=True)
    switch_off(d)
    DistributedDmc(d, walk.n, 'cuda', solo=True)
    d.close()
    eng.close()


# ---- the estimators a module does not test, switched on beside its own -------
EST = dict(num_modes=8, ssf_pure=True, ssf_pfw=3, num_bins=12, dens_pure=False)
G2 = dict(num_bins=20, pure=True, pfw=3)
# the settings of the modules that set every slot (site statistics, sharding)
ALL_SLOTS = dict(g2=dict(num_bins=10, pure=True, pfw=3), cm=True,
                 isf=(3, 2, 2), obdm=((0.0, 0.5, 1.25), 2))


def set_others(d, est=EST, g2=G2, cm=False, isf=None, obdm=None,
               reverse=False):
    """S(k) and the density, g2(r), and on request the centre-of-mass
    diffusion, F(k, tau) = (K, T, q) and g1(s) = (shifts, stride), in this
    order or in the reverse one."""
    todo = [lambda: d.set_estimators(**est),
            lambda: d.set_pair_dist_estimator(**g2)]
    if cm:
        todo.append(lambda: d.set_cm_diffusion_estimator(True))
    if isf is not None:
        todo.append(lambda: d.set_isf_estimator(*isf))
    if obdm is not None:
        todo.append(lambda: d.set_obdm_estimator(*obdm))
    for setter in (reversed(todo) if reverse else todo):
        setter()
