"""The second-order DMC propagator without a GPU: its numpy restatement
(tests/_dmc2_restatement.py) in isolation, the preconditions of
tests/test_gpu_dmc2_steps.py, and the `propagator` option through the Python
layers that need no device.

The order of the drift flow.  R_a -> R_b is the midpoint rule (RK2) for
dR/dtau = 2 F(R): one step of length dt has a local error C dt^3, so over a
FIXED imaginary time T the result with steps dt and the result with steps
dt / 2 differ by (3/4) C T dt^2 -- a factor 4 less when dt is halved -- and a
SINGLE step of dt differs from two of dt / 2 by (3/4) C dt^3, a factor 8 less.
(An Euler drift would give 2 and 4.)  Both are asserted, at 4 +- 1 and 8 +- 1,
on the model without a lattice, whose drift is smooth between pair contacts:
with one the one-body drift has a kink at every edge of a barrier, and a row
with a particle that crosses one inside T shows whatever ratio the kink
leaves.
"""
import numpy as np
import pytest

from . import _dmc2_cases as dc
from . import _dmc2_restatement as r2
from . import _generic_cases as gc
from ._steps import jittered_lattice


def min_image(d, L):
    d = np.abs(d)
    return np.minimum(d, L - d)


def flow(oracle, m, row, dt, steps):
    for _ in range(steps):
        row = r2.drift_flow(oracle, m, row, dt)
    return row


@pytest.mark.parametrize('dt', [2e-3, 1e-3])
def test_drift_flow_is_second_order(oracle, dt):
    """All normals zero (the flow alone), rows without a pair closer than
    0.05: over T = 4e-3 the difference between steps of dt and of dt / 2
    falls by 4 +- 1 when dt is halved; for one step of dt against two of
    dt / 2 by 8 +- 1."""
    case = gc.lean_case('free', 16)
    _, m = gc.oracle_model(oracle, case)
    L, T = case[2], 4e-3
    rng = np.random.RandomState(5)
    rows = [jittered_lattice(rng, 16, L) for _ in range(6)]
    assert all(r2.closest_pair(r, L) * L > 0.05 for r in rows)

    def diff(row, h, time):
        k = int(round(time / h))
        return min_image(flow(oracle, m, row, h, k) -
                         flow(oracle, m, row, h / 2, 2 * k), L).max()

    for row in rows:
        fixed_time = diff(row, dt, T) / diff(row, dt / 2, T)
        one_step = diff(row, dt, dt) / diff(row, dt / 2, dt / 2)
        print(f'dt {dt:g}: fixed time {fixed_time:.3f}, one step '
              f'{one_step:.3f}')
        assert abs(fixed_time - 4.0) <= 1.0, fixed_time
        assert abs(one_step - 8.0) <= 1.0, one_step


def test_free_diffusion_has_variance_two_dt(oracle):
    """F = 0 (no lattice, no interaction): R' - R_p = sqrt(dt) (xi1 + xi2),
    variance 2 dt, mean 0.  4800 displacements: the sample variance of a
    normal has relative standard error sqrt(2 / 4800) = 2 %, the mean
    sqrt(2 dt / 4800); both within 4 standard errors."""
    from phd_qmclib_amd.mrbp_qmc import Spec
    n, L, dt, slots = 16, 16.0, 4e-3, 300
    spec = Spec(lattice_depth=0.0, lattice_ratio=1, interaction_strength=0.0,
                boson_number=n, supercell_size=L, tbf_contact_cutoff=0.25 * L)
    assert spec.is_free and spec.is_ideal
    m = oracle.model_from_cfc(spec.cfc_spec)
    row = (np.arange(n) + 0.5) * (L / n)
    assert np.all(oracle.energy_drift(m, row)[2] == 0.0)
    d = []
    for s in range(slots):
        xi1, xi2 = r2.normals(oracle, 17, s, 5, n)
        new = r2.move(oracle, m, row, dt, xi1, xi2)
        raw = new - row
        d.append(raw - L * np.rint(raw / L))
    d = np.concatenate(d)
    count = d.size
    assert abs(d.var() / (2 * dt) - 1.0) <= 4 * np.sqrt(2.0 / count)
    assert abs(d.mean()) <= 4 * np.sqrt(2 * dt / count)


def test_normals_are_the_two_branches_of_one_block(oracle):
    """xi1, xi2 of step counter t: the oracle's normals of steps 2 t and
    2 t + 1, i.e. both Box-Muller branches of the block keyed with t."""
    xi1, xi2 = r2.normals(oracle, 9, 3, 7, 4)
    for i in range(4):
        assert xi1[i] == oracle.dmc_normal(9, 3, 14, i)
        assert xi2[i] == oracle.dmc_normal(9, 3, 15, i)
    assert not np.array_equal(xi1, xi2)


@pytest.mark.parametrize('mult', dc.MULTS)
@pytest.mark.parametrize('cid', dc.IDS)
def test_preconditions_of_the_device_cases(oracle, cid, mult):
    """The share of walkers left out of the device comparison is 0 for the
    seeds chosen (no branching draw within 1e-9 of an integer, no pair closer
    than 1e-9 L at any of the three evaluated rows), the population branches,
    stays below its cap and crosses the box boundary."""
    ref = dc.preconditions(oracle, cid, mult)
    assert ref.left_out == 0 and ref.pop.branch_margin > dc.MARGIN
    assert ref.pop.min_pair_margin > dc.MARGIN


def test_weight_averages_with_the_parent(oracle):
    """One step of two walkers by hand: log w' = -dt ((E' + E_p) / 2 -
    E_ref) with the PARENT's energy, and the yielded state is the parents as
    cloned."""
    case = gc.lean_case('box', 16)
    _, m = gc.oracle_model(oracle, case)
    L, dt = case[2], 2e-3
    rng = np.random.RandomState(2)
    pos0 = np.array([jittered_lattice(rng, 16, L) for _ in range(2)])
    pop = r2.Population(oracle, m, pos0, dt, 4, 2, 0.5, seed=6)
    e0, ref0 = pop.prev_energy[:2].copy(), pop.ref_energy
    nw, e_t, _ = pop.step()
    assert nw == 2 and np.array_equal(pop.cloning_ref[:2], [0, 1])
    assert np.array_equal(pop.confs[:2, 0], pos0)
    assert e_t == pytest.approx(e0.sum(), rel=1e-14)
    for s in range(2):
        xi1, xi2 = r2.normals(oracle, 6, s, 0, 16)
        new = r2.move(oracle, m, pos0[s], dt, xi1, xi2)
        assert np.array_equal(new, pop.prev_confs[s, 0])
        e_new = oracle.energy_drift(m, new)[0]
        assert pop.prev_logw[s] == -dt * ((e_new + e0[s]) / 2 - ref0)


# ---- the option through the layers that need no device ----------------------

MODEL = dict(lattice_depth=5 * np.pi ** 2, lattice_ratio=1,
             interaction_strength=2, boson_number=8, supercell_size=8,
             tbf_contact_cutoff=2)


def test_propagator_names_and_codes():
    from phd_qmclib_amd import _lib
    from phd_qmclib_amd.engine import DMC_PROPAGATORS, dmc_propagator_code
    assert DMC_PROPAGATORS == {'linear': 0, 'quadratic': 1}
    assert dmc_propagator_code('linear') == 0
    assert dmc_propagator_code('quadratic') == 1
    for bad in ('cubic', 'LINEAR', '', None, 0, 1):
        with pytest.raises(ValueError, match='propagator'):
            dmc_propagator_code(bad)
    # the field took the place of `reserved`: same offset, same size
    fields = [f[0] for f in _lib.DmcParams._fields_]
    assert fields[-1] == 'propagator' and 'reserved' not in fields
    assert _lib.DmcParams.propagator.offset == 52
    import ctypes as C
    assert C.sizeof(_lib.DmcParams) == 56


def test_sampling_and_proc_carry_the_propagator():
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.mrbp_qmc import dmc, dmc_exec
    spec = mrbp_qmc.Spec(**MODEL)
    assert dmc.Sampling(spec, 1e-3, 12, 10, rng_seed=1).propagator == 'linear'
    smp = dmc.Sampling(spec, 1e-3, 12, 10, rng_seed=1, propagator='quadratic')
    assert smp.propagator == 'quadratic'
    with pytest.raises(ValueError, match='propagator'):
        dmc.Sampling(spec, 1e-3, 12, 10, rng_seed=1, propagator='cubic')
    assert dmc_exec.Proc(spec, 1e-3).propagator == 'linear'
    proc = dmc_exec.Proc(spec, 4e-3, propagator='quadratic')
    assert proc.sampling.propagator == 'quadratic'
    assert dmc_exec.Proc(spec, 4e-3).sampling.propagator == 'linear'
    with pytest.raises(ValueError, match='propagator'):
        dmc_exec.Proc(spec, 1e-3, propagator='rk4')
    # the config key, and a config (a result file's proc_spec) without it
    cfg = proc.as_config()
    assert cfg['propagator'] == 'quadratic'
    assert dmc_exec.Proc.from_config(cfg) == proc
    old = {k: v for k, v in cfg.items() if k != 'propagator'}
    assert dmc_exec.Proc.from_config(old).propagator == 'linear'
    # (a linear procedure's config is what it was before the option existed)
    assert 'propagator' not in dmc_exec.Proc(spec, 4e-3).as_config()
    assert dmc_exec.Proc.from_config(dict(old, propagator='linear')) == \
        dmc_exec.Proc(spec, 4e-3)
    with pytest.raises(ValueError, match='propagator'):
        dmc_exec.Proc.from_config(dict(cfg, propagator='cubic'))


def test_result_file_keeps_the_propagator(tmp_path):
    """proc_spec of a result file: 'quadratic' is written and read back; a
    linear procedure writes what it always wrote, and a file without the
    attribute loads as 'linear'."""
    from phd_qmclib_amd import mrbp_qmc
    from phd_qmclib_amd.mrbp_qmc import dmc_exec
    from phd_qmclib_amd.util import h5lite
    spec = mrbp_qmc.Spec(**MODEL)
    handler = dmc_exec.HDF5FileHandler(str(tmp_path / 'r.h5'), 'g')
    for name in ('quadratic', 'linear'):
        proc = dmc_exec.Proc(spec, 4e-3, propagator=name)
        with h5lite.open_file(tmp_path / f'{name}.h5', 'a') as fp:
            handler.save_proc(proc.as_config(), fp.require_group('proc_spec'))
        with h5lite.open_file(tmp_path / f'{name}.h5', 'r') as fp:
            group = fp.get('proc_spec')
            stored = dict(group.attrs.items()).get('propagator')
            if name == 'quadratic':
                assert stored in (name, name.encode())
            else:
                assert stored is None
            loaded = handler.load_proc(group)
            assert loaded == proc and loaded.propagator == name
