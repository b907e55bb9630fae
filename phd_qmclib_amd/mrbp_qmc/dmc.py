"""DMC sampling of the Bloch-Phonon model on the GPU.

`Sampling` keeps the reference surface (mrbp_qmc/dmc.py:143-334): the same
attrs fields and defaults, `build_state`, `states`, `blocks`,
`state_data_blocks`, `cfc_spec`, `ddf_params`.  The population lives in HBM
behind a `qmc_dmc` handle; a block of time steps is enqueued without a host
round trip and only the per-step series come back.

`jit_parallel` is accepted for drop-in compatibility (there is no numba here);
`jit_fastmath` selects the engine's reduced-precision pair loop (float), as in
the reference only together with `jit_parallel`.  `fix_stale_energy` is an extension: False
reproduces the reference's branching weight, True uses the
parent's energy.  `propagator` is an extension too: 'linear' is the
reference's step, 'quadratic' the symmetric drift / diffusion split with error
O(dt^2) (`engine.DmcEnsemble`; `fix_stale_energy` has no effect with it).
The density / S(k) estimators (mixed and pure /
forward-walking) run on the device after every kept
time step and reproduce the reference's semantics, per-block resets included.
The other block estimators of `qmc_base.dmc_est.ESTIMATORS` are extensions
(the reference has none); their spec classes below say what each one is.
"""
import typing as t
from math import pi, sqrt

import attr
import numpy as np

from .. import utils
from ..engine import (DmcEnsemble, ModelEngine, dmc_propagator_code,
                      energy_components,
                      natural_orbitals, one_body_matrix_points,
                      pair_distribution_bins, pair_distribution_norm,
                      triple_distribution_bins, triple_distribution_norm)
from ..qmc_base import dmc as dmc_base, dmc_est
from . import model

__all__ = ['CFCSpec', 'DDFParams', 'DensityEstSpec', 'ISFEstSpec',
           'OBDMEstSpec', 'PairDistEstSpec',
           'Sampling', 'SiteEstSpec', 'SSFEstSpec', 'State', 'StateError',
           'SuperfluidEstSpec']

State = dmc_base.State


class StateError(ValueError):
    """Flags errors related to the handling of a DMC state."""


class DDFParams(t.NamedTuple):
    """Diffusion-and-drift parameters (mrbp_qmc/dmc.py:56-62)."""
    boson_number: int
    time_step: float
    sigma_spread: float
    lower_bound: float
    upper_bound: float


class DensityParams(t.NamedTuple):
    num_bins: int
    as_pure_est: bool
    pfw_num_time_steps: int
    assume_none: bool


class SSFParams(t.NamedTuple):
    num_modes: int
    as_pure_est: bool
    pfw_num_time_steps: int
    assume_none: bool


class CFCSpec(t.NamedTuple):
    model_params: model.Params
    obf_params: model.OBFParams
    tbf_params: model.TBFParams
    ddf_params: DDFParams
    density_params: t.Optional[DensityParams]
    ssf_params: t.Optional[SSFParams] = None


@attr.s(auto_attribs=True, frozen=True)
class DensityEstSpec:
    """mrbp_qmc/dmc.py:103-122."""
    num_bins: int
    as_pure_est: bool = True
    pfw_num_time_steps: int = 99999999


@attr.s(auto_attribs=True, frozen=True)
class SSFEstSpec:
    """mrbp_qmc/dmc.py:125-140."""
    num_modes: int
    as_pure_est: bool = True
    pfw_num_time_steps: t.Optional[int] = None

    def __attrs_post_init__(self):
        if self.pfw_num_time_steps is None:
            object.__setattr__(self, 'pfw_num_time_steps', 99999999)


@attr.s(auto_attribs=True, frozen=True)
class PairDistEstSpec:
    """Pair distribution g2(r) as a block estimator: `num_bins` uniform bins
    over [0, L/2] (1..256); pure (forward walking over `pfw_num_time_steps`
    steps through the cloning table, as that of S(k)) or mixed."""
    num_bins: int
    as_pure_est: bool = True
    pfw_num_time_steps: t.Optional[int] = None

    def __attrs_post_init__(self):
        if self.pfw_num_time_steps is None:
            object.__setattr__(self, 'pfw_num_time_steps', 99999999)


@attr.s(auto_attribs=True, frozen=True)
class SuperfluidEstSpec:
    """Centre-of-mass diffusion as a block estimator, pure, with the start of
    each block as its time origin: rho_s / rho is the large-lag limit of
    `engine.superfluid_ratio`.  It has no parameters."""


@attr.s(auto_attribs=True, frozen=True)
class ISFEstSpec:
    """Imaginary-time density correlations F(k, tau) = <rho_k(tau) rho_-k(0)>
    as a block estimator: `num_modes` momenta k_m = 2 pi m / L (1..64, the
    mode set of `SSFEstSpec`), `num_lags` lags (1..64) tau_l =
    l lag_stride dt, num_modes (num_lags + 2) <= 1024.  The start of each
    block is the time origin and the rows travel through the cloning table:
    the estimate is pure in the limit of a long block and is read at the last
    step of the block (`engine.intermediate_scattering`); lags close to the
    end of the block are mixed at their later end."""
    num_modes: int
    num_lags: int
    lag_stride: int = 1


def _shift_tuple(shifts):
    return tuple(float(s) for s in np.asarray(shifts, dtype=np.float64)
                 .reshape(-1))


@attr.s(auto_attribs=True, frozen=True)
class OBDMEstSpec:
    """One-body density matrix g1(s) as a block estimator, mixed (g1 is
    non-local: forward walking does not apply; extrapolate with the VMC value,
    2 DMC - VMC): 1..256 finite `shifts`, evaluated at every `eval_stride`-th
    step of a block, the first included (one evaluation costs
    len(shifts) N (N - 1) pair factors per walker, a time step N (N - 1) / 2
    pair terms)."""
    shifts: t.Tuple[float, ...] = attr.ib(converter=_shift_tuple)
    eval_stride: int = 1

    def __attrs_post_init__(self):
        if not 1 <= len(self.shifts) <= 256:
            raise ValueError('OBDMEstSpec: 1 to 256 shifts are needed')
        if not all(np.isfinite(self.shifts)):
            raise ValueError('OBDMEstSpec: the shifts must be finite')
        stride = self.eval_stride
        if isinstance(stride, bool) or stride != int(stride) or \
                not 1 <= int(stride) <= 2 ** 31 - 1:
            raise ValueError('OBDMEstSpec: eval_stride must be an integer in '
                             '[1, 2^31 - 1]')
        object.__setattr__(self, 'eval_stride', int(stride))


def _count(value, name):
    if isinstance(value, bool) or value != int(value):
        raise ValueError(f'SiteEstSpec: {name} must be an integer')
    return int(value)


@attr.s(auto_attribs=True, frozen=True)
class SiteEstSpec:
    """Site occupation statistics as a block estimator: per time step the
    `num_occupations` counts occ[n] of the lattice sites that hold n particles
    (the last collects n >= num_occupations - 1) and the `num_distances` sums
    corr[d] = sum_c n_c n_{c+d} over the sites, a site being a well with half
    a barrier on each side (`engine.site_statistics` turns them into P(n), the
    number variance and the connected correlation).  Pure (forward walking
    over `pfw_num_time_steps` steps through the cloning table, as that of
    g2(r); the operator is local and diagonal, so the pure estimate is exact)
    or mixed.  num_occupations >= 1, num_distances >= 0 and at most the
    supercell size, which must be an integer <= 512, and num_occupations +
    num_distances <= 256."""
    num_occupations: int
    num_distances: int = 0
    as_pure_est: bool = True
    pfw_num_time_steps: t.Optional[int] = None

    def __attrs_post_init__(self):
        P = _count(self.num_occupations, 'num_occupations')
        D = _count(self.num_distances, 'num_distances')
        if P < 1 or D < 0 or P + D > 256:
            raise ValueError('SiteEstSpec: num_occupations >= 1, '
                             'num_distances >= 0 and num_occupations + '
                             'num_distances <= 256 are needed')
        object.__setattr__(self, 'num_occupations', P)
        object.__setattr__(self, 'num_distances', D)
        if self.pfw_num_time_steps is None:
            object.__setattr__(self, 'pfw_num_time_steps', 99999999)
        elif _count(self.pfw_num_time_steps, 'pfw_num_time_steps') < 1:
            raise ValueError('SiteEstSpec: pfw_num_time_steps must be >= 1')


@attr.s(auto_attribs=True, frozen=True)
class Sampling:
    """A class to realize a DMC sampling (mrbp_qmc/dmc.py:143-160)."""

    model_spec: model.Spec
    time_step: float
    max_num_walkers: int
    target_num_walkers: int
    num_walkers_control_factor: t.Optional[float] = None
    rng_seed: t.Optional[int] = None
    density_est_spec: t.Optional[DensityEstSpec] = None
    ssf_est_spec: t.Optional[SSFEstSpec] = None
    jit_parallel: bool = True
    jit_fastmath: bool = False
    fix_stale_energy: bool = False
    # (keyword only: the positional order of the others is what it was)
    superfluid_est_spec: t.Optional[SuperfluidEstSpec] = attr.ib(
        default=None, kw_only=True)
    isf_est_spec: t.Optional[ISFEstSpec] = attr.ib(default=None, kw_only=True)
    obdm_est_spec: t.Optional[OBDMEstSpec] = attr.ib(default=None,
                                                     kw_only=True)
    site_est_spec: t.Optional[SiteEstSpec] = attr.ib(default=None,
                                                     kw_only=True)
    propagator: str = attr.ib(default='linear', kw_only=True)
    pair_dist_est_spec: t.Optional[PairDistEstSpec] = None

    def __attrs_post_init__(self):
        dmc_propagator_code(self.propagator)    # (ValueError if unknown)
        if self.rng_seed is None:
            object.__setattr__(self, 'rng_seed',
                               int(utils.get_random_rng_seed()))
        if self.num_walkers_control_factor is None:
            object.__setattr__(self, 'num_walkers_control_factor', 1.25e-1)

    # -- parameters (mrbp_qmc/dmc.py:172-236) ---------------------------------
    @property
    def ddf_params(self) -> DDFParams:
        z_min, z_max = self.model_spec.boundaries
        return DDFParams(self.model_spec.boson_number, self.time_step,
                         sqrt(2 * self.time_step), z_min, z_max)

    @property
    def density_params(self) -> DensityParams:
        """mrbp_qmc/dmc.py:187-204."""
        d = self.density_est_spec
        if d is None:
            return DensityParams(1, False, 1, True)
        return DensityParams(d.num_bins, d.as_pure_est, d.pfw_num_time_steps,
                             False)

    @property
    def ssf_params(self) -> SSFParams:
        """mrbp_qmc/dmc.py:206-225."""
        f = self.ssf_est_spec
        if f is None:
            return SSFParams(1, False, 1, True)
        return SSFParams(f.num_modes, f.as_pure_est, f.pfw_num_time_steps,
                         False)

    @property
    def density_bins_edges(self) -> np.ndarray:
        if self.density_est_spec is None:
            raise TypeError('the density spec has no been specified')
        return np.linspace(0, self.model_spec.supercell_size,
                           self.density_est_spec.num_bins + 1)

    @property
    def pair_dist_bins(self) -> np.ndarray:
        """Bin centres r_b of the pair distribution estimator."""
        if self.pair_dist_est_spec is None:
            raise TypeError('the pair distribution spec has not been '
                            'specified')
        return pair_distribution_bins(self.model_spec.supercell_size,
                                      self.pair_dist_est_spec.num_bins)

    @property
    def isf_momenta(self) -> np.ndarray:
        """Momenta k_m of the F(k, tau) estimator."""
        if self.isf_est_spec is None:
            raise TypeError('the F(k, tau) spec has not been specified')
        return (np.arange(self.isf_est_spec.num_modes) * 2 * pi /
                self.model_spec.supercell_size)

    @property
    def obdm_shifts(self) -> np.ndarray:
        """Shifts s_k of the one-body density matrix estimator."""
        if self.obdm_est_spec is None:
            raise TypeError('the one-body density spec has not been '
                            'specified')
        return np.array(self.obdm_est_spec.shifts, dtype=np.float64)

    @property
    def cfc_spec(self) -> CFCSpec:
        ms = self.model_spec
        return CFCSpec(ms.params, ms.obf_params, ms.tbf_params,
                       self.ddf_params, self.density_params, self.ssf_params)

    @property
    def state_confs_shape(self):
        return (self.max_num_walkers,) + self.model_spec.sys_conf_shape

    @property
    def state_props_shape(self):
        return self.max_num_walkers,

    @property
    def core_funcs(self):
        return model.core_funcs

    # -- engine plumbing --------------------------------------------------------
    def set_replay_tape(self, uniform, normal, n_uniform, n_normal):
        """TEST ONLY: the next generator replays recorded streams instead of
        Philox: the uniforms of the branching loop and the standard normals
        of the diffusion, with the number of draws of every time step."""
        if uniform is None:
            object.__setattr__(self, '_replay_tape', None)
            return
        u_off = np.concatenate([[0], np.cumsum(n_uniform)[:-1]])
        g_off = np.concatenate([[0], np.cumsum(n_normal)[:-1]])
        object.__setattr__(self, '_replay_tape',
                           (np.asarray(uniform, dtype=np.float64),
                            np.asarray(normal, dtype=np.float64),
                            u_off.astype(np.int64), g_off.astype(np.int64)))

    @property
    def fast_math_in_effect(self) -> bool:
        """`jit_fastmath` asks for the reduced-precision pair loop; as in the
        reference it only takes effect together with `jit_parallel`
        (mrbp_qmc/dmc.py:647-654: the (False, True) entry of the core
        functions table is built without fastmath)."""
        return bool(self.jit_parallel and self.jit_fastmath)

    def _new_ensemble(self, target=None, slot0=0, device=None, stream=None,
                      external_reduce=False):
        if self.fast_math_in_effect:
            # in the reference `fastmath` relaxes IEEE rules but still computes
            # in double; here it changes the precision CLASS of the pair loop:
            # say so every time
            import warnings
            warnings.warn(
                'jit_fastmath=True with jit_parallel=True runs the pair loop '
                'in float (fp32) on the device: local energy ~1e-7 relative, '
                'drift of a pair closer than ~1e-6 L loses its leading digits '
                '(DESIGN.md section 4, "Reduced precision"); single steps '
                'with this option are pinned against the reference and the '
                'fp64 oracle at 2e-5, long DMC runs only statistically',
                RuntimeWarning, stacklevel=3)
        eng = ModelEngine(self.model_spec.cfc_spec, device=device,
                          stream=stream, fast_math=self.fast_math_in_effect)
        ens = DmcEnsemble(eng, self.time_step, self.max_num_walkers,
                          target if target is not None
                          else self.target_num_walkers,
                          self.num_walkers_control_factor, self.rng_seed,
                          slot0=slot0, fix_stale_energy=self.fix_stale_energy,
                          external_reduce=external_reduce,
                          propagator=self.propagator)
        return eng, ens

    def _to_state(self, s) -> State:
        props = dmc_base.StateProps(s.energy, s.weight, s.mask)
        bspec = dmc_base.BranchingSpec(
            np.zeros(self.max_num_walkers, dtype=np.int64), s.cloning_ref)
        return State(s.confs, props, s.state_energy, s.state_weight,
                     s.num_walkers, s.ref_energy, s.accum_energy,
                     self.max_num_walkers, bspec)

    def build_state(self, sys_conf_set: np.ndarray,
                    ref_energy: t.Optional[float] = None) -> State:
        """mrbp_qmc/dmc.py:268-328: keep the last `target_num_walkers`
        configurations, evaluate energy + drift of each, unit weights, initial
        E_ref = mean energy unless given."""
        sys_conf_set = np.asarray(sys_conf_set)
        confs_shape = self.state_confs_shape
        if len(confs_shape) == len(sys_conf_set.shape):
            if confs_shape[1:] != sys_conf_set.shape[1:]:
                raise StateError("sys_conf_set is not a valid set of "
                                 "configurations of the model spec")
        sys_conf_set = sys_conf_set[-self.target_num_walkers:]
        nw = len(sys_conf_set)
        if nw > self.max_num_walkers:
            raise StateError('more initial configurations than '
                             'max_num_walkers')
        eng, ens = self._new_ensemble()
        try:
            ens.set_state(sys_conf_set[:, model.SysConfSlot.pos, :],
                          ref_energy)
            s = ens.get_state()
        finally:
            ens.close()
            eng.close()
        e = s.energy[:nw]
        w = s.weight[:nw]
        state_energy = float((e * w).sum())
        state_weight = float(w.sum())
        energy = state_energy / state_weight
        props = dmc_base.StateProps(s.energy, s.weight, s.mask)
        bspec = dmc_base.BranchingSpec(
            np.zeros(self.max_num_walkers, dtype=np.int64),
            np.zeros(self.max_num_walkers, dtype=np.int64))
        return State(s.confs, props, state_energy, state_weight, nw,
                     energy if ref_energy is None else ref_energy, energy,
                     self.max_num_walkers, bspec)

    def _start(self, ini_state: State, target=None):
        if ini_state.max_num_walkers != self.max_num_walkers:
            raise StateError('the state was built for a different '
                             'max_num_walkers')
        eng, ens = self._new_ensemble(target=target)
        nw = int(ini_state.num_walkers)
        ens.set_full_state(ini_state.confs[:nw], ini_state.props.energy[:nw],
                           ini_state.props.weight[:nw], ini_state.ref_energy,
                           slot_energy=ini_state.props.energy)
        tape = getattr(self, '_replay_tape', None)
        if tape is not None:
            ens.set_tape(*tape)
        return eng, ens

    # -- generators (qmc_base/dmc.py:311-364) ---------------------------------
    def states(self, ini_state: State) -> t.Iterator[State]:
        """One State per time step (the post-branching population)."""
        eng, ens = self._start(ini_state)
        try:
            while True:
                ens.run_block(1, read=False)
                yield self._to_state(ens.get_state())
        finally:
            ens.close()
            eng.close()

    def blocks(self, ini_state: State, num_time_steps_block: int,
               burn_in_blocks: int) -> t.Iterator[dmc_base.SamplingBlock]:
        """qmc_base/dmc.py:831-969.  `burn_in_blocks` only gates the
        estimators in the reference; the propagation is identical."""
        nts = int(num_time_steps_block)
        eng, ens = self._start(ini_state)
        dp, sp = self.density_params, self.ssf_params
        # (S(k) and the density are one call of the ensemble, below)
        others = [est for est in dmc_est.ESTIMATORS if est.enable and
                  getattr(self, est.sampling_field) is not None]
        with_est = not (dp.assume_none and sp.assume_none) or bool(others)
        for est in others:
            est.enable(ens, getattr(self, est.sampling_field))
        if not (dp.assume_none and sp.assume_none):
            ens.set_estimators(
                0 if sp.assume_none else sp.num_modes, sp.as_pure_est,
                sp.pfw_num_time_steps,
                0 if dp.assume_none else dp.num_bins, dp.as_pure_est,
                dp.pfw_num_time_steps)
        block_idx = 0
        try:
            while True:
                iter_ssf = iter_density = None
                rows = {}
                if with_est:
                    # estimators only once the burn-in blocks are over
                    # (qmc_base/dmc.py:916, 928)
                    ser, iter_ssf, iter_density = ens.run_block_est(
                        nts, block_idx >= burn_in_blocks)
                    rows = {est.block_field: est.read(ens, nts)
                            for est in others}
                else:
                    ser = ens.run_block(nts)
                props = dmc_base.PropsData(ser.energy, ser.weight,
                                           ser.num_walkers, ser.ref_energy,
                                           ser.accum_energy)
                last = self._to_state(ens.get_state())
                yield dmc_base.SamplingBlock(props, iter_density, iter_ssf,
                                             last, **rows)
                block_idx += 1
        finally:
            ens.close()
            eng.close()

    def state_data_blocks(self, ini_state: State, num_time_steps_block: int
                          ) -> t.Iterator[dmc_base.SamplingStateDataBlock]:
        """qmc_base/dmc.py:988-1068; note the reference overrides the target
        population with the initial one here (:1008)."""
        nts = int(num_time_steps_block)
        eng, ens = self._start(ini_state, target=int(ini_state.num_walkers))
        maxw = self.max_num_walkers
        try:
            while True:
                confs = np.zeros((nts,) + self.state_confs_shape)
                en, wt = np.zeros((nts, maxw)), np.zeros((nts, maxw))
                mk = np.zeros((nts, maxw), dtype=bool)
                rows = []
                for k in range(nts):
                    ser = ens.run_block(1)
                    s = ens.get_state()
                    confs[k], en[k], wt[k], mk[k] = (s.confs, s.energy,
                                                     s.weight, s.mask)
                    rows.append(ser)
                props = dmc_base.PropsData(
                    *[np.concatenate([getattr(r, f) for r in rows])
                      for f in dmc_base.PropsData._fields])
                yield dmc_base.SamplingStateDataBlock(
                    confs, dmc_base.StateProps(en, wt, mk), props)
        finally:
            ens.close()
            eng.close()

    def one_body_density(self, state: State, shifts):
        """Mixed estimate of the one-body density matrix over the live walkers
        of a State: sum_w W_w g1_w(s) / sum_w W_w (g1 of
        qmc_base/jastrow/model.py:932-965 per walker).  The positions of the
        `num_walkers` live walkers are uploaded once; the weighted reduction
        runs on the device -> g1[nshift]."""
        nw = int(state.num_walkers)
        confs = np.asarray(state.confs, dtype=np.float64)
        pos = confs[:nw, model.SysConfSlot.pos, :]
        weight = np.asarray(state.props.weight, dtype=np.float64)[:nw]
        eng = model.core_funcs._engine(*self.model_spec.cfc_spec)
        return eng.one_body_density_weighted(pos, weight, shifts)

    def pair_distribution(self, state: State, num_bins):
        """Mixed estimate of the pair distribution function over the live
        walkers of a State: sum_w W_w H_w / sum_w W_w, H the pair-distance
        histogram of a walker (distances of qmc_base/utils.py:35-51), normalised
        to g2 -> (r[num_bins], g2[num_bins]).  Slots beyond `num_walkers` do
        not count.  The positions are uploaded once; the weighted reduction
        runs on the device."""
        nw = int(state.num_walkers)
        confs = np.asarray(state.confs, dtype=np.float64)
        pos = confs[:nw, model.SysConfSlot.pos, :]
        weight = np.asarray(state.props.weight, dtype=np.float64)[:nw]
        eng = model.core_funcs._engine(*self.model_spec.cfc_spec)
        spec = self.model_spec
        hist = eng.pair_distribution_weighted(pos, weight, num_bins)
        return (pair_distribution_bins(spec.supercell_size, num_bins),
                pair_distribution_norm(hist, spec.boson_number,
                                       spec.supercell_size))

    def energy_components(self, state: State, contact_ranges=None):
        """Mixed estimate of the energy in parts over the live walkers of a
        State -> `engine.EnergyComponents`: every entry is
        sum_w W_w x_w / sum_w W_w with the weights `state.props.weight`; slots
        at or beyond `num_walkers` do not count.  The positions are uploaded
        once; the weighted reduction runs on the device.  `contact_ranges`
        None: no contact window.

        What is exact and what is not:
          total        the DMC energy: the mixed estimate of H is exact for the
                       ground state.
          lattice      a mixed estimate of a local operator, biased at first
                       order in the error of the trial function.  The pure
                       value is already available from the pure density
                       histogram: sum over bins of n(x) V(x), with bins aligned
                       to the barrier edges.
          kinetic, interaction, contact   mixed estimates; extrapolate them
                       with the VMC values of
                       `vmc.EnsembleSampling.energy_components`: 2 DMC - VMC.
        The errors are those of the weighted mean over the walkers of this one
        State, taken as independent: walkers share ancestors, so they are a
        lower bound."""
        nw = int(state.num_walkers)
        confs = np.asarray(state.confs, dtype=np.float64)
        pos = confs[:nw, model.SysConfSlot.pos, :]
        weight = np.asarray(state.props.weight, dtype=np.float64)[:nw]
        cfc = self.model_spec.cfc_spec
        eng = model.core_funcs._engine(*cfc)
        rg = () if contact_ranges is None else contact_ranges
        sums, wsum = eng.energy_parts_weighted(pos, weight, rg)
        return energy_components(sums, wsum, cfc, contact_ranges,
                                 num_confs=nw)

    def triple_distribution(self, state: State, num_bins, max_span=None):
        """Mixed estimate of the three-body distribution over the live
        walkers of a State: sum_w W_w T_w / sum_w W_w, T the triple-span
        histogram of a walker, normalised to g3 -> (d[num_bins], g3[num_bins])
        for spans below `max_span` (in (0, L/2], None = L/2).  Slots beyond
        `num_walkers` do not count.  The positions are uploaded once; the
        weighted reduction runs on the device.  Extrapolate with the VMC value
        of `vmc.EnsembleSampling.triple_distribution`: 2 DMC - VMC."""
        nw = int(state.num_walkers)
        confs = np.asarray(state.confs, dtype=np.float64)
        pos = confs[:nw, model.SysConfSlot.pos, :]
        weight = np.asarray(state.props.weight, dtype=np.float64)[:nw]
        eng = model.core_funcs._engine(*self.model_spec.cfc_spec)
        spec = self.model_spec
        hist = eng.triple_distribution_weighted(pos, weight, num_bins,
                                                max_span)
        return (triple_distribution_bins(spec.supercell_size, num_bins,
                                         max_span),
                triple_distribution_norm(hist, spec.boson_number,
                                         spec.supercell_size, max_span))

    def one_body_matrix(self, state: State, num_points, num_groups=32):
        """Mixed estimate of the one-body density matrix rho1(x, x') on a grid
        of `num_points` = M uniform cells over the live walkers of a State
        with their weights -> (x[M], `engine.NaturalOrbitals`): the cell
        centres and K[a, c] = sum_w W_w R_w[a, c] / sum_w W_w with its
        natural-orbital occupations, condensate fraction, purity and their
        jackknife errors over `num_groups` groups of walkers (walker index mod
        `num_groups`; at most `num_walkers`).  Slots beyond `num_walkers` do
        not count.  The positions are uploaded once; the weighted sums run on
        the device.  A mixed estimate: extrapolate as 2 K_DMC - K_VMC on
        `matrix`, with `vmc.EnsembleSampling.one_body_matrix`, BEFORE
        diagonalising (the eigenvalues are not linear in the matrix)."""
        nw = int(state.num_walkers)
        confs = np.asarray(state.confs, dtype=np.float64)
        pos = confs[:nw, model.SysConfSlot.pos, :]
        weight = np.asarray(state.props.weight, dtype=np.float64)[:nw]
        eng = model.core_funcs._engine(*self.model_spec.cfc_spec)
        spec = self.model_spec
        sums, wsum = eng.one_body_matrix(pos, num_points, num_groups, weight)
        return (one_body_matrix_points(spec.supercell_size, num_points),
                natural_orbitals(sums, wsum, spec.boson_number,
                                 spec.supercell_size))

    @property
    def ssf_momenta(self):
        if self.ssf_est_spec is None:
            raise TypeError('the static structure factor spec has no been '
                            'specified')
        return (np.arange(self.ssf_est_spec.num_modes) * 2 * pi /
                self.model_spec.supercell_size)
