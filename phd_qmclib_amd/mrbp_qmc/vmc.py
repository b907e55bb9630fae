"""VMC sampling of the Bloch-Phonon model on the GPU.

`Sampling` keeps the reference surface (mrbp_qmc/vmc.py:70-171): the same
attrs fields, `build_state`, `states`, `blocks`, `as_chain`,
`state_data_blocks`, `cfc_spec`, `tpf_params`; one Markov chain, arrays shaped
like the reference's.  `EnsembleSampling` is the extension that makes the GPU
worthwhile: W independent chains (Philox stream = chain index) advanced
together, yielding per-chain block sums.

Every step runs on the device through the C-ABI (vmc_block_kernel); there is
no CPU path.
"""
import typing as t
from math import pi, sqrt

import attr
import numpy as np

from .. import utils
from ..engine import (ModelEngine, VmcEnsemble, energy_components,
                      natural_orbitals,
                      one_body_matrix_points, pair_distribution_bins,
                      pair_distribution_norm, particle_entropy, renyi_entropy,
                      renyi_lengths, renyi_mutual_information, renyi_resolved,
                      triple_distribution_bins, triple_distribution_norm)
from ..qmc_base import vmc as vmc_base
from . import model

__all__ = ['CFCSpec', 'EnsembleSampling', 'Sampling', 'NDFSampling',
           'SSFEstSpec', 'SSFParams', 'StateError', 'TPFParams']

STAT_ACCEPTED = vmc_base.STAT_ACCEPTED
STAT_REJECTED = vmc_base.STAT_REJECTED


class TPFParams(t.NamedTuple):
    """Transition probability parameters (mrbp_qmc/vmc.py:29-38)."""
    boson_number: int
    move_spread: float
    lower_bound: float
    upper_bound: float


class SSFParams(t.NamedTuple):
    num_modes: int
    supercell_size: float
    assume_none: bool = False


class CFCSpec(t.NamedTuple):
    model_params: model.Params
    obf_params: model.OBFParams
    tbf_params: model.TBFParams
    tpf_params: TPFParams
    ssf_params: t.Optional[SSFParams] = None


class StateError(ValueError):
    """Flags errors related to the handling of a VMC state."""


@attr.s(auto_attribs=True)
class SSFEstSpec:
    """Structure factor estimator spec (mrbp_qmc/vmc.py:61-66)."""
    num_modes: int


def _fourier_density(momenta, pos):
    """S(k) parts of one configuration (qmc_base/jastrow/model.py:977-1002,
    jastrow/vmc.py:340-349): [num_modes, 3] = |rho_k|^2, Re rho_k, Im rho_k.
    Host-side estimator over device-generated configurations."""
    ph = momenta[:, None] * pos[None, :]
    re, im = np.cos(ph).sum(axis=1), np.sin(ph).sum(axis=1)
    return np.stack([re * re + im * im, re, im], axis=1)


@attr.s(auto_attribs=True, frozen=True)
class Sampling:
    """The spec of a (single chain) VMC sampling, uniform proposal."""

    model_spec: model.Spec
    move_spread: float
    rng_seed: t.Optional[int] = attr.ib(default=None)
    ssf_est_spec: t.Optional[SSFEstSpec] = None

    _gaussian: t.ClassVar[bool] = False

    def __attrs_post_init__(self):
        if self.rng_seed is None:
            object.__setattr__(self, 'rng_seed',
                               int(utils.get_random_rng_seed()))

    # -- parameters (mrbp_qmc/vmc.py:88-143) -----------------------------------
    @property
    def tpf_params(self):
        z_min, z_max = self.model_spec.boundaries
        return TPFParams(self.model_spec.boson_number, self.move_spread,
                         z_min, z_max)

    @property
    def ssf_params(self):
        L = self.model_spec.supercell_size
        if self.ssf_est_spec is None:
            return SSFParams(1, L, assume_none=True)
        return SSFParams(self.ssf_est_spec.num_modes, L, assume_none=False)

    @property
    def cfc_spec(self) -> CFCSpec:
        ms = self.model_spec
        return CFCSpec(ms.params, ms.obf_params, ms.tbf_params,
                       self.tpf_params, self.ssf_params)

    @property
    def ssf_momenta(self):
        if self.ssf_est_spec is None:
            raise TypeError('the static structure factor spec has no been '
                            'specified')
        return (np.arange(self.ssf_est_spec.num_modes) * 2 * pi /
                self.model_spec.supercell_size)

    @property
    def core_funcs(self):
        return model.core_funcs

    # -- engine plumbing ----------------------------------------------------------
    def _proposal_width(self):
        return self.move_spread

    def _engine(self) -> ModelEngine:
        return ModelEngine(self.model_spec.cfc_spec)

    def build_state(self, sys_conf: np.ndarray) -> vmc_base.State:
        """mrbp_qmc/vmc.py:145-165."""
        sys_conf = np.asarray(sys_conf)
        if sys_conf.shape != self.model_spec.sys_conf_shape:
            raise StateError("sys_conf is not a valid configuration "
                             "of the model spec")
        wf = model.core_funcs.wf_abs_log(sys_conf, *self.model_spec.cfc_spec)
        return vmc_base.State(sys_conf, wf, STAT_ACCEPTED)

    def set_replay_tape(self, tape):
        """TEST ONLY: the next generator replays a recorded random stream
        instead of Philox -- tape[steps, N + 1] = the N proposal draws and
        the accept uniform of every step, in the reference's call order."""
        object.__setattr__(self, '_replay_tape',
                           None if tape is None else
                           np.ascontiguousarray(tape, dtype=np.float64))

    def _start(self, ini_state: vmc_base.State):
        eng = self._engine()
        ens = VmcEnsemble(eng, 1, self._proposal_width(), self.rng_seed,
                          gaussian=self._gaussian)
        pos = np.asarray(ini_state.sys_conf, dtype=np.float64)[model.SysConfSlot.pos]
        ens.set_state(pos[None, :])
        tape = getattr(self, '_replay_tape', None)
        if tape is not None:
            ens.set_tape(tape[None, :, :])
        return eng, ens

    def _state_from(self, ens, wf, move_stat):
        pos, _, _ = ens.get_state()
        sys_conf = self.model_spec.get_sys_conf_buffer()
        sys_conf[model.SysConfSlot.pos] = pos[0]
        return vmc_base.State(sys_conf, float(wf), int(move_stat))

    # -- generators (qmc_base/vmc.py:204-251) -----------------------------------
    def states(self, ini_state: vmc_base.State) -> t.Iterator[vmc_base.State]:
        """Yields a State per step; the first one is the initial state flagged
        ACCEPTED (qmc_base/vmc.py:616-618)."""
        eng, ens = self._start(ini_state)
        try:
            while True:
                out = ens.run_block(1, sums=False, series=True)
                yield self._state_from(ens, out['wf_abs_log'][0, 0],
                                       out['move_stat'][0, 0])
        finally:
            ens.close()
            eng.close()

    def blocks(self, num_steps_block: int, ini_state: vmc_base.State
               ) -> t.Iterator[vmc_base.SamplingBlock]:
        """qmc_base/vmc.py:686-768: per block the series wf_abs_log, energy,
        move_stat, the S(k) parts when requested, accept_rate, last_state."""
        ns = int(num_steps_block)
        eng, ens = self._start(ini_state)
        want_ssf = self.ssf_est_spec is not None
        momenta = self.ssf_momenta if want_ssf else None
        try:
            while True:
                out = ens.run_block(ns, series=True, confs=want_ssf)
                props = vmc_base.PropsData(out['wf_abs_log'][:, 0].copy(),
                                           out['energy'][:, 0].copy(),
                                           out['move_stat'][:, 0].copy())
                iter_ssf = None
                if want_ssf:
                    iter_ssf = np.stack([_fourier_density(momenta, p[0])
                                         for p in out['pos']])
                last = self._state_from(ens, props.wf_abs_log[-1],
                                        props.move_stat[-1])
                yield vmc_base.SamplingBlock(
                    props, iter_ssf, float(out['num_accepted'][0]) / ns, last)
        finally:
            ens.close()
            eng.close()

    def state_data_blocks(self, num_steps_block: int,
                          ini_state: vmc_base.State):
        """qmc_base/vmc.py:825-900: blocks that keep every configuration."""
        ns = int(num_steps_block)
        n = self.model_spec.boson_number
        eng, ens = self._start(ini_state)
        try:
            while True:
                out = ens.run_block(ns, series=True, confs=True)
                confs = np.zeros((ns,) + self.model_spec.sys_conf_shape)
                confs[:, model.SysConfSlot.pos, :] = out['pos'][:, 0, :n]
                props = vmc_base.PropsData(out['wf_abs_log'][:, 0].copy(),
                                           out['energy'][:, 0].copy(),
                                           out['move_stat'][:, 0].copy())
                last = vmc_base.State(confs[-1].copy(),
                                      float(props.wf_abs_log[-1]),
                                      int(props.move_stat[-1]))
                yield vmc_base.SamplingStateDataBlock(
                    confs, props, float(out['num_accepted'][0]) / ns, last)
        finally:
            ens.close()
            eng.close()

    def as_chain(self, num_steps: int, ini_state: vmc_base.State):
        """qmc_base/vmc.py:215-229."""
        if not num_steps >= 1:
            raise ValueError('num_steps must be nonzero and positive')
        gen = self.state_data_blocks(num_steps, ini_state)
        try:
            return next(gen)
        finally:
            gen.close()


@attr.s(auto_attribs=True, frozen=True)
class NDFSampling(Sampling):
    """Gaussian-proposal VMC (mrbp_qmc/vmc_ndf.py:23-51): `time_step` is the
    variance of the normal displacement."""

    model_spec: model.Spec
    time_step: float = None
    rng_seed: t.Optional[int] = attr.ib(default=None)
    ssf_est_spec: t.Optional[SSFEstSpec] = None
    move_spread: float = attr.ib(default=None, init=False)

    _gaussian: t.ClassVar[bool] = True

    def _proposal_width(self):
        return sqrt(self.time_step)


@attr.s(auto_attribs=True)
class EnsembleSampling:
    """W independent VMC chains advanced together on one GPU (extension of the
    reference's single-chain sampling: every chain is statistically the chain
    `Sampling` generates, with Philox stream = global chain index).
    `move='particle'`: a yield is a sweep of N single-particle moves instead
    (`engine.VmcEnsemble`)."""

    model_spec: model.Spec
    move_spread: float
    num_chains: int
    rng_seed: t.Optional[int] = None
    first_chain: int = 0          # global index of chain 0 (multi-GPU shard)
    device: t.Optional[int] = None
    stream: t.Optional[int] = None
    move: str = 'all'

    def __attrs_post_init__(self):
        if self.rng_seed is None:
            self.rng_seed = int(utils.get_random_rng_seed())
        self.engine = ModelEngine(self.model_spec.cfc_spec, device=self.device,
                                  stream=self.stream)
        self.ensemble = VmcEnsemble(self.engine, self.num_chains,
                                    self.move_spread, self.rng_seed,
                                    chain0=self.first_chain, move=self.move)

    def set_confs(self, pos):
        """pos[W, N] initial positions (log|psi| is evaluated on the device)."""
        self.ensemble.set_state(pos)

    def init_random(self, seed=None):
        rng = np.random.RandomState(seed)
        L = self.model_spec.supercell_size
        self.set_confs(L * rng.random_sample((self.num_chains,
                                               self.model_spec.boson_number)))

    def blocks(self, num_steps_block: int) -> t.Iterator[vmc_base.EnsembleBlock]:
        ns = int(num_steps_block)
        moves = self.model_spec.boson_number if self.move == 'particle' else 1
        while True:
            out = self.ensemble.run_block(ns)
            yield vmc_base.EnsembleBlock(out['sum_energy'], out['sum_energy2'],
                                         out['num_accepted'], ns, moves)

    def confs(self):
        """Current positions of every chain, [W, N] (VMC -> DMC hand-off)."""
        return self.ensemble.get_state()[0]

    def ssf(self, num_modes: int):
        """Static structure factor of the ensemble's current configurations,
        S(k_m) = (<|rho_k|^2> - <Re rho_k>^2 - <Im rho_k>^2) / N with the
        averages over the chains (qmc_exec/data/vmc.py SSFBlocks.mean), and
        the momenta k_m = 2 pi m / L -> (momenta[M], ssf[M])."""
        parts = self.ensemble.ssf_parts(num_modes)
        n, L = self.model_spec.boson_number, self.model_spec.supercell_size
        ssf = (parts[:, 0] - parts[:, 1] ** 2 - parts[:, 2] ** 2) / n
        return np.arange(int(num_modes)) * 2 * pi / L, ssf

    def one_body_density(self, shifts):
        """One-body density matrix g1(s) over the chains' current
        configurations -> (shifts, mean, stderr); computed on the rows resident
        on the device (no position is copied to the host).  The standard error
        is that of the mean over the chains."""
        shifts = np.ascontiguousarray(shifts, dtype=np.float64)
        parts = self.ensemble.obdm_parts(shifts)
        w = self.num_chains
        mean = parts[:, 0] / w
        var = np.maximum(parts[:, 1] / w - mean ** 2, 0.0)
        stderr = np.sqrt(var / max(w - 1, 1))
        return shifts, mean, stderr

    def pair_distribution(self, num_bins):
        """Pair distribution function g2(r) over the chains' current
        configurations -> (r, mean, stderr) at the bin centres; computed on the
        rows resident on the device (no position is copied to the host, the
        chains are not touched).  The standard error is that of the mean over
        the chains."""
        parts = self.ensemble.pair_dist_parts(num_bins)
        w = self.num_chains
        n, L = self.model_spec.boson_number, self.model_spec.supercell_size
        mean = parts[:, 0] / w
        var = np.maximum(parts[:, 1] / w - mean ** 2, 0.0)
        stderr = np.sqrt(var / max(w - 1, 1))
        return (pair_distribution_bins(L, num_bins),
                pair_distribution_norm(mean, n, L),
                pair_distribution_norm(stderr, n, L))

    def triple_distribution(self, num_bins, max_span=None):
        """Three-body distribution g3(d) over the chains' current
        configurations -> (d, mean, stderr) at the `num_bins` bin centres of
        [0, max_span) (max_span in (0, L/2], None = L/2); computed on the rows
        resident on the device after either move type (no position is copied
        to the host, the chains are not touched).  The standard error is that
        of the mean over the chains.  Its limit d -> 0 is the local g3."""
        parts = self.ensemble.triple_dist_parts(num_bins, max_span)
        w = self.num_chains
        n, L = self.model_spec.boson_number, self.model_spec.supercell_size
        mean = parts[:, 0] / w
        var = np.maximum(parts[:, 1] / w - mean ** 2, 0.0)
        stderr = np.sqrt(var / max(w - 1, 1))
        return (triple_distribution_bins(L, num_bins, max_span),
                triple_distribution_norm(mean, n, L, max_span),
                triple_distribution_norm(stderr, n, L, max_span))

    def energy_components(self, contact_ranges=None):
        """The energy of the chains' current configurations in parts
        -> `engine.EnergyComponents`: total, kinetic <sum_i F_i^2>, lattice
        <sum_i V(z_i)>, the remainder interaction = <E_L - T - V>, and for
        every window of `contact_ranges` (None: none) the contact
        <sum_{i<j} delta(z_ij)>, with coupling * contact a second, more
        precise estimate of the interaction energy that carries a bias of order
        range^2 (`engine.contact_extrapolate`).  Computed on the rows resident
        on the device after either move type (no position is copied to the
        host, the chains are not touched).  The errors are those of the mean
        over the chains."""
        parts = self.ensemble.energy_parts_parts(
            () if contact_ranges is None else contact_ranges)
        return energy_components(parts, self.num_chains,
                                 self.model_spec.cfc_spec, contact_ranges)

    def renyi_entropy(self, lengths, origin=0.0):
        """Renyi-2 entanglement entropy of the segments
        A_k = [origin, origin + lengths[k]) of the ring by replica swap over
        the chains' current configurations, the chains 2p and 2p + 1 being the
        two replicas of pair p (independent chains: an even `num_chains` is
        needed) -> (lengths, S2, S2_err, p_match): S2 = -ln(mean swap), its
        standard error over the pairs, and the fraction of pairs whose
        replicas hold the same number of particles in A_k (the others
        contribute swap = 0).  Computed on the rows resident on the device
        after either move type; the chains are not touched.  The chains sample
        the trial wave function, so S2 is the variational entropy of the
        Bijl-Jastrow state.  In a lattice origin = -barrier_width / 2 puts the
        cut in mid-barrier (segments of whole sites)."""
        ln = renyi_lengths(self.model_spec.supercell_size, lengths)
        parts = self.ensemble.renyi_parts(ln, origin)
        return (ln,) + renyi_entropy(parts, self.num_chains // 2)

    def renyi_entropy_resolved(self, lengths, origin=0.0, num_charges=None):
        """Charge-resolved Renyi-2 entropies of the segments
        A_k = [origin, origin + lengths[k]) by replica swap over the chains'
        current configurations, as `renyi_entropy` -> `engine.ResolvedRenyi`:
        S2, its error and the matched fraction, and for every particle number
        n < num_charges (None: all N + 1) of the segment the counting
        statistics p(n), <swap delta(n_A = n)> and the entropy S2(n) of that
        block of rho_A.  The resolution is done in the device reduction; the
        chains are not touched and an even `num_chains` is needed."""
        ln = renyi_lengths(self.model_spec.supercell_size, lengths)
        q = (self.model_spec.boson_number + 1 if num_charges is None
             else num_charges)
        regions = np.stack([ln, np.zeros_like(ln), np.zeros_like(ln)], axis=1)
        parts = self.ensemble.renyi_region_parts(regions, origin, q)
        return renyi_resolved(parts, self.num_chains // 2, q)

    def renyi_mutual_information(self, length, separations, origin=0.0,
                                 second_length=None):
        """Renyi-2 mutual information I2(A:C) = S2(A) + S2(C) - S2(A u C)
        between the segment A = [origin, origin + length) and the segments
        C_k = [origin + length + separations[k], ... + second_length) (None:
        `length`) by replica swap over the chains' current configurations
        -> (separations, I2, I2_err, S2_A, S2_C, S2_AC), S2_A a number and the
        others arrays over the separations.  One region call at `origin` gives
        A and every A u C_k; S2(C_k) takes a call at the origin of C_k (in a
        lattice with defects C is not a translate of A), one per distinct
        separation.  I2_err is the quadrature sum of the three errors and only
        indicative (`engine.renyi_mutual_information`).  The chains are not
        touched and an even `num_chains` is needed; S2 is variational, of the
        Bijl-Jastrow state."""
        l1 = float(length)
        l2 = l1 if second_length is None else float(second_length)
        sep = np.ascontiguousarray(separations, dtype=np.float64)
        if sep.ndim != 1 or sep.size < 1:
            raise ValueError('separations must be a 1-d array')
        regions = np.concatenate(
            [[[l1, 0.0, 0.0]],
             np.stack([np.full_like(sep, l1), sep, np.full_like(sep, l2)],
                      axis=1)])
        pairs = self.num_chains // 2
        s2, err, _ = renyi_entropy(
            self.ensemble.renyi_region_parts(regions, origin, 0), pairs)
        s_c, err_c = np.empty_like(sep), np.empty_like(sep)
        distinct, inverse = np.unique(sep, return_inverse=True)
        for j, g in enumerate(distinct):
            s, e, _ = renyi_entropy(
                self.ensemble.renyi_region_parts(
                    [[l2, 0.0, 0.0]], float(origin) + l1 + g, 0), pairs)
            s_c[inverse == j], err_c[inverse == j] = s[0], e[0]
        i2, i2_err = renyi_mutual_information(s2[0], s_c, s2[1:], err[0],
                                              err_c, err[1:])
        return sep, i2, i2_err, float(s2[0]), s_c, s2[1:]

    def particle_entropy(self):
        """Purity of the one-body density matrix and the one-particle
        (particle-partition, n = 1) Renyi-2 entropy by replica swap over the
        chains' current configurations, the chains 2p and 2p + 1 being the two
        replicas of pair p (independent chains: an even `num_chains` is
        needed) -> (S2, S2_err, purity, purity_err): purity = Tr rho1^2 =
        sum_k lambda_k^2 over the occupations of the natural orbitals (rho1 of
        trace 1), S2 = -ln purity, the errors over the pairs.  Every pair
        averages over all N^2 one-particle exchanges, so neither the position
        order of the resident rows nor an ordered start biases it; the chains
        are not touched.  The condensate fraction n0 / N = lambda_max obeys
        purity <= n0 / N <= sqrt(purity).  The chains sample the trial wave
        function, so this is the variational purity of the Bijl-Jastrow
        state."""
        parts = self.ensemble.particle_swap_parts()
        return particle_entropy(parts, self.num_chains // 2)

    def one_body_matrix(self, num_points, num_groups=32):
        """The one-body density matrix rho1(x, x') on a grid of `num_points`
        = M uniform cells over the chains' current configurations ->
        (x[M], `engine.NaturalOrbitals`): the cell centres and the matrix
        K[a, c] ~ int_{cell a} rho1(x, x_c) dx with its natural-orbital
        occupations, the condensate fraction lambda_0 / N, the purity and
        their jackknife errors over `num_groups` groups of chains (chain index
        mod `num_groups`; at most `num_chains`).  Computed on the rows resident
        on the device after either move type; the chains are not touched.  The
        chains sample the trial wave function, so this is the variational
        matrix of the Bijl-Jastrow state; `engine.momentum_from_matrix` gives
        n(k) of it."""
        spec = self.model_spec
        sums = self.ensemble.obdm_grid_parts(num_points, num_groups)
        g = sums.shape[0]
        wsum = np.array([len(range(i, self.num_chains, g)) for i in range(g)],
                        dtype=np.float64)
        return (one_body_matrix_points(spec.supercell_size, num_points),
                natural_orbitals(sums, wsum, spec.boson_number,
                                 spec.supercell_size))

    def close(self):
        self.ensemble.close()
        self.engine.close()
