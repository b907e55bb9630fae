"""Model spec of the multi-rods Bloch-Phonon Bijl-Jastrow trial state.

Host-side mirror of the reference `mrbp_qmc.Spec` plugin surface
(reference: mrbp_qmc/model.py:134-400): the same constructor fields, defaults,
validation errors and derived-parameter tuples (`Params` :40-54, `OBFParams`
:57-65, `TBFParams` :68-75, `CFCSpec` :78-83), so an existing model definition
drops in unchanged.  The per-configuration functions (`wf_abs_log`, `energy`,
`drift`, `ith_energy_and_drift`) are served by the HIP engine through
`core_funcs` -- there is no CPU implementation in the product path.

Everything here runs once per `Spec`; it is double-precision scalar Python.
"""
import typing as t
from math import atan, ceil, cos, fabs, pi, sin, sqrt, tan

import attr
import numpy as np
from scipy.optimize import brentq

from .. import ideal

__all__ = ['CSWFOptimizer', 'CFCSpec', 'OBFParams', 'Params', 'Spec', 'TBFParams',
           'SysConfSlot', 'SysConfDistType', 'DIST_RAND', 'DIST_REGULAR',
           'core_funcs', 'PhysicalFuncs', 'pair_distribution_bins',
           'triple_distribution_bins']

import enum


@enum.unique
class SysConfSlot(enum.IntEnum):
    """Rows of a system configuration `sys_conf[2, N]`
    (reference: qmc_base/jastrow/model.py:31-38)."""
    pos = 0
    drift = 1


class SysConfDistType(enum.Enum):
    """Initial particle arrangements (qmc_base/jastrow/model.py:41-44)."""
    RANDOM = 'random'
    REGULAR = 'regular'


DIST_RAND = SysConfDistType.RANDOM
DIST_REGULAR = SysConfDistType.REGULAR


class Params(t.NamedTuple):
    """The model `Spec` flattened (mrbp_qmc/model.py:40-54)."""
    lattice_depth: float
    lattice_ratio: float
    interaction_strength: float
    boson_number: int
    supercell_size: float
    tbf_contact_cutoff: float
    defect_magnitude: float
    defects_sep: int
    well_width: float
    barrier_width: float
    is_free: bool
    is_ideal: bool


class OBFParams(t.NamedTuple):
    """One-body (Kronig-Penney) factor parameters (mrbp_qmc/model.py:57-65)."""
    lattice_depth: float
    lattice_ratio: float
    well_width: float
    barrier_width: float
    param_e0: float
    param_k1: float
    param_kp1: float


class TBFParams(t.NamedTuple):
    """Two-body (phonon-matched) factor parameters (mrbp_qmc/model.py:68-75)."""
    supercell_size: float
    tbf_contact_cutoff: float
    param_k2: float
    param_beta: float
    param_r_off: float
    param_am: float


class CFCSpec(t.NamedTuple):
    """What the core functions need (mrbp_qmc/model.py:78-83)."""
    model_params: Params
    obf_params: OBFParams
    tbf_params: TBFParams


def _as_int(value):
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        return int(value)
    return value


def _opt(fn):
    return lambda v: None if v is None else fn(v)


def _check_cutoff(inst, attribute, value):
    # mrbp_qmc/model.py:95-107
    if not fabs(value) <= fabs(inst.supercell_size / 2):
        raise ValueError("parameter value 'rm' out of domain")


def _check_num_defects(inst, attribute, value):
    # mrbp_qmc/model.py:111-129
    if value is None:
        return
    if not isinstance(value, int):
        raise TypeError("'num_defects' must be an int")
    if value < 0:
        raise ValueError("number of defects can't be negative")
    num_sites = int(ceil(inst.supercell_size))
    if value and (num_sites % value):
        raise ValueError(f"the specified number of defects ({value:d}) "
                         f"can't be evenly distributed in the lattice")


@attr.s(auto_attribs=True, frozen=True)
class Spec:
    """Parameters of a 1D Bose gas in a multi-rods lattice with contact
    repulsion and a Bijl-Jastrow trial wave function
    (mrbp_qmc/model.py:134-171)."""

    #: Barrier height V0 of the Kronig-Penney lattice.
    lattice_depth: float = attr.ib(converter=float)
    #: Barrier width / well width.
    lattice_ratio: float = attr.ib(converter=float)
    #: Contact interaction strength g.
    interaction_strength: float = attr.ib(converter=float)
    #: Number of bosons N.
    boson_number: int = attr.ib(converter=_as_int,
                                validator=attr.validators.instance_of(int))
    #: Length L of the periodic simulation box (lattice periods).
    supercell_size: float = attr.ib(converter=float)
    #: Matching distance rm of the two-body factor (variational parameter).
    tbf_contact_cutoff: float = attr.ib(converter=float,
                                        validator=_check_cutoff)
    #: Number of evenly spaced lattice defects.
    num_defects: t.Optional[int] = attr.ib(default=None,
                                           converter=_opt(_as_int),
                                           validator=_check_num_defects)
    #: Barrier height inside a defect cell.
    defect_magnitude: t.Optional[float] = attr.ib(default=None,
                                                  converter=_opt(float))

    def __attrs_post_init__(self):
        # Defaults of the defect fields (mrbp_qmc/model.py:174-196).
        v0 = self.lattice_depth
        nd, dm = self.num_defects, self.defect_magnitude
        if nd is None and dm is None:
            nd, dm = 0, v0
        elif nd is None:
            nd, dm = 0, v0
        else:
            dm = dm if nd else v0
            if dm is None:
                # the reference compares None > float here and raises
                raise TypeError("'defect_magnitude' is required when "
                                "'num_defects' is nonzero")
            if dm > v0:
                raise ValueError("Defect magnitude can't be greater than "
                                 "the lattice depth.")
        object.__setattr__(self, 'num_defects', nd)
        object.__setattr__(self, 'defect_magnitude', dm)

    # -- geometry ---------------------------------------------------------
    @property
    def boundaries(self):
        return 0., 1. * self.supercell_size

    @property
    def well_width(self):
        return 1 / (1 + self.lattice_ratio)

    @property
    def barrier_width(self):
        return self.lattice_ratio / (1 + self.lattice_ratio)

    @property
    def is_free(self):
        """No external potential (mrbp_qmc/model.py:216-226)."""
        return self.lattice_depth <= 1e-10 or self.lattice_ratio <= 1e-10

    @property
    def is_ideal(self):
        """No interactions (mrbp_qmc/model.py:228-235)."""
        return self.interaction_strength <= 1e-10

    @property
    def sys_conf_shape(self):
        return len(SysConfSlot), self.boson_number

    def get_sys_conf_buffer(self):
        return np.zeros(self.sys_conf_shape, dtype=np.float64)

    def init_get_sys_conf(self, dist_type=DIST_RAND, offset=None):
        """A configuration with random or regular positions
        (mrbp_qmc/model.py:248-273); uses `numpy.random` like the reference."""
        n, L = self.boson_number, self.supercell_size
        z_min, _ = self.boundaries
        offset = offset or 0.
        if dist_type is DIST_RAND:
            spread = L * np.random.random_sample(n)
        elif dist_type is DIST_REGULAR:
            spread = np.linspace(0, L, n, endpoint=False)
        else:
            raise ValueError("unrecognized '{}' dist_type".format(dist_type))
        sys_conf = self.get_sys_conf_buffer()
        sys_conf[SysConfSlot.pos, :] = z_min + (offset + spread) % L
        return sys_conf

    # -- derived parameters -----------------------------------------------
    @property
    def params(self):
        num_sites = int(ceil(self.supercell_size))
        nd = self.num_defects
        defects_sep = 1 if not nd else int(num_sites // nd)
        return Params(self.lattice_depth, self.lattice_ratio,
                      self.interaction_strength, self.boson_number,
                      self.supercell_size, self.tbf_contact_cutoff,
                      self.defect_magnitude, defects_sep, self.well_width,
                      self.barrier_width, self.is_free, self.is_ideal)

    @property
    def obf_params(self):
        """e0 = lowest band edge, k1 = sqrt(e0), kp1 = sqrt(V0 - e0)
        (mrbp_qmc/model.py:298-315)."""
        v0, r = self.lattice_depth, self.lattice_ratio
        e0 = float(ideal.eigen_energy(v0, r))
        return OBFParams(v0, r, self.well_width, self.barrier_width,
                         param_e0=e0, param_k1=sqrt(e0),
                         param_kp1=sqrt(v0 - e0))

    @property
    def tbf_params(self):
        """Match the short-range cos(k2 (r - r_off)) solution of the two-body
        problem to the phononic tail sin(pi r / L)^beta at r = rm
        (mrbp_qmc/model.py:318-393)."""
        g, n, L = self.interaction_strength, self.boson_number, \
            self.supercell_size
        rm = self.tbf_contact_cutoff
        if not fabs(rm) <= fabs(L / 2):
            raise ValueError("parameter value 'rm' out of domain")
        if g == 0:
            return TBFParams(L, rm, param_k2=0., param_beta=0.,
                             param_r_off=1 / 2 * L, param_am=1.0)

        gamma = 0.5 * (L / n) ** 2 * g          # Lieb-Liniger gamma
        a1d = 2.0 / (gamma * n)                 # 1D scattering length / L
        rm /= L                                 # box units from here on

        def beta_rm(u):
            if u == 0:
                return tan(pi * rm) / pi
            return (u / pi * (rm - u * a1d * tan(u)) * tan(pi * rm) /
                    (u * a1d + rm * tan(u)))

        def local_energy_mismatch(u, *_):
            b = beta_rm(u)
            return ((u * sin(pi * rm)) ** 2 + (pi * b * cos(pi * rm)) ** 2 -
                    pi ** 2 * b * rm)

        u = brentq(local_energy_mismatch, 0, pi / 2, args=(a1d,))
        b = beta_rm(u)
        k2 = u / rm
        k2r_off = atan(1 / (k2 * a1d))
        beta = b / rm
        r_off = k2r_off / k2
        am = sin(pi * rm) ** beta / cos(u - k2r_off)
        return TBFParams(L, self.tbf_contact_cutoff, param_k2=k2 / L,
                         param_beta=beta, param_r_off=r_off * L, param_am=am)

    @property
    def cfc_spec(self):
        return CFCSpec(self.params, self.obf_params, self.tbf_params)


class _CoreFuncs:
    """Per-configuration functions of the model, with the call signatures of
    the reference's `mrbp_qmc.core_funcs` (qmc_base/jastrow/model.py:298-366,
    476-564, 756-773, 793-854).  Each call runs the HIP pair-sum kernel on
    the current device through the C-ABI; the engine for a given parameter
    set is created lazily and cached."""

    def __init__(self):
        self._engines = {}

    def _engine(self, model_params, obf_params, tbf_params):
        from ..engine import ModelEngine
        key = (tuple(model_params), tuple(obf_params), tuple(tbf_params))
        eng = self._engines.get(key)
        if eng is None:
            if len(self._engines) > 16:
                self._engines.clear()
            eng = ModelEngine(CFCSpec(model_params, obf_params, tbf_params))
            self._engines[key] = eng
        return eng

    def _eval(self, sys_conf, model_params, obf_params, tbf_params):
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        eng = self._engine(model_params, obf_params, tbf_params)
        return eng.evaluate(sys_conf[SysConfSlot.pos][np.newaxis, :])

    def wf_abs_log(self, sys_conf, model_params, obf_params, tbf_params):
        return float(self._eval(sys_conf, model_params, obf_params,
                                tbf_params).wf_abs_log[0])

    def energy(self, sys_conf, model_params, obf_params, tbf_params):
        return float(self._eval(sys_conf, model_params, obf_params,
                                tbf_params).energy[0])

    def drift(self, sys_conf, model_params, obf_params, tbf_params,
              result=None):
        out = self._eval(sys_conf, model_params, obf_params, tbf_params)
        if result is None:
            result = np.zeros_like(np.asarray(sys_conf, dtype=np.float64))
        result[SysConfSlot.pos, :] = np.asarray(sys_conf)[SysConfSlot.pos, :]
        result[SysConfSlot.drift, :] = out.drift[0]
        return result

    def ith_energy_and_drift(self, i_, sys_conf, model_params, obf_params,
                             tbf_params):
        out = self._eval(sys_conf, model_params, obf_params, tbf_params)
        return float(out.ith_energy[0, i_]), float(out.drift[0, i_])

    def ith_energy(self, i_, sys_conf, model_params, obf_params, tbf_params):
        return self.ith_energy_and_drift(i_, sys_conf, model_params,
                                         obf_params, tbf_params)[0]

    def ith_drift(self, i_, sys_conf, model_params, obf_params, tbf_params):
        return self.ith_energy_and_drift(i_, sys_conf, model_params,
                                         obf_params, tbf_params)[1]


    def ith_one_body_density(self, i_, sz, sys_conf, model_params, obf_params,
                             tbf_params):
        """The term of particle `i_` in the one-body density matrix at the
        shift `sz` (qmc_base/jastrow/model.py:859-930)."""
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        eng = self._engine(model_params, obf_params, tbf_params)
        _, ith = eng.one_body_density(
            sys_conf[SysConfSlot.pos][np.newaxis, :], [float(sz)], ith=True)
        return float(ith[0, 0, i_])

    def one_body_density(self, sz, sys_conf, model_params, obf_params,
                         tbf_params):
        """One-body density matrix g1(sz) of one configuration
        (qmc_base/jastrow/model.py:932-965)."""
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        eng = self._engine(model_params, obf_params, tbf_params)
        g1 = eng.one_body_density(sys_conf[SysConfSlot.pos][np.newaxis, :],
                                  [float(sz)])
        return float(g1[0, 0])


core_funcs = _CoreFuncs()


@attr.s(auto_attribs=True, frozen=True)
class PhysicalFuncs:
    """Functions to calculate the main physical properties of the model over
    batches of configurations (reference: qmc_base/jastrow/model.py:1007-1122,
    mrbp_qmc/model.py:801-815).  The members broadcast as the reference's
    generalised ufuncs do:

        wf_abs_log(sys_conf)              (ns,nop)->()
        energy(sys_conf)                  (ns,nop)->()
        one_body_density(sz, sys_conf)    (),(ns,nop)->()
        pair_distribution(num_bins, sys_conf)  (ns,nop)->(B)
        triple_distribution(num_bins, sys_conf)  (ns,nop)->(B)
        energy_parts(sys_conf, contact_ranges)   (ns,nop)->(4+K)
        renyi_swap(lengths, sys_conf)     (2,ns,nop)->(K)
        renyi_region_swap(regions, sys_conf)  (2,ns,nop)->(K)
        particle_swap(sys_conf)           (2,ns,nop)->()
        one_body_matrix(num_points, sys_conf)  (ns,nop)->(M,M)
        fourier_density(kz_set, sys_conf) (nkz),(ns,nop)->(nkz)   complex

    The loop dimensions broadcast as NumPy's; the whole broadcast batch goes to
    the device in one call (one call per distinct set of shifts for
    `one_body_density`).  `fourier_density` is N nkz sines and cosines per
    configuration and stays on the host in NumPy.  Nothing touches the GPU
    until a member is called."""

    cfc_spec_nt: CFCSpec

    @classmethod
    def from_model_spec(cls, model_spec: Spec):
        """Builds the functions for the given model Spec."""
        return cls(model_spec.cfc_spec)

    @property
    def core_funcs(self):
        """The core functions of the model."""
        return core_funcs

    def _engine(self):
        return core_funcs._engine(*self.cfc_spec_nt)

    @staticmethod
    def _conf_batch(sys_conf):
        """sys_conf[..., ns, nop] -> (loop shape, pos[nconf, nop])."""
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        if sys_conf.ndim < 2:
            raise ValueError('sys_conf must have the core shape (ns, nop)')
        pos = sys_conf[..., SysConfSlot.pos, :]
        return pos.shape[:-1], pos.reshape(-1, pos.shape[-1])

    def wf_abs_log(self, sys_conf):
        """Logarithm of the absolute value of the trial wave function."""
        loop, pos = self._conf_batch(sys_conf)
        out = self._engine().evaluate(pos).wf_abs_log
        return out.reshape(loop)[()]

    def energy(self, sys_conf):
        """Local energy."""
        loop, pos = self._conf_batch(sys_conf)
        out = self._engine().evaluate(pos).energy
        return out.reshape(loop)[()]

    def one_body_density(self, sz, sys_conf):
        """One-body density matrix."""
        sz = np.asarray(sz, dtype=np.float64)
        loop_c, pos = self._conf_batch(sys_conf)
        loop = np.broadcast_shapes(sz.shape, loop_c)
        # the distinct (shift, configuration) index pairs of the broadcast
        # batch: shifts x configurations evaluated once, then gathered
        sz_idx = np.broadcast_to(
            np.arange(sz.size).reshape(sz.shape), loop)
        conf_idx = np.broadcast_to(
            np.arange(pos.shape[0]).reshape(loop_c), loop)
        shifts, inv = np.unique(sz.reshape(-1), return_inverse=True)
        g1 = self._engine().one_body_density(pos, shifts)
        out = g1[conf_idx, inv.reshape(-1)[sz_idx]]
        return out[()]

    def pair_distribution(self, num_bins, sys_conf):
        """Pair distribution function g2(r_b) of every configuration at the
        `num_bins` bin centres of `pair_distribution_bins`: the histogram of
        the minimum-image pair distances (qmc_base/utils.py:35-51) times
        L / (N (N - 1) delta).  `num_bins` is a scalar (it fixes the core
        dimension B); the loop dimensions of sys_conf broadcast."""
        from ..engine import pair_distribution_norm
        loop, pos = self._conf_batch(sys_conf)
        counts = self._engine().pair_distribution(pos, num_bins)
        mp = self.cfc_spec_nt.model_params
        g2 = pair_distribution_norm(counts, mp.boson_number, mp.supercell_size)
        return g2.reshape(loop + g2.shape[-1:])

    def triple_distribution(self, num_bins, sys_conf, max_span=None):
        """Three-body distribution g3(d_b) of every configuration at the
        `num_bins` bin centres of `triple_distribution_bins`: the histogram of
        the triple spans (the shortest arc of the ring that holds the three
        particles) below `max_span` (in (0, L/2], None = L/2) over
        C(N,3) 3 (delta/L)^2 (2 b + 1), which is 1 on average for uncorrelated
        particles.  `num_bins` and `max_span` are scalars; the loop dimensions
        of sys_conf broadcast."""
        from ..engine import triple_distribution_norm
        loop, pos = self._conf_batch(sys_conf)
        counts = self._engine().triple_distribution(pos, num_bins, max_span)
        mp = self.cfc_spec_nt.model_params
        g3 = triple_distribution_norm(counts, mp.boson_number,
                                      mp.supercell_size, max_span)
        return g3.reshape(loop + g3.shape[-1:])

    def renyi_swap(self, lengths, sys_conf, origin=0.0):
        """Replica-swap ratio of the Renyi-2 entanglement entropy: for the two
        replicas sys_conf[..., 0, :, :] and sys_conf[..., 1, :, :] and every
        segment A_k = [origin, origin + lengths[k]) of the ring,
        |psi(R1') psi(R2') / (psi(R1) psi(R2))| with the particles inside A_k
        exchanged between the replicas, 0 where the two hold different numbers
        of particles there.  The mean over independent pairs drawn from
        |psi|^2 is exp(-S2(l_k)): psi is the trial wave function, so this is
        the variational S2 of the Bijl-Jastrow state.  `lengths` (each in
        (0, L)) and `origin` are shared by the batch; the loop dimensions of
        sys_conf in front of the replica axis broadcast.  A lattice user who
        wants segments of whole sites passes origin = -barrier_width / 2 (the
        cut in mid-barrier, the site convention of the site statistics) and
        lengths that are multiples of the lattice period."""
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        if sys_conf.ndim < 3 or sys_conf.shape[-3] != 2:
            raise ValueError('sys_conf must have the core shape (2, ns, nop)')
        loop, pos = self._conf_batch(sys_conf)
        _, log_ratio = self._engine().renyi_swap(pos, lengths, origin)
        swap = np.exp(np.clip(log_ratio, -700.0, 700.0))
        swap[np.isneginf(log_ratio)] = 0.0
        return swap.reshape(loop[:-1] + swap.shape[-1:])

    def renyi_region_swap(self, regions, sys_conf, origin=0.0):
        """Replica-swap ratio of regions made of up to two segments: as
        `renyi_swap`, for every region X_k = regions[k] = (l1, g, l2), the
        segments [origin, origin + l1) and [origin + l1 + g,
        origin + l1 + g + l2) of the ring (l2 = 0: the first alone), with the
        particles inside X_k exchanged between the replicas, 0 where the two
        hold different totals there.  The mean over independent pairs drawn
        from |psi|^2 is exp(-S2(X_k)), and S2(A) + S2(C) - S2(A u C) the
        Renyi-2 mutual information of the two segments (variational, of the
        Bijl-Jastrow state).  `regions` (l1 > 0, g >= 0, l2 >= 0,
        l1 + g + l2 < L) and `origin` are shared by the batch; the loop
        dimensions of sys_conf in front of the replica axis broadcast."""
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        if sys_conf.ndim < 3 or sys_conf.shape[-3] != 2:
            raise ValueError('sys_conf must have the core shape (2, ns, nop)')
        loop, pos = self._conf_batch(sys_conf)
        _, log_ratio = self._engine().renyi_region_swap(pos, regions, origin)
        swap = np.exp(np.clip(log_ratio, -700.0, 700.0))
        swap[np.isneginf(log_ratio)] = 0.0
        return swap.reshape(loop[:-1] + swap.shape[-1:])

    def particle_swap(self, sys_conf):
        """One-particle replica-swap ratio: for the two replicas
        sys_conf[..., 0, :, :] and sys_conf[..., 1, :, :], the average of
        |psi(R1') psi(R2') / (psi(R1) psi(R2))| over all N^2 exchanges of one
        particle of the first with one particle of the second (the order of
        the particles in a configuration does not matter).  The mean over
        independent pairs drawn from |psi|^2 is the purity Tr rho1^2 of the
        one-body density matrix (trace 1) and minus its logarithm the
        particle-partition Renyi-2 entropy at n = 1: psi is the trial wave
        function, so this is the variational purity of the Bijl-Jastrow state.
        The loop dimensions of sys_conf in front of the replica axis
        broadcast."""
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        if sys_conf.ndim < 3 or sys_conf.shape[-3] != 2:
            raise ValueError('sys_conf must have the core shape (2, ns, nop)')
        loop, pos = self._conf_batch(sys_conf)
        mean = self._engine().particle_swap(pos)
        return mean.reshape(loop[:-1])[()]

    def one_body_matrix(self, num_points, sys_conf):
        """The one-body density matrix of every configuration on the grid of
        `num_points` = M uniform cells of [0, L): element [a, c] is the sum
        over the particles in cell a of psi(.. z_i -> x_c ..) / psi(R), x_c
        the centre of cell c (`engine.one_body_matrix_points`).  Its average
        over |psi|^2 is int_{cell a} rho1(x, x_c) dx, whose eigenvalues are the
        occupations of the natural orbitals (`engine.natural_orbitals`).
        `num_points` is a scalar; the loop dimensions of sys_conf broadcast.
        Every configuration is a group of its own here (1024 of them to a
        call of the engine); `ModelEngine.one_body_matrix` sums a batch on the
        device."""
        from ..engine import MAX_OBDM_GRID_GROUPS as step
        loop, pos = self._conf_batch(sys_conf)
        eng = self._engine()
        sums = np.concatenate([
            eng.one_body_matrix(pos[c0:c0 + step], num_points,
                                num_groups=len(pos[c0:c0 + step]))[0]
            for c0 in range(0, max(len(pos), 1), step)])
        return sums.reshape(loop + sums.shape[-2:])

    def energy_parts(self, sys_conf, contact_ranges=()):
        """The local energy of every configuration in parts -> [..., 4 + K]:
        E, T = sum_i F_i^2 (F the drift), V = sum_i V(z_i), the remainder
        I = E - T - V, and the windowed contact C_k of every window in
        `contact_ranges` (`ModelEngine.energy_parts`).  `contact_ranges` is a
        sequence of at most 16 windows (it fixes the core dimension); the loop
        dimensions of sys_conf broadcast."""
        loop, pos = self._conf_batch(sys_conf)
        parts = self._engine().energy_parts(pos, contact_ranges)
        return parts.reshape(loop + parts.shape[-1:])

    def fourier_density(self, kz_set, sys_conf):
        """Fourier density component with momentum k: sum_i exp(i k z_i)."""
        kz_set = np.asarray(kz_set, dtype=np.float64)
        if kz_set.ndim < 1:
            raise ValueError('kz_set must have the core shape (nkz,)')
        sys_conf = np.asarray(sys_conf, dtype=np.float64)
        if sys_conf.ndim < 2:
            raise ValueError('sys_conf must have the core shape (ns, nop)')
        pos = sys_conf[..., SysConfSlot.pos, :]
        loop = np.broadcast_shapes(kz_set.shape[:-1], pos.shape[:-1])
        kz = np.broadcast_to(kz_set, loop + kz_set.shape[-1:])
        z = np.broadcast_to(pos, loop + pos.shape[-1:])
        ang = kz[..., :, np.newaxis] * z[..., np.newaxis, :]
        return np.cos(ang).sum(axis=-1) + 1j * np.sin(ang).sum(axis=-1)


def pair_distribution_bins(model_spec, num_bins):
    """Bin centres r_b = (b + 1/2) delta, delta = (L/2) / num_bins, of the
    pair distribution function of a model Spec (or CFCSpec) -> r[num_bins]."""
    from ..engine import pair_distribution_bins as bins
    mp = getattr(model_spec, 'model_params', model_spec)
    return bins(mp.supercell_size, num_bins)


def triple_distribution_bins(model_spec, num_bins, max_span=None):
    """Bin centres d_b = (b + 1/2) delta, delta = max_span / num_bins
    (max_span None = L/2), of the three-body distribution of a model Spec (or
    CFCSpec) -> d[num_bins]."""
    from ..engine import triple_distribution_bins as bins
    mp = getattr(model_spec, 'model_params', model_spec)
    return bins(mp.supercell_size, num_bins, max_span)


class CSWFOptimizer:
    """Correlated-sampling optimisation of the trial wave function: finds the
    `tbf_contact_cutoff` that minimises the (re-weighted) variance of the
    local energy over a fixed set of configurations (reference:
    mrbp_qmc/model.py:818-942, qmc_base/jastrow/model.py:1125-1206).

    The configuration set is uploaded to HBM once; every trial value of the
    variational parameter is one batched launch of the pair-sum kernel
    (wf_abs_log + energy of all configurations) with that parameter set's
    engine.  The reference's `use_threads` / `num_workers` (dask scheduler
    knobs) are accepted and ignored."""

    def __init__(self, spec: Spec, sys_conf_set, ini_wf_abs_log_set,
                 ref_energy: t.Optional[float] = None,
                 use_threads: bool = True,
                 num_workers: t.Optional[int] = None,
                 verbose: bool = False):
        self.spec = spec
        self.sys_conf_set = np.asarray(sys_conf_set, dtype=np.float64)
        self.ini_wf_abs_log_set = np.asarray(ini_wf_abs_log_set,
                                             dtype=np.float64)
        self.ref_energy = ref_energy
        self.use_threads = use_threads
        self.num_workers = num_workers
        self.verbose = verbose
        scs = self.sys_conf_set
        n = spec.boson_number
        if scs.ndim == 3 and scs.shape[1:] == (len(SysConfSlot), n):
            pos = scs[:, SysConfSlot.pos, :]
        elif scs.ndim == 2 and scs.shape[1] == n:
            pos = scs
        else:
            raise ValueError('sys_conf_set must have shape (nconf, 2, '
                             'boson_number) or (nconf, boson_number)')
        if self.ini_wf_abs_log_set.shape != (pos.shape[0],):
            raise ValueError('ini_wf_abs_log_set must have one value per '
                             'configuration')
        # wf_abs_log and energy are symmetric in the particles: sorted
        # positions make the short-range branch of the kernel wave-uniform
        self._pos = np.sort(pos, axis=1)
        self._dev = None

    # -- device residency ---------------------------------------------
    def _buffers(self):
        if self._dev is None:
            from ..engine import DeviceBuffer
            W, n = self._pos.shape
            self._dev = (DeviceBuffer((W, n)).upload(self._pos),
                         DeviceBuffer((W,)), DeviceBuffer((W,)))
        return self._dev

    def close(self):
        if self._dev is not None:
            for b in self._dev:
                b.close()
            self._dev = None

    def update_spec(self, tbf_contact_cutoff: float):
        """The model spec with a new value of the variational parameter."""
        return attr.evolve(self.spec,
                           tbf_contact_cutoff=float(tbf_contact_cutoff))

    def wf_abs_log_and_energy_set(self, cfc_spec: CFCSpec):
        """wf_abs_log and local energy of every configuration of the set
        under the given parameters."""
        from ..engine import ModelEngine
        pos_d, wf_d, en_d = self._buffers()
        eng = ModelEngine(cfc_spec, device=pos_d.device)
        try:
            eng.evaluate_dev(self._pos.shape[0], pos_d.ptr, wf_d.ptr,
                             en_d.ptr)
            eng.sync()
        finally:
            eng.close()
        return wf_d.download(), en_d.download()

    @staticmethod
    def weighed_variance(weights_log_set, energy_set, ref_energy=None):
        """Weighed variance of the energies
        (qmc_base/jastrow/model.py:1146-1164; the reference ignores
        `ref_energy` and uses the weighed mean)."""
        rel_weights = np.exp(weights_log_set - weights_log_set.max())
        weight_sum = rel_weights.sum()
        ref_energy = (rel_weights * energy_set).sum() / weight_sum
        e_diff = rel_weights * (energy_set - ref_energy) ** 2
        return e_diff.sum() / weight_sum

    def principal_function(self, tbf_contact_cutoff):
        """The weighed variance of the local energy for a trial cutoff."""
        cutoff = float(np.ravel(tbf_contact_cutoff)[0])
        cfc_spec = self.update_spec(cutoff).cfc_spec
        wf_set, energy_set = self.wf_abs_log_and_energy_set(cfc_spec)
        weights_log_set = 2 * (wf_set - self.ini_wf_abs_log_set)
        return self.weighed_variance(weights_log_set, energy_set)

    @property
    def principal_function_bounds(self):
        sc_size = self.spec.supercell_size
        return [(5e-2, (0.5 - 5e-3) * sc_size)]

    def exec(self, seed=None):
        """Runs the minimisation (scipy `differential_evolution`, as the
        reference) and returns the spec with the optimal cutoff."""
        from scipy.optimize import differential_evolution
        try:
            res = differential_evolution(self.principal_function,
                                         bounds=self.principal_function_bounds,
                                         disp=self.verbose, seed=seed)
        finally:
            self.close()
        opt_cutoff, = res.x
        return self.update_spec(opt_cutoff)
