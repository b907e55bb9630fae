"""DMC block containers (reference: qmc_exec/data/dmc.py:24-318).

A DMC expectation value is a ratio of block totals, <O w> / <w>; its error
combines the reblocked variances of numerator, denominator and their product
(the reference's formula, restated in `PropBlocks.mean_error`).
"""
import typing as t

import attr
import numpy as np

from ...qmc_base import dmc_est
from ...stats import reblock

__all__ = ['CMDiffusionBlocks', 'DensityBlocks', 'EnergyBlocks',
           'ISFBlocks', 'NumWalkersBlocks', 'OBDMBlocks',
           'PairDistBlocks', 'PropBlocks',
           'SiteBlocks', 'SSFBlocks', 'SSFPartBlocks',
           'PropsDataBlocks', 'PropsDataSeries', 'SamplingData', 'UnWeightedPropBlocks',
           'WeightBlocks']


@attr.s(auto_attribs=True, frozen=True)
class PropBlocks:
    """Weighted block totals."""
    totals: np.ndarray
    weight_totals: t.Optional[np.ndarray]

    @property
    def reblock(self):
        return reblock.OTFObject.from_non_obj_data(self.totals)

    @property
    def weight_reblock(self):
        if self.weight_totals is None:
            return None
        return reblock.OTFObject.from_non_obj_data(self.weight_totals)

    @property
    def cross_weight_reblock(self):
        if self.weight_totals is None:
            return None
        return reblock.OTFObject.from_non_obj_data(self.totals *
                                                   self.weight_totals)

    @property
    def mean(self):
        w = self.weight_reblock
        return self.reblock.mean if w is None else self.reblock.mean / w.mean

    @property
    def mean_error(self):
        """qmc_exec/data/dmc.py:41-75."""
        ow = self.reblock
        ow_mean, ow_var, ow_eff = ow.mean, ow.var, ow.eff_size
        if self.weight_reblock is None:
            w_mean, w_var, oww_mean = 1., 0., ow_mean
            w_eff = oww_eff = 0.5
        else:
            w, oww = self.weight_reblock, self.cross_weight_reblock
            w_mean, w_var, oww_mean = w.mean, w.var, oww.mean
            w_eff, oww_eff = w.eff_size, oww.eff_size
        err_ow = ow_var / ow_mean ** 2
        err_w = w_var / w_mean ** 2
        err_oww = (oww_mean - ow_mean * w_mean) / (ow_mean * w_mean)
        return np.abs(self.mean) * np.sqrt(err_ow / ow_eff + err_w / w_eff -
                                           2 * err_oww / oww_eff)

    def __len__(self):
        return len(self.totals)

    def __add__(self, other):
        if not isinstance(other, PropBlocks):
            return NotImplemented
        return type(self)(
            np.concatenate((self.totals, other.totals), axis=0),
            np.concatenate((self.weight_totals, other.weight_totals), axis=0))


@attr.s(auto_attribs=True, frozen=True)
class UnWeightedPropBlocks:
    totals: np.ndarray

    @property
    def reblock(self):
        return reblock.OTFObject.from_non_obj_data(self.totals)

    @property
    def mean(self):
        return self.reblock.mean

    @property
    def mean_error(self):
        return self.reblock.mean_eff_error

    def __len__(self):
        return len(self.totals)

    def __add__(self, other):
        if not isinstance(other, UnWeightedPropBlocks):
            return NotImplemented
        return type(self)(np.concatenate((self.totals, other.totals), axis=0))


@attr.s(auto_attribs=True, frozen=True)
class NumWalkersBlocks(UnWeightedPropBlocks):
    totals: np.ndarray

    @classmethod
    def from_data(cls, data, reduce_data: bool = True):
        nw = np.asarray(data.num_walkers)
        return cls(nw.sum(axis=1) if reduce_data else nw)


@attr.s(auto_attribs=True, frozen=True)
class WeightBlocks(UnWeightedPropBlocks):
    totals: np.ndarray

    @classmethod
    def from_data(cls, data, reduce_data: bool = True):
        w = np.asarray(data.weight)
        return cls(w.sum(axis=1) if reduce_data else w)


@attr.s(auto_attribs=True, frozen=True)
class EnergyBlocks(PropBlocks):
    totals: np.ndarray
    weight_totals: np.ndarray

    @classmethod
    def from_data(cls, data, reduce_data: bool = True):
        e, w = np.asarray(data.energy), np.asarray(data.weight)
        if reduce_data:
            return cls(e.sum(axis=1), w.sum(axis=1))
        return cls(e, w)


def _est_totals(nts_block, data, weight, reduce_data, as_pure_est,
                pure_est_reduce_factor):
    """Block totals of an estimator (qmc_exec/data/dmc.py:329-371, 425-466):
    mixed estimators sum over the block, pure ones take the last time step."""
    data, weight = np.asarray(data), np.asarray(weight)
    if not as_pure_est:
        if reduce_data:
            return data.sum(axis=1), weight.sum(axis=1)[:, np.newaxis]
        return data, weight[:, np.newaxis]
    if reduce_data:
        return (data[:, nts_block - 1, :],
                weight[:, nts_block - 1][:, np.newaxis])
    return data, (weight * pure_est_reduce_factor)[:, np.newaxis]


@attr.s(auto_attribs=True, frozen=True)
class SetPropBlocks(PropBlocks):
    """Weighted block totals of a vector-valued property (one column per bin
    or momentum); statistics per column through `reblock.OTFSet`."""
    totals: np.ndarray
    weight_totals: np.ndarray

    @property
    def reblock(self):
        return reblock.OTFSet.from_non_obj_data(self.totals)

    @property
    def weight_reblock(self):
        if self.weight_totals is None:
            return None
        return reblock.OTFSet.from_non_obj_data(self.weight_totals)

    @property
    def cross_weight_reblock(self):
        if self.weight_totals is None:
            return None
        return reblock.OTFSet.from_non_obj_data(self.totals *
                                                self.weight_totals)


@attr.s(auto_attribs=True, frozen=True)
class DensityBlocks(SetPropBlocks):
    """Density data in blocks (qmc_exec/data/dmc.py:321-393)."""
    totals: np.ndarray
    weight_totals: np.ndarray

    @classmethod
    def from_data(cls, num_time_steps_block, density_data, props_data,
                  reduce_data=True, as_pure_est=True,
                  pure_est_reduce_factor=None):
        return cls(*_est_totals(num_time_steps_block, density_data,
                                props_data.weight, reduce_data, as_pure_est,
                                pure_est_reduce_factor))


@attr.s(auto_attribs=True, frozen=True)
class PairDistBlocks(SetPropBlocks):
    """Pair-distance histograms in blocks (an extension: the reference has no
    g2): totals[num_blocks, num_bins] are sums over walkers (and, for the
    mixed estimator, over the time steps of a block) of the integer
    histograms; `pair_distribution` normalises their weighted mean to g2(r)."""
    totals: np.ndarray
    weight_totals: np.ndarray

    @classmethod
    def from_data(cls, num_time_steps_block, pair_dist_data, props_data,
                  reduce_data=True, as_pure_est=True,
                  pure_est_reduce_factor=None):
        return cls(*_est_totals(num_time_steps_block, pair_dist_data,
                                props_data.weight, reduce_data, as_pure_est,
                                pure_est_reduce_factor))

    def pair_distribution(self, model_spec):
        """-> (r[num_bins], g2[num_bins], g2_err[num_bins]): bin centres, the
        weighted mean histogram normalised to g2 and its error."""
        from ...engine import pair_distribution_bins, pair_distribution_norm
        n, size = model_spec.boson_number, model_spec.supercell_size
        num_bins = np.asarray(self.totals).shape[-1]
        return (pair_distribution_bins(size, num_bins),
                pair_distribution_norm(self.mean, n, size),
                pair_distribution_norm(self.mean_error, n, size))


@attr.s(auto_attribs=True, frozen=True)
class SiteBlocks(SetPropBlocks):
    """Site occupation rows in blocks (an extension: the reference has no
    such estimator): totals[num_blocks, P + D] are sums over walkers (and, for
    the mixed estimator, over the time steps of a block) of the integer rows
    [occ | corr] of `engine.site_statistics`, P = `num_occupations`; the
    weighted mean is the row of one walker, whose first P entries add up to
    the number of sites."""
    totals: np.ndarray
    weight_totals: np.ndarray
    num_occupations: int = 1

    @classmethod
    def from_data(cls, num_time_steps_block, site_data, props_data,
                  reduce_data=True, as_pure_est=True,
                  pure_est_reduce_factor=None, num_occupations=1):
        return cls(*_est_totals(num_time_steps_block, site_data,
                                props_data.weight, reduce_data, as_pure_est,
                                pure_est_reduce_factor),
                   num_occupations=int(num_occupations))

    def __add__(self, other):
        if not isinstance(other, SiteBlocks) or \
                other.num_occupations != self.num_occupations:
            return NotImplemented
        return type(self)(
            np.concatenate((self.totals, other.totals), axis=0),
            np.concatenate((self.weight_totals, other.weight_totals), axis=0),
            self.num_occupations)

    def occupation_distribution(self):
        """-> (P(n)[P], P_err[P]): the share of the sites that hold n
        particles (the last entry collects n >= P - 1) and its error from the
        reblocking over blocks.  The occupation counts of a walker add up to
        the number of sites, which normalises them."""
        P = self.num_occupations
        occ = np.asarray(self.mean, dtype=np.float64)[:P]
        with np.errstate(invalid='ignore', divide='ignore'):
            err = np.asarray(self.mean_error, dtype=np.float64)[:P]
        sites = occ.sum()
        # (a count that is the same in every block has no scatter: the error
        # formula is 0 / 0 there)
        return occ / sites, np.nan_to_num(err) / sites

    def site_correlation(self, model_spec):
        """-> (C(d)[D], C_err[D]): the connected correlation
        <n_c n_{c+d}> - (N / S)^2 of the site occupations, d = 0 .. D-1 (C(0)
        is the on-site number variance), and its error."""
        from ...engine import site_statistics
        P = self.num_occupations
        n, sites = model_spec.boson_number, int(model_spec.supercell_size)
        with np.errstate(invalid='ignore', divide='ignore'):
            err = np.asarray(self.mean_error, dtype=np.float64)[P:]
        stats = site_statistics(self.mean, 1.0, n, sites, P)
        return stats.correlation, np.nan_to_num(err) / sites

    def number_variance(self, max_len, model_spec):
        """-> (ell[max_len], var[max_len], var_err[max_len]): the variance of
        the number of particles on ell = 1 .. max_len consecutive sites,
        sum_{|d| < ell} (ell - |d|) C(d) (max_len <= D); the error adds the
        errors of C(d) in quadrature through the same weights, as if the
        distances were independent."""
        from ...engine import SiteStatistics
        corr, err = self.site_correlation(model_spec)
        max_len = int(max_len)
        if not 1 <= max_len <= corr.shape[-1]:
            raise ValueError('number_variance: 1 <= max_len <= num_distances '
                             'is needed')
        ells = np.arange(1, max_len + 1)
        # the sum is linear in C: the same weights on the squared errors
        var = np.array([SiteStatistics(None, 0.0, None, corr)
                        .number_variance(ell) for ell in ells])
        w = np.where(np.arange(max_len)[None, :] < ells[:, None],
                     ells[:, None] - np.arange(max_len)[None, :], 0.0)
        w[:, 1:] *= 2.0
        return ells, var, np.sqrt((w ** 2) @ (err[:max_len] ** 2))


@attr.s(auto_attribs=True, frozen=True)
class CMDiffusionBlocks(UnWeightedPropBlocks):
    """Centre-of-mass diffusion curves in blocks (an extension: the reference
    has no superfluid fraction): totals[num_blocks, nts] holds, per kept block
    and time step t, <Y^2> = iter_cm_diffusion[t, 1] / num_walkers[t], Y being
    N times the unwrapped centre-of-mass displacement since the start of the
    block.  The yielded walkers have unit weight and every block restarts the
    clock, so the blocks are averaged as they are, one column per lag."""
    totals: np.ndarray

    @property
    def reblock(self):
        return reblock.OTFSet.from_non_obj_data(self.totals)

    def superfluid_fraction(self, model_spec, time_step):
        """-> (tau[nts - 1], ratio[nts - 1], ratio_err[nts - 1]) for the
        lags tau = t dt, t >= 1: the mean over the blocks of
        <Y^2>(t) / (2 N t dt), which tends to rho_s / rho at large lag, and
        its error from the reblocking over blocks."""
        curves = np.asarray(self.totals)
        tau = np.arange(1, curves.shape[-1]) * float(time_step)
        norm = 2.0 * model_spec.boson_number * tau
        # (lag 0 is zero in every block: it has no statistics)
        rb = reblock.OTFSet.from_non_obj_data(curves[:, 1:])
        return tau, rb.mean / norm, rb.mean_eff_error / norm


@attr.s(auto_attribs=True, frozen=True)
class ISFBlocks(UnWeightedPropBlocks):
    """Imaginary-time density correlations in blocks (an extension: the
    reference has none): totals[num_blocks, K, T + 2] holds, per kept block,
    the row of the last time step of the block over its num_walkers,
    iter_isf[nts - 1] / num_walkers[nts - 1]: columns l < T are
    F(k_m, tau_l), columns T, T + 1 the pure Re, Im <rho_m>.  The yielded
    walkers have unit weight and every block resets the origin, so the blocks
    are averaged as they are, one column per (mode, lag).  The estimate is
    pure in the limit of a long block: lag l has (nts - 1 - l lag_stride) dt
    of projection behind its later end, and lags close to the end of the block
    are mixed there."""
    totals: np.ndarray

    @property
    def reblock(self):
        rows = np.asarray(self.totals)
        return reblock.OTFSet.from_non_obj_data(rows.reshape(len(rows), -1))

    def scattering_function(self, model_spec, time_step, lag_stride=1):
        """-> (tau[T], F[T, K] / N, F_err[T, K] / N, F_conn[T, K] / N): the
        lags tau_l = l lag_stride dt, per mode the mean over the blocks of
        F(k_m, tau_l) with its error from the reblocking over blocks, and the
        connected function F - |<rho_m>|^2 from the means of columns T, T + 1
        (it matters at the reciprocal vectors of the lattice); all per
        particle, so that lag 0 is S(k_m)."""
        rows = np.asarray(self.totals)
        num_lags = rows.shape[-1] - 2
        n = model_spec.boson_number
        tau = np.arange(num_lags) * (int(lag_stride) * float(time_step))
        rb = self.reblock
        mean = rb.mean.reshape(rows.shape[1:])
        err = rb.mean_eff_error.reshape(rows.shape[1:])
        rho_sqr = mean[:, num_lags] ** 2 + mean[:, num_lags + 1] ** 2
        f = mean[:, :num_lags]
        return (tau, f.T / n, err[:, :num_lags].T / n,
                (f - rho_sqr[:, np.newaxis]).T / n)


@attr.s(auto_attribs=True, frozen=True)
class OBDMBlocks(SetPropBlocks):
    """Mixed one-body density matrix in blocks (an extension: the reference
    has no DMC g1): totals[num_blocks, num_shifts] holds, per kept block, the
    sum over the evaluated time steps of iter_obdm[t] (each a sum over the
    walkers, unweighted), weight_totals[num_blocks, 1] the number of walkers
    of those steps.  A zero shift contributes exactly 1 per walker, so its
    column equals the weights and g1(0) is exactly 1."""
    totals: np.ndarray
    weight_totals: np.ndarray

    def one_body_density(self):
        """-> (g1[num_shifts], g1_err[num_shifts]): the mean over the walkers
        of all kept blocks and its error from the reblocking over blocks.  (A
        column that equals the weights in every block, a zero shift, has the
        ratio 1 with no error: the error formula is 0 / 0 there.)"""
        with np.errstate(invalid='ignore', divide='ignore'):
            err = np.asarray(self.mean_error, dtype=np.float64)
        exact = np.all(np.asarray(self.totals) ==
                       np.asarray(self.weight_totals), axis=0)
        return self.mean, np.where(exact, 0.0, err)

    def momentum_distribution(self, shifts, momenta, model_spec):
        """-> (n[len(momenta)], n_err[len(momenta)]): the trapezoid-rule
        transform of g1 on the non-negative increasing grid `shifts`
        (`engine.momentum_distribution`) at the density N / L; the error adds
        the errors of g1 in quadrature through the same weights, as if the
        shifts were independent."""
        from ...engine import momentum_distribution
        g1, g1_err = self.one_body_density()
        dens = model_spec.boson_number / model_spec.supercell_size
        k = np.atleast_1d(np.asarray(momenta, dtype=np.float64))
        nk = momentum_distribution(shifts, g1, k, dens)
        # the transform is linear in g1: transform unit vectors scaled by the
        # errors and add the squares
        jac = momentum_distribution(shifts, np.diag(g1_err), k, dens)
        return nk, np.sqrt((jac ** 2).sum(axis=0))


@attr.s(auto_attribs=True, frozen=True)
class SSFPartBlocks(SetPropBlocks):
    totals: np.ndarray
    weight_totals: np.ndarray


@attr.s(auto_attribs=True, frozen=True)
class SSFBlocks:
    """Structure factor data in blocks (qmc_exec/data/dmc.py:495-621):
    S(k) = <|rho_k|^2> - <Re rho_k>^2 - <Im rho_k>^2."""
    fdk_sqr_abs_part: SSFPartBlocks
    fdk_real_part: SSFPartBlocks
    fdk_imag_part: SSFPartBlocks

    @classmethod
    def from_data(cls, num_time_steps_block, ssf_data, props_data,
                  reduce_data=True, as_pure_est=True,
                  pure_est_reduce_factor=None):
        totals, w = _est_totals(num_time_steps_block, ssf_data,
                                props_data.weight, reduce_data, as_pure_est,
                                pure_est_reduce_factor)
        return cls(SSFPartBlocks(totals[:, :, 0], w),
                   SSFPartBlocks(totals[:, :, 1], w),
                   SSFPartBlocks(totals[:, :, 2], w))

    @property
    def mean(self):
        return (self.fdk_sqr_abs_part.mean - self.fdk_real_part.mean ** 2 -
                self.fdk_imag_part.mean ** 2)

    @property
    def mean_error(self):
        re, im = self.fdk_real_part, self.fdk_imag_part
        return (self.fdk_sqr_abs_part.mean_error +
                2 * (re.mean * re.mean_error + im.mean * im.mean_error))

    def __add__(self, other):
        if not isinstance(other, SSFBlocks):
            return NotImplemented
        return SSFBlocks(self.fdk_sqr_abs_part + other.fdk_sqr_abs_part,
                         self.fdk_real_part + other.fdk_real_part,
                         self.fdk_imag_part + other.fdk_imag_part)


@attr.s(auto_attribs=True, frozen=True)
class PropsDataBlocks:
    energy: EnergyBlocks
    weight: WeightBlocks
    num_walkers: NumWalkersBlocks
    density: t.Optional[t.Any] = None
    ss_factor: t.Optional[t.Any] = None
    # (keyword only: the positional order of the others is what it was)
    cm_diffusion: t.Optional[t.Any] = attr.ib(default=None, kw_only=True)
    isf: t.Optional[t.Any] = attr.ib(default=None, kw_only=True)
    obdm: t.Optional[t.Any] = attr.ib(default=None, kw_only=True)
    site: t.Optional[t.Any] = attr.ib(default=None, kw_only=True)
    pair_dist: t.Optional[t.Any] = None


@attr.s(auto_attribs=True, frozen=True)
class PropsDataSeries:
    """Per-time-step data kept with `keep_iter_data`
    (qmc_exec/data/dmc.py:624-660)."""
    iter_props_blocks: t.Any
    ssf_blocks: t.Optional[np.ndarray] = None
    #: pair histograms per block and time step [num_blocks, nts, num_bins]
    pair_dist_blocks: t.Optional[np.ndarray] = None
    #: centre-of-mass diffusion sums per block and time step [num_blocks, nts, 2]
    cm_diffusion_blocks: t.Optional[np.ndarray] = None
    #: F(k, tau) row sums per block and time step [num_blocks, nts, K, T + 2]
    isf_blocks: t.Optional[np.ndarray] = None
    #: g1(s) row sums per block and time step [num_blocks, nts, num_shifts]
    obdm_blocks: t.Optional[np.ndarray] = None

    @property
    def props(self):
        p = self.iter_props_blocks
        return type(p)(*[np.hstack(getattr(p, f)) for f in p._fields])


@attr.s(auto_attribs=True, frozen=True)
class SamplingData:
    blocks: PropsDataBlocks
    series: t.Optional[PropsDataSeries] = None


# ---- HDF5 layout (qmc_exec/data/dmc.py:99-120, 192-211, 581-613, 683-735,
# 770-793): <group>/totals [, weight_totals]; ss_factor/{fdk_sqr_abs,fdk_real,
# fdk_imag}/...; blocks/{energy,weight,num_walkers[,density][,ss_factor][,...
# the further keys of `dmc_est.ESTIMATORS`, in that order]} ----
def _export_weighted(self, group):
    group.create_dataset('totals', data=self.totals)
    group.create_dataset('weight_totals', data=self.weight_totals)


def _import_weighted(cls, group):
    return cls(totals=group.get('totals')[()],
               weight_totals=group.get('weight_totals')[()])


def _export_unweighted(self, group):
    group.create_dataset('totals', data=self.totals)


def _import_unweighted(cls, group):
    return cls(totals=group.get('totals')[()])


PropBlocks.hdf5_export = _export_weighted
PropBlocks.from_hdf5_data = classmethod(_import_weighted)
UnWeightedPropBlocks.hdf5_export = _export_unweighted
UnWeightedPropBlocks.from_hdf5_data = classmethod(_import_unweighted)


def _ssf_export(self, group):
    self.fdk_sqr_abs_part.hdf5_export(group.require_group('fdk_sqr_abs'))
    self.fdk_real_part.hdf5_export(group.require_group('fdk_real'))
    self.fdk_imag_part.hdf5_export(group.require_group('fdk_imag'))


def _ssf_import(cls, group):
    return cls(SSFPartBlocks.from_hdf5_data(group.get('fdk_sqr_abs')),
               SSFPartBlocks.from_hdf5_data(group.get('fdk_real')),
               SSFPartBlocks.from_hdf5_data(group.get('fdk_imag')))


def _site_export(self, group):
    _export_weighted(self, group)
    group.attrs.update({'num_occupations': int(self.num_occupations)})


def _site_import(cls, group):
    return cls(totals=group.get('totals')[()],
               weight_totals=group.get('weight_totals')[()],
               num_occupations=int(group.attrs['num_occupations']))


SiteBlocks.hdf5_export = _site_export
SiteBlocks.from_hdf5_data = classmethod(_site_import)
SSFBlocks.hdf5_export = _ssf_export
SSFBlocks.from_hdf5_data = classmethod(_ssf_import)


def _blocks_export(self, group):
    self.energy.hdf5_export(group.require_group('energy'))
    self.weight.hdf5_export(group.require_group('weight'))
    self.num_walkers.hdf5_export(group.require_group('num_walkers'))
    for est in dmc_est.ESTIMATORS:
        est_blocks = getattr(self, est.key)
        if est_blocks is not None:
            est_blocks.hdf5_export(group.require_group(est.key))


def _blocks_import(cls, group):
    est_blocks = {
        est.key: globals()[est.blocks_class].from_hdf5_data(group.get(est.key))
        for est in dmc_est.ESTIMATORS if group.get(est.key) is not None}
    return cls(EnergyBlocks.from_hdf5_data(group.get('energy')),
               WeightBlocks.from_hdf5_data(group.get('weight')),
               NumWalkersBlocks.from_hdf5_data(group.get('num_walkers')),
               **est_blocks)


PropsDataBlocks.hdf5_export = _blocks_export
PropsDataBlocks.from_hdf5_data = classmethod(_blocks_import)


def _sampling_export(self, group):
    # (the reference does not store the per-step series either)
    self.blocks.hdf5_export(group.require_group('blocks'))


def _sampling_import(cls, group):
    return cls(PropsDataBlocks.from_hdf5_data(group.get('blocks')))


SamplingData.hdf5_export = _sampling_export
SamplingData.from_hdf5_data = classmethod(_sampling_import)
