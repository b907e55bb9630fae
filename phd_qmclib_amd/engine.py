"""Thin object wrappers over the C-ABI handles (engine, VMC ensemble, DMC
ensemble).  numpy on the host side, HBM-resident state behind the handles.
The `Sampling` classes in `mrbp_qmc.vmc` / `mrbp_qmc.dmc` are built on these.
"""
import ctypes as C
import typing as t

import numpy as np

from . import _lib
from ._lib import (DmcEstParams, DmcParams, ModelParams, QmcError, VmcParams,
                   check, ptr,
                   _i64p, _u64p, _u8p)

__all__ = ['ModelEngine', 'VmcEnsemble', 'DmcEnsemble', 'EvalResult',
           'vmc_move_code', 'DeviceBuffer', 'momentum_distribution',
           'site_statistics', 'EnergyComponents', 'energy_components',
           'contact_extrapolate', 'contact_coupling', 'contact_ranges_array',
           'model_params_struct', 'QmcError']


class EvalResult(t.NamedTuple):
    wf_abs_log: np.ndarray    # [W]
    energy: np.ndarray        # [W]
    ith_energy: np.ndarray    # [W, N]
    drift: np.ndarray         # [W, N]


def model_params_struct(cfc_spec) -> ModelParams:
    """Flatten (Params, OBFParams, TBFParams) into the C struct."""
    mp, ob, tb = cfc_spec.model_params, cfc_spec.obf_params, \
        cfc_spec.tbf_params
    s = ModelParams()
    for k in ('lattice_depth', 'lattice_ratio', 'interaction_strength',
              'supercell_size', 'tbf_contact_cutoff', 'defect_magnitude',
              'well_width', 'barrier_width'):
        setattr(s, k, float(getattr(mp, k)))
    s.boson_number = int(mp.boson_number)
    s.defects_sep = int(mp.defects_sep)
    s.is_free = int(bool(mp.is_free))
    s.is_ideal = int(bool(mp.is_ideal))
    s.param_e0, s.param_k1, s.param_kp1 = (float(ob.param_e0),
                                           float(ob.param_k1),
                                           float(ob.param_kp1))
    s.param_k2, s.param_beta = float(tb.param_k2), float(tb.param_beta)
    s.param_r_off, s.param_am = float(tb.param_r_off), float(tb.param_am)
    return s


def _current_device():
    """Device index to bind to: LOCAL_RANK-aware through torch when a process
    group set the device, else 0."""
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except Exception:     # torch missing or no GPU runtime
        pass
    return 0


MAX_PAIR_DIST_BINS = 4096      # PD_MAX_BINS of csrc/qmc_pairdist.h


def pair_distribution_bins(supercell_size, num_bins):
    """Bin centres r_b = (b + 1/2) delta, delta = (L/2) / num_bins, of the
    pair-distance histograms -> r[num_bins]."""
    nb = ModelEngine._num_bins(num_bins)
    delta = 0.5 * float(supercell_size) / nb
    return (np.arange(nb) + 0.5) * delta


def pair_distribution_norm(counts, boson_number, supercell_size):
    """g2 = H L / (N (N - 1) delta) of (mean) histograms H[..., num_bins]: 1 on
    average for uncorrelated uniform particles."""
    counts = np.asarray(counts, dtype=np.float64)
    n, L = int(boson_number), float(supercell_size)
    delta = 0.5 * L / counts.shape[-1]
    return counts * (L / (n * (n - 1) * delta))


MAX_TRIPLE_DIST_BINS = 4096    # TD_MAX_BINS of csrc/qmc_tripledist.h


def _max_span(supercell_size, max_span):
    """max_span of the triple-span histograms: None is L/2, anything outside
    (0, L/2] a ValueError."""
    half = 0.5 * float(supercell_size)
    if max_span is None:
        return half
    span = float(max_span)
    if not 0.0 < span <= half:
        raise ValueError('max_span must be in (0, supercell_size / 2]')
    return span


def triple_distribution_bins(supercell_size, num_bins, max_span=None):
    """Bin centres d_b = (b + 1/2) delta, delta = max_span / num_bins, of the
    triple-span histograms (without the overflow bin) -> d[num_bins]."""
    nb = ModelEngine._num_bins(num_bins)
    delta = _max_span(supercell_size, max_span) / nb
    return (np.arange(nb) + 0.5) * delta


def triple_distribution_norm(counts, boson_number, supercell_size,
                             max_span=None):
    """g3 = T / (C(N,3) 3 (delta/L)^2 (2 b + 1)) of (mean) histograms
    T[..., num_bins + 1], the overflow bin dropped -> [..., num_bins]: 1 on
    average for uncorrelated uniform particles (three uniform points of a ring
    lie within an arc x L with probability 3 x^2, x <= 1/2)."""
    counts = np.asarray(counts, dtype=np.float64)
    n, L = int(boson_number), float(supercell_size)
    nb = counts.shape[-1] - 1
    if nb < 1:
        raise ValueError('counts[..., num_bins + 1] expected')
    if n < 3:
        raise ValueError('g3 needs boson_number >= 3')
    delta = _max_span(L, max_span) / nb
    triples = n * (n - 1) * (n - 2) / 6.0
    expect = triples * 3.0 * (delta / L) ** 2 * (2.0 * np.arange(nb) + 1.0)
    return counts[..., :nb] / expect


MAX_RENYI_LENGTHS = 4096       # RENYI_MAX_LEN of csrc/qmc_renyi.h


def renyi_lengths(supercell_size, lengths):
    """Segment lengths of the replica-swap estimator as a contiguous fp64
    array: 1 to 4096 finite values in (0, L), anything else a ValueError."""
    ln = np.ascontiguousarray(lengths, dtype=np.float64)
    if ln.ndim != 1 or not 1 <= ln.size <= MAX_RENYI_LENGTHS:
        raise ValueError('lengths must be a 1-d array of 1 to %d values'
                         % MAX_RENYI_LENGTHS)
    if not np.all((ln > 0.0) & (ln < float(supercell_size))):
        raise ValueError('every length must be in (0, supercell_size)')
    return ln


def _renyi_origin(origin):
    a0 = float(origin)
    if not np.isfinite(a0):
        raise ValueError('origin must be finite')
    return a0


def renyi_entropy(sums, num_pairs):
    """Renyi-2 entropy from the replica-swap sums[K, 3] = sum swap,
    sum swap^2, matched pairs over `num_pairs` replica pairs
    -> (S2[K], S2_err[K], p_match[K]): S2 = -ln(mean swap), its standard error
    stderr(swap) / mean(swap), and the fraction of matched pairs.  A length no
    pair matched at has S2 = inf and S2_err = nan."""
    sums = np.asarray(sums, dtype=np.float64)
    p = int(num_pairs)
    if sums.ndim != 2 or sums.shape[1] != 3:
        raise ValueError('sums[K, 3] expected')
    if p != num_pairs or p < 1:
        raise ValueError('num_pairs must be a positive integer')
    mean = sums[:, 0] / p
    var = np.maximum(sums[:, 1] / p - mean ** 2, 0.0)
    stderr = np.sqrt(var / max(p - 1, 1))
    with np.errstate(divide='ignore', invalid='ignore'):
        return -np.log(mean), stderr / mean, sums[:, 2] / p


def renyi_regions(supercell_size, regions):
    """Regions of the two-segment replica-swap estimator as a contiguous fp64
    array [K, 3] of (l1, g, l2): 1 to 4096 rows, all finite, l1 > 0, g >= 0,
    l2 >= 0 and (l1 + g) + l2 < L; anything else a ValueError."""
    rg = np.ascontiguousarray(regions, dtype=np.float64)
    if (rg.ndim != 2 or rg.shape[1] != 3
            or not 1 <= rg.shape[0] <= MAX_RENYI_LENGTHS):
        raise ValueError('regions[K, 3] of 1 to %d rows (l1, g, l2) expected'
                         % MAX_RENYI_LENGTHS)
    end = (rg[:, 0] + rg[:, 1]) + rg[:, 2]
    if not (np.all(np.isfinite(rg)) and np.all(rg[:, 0] > 0.0)
            and np.all(rg[:, 1:] >= 0.0)
            and np.all(end < float(supercell_size))):
        raise ValueError('every region needs l1 > 0, g >= 0, l2 >= 0 and '
                         'l1 + g + l2 < supercell_size')
    return rg


MAX_RENYI_REGION_SUMS = 1 << 20    # RG_MAX_SUMS of csrc/qmc_renyi_region.h


def _num_charges(num_charges, boson_number, nreg):
    if num_charges is None:
        num_charges = int(boson_number) + 1
    q = int(num_charges)
    if q != num_charges or not 0 <= q <= int(boson_number) + 1:
        raise ValueError('num_charges must be an integer in '
                         '[0, boson_number + 1]')
    if nreg * (3 + 2 * q) > MAX_RENYI_REGION_SUMS:
        raise ValueError('nreg (3 + 2 num_charges) exceeds 2^20')
    return q


class ResolvedRenyi(t.NamedTuple):
    """`renyi_resolved`: the Renyi-2 entropy of K regions, its error and the
    matched fraction as `renyi_entropy` gives them, and the resolution by the
    particle number n = 0 ... Q - 1 of the region."""
    entropy: np.ndarray           # [K]
    entropy_err: np.ndarray       # [K]
    p_match: np.ndarray           # [K]
    charge_prob: np.ndarray       # [K, Q] p(n), the counting statistics
    charge_swap: np.ndarray       # [K, Q] <swap delta(n_X = n)>
    charge_entropy: np.ndarray    # [K, Q] S2(n)


def renyi_resolved(sums, num_pairs, num_charges):
    """Charge-resolved Renyi-2 entropies from the region sums[K, 3 + 2Q] of
    `ModelEngine.renyi_region_swap_reduce_dev` over P = `num_pairs` replica
    pairs -> ResolvedRenyi.  entropy, entropy_err and p_match are
    `renyi_entropy` of the columns 0-2.  charge_prob[K, Q] = column(4 + 2n) /
    (2P) is the probability p(n) that the region holds n particles,
    charge_swap[K, Q] = column(3 + 2n) / P = <swap delta(n_X = n)> =
    p(n)^2 Tr rho_n^2, and charge_entropy = -ln(charge_swap / charge_prob^2)
    the entropy S2(n) of the block of rho_X with n particles, nan where
    charge_swap is 0 (no matched pair held n particles).  With Q = N + 1 every
    charge is collected and sum_n charge_swap = <swap>, sum_n charge_prob =
    1."""
    sums = np.asarray(sums, dtype=np.float64)
    p, q = int(num_pairs), int(num_charges)
    if q != num_charges or q < 0:
        raise ValueError('num_charges must be a non-negative integer')
    if sums.ndim != 2 or sums.shape[1] != 3 + 2 * q:
        raise ValueError('sums[K, 3 + 2 num_charges] expected')
    s2, s2_err, p_match = renyi_entropy(sums[:, :3], num_pairs)
    prob = sums[:, 4::2] / (2.0 * p)
    swap = sums[:, 3::2] / p
    with np.errstate(divide='ignore', invalid='ignore'):
        s2n = np.where(swap > 0.0, -np.log(swap / prob ** 2), np.nan)
    return ResolvedRenyi(s2, s2_err, p_match, prob, swap, s2n)


def renyi_mutual_information(s_a, s_c, s_ac, err_a, err_c, err_ac):
    """Renyi-2 mutual information I2(A:C) = S2(A) + S2(C) - S2(A u C) of two
    disjoint segments -> (I2, I2_err).  I2_err is the quadrature sum of the
    three errors and only indicative: estimates taken from the same replica
    pairs are correlated, as `contact_extrapolate` says of its own."""
    s = [np.asarray(x, dtype=np.float64) for x in (s_a, s_c, s_ac)]
    e = [np.asarray(x, dtype=np.float64) for x in (err_a, err_c, err_ac)]
    return (s[0] + s[1] - s[2], np.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2))


def particle_entropy(sums, num_pairs):
    """One-particle Renyi-2 entropy from the one-particle swap
    sums[3] = sum m, sum m^2, P over `num_pairs` = P replica pairs
    -> (S2, S2_err, purity, purity_err): purity = mean m = Tr rho1^2 (rho1 of
    trace 1), its standard error over the pairs, S2 = -ln purity and
    S2_err = purity_err / purity.  The condensate fraction lies in
    [purity, sqrt(purity)]."""
    sums = np.asarray(sums, dtype=np.float64)
    p = int(num_pairs)
    if sums.shape != (3,):
        raise ValueError('sums[3] expected')
    if p != num_pairs or p < 1:
        raise ValueError('num_pairs must be a positive integer')
    if sums[2] != p:
        raise ValueError('sums[2] is not num_pairs')
    mean = sums[0] / p
    var = max(sums[1] / p - mean ** 2, 0.0)
    stderr = np.sqrt(var / max(p - 1, 1))
    with np.errstate(divide='ignore', invalid='ignore'):
        return (float(-np.log(mean)), float(stderr / mean), float(mean),
                float(stderr))


MAX_CONTACT_RANGES = 16        # EP_MAX_RANGES of csrc/qmc_energy_parts.h
ENERGY_PARTS_COLS = 4          # E, T, V, I in front of the windows


def contact_ranges_array(cfc_spec, contact_ranges):
    """The windows of the contact estimator as a contiguous fp64 array, checked
    against the limits of qmc_energy_parts: at most 16 of them (None or () is
    none), each finite and in (0, L/2], and on a model with interactions at
    most |tbf_contact_cutoff| -- the cosine form of the two-body factor, whose
    cusp the estimator divides out, holds only there."""
    rg = np.ascontiguousarray(() if contact_ranges is None else contact_ranges,
                              dtype=np.float64)
    if rg.ndim != 1 or rg.size > MAX_CONTACT_RANGES:
        raise ValueError('contact_ranges must be a 1-d sequence of at most %d '
                         'windows' % MAX_CONTACT_RANGES)
    mp = cfc_spec.model_params
    if not np.all(np.isfinite(rg)) or not np.all(rg > 0.0):
        raise ValueError('contact_ranges must be finite and positive')
    if np.any(rg > 0.5 * float(mp.supercell_size)):
        raise ValueError('contact_ranges must be in (0, supercell_size / 2]')
    if not mp.is_ideal and np.any(rg > abs(float(mp.tbf_contact_cutoff))):
        raise ValueError('contact_ranges must not exceed |tbf_contact_cutoff| '
                         'on a model with interactions')
    return rg


def contact_coupling(cfc_spec):
    """g = 4 kappa, kappa = f2'(0+) / f2(0) = k2 tan(k2 r_off): the strength of
    the contact term the cusp of the two-body factor stands for, computed from
    the two-body parameters (0 on an ideal model).  `Spec.tbf_params` sets
    k2 r_off = atan(1 / (k2 a1d)), which makes it interaction_strength L / N:
    interaction_strength itself at one boson per lattice period."""
    tb = cfc_spec.tbf_params
    k2 = float(tb.param_k2)
    if cfc_spec.model_params.is_ideal or k2 == 0.0:
        return 0.0
    return 4.0 * k2 * float(np.tan(k2 * float(tb.param_r_off)))


class EnergyComponents(t.NamedTuple):
    """Result of `energy_components`: means over the configurations and the
    standard errors of those means."""
    total: float                    # <E_L>
    total_err: float
    kinetic: float                  # <sum_i F_i^2>
    kinetic_err: float
    lattice: float                  # <sum_i V(z_i)>
    lattice_err: float
    interaction: float              # <E_L - T - V>, the remainder
    interaction_err: float
    contact: np.ndarray             # [K] <sum_{i<j} delta(z_ij)> per window
    contact_err: np.ndarray
    contact_ranges: np.ndarray      # [K]
    coupling: float                 # g = 4 kappa: g * contact ~ interaction


def energy_components(sums, wsum, cfc_spec, contact_ranges=None,
                      num_confs=None):
    """EnergyComponents from the sums of `ModelEngine.energy_parts_weighted`
    (or `VmcEnsemble.energy_parts_parts` with wsum = number of chains):
    sums[4 + K, 2] = sum_c w_c x_c, sum_c w_c x_c^2 over the columns
    E, T, V, I, C_0 .. C_{K-1} and wsum = sum_c w_c.  Every mean is
    sum w x / sum w.  The errors are those of the mean over the configurations,
    sqrt(var / (n - 1)) with the weighted variance and n = `num_confs`
    configurations (None: unit weights, n = wsum); with unequal weights that
    is exact only as far as the weights are alike, and configurations of one
    run are correlated in time: treat it as a lower bound there."""
    rg = contact_ranges_array(cfc_spec, contact_ranges)
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape != (ENERGY_PARTS_COLS + rg.size, 2):
        raise ValueError('sums[4 + len(contact_ranges), 2] expected')
    wsum = float(wsum)
    if not wsum > 0.0:
        raise ValueError('a positive weight sum is needed')
    n = wsum if num_confs is None else float(num_confs)
    mean = sums[:, 0] / wsum
    var = np.maximum(sums[:, 1] / wsum - mean ** 2, 0.0)
    err = np.sqrt(var / max(n - 1.0, 1.0))
    c = ENERGY_PARTS_COLS
    return EnergyComponents(
        float(mean[0]), float(err[0]), float(mean[1]), float(err[1]),
        float(mean[2]), float(err[2]), float(mean[3]), float(err[3]),
        mean[c:].copy(), err[c:].copy(), rg.copy(), contact_coupling(cfc_spec))


def contact_extrapolate(ranges, values, errors):
    """The windowed contact at zero range: a weighted least-squares fit
    C(r) = C_0 + b r^2 to `values` with `errors` at the windows `ranges`
    (at least two different ones) -> (C_0, its error).  The bias of a window
    is of order r^2.  The windows share pairs -- every pair inside a window is
    inside all the larger ones -- so their values are positively correlated;
    the fit treats them as independent, which is an approximation: the
    returned error is indicative, not a confidence interval."""
    r = np.asarray(ranges, dtype=np.float64)
    y = np.asarray(values, dtype=np.float64)
    sig = np.asarray(errors, dtype=np.float64)
    if r.ndim != 1 or r.shape != y.shape or r.shape != sig.shape:
        raise ValueError('ranges, values and errors must be 1-d and alike')
    if np.unique(r).size < 2:
        raise ValueError('at least two different windows are needed')
    if not np.all(np.isfinite(sig)) or not np.all(sig > 0.0):
        raise ValueError('errors must be finite and positive')
    x = np.stack([np.ones_like(r), r ** 2], axis=1)            # [K, 2]
    wgt = 1.0 / sig ** 2
    cov = np.linalg.inv(x.T @ (wgt[:, None] * x))
    coef = cov @ (x.T @ (wgt * y))
    return float(coef[0]), float(np.sqrt(cov[0, 0]))


def superfluid_ratio(iter_cm, num_walkers, boson_number, time_step):
    """The normalised centre-of-mass diffusion curve of one estimator block,
    iter_cm[nts, 2] (`DmcEnsemble.read_cm_diffusion`) and num_walkers[nts]:
    ratio[t] = iter_cm[t, 1] / num_walkers[t] / (2 N t dt) for t >= 1, which
    tends to rho_s / rho at large lag -> (tau[1:], ratio[1:]), tau = t dt."""
    iter_cm = np.asarray(iter_cm, dtype=np.float64)
    nw = np.asarray(num_walkers, dtype=np.float64)
    tau = np.arange(1, iter_cm.shape[0]) * float(time_step)
    return tau, iter_cm[1:, 1] / nw[1:] / (2.0 * int(boson_number) * tau)


def intermediate_scattering(iter_isf, num_walkers, boson_number, time_step,
                            lag_stride):
    """The imaginary-time density correlations of one estimator block,
    iter_isf[nts, K, T + 2] (`DmcEnsemble.read_isf`) and num_walkers[nts], read
    at the last step of the block, where the projection behind every lag is
    longest -> (tau[T], F[T, K] / N, rho_mean[K] complex):
    tau[l] = l lag_stride dt, F[l, m] / N = iter_isf[-1, m, l] /
    num_walkers[-1] / N (it is S(k_m) at lag 0 and decays as
    sum_n |<n|rho_k|0>|^2 exp(-(E_n - E_0) tau)), rho_mean[m] the pure
    <rho_m> of columns T, T + 1.  The estimate is pure in the limit of a long
    block: lag l has projection time (nts - 1 - l lag_stride) dt behind its
    later end, and lags close to the end of the block are mixed there.  Lags
    the block did not reach (l lag_stride >= nts) are zero.  The connected
    function, which matters at the reciprocal vectors of the lattice, is
    F[l, m] - |rho_mean[m]|^2 (before the division by N)."""
    iter_isf = np.asarray(iter_isf, dtype=np.float64)
    nw = float(np.asarray(num_walkers)[-1])
    num_lags = iter_isf.shape[-1] - 2
    last = iter_isf[-1] / nw
    tau = np.arange(num_lags) * (int(lag_stride) * float(time_step))
    rho_mean = last[:, num_lags] + 1j * last[:, num_lags + 1]
    return tau, last[:, :num_lags].T / int(boson_number), rho_mean


class SiteStatistics(t.NamedTuple):
    """What `site_statistics` returns."""
    #: P(n)[..., num_occ]: the share of the sites that hold n particles (the
    #: last entry collects n >= num_occ - 1); it sums to 1
    occupation_dist: np.ndarray
    #: N / S
    mean_occupation: float
    #: <n_c^2> - (N / S)^2 [...], or None without a correlation part
    variance: t.Optional[np.ndarray]
    #: C(d) = <n_c n_{c+d}> - (N / S)^2 [..., num_dist]
    correlation: np.ndarray

    def number_variance(self, length):
        """Variance of the number of particles on `length` consecutive sites,
        sum_{|d| < length} (length - |d|) C(d) (C is even in d) -> [...];
        it needs the distances d < length."""
        ell = int(length)
        if ell < 1 or ell > self.correlation.shape[-1]:
            raise ValueError('number_variance: 1 <= length <= num_dist is '
                             'needed')
        w = np.full(ell, 2.0) * (ell - np.arange(ell))
        w[0] = ell
        return self.correlation[..., :ell] @ w


def site_statistics(rows, num_walkers, boson_number, num_sites, num_occ):
    """The site occupation statistics from rows[..., num_occ + num_dist] =
    [occ | corr] (`DmcEnsemble.read_site`) summed over `num_walkers` walkers
    (a number, or an array shaped as the leading axes of rows; for the sum of
    the mixed rows of several steps, the summed walkers) -> SiteStatistics:
    P(n) = occ / (S W), the mean occupation N / S, the on-site variance and the
    connected correlation C(d) = corr[d] / (S W) - (N / S)^2."""
    rows = np.asarray(rows, dtype=np.float64)
    P, S = int(num_occ), int(num_sites)
    if not 1 <= P <= rows.shape[-1]:
        raise ValueError('site_statistics: num_occ must be in [1, row length]')
    norm = S * np.asarray(num_walkers, dtype=np.float64)[..., np.newaxis]
    mean = int(boson_number) / S
    corr = rows[..., P:] / norm - mean ** 2
    return SiteStatistics(rows[..., :P] / norm, mean,
                          corr[..., 0] if corr.shape[-1] else None, corr)


def momentum_distribution(shifts, g1, momenta, density):
    """n(k) = density * 2 int_0^{s_max} g1(s) cos(k s) ds by the trapezoid
    rule on the grid `shifts` (non-negative, increasing; g1 is even in s) ->
    n[..., len(momenta)] for g1[..., len(shifts)]."""
    s = np.asarray(shifts, dtype=np.float64)
    g1 = np.asarray(g1, dtype=np.float64)
    k = np.atleast_1d(np.asarray(momenta, dtype=np.float64))
    if s.ndim != 1 or s.size < 2 or g1.shape[-1] != s.size:
        raise ValueError('shifts must be a 1-d grid of at least two points '
                         'and the last axis of g1 must match it')
    if s[0] < 0 or not np.all(np.diff(s) > 0):
        raise ValueError('shifts must be non-negative and increasing')
    # trapezoid weights of the grid
    w = np.zeros_like(s)
    ds = np.diff(s)
    w[:-1] += 0.5 * ds
    w[1:] += 0.5 * ds
    kern = np.cos(s[:, None] * k[None, :]) * w[:, None]       # [S, M]
    return 2.0 * float(density) * (g1 @ kern)


#: limits of `ModelEngine.one_body_matrix` (qmc_obdm_grid)
MAX_OBDM_GRID_POINTS = 512
MAX_OBDM_GRID_GROUPS = 1024


def _obdm_grid_args(num_points, num_groups, nconf):
    """(M, G) of a density-matrix grid as integers, checked against the
    limits of qmc_obdm_grid: M in [1, 512], G in [1, min(1024, nconf)]."""
    m, g, nc = int(num_points), int(num_groups), int(nconf)
    if m != num_points or not 1 <= m <= MAX_OBDM_GRID_POINTS:
        raise ValueError('num_points must be an integer in [1, %d]'
                         % MAX_OBDM_GRID_POINTS)
    if nc < 1:
        raise ValueError('at least one configuration is needed')
    if g != num_groups or not 1 <= g <= min(MAX_OBDM_GRID_GROUPS, nc):
        raise ValueError('num_groups must be an integer in [1, min(%d, '
                         'number of configurations)]' % MAX_OBDM_GRID_GROUPS)
    return m, g


def one_body_matrix_points(supercell_size, num_points):
    """Cell centres x_c = (c + 1/2) L / M of the `num_points` = M uniform
    cells of [0, L): the columns of `ModelEngine.one_body_matrix` (its rows
    are the cells themselves) -> x[M]."""
    m = int(num_points)
    if m != num_points or not 1 <= m <= MAX_OBDM_GRID_POINTS:
        raise ValueError('num_points must be an integer in [1, %d]'
                         % MAX_OBDM_GRID_POINTS)
    return (np.arange(m) + 0.5) * float(supercell_size) / m


class NaturalOrbitals(t.NamedTuple):
    """Result of `natural_orbitals`."""
    matrix: np.ndarray              # K[M, M], symmetrised
    occupations: np.ndarray         # lambda_k, descending
    occupations_err: np.ndarray
    orbitals: np.ndarray            # [M, M], column k belongs to lambda_k
    condensate_fraction: float      # lambda_0 / N
    condensate_fraction_err: float
    purity: float                   # sum_k lambda_k^2 / N^2
    purity_err: float
    trace: float                    # ~ N


def _cross_purity(kg, boson_number):
    """Purity from the group matrices kg[G, M, M]: the mean of <K_g, K_h>_F
    over the ordered pairs g != h, over N^2; one group: |K|_F^2 / N^2."""
    g = kg.shape[0]
    n2 = float(boson_number) ** 2
    if g == 1:
        return float(np.sum(kg[0] ** 2)) / n2
    tot = kg.sum(axis=0)
    cross = np.sum(tot ** 2) - np.sum(kg ** 2)
    return float(cross) / (g * (g - 1) * n2)


def natural_orbitals(sums, wsum, boson_number, supercell_size=None):
    """Natural orbitals from the group sums of `ModelEngine.one_body_matrix`,
    sums[G, M, M] and wsum[G] -> NaturalOrbitals:

    matrix       K = (A + A^T) / 2 with A = sum_g sums / sum_g wsum, the
                 estimate of int_{bin a} rho1(x, x_c) dx
    occupations  the eigenvalues of K (`eigvalsh`), descending; they add up to
                 `trace` ~ N
    occupations_err  delete-one-group jackknife of every sorted eigenvalue
                 (zeros for G = 1)
    orbitals     column k is the eigenvector of occupations[k], normalised to
                 sum_a |phi_a|^2 delta = 1 on the grid with delta = L / M
                 (`supercell_size` None: delta = 1)
    condensate_fraction, condensate_fraction_err  occupations[0] / N
    purity       Tr rho1^2 (rho1 of trace 1) as the CROSS-GROUP estimate
                 sum_{g != h} <K_g, K_h>_F / (G (G - 1) N^2), K_g the
                 symmetrised matrix of group g alone.  The noise of two
                 different groups is independent, so this is unbiased by the
                 noise; the plain |K|_F^2 / N^2 is biased upwards by the
                 variance of every cell.  For G = 1 there is only the plain
                 |K|_F^2 / N^2, and that is what is returned.
    purity_err   delete-one-group jackknife (zero for G = 1)
    trace        Tr K

    The largest eigenvalue of a noisy symmetric matrix is biased UPWARDS at
    second order in the noise (level repulsion), so condensate_fraction
    overestimates n0 / N by a term that falls like 1 / (number of
    configurations); the jackknife error does not contain it.  Extrapolate a
    DMC mixed estimate as 2 K_DMC - K_VMC on `matrix` before diagonalising."""
    sums = np.asarray(sums, dtype=np.float64)
    wsum = np.atleast_1d(np.asarray(wsum, dtype=np.float64))
    if sums.ndim == 2:
        sums = sums[None]
    if (sums.ndim != 3 or sums.shape[1] != sums.shape[2] or
            wsum.shape != sums.shape[:1]):
        raise ValueError('sums[G, M, M] and wsum[G] expected')
    if not np.all(wsum > 0):
        raise ValueError('every group needs a positive weight sum')
    n = float(boson_number)
    if not n > 0:
        raise ValueError('boson_number must be positive')
    g, m = sums.shape[0], sums.shape[1]
    delta = 1.0 if supercell_size is None else float(supercell_size) / m

    def sym(a):
        return 0.5 * (a + np.swapaxes(a, -1, -2))

    def eig(a):
        return np.linalg.eigvalsh(a)[::-1]

    tot, wtot = sums.sum(axis=0), wsum.sum()
    k = sym(tot / wtot)
    lam, vec = np.linalg.eigh(k)
    lam, vec = lam[::-1], vec[:, ::-1] / np.sqrt(delta)
    kg = sym(sums / wsum[:, None, None])
    purity = _cross_purity(kg, n)
    lam_err, purity_err = np.zeros(m), 0.0
    if g > 1:
        jl = np.array([eig(sym((tot - sums[i]) / (wtot - wsum[i])))
                       for i in range(g)])
        jp = np.array([_cross_purity(np.delete(kg, i, axis=0), n)
                       for i in range(g)])
        f = (g - 1.0) / g
        lam_err = np.sqrt(f * np.sum((jl - jl.mean(axis=0)) ** 2, axis=0))
        purity_err = float(np.sqrt(f * np.sum((jp - jp.mean()) ** 2)))
    return NaturalOrbitals(k, lam, lam_err, vec, float(lam[0] / n),
                           float(lam_err[0] / n), purity, purity_err,
                           float(np.trace(k)))


def momentum_from_matrix(matrix, momenta, supercell_size):
    """Momentum distribution of a grid matrix K[M, M]
    (`natural_orbitals(...).matrix`): n(k) = (1 / M) v^dagger K v with
    v_a = exp(-i k x_a) on the cell centres x_a -> n[len(momenta)].  Over the M
    momenta 2 pi m / L, m = 0 .. M - 1, the values add up to Tr K."""
    k = np.asarray(matrix, dtype=np.float64)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError('a square matrix K[M, M] expected')
    m = k.shape[0]
    q = np.atleast_1d(np.asarray(momenta, dtype=np.float64))
    x = one_body_matrix_points(supercell_size, m)
    v = np.exp(-1j * q[:, None] * x[None, :])                  # [Q, M]
    return np.real(np.einsum('qa,ab,qb->q', np.conj(v), k, v)) / m


def _pos2d(pos, num_particles,
           expected='pos must have shape (W, boson_number)'):
    """pos as a contiguous fp64 [rows, num_particles] array."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != num_particles:
        raise ValueError(expected)
    return pos


class DeviceBuffer:
    """A plain fp64 array in HBM (qmc_buffer_*): inputs / outputs of
    `ModelEngine.evaluate_dev` that stay resident across calls."""

    def __init__(self, shape, device: t.Optional[int] = None):
        self._lib = _lib.load()
        self.shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.nbytes = int(np.prod(self.shape)) * 8
        self.device = _current_device() if device is None else int(device)
        h = C.c_void_p()
        check(self._lib.qmc_buffer_alloc(self.device, self.nbytes, C.byref(h)))
        self._h = h

    @property
    def ptr(self):
        return self._h

    def upload(self, array):
        a = np.ascontiguousarray(array, dtype=np.float64)
        if a.shape != self.shape:
            raise ValueError(f'expected shape {self.shape}, got {a.shape}')
        check(self._lib.qmc_buffer_upload(self._h, a.ctypes.data, a.nbytes))
        return self

    def download(self):
        out = np.empty(self.shape)
        check(self._lib.qmc_buffer_download(out.ctypes.data, self._h,
                                            out.nbytes))
        return out

    def close(self):
        if getattr(self, '_h', None):
            self._lib.qmc_buffer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelEngine:
    """Model constants bound to one GPU + stream (qmc_engine).

    `stream=None`: the engine creates its own non-blocking stream.
    `stream=<int>`: the caller's hipStream_t handle, used as it is -- 0 is the
    legacy default stream, which is what `torch.cuda.current_stream()
    .cuda_stream` returns unless a side stream is current.  Pass the stream
    torch is using whenever torch.distributed (RCCL) collectives must be
    ordered with the engine's kernels (`dist.DistributedDmc` checks it)."""

    def __init__(self, cfc_spec, device: t.Optional[int] = None,
                 stream: t.Optional[int] = None, fast_math: bool = False):
        self._lib = _lib.load()
        self.cfc_spec = cfc_spec
        self.num_particles = int(cfc_spec.model_params.boson_number)
        self.device = _current_device() if device is None else int(device)
        self._params = model_params_struct(cfc_spec)
        h = C.c_void_p()
        if stream is None:
            check(self._lib.qmc_engine_create(C.byref(self._params),
                                              self.device, None, C.byref(h)))
        else:
            check(self._lib.qmc_engine_create_on_stream(
                C.byref(self._params), self.device, C.c_void_p(int(stream)),
                C.byref(h)))
        self._h = h
        self.fast_math = False
        if fast_math:
            self.set_fast_math(True)

    def set_fast_math(self, on: bool) -> bool:
        """The reference's `jit_fastmath` knob: float pair loop (tables, sums
        over walkers, one-body factor, logs and the Metropolis test stay in
        double).  -> whether the variant is in effect for this model (it
        exists for boson_number > 32 and cutoffs not close to L/2)."""
        eff = C.c_int(0)
        check(self._lib.qmc_engine_set_fast_math(self._h, int(bool(on)),
                                                 C.byref(eff)))
        self.fast_math = bool(eff.value)
        return self.fast_math

    @property
    def stream_handle(self) -> int:
        """hipStream_t the engine launches on (0 = legacy default stream)."""
        st, owned = C.c_void_p(), C.c_int(0)
        check(self._lib.qmc_engine_stream(self._h, C.byref(st),
                                          C.byref(owned)))
        return int(st.value or 0)

    @property
    def owns_stream(self) -> bool:
        st, owned = C.c_void_p(), C.c_int(0)
        check(self._lib.qmc_engine_stream(self._h, C.byref(st),
                                          C.byref(owned)))
        return bool(owned.value)

    def profile_begin(self, max_launches: int = 4096):
        """Start timing every launch of the dominant kernel (one HIP event
        pair each, on the engine's stream)."""
        check(self._lib.qmc_engine_profile_begin(self._h, int(max_launches)))

    def profile_end(self):
        """-> (launches, total_ms, min_ms, max_ms); synchronises."""
        n = C.c_int64(0)
        tot, mn, mx = C.c_double(0), C.c_double(0), C.c_double(0)
        check(self._lib.qmc_engine_profile_end(self._h, C.byref(n),
                                               C.byref(tot), C.byref(mn),
                                               C.byref(mx)))
        return int(n.value), float(tot.value), float(mn.value), float(mx.value)

    def section_profile(self, reset: bool = True):
        """Diagnostic libraries only (built with -DQMC_TIMING,
        tools/section_times.py): {section name: (cycles, visits)} of wavefront
        lifetime per kernel section since the last reset; names ending in
        '@energy' are the sections inside the energy pass of the VMC step.
        Raises with the shipped library."""
        nsec = 32
        cyc = (C.c_uint64 * nsec)()
        vis = (C.c_uint64 * nsec)()
        check(self._lib.qmc_engine_section_profile(self._h, cyc, vis, nsec,
                                                   int(reset)))
        out = {}
        for i in range(nsec):
            if vis[i]:
                name = self._lib.qmc_section_name(i).decode()
                if i >= nsec // 2:
                    name += '@energy'
                out[name] = (int(cyc[i]), int(vis[i]))
        return out

    def section_cut(self, section: int):
        """Diagnostic libraries only (built with -DQMC_CUTS,
        tools/section_counts.py): end every wavefront of the walker kernels at
        section mark `section` (-1: never).  Raises with the shipped library."""
        check(self._lib.qmc_engine_section_cut(self._h, int(section)))

    def general_path_walkers(self, reset: bool = True) -> int:
        """Walker evaluations of the VMC / DMC stepping kernels that left the
        sorted-row pair sums (33 <= N <= 128) for the general one inside the
        same kernel since the last reset: 0 on equilibrated boxes, > 0 for
        clustered walkers (a device counter on the cold path only)."""
        out = (C.c_uint64 * 4)()
        check(self._lib.qmc_engine_diag_counters(self._h, out, 4, int(reset)))
        return int(out[0])

    # qmc_engine_probe function ids (include/qmcwalk.h QMC_PROBE_*): name ->
    # (id, input width, output width)
    PROBE_FUNCS = {
        'fast_div': (0, 2, 1), 'pair_div': (1, 2, 1), 'pair_div_f32': (2, 2, 1),
        'fast_rcp': (3, 1, 1), 'fast_sqrt': (4, 1, 1),
        'sincos_kernel': (5, 1, 2), 'sincos_halfpi': (6, 1, 2),
        'exp_bounded': (7, 1, 1), 'log_pos': (8, 1, 1), 'wrap_box': (9, 1, 1),
        'trig_tab': (10, 1, 5), 'one_body_tab': (11, 1, 3),
        'one_body': (12, 1, 4), 'vmc_move_unit': (13, 1, 1),
        'normal2_words': (14, 2, 2), 'normal2_uniforms': (15, 2, 2),
        'philox2x32': (16, 3, 2), 'philox4x32': (17, 6, 4),
    }

    def probe(self, fn: str, inputs) -> np.ndarray:
        """Diagnostic: the device primitive `fn` of the shipped kernels on
        `inputs` [n, in_width] (or [n] for one input) with this engine's
        model and tables -> [n, out_width] (see qmc_engine_probe).  Inputs run
        64 to a wavefront, in order."""
        fid, nin, nout = self.PROBE_FUNCS[fn]
        x = np.ascontiguousarray(np.asarray(inputs, dtype=np.float64)
                                 .reshape(-1, nin))
        out = np.empty((x.shape[0], nout))
        check(self._lib.qmc_engine_probe(self._h, fid, x.shape[0],
                                         ptr(x), ptr(out)))
        return out

    def section_names(self):
        return [self._lib.qmc_section_name(i).decode() for i in range(16)]

    def close(self):
        if getattr(self, '_h', None):
            self._lib.qmc_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.qmc_engine_sync(self._h))

    def timer_start(self):
        check(self._lib.qmc_engine_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        check(self._lib.qmc_engine_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    def evaluate(self, pos) -> EvalResult:
        """log|psi|, local energy, per-particle energy and drift of every
        configuration in pos[W, N]."""
        pos = _pos2d(pos, self.num_particles)
        W, n = pos.shape
        wf, en = np.zeros(W), np.zeros(W)
        ith, dr = np.zeros((W, n)), np.zeros((W, n))
        check(self._lib.qmc_evaluate(self._h, W, ptr(pos), ptr(wf), ptr(en),
                                     ptr(ith), ptr(dr)))
        return EvalResult(wf, en, ith, dr)

    def evaluate_dev(self, nconf, pos_ptr, wf_ptr=0, energy_ptr=0, ith_ptr=0,
                     drift_ptr=0):
        """Asynchronous evaluation on device-resident buffers (raw pointers,
        e.g. torch `tensor.data_ptr()`)."""
        check(self._lib.qmc_evaluate_dev(self._h, int(nconf), pos_ptr, wf_ptr,
                                         energy_ptr, ith_ptr, drift_ptr))

    def _shifts(self, shifts):
        sh = np.ascontiguousarray(shifts, dtype=np.float64)
        if sh.ndim != 1 or sh.size < 1:
            raise ValueError('shifts must be a non-empty 1-d array')
        return sh

    def one_body_density(self, pos, shifts, ith: bool = False):
        """One-body density matrix g1(s) of every configuration in pos[W, N]
        for every shift -> g1[W, nshift]; with ith=True also the per-particle
        terms -> (g1, ith[W, nshift, N])."""
        pos = _pos2d(pos, self.num_particles)
        sh = self._shifts(shifts)
        W, n = pos.shape
        g1 = np.zeros((W, sh.size))
        parts = np.zeros((W, sh.size, n)) if ith else None
        check(self._lib.qmc_obdm(self._h, W, ptr(pos), sh.size, ptr(sh),
                                 ptr(g1), ptr(parts)))
        return (g1, parts) if ith else g1

    def one_body_density_dev(self, nconf, pos_ptr, nshift, shifts_ptr, g1_ptr,
                             ith_ptr=0):
        """Asynchronous g1 on device-resident buffers (raw pointers):
        pos[nconf, N], shifts[nshift] -> g1[nconf, nshift] and, unless 0,
        ith[nconf, nshift, N]."""
        check(self._lib.qmc_obdm_dev(self._h, int(nconf), pos_ptr, int(nshift),
                                     shifts_ptr, g1_ptr, ith_ptr))

    def one_body_density_reduce_dev(self, nconf, pos_ptr, w_ptr, nshift,
                                    shifts_ptr, sums_ptr, wsum_ptr=0):
        """Asynchronous weighted sums over the configurations, device buffers:
        sums[nshift, 2] = sum_c w_c g1_c, sum_c w_c g1_c^2 and wsum[0] =
        sum_c w_c (w_ptr = 0: unit weights), in a fixed summation order."""
        check(self._lib.qmc_obdm_reduce_dev(self._h, int(nconf), pos_ptr,
                                            w_ptr, int(nshift), shifts_ptr,
                                            sums_ptr, wsum_ptr))

    def _weighted_mean(self, pos, weights, num_out, extra, reduce):
        """sum_c w_c x_c / sum_c w_c of the `num_out` per-configuration values
        x_c that `reduce(nconf, pos_ptr, w_ptr, *extra_ptrs, sums_ptr,
        wsum_ptr)` sums on the device (one upload of the positions and of the
        host arrays `extra`)."""
        expected = 'pos[W, boson_number] and weights[W] expected'
        pos = _pos2d(pos, self.num_particles, expected)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (pos.shape[0],):
            raise ValueError(expected)
        bufs = [DeviceBuffer(x.shape, self.device).upload(x)
                for x in (pos, w, *extra)]
        bufs += [DeviceBuffer((num_out, 2), self.device),
                 DeviceBuffer((1,), self.device)]
        try:
            reduce(pos.shape[0], *(b.ptr for b in bufs))
            self.sync()
            sums, wsum = bufs[-2].download(), bufs[-1].download()
        finally:
            for b in bufs:
                b.close()
        return sums[:, 0] / wsum[0]

    def one_body_density_weighted(self, pos, weights, shifts):
        """sum_c w_c g1_c(s) / sum_c w_c over the configurations pos[W, N]
        (one upload of the positions, the weighted reduction on the device)
        -> g1[nshift]."""
        sh = self._shifts(shifts)
        return self._weighted_mean(
            pos, weights, sh.size, [sh],
            lambda nconf, pos_ptr, w_ptr, sh_ptr, sums_ptr, wsum_ptr:
            self.one_body_density_reduce_dev(nconf, pos_ptr, w_ptr, sh.size,
                                             sh_ptr, sums_ptr, wsum_ptr))

    @staticmethod
    def _num_bins(num_bins):
        nb = int(num_bins)
        if nb != num_bins or not 1 <= nb <= MAX_PAIR_DIST_BINS:
            raise ValueError('num_bins must be an integer in [1, %d]'
                             % MAX_PAIR_DIST_BINS)
        return nb

    def pair_distribution(self, pos, num_bins):
        """Pair-distance histogram of every configuration in pos[W, N]:
        counts[W, num_bins] (uint32) of the unordered pairs over num_bins
        uniform bins of the minimum-image distance in [0, L/2]; every row adds
        up to N (N - 1) / 2.  `pair_distribution_norm` turns counts into
        g2."""
        pos = _pos2d(pos, self.num_particles)
        nb = self._num_bins(num_bins)
        counts = np.zeros((pos.shape[0], nb), dtype=np.uint32)
        check(self._lib.qmc_pair_dist(self._h, pos.shape[0], ptr(pos), nb,
                                      ptr(counts, _lib._u32p)))
        return counts

    def pair_distribution_dev(self, nconf, pos_ptr, num_bins, counts_ptr):
        """Asynchronous histograms on device-resident buffers (raw pointers):
        pos[nconf, N] (fp64) -> counts[nconf, num_bins] (uint32)."""
        check(self._lib.qmc_pair_dist_dev(self._h, int(nconf), pos_ptr,
                                          int(num_bins), counts_ptr))

    def pair_distribution_reduce_dev(self, nconf, pos_ptr, w_ptr, num_bins,
                                     sums_ptr, wsum_ptr=0):
        """Asynchronous weighted sums over the configurations, device buffers:
        sums[num_bins, 2] = sum_c w_c H_c, sum_c w_c H_c^2 and wsum[0] =
        sum_c w_c (w_ptr = 0: unit weights), in a fixed summation order."""
        check(self._lib.qmc_pair_dist_reduce_dev(self._h, int(nconf), pos_ptr,
                                                 w_ptr, int(num_bins),
                                                 sums_ptr, wsum_ptr))

    def pair_distribution_weighted(self, pos, weights, num_bins):
        """sum_c w_c H_c / sum_c w_c over the configurations pos[W, N] (one
        upload of the positions, the weighted reduction on the device)
        -> mean histogram[num_bins]."""
        nb = self._num_bins(num_bins)
        return self._weighted_mean(
            pos, weights, nb, [],
            lambda nconf, pos_ptr, w_ptr, sums_ptr, wsum_ptr:
            self.pair_distribution_reduce_dev(nconf, pos_ptr, w_ptr, nb,
                                              sums_ptr, wsum_ptr))

    def _span(self, max_span):
        return _max_span(self.cfc_spec.model_params.supercell_size, max_span)

    def triple_distribution(self, pos, num_bins, max_span=None):
        """Triple-span histogram of every configuration in pos[W, N]:
        counts[W, num_bins + 1] (uint32) of the unordered triples over num_bins
        uniform bins of the span (the shortest arc that holds the three) in
        [0, max_span) and one overflow bin; max_span in (0, L/2], None = L/2.
        Every row adds up to N (N - 1) (N - 2) / 6.
        `triple_distribution_norm` turns counts into g3."""
        pos = _pos2d(pos, self.num_particles)
        nb, span = self._num_bins(num_bins), self._span(max_span)
        counts = np.zeros((pos.shape[0], nb + 1), dtype=np.uint32)
        check(self._lib.qmc_triple_dist(self._h, pos.shape[0], ptr(pos), nb,
                                        span, ptr(counts, _lib._u32p)))
        return counts

    def triple_distribution_dev(self, nconf, pos_ptr, num_bins, max_span,
                                counts_ptr):
        """Asynchronous histograms on device-resident buffers (raw pointers):
        pos[nconf, N] (fp64) -> counts[nconf, num_bins + 1] (uint32)."""
        check(self._lib.qmc_triple_dist_dev(self._h, int(nconf), pos_ptr,
                                            int(num_bins),
                                            self._span(max_span), counts_ptr))

    def triple_distribution_reduce_dev(self, nconf, pos_ptr, w_ptr, num_bins,
                                       max_span, sums_ptr, wsum_ptr=0):
        """Asynchronous weighted sums over the configurations, device buffers:
        sums[num_bins + 1, 2] = sum_c w_c T_c, sum_c w_c T_c^2 and wsum[0] =
        sum_c w_c (w_ptr = 0: unit weights), in a fixed summation order."""
        check(self._lib.qmc_triple_dist_reduce_dev(
            self._h, int(nconf), pos_ptr, w_ptr, int(num_bins),
            self._span(max_span), sums_ptr, wsum_ptr))

    def triple_distribution_weighted(self, pos, weights, num_bins,
                                     max_span=None):
        """sum_c w_c T_c / sum_c w_c over the configurations pos[W, N] (one
        upload of the positions, the weighted reduction on the device)
        -> mean histogram[num_bins + 1]."""
        nb, span = self._num_bins(num_bins), self._span(max_span)
        return self._weighted_mean(
            pos, weights, nb + 1, [],
            lambda nconf, pos_ptr, w_ptr, sums_ptr, wsum_ptr:
            self.triple_distribution_reduce_dev(nconf, pos_ptr, w_ptr, nb,
                                                span, sums_ptr, wsum_ptr))

    def _ranges(self, contact_ranges):
        rg = contact_ranges_array(self.cfc_spec, contact_ranges)
        return rg, (ptr(rg) if rg.size else None)

    def energy_parts(self, pos, contact_ranges=()):
        """The local energy of every configuration in pos[W, N] in parts
        -> parts[W, 4 + K]: E (as `evaluate`), T = sum_i F_i^2 (F the drift),
        V = sum_i V(z_i) (the lattice potential the energy contains),
        I = (E - T) - V, and the windowed contact C_k of every window in
        `contact_ranges` (K <= 16, `contact_ranges_array`):
        1 / (2 r_k) sum_{i<j, d_ij < r_k} f2(0)^2 / f2(d_ij)^2.  Over |psi|^2,
        <T> is the kinetic energy and <I> = g <C_k> + O(r_k^2) the interaction
        energy, g = `contact_coupling`.  Always fp64."""
        pos = _pos2d(pos, self.num_particles)
        rg, rg_ptr = self._ranges(contact_ranges)
        parts = np.zeros((pos.shape[0], ENERGY_PARTS_COLS + rg.size))
        check(self._lib.qmc_energy_parts(self._h, pos.shape[0], ptr(pos),
                                         rg.size, rg_ptr, ptr(parts)))
        return parts

    def energy_parts_dev(self, nconf, pos_ptr, contact_ranges, parts_ptr):
        """Asynchronous rows on device-resident buffers (raw pointers):
        pos[nconf, N] -> parts[nconf, 4 + K]; `contact_ranges` is a host
        sequence."""
        rg, rg_ptr = self._ranges(contact_ranges)
        check(self._lib.qmc_energy_parts_dev(self._h, int(nconf), pos_ptr,
                                             rg.size, rg_ptr, parts_ptr))

    def energy_parts_reduce_dev(self, nconf, pos_ptr, w_ptr, contact_ranges,
                                sums_ptr, wsum_ptr=0):
        """Asynchronous weighted sums over the configurations, device buffers:
        sums[4 + K, 2] = sum_c w_c x_c, sum_c w_c x_c^2 of every column and
        wsum[0] = sum_c w_c (w_ptr = 0: unit weights), in a fixed summation
        order; `contact_ranges` is a host sequence."""
        rg, rg_ptr = self._ranges(contact_ranges)
        check(self._lib.qmc_energy_parts_reduce_dev(
            self._h, int(nconf), pos_ptr, w_ptr, rg.size, rg_ptr, sums_ptr,
            wsum_ptr))

    def energy_parts_weighted(self, pos, weights, contact_ranges=()):
        """Weighted sums of the rows of `energy_parts` over the configurations
        pos[W, N] with weights[W] (one upload of the positions, the reduction
        on the device) -> (sums[4 + K, 2], wsum): what `energy_components`
        takes."""
        expected = 'pos[W, boson_number] and weights[W] expected'
        pos = _pos2d(pos, self.num_particles, expected)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (pos.shape[0],):
            raise ValueError(expected)
        rg, _ = self._ranges(contact_ranges)
        bufs = [DeviceBuffer(pos.shape, self.device).upload(pos),
                DeviceBuffer(w.shape, self.device).upload(w),
                DeviceBuffer((ENERGY_PARTS_COLS + rg.size, 2), self.device),
                DeviceBuffer((1,), self.device)]
        try:
            self.energy_parts_reduce_dev(pos.shape[0], bufs[0].ptr,
                                         bufs[1].ptr, rg, bufs[2].ptr,
                                         bufs[3].ptr)
            self.sync()
            sums, wsum = bufs[2].download(), bufs[3].download()
        finally:
            for b in bufs:
                b.close()
        return sums, float(wsum[0])

    def _lengths(self, lengths):
        return renyi_lengths(self.cfc_spec.model_params.supercell_size,
                             lengths)

    @staticmethod
    def _num_replicas(nconf):
        nconf = int(nconf)
        if nconf < 2 or nconf % 2:
            raise ValueError('an even, positive number of configurations '
                             'expected: rows 2p and 2p + 1 are a replica pair')
        return nconf

    def renyi_swap(self, pos, lengths, origin=0.0):
        """Replica swap of the segments A_k = [origin, origin + lengths[k]) of
        the ring between the rows (2p, 2p + 1) of pos[W, N], W even
        -> (n_a[W, K] (int32), log_ratio[W / 2, K]): the particles of every
        row inside A_k, and ln|psi(R1') psi(R2') / (psi(R1) psi(R2))| of the
        pair with its particles inside A_k exchanged, -inf where the two rows
        hold different numbers there.  swap = exp(log_ratio);
        S2 = -ln(mean swap) over independent pairs drawn from |psi|^2
        (`renyi_entropy`)."""
        pos = _pos2d(pos, self.num_particles)
        ln, a0 = self._lengths(lengths), _renyi_origin(origin)
        W = self._num_replicas(pos.shape[0])
        n_a = np.zeros((W, ln.size), dtype=np.int32)
        log_ratio = np.zeros((W // 2, ln.size))
        check(self._lib.qmc_renyi_swap(self._h, W, ptr(pos), ln.size, ptr(ln),
                                       a0, ptr(n_a, _lib._i32p),
                                       ptr(log_ratio)))
        return n_a, log_ratio

    def renyi_swap_dev(self, nconf, pos_ptr, nlen, lengths_ptr, origin,
                       n_a_ptr, log_ratio_ptr):
        """Asynchronous replica swap on device-resident buffers (raw
        pointers): pos[nconf, N], lengths[nlen] (fp64) -> n_a[nconf, nlen]
        (int32) and log_ratio[nconf / 2, nlen]; either output may be 0."""
        check(self._lib.qmc_renyi_swap_dev(
            self._h, self._num_replicas(nconf), pos_ptr, int(nlen),
            lengths_ptr, _renyi_origin(origin), n_a_ptr, log_ratio_ptr))

    def renyi_swap_reduce_dev(self, nconf, pos_ptr, nlen, lengths_ptr, origin,
                              sums_ptr):
        """Asynchronous sums over the nconf / 2 replica pairs, device buffers:
        sums[nlen, 3] = sum swap, sum swap^2, matched pairs, in a fixed
        summation order (`renyi_entropy` turns them into S2)."""
        check(self._lib.qmc_renyi_swap_reduce_dev(
            self._h, self._num_replicas(nconf), pos_ptr, int(nlen),
            lengths_ptr, _renyi_origin(origin), sums_ptr))

    def _regions(self, regions):
        return renyi_regions(self.cfc_spec.model_params.supercell_size,
                             regions)

    def renyi_region_swap(self, pos, regions, origin=0.0):
        """Replica swap of the regions X_k = regions[k] = (l1, g, l2) -- the
        segments [origin, origin + l1) and [origin + l1 + g,
        origin + l1 + g + l2) of the ring; l2 = 0 is a single segment --
        between the rows (2p, 2p + 1) of pos[W, N], W even
        -> (n_x[W, K] (int32), log_ratio[W / 2, K]): the particles of every
        row inside X_k, and ln|psi(R1') psi(R2') / (psi(R1) psi(R2))| of the
        pair with its particles inside X_k exchanged, -inf where the two rows
        hold different totals there.  S2(X) = -ln(mean exp(log_ratio)) over
        independent pairs drawn from |psi|^2; I2 = S2(A) + S2(C) - S2(A u C)
        (`renyi_mutual_information`)."""
        pos = _pos2d(pos, self.num_particles)
        rg, a0 = self._regions(regions), _renyi_origin(origin)
        W = self._num_replicas(pos.shape[0])
        n_x = np.zeros((W, rg.shape[0]), dtype=np.int32)
        log_ratio = np.zeros((W // 2, rg.shape[0]))
        check(self._lib.qmc_renyi_region_swap(
            self._h, W, ptr(pos), rg.shape[0], ptr(rg), a0,
            ptr(n_x, _lib._i32p), ptr(log_ratio)))
        return n_x, log_ratio

    def renyi_region_swap_dev(self, nconf, pos_ptr, nreg, regions_ptr, origin,
                              n_x_ptr, log_ratio_ptr):
        """Asynchronous region swap on device-resident buffers (raw
        pointers): pos[nconf, N], regions[nreg, 3] (fp64) -> n_x[nconf, nreg]
        (int32) and log_ratio[nconf / 2, nreg]; either output may be 0."""
        check(self._lib.qmc_renyi_region_swap_dev(
            self._h, self._num_replicas(nconf), pos_ptr, int(nreg),
            regions_ptr, _renyi_origin(origin), n_x_ptr, log_ratio_ptr))

    def renyi_region_swap_reduce_dev(self, nconf, pos_ptr, nreg, regions_ptr,
                                     origin, num_charges, sums_ptr):
        """Asynchronous sums over the nconf / 2 replica pairs, device buffers:
        sums[nreg, 3 + 2 Q] = sum swap, sum swap^2, matched pairs, then per
        charge n < Q = num_charges sum swap [n_X(R1) = n] and the number of
        configurations with n particles in the region, in a fixed summation
        order (`renyi_resolved` turns them into entropies)."""
        check(self._lib.qmc_renyi_region_swap_reduce_dev(
            self._h, self._num_replicas(nconf), pos_ptr, int(nreg),
            regions_ptr, _renyi_origin(origin), int(num_charges), sums_ptr))

    def particle_swap(self, pos, matrix=False):
        """One-particle replica swap between the rows (2p, 2p + 1) of
        pos[W, N], W even, N <= 512 -> mean[W / 2], or with `matrix`
        (mean, log_ratio[W / 2, N, N]): log_ratio[p, i, j] is
        ln|psi(R1') psi(R2') / (psi(R1) psi(R2))| for the exchange of particle
        i of row 2p with particle j of row 2p + 1, and mean[p] the average of
        exp(log_ratio[p]) over all N^2 exchanges, which does not depend on the
        order of the particles in a row.  The mean over independent pairs drawn
        from |psi|^2 is the purity Tr rho1^2 of the one-body density matrix
        (`particle_entropy`)."""
        pos = _pos2d(pos, self.num_particles)
        W, n = self._num_replicas(pos.shape[0]), self.num_particles
        mean = np.zeros(W // 2)
        log_ratio = np.zeros((W // 2, n, n)) if matrix else None
        check(self._lib.qmc_particle_swap(self._h, W, ptr(pos), ptr(mean),
                                          ptr(log_ratio)))
        return (mean, log_ratio) if matrix else mean

    def particle_swap_dev(self, nconf, pos_ptr, mean_ptr, log_ratio_ptr):
        """Asynchronous one-particle swap on device-resident buffers (raw
        pointers): pos[nconf, N] -> mean[nconf / 2] and
        log_ratio[nconf / 2, N, N]; either output may be 0."""
        check(self._lib.qmc_particle_swap_dev(
            self._h, self._num_replicas(nconf), pos_ptr, mean_ptr,
            log_ratio_ptr))

    def particle_swap_reduce_dev(self, nconf, pos_ptr, sums_ptr):
        """Asynchronous sums over the P = nconf / 2 replica pairs, device
        buffers: sums[3] = sum mean, sum mean^2, P, in a fixed summation order
        (`particle_entropy` turns them into the purity and S2)."""
        check(self._lib.qmc_particle_swap_reduce_dev(
            self._h, self._num_replicas(nconf), pos_ptr, sums_ptr))


    def one_body_matrix(self, pos, num_points, num_groups=1, weights=None):
        """The one-body density matrix on a grid, summed over the
        configurations pos[W, N] in `num_groups` = G independent groups
        (configuration index mod G) -> (sums[G, M, M], wsum[G]), M =
        `num_points`:

            sums[g, a, c] = sum_{conf in g} w_conf sum_{i in cell a}
                            psi(.. z_i -> x_c ..) / psi(R)

        with the cells and centres of `one_body_matrix_points` (a particle
        counts in the cell that holds its image in [0, L)) and unit weights
        for `weights` None; wsum[g] is the sum of the weights of the group.
        sum_g sums / sum_g wsum estimates int_{cell a} rho1(x, x_c) dx;
        `natural_orbitals` diagonalises it.  M in [1, 512], G in
        [1, min(1024, W)]; the particles of a row may come in any order; two
        calls give the same bits."""
        pos = _pos2d(pos, self.num_particles)
        m, g = _obdm_grid_args(num_points, num_groups, pos.shape[0])
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (pos.shape[0],):
                raise ValueError('weights must have one entry per '
                                 'configuration')
        sums, wsum = np.zeros((g, m, m)), np.zeros(g)
        check(self._lib.qmc_obdm_grid(self._h, pos.shape[0], ptr(pos), ptr(w),
                                      m, g, ptr(sums), ptr(wsum)))
        return sums, wsum

    def one_body_matrix_dev(self, nconf, pos_ptr, w_ptr, num_points,
                            num_groups, sums_ptr, wsum_ptr=0):
        """Asynchronous `one_body_matrix` on device-resident buffers (raw
        pointers): pos[nconf, N], w[nconf] (0: unit weights) ->
        sums[G, M, M] and wsum[G] (0: not wanted)."""
        check(self._lib.qmc_obdm_grid_dev(self._h, int(nconf), pos_ptr, w_ptr,
                                          int(num_points), int(num_groups),
                                          sums_ptr, wsum_ptr))


#: VmcEnsemble(move=...) -> qmc_vmc_params.gaussian (the proposal code;
#: 1 is the Gaussian all-particle proposal, `gaussian=True`)
VMC_MOVES = {'all': 0, 'particle': 2}


def vmc_move_code(name) -> int:
    """The C ABI's code of a move type; ValueError for an unknown one."""
    if not isinstance(name, str) or name not in VMC_MOVES:
        raise ValueError(f'unknown VMC move {name!r}: one of '
                         f'{sorted(VMC_MOVES)}')
    return VMC_MOVES[name]


class VmcEnsemble:
    """W independent Metropolis chains resident on the GPU (qmc_vmc).

    `move`: 'all' -- the reference's step, every particle displaced at once
    -- or 'particle', an extension: one yield is a SWEEP of N single-particle
    Metropolis moves in label order (the label is the particle's index in the
    rows of `set_state`), each within +- move_spread / 2 and each accepted or
    rejected on its own (csrc/qmc_vmc_sweep.h).  Word 0 of a particle's Philox
    move block displaces it, word 1 of the same block is that move's accept
    draw.  The yielded log|psi| and energy are those of the configuration after
    the sweep, `num_accepted` counts accepted particle moves (the initial yield
    counts N) and `move_stat` says whether any move of the sweep was accepted.
    No tape, no Gaussian proposal, fp64 whatever `set_fast_math` says."""

    def __init__(self, engine: ModelEngine, num_chains: int,
                 move_spread: float, rng_seed: int, chain0: int = 0,
                 gaussian: bool = False, move: str = 'all'):
        code = vmc_move_code(move)
        if code and gaussian:
            raise ValueError("move='particle' has no Gaussian proposal")
        self.move = move
        self.engine = engine
        self._lib = engine._lib
        self.num_chains = int(num_chains)
        self.num_particles = engine.num_particles
        p = VmcParams(self.num_chains, float(move_spread),
                      int(rng_seed) & 0xFFFFFFFFFFFFFFFF, int(chain0),
                      code or int(bool(gaussian)))
        h = C.c_void_p()
        check(self._lib.qmc_vmc_create(engine._h, C.byref(p), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            self._lib.qmc_vmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, pos):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.shape != (self.num_chains, self.num_particles):
            raise ValueError('pos must have shape (num_chains, boson_number)')
        check(self._lib.qmc_vmc_set_state(self._h, ptr(pos)))

    def ssf_parts(self, num_modes: int) -> np.ndarray:
        """Mean over the chains of the S(k) parts (|rho_k|^2, Re rho_k,
        Im rho_k) of the current configurations, k_m = 2 pi m / L,
        m < num_modes -> [num_modes, 3]."""
        out = np.zeros((int(num_modes), 3))
        check(self._lib.qmc_vmc_ssf(self._h, int(num_modes), ptr(out)))
        return out / self.num_chains

    def obdm_parts(self, shifts) -> np.ndarray:
        """Sums over the chains of g1(s) and g1(s)^2 of the current
        configurations -> [nshift, 2]; computed on the resident rows."""
        sh = self.engine._shifts(shifts)
        out = np.zeros((sh.size, 2))
        check(self._lib.qmc_vmc_obdm(self._h, sh.size, ptr(sh), ptr(out)))
        return out

    def pair_dist_parts(self, num_bins) -> np.ndarray:
        """Sums over the chains of the pair-distance histogram H and of H^2
        of the current configurations -> [num_bins, 2]; computed on the
        resident rows, which are only read."""
        nb = ModelEngine._num_bins(num_bins)
        out = np.zeros((nb, 2))
        check(self._lib.qmc_vmc_pair_dist(self._h, nb, ptr(out)))
        return out

    def triple_dist_parts(self, num_bins, max_span=None) -> np.ndarray:
        """Sums over the chains of the triple-span histogram T and of T^2 of
        the current configurations -> [num_bins + 1, 2]; computed on the
        resident rows, which are only read."""
        nb = ModelEngine._num_bins(num_bins)
        span = self.engine._span(max_span)
        out = np.zeros((nb + 1, 2))
        check(self._lib.qmc_vmc_triple_dist(self._h, nb, span, ptr(out)))
        return out

    def renyi_parts(self, lengths, origin=0.0) -> np.ndarray:
        """Replica-swap sums of the current configurations, the chains 2p and
        2p + 1 being the replicas of pair p -> [K, 3] = sum swap, sum swap^2,
        matched pairs (`ModelEngine.renyi_swap_reduce_dev`); computed on the
        resident rows, which are only read.  An odd number of chains is a
        ValueError."""
        ln, a0 = self.engine._lengths(lengths), _renyi_origin(origin)
        ModelEngine._num_replicas(self.num_chains)
        out = np.zeros((ln.size, 3))
        check(self._lib.qmc_vmc_renyi_swap(self._h, ln.size, ptr(ln), a0,
                                           ptr(out)))
        return out

    def renyi_region_parts(self, regions, origin=0.0,
                           num_charges=0) -> np.ndarray:
        """Region swap sums of the current configurations, the chains 2p and
        2p + 1 being the replicas of pair p -> [K, 3 + 2 num_charges]
        (`ModelEngine.renyi_region_swap_reduce_dev`; None collects every
        charge, N + 1 of them); computed on the resident rows, which are only
        read.  An odd number of chains is a ValueError."""
        rg, a0 = self.engine._regions(regions), _renyi_origin(origin)
        q = _num_charges(num_charges, self.num_particles, rg.shape[0])
        ModelEngine._num_replicas(self.num_chains)
        out = np.zeros((rg.shape[0], 3 + 2 * q))
        check(self._lib.qmc_vmc_renyi_region_swap(
            self._h, rg.shape[0], ptr(rg), a0, q, ptr(out)))
        return out

    def particle_swap_parts(self) -> np.ndarray:
        """One-particle swap sums of the current configurations, the chains 2p
        and 2p + 1 being the replicas of pair p -> [3] = sum mean,
        sum mean^2, pairs (`ModelEngine.particle_swap_reduce_dev`); computed
        on the resident rows, which are only read.  An odd number of chains is
        a ValueError."""
        ModelEngine._num_replicas(self.num_chains)
        out = np.zeros(3)
        check(self._lib.qmc_vmc_particle_swap(self._h, ptr(out)))
        return out

    def obdm_grid_parts(self, num_points, num_groups) -> np.ndarray:
        """Density-matrix sums on a grid of the current configurations, group
        = chain index mod `num_groups`, unit weights -> sums[G, M, M]
        (`ModelEngine.one_body_matrix`; every group's weight sum is its number
        of chains); computed on the resident rows, which are only read."""
        m, g = _obdm_grid_args(num_points, num_groups, self.num_chains)
        out = np.zeros((g, m, m))
        check(self._lib.qmc_vmc_obdm_grid(self._h, m, g, ptr(out)))
        return out

    def energy_parts_parts(self, contact_ranges=()) -> np.ndarray:
        """Sums over the chains of every column of `ModelEngine.energy_parts`
        and of its square for the current configurations -> [4 + K, 2];
        computed on the resident rows, which are only read."""
        rg, rg_ptr = self.engine._ranges(contact_ranges)
        out = np.zeros((ENERGY_PARTS_COLS + rg.size, 2))
        check(self._lib.qmc_vmc_energy_parts(self._h, rg.size, rg_ptr,
                                             ptr(out)))
        return out

    def get_state(self):
        """-> (pos[W, N], wf_abs_log[W], energy_carry[W])"""
        W, n = self.num_chains, self.num_particles
        pos, wf, ec = np.zeros((W, n)), np.zeros(W), np.zeros(W)
        check(self._lib.qmc_vmc_get_state(self._h, ptr(pos), ptr(wf), ptr(ec)))
        return pos, wf, ec

    def set_tape(self, tape):
        """TEST ONLY: tape[W, steps, N + 1]."""
        if tape is None:
            check(self._lib.qmc_vmc_set_tape(self._h, None, 0))
            return
        tape = np.ascontiguousarray(tape, dtype=np.float64)
        assert tape.ndim == 3 and tape.shape[0] == self.num_chains \
            and tape.shape[2] == self.num_particles + 1
        check(self._lib.qmc_vmc_set_tape(self._h, ptr(tape), tape.shape[1]))

    def run_block(self, nyield: int, sums: bool = True, series: bool = False,
                  confs: bool = False):
        """Advance every chain by `nyield` generator yields.
        -> dict with sum_energy, sum_energy2, num_accepted ([W]) and, if
        `series`, wf_abs_log / energy / move_stat ([nyield, W]) -- move_stat
        alone with series='stat' --; if `confs`, pos ([nyield, W, N])."""
        W = self.num_chains
        out = {}
        se = se2 = na = swf = sen = sst = spos = None
        if confs:
            spos = np.zeros((nyield, W, self.num_particles))
        if sums:
            se, se2 = np.zeros(W), np.zeros(W)
            na = np.zeros(W, dtype=np.int64)
        if series == 'stat':
            # (the move status alone: one byte per chain and yield)
            sst = np.zeros((nyield, W), dtype=np.uint8)
        elif series:
            swf, sen = np.zeros((nyield, W)), np.zeros((nyield, W))
            sst = np.zeros((nyield, W), dtype=np.uint8)
        check(self._lib.qmc_vmc_run_block(self._h, int(nyield), ptr(se),
                                          ptr(se2), ptr(na, _i64p), ptr(swf),
                                          ptr(sen), ptr(sst, _u8p),
                                          ptr(spos)))
        if confs:
            out.update(pos=spos)
        if sums:
            out.update(sum_energy=se, sum_energy2=se2, num_accepted=na)
        if series == 'stat':
            out.update(move_stat=sst.astype(bool))
        elif series:
            out.update(wf_abs_log=swf, energy=sen, move_stat=sst.astype(bool))
        return out

    def state_dev(self):
        """Device addresses (ints) of pos[W, N] and wf[W]."""
        a, b = C.c_void_p(), C.c_void_p()
        check(self._lib.qmc_vmc_state_dev(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def block_sums_dev(self):
        """Device addresses (ints) of sum_e[W], sum_e2[W], n_acc[W]."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self._lib.qmc_vmc_block_sums_dev(self._h, C.byref(a),
                                               C.byref(b), C.byref(c)))
        return a.value, b.value, c.value


class DmcState(t.NamedTuple):
    confs: np.ndarray         # [maxw, 2, N]
    energy: np.ndarray        # [maxw]
    weight: np.ndarray        # [maxw]
    mask: np.ndarray          # [maxw] bool
    cloning_ref: np.ndarray   # [maxw] int64
    state_energy: float
    state_weight: float
    ref_energy: float
    accum_energy: float
    num_walkers: int


class DmcSeries(t.NamedTuple):
    energy: np.ndarray
    weight: np.ndarray
    num_walkers: np.ndarray   # uint64
    ref_energy: np.ndarray
    accum_energy: np.ndarray


#: DmcEnsemble(propagator=...) -> qmc_dmc_params.propagator
DMC_PROPAGATORS = {'linear': 0, 'quadratic': 1}


def dmc_propagator_code(name) -> int:
    """The C ABI's code of a propagator name; ValueError for an unknown one."""
    if not isinstance(name, str) or name not in DMC_PROPAGATORS:
        raise ValueError(f'unknown DMC propagator {name!r}: one of '
                         f'{sorted(DMC_PROPAGATORS)}')
    return DMC_PROPAGATORS[name]


class DmcEnsemble:
    """A walker population resident on the GPU (qmc_dmc).

    `propagator`: 'linear' -- the reference's step z' = wrap(z + 2 F dt +
    sqrt(2 dt) g), time-step error O(dt) -- or 'quadratic', an extension: the
    symmetric split half diffusion, drift (RK2 through the midpoint), half
    diffusion, with the branching weight averaged over the PARENT's and the
    child's energy, error O(dt^2), three pair sums per step
    (csrc/qmc_evolve2.h).  `fix_stale_energy` has no effect with 'quadratic':
    the stale-slot average would break the symmetry the order
    rests on.  Both normals of a particle's Philox block move it in ONE step
    (the block is keyed with the step counter t, not t >> 1); a replay tape
    holds [slot][2][N] normals per step.  The centre-of-mass estimator's
    condition |sum of displacements| < L / 2 per step (csrc/qmc_cmdiff.h)
    holds for either propagator: mind it at the longer steps this one
    allows."""

    def __init__(self, engine: ModelEngine, time_step: float,
                 max_num_walkers: int, target_num_walkers: int,
                 num_walkers_control_factor: float, rng_seed: int,
                 slot0: int = 0, fix_stale_energy: bool = False,
                 external_reduce: bool = False, propagator: str = 'linear'):
        self.propagator = propagator
        code = dmc_propagator_code(propagator)
        self.engine = engine
        self._lib = engine._lib
        self.max_num_walkers = int(max_num_walkers)
        self.num_particles = engine.num_particles
        p = DmcParams(self.max_num_walkers, int(target_num_walkers),
                      float(time_step), float(num_walkers_control_factor),
                      int(rng_seed) & 0xFFFFFFFFFFFFFFFF, int(slot0),
                      int(bool(fix_stale_energy)), int(bool(external_reduce)),
                      code)
        h = C.c_void_p()
        check(self._lib.qmc_dmc_create(engine._h, C.byref(p), C.byref(h)))
        self._h = h
        self.num_modes = self.num_bins = 0
        self.pair_dist_bins = 0
        self.cm_diffusion = False
        self.isf_shape = None
        self.obdm_shifts = None
        self.site_shape = None
        self._record_rows = False

    def close(self):
        if getattr(self, '_h', None):
            self._lib.qmc_dmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, pos, ref_energy: t.Optional[float] = None):
        """build_state semantics: energies and drifts are computed here."""
        pos = _pos2d(pos, self.num_particles,
                     'pos must have shape (nw, boson_number)')
        check(self._lib.qmc_dmc_set_state(
            self._h, pos.shape[0], ptr(pos), int(ref_energy is not None),
            float(ref_energy if ref_energy is not None else 0.0)))

    def set_state_from_vmc(self, vmc: 'VmcEnsemble', num_walkers=None,
                           ref_energy: t.Optional[float] = None,
                           replicate: bool = False):
        """build_state from the current configurations of a VMC ensemble on
        the same engine, device to device (the first `num_walkers` chains;
        with `replicate` more walkers than chains are allowed and the chains
        are reused cyclically)."""
        nw = vmc.num_chains if num_walkers is None else int(num_walkers)
        if nw > vmc.num_chains and not replicate:
            raise ValueError('more walkers requested than chains')
        self.engine.sync()
        check(self._lib.qmc_dmc_set_state_from_vmc(
            self._h, vmc._h, nw, int(ref_energy is not None),
            float(ref_energy if ref_energy is not None else 0.0)))

    def set_full_state(self, confs, energy, weight, ref_energy: float,
                       slot_energy=None):
        confs = np.ascontiguousarray(confs, dtype=np.float64)
        energy = np.ascontiguousarray(energy, dtype=np.float64)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        nw = confs.shape[0]
        assert confs.shape == (nw, 2, self.num_particles)
        assert energy.shape == (nw,) and weight.shape == (nw,)
        if slot_energy is not None:
            slot_energy = np.ascontiguousarray(slot_energy, dtype=np.float64)
            assert slot_energy.shape == (self.max_num_walkers,)
        check(self._lib.qmc_dmc_set_full_state(self._h, nw, ptr(confs),
                                               ptr(energy), ptr(weight),
                                               ptr(slot_energy),
                                               float(ref_energy)))

    def set_tape(self, u, g, u_off, g_off):
        """TEST ONLY: recorded uniforms / standard normals + per-step offsets."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        u_off = np.ascontiguousarray(u_off, dtype=np.int64)
        g_off = np.ascontiguousarray(g_off, dtype=np.int64)
        check(self._lib.qmc_dmc_set_tape(self._h, ptr(u), u.size, ptr(g),
                                         g.size, ptr(u_off, _i64p),
                                         ptr(g_off, _i64p), u_off.size))

    @staticmethod
    def _series(nsteps):
        """-> (DmcSeries of zeros, the pointers to its five arrays)."""
        e, w, r, a = (np.zeros(nsteps) for _ in range(4))
        nw = np.zeros(nsteps, dtype=np.uint64)
        return (DmcSeries(e, w, nw, r, a),
                (ptr(e), ptr(w), ptr(nw, _u64p), ptr(r), ptr(a)))

    def _read_rows(self, fn, nsteps, row_shape):
        out = np.zeros((int(nsteps),) + tuple(row_shape))
        check(fn(self._h, int(nsteps), ptr(out)))
        return out

    def run_block(self, nsteps: int, read: bool = True):
        """`nsteps` time steps; -> DmcSeries (or None when read=False: the
        series stay on the device until `read_series`)."""
        if not read:
            check(self._lib.qmc_dmc_run_block(self._h, int(nsteps), None, None,
                                              None, None, None))
            return None
        ser, ptrs = self._series(nsteps)
        check(self._lib.qmc_dmc_run_block(self._h, int(nsteps), *ptrs))
        return ser

    def set_estimators(self, num_modes=0, ssf_pure=False, ssf_pfw=1,
                       num_bins=0, dens_pure=False, dens_pfw=1):
        """Enable the S(k) / density estimators (0 disables one)."""
        self.num_modes, self.num_bins = int(num_modes), int(num_bins)
        p = DmcEstParams(self.num_modes, int(bool(ssf_pure)), int(ssf_pfw),
                         self.num_bins, int(bool(dens_pure)), int(dens_pfw))
        check(self._lib.qmc_dmc_set_estimators(self._h, C.byref(p)))

    def run_block_est(self, nsteps: int, eval_estimators: bool = True):
        """-> (DmcSeries, iter_ssf[nsteps, M, 3] or None,
        iter_density[nsteps, B, 1] or None)."""
        ser, ptrs = self._series(nsteps)
        ssf = np.zeros((nsteps, self.num_modes, 3)) if self.num_modes else None
        dens = np.zeros((nsteps, self.num_bins, 1)) if self.num_bins else None
        check(self._lib.qmc_dmc_run_block_est(
            self._h, int(nsteps), int(bool(eval_estimators)), *ptrs, ptr(ssf),
            ptr(dens)))
        return ser, ssf, dens

    def set_pair_dist_estimator(self, num_bins, pure=False, pfw=1):
        """Enable the pair distribution estimator g2(r) of the estimator
        blocks: `num_bins` bins over [0, L/2] (1..256; 0 disables it), mixed
        or pure with forward-walking length `pfw`.  Independent of
        `set_estimators`."""
        nb = int(num_bins)
        check(self._lib.qmc_dmc_set_pair_dist_estimator(
            self._h, nb, int(bool(pure)), int(pfw)))
        self.pair_dist_bins = nb

    def read_pair_dist(self, nsteps: int) -> np.ndarray:
        """Rows of the last estimator block -> iter_pair_dist[nsteps, B]:
        per time step the pair histograms summed over the walkers (pure: the
        forward-walking rows over min(step + 1, pfw))."""
        return self._read_rows(self._lib.qmc_dmc_read_pair_dist, nsteps,
                               (self.pair_dist_bins,))

    def set_cm_diffusion_estimator(self, on=True):
        """Enable (or disable) the centre-of-mass diffusion estimator of the
        estimator blocks: the winding-number estimator of the superfluid
        fraction (`superfluid_ratio`).  Independent of `set_estimators` and
        `set_pair_dist_estimator`."""
        check(self._lib.qmc_dmc_set_cm_diffusion_estimator(
            self._h, int(bool(on))))
        self.cm_diffusion = bool(on)

    def read_cm_diffusion(self, nsteps: int) -> np.ndarray:
        """Rows of the last estimator block -> iter_cm[nsteps, 2]: per time
        step t the sums over the yielded walkers of Y and Y^2, Y being N
        times the unwrapped centre-of-mass displacement of a walker since the
        first yielded state of the block (row 0 is zero)."""
        return self._read_rows(self._lib.qmc_dmc_read_cm_diffusion, nsteps,
                               (2,))

    def set_isf_estimator(self, num_modes, num_lags=1, lag_stride=1):
        """Enable the imaginary-time density correlations F(k, tau) of the
        estimator blocks (`intermediate_scattering`): num_modes momenta
        k_m = 2 pi m / L (the mode set of S(k)), num_lags lags tau_l =
        l lag_stride dt; num_modes = 0 disables them.  1 <= num_modes <= 64,
        1 <= num_lags <= 64, num_modes (num_lags + 2) <= 1024.  Independent of
        the other estimators."""
        check(self._lib.qmc_dmc_set_isf_estimator(
            self._h, int(num_modes), int(num_lags), int(lag_stride)))
        self.isf_shape = (int(num_modes), int(num_lags) + 2) \
            if int(num_modes) > 0 else None

    def read_isf(self, nsteps: int) -> np.ndarray:
        """Rows of the last estimator block -> iter_isf[nsteps, K, T + 2]: per
        time step t and mode m the sums over the yielded walkers of
        rho_m(t) rho_m(0)^* (real part) in column l once step l lag_stride has
        run (zero before), and of Re, Im rho_m(0) in columns T, T + 1; the
        rows travel through the cloning table, so the earlier end is weighted
        by its descendants (pure in the limit of a long block; read the last
        step)."""
        if self.isf_shape is None:
            raise QmcError('read_isf: the F(k, tau) estimator is not set')
        return self._read_rows(self._lib.qmc_dmc_read_isf, nsteps,
                               self.isf_shape)

    def set_obdm_estimator(self, shifts, eval_stride=1):
        """Enable the mixed one-body density matrix g1(s) of the estimator
        blocks at the given shifts (1..256 finite values; None or an empty
        sequence disables it), evaluated at every `eval_stride`-th step of a
        block, the first included.  The ensemble keeps its own shift table:
        `ModelEngine.one_body_density` calls in between do not disturb it.
        Independent of the other estimators."""
        sh = None if shifts is None else \
            np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1)
        if sh is None or sh.size == 0:
            check(self._lib.qmc_dmc_set_obdm_estimator(self._h, 0, None, 1))
            self.obdm_shifts = None
            return
        self.obdm_shifts = None     # (a failed call leaves it off)
        check(self._lib.qmc_dmc_set_obdm_estimator(
            self._h, sh.size, ptr(sh), int(eval_stride)))
        self.obdm_shifts = sh.copy()

    def read_obdm(self, nsteps: int) -> np.ndarray:
        """Rows of the last estimator block -> iter_obdm[nsteps, K]: per
        evaluated time step the g1(shift_k) of the yielded walkers, summed
        unweighted (divide by num_walkers for the mixed g1; a zero shift gives
        num_walkers exactly); the rows of the steps in between are zero."""
        if self.obdm_shifts is None:
            raise QmcError('read_obdm: the one-body density estimator is not '
                           'set')
        return self._read_rows(self._lib.qmc_dmc_read_obdm, nsteps,
                               (self.obdm_shifts.size,))

    def set_site_estimator(self, num_occ, num_dist=0, pure=False, pfw=1):
        """Enable the site occupation statistics of the estimator blocks
        (`site_statistics`): per time step the `num_occ` counts occ[n] of the
        sites that hold n particles (the last collects n >= num_occ - 1) and
        the `num_dist` sums corr[d] = sum_c n_c n_{c+d} over the sites of the
        supercell, mixed or pure with forward-walking length `pfw`.  The
        supercell size must be an integer <= 512, num_occ >= 1,
        0 <= num_dist <= supercell size, num_occ + num_dist <= 256;
        num_occ = 0 disables it.  Independent of the other estimators."""
        P, D = int(num_occ), int(num_dist)
        check(self._lib.qmc_dmc_set_site_estimator(
            self._h, P, D, int(bool(pure)), int(pfw)))
        self.site_shape = (P, D) if P > 0 else None

    def read_site(self, nsteps: int) -> np.ndarray:
        """Rows of the last estimator block -> iter_site[nsteps, P + D]: per
        time step [occ | corr] summed over the walkers (pure: the
        forward-walking rows over min(step + 1, pfw))."""
        if self.site_shape is None:
            raise QmcError('read_site: the site occupation estimator is not '
                           'set')
        return self._read_rows(self._lib.qmc_dmc_read_site, nsteps,
                               (sum(self.site_shape),))

    def read_series(self, nsteps: int) -> DmcSeries:
        ser, ptrs = self._series(nsteps)
        check(self._lib.qmc_dmc_read_series(self._h, int(nsteps), *ptrs))
        return ser

    def get_state(self) -> DmcState:
        W, n = self.max_num_walkers, self.num_particles
        confs = np.zeros((W, 2, n))
        energy, weight = np.zeros(W), np.zeros(W)
        mask = np.zeros(W, dtype=np.uint8)
        ref = np.zeros(W, dtype=np.int64)
        sc = np.zeros(5)
        check(self._lib.qmc_dmc_get_state(self._h, ptr(confs), ptr(energy),
                                          ptr(weight), ptr(mask, _u8p),
                                          ptr(ref, _i64p), ptr(sc)))
        return DmcState(confs, energy, weight, mask.astype(bool), ref,
                        float(sc[0]), float(sc[1]), float(sc[2]),
                        float(sc[3]), int(sc[4]))

    def get_scalars(self):
        """-> (state_energy, state_weight, ref_energy, accum_energy,
        num_walkers) without downloading the population."""
        sc = np.zeros(5)
        check(self._lib.qmc_dmc_get_state(self._h, None, None, None, None,
                                          None, ptr(sc)))
        return (float(sc[0]), float(sc[1]), float(sc[2]), float(sc[3]),
                int(sc[4]))

    # -- multi-GPU building blocks ------------------------------------------
    def step_local(self, partial_ptr: int):
        check(self._lib.qmc_dmc_step_local(self._h, partial_ptr))

    def step_finish(self, total_ptr: int):
        check(self._lib.qmc_dmc_step_finish(self._h, total_ptr))

    def num_walkers(self) -> int:
        n = C.c_int64(0)
        check(self._lib.qmc_dmc_num_walkers(self._h, C.byref(n)))
        return int(n.value)

    def walker_record_size(self) -> int:
        """Doubles per walker record of export / import (3N + 2 + the
        forward-walking rows of S(k) and the density when they are set, and
        with `set_record_rows` those of every other estimator that keeps
        per-walker rows)."""
        n = C.c_int64(0)
        check(self._lib.qmc_dmc_walker_record_size(self._h, C.byref(n)))
        return int(n.value)

    def export_walkers(self, first: int, count: int, buf_ptr: int):
        check(self._lib.qmc_dmc_export_walkers(self._h, int(first), int(count),
                                               buf_ptr))

    def import_walkers(self, count: int, buf_ptr: int):
        """Append at the device's population count (synchronises)."""
        check(self._lib.qmc_dmc_import_walkers(self._h, int(count), buf_ptr))

    def import_walkers_at(self, first: int, count: int, buf_ptr: int):
        """Stream-ordered: records -> slots [first, first + count); the
        population size becomes first + count."""
        check(self._lib.qmc_dmc_import_walkers_at(self._h, int(first),
                                                  int(count), buf_ptr))

    def set_num_walkers(self, nw: int):
        """Stream-ordered truncation (the caller knows the population size)."""
        check(self._lib.qmc_dmc_set_num_walkers(self._h, int(nw)))

    def truncate(self, new_nw: int):
        check(self._lib.qmc_dmc_truncate(self._h, int(new_nw)))

    # -- estimators of a split-step (multi-GPU) run -------------------------
    def est_begin_block(self, nsteps: int):
        check(self._lib.qmc_dmc_est_begin_block(self._h, int(nsteps)))

    def step_estimators(self, step_idx: int):
        check(self._lib.qmc_dmc_step_estimators(self._h, int(step_idx)))

    def est_iter_dev(self):
        """Device addresses (ints or None) of this rank's iter_ssf /
        iter_density rows of the open estimator block."""
        a, b = C.c_void_p(), C.c_void_p()
        check(self._lib.qmc_dmc_est_iter_dev(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def est_rows_dev(self, slot: int):
        """-> (device address or None, doubles per time step) of this rank's
        per-step rows of estimator slot `slot` (`dmc_est.Estimator.slot`; the
        QMC_EST_* of the header) in the open estimator block; (None, 0) for a
        slot that is off."""
        rows, width = C.c_void_p(), C.c_int64(0)
        check(self._lib.qmc_dmc_est_rows_dev(self._h, int(slot),
                                             C.byref(rows), C.byref(width)))
        return rows.value, int(width.value)

    def set_record_rows(self, on: bool = True):
        """The walker records of export / import carry the per-walker rows of
        every estimator that keeps some (pure g2, centre-of-mass diffusion,
        F(k, tau), pure site statistics), not those of S(k) and the density
        alone.  Before or after the estimator setters; default off."""
        check(self._lib.qmc_dmc_set_record_rows(self._h, int(bool(on))))
        self._record_rows = bool(on)

    @property
    def record_rows(self) -> bool:
        return self._record_rows
