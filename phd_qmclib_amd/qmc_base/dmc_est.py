"""The DMC block estimators, one record each: the procedure, the sampling, the
block loop, the result file and the distributed driver loop over `ESTIMATORS`.
Classes are given by name, so that every layer can import this module."""
import typing as t

import numpy as np

__all__ = ['ESTIMATORS', 'Estimator']


def _kwargs(cfg):
    return None if cfg is None else dict(cfg)


def _kwargs_no_pfw(cfg):
    """The forward walking spans a block: a configured length is dropped
    (dmc_exec/proc.py:262-266; the density spec has no such key)."""
    return None if cfg is None else {k: v for k, v in dict(cfg).items()
                                     if k != 'pfw_num_time_steps'}


def _kwargs_flag(cfg):
    """No parameters: an empty mapping, or just `true`."""
    if cfg is None or cfg is False:
        return None
    return {} if cfg is True else dict(cfg)


def _fw_reduce(rows, props, nts, keep, spec):
    """A mixed estimator sums over the block, a pure one takes the last time
    step; with keep_iter_data the container reduces the kept rows itself."""
    if keep:
        return ()
    return (rows[nts - 1] if spec.as_pure_est else rows.sum(axis=0),)


def _fw_wrap(cls, totals, series, props, nts, keep, spec, pure_fac):
    return cls.from_data(nts, series if keep else totals[0], props, keep,
                         spec.as_pure_est, pure_fac)


def _density_wrap(cls, totals, series, *rest):
    # (the rows have a trailing axis of one, the container has none)
    return _fw_wrap(cls, [totals[0][..., 0]],
                    None if series is None else series[..., 0], *rest)


def _site_wrap(cls, totals, series, props, nts, keep, spec, pure_fac):
    # (the container splits a row at the number of occupation bins)
    return cls.from_data(nts, series if keep else totals[0], props, keep,
                         spec.as_pure_est, pure_fac, spec.num_occupations)


def _cm_reduce(rows, props, nts, keep, spec):
    """The curve <Y^2>(t) of the block."""
    return rows[:, 1] / props.num_walkers,


def _isf_reduce(rows, props, nts, keep, spec):
    """The last step's row of the block over its walkers."""
    return rows[nts - 1] / props.num_walkers[nts - 1],


def _obdm_reduce(rows, props, nts, keep, spec):
    """The rows of the evaluated steps summed, weighed by the walkers of
    those steps (the walkers enter the rows unweighted, so a zero shift gives
    exactly 1)."""
    evaluated = np.arange(nts) % spec.eval_stride == 0
    return rows[evaluated].sum(axis=0), props.num_walkers[evaluated].sum()


#: the closing sentence of every refusal
_OPT_IN = ('.  Or pass block_estimators=True to DistributedDmc: the walker '
           'record then carries the per-walker rows of every estimator, and '
           'read_estimator returns the rows summed over the ranks')


class Estimator(t.NamedTuple):
    """One DMC block estimator; `spec` is its `Proc` level spec."""
    #: group under blocks/ of the result file, and field of `PropsDataBlocks`
    key: str
    #: fields of `Proc` (and group under proc_spec/), `Sampling`,
    #: `SamplingBlock`, `PropsDataSeries` (None: the rows are not kept)
    proc_field: str
    sampling_field: str
    block_field: str
    series_field: t.Optional[str]
    #: spec class in `mrbp_qmc.dmc_exec` and in `mrbp_qmc.dmc`; container
    #: class in `qmc_exec.data.dmc`
    spec_class: str
    blocks_class: str
    #: (spec, forward-walking length, model spec) -> arguments of the
    #: `Sampling` level spec; spec -> shape of one time step's row
    sampling_args: t.Callable
    row_shape: t.Callable
    #: configuration mapping -> keywords of the `Proc` level spec, or None
    config_kwargs: t.Callable = _kwargs
    #: (ensemble, `Sampling` level spec): switch it on; (ensemble, nts) ->
    #: rows of the last block.  None: S(k) and the density are set by
    #: `set_estimators` and come back from `run_block_est`
    enable: t.Optional[t.Callable] = None
    read: t.Optional[t.Callable] = None
    #: (row shape, nts) -> shapes of the totals of a block; (rows, props, nts,
    #: keep, spec) -> these totals; (container class, totals, kept rows or
    #: None, props, nts, keep, spec, pure_fac) -> the container
    totals_shapes: t.Callable = lambda row, nts: (row,)
    reduce: t.Callable = _fw_reduce
    wrap: t.Callable = lambda cls, totals, *rest: cls(*totals)
    #: `DmcEnsemble` attribute that tells it is on (a count, a flag, a shape
    #: or an array; off is 0, False or None, or no attribute at all), and why
    #: `DistributedDmc` refuses it then unless it was created with
    #: `block_estimators=True` (None: it works across ranks either way)
    ensemble_attr: t.Optional[str] = None
    refusal: t.Optional[str] = None
    #: its slot in the ensemble (the QMC_EST_* of include/qmcwalk.h):
    #: `DmcEnsemble.est_rows_dev(slot)` gives a rank's rows on the device, and
    #: the per-walker rows of the slots follow one another in this order in a
    #: walker record
    slot: t.Optional[int] = None
    #: ensemble -> shape of one time step's row as the ensemble was set
    #: (`row_shape` of the spec that switched it on)
    ensemble_row_shape: t.Optional[t.Callable] = None


#: in the order in which the groups of the result file are created
ESTIMATORS = (
    Estimator(
        'density', 'density_spec', 'density_est_spec', 'iter_density', None,
        'DensityEstSpec', 'DensityBlocks',
        sampling_args=lambda spec, pfw, model_spec: (
            spec.num_bins, spec.as_pure_est, pfw),
        row_shape=lambda spec: (spec.num_bins, 1), wrap=_density_wrap, slot=1),
    Estimator(
        'ss_factor', 'ssf_spec', 'ssf_est_spec', 'iter_ssf', 'ssf_blocks',
        'SSFEstSpec', 'SSFBlocks', config_kwargs=_kwargs_no_pfw,
        sampling_args=lambda spec, pfw, model_spec: (
            spec.num_modes, spec.as_pure_est, pfw),
        row_shape=lambda spec: (spec.num_modes, 3), wrap=_fw_wrap, slot=0),
    Estimator(
        'pair_dist', 'pair_dist_spec', 'pair_dist_est_spec', 'iter_pair_dist',
        'pair_dist_blocks', 'PairDistEstSpec', 'PairDistBlocks',
        config_kwargs=_kwargs_no_pfw,
        sampling_args=lambda spec, pfw, model_spec: (
            spec.num_bins, spec.as_pure_est, pfw),
        row_shape=lambda spec: (spec.num_bins,), wrap=_fw_wrap,
        enable=lambda ens, s: ens.set_pair_dist_estimator(
            s.num_bins, s.as_pure_est, s.pfw_num_time_steps),
        read=lambda ens, nts: ens.read_pair_dist(nts),
        ensemble_attr='pair_dist_bins', slot=2,
        ensemble_row_shape=lambda ens: (ens.pair_dist_bins,),
        refusal='the pair distribution estimator is single-GPU only: its '
        'forward-walking rows are not part of the walker record that '
        'the population rebalance moves between ranks; switch it off '
        '(set_pair_dist_estimator(0)) for a distributed run' + _OPT_IN),
    Estimator(
        'cm_diffusion', 'superfluid_spec', 'superfluid_est_spec',
        'iter_cm_diffusion', 'cm_diffusion_blocks', 'SuperfluidEstSpec',
        'CMDiffusionBlocks', config_kwargs=_kwargs_flag,
        sampling_args=lambda spec, pfw, model_spec: (),
        row_shape=lambda spec: (2,),
        enable=lambda ens, s: ens.set_cm_diffusion_estimator(True),
        read=lambda ens, nts: ens.read_cm_diffusion(nts),
        totals_shapes=lambda row, nts: ((nts,),), reduce=_cm_reduce,
        ensemble_attr='cm_diffusion', slot=3,
        ensemble_row_shape=lambda ens: (2,),
        refusal='the centre-of-mass diffusion estimator is single-GPU only: '
        'its per-walker rows are not part of the walker record that '
        'the population rebalance moves between ranks; switch it off '
        '(set_cm_diffusion_estimator(False)) for a distributed run'
        + _OPT_IN),
    Estimator(
        'isf', 'isf_spec', 'isf_est_spec', 'iter_isf', 'isf_blocks',
        'ISFEstSpec', 'ISFBlocks',
        sampling_args=lambda spec, pfw, model_spec: (
            spec.num_modes, spec.num_lags, spec.lag_stride),
        row_shape=lambda spec: (spec.num_modes, spec.num_lags + 2),
        enable=lambda ens, s: ens.set_isf_estimator(
            s.num_modes, s.num_lags, s.lag_stride),
        read=lambda ens, nts: ens.read_isf(nts),
        reduce=_isf_reduce, ensemble_attr='isf_shape', slot=4,
        ensemble_row_shape=lambda ens: tuple(ens.isf_shape),
        refusal='the F(k, tau) estimator is single-GPU only: '
        'its per-walker rows are not part of the walker record that '
        'the population rebalance moves between ranks; switch it off '
        '(set_isf_estimator(0)) for a distributed run' + _OPT_IN),
    Estimator(
        'obdm', 'obdm_spec', 'obdm_est_spec', 'iter_obdm', 'obdm_blocks',
        'OBDMEstSpec', 'OBDMBlocks',
        sampling_args=lambda spec, pfw, model_spec: (
            spec.shifts(model_spec.supercell_size), spec.eval_stride),
        row_shape=lambda spec: (spec.num_shifts,),
        enable=lambda ens, s: ens.set_obdm_estimator(s.shifts, s.eval_stride),
        read=lambda ens, nts: ens.read_obdm(nts),
        totals_shapes=lambda row, nts: (row, (1,)), reduce=_obdm_reduce,
        ensemble_attr='obdm_shifts', slot=5,
        ensemble_row_shape=lambda ens: (len(ens.obdm_shifts),),
        refusal='the one-body density estimator is single-GPU only: its rows '
        'are not yet summed across ranks; switch it off '
        '(set_obdm_estimator(None)) for a distributed run' + _OPT_IN),
    Estimator(
        'site', 'site_spec', 'site_est_spec', 'iter_site', None,
        'SiteEstSpec', 'SiteBlocks', config_kwargs=_kwargs_no_pfw,
        sampling_args=lambda spec, pfw, model_spec: (
            spec.num_occupations, spec.num_distances, spec.as_pure_est, pfw),
        row_shape=lambda spec: (spec.num_occupations + spec.num_distances,),
        wrap=_site_wrap,
        enable=lambda ens, s: ens.set_site_estimator(
            s.num_occupations, s.num_distances, s.as_pure_est,
            s.pfw_num_time_steps),
        read=lambda ens, nts: ens.read_site(nts),
        ensemble_attr='site_shape', slot=6,
        ensemble_row_shape=lambda ens: (sum(ens.site_shape),),
        refusal='the site occupation estimator is single-GPU only: its '
        'forward-walking rows are not part of the walker record that '
        'the population rebalance moves between ranks; switch it off '
        '(set_site_estimator(0)) for a distributed run' + _OPT_IN),
)


