/*
 * qmcwalk.h -- C-ABI of libqmcwalk.so, the MI355X (gfx950) walker-propagation
 * engine for the PhD-QMCLib `mrbp_qmc` VMC/DMC sampling hot path.
 *
 * The reference has no FFI: its boundary is the Python object protocol
 * `Sampling.core_funcs` / `Sampling.blocks()` (numba-compiled callables,
 * qmc_base/vmc.py:204-257, qmc_base/dmc.py:297-370).  Each entry point below
 * names the reference interface it stands in for (paths under
 * /root/reference/src/phd_qmclib/).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error;
 *     `qmc_last_error()` gives the message (thread-local).
 *   - "host" pointers are caller-owned CPU buffers; "dev" pointers are device
 *     (HBM) addresses.  All device memory of an ensemble is owned by its handle.
 *   - a handle is bound to one HIP device and one stream and is not
 *     thread-safe.  `stream` is a hipStream_t passed as void*.
 *     qmc_engine_create: NULL = the engine creates its own non-blocking
 *     stream; qmc_engine_create_on_stream: the caller's stream as it is, NULL
 *     being the legacy default stream (what torch.cuda.current_stream() is
 *     unless a side stream is current) -- use it whenever another library
 *     (torch.distributed / RCCL) must be stream-ordered with the engine.
 *   - configurations use the reference's row layout: positions pos[W][N],
 *     full system configurations confs[W][2][N] (row 0 position, row 1 drift;
 *     qmc_base/jastrow/model.py:31-38).
 */
#ifndef QMCWALK_H
#define QMCWALK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMCWALK_ABI_VERSION 1

typedef struct qmc_engine qmc_engine;
typedef struct qmc_vmc qmc_vmc;
typedef struct qmc_dmc qmc_dmc;

/* mrbp_qmc/model.py:40-75 -- Params, OBFParams, TBFParams flattened in
 * declaration order (what `Spec.cfc_spec` hands to every core function). */
typedef struct {
    double lattice_depth;
    double lattice_ratio;
    double interaction_strength;
    int64_t boson_number;
    double supercell_size;
    double tbf_contact_cutoff;
    double defect_magnitude;
    int64_t defects_sep;
    double well_width;
    double barrier_width;
    int64_t is_free;
    int64_t is_ideal;
    double param_e0;
    double param_k1;
    double param_kp1;
    double param_k2;
    double param_beta;
    double param_r_off;
    double param_am;
} qmc_model_params;

/* mrbp_qmc/vmc.py:29-38 (TPFParams) + Sampling fields :70-80; `gaussian`
 * is the proposal code: QMC_VMC_UNIFORM, the reference's all-particle move;
 * QMC_VMC_GAUSSIAN, the vmc_ndf proposal (mrbp_qmc/vmc_ndf.py:23-51,
 * move_spread = sigma = sqrt(time_step)); QMC_VMC_PARTICLE, an extension: one
 * yield is a sweep of N single-particle Metropolis moves in label order
 * (csrc/qmc_vmc_sweep.h: word 0 of a particle's move block displaces it, word
 * 1 is that move's accept draw; num_accepted counts particle moves; no tape).
 * Anything else: qmc_vmc_create fails. */
enum { QMC_VMC_UNIFORM = 0, QMC_VMC_GAUSSIAN = 1, QMC_VMC_PARTICLE = 2 };
typedef struct {
    int64_t num_chains;
    double move_spread;
    uint64_t rng_seed;
    uint32_t chain0;      /* Philox slot of chain 0 (rank offset)          */
    int32_t gaussian;     /* QMC_VMC_* */
} qmc_vmc_params;

/* mrbp_qmc/dmc.py:143-185 (Sampling fields + DDFParams) */
typedef struct {
    int64_t max_num_walkers;
    int64_t target_num_walkers;
    double time_step;
    double num_walkers_control_factor;
    uint64_t rng_seed;
    uint32_t slot0;            /* Philox slot of walker slot 0 (rank offset) */
    int32_t fix_stale_energy;  /* 0: reference behaviour         */
    int32_t external_reduce;   /* 1: E_t/W_t are reduced across ranks by the
                                  caller between step_local and step_finish  */
    int32_t propagator;        /* QMC_DMC_LINEAR: the reference's step, error
                                  O(dt); QMC_DMC_QUADRATIC: the symmetric
                                  drift / diffusion split, error O(dt^2) (an
                                  extension, csrc/qmc_evolve2.h: three pair
                                  sums per step, fix_stale_energy without
                                  effect, tapes of [slot][2][N] normals per
                                  step).  Anything else: qmc_dmc_create fails.
                                  (Was `reserved`, 0: same place and size.)
                                  The centre-of-mass estimator's condition
                                  |sum of displacements| < L / 2 per step holds
                                  for either (csrc/qmc_cmdiff.h).              */
} qmc_dmc_params;
enum { QMC_DMC_LINEAR = 0, QMC_DMC_QUADRATIC = 1 };

/* Estimator specs of a DMC sampling (mrbp_qmc/dmc.py:103-140, 187-225):
 * static structure factor over num_modes momenta k_m = 2 pi m / L and density
 * histogram over num_bins bins, each mixed or pure (forward walking over
 * pfw_num_time_steps).  0 modes / bins disables an estimator. */
typedef struct {
    int32_t num_modes;
    int32_t ssf_pure;
    int64_t ssf_pfw;
    int32_t num_bins;
    int32_t dens_pure;
    int64_t dens_pfw;
} qmc_dmc_est_params;

const char *qmc_last_error(void);
int qmc_abi_version(void);
/* Identity of the kernels this library was built from: the first 16 hex digits
 * of sha256 over csrc/ sources + compiler flags (csrc/Makefile).  Measurement
 * records (profiles/traffic.json) carry it, so that a figure measured on other
 * kernels is recognised as stale. */
const char *qmc_source_hash(void);
int qmc_device_count(int *count);

/* Diagnostic (no GPU needed): the piecewise-polynomial table of the one-body
 * factor (mrbp_qmc/model.py:404-464: f1'/f1 and log f1 inside the unit cell)
 * the kernels would use for this model: intervals over the well and over the
 * barrier (0, 0 = the closed forms are evaluated directly) and the worst
 * deviation from the closed forms found while building it. */
int qmc_model_one_body_table_info(const qmc_model_params *model,
                                  int32_t *rows_well, int32_t *rows_barrier,
                                  double *max_err);

/* Diagnostic (no GPU needed): the row table of the pair-function angles
 * (sin / cos of pi z / L and of k2 z, mrbp_qmc/model.py:466-531) the kernels
 * would use for this model: rows over [0, L) (0 = the angles are evaluated by
 * polynomial `sincos` directly) and the worst absolute deviation of the
 * kernels' row + angle-addition arithmetic from long-double sin / cos. */
int qmc_model_trig_table_info(const qmc_model_params *model, int32_t *rows,
                              double *max_err);

/* Diagnostic (no GPU needed): the kernels' natural logarithm (row table of
 * 1/c and log c + five terms of log1p; it takes the place of numpy's log in
 * log|psi| = sum log f, the Metropolis test log(u) < 2 (log|psi'| - log|psi|),
 * qmc_base/vmc.py:636, and the Box-Muller normals) restated on the host: rows
 * and the worst |error| / (1 + |log x|) against long double over 2*10^5
 * arguments of every size. */
int qmc_log_table_info(int32_t *rows, double *max_err);

/* ---- engine: model constants on one device --------------------------- */
int qmc_engine_create(const qmc_model_params *model, int device, void *stream,
                      qmc_engine **out);
int qmc_engine_create_on_stream(const qmc_model_params *model, int device,
                                void *stream, qmc_engine **out);
void qmc_engine_destroy(qmc_engine *eng);
/* the stream the engine launches on; *owned = 1 if the engine created it */
int qmc_engine_stream(qmc_engine *eng, void **stream, int *owned);
/* The reference's reduced-precision knob, `jit_fastmath`
 * (mrbp_qmc/dmc.py:159-160; qmc_base/jastrow/dmc.py `fastmath=`): with on != 0
 * the O(N^2) pair loop (products of the per-particle sin/cos tables, the
 * quotient per pair, the pair sums) runs in float; positions, the tables
 * themselves, the one-body factor, the energy assembly, the logarithms and
 * the Metropolis test stay in double.  Off by default; relative error of the
 * local energy ~1e-6 (tests/test_gpu_fastmath.py reports it).  *in_effect
 * tells whether the engine has the variant for its model (boson_number > 32,
 * cutoff not close to L/2); where it has not, the call changes nothing. */
int qmc_engine_set_fast_math(qmc_engine *eng, int on, int *in_effect);
int qmc_engine_sync(qmc_engine *eng);
/* HIP-event timing on the engine's stream (bench / roofline) */
int qmc_engine_timer_start(qmc_engine *eng);
int qmc_engine_timer_stop(qmc_engine *eng, float *elapsed_ms);
/* Kernel profile: while open, every launch of the dominant kernel of a step
 * (vmc_step_kernel / dmc_evolve_kernel) is bracketed by its own HIP event
 * pair on the engine's stream (at most max_launches of them); profile_end
 * synchronises and returns the number of launches, the sum, the shortest and
 * the longest of their durations.  bench.py derives roofline.achieved from
 * it. */
int qmc_engine_profile_begin(qmc_engine *eng, int64_t max_launches);
int qmc_engine_profile_end(qmc_engine *eng, int64_t *launches,
                           double *total_ms, double *min_ms, double *max_ms);

/* Diagnostic (no reference counterpart): a library built
 * with -DQMC_TIMING stamps the shader clock at the section marks of the walker
 * kernels; this returns, per section, the cycles of wavefront lifetime spent
 * in it and the number of visits since the last reset (nsec must be 32;
 * entries 16..31 are the sections inside the energy pass of the VMC step).
 * The shipped library carries no stamps and returns an error. */
int qmc_engine_section_profile(qmc_engine *eng, uint64_t *cycles,
                               uint64_t *visits, int32_t nsec, int32_t reset);
const char *qmc_section_name(int32_t section);
/* Diagnostic: a library built with -DQMC_CUTS ends every wavefront of the walker
 * kernels at the section mark selected here (-1: never); hardware counters of
 * runs cut at successive marks give per-section executed instructions.  The
 * shipped library returns an error. */
int qmc_engine_section_cut(qmc_engine *eng, int32_t section);
/* Diagnostic counters of the shipped kernels (test-visible evidence of which
 * code path ran; no reference counterpart).  out[0]: walkers of the
 * one-wavefront-per-walker shapes (33 <= N <= 128) that failed the per-walker
 * checks of the sorted-row pair sums (csrc/qmc_sorted64.h, qmc_sorted128.h) in
 * a VMC / DMC stepping kernel and were evaluated by the general pair sum
 * inside the same kernel, since the last reset.  n <= 4; synchronises. */
int qmc_engine_diag_counters(qmc_engine *eng, uint64_t *out, int32_t n,
                             int32_t reset);
/* Diagnostic: runs one device primitive of the shipped kernels
 * (csrc/qmc_math.h, csrc/qmc_device.h; the kernel is csrc/qmc_probe.h) on n
 * host inputs, with this engine's model constants and device tables, and
 * returns its outputs (test-visible evidence of what the kernels compute; no
 * reference counterpart).  in[n][in_width] -> out[n][out_width], widths per
 * function below.  Inputs run in order, 64 to a wavefront: wrap_box and the
 * trig-table load decide for a whole wavefront.  Integers (Philox words,
 * counters, keys) travel as exact doubles.  Inputs no production caller can
 * produce are refused: non-finite ones for every function, non-positive or
 * non-normal ones to log_pos, positions outside (-4 L, 4 L) to the functions
 * that read a model table; a model without the table asked for is an error.
 * Synchronises. */
enum {
    QMC_PROBE_FAST_DIV = 0,        /* (x, y) -> x / y */
    QMC_PROBE_PAIR_DIV = 1,        /* (x, y) -> x / y, pair-loop form */
    QMC_PROBE_PAIR_DIV_F32 = 2,    /* (x, y) -> float pair_div of (float) x, y */
    QMC_PROBE_FAST_RCP = 3,        /* y -> 1 / y */
    QMC_PROBE_FAST_SQRT = 4,       /* x -> sqrt x */
    QMC_PROBE_SINCOS_KERNEL = 5,   /* x -> (sin x, cos x), |x| <= pi/4 */
    QMC_PROBE_SINCOS_HALFPI = 6,   /* u -> (sin, cos)(pi u / 2) */
    QMC_PROBE_EXP_BOUNDED = 7,     /* x -> exp x */
    QMC_PROBE_LOG_POS = 8,         /* x -> log x */
    QMC_PROBE_WRAP_BOX = 9,        /* z -> z wrapped into [0, L) */
    QMC_PROBE_TRIG_TAB = 10,       /* z -> (s, c, su, cu, ok) */
    QMC_PROBE_ONE_BODY_TAB = 11,   /* z -> (f1'/f1, log f1, barrier) */
    QMC_PROBE_ONE_BODY = 12,       /* z -> (f1'/f1, kin_pot, f1, xoff) */
    QMC_PROBE_VMC_MOVE_UNIT = 13,  /* w -> (w + 1/2) 2^-32 - 1/2 */
    QMC_PROBE_NORMAL2_WORDS = 14,  /* (w0, w1) -> (g0, g1) of dmc_normal2 */
    QMC_PROBE_NORMAL2_UNIFORMS = 15, /* (u0, u1) -> (g0, g1) of philox_normal2 */
    QMC_PROBE_PHILOX2X32 = 16,     /* (c0, c1, k) -> (c0', c1') */
    QMC_PROBE_PHILOX4X32 = 17,     /* (c0..c3, k0, k1) -> (c0'..c3') */
    QMC_PROBE_COUNT = 18
};
int qmc_engine_probe(qmc_engine *eng, int32_t fn, int64_t n, const double *in,
                     double *out);

/* Stands in for model.core_funcs.{wf_abs_log, energy, drift,
 * ith_energy_and_drift} (qmc_base/jastrow/model.py:298-366, 476-564, 756-773,
 * 793-854) over a batch of configurations.  Host buffers; any output may be
 * NULL.  pos[nconf][N] -> wf[nconf], energy[nconf], ith_energy[nconf][N],
 * drift[nconf][N]. */
int qmc_evaluate(qmc_engine *eng, int64_t nconf, const double *pos,
                 double *wf_abs_log, double *energy, double *ith_energy,
                 double *drift);
/* Same on device-resident buffers, asynchronous on the engine's stream. */
int qmc_evaluate_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                     double *wf_dev, double *energy_dev, double *ith_dev,
                     double *drift_dev);

/* One-body density matrix g1(s) (qmc_base/jastrow/model.py:859-965:
 * core_funcs.ith_one_body_density / one_body_density; the batch front end is
 * PhysicalFuncs.one_body_density, qmc_base/jastrow/model.py:1064-1087,
 * mrbp_qmc/model.py:801-815) over a batch of configurations and a set of
 * shifts: g1[nconf][nshift] and, when ith is not NULL, the per-particle terms
 * ith[nconf][nshift][N] in the particle order of pos.  Any real shift and any
 * position are accepted, as by the reference.  g1 is symmetric in the
 * particles, ith follows the order of the row.  Always fp64:
 * qmc_engine_set_fast_math does not apply (csrc/qmc_obdm.h).
 * qmc_obdm: host buffers, synchronous; nshift < 1, a NULL pos / shifts / g1
 * or a non-finite shift is an error. */
int qmc_obdm(qmc_engine *eng, int64_t nconf, const double *pos, int32_t nshift,
             const double *shifts, double *g1, double *ith);
/* Same on device-resident buffers, asynchronous on the engine's stream.  The
 * shifts are taken as given (a non-finite one gives non-finite output, no
 * error). */
int qmc_obdm_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                 int32_t nshift, const double *shifts_dev, double *g1_dev,
                 double *ith_dev);
/* Weighted sums over the configurations, device buffers, asynchronous:
 * sums_dev[nshift][2] = sum_c w_c g1_c(s), sum_c w_c g1_c(s)^2 and (unless
 * NULL) wsum_dev[0] = sum_c w_c; w_dev = NULL means unit weights.  Fixed
 * summation order: two calls give the same bits.  The per-configuration values
 * live in an engine-owned scratch filled in tiles of 2^16 configurations. */
int qmc_obdm_reduce_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                        const double *w_dev, int32_t nshift,
                        const double *shifts_dev, double *sums_dev,
                        double *wsum_dev);

/* Pair distribution function g2(r): per configuration the histogram of the
 * N (N - 1) / 2 minimum-image pair distances r_ij = |min_distance(z_i, z_j, L)|
 * (qmc_base/utils.py:35-51, reached through _real_distance,
 * mrbp_qmc/model.py:555-562) over num_bins uniform bins of [0, L/2]:
 * bin = min(floor(r / delta), num_bins - 1), delta = (L/2) / num_bins, the
 * `int(z // bin_size)` convention of mrbp_qmc/dmc.py:522-545; a pair at
 * exactly L/2 counts in the last bin.  counts[nconf][num_bins] holds unordered
 * pairs, so every row adds up to N (N - 1) / 2, and
 * g2(r_b) = counts[b] L / (N (N - 1) delta) at r_b = (b + 1/2) delta.
 * Positions outside [0, L) are brought into the box first; the particle order
 * is irrelevant.  Always fp64: qmc_engine_set_fast_math does not apply
 * (csrc/qmc_pairdist.h).
 * qmc_pair_dist: host buffers, synchronous; a NULL pos / counts or num_bins
 * outside [1, 4096] is an error. */
int qmc_pair_dist(qmc_engine *eng, int64_t nconf, const double *pos,
                  int32_t num_bins, uint32_t *counts);
/* Same on device-resident buffers, asynchronous on the engine's stream. */
int qmc_pair_dist_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                      int32_t num_bins, uint32_t *counts_dev);
/* Weighted sums over the configurations, device buffers, asynchronous:
 * sums_dev[num_bins][2] = sum_c w_c H_c[b], sum_c w_c H_c[b]^2 and (unless
 * NULL) wsum_dev[0] = sum_c w_c; w_dev = NULL means unit weights (the mixed
 * estimate sum W H / sum W of a DMC State, the twin of mrbp_qmc/dmc.py:345-356,
 * and the ensemble mean of qmc_vmc_pair_dist).  Fixed summation order: two
 * calls give the same bits; with unit weights both sums are exact integers.
 * The per-configuration histograms live in an engine-owned scratch filled in
 * tiles of at most 2^16 configurations. */
int qmc_pair_dist_reduce_dev(qmc_engine *eng, int64_t nconf,
                             const double *pos_dev, const double *w_dev,
                             int32_t num_bins, double *sums_dev,
                             double *wsum_dev);

/* Three-body distribution g3(d): per configuration the histogram of the spans
 * of the N (N - 1) (N - 2) / 6 particle triples on the ring of length L.  The
 * span of a triple is the shortest arc that holds its three (wrapped)
 * positions, L minus the largest of the three gaps between them, in
 * [0, 2 L / 3].  num_bins uniform bins of width delta = max_span / num_bins
 * cover [0, max_span), 0 < max_span <= L/2: a span d < max_span counts in
 * bin min(floor(d / delta), num_bins - 1), every other one in the overflow bin
 * num_bins.  counts[nconf][num_bins + 1]; every row adds up to
 * N (N - 1) (N - 2) / 6 (all zeros for N < 3), and
 * g3(d_b) = counts[b] / (C(N,3) 3 (delta/L)^2 (2 b + 1)) at
 * d_b = (b + 1/2) delta is 1 on average for uncorrelated uniform particles.
 * Positions outside [0, L) are brought into the box first; the particle order
 * is irrelevant.  Always fp64: qmc_engine_set_fast_math does not apply
 * (csrc/qmc_tripledist.h).
 * qmc_triple_dist: host buffers, synchronous; a NULL pos / counts, num_bins
 * outside [1, 4096] or max_span outside (0, L/2] is an error. */
int qmc_triple_dist(qmc_engine *eng, int64_t nconf, const double *pos,
                    int32_t num_bins, double max_span, uint32_t *counts);
/* Same on device-resident buffers, asynchronous on the engine's stream. */
int qmc_triple_dist_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                        int32_t num_bins, double max_span,
                        uint32_t *counts_dev);
/* Weighted sums over the configurations, device buffers, asynchronous:
 * sums_dev[num_bins + 1][2] = sum_c w_c T_c[b], sum_c w_c T_c[b]^2 and (unless
 * NULL) wsum_dev[0] = sum_c w_c; w_dev = NULL means unit weights.  Fixed
 * summation order, as qmc_pair_dist_reduce_dev; the per-configuration rows
 * live in an engine-owned scratch filled in tiles of at most 2^16
 * configurations. */
int qmc_triple_dist_reduce_dev(qmc_engine *eng, int64_t nconf,
                               const double *pos_dev, const double *w_dev,
                               int32_t num_bins, double max_span,
                               double *sums_dev, double *wsum_dev);

/* Energy components and Tan's contact.  The local energy of
 * qmc_base/jastrow/model.py:681-743 leaves the contact term g sum_{i<j}
 * delta(z_ij) of the Hamiltonian out: the cusp of the two-body factor accounts
 * for it.  Per configuration a row of 4 + nrange doubles:
 *   [0] E  the local energy, as qmc_evaluate returns it
 *   [1] T  = sum_i F_i^2, F the drift as qmc_evaluate returns it; its mean
 *          over |psi|^2 is the kinetic energy
 *   [2] V  = sum_i V(z_i), the lattice potential of mrbp_qmc/model.py:533-551
 *          exactly as the local energy contains it: a barrier where
 *          z_a < z - floor(z) on the position as given, of height
 *          defect_magnitude where floor(z) % defects_sep == 0 and
 *          lattice_depth elsewhere; 0 for is_free
 *   [3] I  = (E - T) - V; its mean is the interaction energy
 *          g <sum_{i<j} delta(z_ij)>, g = 4 k2 tan(k2 r_off)
 *   [4 + k] C_k = 1 / (2 r_k) sum_{i<j, d_ij < r_k}
 *          [cos(k2 r_off) / cos(k2 (d_ij - r_off))]^2, the windowed contact at
 *          range r_k = ranges[k]: d_ij the minimum-image distance, the compare
 *          strict, the weight f2(0)^2 / f2(d)^2 (1 on an ideal model).  g C_k
 *          estimates the interaction energy with a bias of order r_k^2.
 * 0 <= nrange <= 16; every range finite, in (0, L/2] and, unless the model is
 * ideal, at most |tbf_contact_cutoff| (the cosine form holds only there).
 * `ranges` is a HOST array in all four calls.  Any real position is accepted,
 * as by qmc_evaluate; pairs use the image inside the box.  N = 1: C_k = 0.
 * Always fp64: qmc_engine_set_fast_math does not apply
 * (csrc/qmc_energy_parts.h).
 * qmc_energy_parts: host buffers, synchronous, parts[nconf][4 + nrange]; a
 * NULL pos / parts (or ranges with nrange > 0) or a range outside the limits
 * is an error. */
int qmc_energy_parts(qmc_engine *eng, int64_t nconf, const double *pos,
                     int32_t nrange, const double *ranges, double *parts);
/* Same on device-resident pos / parts, asynchronous on the engine's stream. */
int qmc_energy_parts_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                         int32_t nrange, const double *ranges,
                         double *parts_dev);
/* Weighted sums over the configurations, device buffers, asynchronous:
 * sums_dev[4 + nrange][2] = sum_c w_c x_c, sum_c w_c x_c^2 of every column x
 * and (unless NULL) wsum_dev[0] = sum_c w_c; w_dev = NULL means unit weights.
 * Fixed summation order, as qmc_pair_dist_reduce_dev; the per-configuration
 * rows live in an engine-owned scratch filled in tiles of at most 2^16
 * configurations. */
int qmc_energy_parts_reduce_dev(qmc_engine *eng, int64_t nconf,
                                const double *pos_dev, const double *w_dev,
                                int32_t nrange, const double *ranges,
                                double *sums_dev, double *wsum_dev);

/* Renyi-2 entanglement entropy of a segment by replica swap (no counterpart
 * in the reference).  The configurations 2p and 2p + 1 of pos[nconf][N]
 * (nconf even) are the replicas R1, R2 of pair p; nlen segments
 * A_k = [origin, origin + lengths[k]) of the ring of length L, each length in
 * (0, L), B_k the complement.  Particle z is in A_k when t < lengths[k],
 * t = zw - a0w (+ L where negative), zw and a0w the images of z and origin in
 * [0, L).  n_a[nconf][nlen] is the number of particles of every configuration
 * in A_k (exact).  Where the two replicas of a pair hold the same number
 * (a matched pair) the particles inside A_k can be exchanged,
 * R1' = A(R2) u B(R1), R2' = A(R1) u B(R2), and
 *   log_ratio[nconf / 2][nlen] =
 *       ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|,
 * formed from the pair factors across the cut alone (the one-body factors and
 * the pairs inside A and inside B cancel identically: exactly 0 without
 * interactions); -inf where the pair is not matched.  With swap =
 * exp(log_ratio) (0 where unmatched) over P independent pairs drawn from
 * |psi|^2, S2(l_k) = -ln(sum_p swap[p][k] / P) is the Renyi-2 entropy of the
 * segment in the state psi: for VMC chains the variational S2 of the trial
 * wave function.  Always fp64: qmc_engine_set_fast_math does not apply
 * (csrc/qmc_renyi.h).
 * qmc_renyi_swap: host buffers, synchronous; either output may be NULL, not
 * both.  An odd or non-positive nconf, nlen outside [1, 4096], a length
 * outside (0, L) or not finite, an origin that is not finite, a NULL pos /
 * lengths is an error. */
int qmc_renyi_swap(qmc_engine *eng, int64_t nconf, const double *pos,
                   int32_t nlen, const double *lengths, double origin,
                   int32_t *n_a, double *log_ratio);
/* Same on device-resident buffers, asynchronous on the engine's stream (the
 * values of lengths_dev are not checked: the host does not see them). */
int qmc_renyi_swap_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                       int32_t nlen, const double *lengths_dev, double origin,
                       int32_t *n_a_dev, double *log_ratio_dev);
/* Sums over the nconf / 2 pairs, device buffers, asynchronous:
 * sums_dev[nlen][3] = sum_p swap, sum_p swap^2, number of matched pairs (the
 * argument of exp clamped to +-700).  Fixed summation order: two calls give
 * the same bits; the per-pair rows live in an engine-owned scratch filled in
 * tiles of at most 2^16 pairs. */
int qmc_renyi_swap_reduce_dev(qmc_engine *eng, int64_t nconf,
                              const double *pos_dev, int32_t nlen,
                              const double *lengths_dev, double origin,
                              double *sums_dev);

/* Renyi-2 replica swap of regions made of up to two disjoint segments, with
 * the particle number of the region resolved in the reduction (no counterpart
 * in the reference).  Replicas, origin and t as for qmc_renyi_swap.  Entry k
 * of regions[nreg][3] is a region X_k = (l1, g, l2): particle z is in X_k when
 *   t < l1  or  (m1 <= t && t < m2),   m1 = l1 + g,  m2 = m1 + l2,
 * the marks formed in fp64 in exactly this order; Y_k is the complement.
 * Limits: l1 > 0, g >= 0, l2 >= 0, m2 < L, all finite; l2 = 0 is a single
 * segment (its g is not used but must obey the limits); 1 <= nreg <= 4096.
 * n_x[nconf][nreg] is the number of particles of every configuration in X_k
 * (exact).  A pair is matched at k when its two replicas hold the same TOTAL
 * number in X_k; then, with R1' = X(R2) u Y(R1), R2' = X(R1) u Y(R2),
 *   log_ratio[nconf / 2][nreg] =
 *       ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|,
 * formed from the pair factors across the cut alone,
 * S(X2,Y1) + S(X1,Y2) - S(X1,Y1) - S(X2,Y2): exactly 0 without interactions
 * and where either side is empty in both replicas; -inf where the pair is
 * not matched.  With S2(X) = -ln <swap>, the Renyi-2 mutual information of two
 * segments A, C is I2 = S2(A) + S2(C) - S2(A u C).  Always fp64:
 * qmc_engine_set_fast_math does not apply (csrc/qmc_renyi_region.h).
 * qmc_renyi_region_swap: host buffers, synchronous; either output may be
 * NULL, not both.  An odd or non-positive nconf, nreg outside [1, 4096], a
 * region outside the limits or not finite, an origin that is not finite, a
 * NULL pos / regions is an error. */
int qmc_renyi_region_swap(qmc_engine *eng, int64_t nconf, const double *pos,
                          int32_t nreg, const double *regions, double origin,
                          int32_t *n_x, double *log_ratio);
/* Same on device-resident buffers, asynchronous on the engine's stream (the
 * values of regions_dev are not checked: the host does not see them). */
int qmc_renyi_region_swap_dev(qmc_engine *eng, int64_t nconf,
                              const double *pos_dev, int32_t nreg,
                              const double *regions_dev, double origin,
                              int32_t *n_x_dev, double *log_ratio_dev);
/* Sums over the P = nconf / 2 pairs, device buffers, asynchronous:
 * sums_dev[nreg][3 + 2 Q], Q = num_charges in [0, N + 1].  Columns 0, 1, 2 =
 * sum_p swap, sum_p swap^2, number of matched pairs (the argument of exp
 * clamped to +-700), as qmc_renyi_swap_reduce_dev.  Column 3 + 2n =
 * sum_p swap [n_X(R1) = n] and column 4 + 2n = sum_p ([n_X(R1) = n] +
 * [n_X(R2) = n]), n = 0 ... Q - 1, the latter over every configuration,
 * matched or not (an exact integer in a double): p(n) = column(4 + 2n) / 2P
 * is the counting statistics of X, <swap delta_n> = column(3 + 2n) / P =
 * p(n)^2 Tr rho_n^2, and S2(n) = -ln(<swap delta_n> / p(n)^2) the
 * charge-resolved entropy.  Charges >= Q are not collected.
 * nreg (3 + 2 Q) > 2^20 is an error.  Fixed summation order, no
 * floating-point atomics: two calls give the same bits; the per-pair rows
 * live in an engine-owned scratch filled in tiles of at most 2^16 pairs. */
int qmc_renyi_region_swap_reduce_dev(qmc_engine *eng, int64_t nconf,
                                     const double *pos_dev, int32_t nreg,
                                     const double *regions_dev, double origin,
                                     int32_t num_charges, double *sums_dev);

/* Purity of the one-body density matrix by a one-particle replica swap (no
 * counterpart in the reference).  The configurations 2p and 2p + 1 of
 * pos[nconf][N] (nconf even, N <= 512) are the replicas R1 = x1, R2 = x2 of
 * pair p, in any particle order.  For the exchange x1_i <-> x2_j,
 *   log_ratio[nconf / 2][N][N] =
 *       ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|,
 * R1' being R1 with its particle i replaced by particle j of R2 and R2' the
 * converse, formed from the pair factors alone (the one-body factors cancel
 * identically: exactly 0 without interactions), and
 *   mean[nconf / 2] = N^-2 sum_ij exp(log_ratio[p][i][j])
 * (the argument of exp clamped to +-700), a symmetric function of each row:
 * the order of the particles in a row does not matter.  Over P independent
 * pairs drawn from |psi|^2, sum_p mean[p] / P = Tr rho1^2 = sum_k lambda_k^2,
 * the purity of the one-body density matrix normalised to trace 1, and
 * S2 = -ln Tr rho1^2 the particle-partition Renyi-2 entropy at n = 1; the
 * condensate fraction obeys Tr rho1^2 <= lambda_max <= sqrt(Tr rho1^2).  For
 * VMC chains this is the variational purity of the trial wave function.
 * Positions enter through their images in [0, L).  Two particles of the same
 * row at the same place (psi = 0) are undefined.  Always fp64:
 * qmc_engine_set_fast_math does not apply (csrc/qmc_partent.h).
 * qmc_particle_swap: host buffers, synchronous; either output may be NULL, not
 * both.  An odd or non-positive nconf or a NULL pos is an error (N is at
 * most 512 for every engine). */
int qmc_particle_swap(qmc_engine *eng, int64_t nconf, const double *pos,
                      double *mean, double *log_ratio);
/* Same on device-resident buffers, asynchronous on the engine's stream. */
int qmc_particle_swap_dev(qmc_engine *eng, int64_t nconf,
                          const double *pos_dev, double *mean_dev,
                          double *log_ratio_dev);
/* Sums over the P = nconf / 2 pairs, device buffers, asynchronous:
 * sums_dev[3] = sum_p mean[p], sum_p mean[p]^2, P.  Fixed summation order: two
 * calls give the same bits; the per-pair means live in an engine-owned scratch
 * filled in tiles of at most 2^16 pairs. */
int qmc_particle_swap_reduce_dev(qmc_engine *eng, int64_t nconf,
                                 const double *pos_dev, double *sums_dev);

/* One-body density matrix rho1(x, x') on a grid (no counterpart in the
 * reference): what g1(s) integrates away in a lattice.  num_points = M uniform
 * cells of [0, L), delta = L / M, centres x_c = (c + 1/2) L / M (rounded in
 * that order: the product, then the quotient).  For one
 * configuration, z_i the image of particle i in [0, L) and
 * a(i) = min(floor(z_i / delta), M - 1) its row bin (a particle on the edge
 * a delta counts in bin a),
 *   R_conf[a][c] = sum_{i : a(i) = a} psi(z_1 .. z_i -> x_c .. z_N) / psi(R),
 * the ratio being that of qmc_obdm at the shift x_c - z_i (the argument of exp
 * clamped to +-700): the row follows the particle's actual position, the
 * column is the cell centre, so that the average over |psi|^2 is
 * int_{bin a} rho1(x, x_c) dx ~ delta rho1(x_a, x_c).  The symmetrised mean
 * has the occupations of the natural orbitals as eigenvalues (sum ~ N; the
 * largest over N is the condensate fraction).  The call reduces over the
 * configurations itself, into num_groups = G independent sums
 *   sums[G][M][M]: sums[g][a][c] = sum_{conf = g (mod G)} w_conf R_conf[a][c]
 *   wsum[G]:       wsum[g]       = sum_{conf = g (mod G)} w_conf
 * (w NULL: unit weights; wsum may be NULL).  Summation order: a group is cut
 * into S interleaved partial sums (member q of the group goes to q mod S; S a
 * function of nconf, M, G and N alone), each adds its configurations in rising
 * index and the particles of a configuration in the order of the row, and the
 * partial sums are added in rising order; wsum by 256 strided partial sums and
 * a fixed tree.  No floating-point atomics: two calls give the same bits.
 * The particles of a row may come in any order.  Always fp64:
 * qmc_engine_set_fast_math does not apply (csrc/qmc_obdm_grid.h).
 * Limits: N <= 512, M in [1, 512], G in [1, 1024] and G <= nconf, nconf > 0;
 * anything else, or a NULL pos or sums, is an error and leaves the outputs
 * untouched.
 * qmc_obdm_grid: host buffers, synchronous. */
int qmc_obdm_grid(qmc_engine *eng, int64_t nconf, const double *pos,
                  const double *w, int32_t num_points, int32_t num_groups,
                  double *sums, double *wsum);
/* Same on device-resident buffers, asynchronous on the engine's stream; the
 * partial sums live in an engine-owned scratch of at most 128 MB (S = 1:
 * in sums_dev itself). */
int qmc_obdm_grid_dev(qmc_engine *eng, int64_t nconf, const double *pos_dev,
                      const double *w_dev, int32_t num_points,
                      int32_t num_groups, double *sums_dev, double *wsum_dev);

/* Plain device buffers, so that a configuration set can stay resident across
 * many qmc_evaluate_dev calls with different engines: the correlated-sampling
 * optimiser re-evaluates wf_abs_log / energy of one fixed set for every trial
 * value of the variational parameter (mrbp_qmc/model.py:818-942,
 * qmc_base/jastrow/model.py:1125-1206).  upload/download are synchronous. */
int qmc_buffer_alloc(int device, size_t bytes, void **out);
int qmc_buffer_free(void *buf);
int qmc_buffer_upload(void *dst_dev, const void *src_host, size_t bytes);
int qmc_buffer_download(void *dst_host, const void *src_dev, size_t bytes);

/* ---- VMC ensemble of independent Metropolis chains -------------------- */
/* vmc.Sampling + core_funcs.states_generator/blocks (qmc_base/vmc.py:557-648,
 * 670-770; jastrow/vmc.py:169-264; mrbp_qmc/vmc.py:174-233). */
int qmc_vmc_create(qmc_engine *eng, const qmc_vmc_params *p, qmc_vmc **out);
void qmc_vmc_destroy(qmc_vmc *v);
/* build_state (mrbp_qmc/vmc.py:145-165) for every chain: uploads pos[W][N],
 * evaluates log|psi|, resets the step counter; the next block's first yield
 * is the initial state flagged ACCEPTED (qmc_base/vmc.py:616-618). */
int qmc_vmc_set_state(qmc_vmc *v, const double *pos);
int qmc_vmc_get_state(qmc_vmc *v, double *pos, double *wf_abs_log,
                      double *energy_carry);
/* One block of `nyield` generator yields per chain.  Per-chain block sums
 * (sum of energy, of energy^2, accepted count) are always produced on the
 * device; the host copies requested here synchronise.  Series buffers are
 * [nyield][W] (step-major) host arrays or NULL; series_pos is [nyield][W][N]
 * (the chain configurations `as_chain` returns, qmc_base/vmc.py:785-900). */
int qmc_vmc_run_block(qmc_vmc *v, int64_t nyield, double *sum_energy,
                      double *sum_energy2, int64_t *num_accepted,
                      double *series_wf, double *series_energy,
                      uint8_t *series_stat, double *series_pos);
/* Device addresses of the chain state, pos[W][N] and wf[W].  NOTE: on the
 * device the particles of a configuration are kept in position order (an
 * internal label array maps lanes back to the caller's particle indices;
 * every host-facing call un-permutes).  Symmetric functions of a
 * configuration can be evaluated on these buffers directly. */
int qmc_vmc_state_dev(qmc_vmc *v, double **pos, double **wf);
/* Static structure factor parts of the CURRENT configurations summed over the
 * chains: out[num_modes][3] = sum_w (|rho_m|^2, Re rho_m, Im rho_m),
 * rho_m = sum_i exp(i 2 pi m z_i / L)  (the per-step quantity of
 * qmc_base/jastrow/vmc.py:304-351, evaluated for a whole ensemble in one
 * launch).  Host buffer; synchronous. */
int qmc_vmc_ssf(qmc_vmc *v, int32_t num_modes, double *out);
/* One-body density matrix parts of the CURRENT configurations summed over the
 * chains: out[nshift][2] = sum_w g1_w(s), sum_w g1_w(s)^2 (the quantity of
 * qmc_base/jastrow/model.py:932-965 for a whole ensemble, on the resident rows;
 * no position leaves the device).  Host buffers; synchronous; shifts checked
 * as by qmc_obdm. */
int qmc_vmc_obdm(qmc_vmc *v, int32_t nshift, const double *shifts, double *out);
/* Pair-distance histogram parts of the CURRENT configurations summed over the
 * chains: out[num_bins][2] = sum_w H_w[b], sum_w H_w[b]^2 (H as qmc_pair_dist,
 * distances as qmc_base/utils.py:35-51), on the resident rows; no position
 * leaves the device and the chain state is not touched.  Host buffer;
 * synchronous; num_bins checked as by qmc_pair_dist. */
int qmc_vmc_pair_dist(qmc_vmc *v, int32_t num_bins, double *out);
/* Triple-span histogram parts of the CURRENT configurations summed over the
 * chains: out[num_bins + 1][2] = sum_w T_w[b], sum_w T_w[b]^2 (T as
 * qmc_triple_dist), on the resident rows, after either move type; no position
 * leaves the device and the chain state is not touched.  Host buffer;
 * synchronous; num_bins and max_span checked as by qmc_triple_dist. */
int qmc_vmc_triple_dist(qmc_vmc *v, int32_t num_bins, double max_span,
                        double *out);
/* Energy parts of the CURRENT configurations summed over the chains:
 * out[4 + nrange][2] = sum_w x_w, sum_w x_w^2 of every column x of
 * qmc_energy_parts, on the resident rows, after either move type; no position
 * leaves the device and the chain state is not touched.  Host buffers;
 * synchronous; nrange and ranges checked as by qmc_energy_parts. */
int qmc_vmc_energy_parts(qmc_vmc *v, int32_t nrange, const double *ranges,
                         double *out);
/* Replica-swap sums of the CURRENT configurations, the chains 2p and 2p + 1
 * being the replicas of pair p: out[nlen][3] as sums_dev of
 * qmc_renyi_swap_reduce_dev, on the resident rows, after either move type; no
 * position leaves the device and the chain state is not touched.  An odd
 * num_chains is an error.  Host buffers; synchronous; nlen, lengths and origin
 * checked as by qmc_renyi_swap. */
int qmc_vmc_renyi_swap(qmc_vmc *v, int32_t nlen, const double *lengths,
                       double origin, double *out);
/* Region swap sums of the CURRENT configurations, the chains 2p and 2p + 1
 * being the replicas of pair p: out[nreg][3 + 2 num_charges] as sums_dev of
 * qmc_renyi_region_swap_reduce_dev (no counterpart in the reference), on the
 * resident rows, after either move type; no position leaves the device and
 * the chain state is not touched.  An odd num_chains is an error.  Host
 * buffers; synchronous; nreg, regions and origin checked as by
 * qmc_renyi_region_swap, num_charges as by the reduction. */
int qmc_vmc_renyi_region_swap(qmc_vmc *v, int32_t nreg, const double *regions,
                              double origin, int32_t num_charges, double *out);
/* One-particle swap sums of the CURRENT configurations, the chains 2p and
 * 2p + 1 being the replicas of pair p: out[3] as sums_dev of
 * qmc_particle_swap_reduce_dev, on the resident rows, after either move type
 * (the estimator does not depend on the order of a row); no position leaves
 * the device and the chain state is not touched.  An odd num_chains is an
 * error.  Host buffer; synchronous. */
int qmc_vmc_particle_swap(qmc_vmc *v, double *out);
/* Density-matrix sums on a grid of the CURRENT configurations, group = chain
 * index mod num_groups, unit weights: sums[num_groups][M][M] as sums of
 * qmc_obdm_grid, on the resident rows, after either move type (nothing depends
 * on the order of a row); no position leaves the device and the chain state
 * is not touched.  num_groups <= num_chains.  Host buffer; synchronous. */
int qmc_vmc_obdm_grid(qmc_vmc *v, int32_t num_points, int32_t num_groups,
                      double *sums);
/* Device addresses of the per-chain block sums of the last block
 * (sum_e[W], sum_e2[W], n_acc[W]) for on-device reductions / collectives. */
int qmc_vmc_block_sums_dev(qmc_vmc *v, double **sum_e, double **sum_e2,
                           int64_t **n_acc);
/* TEST ONLY: replay a recorded random stream instead of Philox.  tape is
 * host [W][steps][N + 1] (N proposal draws, then the accept uniform). */
int qmc_vmc_set_tape(qmc_vmc *v, const double *tape, int64_t steps);

/* ---- DMC walker ensemble ---------------------------------------------- */
/* dmc.Sampling + core_funcs.states_generator/blocks (qmc_base/dmc.py:614-787,
 * 815-971; jastrow/dmc.py:634-951, 1030-1174; mrbp_qmc/dmc.py:268-328). */
int qmc_dmc_create(qmc_engine *eng, const qmc_dmc_params *p, qmc_dmc **out);
void qmc_dmc_destroy(qmc_dmc *d);
/* build_state (mrbp_qmc/dmc.py:268-328): uploads pos[nw][N], computes energy
 * and drift of every walker, unit weights; ref_energy = mean energy unless
 * use_ref_energy.  The caller has already applied `[-target_num_walkers:]`. */
int qmc_dmc_set_state(qmc_dmc *d, int64_t nw, const double *pos,
                      int use_ref_energy, double ref_energy);
/* build_state from positions already in HBM; set_state_from_vmc takes the
 * first nw chains of a VMC ensemble of the same engine (VMC -> DMC hand-off
 * without a host round trip, tests/mrbp_qmc/test_dmc.py:76-83); when nw
 * exceeds the number of chains they are reused cyclically. */
int qmc_dmc_set_state_dev(qmc_dmc *d, int64_t nw, const double *pos_dev,
                          int use_ref_energy, double ref_energy);
int qmc_dmc_set_state_from_vmc(qmc_dmc *d, qmc_vmc *v, int64_t nw,
                               int use_ref_energy, double ref_energy);
/* Restart from a yielded State (qmc_base/dmc.py:707-716): confs[nw][2][N],
 * energy[nw], weight[nw] copied as they are; slot_energy[maxw] (or NULL) is the
 * whole props.energy array of that State. */
int qmc_dmc_set_full_state(qmc_dmc *d, int64_t nw, const double *confs,
                           const double *energy, const double *weight,
                           const double *slot_energy, double ref_energy);
/* `nsteps` generator iterations (branch -> diffuse/evaluate -> estimators ->
 * E_ref feedback).  Per-step series are host arrays of length nsteps or NULL
 * (PropsData, qmc_base/dmc.py:130-143). */
int qmc_dmc_run_block(qmc_dmc *d, int64_t nsteps, double *energy,
                      double *weight, uint64_t *num_walkers,
                      double *ref_energy, double *accum_energy);
/* Estimators of core_funcs.blocks (qmc_base/dmc.py:897-940;
 * qmc_base/jastrow/dmc.py:195-302, 363-631; mrbp_qmc/dmc.py:472-547).
 * run_block_est = run_block + per-step iter_ssf[nsteps][num_modes][3] /
 * iter_density[nsteps][num_bins] (host, may be NULL); the per-walker
 * forward-walking buffers are reset at the start of every block and the
 * estimators are skipped when eval_estimators == 0 (burn-in blocks). */
int qmc_dmc_set_estimators(qmc_dmc *d, const qmc_dmc_est_params *p);
int qmc_dmc_run_block_est(qmc_dmc *d, int64_t nsteps, int eval_estimators,
                          double *energy, double *weight, uint64_t *num_walkers,
                          double *ref_energy, double *accum_energy,
                          double *iter_ssf, double *iter_density);
/* The same for split-step (multi-GPU) drivers: est_begin_block opens a block
 * of nsteps steps (per-block resets), step_estimators evaluates the
 * estimators on the population yielded by the last step_finish into row
 * step_idx of this rank's iter buffers, est_iter_dev returns their device
 * addresses (iter_ssf[nsteps][num_modes][3], iter_density[nsteps][num_bins];
 * sums over this rank's walkers: linear, so ranks add them up). */
int qmc_dmc_est_begin_block(qmc_dmc *d, int64_t nsteps);
int qmc_dmc_step_estimators(qmc_dmc *d, int64_t step_idx);
int qmc_dmc_est_iter_dev(qmc_dmc *d, double **iter_ssf, double **iter_density);
/* est_iter_dev for any estimator: the device address of the per-step outputs
 * of slot `slot` ([nsteps][row_doubles] of the open block, sums over this
 * rank's walkers) and the doubles per step; NULL and 0 for a slot that is
 * off.  The slots, in the order in which a step evaluates them and in which
 * their per-walker rows follow one another in a walker record: */
enum {
    QMC_EST_SSF = 0,            /* S(k) */
    QMC_EST_DENSITY = 1,        /* density */
    QMC_EST_PAIR_DIST = 2,      /* g2(r) */
    QMC_EST_CM_DIFFUSION = 3,   /* centre-of-mass diffusion */
    QMC_EST_ISF = 4,            /* F(k, tau) */
    QMC_EST_OBDM = 5,           /* g1(s) */
    QMC_EST_SITE = 6,           /* site occupation statistics */
    QMC_EST_SLOTS = 7
};
int qmc_dmc_est_rows_dev(qmc_dmc *d, int32_t slot, double **rows,
                         int64_t *row_doubles);
/* Pair distribution g2(r) as a third block estimator (an extension: the
 * reference has none).  Per time step and bin, the pair-distance histograms
 * (as qmc_pair_dist: num_bins uniform bins over [0, L/2]) summed over the
 * yielded walkers: mixed, or pure with the per-walker rows carried through the
 * cloning table for pfw steps and divided by min(step + 1, pfw), the S(k)
 * transport.  num_bins in [1, 256]; 0 switches it off.  Set on its own:
 * neither this call nor qmc_dmc_set_estimators disturbs the other's settings,
 * and run_block_est / est_begin_block / step_estimators evaluate whichever of
 * the three are set.  read_pair_dist copies the first nsteps rows of the last
 * estimator block to the host, iter_out[nsteps][num_bins] (synchronises);
 * rows of a block run with eval_estimators == 0 are zero.  The rows are not
 * part of the walker record: single-GPU only. */
int qmc_dmc_set_pair_dist_estimator(qmc_dmc *d, int32_t num_bins, int32_t pure,
                                    int64_t pfw);
int qmc_dmc_read_pair_dist(qmc_dmc *d, int64_t nsteps, double *iter_out);
/* Centre-of-mass diffusion as a fourth block estimator (an extension: the
 * reference has none): the winding-number estimator of the superfluid
 * fraction.  Per time step t of an estimator block two doubles,
 * (sum_s Y_t(s), sum_s Y_t(s)^2) over the yielded walkers, where Y_t(s) is N
 * times the unwrapped centre-of-mass displacement of walker s since the first
 * yielded state of the block, carried through the cloning table (pure, unit
 * weights); row 0 is zero.  rho_s / rho is the large-t limit of
 * iter[t][1] / num_walkers[t] / (2 N t dt).  Needs |sum_i displacement_i| <
 * L / 2 per time step.  on != 0 switches it on, 0 off.  Set on its own, as the
 * pair distribution.  read_cm_diffusion copies the first nsteps rows of the
 * last estimator block to the host, iter_out[nsteps][2] (synchronises); rows
 * of a block run with eval_estimators == 0 are zero.  The per-walker rows are
 * not part of the walker record: single-GPU only. */
int qmc_dmc_set_cm_diffusion_estimator(qmc_dmc *d, int32_t on);
int qmc_dmc_read_cm_diffusion(qmc_dmc *d, int64_t nsteps, double *iter_out);
/* Imaginary-time density correlations F(k, tau) = <rho_k(tau) rho_-k(0)> as a
 * fifth block estimator (an extension: the reference has none).  num_modes K:
 * k_m = 2 pi m / L, m = 0 .. K-1, the mode set of S(k); num_lags T; lag l is
 * tau_l = l lag_stride dt.  Per time step t of an estimator block K (T + 2)
 * doubles, [m][c]: the sums over the yielded walkers of their rows.  The first
 * step of a block writes the origin of a row, columns T and T+1 = Re, Im
 * rho_m, and column 0 = |rho_m|^2; step t = l lag_stride, l < T, writes column
 * l = Re rho_m row[m][T] + Im rho_m row[m][T+1]; the rows travel through the
 * cloning table (pure, unit weights).  iter[t][m][l] / num_walkers[t]
 * estimates F(k_m, tau_l) with projection time (t - l lag_stride) dt behind
 * the later end: pure in the limit of a long block, to be read at the last
 * step of the block; columns T, T+1 over num_walkers[t] are the pure
 * <rho_m>.  Columns not measured yet are zero.  Limits: 1 <= num_modes <= 64,
 * 1 <= num_lags <= 64, lag_stride >= 1, num_modes (num_lags + 2) <= 1024;
 * num_modes = 0 switches it off.  Set on its own, as the pair distribution.
 * read_isf copies the first nsteps rows of the last estimator block to the
 * host, iter_out[nsteps][K][T+2] (synchronises); rows of a block run with
 * eval_estimators == 0 are zero.  The per-walker rows are not part of the
 * walker record: single-GPU only. */
int qmc_dmc_set_isf_estimator(qmc_dmc *d, int32_t num_modes, int32_t num_lags,
                              int64_t lag_stride);
int qmc_dmc_read_isf(qmc_dmc *d, int64_t nsteps, double *iter_out);
/* One-body density matrix g1(s) as a sixth block estimator, last in launch
 * order: the mixed estimator (g1 is non-local, forward walking does not
 * apply).  Per evaluated time step t of an estimator block nshift doubles,
 * iter[t][k] = sum over the yielded walkers, unweighted, of the g1 of the
 * walker's configuration at shifts[k] (host, as qmc_obdm takes them: any
 * finite value), computed by the code of qmc_obdm, fp64 whatever fast_math
 * says; a zero shift gives exactly num_walkers[t].  The estimator costs
 * nshift N (N - 1) shifted pair factors per walker, so it is evaluated only at
 * the steps with t % eval_stride == 0 (the first step of a block always); the
 * rows of the other steps are zero.  Limits: 0 <= nshift <= 256 (0 switches it
 * off; shifts and eval_stride are not read then), 1 <= eval_stride <=
 * 2^31 - 1.  The ensemble keeps a shift table of its own: qmc_obdm* calls on
 * the engine do not disturb it.  Set on its own, as the pair distribution.
 * read_obdm copies the first nsteps rows of the last estimator block to the
 * host, iter_out[nsteps][nshift] (synchronises); rows of a block run with
 * eval_estimators == 0 are zero.  The rows of several ranks are not summed:
 * single-GPU only. */
int qmc_dmc_set_obdm_estimator(qmc_dmc *d, int32_t nshift,
                               const double *shifts, int64_t eval_stride);
int qmc_dmc_read_obdm(qmc_dmc *d, int64_t nsteps, double *iter_out);
/* Site occupation statistics as a seventh block estimator, last in launch
 * order (an extension: the reference has none; csrc/qmc_site.h).  The lattice
 * period is 1 and the supercell holds S = supercell_size sites; site c is well
 * c with half a barrier (z_b / 2, z_b = 1 - z_a) on each side: particle i sits
 * on site c_i = min((int)wrap_box(z_i + z_b / 2, L), S - 1), and n_c is the
 * number of particles on site c.  Per time step num_occ + num_dist doubles,
 * [occ | corr], summed over the yielded walkers: occ[n], n < num_occ, the
 * number of sites with n_c = n (the last bin collects n_c >= num_occ - 1, so
 * sum_n occ[n] = S per walker), and corr[d], d < num_dist, the sum over c of
 * n_c n_{(c + d) mod S} (corr[0] = sum_c n_c^2; with num_dist = S,
 * sum_d corr[d] = N^2 per walker).  Mixed, or pure with the per-walker rows
 * carried through the cloning table for pfw steps and divided by
 * min(step + 1, pfw), as the pair distribution; the operator is local and
 * diagonal, so the pure estimate needs no extrapolation.  Every value is an
 * integer held in a double; fp64 whatever fast_math says.  Limits:
 * supercell_size integral, 1 <= S <= 512; num_occ >= 1, 0 <= num_dist <= S,
 * num_occ + num_dist <= 256; pfw >= 1 when pure; num_occ = 0 switches it off
 * (the rest is not read then).  Set on its own, as the pair distribution.
 * read_site copies the first nsteps rows of the last estimator block to the
 * host, iter_out[nsteps][num_occ + num_dist] (synchronises); rows of a block
 * run with eval_estimators == 0 are zero.  Single-GPU only: the rows are not
 * part of the walker record. */
int qmc_dmc_set_site_estimator(qmc_dmc *d, int32_t num_occ, int32_t num_dist,
                               int32_t pure, int64_t pfw);
int qmc_dmc_read_site(qmc_dmc *d, int64_t nsteps, double *iter_out);
/* The yielded ("actual") State after the last step (qmc_base/dmc.py:773-780):
 * confs[maxw][2][N], energy/weight[maxw], mask[maxw], cloning_ref[maxw];
 * scalars[5] = energy, weight, ref_energy, accum_energy, num_walkers. */
int qmc_dmc_get_state(qmc_dmc *d, double *confs, double *energy,
                      double *weight, uint8_t *mask, int64_t *cloning_ref,
                      double *scalars);
/* Split step for multi-GPU runs (external_reduce = 1): step_local runs the
 * branching and propagation of this rank's walkers and leaves this rank's
 * (E_t, W_t) in partial_dev[0..1]; the caller all-reduces them (RCCL) into
 * total_dev[0..1] on the same stream; step_finish applies the E_ref feedback
 * with the global sums and the global target. */
int qmc_dmc_step_local(qmc_dmc *d, double *partial_dev);
int qmc_dmc_step_finish(qmc_dmc *d, const double *total_dev);
int qmc_dmc_read_series(qmc_dmc *d, int64_t nsteps, double *energy,
                        double *weight, uint64_t *num_walkers,
                        double *ref_energy, double *accum_energy);
/* Population rebalance.  A walker record is walker_record_size doubles: pos[N],
 * drift[N], lane labels[N], energy, LOG of the branching weight (the device's
 * own storage form: records are opaque between engines of one build) and,
 * when estimators are set, the
 * walker's forward-walking rows (S(k) parts [num_modes][3], density
 * [num_bins]).  After set_record_rows(d, 1) one segment follows for every
 * other estimator that is on and keeps per-walker rows, in slot order: g2(r)
 * when pure [num_bins], the centre-of-mass diffusion [1], F(k, tau)
 * [num_modes][num_lags + 2], the site statistics when pure [num_occ +
 * num_dist]; the mixed g2 / site statistics and g1(s) keep no rows and add
 * nothing.  The switch may be set before or after the estimators: the layout
 * is that of the slots at the time of each walker_record_size / export /
 * import call (default off: S(k) and density rows only).  export packs walkers [first, first+count) of the current
 * population into buf_dev; import_walkers_at writes `count` records into
 * slots [first, first+count) and makes first+count the population size;
 * set_num_walkers drops the tail.  These three are stream-ordered (no host
 * synchronisation: the caller planned the transfer from num_walkers of every
 * rank).  num_walkers, import_walkers (append at the device's count) and
 * truncate (checked against it) read the device and synchronise. */
int qmc_dmc_num_walkers(qmc_dmc *d, int64_t *nw);
int qmc_dmc_set_record_rows(qmc_dmc *d, int32_t on);
int qmc_dmc_walker_record_size(qmc_dmc *d, int64_t *doubles);
int qmc_dmc_export_walkers(qmc_dmc *d, int64_t first, int64_t count,
                           double *buf_dev);
int qmc_dmc_import_walkers_at(qmc_dmc *d, int64_t first, int64_t count,
                              const double *buf_dev);
int qmc_dmc_set_num_walkers(qmc_dmc *d, int64_t nw);
int qmc_dmc_import_walkers(qmc_dmc *d, int64_t count, const double *buf_dev);
int qmc_dmc_truncate(qmc_dmc *d, int64_t new_nw);
/* TEST ONLY: replay recorded streams.  u[] / g[] are host arrays; step t
 * reads its branching uniforms at u[u_off[t] + parent] and its standard
 * normals at g[g_off[t] + slot*N + i]. */
int qmc_dmc_set_tape(qmc_dmc *d, const double *u, int64_t nu, const double *g,
                     int64_t ng, const int64_t *u_off, const int64_t *g_off,
                     int64_t nsteps);

#ifdef __cplusplus
}
#endif
#endif
