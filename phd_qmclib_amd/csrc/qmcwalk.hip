// qmcwalk.hip -- kernels and C-ABI of libqmcwalk.so (gfx950 / MI355X).
// Interface: include/qmcwalk.h.  Device building blocks: qmc_device.h.
//
// HBM layout (all fp64, "slot-major"): a walker slot owns one contiguous row
// of N positions and one of N drifts, pos[W][N] / drift[W][N]; the lane that
// owns particle i of walker w reads pos[w][i], so a lane group loads its row
// with one coalesced 8*G-byte access.  Per-walker scalars (energy, weight,
// slot energy, parent index) are plain [W] arrays.  DMC keeps two such
// population buffers (parents / children) that swap roles every time step.
#include "qmc_inst.h"
#include "qmc_kernels_misc.h"
#include "qmc_obdm.h"
#include "qmc_pairdist.h"
#include "qmc_tripledist.h"
#include "qmc_energy_parts.h"
#include "qmc_renyi.h"
#include "qmc_renyi_region.h"
#include "qmc_partent.h"
#include "qmc_obdm_grid.h"
#include "qmc_cmdiff.h"
#include "qmc_isf.h"
#include "qmc_site.h"
#include "qmc_vmc_sweep.h"
#include "../../include/qmcwalk.h"
#include "qmc_probe.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

// --------------------------------------------------------------- errors ---
static thread_local std::string g_err;

static int fail(const std::string &msg)
{
    g_err = msg;
    return 1;
}

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess)                                                \
            return fail(std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

// One hipMalloc allocation of T, freed with its owner: the members of the
// handles below and the temporaries of an entry point.  hipFree synchronises
// the device, so a temporary is declared where it may die: at the scope of the
// entry point, never inside a step loop.
template <typename T>
class DevBuf {
    T *p = nullptr;
    size_t cap = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // `count` elements in place of what it holds (an empty series: one)
    int alloc(size_t count)
    {
        release();
        if (count == 0) count = 1;
        HIP_TRY(hipMalloc((void **)&p, count * sizeof(T)));
        cap = count;
        return 0;
    }
    // grow-only: at least `count` elements; the contents do not survive growth
    int reserve(size_t count) { return count <= cap ? 0 : alloc(count); }
    T *get() const { return p; }
    operator T *() const { return p; }
};

extern "C" const char *qmc_last_error(void) { return g_err.c_str(); }
extern "C" int qmc_abi_version(void) { return QMCWALK_ABI_VERSION; }
#ifndef QMC_SRC_SHA
#define QMC_SRC_SHA "unknown"
#endif
extern "C" const char *qmc_source_hash(void) { return QMC_SRC_SHA; }
extern "C" int qmc_device_count(int *count)
{
    HIP_TRY(hipGetDeviceCount(count));
    return 0;
}

// ------------------------------------------------------------- handles ----
struct qmc_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevModel dm;
    DevBuf<DevModel> dm_dev;
    DevBuf<double> ob_table_dev;        // one-body table rows (or null)
    DevBuf<double> trig_table_dev;      // pair-angle row table (or null)
    DevBuf<unsigned long long> sec_prof_dev;     // QMC_TIMING builds only
    DevBuf<unsigned long long> diag_dev;         // DevModel::diag (QMC_NDIAG)
    qmc_model_params mp;
    int G = 64, P = 1;
    bool pad = false;
    bool fast = false;      // reduced-precision pair loop (float), off by default
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // kernel profile (qmc_engine_profile_begin/end): one event pair around
    // every launch of the dominant kernel (vmc_step / dmc_evolve)
    std::vector<hipEvent_t> prof_ev;
    size_t prof_used = 0;
    bool prof_on = false;
    // one-body density matrix scratch (qmc_obdm*): the shift table and the
    // per-configuration tile g1[tile][nshift], grown on demand
    DevBuf<double> obdm_stab, obdm_g1, obdm_sums;
    // pair distribution scratch (qmc_pair_dist*): the per-configuration tile
    // of histograms as doubles and the sums of qmc_vmc_pair_dist
    DevBuf<double> pd_hist, pd_sums;
    // three-body distribution scratch (qmc_triple_dist*), as the pair one
    DevBuf<double> td_hist, td_sums;
    // energy parts scratch (qmc_energy_parts*): the per-configuration tile of
    // rows and the sums of qmc_vmc_energy_parts
    DevBuf<double> ep_rows, ep_sums;
    // replica-swap scratch (qmc_renyi_swap*): the per-pair tile of rows
    // (swap, matched), their column sums, and the lengths and sums of
    // qmc_vmc_renyi_swap
    DevBuf<double> ry_rows, ry_colsum, ry_vmc;
    // two-segment replica-swap scratch (qmc_renyi_region_swap*): the per-pair
    // tile of rows (swap, occupations), column by column, and the regions
    // and sums of qmc_vmc_renyi_region_swap
    DevBuf<double> rg_rows, rg_vmc;
    // one-particle swap scratch (qmc_particle_swap*): the per-pair tile of
    // means and the sums of qmc_vmc_particle_swap
    DevBuf<double> pe_mean, pe_vmc;
    // density matrix on a grid (qmc_obdm_grid*): the partial matrices that
    // obdm_grid_fold_kernel adds up and the sums of qmc_vmc_obdm_grid
    DevBuf<double> og_part, og_vmc;

    qmc_engine() = default;
    qmc_engine(const qmc_engine &) = delete;
    // (with the engine's device current, as every entry point makes it; the
    // buffers go after this body)
    ~qmc_engine()
    {
        for (hipEvent_t ev : prof_ev) (void)hipEventDestroy(ev);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

// Bracket a launch of the dominant kernel with an event pair while a profile
// is open (bench.py: roofline.achieved needs that kernel's own duration).
struct ProfScope {
    qmc_engine *e;
    bool on;
    explicit ProfScope(const qmc_engine *ce) : e(const_cast<qmc_engine *>(ce))
    {
        on = e->prof_on && e->prof_used + 2 <= e->prof_ev.size();
        if (on) (void)hipEventRecord(e->prof_ev[e->prof_used], e->stream);
    }
    ~ProfScope()
    {
        if (on) {
            (void)hipEventRecord(e->prof_ev[e->prof_used + 1], e->stream);
            e->prof_used += 2;
        }
    }
};


static int pick_shape(int n, int &G, int &P, bool &pad)
{
    if (n < 1) return 1;
    // tuning knob (tools/shape_bench.py): QMCWALK_SHAPE="G,P" forces a lane
    // group shape when it can hold the model (n <= G * P)
    if (const char *env = getenv("QMCWALK_SHAPE")) {
        int g = 0, p = 0;
        if (sscanf(env, "%d,%d", &g, &p) == 2 && n <= g * p) {
#define QMC_LEGAL(sg, sp) || (g == sg && p == sp)
            if (false QMC_FOR_ALL_SHAPES(QMC_LEGAL)) {
                G = g; P = p; pad = (n != G * P);
                return 0;
            }
#undef QMC_LEGAL
        }
    }
    if (n <= 16) { G = 16; P = 1; }
    else if (n <= 32) { G = 16; P = 2; }
    else if (n <= 64) { G = 64; P = 1; }
    else if (n <= 128) { G = 64; P = 2; }
    else if (n <= 256) { G = 64; P = 4; }
    else if (n <= 512) { G = 64; P = 8; }
    else return 1;
    pad = (n != G * P);
    return 0;
}

// kernels are instantiated in inst_G_P.hip (one translation unit per shape)
#define QMC_EXTERN_TU(name) QMC_TU_##name(extern)
QMC_FOR_ALL_TUS(QMC_EXTERN_TU)
#undef QMC_EXTERN_TU
// (the single-particle sweeps, qmc_vmc_sweep.h: inst_SWEEP.hip)
QMC_TU_SWEEP(extern)
// (the energy parts, qmc_energy_parts.h: inst_EPARTS.hip)
QMC_TU_EPARTS(extern)

// ------------------------------------------------------------ dispatch ----
// The masked variant is also the leaner one in registers (its per-pair guards
// stop the compiler from keeping several pairs in flight: 110-160 VGPRs
// against 134-282 at P = 4, 8), and occupancy is what the large shapes lack:
// from this P on every kernel family runs it whether the model fills the shape
// or not (and the unmasked variants never launched are not instantiated,
// qmc_inst.h).
// (P = 8: the unmasked dmc_evolve needs 253 registers and ran 1.7x slower,
// profiles/r02_n512_tile_sweep.txt)
static constexpr int MASK_FROM_P = 4;

template <template <int, int, bool, bool> class L, typename... A>
static int dispatch_shape(const qmc_engine *e, A &&...args)
{
    const bool zc = e->dm.zclass != 0;
#define QMC_CASE(g, p)                                                        \
    if (e->G == g && e->P == p) {                                             \
        if (p >= MASK_FROM_P || e->pad) {                                     \
            if (zc) return L<g, p, true, true>::run(e, args...);              \
            return L<g, p, true, false>::run(e, args...);                     \
        }                                                                     \
        if constexpr (p < MASK_FROM_P) {                                      \
            if (zc) return L<g, p, false, true>::run(e, args...);             \
            return L<g, p, false, false>::run(e, args...);                    \
        }                                                                     \
    }
    QMC_FOR_ALL_SHAPES(QMC_CASE)
#undef QMC_CASE
    return fail("unsupported boson_number");
}

template <int G, int P, bool ZC>
static size_t lds_bytes()
{
    return (size_t)(WalkBlock<G>::N / G) * GroupLds<G, P, ZC>::DOUBLES *
           sizeof(double);
}

// (the stepping kernels: StepLds, qmc_kernels.h)
template <int G, int P, bool PAD, bool ZC, bool DMC = false>
static size_t step_lds_bytes()
{
    return (size_t)(WalkBlock<G>::N / G) *
           StepLds<G, P, PAD, ZC, DMC>::DOUBLES * sizeof(double);
}

// Dynamic LDS above the default limit must be opted into per kernel.
template <typename K>
static void allow_lds(K kernel, size_t bytes)
{
    if (bytes > 48 * 1024)
        (void)hipFuncSetAttribute((const void *)kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes);
}

template <int G>
static unsigned grid_for(long long nwalkers)
{
    const long long gpb = WalkBlock<G>::N / G;
    long long blocks = (nwalkers + gpb - 1) / gpb;
    // (one wavefront per workgroup: walker_of_block permutes runs of 128)
    if (gpb == 1) blocks = (blocks + 127) / 128 * 128;
    return (unsigned)blocks;
}

// The one place that launches a walker kernel: lane groups of G for `nwalkers`
// walkers, on the engine's stream, with the model constants.
template <int G, typename A>
static int launch_walkers(const qmc_engine *e,
                          void (*kernel)(const DevModel *, A), size_t lds,
                          long long nwalkers, const A &a)
{
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(grid_for<G>(nwalkers)),
                       dim3(WalkBlock<G>::N), lds, e->stream, e->dm_dev, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The float pair loop exists for the one-wavefront-per-walker shapes with
// pairs classified from the sines (qmc_inst.h).
template <int G, bool ZC>
static constexpr bool has_fast() { return G == 64 && !ZC; }

// f(R{}) with the pair-loop type R of this engine on this shape; f names a
// float instantiation only where one exists.
template <int G, bool ZC, typename F>
static int with_pair_type(const qmc_engine *e, F f)
{
    if constexpr (has_fast<G, ZC>())
        if (e->fast) return f(float{});
    return f(double{});
}

template <int G, int P, bool PAD, bool ZC>
struct LaunchEval {
    static int run(const qmc_engine *e, const EvalArgs &a)
    {
        if (a.nconf <= 0) return 0;
        return with_pair_type<G, ZC>(e, [&](auto r) {
            return launch_walkers<G>(
                e, evaluate_kernel<G, P, PAD, ZC, decltype(r)>,
                lds_bytes<G, P, ZC>(), a.nconf, a);
        });
    }
};

template <int G, int P, bool PAD, bool ZC>
struct LaunchPrep {
    static int run(const qmc_engine *e, const PrepArgs &a)
    {
        if (a.nconf <= 0) return 0;
        return with_pair_type<G, ZC>(e, [&](auto r) {
            return launch_walkers<G>(
                e, prepare_kernel<G, P, PAD, ZC, decltype(r)>,
                lds_bytes<G, P, ZC>(), a.nconf, a);
        });
    }
};

template <int G, int P, bool PAD, bool ZC>
struct LaunchVmc {
    // One launch from yield a.y on; *ran = the yields it ran: 1, or on a
    // VmcFused shape all a.nsteps steady yields left in the block.
    static int run(const qmc_engine *e, const VmcArgs &a, long long *ran)
    {
        const size_t lds = step_lds_bytes<G, P, PAD, ZC>();
        const bool lean = !a.tape && !a.gaussian && !a.ser_wf && !a.ser_e &&
                          !a.ser_stat && !a.ser_pos;
        // (the steady variant: every yield of a block after its first; on a
        // VmcFused shape the first as well, unless it is the forced initial
        // yield -- the fused kernel restarts the sums itself)
        constexpr bool FUSED = VmcFused<G, P, ZC>::ON;
        const bool steady = lean && !a.forced && (FUSED || !a.reset_sums);
        *ran = (steady && FUSED) ? (long long)a.nsteps : 1;
        ProfScope prof(e);
        return with_pair_type<G, ZC>(e, [&](auto r) {
            using R = decltype(r);
            auto kernel = steady ? vmc_step_kernel<G, P, PAD, ZC, true, R, true>
                          : lean ? vmc_step_kernel<G, P, PAD, ZC, true, R, false>
                                 : vmc_step_kernel<G, P, PAD, ZC, false, R, false>;
            return launch_walkers<G>(e, kernel, lds, a.W, a);
        });
    }
};

// The single-particle sweeps (qmc_vmc_sweep.h): every yield of a block in one
// launch, fp64 whatever fast_math says; the proposals and the by-label tables
// of a chain behind the LDS region of the pair sums.
template <int G, int P, bool PAD, bool ZC>
struct LaunchSweep {
    static int run(const qmc_engine *e, const VmcArgs &a)
    {
        ProfScope prof(e);
        const size_t lds = (size_t)(WalkBlock<G>::N / G) *
                           SweepLds<G, P, PAD, ZC>::DOUBLES * sizeof(double);
        return launch_walkers<G>(e, vmc_sweep_kernel<G, P, PAD, ZC>, lds, a.W,
                                 a);
    }
};

template <int G, int P, bool PAD, bool ZC>
struct LaunchEvolve {
    static int run(const qmc_engine *e, const EvolveArgs &a)
    {
        ProfScope prof(e);
        return with_pair_type<G, ZC>(e, [&](auto r) {
            return launch_walkers<G>(
                e, dmc_evolve_kernel<G, P, PAD, ZC, decltype(r)>,
                step_lds_bytes<G, P, PAD, ZC, true>(), a.maxw, a);
        });
    }
};

// The second-order step (qmc_evolve2.h): the same arguments, two more rows of
// LDS per walker.
template <int G, int P, bool PAD, bool ZC>
struct LaunchEvolve2 {
    static int run(const qmc_engine *e, const EvolveArgs &a)
    {
        ProfScope prof(e);
        const size_t lds = (size_t)(WalkBlock<G>::N / G) *
                           Step2Lds<G, P, PAD, ZC>::DOUBLES * sizeof(double);
        return with_pair_type<G, ZC>(e, [&](auto r) {
            return launch_walkers<G>(
                e, dmc_evolve2_kernel<G, P, PAD, ZC, decltype(r)>, lds, a.maxw,
                a);
        });
    }
};

// -------------------------------------------------------------- engine ----
static void build_dev_model(const qmc_model_params &p, DevModel &d)
{
    memset(&d, 0, sizeof(d));
    d.n = (int)p.boson_number;
    d.is_free = p.is_free != 0;
    d.is_ideal = p.is_ideal != 0;
    d.defects_sep = (int)(p.defects_sep > 0 ? p.defects_sep : 1);
    d.L = p.supercell_size;
    d.half_L = 0.5 * d.L;
    d.rm = fabs(p.tbf_contact_cutoff);
    d.L_minus_rm = d.L - d.rm;
    d.two_over_L = 2.0 / d.L;
    d.k2_2pi = p.param_k2 * (2.0 / QMC_PI);
    d.k2 = p.param_k2;
    d.k2sq = d.k2 * d.k2;
    double phi = p.param_k2 * p.param_r_off;
    d.cphi = cos(phi);
    d.sphi = sin(phi);
    d.sec_cut = -1;
    d.am_cphi = fabs(p.param_am) * d.cphi;
    d.am_sphi = fabs(p.param_am) * d.sphi;
    d.m_k2cphi = -d.k2 * d.cphi;
    d.k2sphi = d.k2 * d.sphi;
    double th = p.param_k2 * d.L;
    d.cth = cos(th);
    d.sth = fabs(sin(th));
    d.sth_sign = sin(th) < 0.0 ? (int)0x80000000u : 0;
    d.sth_signed = sin(th);
    // leading all-short steps (qmc_device.h): theta = k2 D' - phi must identify
    // D' within a window of two box lengths
    d.sp_ok = (!d.is_ideal && th > 0.0 && th < QMC_PI - 1e-9 &&
               d.rm < d.half_L) ? 1 : 0;
    d.sp_xlo = -d.k2 * sin(d.k2 * d.rm - phi);
    d.sp_xhi = d.k2 * sin(phi);
    d.sp_cos = cos(d.k2 * d.rm);
    {
        // angles added to k2 z_own for the four short-range cases
        const double ang[4] = { -phi, phi, phi - th, th - phi };
        for (int v = 0; v < 4; ++v) {
            d.var_cos[v] = cos(ang[v]);
            d.var_sin[v] = sin(ang[v]);
        }
        d.m_k2 = -d.k2;
    }
    d.sin_rm = (d.rm >= d.half_L) ? 1.0 : sin(QMC_PI * d.rm / d.L);
    // sin(pi r / L) is flat near r = L/2: classify from positions there
    d.zclass = d.rm > 0.45 * d.L;
    double pi_L = QMC_PI / d.L;
    d.a_long = pi_L * p.param_beta;
    d.b_long = pi_L * pi_L * p.param_beta;
    d.a_long_sq = d.a_long * d.a_long;
    d.m_k2_over_a = d.a_long != 0.0 ? -d.k2 / d.a_long : 0.0;
    d.m_a_over_k2 = d.k2 != 0.0 ? -d.a_long / d.k2 : 0.0;
    d.beta = p.param_beta;
    d.inv_beta = p.param_beta != 0.0 ? 1.0 / p.param_beta : 0.0;
    d.one_minus_beta = 1.0 - p.param_beta;
    d.log_am = log(fabs(p.param_am));
    d.z_a = 1.0 / (1.0 + p.lattice_ratio);
    d.z_b = p.lattice_ratio / (1.0 + p.lattice_ratio);
    d.k1 = p.param_k1;
    d.k1_2pi = p.param_k1 * (2.0 / QMC_PI);
    d.kp1 = p.param_kp1;
    d.e0 = p.param_e0;
    d.v0 = p.lattice_depth;
    d.v0d = p.defect_magnitude;
    d.uniform_barrier = (d.defects_sep == 1 || d.v0d == d.v0) ? 1 : 0;
    d.v_barrier = (d.defects_sep == 1) ? d.v0d : d.v0;
    d.k1_half = 0.5 * p.param_k1;
    d.v0_minus_e0 = p.lattice_depth - p.param_e0;
    if (!d.is_free) {
        double sh = sinh(0.5 * sqrt(d.v0 - d.e0) * d.z_b);
        d.cf = sqrt(1 + d.v0 / d.e0 * sh * sh);
    } else {
        d.cf = 1.0;
    }
}

// ---- one-body table (qmc_device.h one_body_tab) ---------------------------
// Closed forms of mrbp_qmc/model.py:404-464 in long double.
static void ob_exact(const DevModel &d, long double zc, bool barrier,
                     long double &ldz, long double &logf)
{
    if (barrier) {
        const long double x = (long double)d.kp1 *
                              (zc - 1.0L + 0.5L * (long double)d.z_b);
        ldz = (long double)d.kp1 * tanhl(x);
        logf = logl(coshl(x));
    } else {
        const long double x = (long double)d.k1 *
                              (zc - 0.5L * (long double)d.z_a);
        ldz = -(long double)d.k1 * tanl(x);
        logf = logl((long double)d.cf * cosl(x));
    }
}

// Degree-DEG interpolant of f on [a, a + h] at Chebyshev nodes, as monomial
// coefficients in t = (x - a) / h (long double elimination, partial pivoting).
template <int DEG, typename F>
static void ob_fit(F f, long double a, long double h, double *coef)
{
    constexpr int K = DEG + 1;
    long double A[K][K + 1];
    for (int j = 0; j < K; ++j) {
        const long double t = 0.5L * (1.0L + cosl(3.14159265358979323846264338L *
                                                  (2 * j + 1) / (2.0L * K)));
        long double pw = 1.0L;
        for (int k = 0; k < K; ++k) { A[j][k] = pw; pw *= t; }
        A[j][K] = f(a + h * t);
    }
    for (int c = 0; c < K; ++c) {
        int piv = c;
        for (int r = c + 1; r < K; ++r)
            if (fabsl(A[r][c]) > fabsl(A[piv][c])) piv = r;
        for (int k = 0; k <= K; ++k) std::swap(A[c][k], A[piv][k]);
        for (int r = c + 1; r < K; ++r) {
            const long double g = A[r][c] / A[c][c];
            for (int k = c; k <= K; ++k) A[r][k] -= g * A[c][k];
        }
    }
    for (int r = K - 1; r >= 0; --r) {
        long double v = A[r][K];
        for (int k = r + 1; k < K; ++k) v -= A[r][k] * (long double)coef[k];
        coef[r] = (double)(v / A[r][r]);
    }
}

static double ob_horner(const double *c, int deg, double t)
{
    double p = c[deg];
    for (int k = deg - 1; k >= 0; --k) p = fma(p, t, c[k]);
    return p;
}

// Rows of one lattice region at `m` intervals; -> worst error of the double
// Horner evaluation against the closed forms, relative to max(1, |f|).
static double ob_build_region(const DevModel &d, bool barrier, int m,
                              double *rows)
{
    const long double lo = barrier ? (long double)d.z_a : 0.0L;
    const long double len = barrier ? 1.0L - (long double)d.z_a
                                    : (long double)d.z_a;
    const long double h = len / m;
    double worst = 0.0;
    for (int i = 0; i < m; ++i) {
        const long double a = lo + h * i;
        double *r = rows + (size_t)i * OB_ROW;
        ob_fit<OB_DEG>([&](long double x) {
            long double l, g; ob_exact(d, x, barrier, l, g); return l; },
            a, h, r);
        ob_fit<OB_DEG>([&](long double x) {
            long double l, g; ob_exact(d, x, barrier, l, g); return g; },
            a, h, r + 8);
        for (int q = 0; q <= 12; ++q) {
            const double t = q / 12.0;
            long double l, g;
            ob_exact(d, a + h * (long double)t, barrier, l, g);
            const double e1 = fabs(ob_horner(r, OB_DEG, t) - (double)l) /
                              fmax(1.0, fabs((double)l));
            const double e2 = fabs(ob_horner(r + 8, OB_DEG, t) - (double)g) /
                              fmax(1.0, fabs((double)g));
            worst = fmax(worst, fmax(e1, e2));
        }
    }
    return worst;
}

static double g_ob_last_err[2] = { 0.0, 0.0 };   // diagnostics (info call)
// (checked at the builder's sample points; between them the device's rows
// reach 3.2e-15, tests/test_gpu_device_math.py)
static constexpr double OB_TOL = 2e-15;
static constexpr int OB_MAX_ROWS = 1024;        // per region (128 KB)

// -> host table (empty when the model does not reach OB_TOL: the kernels then
// evaluate the closed forms directly) and the interval counts.
static void build_ob_table(const DevModel &d, std::vector<double> &tab,
                           int &m1, int &m2)
{
    tab.clear();
    m1 = m2 = 0;
    if (d.is_free) return;
    if (const char *env = getenv("QMCWALK_OB_TABLE"))
        if (env[0] == '0') return;              // tuning / A-B knob
    if (!(d.z_a > 0.0 && d.z_a < 1.0) || !std::isfinite(d.k1) ||
        !std::isfinite(d.kp1) || !std::isfinite(d.cf))
        return;
    std::vector<double> reg[2];
    int m[2] = { 0, 0 };
    for (int b = 0; b < 2; ++b) {
        for (int cand = 16; cand <= OB_MAX_ROWS; cand *= 2) {
            reg[b].assign((size_t)cand * OB_ROW, 0.0);
            const double err = ob_build_region(d, b == 1, cand, reg[b].data());
            g_ob_last_err[b] = err;
            if (std::isfinite(err) && err <= OB_TOL) { m[b] = cand; break; }
        }
        if (!m[b]) return;
    }
    // the row map of the kernel is the larger of two lines: the barrier's
    // intervals must not be wider than the well's
    const int need2 = (int)std::ceil((double)m[0] * (1.0 - d.z_a) / d.z_a);
    if (need2 > m[1]) {
        if (need2 > 8 * OB_MAX_ROWS) return;
        m[1] = need2;
        reg[1].assign((size_t)m[1] * OB_ROW, 0.0);
        const double err = ob_build_region(d, true, m[1], reg[1].data());
        g_ob_last_err[1] = err;
        if (!(std::isfinite(err) && err <= OB_TOL)) return;
    }
    m1 = m[0]; m2 = m[1];
    tab = reg[0];
    tab.insert(tab.end(), reg[1].begin(), reg[1].end());
    // closing row: z_cell -> 1 rounds into it at t = 0, where the periodic
    // factor continues with the first well interval
    tab.insert(tab.end(), reg[0].begin(), reg[0].begin() + OB_ROW);
}

// Row table of the pair-table angles (qmc_device.h trig_tab): the smallest
// power-of-two row count that keeps both angle offsets inside QMC_TRIG_DMAX,
// nothing if that takes more than QMC_TRIG_MAX_ROWS rows (128 KB).
#define QMC_TRIG_DMAX 4.0e-3
#define QMC_TRIG_MAX_ROWS 4096
static void build_trig_table(DevModel &d, std::vector<double> &tab)
{
    tab.clear();
    d.trig_table = nullptr;
    d.tg_rows = 0;
    if (d.is_ideal || !(d.L > 0.0)) return;
    const double span = fmax(QMC_PI, fabs(d.k2) * d.L);
    int rows = 256;
    while (rows <= QMC_TRIG_MAX_ROWS && span / (2.0 * rows) > QMC_TRIG_DMAX)
        rows *= 2;
    if (rows > QMC_TRIG_MAX_ROWS) return;
    const double h = d.L / rows;
    tab.resize((size_t)rows * 4);
    const long double pil = 3.141592653589793238462643383279502884L;
    for (int r = 0; r < rows; ++r) {
        const long double zr = ((long double)r + 0.5L) * (long double)h;
        const long double a1 = pil * zr / (long double)d.L;
        const long double a2 = (long double)d.k2 * zr;
        tab[4 * r + 0] = (double)sinl(a1);
        tab[4 * r + 1] = (double)cosl(a1);
        tab[4 * r + 2] = (double)sinl(a2);
        tab[4 * r + 3] = (double)cosl(a2);
    }
    d.tg_rows = rows;
    d.tg_h = h;
    d.tg_inv_h = (double)rows / d.L;
    d.tg_a1 = QMC_PI / d.L;
    d.tg_b1 = -d.tg_a1 * 0.5 * h;
    d.tg_a2 = d.k2;
    d.tg_b2 = -d.k2 * 0.5 * h;
}

// Diagnostic, no GPU needed: the table a model would get.
extern "C" int qmc_model_one_body_table_info(const qmc_model_params *model,
                                             int32_t *rows_well,
                                             int32_t *rows_barrier,
                                             double *max_err)
{
    if (!model) return fail("qmc_model_one_body_table_info: null argument");
    DevModel d;
    build_dev_model(*model, d);
    std::vector<double> tab;
    int m1 = 0, m2 = 0;
    g_ob_last_err[0] = g_ob_last_err[1] = 0.0;
    build_ob_table(d, tab, m1, m2);
    if (rows_well) *rows_well = m1;
    if (rows_barrier) *rows_barrier = m2;
    if (max_err) *max_err = fmax(g_ob_last_err[0], g_ob_last_err[1]);
    return 0;
}

static int engine_create_impl(const qmc_model_params *model, int device,
                              void *stream, bool caller_stream,
                              qmc_engine **out)
{
    if (!model || !out) return fail("qmc_engine_create: null argument");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail("qmc_engine_create: no HIP device");
    if (device < 0 || device >= ndev)
        return fail("qmc_engine_create: bad device index");
    // (nothing of the device is held before hipSetDevice below)
    std::unique_ptr<qmc_engine> e(new qmc_engine());
    e->device = device;
    e->mp = *model;
    if (pick_shape((int)model->boson_number, e->G, e->P, e->pad))
        return fail("qmc_engine_create: boson_number must be in [1, 512]");
    build_dev_model(*model, e->dm);
    // lanes of a group the rotation runs over: all of them when the model
    // fills the shape, else the smallest even number that holds it
    e->dm.ge = e->pad ? 2 * ((e->dm.n + 2 * e->P - 1) / (2 * e->P)) : e->G;
    // domain of the short-range kernel (qmc_device.h pair_core): the matching
    // conditions of mrbp_qmc/model.py:340-392 give phi = k2 r_off in (0, pi/2)
    // and k2 rm in (0, pi/2) for every repulsive model
    if (!e->dm.is_ideal &&
        (e->dm.sphi < 0.0 || e->dm.cphi < 0.0 ||
         e->dm.k2 * e->dm.rm >= 0.5 * QMC_PI || e->dm.k2 <= 0.0))
        return fail("qmc_engine_create: two-body parameters outside the "
                    "model's domain (need 0 < k2 rm < pi/2, 0 <= k2 r_off <= pi/2)");
    // the sorted-row pair sums (qmc_sorted64.h) count every pair quotient in
    // units of a_long = (pi / L) beta: a non-ideal model with beta = 0 (which
    // the reference's matching conditions never produce, mrbp_qmc/model.py:
    // 255-274) would lose its short-range terms there without an error
    if (!e->dm.is_ideal && !(e->dm.a_long != 0.0))
        return fail("qmc_engine_create: a non-ideal model needs "
                    "param_beta != 0");
    HIP_TRY(hipSetDevice(device));
    if (caller_stream) {
        // the caller's stream as it is; NULL is the legacy default stream
        e->stream = (hipStream_t)stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->own_stream = true;
    }
    HIP_TRY(hipEventCreate(&e->ev0));
    HIP_TRY(hipEventCreate(&e->ev1));
    {
        std::vector<double> tab;
        int m1 = 0, m2 = 0;
        build_ob_table(e->dm, tab, m1, m2);
        if (!tab.empty()) {
            if (e->ob_table_dev.alloc(tab.size())) return 1;
            HIP_TRY(hipMemcpy(e->ob_table_dev, tab.data(),
                              tab.size() * sizeof(double),
                              hipMemcpyHostToDevice));
            DevModel &d = e->dm;
            d.ob_table = e->ob_table_dev;
            d.ob_m1 = m1; d.ob_m2 = m2;
            d.ob_invh1 = (double)m1 / d.z_a;
            d.ob_invh2 = (double)m2 / (1.0 - d.z_a);
            d.ob_shift2 = (double)m1 / d.ob_invh2 - d.z_a;
        }
    }
    {
        std::vector<double> tab;
        build_trig_table(e->dm, tab);
        if (!tab.empty()) {
            if (e->trig_table_dev.alloc(tab.size())) return 1;
            HIP_TRY(hipMemcpy(e->trig_table_dev, tab.data(),
                              tab.size() * sizeof(double),
                              hipMemcpyHostToDevice));
            e->dm.trig_table = e->trig_table_dev;
        }
    }
#if defined(QMC_TIMING)
    if (e->sec_prof_dev.alloc((size_t)QMC_SEC_COPIES * 2 * QMC_NSEC)) return 1;
    HIP_TRY(hipMemset(e->sec_prof_dev, 0, (size_t)QMC_SEC_COPIES * 2 *
                      QMC_NSEC * sizeof(unsigned long long)));
    e->dm.sec_prof = e->sec_prof_dev;
#endif
    if (e->diag_dev.alloc(QMC_NDIAG)) return 1;
    HIP_TRY(hipMemset(e->diag_dev, 0, QMC_NDIAG * sizeof(unsigned long long)));
    e->dm.diag = e->diag_dev;
    if (e->dm_dev.alloc(1)) return 1;
    HIP_TRY(hipMemcpy(e->dm_dev, &e->dm, sizeof(DevModel),
                      hipMemcpyHostToDevice));
    *out = e.release();
    return 0;
}

// Diagnostic, no GPU needed: the pair-angle row table a model would get and
// the worst deviation of trig_tab's arithmetic (restated here on the host,
// operation for operation) from long-double sin / cos over [0, L).
static void trig_small_host(double d, double &s, double &c)
{
    const double d2 = d * d;
    s = fma(d * d2, fma(d2, 1.0 / 120.0, -1.0 / 6.0), d);
    c = fma(d2, fma(d2, 1.0 / 24.0, -0.5), 1.0);
}

extern "C" int qmc_model_trig_table_info(const qmc_model_params *model,
                                         int32_t *rows, double *max_err)
{
    if (!model) return fail("qmc_model_trig_table_info: null argument");
    DevModel d;
    build_dev_model(*model, d);
    std::vector<double> tab;
    build_trig_table(d, tab);
    if (rows) *rows = d.tg_rows;
    double worst = 0.0;
    if (d.tg_rows) {
        const long double pil = 3.141592653589793238462643383279502884L;
        const int samples = 7;            // per row, edges included
        for (int r = 0; r < d.tg_rows; ++r) {
            for (int j = 0; j <= samples; ++j) {
                double z = ((double)r + (double)j / samples) * d.tg_h;
                if (j == samples) z = nextafter(z, 0.0);
                const int rr = (int)(z * d.tg_inv_h);
                if (rr < 0 || rr >= d.tg_rows) continue;   // device falls back
                const double dz = fma(-(double)rr, d.tg_h, z);
                const double *row = &tab[4 * (size_t)rr];
                double sd, cd, got[4];
                trig_small_host(fma(dz, d.tg_a1, d.tg_b1), sd, cd);
                got[0] = fma(row[0], cd, row[1] * sd);
                got[1] = fma(row[1], cd, -(row[0] * sd));
                trig_small_host(fma(dz, d.tg_a2, d.tg_b2), sd, cd);
                got[2] = fma(row[2], cd, row[3] * sd);
                got[3] = fma(row[3], cd, -(row[2] * sd));
                const long double a1 = pil * (long double)z / (long double)d.L;
                const long double a2 = (long double)d.k2 * (long double)z;
                const long double ref[4] = { sinl(a1), cosl(a1), sinl(a2),
                                             cosl(a2) };
                for (int k = 0; k < 4; ++k)
                    worst = fmax(worst, (double)fabsl((long double)got[k] - ref[k]));
            }
        }
    }
    if (max_err) *max_err = worst;
    return 0;
}

// Diagnostic, no GPU needed: log_pos (qmc_math.h) restated on the host,
// operation for operation, over 10^5 arguments between 1e-300 and 1e300 and
// a dense sweep around 1; worst |got - log x| / (1 + |log x|) against long
// double.
static const double g_log_tab_host[2 * QMC_LOG_ROWS] = { QMC_LOG_TAB_VALUES };

static double log_pos_host(double x)
{
    const double LN2_HI = 6.93147180369123816490e-01;
    const double LN2_LO = 1.90821492927058770002e-10;
    int k;
    const double m = frexp(x, &k);                         // [1/2, 1)
    const int r = (int)fma(m, (double)(2 * QMC_LOG_ROWS), -(double)QMC_LOG_ROWS) &
                  (QMC_LOG_ROWS - 1);                      // (as on the device)
    const double inv_c = g_log_tab_host[2 * r], L = g_log_tab_host[2 * r + 1];
    const double d = fma(m, inv_c, -1.0);
    double q = fma(d, 0.2, -0.25);
    q = fma(q, d, 1.0 / 3.0);
    q = fma(q, d, -0.5);
    const double lm = fma(d * d, q, d) + L;
    const double kd = (double)k;
    return fma(kd, LN2_HI, fma(kd, LN2_LO, lm));
}

extern "C" int qmc_log_table_info(int32_t *rows, double *max_err)
{
    if (rows) *rows = QMC_LOG_ROWS;
    double worst = 0.0;
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 200000; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const double u = (double)(state >> 11) * (1.0 / 9007199254740992.0);
        double x;
        if (i < 100000) x = pow(10.0, -300.0 + 600.0 * u);          // any size
        else if (i < 150000) x = 1.0 + (u - 0.5) * 1e-3 * (i % 1000); // near 1
        else x = u + 1e-17;                                          // (0, 1)
        const long double ref = logl((long double)x);
        const double err = (double)(fabsl((long double)log_pos_host(x) - ref) /
                                    (1.0L + fabsl(ref)));
        if (err > worst) worst = err;
    }
    // row edges
    for (int r = 0; r <= QMC_LOG_ROWS; ++r) {
        for (int s = -1; s <= 1; ++s) {
            double x = QMC_LOG_LO + (double)r / QMC_LOG_INVW;
            if (s < 0) x = nextafter(x, 0.0);
            if (s > 0) x = nextafter(x, 2.0);
            const long double ref = logl((long double)x);
            const double err = (double)(fabsl((long double)log_pos_host(x) - ref) /
                                        (1.0L + fabsl(ref)));
            if (err > worst) worst = err;
        }
    }
    if (max_err) *max_err = worst;
    return 0;
}

extern "C" int qmc_engine_create(const qmc_model_params *model, int device,
                                 void *stream, qmc_engine **out)
{
    return engine_create_impl(model, device, stream, stream != nullptr, out);
}

extern "C" int qmc_engine_create_on_stream(const qmc_model_params *model,
                                           int device, void *stream,
                                           qmc_engine **out)
{
    return engine_create_impl(model, device, stream, true, out);
}

extern "C" int qmc_engine_set_fast_math(qmc_engine *e, int on, int *in_effect)
{
    if (!e) return fail("qmc_engine_set_fast_math: null engine");
    // available for the one-wavefront-per-walker shapes (boson_number > 32)
    // unless pairs are classified from positions (cutoff close to L/2);
    // elsewhere the request is a no-op: the knob grants a permission
    const bool can = e->G == 64 && !e->dm.zclass && !e->dm.is_ideal;
    e->fast = on && can;
    if (in_effect) *in_effect = e->fast ? 1 : 0;
    return 0;
}

extern "C" int qmc_engine_stream(qmc_engine *e, void **stream, int *owned)
{
    if (!e || !stream) return fail("qmc_engine_stream: null argument");
    *stream = (void *)e->stream;
    if (owned) *owned = e->own_stream ? 1 : 0;
    return 0;
}

extern "C" int qmc_engine_profile_begin(qmc_engine *e, int64_t max_launches)
{
    if (!e) return fail("qmc_engine_profile_begin: null engine");
    if (max_launches <= 0 || max_launches > (1 << 20))
        return fail("qmc_engine_profile_begin: max_launches out of range");
    HIP_TRY(hipSetDevice(e->device));
    while (e->prof_ev.size() < (size_t)max_launches * 2) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        e->prof_ev.push_back(ev);
    }
    e->prof_used = 0;
    e->prof_on = true;
    return 0;
}

extern "C" int qmc_engine_profile_end(qmc_engine *e, int64_t *launches,
                                      double *total_ms, double *min_ms,
                                      double *max_ms)
{
    if (!e) return fail("qmc_engine_profile_end: null engine");
    HIP_TRY(hipSetDevice(e->device));
    e->prof_on = false;
    double tot = 0.0, mn = 0.0, mx = 0.0;
    const size_t n = e->prof_used / 2;
    if (n) HIP_TRY(hipEventSynchronize(e->prof_ev[e->prof_used - 1]));
    for (size_t i = 0; i < n; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->prof_ev[2 * i],
                                    e->prof_ev[2 * i + 1]));
        tot += ms;
        if (i == 0 || ms < mn) mn = ms;
        if (i == 0 || ms > mx) mx = ms;
    }
    e->prof_used = 0;
    if (launches) *launches = (int64_t)n;
    if (total_ms) *total_ms = tot;
    if (min_ms) *min_ms = mn;
    if (max_ms) *max_ms = mx;
    return 0;
}

// Diagnostic libraries built with -DQMC_TIMING (tools/section_times.py): cycles
// of wavefront lifetime and visits per kernel section since the last reset,
// summed over every walker kernel launched on this engine.  Section i of the
// first pass of a kernel is qmc_section_name(i); i + nsec / 2 is the same
// section inside the energy pass of the VMC step.  The shipped library has no
// stamps in its kernels and returns an error here.
extern "C" int qmc_engine_section_profile(qmc_engine *e, uint64_t *cycles,
                                          uint64_t *visits, int32_t nsec,
                                          int32_t reset)
{
    if (!e) return fail("qmc_engine_section_profile: null engine");
#if defined(QMC_TIMING)
    if (nsec != QMC_NSEC)
        return fail("qmc_engine_section_profile: nsec must be 32");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::vector<unsigned long long> host((size_t)QMC_SEC_COPIES * 2 * QMC_NSEC);
    const size_t bytes = host.size() * sizeof(unsigned long long);
    HIP_TRY(hipMemcpy(host.data(), e->sec_prof_dev, bytes,
                      hipMemcpyDeviceToHost));
    for (int i = 0; i < QMC_NSEC; ++i) {
        unsigned long long c = 0, v = 0;
        for (int k = 0; k < QMC_SEC_COPIES; ++k) {
            c += host[(size_t)k * 2 * QMC_NSEC + i];
            v += host[(size_t)k * 2 * QMC_NSEC + QMC_NSEC + i];
        }
        if (cycles) cycles[i] = c;
        if (visits) visits[i] = v;
    }
    if (reset) HIP_TRY(hipMemset(e->sec_prof_dev, 0, bytes));
    return 0;
#else
    (void)cycles; (void)visits; (void)nsec; (void)reset;
    return fail("qmc_engine_section_profile: this library was built without "
                "-DQMC_TIMING (see tools/section_times.py)");
#endif
}

// Diagnostic libraries built with -DQMC_CUTS (tools/section_counts.py): from
// now on every wavefront of the walker kernels ends when it reaches section
// mark `section` (-1: never).  The results of such launches are meaningless;
// hardware counters of runs cut at successive marks give the instructions each
// section executes.  The shipped library has no cut tests in its kernels.
extern "C" int qmc_engine_section_cut(qmc_engine *e, int32_t section)
{
    if (!e) return fail("qmc_engine_section_cut: null engine");
#if defined(QMC_CUTS)
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->dm.sec_cut = section;
    HIP_TRY(hipMemcpy(e->dm_dev, &e->dm, sizeof(DevModel),
                      hipMemcpyHostToDevice));
    return 0;
#else
    (void)section;
    return fail("qmc_engine_section_cut: this library was built without "
                "-DQMC_CUTS (see tools/section_counts.py)");
#endif
}

// Diagnostic counters the kernels keep (DevModel::diag); synchronises.
extern "C" int qmc_engine_diag_counters(qmc_engine *e, uint64_t *out,
                                        int32_t n, int32_t reset)
{
    if (!e) return fail("qmc_engine_diag_counters: null engine");
    if (n < 0 || n > QMC_NDIAG)
        return fail("qmc_engine_diag_counters: at most 4 counters");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (out && n > 0)
        HIP_TRY(hipMemcpy(out, e->diag_dev, (size_t)n * sizeof(uint64_t),
                          hipMemcpyDeviceToHost));
    if (reset)
        HIP_TRY(hipMemset(e->diag_dev, 0,
                          QMC_NDIAG * sizeof(unsigned long long)));
    return 0;
}

extern "C" const char *qmc_section_name(int32_t i)
{
    if (i < 0 || i >= QMC_NSEC) return "";
    return QMC_SEC_NAMES[i % (QMC_NSEC / 2)];
}

extern "C" void qmc_engine_destroy(qmc_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    delete e;
}

extern "C" int qmc_engine_sync(qmc_engine *e)
{
    if (!e) return fail("qmc_engine_sync: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int qmc_engine_timer_start(qmc_engine *e)
{
    if (!e) return fail("qmc_engine_timer_start: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    return 0;
}

extern "C" int qmc_engine_timer_stop(qmc_engine *e, float *ms)
{
    if (!e || !ms) return fail("qmc_engine_timer_stop: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipEventSynchronize(e->ev1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return 0;
}

// Diagnostic: one device primitive on host inputs (qmc_probe.h); synchronises.
extern "C" int qmc_engine_probe(qmc_engine *e, int32_t fn, int64_t n,
                                const double *in, double *out)
{
    if (!e) return fail("qmc_engine_probe: null engine");
    int nin = 0, nout = 0;
    qmc_probe_width(fn, nin, nout);
    if (!nin) return fail("qmc_engine_probe: unknown function id");
    if (n < 0 || n > (1ll << 24))
        return fail("qmc_engine_probe: n must be in [0, 2^24]");
    if (n == 0) return 0;
    if (!in || !out) return fail("qmc_engine_probe: null argument");
    const DevModel &d = e->dm;
    const bool table = fn == QMC_PROBE_TRIG_TAB || fn == QMC_PROBE_ONE_BODY_TAB;
    if (fn == QMC_PROBE_TRIG_TAB && !d.trig_table)
        return fail("qmc_engine_probe: this model has no trig row table");
    if (fn == QMC_PROBE_ONE_BODY_TAB && !d.ob_table)
        return fail("qmc_engine_probe: this model has no one-body table");
    if (fn == QMC_PROBE_ONE_BODY && d.is_free)
        return fail("qmc_engine_probe: a free model has no one-body factor");
    for (int64_t i = 0; i < n * nin; ++i) {
        const double x = in[i];
        if (!std::isfinite(x))
            return fail("qmc_engine_probe: non-finite input");
        if (fn == QMC_PROBE_LOG_POS && !(x >= 2.2250738585072014e-308))
            return fail("qmc_engine_probe: log_pos takes positive normal "
                        "numbers");
        if (table && !(fabs(x) < 4.0 * d.L))
            return fail("qmc_engine_probe: table positions must lie in "
                        "(-4 L, 4 L)");
    }
    HIP_TRY(hipSetDevice(e->device));
    DevBuf<double> din, dout;
    if (din.alloc((size_t)n * nin) || dout.alloc((size_t)n * nout)) return 1;
    HIP_TRY(hipMemcpyAsync(din, in, (size_t)n * nin * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(probe_kernel, dim3((unsigned)((n + 63) / 64)),
                       dim3(64), 0, e->stream, e->dm_dev, (int)fn,
                       (long long)n, din, dout, nin, nout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n * nout * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int qmc_evaluate_dev(qmc_engine *e, int64_t nconf,
                                const double *pos, double *wf, double *energy,
                                double *ith, double *drift)
{
    if (!e || !pos) return fail("qmc_evaluate_dev: null argument");
    HIP_TRY(hipSetDevice(e->device));
    EvalArgs a{ pos, wf, energy, ith, drift, (long long)nconf };
    return dispatch_shape<LaunchEval>(e, a);
}

// Plain device buffers (configuration sets kept resident across
// qmc_evaluate_dev calls by callers without a device-memory library).
extern "C" int qmc_buffer_alloc(int device, size_t bytes, void **out)
{
    if (!out || !bytes) return fail("qmc_buffer_alloc: null argument");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out, bytes));
    return 0;
}

extern "C" int qmc_buffer_free(void *buf)
{
    if (buf) HIP_TRY(hipFree(buf));
    return 0;
}

extern "C" int qmc_buffer_upload(void *dst_dev, const void *src_host,
                                 size_t bytes)
{
    if (!dst_dev || !src_host) return fail("qmc_buffer_upload: null argument");
    HIP_TRY(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int qmc_buffer_download(void *dst_host, const void *src_dev,
                                   size_t bytes)
{
    if (!dst_host || !src_dev)
        return fail("qmc_buffer_download: null argument");
    HIP_TRY(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int qmc_evaluate(qmc_engine *e, int64_t nconf, const double *pos,
                            double *wf, double *energy, double *ith,
                            double *drift)
{
    if (!e || !pos) return fail("qmc_evaluate: null argument");
    if (nconf <= 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, W = (size_t)nconf;
    DevBuf<double> dpos, dwf, den, dith, ddr;
    if (dpos.alloc(W * n) || dwf.alloc(W) || den.alloc(W) ||
        dith.alloc(W * n) || ddr.alloc(W * n))
        return 1;
    HIP_TRY(hipMemcpyAsync(dpos, pos, W * n * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    if (qmc_evaluate_dev(e, nconf, dpos, dwf, den, dith, ddr)) return 1;
    if (wf) HIP_TRY(hipMemcpyAsync(wf, dwf, W * sizeof(double),
                                   hipMemcpyDeviceToHost, e->stream));
    if (energy) HIP_TRY(hipMemcpyAsync(energy, den, W * sizeof(double),
                                       hipMemcpyDeviceToHost, e->stream));
    if (ith) HIP_TRY(hipMemcpyAsync(ith, dith, W * n * sizeof(double),
                                    hipMemcpyDeviceToHost, e->stream));
    if (drift) HIP_TRY(hipMemcpyAsync(drift, ddr, W * n * sizeof(double),
                                      hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

// Sort every configuration by position; label[w][lane] = original particle
// index held by the lane (see resort_step in qmc_device.h).
static void sort_rows(const double *pos, size_t W, size_t n,
                      std::vector<double> &sorted,
                      std::vector<unsigned short> &label,
                      const double *extra = nullptr,
                      std::vector<double> *extra_sorted = nullptr,
                      size_t pos_stride = 0, size_t extra_stride = 0)
{
    if (!pos_stride) pos_stride = n;
    if (!extra_stride) extra_stride = n;
    sorted.resize(W * n);
    label.resize(W * n);
    if (extra_sorted) extra_sorted->resize(W * n);
    std::vector<unsigned short> idx(n);
    for (size_t w = 0; w < W; ++w) {
        const double *row = pos + w * pos_stride;
        for (size_t i = 0; i < n; ++i) idx[i] = (unsigned short)i;
        std::stable_sort(idx.begin(), idx.end(),
                         [row](unsigned short a, unsigned short b) {
                             return row[a] < row[b];
                         });
        for (size_t i = 0; i < n; ++i) {
            sorted[w * n + i] = row[idx[i]];
            label[w * n + i] = idx[i];
            if (extra_sorted)
                (*extra_sorted)[w * n + i] = extra[w * extra_stride + idx[i]];
        }
    }
}

// ----------------------------------------------------------------- VMC ----
struct qmc_vmc {
    qmc_engine *eng = nullptr;
    qmc_vmc_params p;
    long long W = 0;
    DevBuf<double> pos, wf, ecarry;
    DevBuf<unsigned short> label;
    DevBuf<double> sum_e, sum_e2;
    DevBuf<long long> n_acc;
    // the per-chain scalars the step kernel reads and writes; wf, ecarry,
    // sum_e, sum_e2 and n_acc above are their copies for the C ABI, refreshed
    // at the end of every run_block
    DevBuf<VmcRec> rec;
    DevBuf<double> tape;
    long long tape_steps = 0, tape_used = 0;
    unsigned int step = 0;
    int yield_initial = 1;
    DevBuf<double> ssf_partial, ssf_out;                 // qmc_vmc_ssf scratch
};

extern "C" int qmc_vmc_create(qmc_engine *e, const qmc_vmc_params *p,
                              qmc_vmc **out)
{
    if (!e || !p || !out) return fail("qmc_vmc_create: null argument");
    if (p->num_chains <= 0) return fail("qmc_vmc_create: num_chains <= 0");
    if (p->gaussian != QMC_VMC_UNIFORM && p->gaussian != QMC_VMC_GAUSSIAN &&
        p->gaussian != QMC_VMC_PARTICLE)
        return fail("qmc_vmc_create: unknown proposal code");
    HIP_TRY(hipSetDevice(e->device));
    std::unique_ptr<qmc_vmc> v(new qmc_vmc());
    v->eng = e;
    v->p = *p;
    v->W = p->num_chains;
    const size_t W = (size_t)v->W, n = (size_t)e->dm.n;
    if (v->pos.alloc(W * n) || v->label.alloc(W * n) || v->wf.alloc(W) ||
        v->ecarry.alloc(W) || v->sum_e.alloc(W) || v->sum_e2.alloc(W) ||
        v->n_acc.alloc(W) || v->rec.alloc(W))
        return 1;
    *out = v.release();
    return 0;
}

extern "C" void qmc_vmc_destroy(qmc_vmc *v)
{
    if (!v) return;
    (void)hipSetDevice(v->eng->device);
    delete v;
}

extern "C" int qmc_vmc_set_state(qmc_vmc *v, const double *pos)
{
    if (!v || !pos) return fail("qmc_vmc_set_state: null argument");
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t W = (size_t)v->W, n = (size_t)e->dm.n;
    std::vector<double> sorted;
    std::vector<unsigned short> label;
    sort_rows(pos, W, n, sorted, label);
    HIP_TRY(hipMemcpyAsync(v->pos, sorted.data(), W * n * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(v->label, label.data(), W * n * sizeof(unsigned short),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(v->ecarry, 0, W * sizeof(double), e->stream));
    int rc = qmc_evaluate_dev(e, v->W, v->pos, v->wf, nullptr, nullptr,
                              nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(vmc_pack_kernel, dim3((unsigned)((W + BLOCK - 1) / BLOCK)),
                       dim3(BLOCK), 0, e->stream, v->rec, v->W, v->wf,
                       v->ecarry);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    v->step = 0;
    v->yield_initial = 1;
    v->tape_used = 0;
    return 0;
}

extern "C" int qmc_vmc_get_state(qmc_vmc *v, double *pos, double *wf,
                                 double *ecarry)
{
    if (!v) return fail("qmc_vmc_get_state: null argument");
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t W = (size_t)v->W, n = (size_t)e->dm.n;
    std::vector<double> lane_pos;
    std::vector<unsigned short> label;
    if (pos) {
        lane_pos.resize(W * n);
        label.resize(W * n);
        HIP_TRY(hipMemcpyAsync(lane_pos.data(), v->pos, W * n * sizeof(double),
                               hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(label.data(), v->label,
                               W * n * sizeof(unsigned short),
                               hipMemcpyDeviceToHost, e->stream));
    }
    if (wf) HIP_TRY(hipMemcpyAsync(wf, v->wf, W * sizeof(double),
                                   hipMemcpyDeviceToHost, e->stream));
    if (ecarry) HIP_TRY(hipMemcpyAsync(ecarry, v->ecarry, W * sizeof(double),
                                       hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (pos)       // back to the caller's particle order
        for (size_t w = 0; w < W; ++w)
            for (size_t i = 0; i < n; ++i)
                pos[w * n + label[w * n + i]] = lane_pos[w * n + i];
    return 0;
}

extern "C" int qmc_vmc_set_tape(qmc_vmc *v, const double *tape, int64_t steps)
{
    if (!v) return fail("qmc_vmc_set_tape: null argument");
    // (the sweep's stream is restated exactly: nothing to replay)
    if (v->p.gaussian == QMC_VMC_PARTICLE)
        return fail("qmc_vmc_set_tape: no tape with single-particle sweeps");
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    v->tape.release();
    v->tape_steps = 0;
    v->tape_used = 0;
    if (!tape || steps <= 0) return 0;
    size_t cnt = (size_t)v->W * (size_t)steps * (size_t)(e->dm.n + 1);
    if (v->tape.alloc(cnt)) return 1;
    HIP_TRY(hipMemcpy(v->tape, tape, cnt * sizeof(double),
                      hipMemcpyHostToDevice));
    v->tape_steps = steps;
    return 0;
}

extern "C" int qmc_vmc_state_dev(qmc_vmc *v, double **pos, double **wf)
{
    if (!v) return fail("qmc_vmc_state_dev: null argument");
    if (pos) *pos = v->pos;
    if (wf) *wf = v->wf;
    return 0;
}

// `count` doubles of a device result to the host, complete on return
static int read_doubles(const qmc_engine *e, double *out, const double *dev,
                        size_t count)
{
    HIP_TRY(hipMemcpyAsync(out, dev, count * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

template <int KD>
static void launch_ssf_kd(const qmc_engine *e, const EstArgs &a)
{
    const size_t lds = (size_t)(BLOCK / 64) * SsfShape<KD>::WAVE_DOUBLES *
                       sizeof(double);
    allow_lds(dmc_ssf_mfma_kernel<KD>, lds);
    hipLaunchKernelGGL(dmc_ssf_mfma_kernel<KD>, dim3(EST_BLOCKS), dim3(BLOCK),
                       lds, e->stream, a);
}

// The one place that launches the matrix-core S(k) kernel: 8 rows of modes
// per pass up to 64 modes, 16 beyond (the caller checks the launch with the
// reduction that follows).
static void launch_ssf(const qmc_engine *e, const EstArgs &a)
{
    if (a.K <= 64) launch_ssf_kd<8>(e, a);
    else launch_ssf_kd<16>(e, a);
}

// Static structure factor parts of the current configurations, summed over
// the chains: out[m] = sum_w (|rho_m|^2, Re rho_m, Im rho_m), m < num_modes
// (qmc_base/jastrow/vmc.py:304-351 evaluates them per step of one chain; an
// ensemble gets them in one launch of the matrix-core kernel).
extern "C" int qmc_vmc_ssf(qmc_vmc *v, int32_t num_modes, double *out)
{
    if (!v || !out) return fail("qmc_vmc_ssf: null argument");
    if (num_modes <= 0 || num_modes > EST_MAXK)
        return fail("qmc_vmc_ssf: num_modes must be in [1, 256]");
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const int M = num_modes;
    if (v->ssf_partial.reserve((size_t)EST_BLOCKS * M * 3) ||
        v->ssf_out.reserve((size_t)M * 3))
        return 1;
    EstArgs a;
    a.ppos = v->pos; a.ref = nullptr; a.ctl = nullptr;
    a.aux_prev = nullptr; a.aux_act = nullptr; a.partial = v->ssf_partial;
    a.maxw = v->W; a.step_idx = 0; a.pfw = 0; a.n = e->dm.n; a.K = M;
    a.pure = 0; a.scale = 4.0 / e->dm.L; a.scale2 = 0.0;
    launch_ssf(e, a);
    hipLaunchKernelGGL(est_reduce_kernel, dim3((M * 3 + 31) / 32), dim3(256), 0,
                       e->stream, v->ssf_partial, EST_BLOCKS, M * 3, 1.0,
                       v->ssf_out);
    HIP_TRY(hipGetLastError());
    return read_doubles(e, out, v->ssf_out, (size_t)M * 3);
}

// ---- batch estimators: what g1(s) and g2(r) share ------------------------
// lane-group width of the kernels for n particles
static int est_width(int n)
{
    return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64;
}

// launch(std::integral_constant<int, G>, c0, nc) for the run-time width G over
// nconf configurations, at most `xmax` to a launch (a grid's first dimension
// holds 2^31 - 1 blocks)
template <typename F>
static int launch_width_chunks(int G, long long nconf, long long xmax, F launch)
{
    for (long long c0 = 0; c0 < nconf; c0 += xmax) {
        const long long nc = std::min(xmax, nconf - c0);
        switch (G) {
        case 8: launch(std::integral_constant<int, 8>{}, c0, nc); break;
        case 16: launch(std::integral_constant<int, 16>{}, c0, nc); break;
        case 32: launch(std::integral_constant<int, 32>{}, c0, nc); break;
        default: launch(std::integral_constant<int, 64>{}, c0, nc); break;
        }
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// sums[K][2] and wsum over nconf configurations, `tile` at a time:
// fill(c0, nc) leaves rows[nc][K] of the tile from c0 on the stream and
// obdm_reduce_kernel adds them up in tile order, into sums and wsum from the
// second tile on.  (No configurations: one reduction of an empty tile, which
// zeroes sums.)
template <typename F>
static int reduce_tiles(const qmc_engine *e, long long nconf, long long tile,
                        const double *rows, const double *w, int K,
                        double *sums, double *wsum, F fill)
{
    long long c0 = 0;
    do {
        const long long nc = std::min(tile, nconf - c0);
        if (fill(c0, nc)) return 1;
        hipLaunchKernelGGL(obdm_reduce_kernel, dim3(K + 1), dim3(256), 0,
                           e->stream, rows, w ? w + c0 : nullptr, nc, K,
                           c0 > 0 ? 1 : 0, sums, wsum);
        HIP_TRY(hipGetLastError());
        c0 += tile;
    } while (c0 < nconf);
    return 0;
}

// A per-configuration output of a host entry point: `bytes` per configuration
// from the device tile `dev` to `host` (null: not asked for).
struct HostOut {
    void *host;
    const void *dev;
    size_t bytes;
};

// Host positions pos[nconf][n] through the device, `tile` configurations at a
// time: upload to dpos, launch(nc), download the outputs, wait.
template <typename F>
static int run_host_tiles(const qmc_engine *e, long long nconf, long long tile,
                          const double *pos, double *dpos,
                          std::initializer_list<HostOut> outs, F launch)
{
    const size_t n = (size_t)e->dm.n;
    for (long long c0 = 0; c0 < nconf; c0 += tile) {
        const size_t nc = (size_t)std::min(tile, nconf - c0);
        HIP_TRY(hipMemcpyAsync(dpos, pos + (size_t)c0 * n,
                               nc * n * sizeof(double),
                               hipMemcpyHostToDevice, e->stream));
        if (launch((long long)nc)) return 1;
        for (const HostOut &o : outs)
            if (o.host)
                HIP_TRY(hipMemcpyAsync((char *)o.host + (size_t)c0 * o.bytes,
                                       o.dev, nc * o.bytes,
                                       hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    return 0;
}

// ---- one-body density matrix (csrc/qmc_obdm.h) --------------------------
// Configurations per launch where the entry point owns the [nconf][nshift]
// scratch: 2^16 configurations of 64 shifts are 32 MB (2^20 chains at once
// would be 512 MB); tiles run one after the other on the stream and the
// reduction adds them up in tile order.
static constexpr long long OBDM_TILE = 1ll << 16;
// Doubles of per-configuration output (g1 and, when asked for, ith) that
// qmc_obdm keeps on the device at a time (128 MB).
static constexpr long long OBDM_HOST_TILE_DOUBLES = 1ll << 24;

// rows [nshift][OBDM_SROW] of a set of device-resident shifts, on the
// engine's stream
static int obdm_fill_shift_table(const qmc_engine *e, int32_t nshift,
                                 const double *shifts_dev, double *stab_dev)
{
    hipLaunchKernelGGL(obdm_shift_kernel, dim3((nshift + 63) / 64), dim3(64),
                       0, e->stream, e->dm_dev, shifts_dev, (int)nshift,
                       stab_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the engine's shift table (every qmc_obdm* call rewrites it)
static int obdm_make_shift_table(qmc_engine *e, int32_t nshift,
                                 const double *shifts_dev)
{
    if (e->obdm_stab.reserve((size_t)nshift * OBDM_SROW)) return 1;
    return obdm_fill_shift_table(e, nshift, shifts_dev, e->obdm_stab);
}

// g1 (and ith) of nconf configurations against the engine's shift table
static int obdm_launch(qmc_engine *e, long long nconf, const double *pos_dev,
                       int32_t nshift, double *g1_dev, double *ith_dev)
{
    if (nconf <= 0) return 0;
    const int n = e->dm.n, G = est_width(n);
    const int unit = (64 / G) * OBDM_U;       // shifts of one wavefront pass
    // shifts per wavefront: all of them once the batch alone fills the chip
    // (the unshifted rows are computed once per wavefront), fewer for a small
    // batch; the grid's second dimension holds at most 65535 chunks
    long long chunks = std::max(1ll, std::min<long long>(
        (nshift + unit - 1) / unit, 8192 / nconf));
    int chunk = (int)((nshift + chunks - 1) / chunks);
    chunk = ((chunk + unit - 1) / unit) * unit;
    chunk = std::max(chunk, (nshift + 65534) / 65535);
    const unsigned ny = (unsigned)((nshift + chunk - 1) / chunk);
    const size_t lds = (size_t)n * OBDM_LDS_PER_PARTICLE * sizeof(double);
    return launch_width_chunks(G, nconf, 1ll << 30, [&](auto g, long long c0,
                                                         long long nc) {
        ObdmArgs a{ pos_dev + (size_t)c0 * n, e->obdm_stab,
                    g1_dev + (size_t)c0 * nshift,
                    ith_dev ? ith_dev + (size_t)c0 * nshift * n : nullptr, nc,
                    (int)nshift, chunk };
        hipLaunchKernelGGL(obdm_kernel<decltype(g)::value>,
                           dim3((unsigned)nc, ny), dim3(64), lds, e->stream,
                           e->dm_dev, a);
    });
}

extern "C" int qmc_obdm_dev(qmc_engine *e, int64_t nconf, const double *pos,
                            int32_t nshift, const double *shifts, double *g1,
                            double *ith)
{
    if (!e || !pos || !shifts || !g1)
        return fail("qmc_obdm_dev: null argument");
    if (nshift < 1) return fail("qmc_obdm_dev: nshift < 1");
    if (nconf < 0) return fail("qmc_obdm_dev: nconf < 0");
    HIP_TRY(hipSetDevice(e->device));
    if (obdm_make_shift_table(e, nshift, shifts)) return 1;
    return obdm_launch(e, nconf, pos, nshift, g1, ith);
}

extern "C" int qmc_obdm_reduce_dev(qmc_engine *e, int64_t nconf,
                                   const double *pos, const double *w,
                                   int32_t nshift, const double *shifts,
                                   double *sums, double *wsum)
{
    if (!e || !pos || !shifts || !sums)
        return fail("qmc_obdm_reduce_dev: null argument");
    if (nshift < 1) return fail("qmc_obdm_reduce_dev: nshift < 1");
    if (nconf < 0) return fail("qmc_obdm_reduce_dev: nconf < 0");
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    const long long tile = std::min<long long>(std::max<long long>(nconf, 1),
                                               OBDM_TILE);
    if (obdm_make_shift_table(e, nshift, shifts) ||
        e->obdm_g1.reserve((size_t)tile * nshift))
        return 1;
    return reduce_tiles(e, nconf, tile, e->obdm_g1, w, nshift, sums, wsum,
                        [&](long long c0, long long nc) {
        return obdm_launch(e, nc, pos + (size_t)c0 * n, nshift, e->obdm_g1,
                           nullptr);
    });
}

static int obdm_check_host_shifts(const char *who, int32_t nshift,
                                  const double *shifts)
{
    if (nshift < 1) return fail(std::string(who) + ": nshift < 1");
    if (!shifts) return fail(std::string(who) + ": null argument");
    for (int32_t k = 0; k < nshift; ++k)
        if (!std::isfinite(shifts[k]))
            return fail(std::string(who) + ": shift " + std::to_string(k) +
                        " is not finite");
    return 0;
}

extern "C" int qmc_obdm(qmc_engine *e, int64_t nconf, const double *pos,
                        int32_t nshift, const double *shifts, double *g1,
                        double *ith)
{
    if (!e || !pos || !g1) return fail("qmc_obdm: null argument");
    if (obdm_check_host_shifts("qmc_obdm", nshift, shifts)) return 1;
    if (nconf < 0) return fail("qmc_obdm: nconf < 0");
    if (nconf == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, M = (size_t)nshift;
    const size_t per_conf = M * (ith ? n + 1 : 1);
    const long long tile = std::max<long long>(
        1, std::min<long long>(nconf, OBDM_HOST_TILE_DOUBLES / (long long)per_conf));
    DevBuf<double> dsh, dpos, dg1, dith;
    if (dsh.alloc(M) || dpos.alloc((size_t)tile * n) ||
        dg1.alloc((size_t)tile * M) || (ith && dith.alloc((size_t)tile * M * n)))
        return 1;
    HIP_TRY(hipMemcpyAsync(dsh, shifts, M * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    if (obdm_make_shift_table(e, nshift, dsh)) return 1;
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { g1, dg1.get(), M * sizeof(double) },
                            { ith, dith.get(), M * n * sizeof(double) } },
                          [&](long long nc) {
        return obdm_launch(e, nc, dpos, nshift, dg1, dith);
    });
}

// g1 parts of the CURRENT configurations of the chains, summed over the
// chains: the resident, position-sorted rows go to the kernel as they are (g1
// is symmetric in the particles).
extern "C" int qmc_vmc_obdm(qmc_vmc *v, int32_t nshift, const double *shifts,
                            double *out)
{
    if (!v || !out) return fail("qmc_vmc_obdm: null argument");
    if (obdm_check_host_shifts("qmc_vmc_obdm", nshift, shifts)) return 1;
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t M = (size_t)nshift;
    if (e->obdm_sums.reserve(3 * M)) return 1;
    double *dsh = e->obdm_sums + 2 * M;
    HIP_TRY(hipMemcpyAsync(dsh, shifts, M * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    int rc = qmc_obdm_reduce_dev(e, v->W, v->pos, nullptr, nshift, dsh,
                                 e->obdm_sums, nullptr);
    return rc ? rc : read_doubles(e, out, e->obdm_sums, 2 * M);
}

// ---- pair distribution g2(r) (csrc/qmc_pairdist.h) ----------------------
// Configurations per launch of the reduction (as OBDM_TILE), fewer where the
// tile of histograms would exceed PD_SCRATCH_ELEMS doubles (128 MB): 2^16 up to
// 256 bins, 2^12 at 4096.  The same count of 32-bit counters bounds what
// qmc_pair_dist keeps on the device at a time.
static constexpr long long PD_TILE = 1ll << 16;
static constexpr long long PD_SCRATCH_ELEMS = 1ll << 24;

static int pair_dist_check(const char *who, int64_t nconf, int32_t num_bins)
{
    if (num_bins < 1 || num_bins > PD_MAX_BINS)
        return fail(std::string(who) + ": num_bins outside [1, " +
                    std::to_string(PD_MAX_BINS) + "]");
    if (nconf < 0) return fail(std::string(who) + ": nconf < 0");
    return 0;
}

// histograms of nconf device-resident configurations -> out[nconf][B]
template <typename OutT>
static int pair_dist_launch(qmc_engine *e, long long nconf,
                            const double *pos_dev, int32_t B, OutT *out)
{
    if (nconf <= 0) return 0;
    const int n = e->dm.n;
    int G = est_width(n);
    const size_t per_conf = (size_t)n * sizeof(double) + (size_t)B * sizeof(unsigned);
    while (G < 64 && (64 / G) * per_conf > PD_LDS_BUDGET) G *= 2;
    const int gpw = 64 / G;
    const size_t lds = gpw * per_conf;
    const double L = e->dm.L, half = 0.5 * L;
    return launch_width_chunks(G, nconf, (1ll << 30) * gpw,
                               [&](auto g, long long c0, long long nc) {
        PairDistArgs a{ pos_dev + (size_t)c0 * n, out + (size_t)c0 * B, nc, n,
                        (int)B, L, half, (double)B / half };
        hipLaunchKernelGGL((pair_dist_kernel<decltype(g)::value, OutT>),
                           dim3((unsigned)((nc + gpw - 1) / gpw)), dim3(64),
                           lds, e->stream, a);
    });
}

extern "C" int qmc_pair_dist_dev(qmc_engine *e, int64_t nconf,
                                 const double *pos, int32_t num_bins,
                                 uint32_t *counts)
{
    if (!e || !pos || !counts)
        return fail("qmc_pair_dist_dev: null argument");
    if (pair_dist_check("qmc_pair_dist_dev", nconf, num_bins)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return pair_dist_launch(e, nconf, pos, num_bins, counts);
}

extern "C" int qmc_pair_dist_reduce_dev(qmc_engine *e, int64_t nconf,
                                        const double *pos, const double *w,
                                        int32_t num_bins, double *sums,
                                        double *wsum)
{
    if (!e || !pos || !sums)
        return fail("qmc_pair_dist_reduce_dev: null argument");
    if (pair_dist_check("qmc_pair_dist_reduce_dev", nconf, num_bins)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    const long long tile = std::min<long long>(
        std::max<long long>(nconf, 1),
        std::min(PD_TILE, PD_SCRATCH_ELEMS / num_bins));
    if (e->pd_hist.reserve((size_t)tile * num_bins)) return 1;
    return reduce_tiles(e, nconf, tile, e->pd_hist, w, num_bins, sums, wsum,
                        [&](long long c0, long long nc) {
        return pair_dist_launch(e, nc, pos + (size_t)c0 * n, num_bins,
                                e->pd_hist.get());
    });
}

extern "C" int qmc_pair_dist(qmc_engine *e, int64_t nconf, const double *pos,
                             int32_t num_bins, uint32_t *counts)
{
    if (!e || !pos || !counts) return fail("qmc_pair_dist: null argument");
    if (pair_dist_check("qmc_pair_dist", nconf, num_bins)) return 1;
    if (nconf == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, B = (size_t)num_bins;
    const long long tile = std::max<long long>(
        1, std::min<long long>(nconf, PD_SCRATCH_ELEMS / (long long)std::max(n, B)));
    DevBuf<double> dpos;
    DevBuf<uint32_t> dcnt;
    if (dpos.alloc((size_t)tile * n) || dcnt.alloc((size_t)tile * B)) return 1;
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { counts, dcnt.get(), B * sizeof(uint32_t) } },
                          [&](long long nc) {
        return pair_dist_launch(e, nc, dpos, num_bins, dcnt.get());
    });
}

// Histogram sums of the CURRENT configurations of the chains: the resident
// rows go to the kernel as they are (the particle order is irrelevant); the
// chain state is only read.
extern "C" int qmc_vmc_pair_dist(qmc_vmc *v, int32_t num_bins, double *out)
{
    if (!v || !out) return fail("qmc_vmc_pair_dist: null argument");
    if (pair_dist_check("qmc_vmc_pair_dist", 0, num_bins)) return 1;
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t B = (size_t)num_bins;
    if (e->pd_sums.reserve(2 * B)) return 1;
    int rc = qmc_pair_dist_reduce_dev(e, v->W, v->pos, nullptr, num_bins,
                                      e->pd_sums, nullptr);
    return rc ? rc : read_doubles(e, out, e->pd_sums, 2 * B);
}

// ---- three-body distribution g3(d) (csrc/qmc_tripledist.h) ---------------
// Tiles as for g2 (PD_TILE, PD_SCRATCH_ELEMS), on rows of num_bins + 1.
static int triple_dist_check(const char *who, const qmc_engine *e,
                             int64_t nconf, int32_t num_bins, double max_span)
{
    if (num_bins < 1 || num_bins > TD_MAX_BINS)
        return fail(std::string(who) + ": num_bins outside [1, " +
                    std::to_string(TD_MAX_BINS) + "]");
    if (!(max_span > 0.0) || !(max_span <= 0.5 * e->dm.L))
        return fail(std::string(who) + ": max_span outside (0, L/2]");
    if (nconf < 0) return fail(std::string(who) + ": nconf < 0");
    return 0;
}

// histograms of nconf device-resident configurations -> out[nconf][B + 1]
template <typename OutT>
static int triple_dist_launch(qmc_engine *e, long long nconf,
                              const double *pos_dev, int32_t B, double max_span,
                              OutT *out)
{
    if (nconf <= 0) return 0;
    const int n = e->dm.n;
    int G = est_width(n);
    const size_t per_conf = td_lds_per_conf(n, B);
    while (G < 64 && (64 / G) * per_conf > TD_LDS_BUDGET) G *= 2;
    const int gpw = 64 / G;
    const size_t lds = gpw * per_conf;
    const unsigned ntriples =
        (unsigned)((long long)n * (n - 1) * (n - 2) / 6);
    return launch_width_chunks(G, nconf, (1ll << 30) * gpw,
                               [&](auto g, long long c0, long long nc) {
        TripleDistArgs a{ pos_dev + (size_t)c0 * n,
                          out + (size_t)c0 * (B + 1), nc, n, (int)B, ntriples,
                          e->dm.L, max_span, (double)B / max_span };
        hipLaunchKernelGGL((triple_dist_kernel<decltype(g)::value, OutT>),
                           dim3((unsigned)((nc + gpw - 1) / gpw)), dim3(64),
                           lds, e->stream, a);
    });
}

extern "C" int qmc_triple_dist_dev(qmc_engine *e, int64_t nconf,
                                   const double *pos, int32_t num_bins,
                                   double max_span, uint32_t *counts)
{
    if (!e || !pos || !counts)
        return fail("qmc_triple_dist_dev: null argument");
    if (triple_dist_check("qmc_triple_dist_dev", e, nconf, num_bins, max_span))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    return triple_dist_launch(e, nconf, pos, num_bins, max_span, counts);
}

extern "C" int qmc_triple_dist_reduce_dev(qmc_engine *e, int64_t nconf,
                                          const double *pos, const double *w,
                                          int32_t num_bins, double max_span,
                                          double *sums, double *wsum)
{
    if (!e || !pos || !sums)
        return fail("qmc_triple_dist_reduce_dev: null argument");
    if (triple_dist_check("qmc_triple_dist_reduce_dev", e, nconf, num_bins,
                          max_span))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    const int K = num_bins + 1;
    const long long tile = std::min<long long>(
        std::max<long long>(nconf, 1),
        std::min(PD_TILE, PD_SCRATCH_ELEMS / K));
    if (e->td_hist.reserve((size_t)tile * K)) return 1;
    return reduce_tiles(e, nconf, tile, e->td_hist, w, K, sums, wsum,
                        [&](long long c0, long long nc) {
        return triple_dist_launch(e, nc, pos + (size_t)c0 * n, num_bins,
                                  max_span, e->td_hist.get());
    });
}

extern "C" int qmc_triple_dist(qmc_engine *e, int64_t nconf, const double *pos,
                               int32_t num_bins, double max_span,
                               uint32_t *counts)
{
    if (!e || !pos || !counts) return fail("qmc_triple_dist: null argument");
    if (triple_dist_check("qmc_triple_dist", e, nconf, num_bins, max_span))
        return 1;
    if (nconf == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, K = (size_t)num_bins + 1;
    const long long tile = std::max<long long>(
        1, std::min<long long>(nconf, PD_SCRATCH_ELEMS / (long long)std::max(n, K)));
    DevBuf<double> dpos;
    DevBuf<uint32_t> dcnt;
    if (dpos.alloc((size_t)tile * n) || dcnt.alloc((size_t)tile * K)) return 1;
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { counts, dcnt.get(), K * sizeof(uint32_t) } },
                          [&](long long nc) {
        return triple_dist_launch(e, nc, dpos, num_bins, max_span, dcnt.get());
    });
}

// Histogram sums of the CURRENT configurations of the chains, on the resident
// rows (the kernel orders every row itself, so neither the position order of
// the 'all' rows nor the label order of the 'particle' rows matters); the
// chain state is only read.
extern "C" int qmc_vmc_triple_dist(qmc_vmc *v, int32_t num_bins,
                                   double max_span, double *out)
{
    if (!v || !out) return fail("qmc_vmc_triple_dist: null argument");
    qmc_engine *e = v->eng;
    if (triple_dist_check("qmc_vmc_triple_dist", e, 0, num_bins, max_span))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t K = (size_t)num_bins + 1;
    if (e->td_sums.reserve(2 * K)) return 1;
    int rc = qmc_triple_dist_reduce_dev(e, v->W, v->pos, nullptr, num_bins,
                                        max_span, e->td_sums, nullptr);
    return rc ? rc : read_doubles(e, out, e->td_sums, 2 * K);
}


// ---- energy parts and the windowed contact (csrc/qmc_energy_parts.h) -----
// The windows are a host array in every entry point: they travel in the
// kernel's argument block.  Tiles as for g2 (PD_TILE, PD_SCRATCH_ELEMS), on
// rows of EP_COLS + nrange.
static int energy_parts_args(const char *who, const qmc_engine *e,
                             int64_t nconf, int32_t nrange,
                             const double *ranges, EnergyPartsArgs &a)
{
    if (nrange < 0 || nrange > EP_MAX_RANGES)
        return fail(std::string(who) + ": nrange outside [0, " +
                    std::to_string(EP_MAX_RANGES) + "]");
    if (nrange > 0 && !ranges)
        return fail(std::string(who) + ": null argument");
    if (nconf < 0) return fail(std::string(who) + ": nconf < 0");
    memset(&a, 0, sizeof(a));
    a.K = nrange;
    for (int k = 0; k < nrange; ++k) {
        const double r = ranges[k];
        if (!std::isfinite(r) || !(r > 0.0) || !(r <= 0.5 * e->dm.L))
            return fail(std::string(who) + ": range outside (0, L/2]");
        // (the cosine form of the pair factor holds inside the cutoff only)
        if (!e->dm.is_ideal && !(r <= e->dm.rm))
            return fail(std::string(who) +
                        ": range beyond |tbf_contact_cutoff|");
        a.r[k] = r;
        a.rmax = std::max(a.rmax, r);
    }
    return 0;
}

template <int G, int P, bool PAD, bool ZC>
struct LaunchEnergyParts {
    static int run(const qmc_engine *e, const EnergyPartsArgs &a)
    {
        return launch_walkers<G>(e, energy_parts_kernel<G, P, PAD, ZC>,
                                 lds_bytes<G, P, ZC>(), a.nconf, a);
    }
};

// rows of nconf device-resident configurations -> parts[nconf][EP_COLS + K],
// at most 2^24 configurations to a launch (a multiple of the runs of
// walker_of_block)
static int energy_parts_launch(const qmc_engine *e, EnergyPartsArgs a,
                               long long nconf, const double *pos_dev,
                               double *parts_dev)
{
    const size_t n = (size_t)e->dm.n, cols = (size_t)(EP_COLS + a.K);
    const long long chunk = 1ll << 24;
    for (long long c0 = 0; c0 < nconf; c0 += chunk) {
        a.pos = pos_dev + (size_t)c0 * n;
        a.parts = parts_dev + (size_t)c0 * cols;
        a.nconf = std::min(chunk, nconf - c0);
        if (dispatch_shape<LaunchEnergyParts>(e, a)) return 1;
    }
    return 0;
}

extern "C" int qmc_energy_parts_dev(qmc_engine *e, int64_t nconf,
                                    const double *pos, int32_t nrange,
                                    const double *ranges, double *parts)
{
    if (!e || !pos || !parts)
        return fail("qmc_energy_parts_dev: null argument");
    EnergyPartsArgs a;
    if (energy_parts_args("qmc_energy_parts_dev", e, nconf, nrange, ranges, a))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    return energy_parts_launch(e, a, nconf, pos, parts);
}

extern "C" int qmc_energy_parts_reduce_dev(qmc_engine *e, int64_t nconf,
                                           const double *pos, const double *w,
                                           int32_t nrange, const double *ranges,
                                           double *sums, double *wsum)
{
    if (!e || !pos || !sums)
        return fail("qmc_energy_parts_reduce_dev: null argument");
    EnergyPartsArgs a;
    if (energy_parts_args("qmc_energy_parts_reduce_dev", e, nconf, nrange,
                          ranges, a))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    const int cols = EP_COLS + nrange;
    const long long tile = std::min<long long>(
        std::max<long long>(nconf, 1),
        std::min(PD_TILE, PD_SCRATCH_ELEMS / cols));
    if (e->ep_rows.reserve((size_t)tile * cols)) return 1;
    return reduce_tiles(e, nconf, tile, e->ep_rows, w, cols, sums, wsum,
                        [&](long long c0, long long nc) {
        return energy_parts_launch(e, a, nc, pos + (size_t)c0 * n,
                                   e->ep_rows.get());
    });
}

extern "C" int qmc_energy_parts(qmc_engine *e, int64_t nconf, const double *pos,
                                int32_t nrange, const double *ranges,
                                double *parts)
{
    if (!e || !pos || !parts) return fail("qmc_energy_parts: null argument");
    EnergyPartsArgs a;
    if (energy_parts_args("qmc_energy_parts", e, nconf, nrange, ranges, a))
        return 1;
    if (nconf == 0) return 0;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, cols = (size_t)(EP_COLS + nrange);
    const long long tile = std::max<long long>(
        1, std::min<long long>(nconf,
                               PD_SCRATCH_ELEMS / (long long)std::max(n, cols)));
    DevBuf<double> dpos, drows;
    if (dpos.alloc((size_t)tile * n) || drows.alloc((size_t)tile * cols))
        return 1;
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { parts, drows.get(), cols * sizeof(double) } },
                          [&](long long nc) {
        return energy_parts_launch(e, a, nc, dpos, drows.get());
    });
}

// Sums of the rows of the CURRENT configurations of the chains, on the
// resident rows (every column is a sum over particles or over pairs, so
// neither the position order of the 'all' rows nor the label order of the
// 'particle' rows matters); the chain state is only read.
extern "C" int qmc_vmc_energy_parts(qmc_vmc *v, int32_t nrange,
                                    const double *ranges, double *out)
{
    if (!v || !out) return fail("qmc_vmc_energy_parts: null argument");
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t cols = (size_t)EP_COLS + (size_t)std::max(nrange, 0);
    if (e->ep_sums.reserve(2 * cols)) return 1;
    int rc = qmc_energy_parts_reduce_dev(e, v->W, v->pos, nullptr, nrange,
                                         ranges, e->ep_sums, nullptr);
    return rc ? rc : read_doubles(e, out, e->ep_sums, 2 * cols);
}

// ---- Renyi-2 replica swap (csrc/qmc_renyi.h) -----------------------------
// Tiles as for g2 (PD_TILE, PD_SCRATCH_ELEMS), on rows of 2 nlen per pair.
static int renyi_check(const char *who, int64_t nconf, int32_t nlen,
                       double origin, const char *what = "nlen")
{
    if (nlen < 1 || nlen > RENYI_MAX_LEN)
        return fail(std::string(who) + ": " + what + " outside [1, " +
                    std::to_string(RENYI_MAX_LEN) + "]");
    if (nconf <= 0 || (nconf & 1))
        return fail(std::string(who) +
                    ": nconf must be positive and even (replica pairs)");
    if (!std::isfinite(origin))
        return fail(std::string(who) + ": origin is not finite");
    return 0;
}

static int renyi_check_host_lengths(const char *who, const qmc_engine *e,
                                    int32_t nlen, const double *lengths)
{
    for (int32_t k = 0; k < nlen; ++k)
        if (!std::isfinite(lengths[k]) || !(lengths[k] > 0.0) ||
            !(lengths[k] < e->dm.L))
            return fail(std::string(who) + ": length " + std::to_string(k) +
                        " outside (0, L)");
    return 0;
}

// npair device-resident replica pairs -> n_a, log_ratio and / or rows
static int renyi_launch(qmc_engine *e, long long npair, const double *pos_dev,
                        int32_t K, const double *lengths_dev, double origin,
                        int32_t *n_a, double *log_ratio, double *rows)
{
    const size_t n2 = 2 * (size_t)e->dm.n;
    const size_t lds = renyi_lds_bytes(e->dm.n, K);
    if (lds > RENYI_LDS_LIMIT)
        return fail("qmc_renyi_swap: boson_number too large for the LDS of a "
                    "workgroup");
    allow_lds(renyi_swap_kernel, lds);      // 56 KB at N = 512, K = 4096
    const long long xmax = 1ll << 30;
    for (long long p0 = 0; p0 < npair; p0 += xmax) {
        const long long np = std::min(xmax, npair - p0);
        RenyiArgs a{ pos_dev + (size_t)p0 * n2, lengths_dev,
                     n_a ? n_a + (size_t)p0 * 2 * K : nullptr,
                     log_ratio ? log_ratio + (size_t)p0 * K : nullptr,
                     rows ? rows + (size_t)p0 * 2 * K : nullptr, np, (int)K,
                     origin };
        hipLaunchKernelGGL(renyi_swap_kernel, dim3((unsigned)np), dim3(64),
                           lds, e->stream, e->dm_dev, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int qmc_renyi_swap_dev(qmc_engine *e, int64_t nconf,
                                  const double *pos, int32_t nlen,
                                  const double *lengths, double origin,
                                  int32_t *n_a, double *log_ratio)
{
    if (!e || !pos || !lengths || (!n_a && !log_ratio))
        return fail("qmc_renyi_swap_dev: null argument");
    if (renyi_check("qmc_renyi_swap_dev", nconf, nlen, origin)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return renyi_launch(e, nconf / 2, pos, nlen, lengths, origin, n_a,
                        log_ratio, nullptr);
}

extern "C" int qmc_renyi_swap_reduce_dev(qmc_engine *e, int64_t nconf,
                                         const double *pos, int32_t nlen,
                                         const double *lengths, double origin,
                                         double *sums)
{
    if (!e || !pos || !lengths || !sums)
        return fail("qmc_renyi_swap_reduce_dev: null argument");
    if (renyi_check("qmc_renyi_swap_reduce_dev", nconf, nlen, origin))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n2 = 2 * (size_t)e->dm.n;
    const int C = 2 * nlen;                     // columns of a pair's row
    const long long npair = nconf / 2;
    const long long tile = std::min<long long>(
        npair, std::min(PD_TILE, PD_SCRATCH_ELEMS / C));
    if (e->ry_rows.reserve((size_t)tile * C) ||
        e->ry_colsum.reserve((size_t)2 * C))
        return 1;
    if (reduce_tiles(e, npair, tile, e->ry_rows, nullptr, C, e->ry_colsum,
                     nullptr, [&](long long p0, long long np) {
            return renyi_launch(e, np, pos + (size_t)p0 * n2, nlen, lengths,
                                origin, nullptr, nullptr, e->ry_rows.get());
        }))
        return 1;
    hipLaunchKernelGGL(renyi_pack_kernel, dim3((nlen + 63) / 64), dim3(64), 0,
                       e->stream, e->ry_colsum.get(), (int)nlen, sums);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int qmc_renyi_swap(qmc_engine *e, int64_t nconf, const double *pos,
                              int32_t nlen, const double *lengths,
                              double origin, int32_t *n_a, double *log_ratio)
{
    if (!e || !pos || !lengths || (!n_a && !log_ratio))
        return fail("qmc_renyi_swap: null argument");
    if (renyi_check("qmc_renyi_swap", nconf, nlen, origin) ||
        renyi_check_host_lengths("qmc_renyi_swap", e, nlen, lengths))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, K = (size_t)nlen;
    // an even number of configurations to a tile: whole pairs
    const long long tile = std::max<long long>(
        2, std::min<long long>(
               nconf, PD_SCRATCH_ELEMS / (long long)std::max(n, K)) & ~1ll);
    DevBuf<double> dlen, dpos, dlr;
    DevBuf<int32_t> dna;
    if (dlen.alloc(K) || dpos.alloc((size_t)tile * n) ||
        (n_a && dna.alloc((size_t)tile * K)) ||
        (log_ratio && dlr.alloc((size_t)(tile / 2) * K)))
        return 1;
    HIP_TRY(hipMemcpyAsync(dlen, lengths, K * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    // log_ratio has a row per pair: half a row per configuration
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { n_a, dna.get(), K * sizeof(int32_t) },
                            { log_ratio, dlr.get(), K * sizeof(double) / 2 } },
                          [&](long long nc) {
        return renyi_launch(e, nc / 2, dpos, nlen, dlen, origin, dna.get(),
                            dlr.get(), nullptr);
    });
}

// Swap sums of the CURRENT configurations of the chains, chains 2p and 2p + 1
// the replicas of pair p, on the resident rows (the estimator is symmetric in
// the particles of a row, so neither the position order of the 'all' rows nor
// the label order of the 'particle' rows matters); the chain state is only
// read.
extern "C" int qmc_vmc_renyi_swap(qmc_vmc *v, int32_t nlen,
                                  const double *lengths, double origin,
                                  double *out)
{
    if (!v || !lengths || !out)
        return fail("qmc_vmc_renyi_swap: null argument");
    qmc_engine *e = v->eng;
    if (v->W & 1)
        return fail("qmc_vmc_renyi_swap: an odd number of chains has no "
                    "replica pairs");
    if (renyi_check("qmc_vmc_renyi_swap", v->W, nlen, origin) ||
        renyi_check_host_lengths("qmc_vmc_renyi_swap", e, nlen, lengths))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t K = (size_t)nlen;
    if (e->ry_vmc.reserve(4 * K)) return 1;
    double *dlen = e->ry_vmc + 3 * K;
    HIP_TRY(hipMemcpyAsync(dlen, lengths, K * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    int rc = qmc_renyi_swap_reduce_dev(e, v->W, v->pos, nlen, dlen, origin,
                                       e->ry_vmc);
    return rc ? rc : read_doubles(e, out, e->ry_vmc, 3 * K);
}

// ---- Renyi-2 replica swap of two-segment regions (csrc/qmc_renyi_region.h) --
// Tiles as for g2 (PD_TILE, PD_SCRATCH_ELEMS), on rows of 2 nreg per pair.
static int region_check_host_regions(const char *who, const qmc_engine *e,
                                     int32_t nreg, const double *regions)
{
    for (int32_t k = 0; k < nreg; ++k) {
        const double l1 = regions[3 * k], g = regions[3 * k + 1];
        const double l2 = regions[3 * k + 2];
        const double m1 = l1 + g, m2 = m1 + l2;     // as the kernel forms them
        if (!std::isfinite(l1) || !std::isfinite(g) || !std::isfinite(l2) ||
            !(l1 > 0.0) || !(g >= 0.0) || !(l2 >= 0.0) || !(m2 < e->dm.L))
            return fail(std::string(who) + ": region " + std::to_string(k) +
                        " outside the limits (l1 > 0, g >= 0, l2 >= 0, "
                        "l1 + g + l2 < L)");
    }
    return 0;
}

static int region_check_charges(const char *who, const qmc_engine *e,
                                int32_t nreg, int32_t num_charges)
{
    if (num_charges < 0 || num_charges > e->dm.n + 1)
        return fail(std::string(who) +
                    ": num_charges outside [0, boson_number + 1]");
    if ((long long)nreg * (3 + 2 * (long long)num_charges) > RG_MAX_SUMS)
        return fail(std::string(who) +
                    ": nreg (3 + 2 num_charges) exceeds 2^20");
    return 0;
}

// npair device-resident replica pairs -> n_x, log_ratio and / or the rows of
// a tile of `stride` pairs
static int region_launch(qmc_engine *e, long long npair, const double *pos_dev,
                         int32_t K, const double *regions_dev, double origin,
                         int32_t *n_x, double *log_ratio, double *rows,
                         long long stride)
{
    const size_t n2 = 2 * (size_t)e->dm.n;
    const size_t lds = renyi_region_lds_bytes(e->dm.n, K);
    if (e->dm.n > RG_MAX_N || lds > RENYI_LDS_LIMIT)
        return fail("qmc_renyi_region_swap: boson_number too large for the "
                    "LDS of a workgroup");
    allow_lds(renyi_region_kernel, lds);    // 88 KB at N = 512, K = 4096
    const long long xmax = 1ll << 30;
    for (long long p0 = 0; p0 < npair; p0 += xmax) {
        const long long np = std::min(xmax, npair - p0);
        RegionArgs a{ pos_dev + (size_t)p0 * n2, regions_dev,
                      n_x ? n_x + (size_t)p0 * 2 * K : nullptr,
                      log_ratio ? log_ratio + (size_t)p0 * K : nullptr,
                      rows ? rows + p0 : nullptr, np, stride, (int)K, origin };
        hipLaunchKernelGGL(renyi_region_kernel, dim3((unsigned)np), dim3(64),
                           lds, e->stream, e->dm_dev, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int qmc_renyi_region_swap_dev(qmc_engine *e, int64_t nconf,
                                         const double *pos, int32_t nreg,
                                         const double *regions, double origin,
                                         int32_t *n_x, double *log_ratio)
{
    if (!e || !pos || !regions || (!n_x && !log_ratio))
        return fail("qmc_renyi_region_swap_dev: null argument");
    if (renyi_check("qmc_renyi_region_swap_dev", nconf, nreg, origin, "nreg"))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    return region_launch(e, nconf / 2, pos, nreg, regions, origin, n_x,
                         log_ratio, nullptr, 0);
}

extern "C" int qmc_renyi_region_swap_reduce_dev(
    qmc_engine *e, int64_t nconf, const double *pos, int32_t nreg,
    const double *regions, double origin, int32_t num_charges, double *sums)
{
    const char *who = "qmc_renyi_region_swap_reduce_dev";
    if (!e || !pos || !regions || !sums)
        return fail(std::string(who) + ": null argument");
    if (renyi_check(who, nconf, nreg, origin, "nreg") ||
        region_check_charges(who, e, nreg, num_charges))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n2 = 2 * (size_t)e->dm.n;
    const int C = 2 * nreg;                     // columns of a pair's row
    const long long npair = nconf / 2;
    const long long tile = std::min<long long>(
        npair, std::min(PD_TILE, PD_SCRATCH_ELEMS / C));
    if (e->rg_rows.reserve((size_t)tile * C)) return 1;
    for (long long p0 = 0; p0 < npair; p0 += tile) {
        const long long np = std::min(tile, npair - p0);
        if (region_launch(e, np, pos + (size_t)p0 * n2, nreg, regions, origin,
                          nullptr, nullptr, e->rg_rows.get(), tile))
            return 1;
        hipLaunchKernelGGL(renyi_region_reduce_kernel,
                           dim3(nreg, 1 + num_charges), dim3(256), 0,
                           e->stream, e->rg_rows.get(), np, tile, (int)nreg,
                           (int)num_charges, p0 > 0 ? 1 : 0, sums);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int qmc_renyi_region_swap(qmc_engine *e, int64_t nconf,
                                     const double *pos, int32_t nreg,
                                     const double *regions, double origin,
                                     int32_t *n_x, double *log_ratio)
{
    if (!e || !pos || !regions || (!n_x && !log_ratio))
        return fail("qmc_renyi_region_swap: null argument");
    if (renyi_check("qmc_renyi_region_swap", nconf, nreg, origin, "nreg") ||
        region_check_host_regions("qmc_renyi_region_swap", e, nreg, regions))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, K = (size_t)nreg;
    // an even number of configurations to a tile: whole pairs
    const long long tile = std::max<long long>(
        2, std::min<long long>(
               nconf, PD_SCRATCH_ELEMS / (long long)std::max(n, K)) & ~1ll);
    DevBuf<double> dreg, dpos, dlr;
    DevBuf<int32_t> dnx;
    if (dreg.alloc(3 * K) || dpos.alloc((size_t)tile * n) ||
        (n_x && dnx.alloc((size_t)tile * K)) ||
        (log_ratio && dlr.alloc((size_t)(tile / 2) * K)))
        return 1;
    HIP_TRY(hipMemcpyAsync(dreg, regions, 3 * K * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    // log_ratio has a row per pair: half a row per configuration
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { n_x, dnx.get(), K * sizeof(int32_t) },
                            { log_ratio, dlr.get(), K * sizeof(double) / 2 } },
                          [&](long long nc) {
        return region_launch(e, nc / 2, dpos, nreg, dreg, origin, dnx.get(),
                             dlr.get(), nullptr, 0);
    });
}

// Region sums of the CURRENT configurations of the chains, chains 2p and
// 2p + 1 the replicas of pair p, on the resident rows (symmetric in the
// particles of a row, as qmc_vmc_renyi_swap); the chain state is only read.
extern "C" int qmc_vmc_renyi_region_swap(qmc_vmc *v, int32_t nreg,
                                         const double *regions, double origin,
                                         int32_t num_charges, double *out)
{
    const char *who = "qmc_vmc_renyi_region_swap";
    if (!v || !regions || !out)
        return fail(std::string(who) + ": null argument");
    qmc_engine *e = v->eng;
    if (v->W & 1)
        return fail(std::string(who) + ": an odd number of chains has no "
                    "replica pairs");
    if (renyi_check(who, v->W, nreg, origin, "nreg") ||
        region_check_host_regions(who, e, nreg, regions) ||
        region_check_charges(who, e, nreg, num_charges))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t K = (size_t)nreg, cols = 3 + 2 * (size_t)num_charges;
    if (e->rg_vmc.reserve((cols + 3) * K)) return 1;
    double *dreg = e->rg_vmc + cols * K;
    HIP_TRY(hipMemcpyAsync(dreg, regions, 3 * K * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    int rc = qmc_renyi_region_swap_reduce_dev(e, v->W, v->pos, nreg, dreg,
                                              origin, num_charges, e->rg_vmc);
    return rc ? rc : read_doubles(e, out, e->rg_vmc, cols * K);
}


// ---- one-particle replica swap (csrc/qmc_partent.h) -----------------------
// Tiles of at most PD_TILE pairs, one mean per pair.
static int partent_check(const char *who, int64_t nconf)
{
    if (nconf <= 0 || (nconf & 1))
        return fail(std::string(who) +
                    ": nconf must be positive and even (replica pairs)");
    return 0;
}

// npair device-resident replica pairs -> mean and / or log_ratio
static int partent_launch(qmc_engine *e, long long npair,
                          const double *pos_dev, double *mean,
                          double *log_ratio)
{
    const size_t n = (size_t)e->dm.n;
    const size_t lds = partent_lds_bytes(e->dm.n);
    if (lds > PARTENT_LDS_LIMIT)
        return fail("qmc_particle_swap: boson_number too large for the LDS of "
                    "a workgroup");
    allow_lds(particle_swap_kernel, lds);       // 40 KB at N = 512
    const long long xmax = 1ll << 30;
    for (long long p0 = 0; p0 < npair; p0 += xmax) {
        const long long np = std::min(xmax, npair - p0);
        PartEntArgs a{ pos_dev + (size_t)p0 * 2 * n,
                       mean ? mean + p0 : nullptr,
                       log_ratio ? log_ratio + (size_t)p0 * n * n : nullptr,
                       np };
        hipLaunchKernelGGL(particle_swap_kernel, dim3((unsigned)np), dim3(64),
                           lds, e->stream, e->dm_dev, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int qmc_particle_swap_dev(qmc_engine *e, int64_t nconf,
                                     const double *pos, double *mean,
                                     double *log_ratio)
{
    if (!e || !pos || (!mean && !log_ratio))
        return fail("qmc_particle_swap_dev: null argument");
    if (partent_check("qmc_particle_swap_dev", nconf)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    return partent_launch(e, nconf / 2, pos, mean, log_ratio);
}

extern "C" int qmc_particle_swap_reduce_dev(qmc_engine *e, int64_t nconf,
                                            const double *pos, double *sums)
{
    if (!e || !pos || !sums)
        return fail("qmc_particle_swap_reduce_dev: null argument");
    if (partent_check("qmc_particle_swap_reduce_dev", nconf)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n2 = 2 * (size_t)e->dm.n;
    const long long npair = nconf / 2;
    const long long tile = std::min(npair, PD_TILE);
    if (e->pe_mean.reserve((size_t)tile)) return 1;
    // one column: sums[0..1] = sum m, sum m^2, and the count of rows in
    // sums[2] (the weight sum of unweighted rows)
    return reduce_tiles(e, npair, tile, e->pe_mean, nullptr, 1, sums, sums + 2,
                        [&](long long p0, long long np) {
        return partent_launch(e, np, pos + (size_t)p0 * n2, e->pe_mean.get(),
                              nullptr);
    });
}

extern "C" int qmc_particle_swap(qmc_engine *e, int64_t nconf,
                                 const double *pos, double *mean,
                                 double *log_ratio)
{
    if (!e || !pos || (!mean && !log_ratio))
        return fail("qmc_particle_swap: null argument");
    if (partent_check("qmc_particle_swap", nconf)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    // an even number of configurations to a tile: whole pairs; a pair holds
    // N^2 doubles of log_ratio, half of them to a configuration
    const long long per_conf =
        log_ratio ? (long long)std::max<size_t>(n * n / 2, n) : (long long)n;
    const long long tile = std::max<long long>(
        2, std::min<long long>(nconf, PD_SCRATCH_ELEMS / per_conf) & ~1ll);
    DevBuf<double> dpos, dmean, dlr;
    if (dpos.alloc((size_t)tile * n) ||
        (mean && dmean.alloc((size_t)(tile / 2))) ||
        (log_ratio && dlr.alloc((size_t)(tile / 2) * n * n)))
        return 1;
    return run_host_tiles(e, nconf, tile, pos, dpos,
                          { { mean, dmean.get(), sizeof(double) / 2 },
                            { log_ratio, dlr.get(),
                              n * n * sizeof(double) / 2 } },
                          [&](long long nc) {
        return partent_launch(e, nc / 2, dpos, dmean.get(), dlr.get());
    });
}

// Sums of the CURRENT configurations of the chains, chains 2p and 2p + 1 the
// replicas of pair p, on the resident rows (the estimator is symmetric in the
// particles of a row, so neither the position order of the 'all' rows nor the
// label order of the 'particle' rows matters); the chain state is only read.
extern "C" int qmc_vmc_particle_swap(qmc_vmc *v, double *out)
{
    if (!v || !out) return fail("qmc_vmc_particle_swap: null argument");
    qmc_engine *e = v->eng;
    if (v->W & 1)
        return fail("qmc_vmc_particle_swap: an odd number of chains has no "
                    "replica pairs");
    if (partent_check("qmc_vmc_particle_swap", v->W)) return 1;
    HIP_TRY(hipSetDevice(e->device));
    if (e->pe_vmc.reserve(3)) return 1;
    int rc = qmc_particle_swap_reduce_dev(e, v->W, v->pos, e->pe_vmc);
    return rc ? rc : read_doubles(e, out, e->pe_vmc, 3);
}


// ---- one-body density matrix on a grid (csrc/qmc_obdm_grid.h) -------------
// Doubles of partial matrices the engine keeps (128 MB): with the wavefronts
// wanted below, what bounds the number S of partial matrices of a group.
static constexpr long long OGRID_SCRATCH_ELEMS = 1ll << 24;
// Wavefronts a launch aims at: a few to every SIMD of a device of this class
// (the bound is a constant of the decomposition, so that the summation order
// is the same on every device).
static constexpr long long OGRID_WAVES = 4096;

struct ObdmGridPlan {
    int M, G, S, rows, nrt, nct;
    double *part;          // the partial matrices: scratch, or sums at S = 1
};

static int obdm_grid_check(const char *who, const qmc_engine *e, int64_t nconf,
                           const void *pos, int32_t M, int32_t G,
                           const void *sums)
{
    const std::string w(who);
    if (!e || !pos || !sums) return fail(w + ": null argument");
    if (nconf <= 0) return fail(w + ": nconf must be positive");
    if (M < 1 || M > OGRID_MAX_POINTS)
        return fail(w + ": num_points must be in [1, 512]");
    if (G < 1 || G > OGRID_MAX_GROUPS || G > nconf)
        return fail(w + ": num_groups must be in [1, min(1024, nconf)]");
    return 0;
}

// The decomposition of nconf configurations (a function of nconf, M, G and N
// alone), the scratch it needs, and the partial matrices zeroed on the stream.
static int obdm_grid_plan(qmc_engine *e, long long nconf, int M, int G,
                          double *sums_dev, ObdmGridPlan &pl)
{
    const int n = e->dm.n;
    const long long mm = (long long)M * M;
    pl.M = M; pl.G = G;
    pl.nct = (M + 63) / 64;
    // about 32 particles of a configuration to a row tile: the tables and
    // the denominators, which every wavefront of a configuration computes for
    // itself (N pair factors to a lane and 64 particles), stay a few percent
    // of its work (N to a lane and particle)
    pl.nrt = std::max(1, std::min({ n / 32, M, 32 }));
    pl.rows = (M + pl.nrt - 1) / pl.nrt;
    pl.nrt = (M + pl.rows - 1) / pl.rows;
    const long long per = (long long)G * pl.nct * pl.nrt;
    long long S = (OGRID_WAVES + per - 1) / per;
    S = std::min(S, (nconf + G - 1) / G);
    S = std::min(S, OGRID_SCRATCH_ELEMS / (G * mm));
    pl.S = (int)std::max(1ll, S);
    if (pl.S > 1) {
        if (e->og_part.reserve((size_t)pl.S * G * mm)) return 1;
        pl.part = e->og_part;
    } else {
        pl.part = sums_dev;
    }
    HIP_TRY(hipMemsetAsync(pl.part, 0, (size_t)pl.S * G * mm * sizeof(double),
                           e->stream));
    return 0;
}

// the configurations c_base .. c_base + nc of the batch into the partial
// matrices (tiles of a batch arrive in order)
static int obdm_grid_launch(qmc_engine *e, const ObdmGridPlan &pl,
                            long long c_base, long long nc,
                            const double *pos_dev, const double *w_dev)
{
    const size_t lds = obdm_grid_lds_bytes(e->dm.n);
    allow_lds(obdm_grid_kernel, lds);           // 32 KB at N = 512
    ObdmGridArgs a{ pos_dev, w_dev, pl.part, c_base, nc, pl.M, pl.G, pl.S,
                    pl.rows, pl.nrt, pl.nct };
    const long long blocks = (long long)pl.S * pl.G * pl.nrt * pl.nct;
    hipLaunchKernelGGL(obdm_grid_kernel, dim3((unsigned)blocks), dim3(64), lds,
                       e->stream, e->dm_dev, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// partial matrices -> sums, and wsum from the whole batch's weights
static int obdm_grid_finish(qmc_engine *e, const ObdmGridPlan &pl,
                            long long nconf, const double *w_dev,
                            double *sums_dev, double *wsum_dev)
{
    const long long mm = (long long)pl.M * pl.M;
    if (pl.S > 1) {
        const long long total = (long long)pl.G * mm;
        hipLaunchKernelGGL(obdm_grid_fold_kernel,
                           dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           e->stream, pl.part, pl.G, pl.S, mm, sums_dev);
        HIP_TRY(hipGetLastError());
    }
    if (wsum_dev) {
        hipLaunchKernelGGL(obdm_grid_wsum_kernel, dim3((unsigned)pl.G),
                           dim3(256), 0, e->stream, w_dev, nconf, pl.G,
                           wsum_dev);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int qmc_obdm_grid_dev(qmc_engine *e, int64_t nconf,
                                 const double *pos, const double *w,
                                 int32_t num_points, int32_t num_groups,
                                 double *sums, double *wsum)
{
    if (obdm_grid_check("qmc_obdm_grid_dev", e, nconf, pos, num_points,
                        num_groups, sums))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    ObdmGridPlan pl;
    if (obdm_grid_plan(e, nconf, num_points, num_groups, sums, pl) ||
        obdm_grid_launch(e, pl, 0, nconf, pos, w))
        return 1;
    return obdm_grid_finish(e, pl, nconf, w, sums, wsum);
}

extern "C" int qmc_obdm_grid(qmc_engine *e, int64_t nconf, const double *pos,
                             const double *w, int32_t num_points,
                             int32_t num_groups, double *sums, double *wsum)
{
    if (obdm_grid_check("qmc_obdm_grid", e, nconf, pos, num_points, num_groups,
                        sums))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    const size_t G = (size_t)num_groups, mm = (size_t)num_points * num_points;
    const long long tile = std::max<long long>(
        1, std::min<long long>(nconf, PD_SCRATCH_ELEMS / (long long)n));
    DevBuf<double> dpos, dw, dsums, dwsum;
    if (dpos.alloc((size_t)tile * n) || (w && dw.alloc((size_t)nconf)) ||
        dsums.alloc(G * mm) || (wsum && dwsum.alloc(G)))
        return 1;
    if (w)
        HIP_TRY(hipMemcpyAsync(dw, w, (size_t)nconf * sizeof(double),
                               hipMemcpyHostToDevice, e->stream));
    ObdmGridPlan pl;
    if (obdm_grid_plan(e, nconf, num_points, num_groups, dsums, pl)) return 1;
    long long c0 = 0;
    if (run_host_tiles(e, nconf, tile, pos, dpos, {}, [&](long long nc) {
            const int rc = obdm_grid_launch(e, pl, c0, nc, dpos,
                                            w ? dw.get() + c0 : nullptr);
            c0 += nc;
            return rc;
        }))
        return 1;
    if (obdm_grid_finish(e, pl, nconf, w ? dw.get() : nullptr, dsums,
                         wsum ? dwsum.get() : nullptr))
        return 1;
    // into a host copy first: the outputs are left untouched by a failure
    std::vector<double> hs(G * mm), hw(wsum ? G : 0);
    if (read_doubles(e, hs.data(), dsums, G * mm) ||
        (wsum && read_doubles(e, hw.data(), dwsum, G)))
        return 1;
    std::copy(hs.begin(), hs.end(), sums);
    if (wsum) std::copy(hw.begin(), hw.end(), wsum);
    return 0;
}

// The matrix sums of the CURRENT configurations of the chains, group = chain
// index mod num_groups, on the resident rows (nothing depends on the order of
// a row: position-sorted after move = 'all', by label after 'particle'); the
// chain state is only read.
extern "C" int qmc_vmc_obdm_grid(qmc_vmc *v, int32_t num_points,
                                 int32_t num_groups, double *sums)
{
    if (!v) return fail("qmc_vmc_obdm_grid: null argument");
    qmc_engine *e = v->eng;
    if (obdm_grid_check("qmc_vmc_obdm_grid", e, v->W, v->pos, num_points,
                        num_groups, sums))
        return 1;
    HIP_TRY(hipSetDevice(e->device));
    const size_t count = (size_t)num_groups * num_points * num_points;
    if (e->og_vmc.reserve(count)) return 1;
    if (qmc_obdm_grid_dev(e, v->W, v->pos, nullptr, num_points, num_groups,
                          e->og_vmc, nullptr))
        return 1;
    std::vector<double> hs(count);
    if (read_doubles(e, hs.data(), e->og_vmc, count)) return 1;
    std::copy(hs.begin(), hs.end(), sums);
    return 0;
}


extern "C" int qmc_vmc_block_sums_dev(qmc_vmc *v, double **se, double **se2,
                                      int64_t **na)
{
    if (!v) return fail("qmc_vmc_block_sums_dev: null argument");
    if (se) *se = v->sum_e;
    if (se2) *se2 = v->sum_e2;
    if (na) *na = (int64_t *)v->n_acc.get();
    return 0;
}

extern "C" int qmc_vmc_run_block(qmc_vmc *v, int64_t nyield, double *sum_e,
                                 double *sum_e2, int64_t *n_acc,
                                 double *ser_wf, double *ser_e,
                                 uint8_t *ser_stat, double *ser_pos)
{
    if (!v) return fail("qmc_vmc_run_block: null argument");
    if (nyield <= 0) return fail("qmc_vmc_run_block: nyield must be >= 1");
    qmc_engine *e = v->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t W = (size_t)v->W, ny = (size_t)nyield;
    const long long real = nyield - (v->yield_initial ? 1 : 0);
    if (v->tape && v->tape_used + real > v->tape_steps)
        return fail("qmc_vmc_run_block: tape exhausted");
    // (the series of this block; they go when the entry point returns)
    DevBuf<double> dwf, de, dpos;
    DevBuf<unsigned char> dst;
    if ((ser_pos && dpos.alloc(ny * W * (size_t)e->dm.n)) ||
        (ser_wf && dwf.alloc(ny * W)) || (ser_e && de.alloc(ny * W)) ||
        (ser_stat && dst.alloc(ny * W)))
        return 1;
    VmcArgs a;
    a.pos = v->pos; a.label = v->label; a.rec = v->rec;
    a.ser_wf = dwf; a.ser_e = de; a.ser_stat = dst; a.ser_pos = dpos;
    a.tape = v->tape;
    a.tape_steps = v->tape_steps;
    a.W = v->W;
    a.gaussian = v->p.gaussian;
    a.chain0 = v->p.chain0;
    a.seed = v->p.rng_seed; a.move_spread = v->p.move_spread;
    if (v->p.gaussian == QMC_VMC_PARTICLE) {
        // single-particle sweeps: the whole block in one launch
        a.y = 0;
        a.forced = v->yield_initial ? 1 : 0;
        a.reset_sums = 1;
        a.step = v->step;
        a.tape = nullptr; a.tape_steps = 0; a.tape_idx = 0;
        a.nsteps = (unsigned int)nyield;
        int rc = dispatch_shape<LaunchSweep>(e, a);
        if (rc) return rc;
        v->step += (unsigned int)real;
    }
    for (long long y = (v->p.gaussian == QMC_VMC_PARTICLE) ? nyield : 0;
         y < nyield;) {
        a.y = y;
        a.forced = (y == 0 && v->yield_initial) ? 1 : 0;
        a.reset_sums = (y == 0) ? 1 : 0;
        a.step = v->step;
        a.tape_idx = v->tape_used;
        a.nsteps = (unsigned int)(nyield - y);
        long long ran = 1;
        int rc = dispatch_shape<LaunchVmc>(e, a, &ran);
        if (rc) return rc;
        if (!a.forced) { v->step += ran; v->tape_used += ran; }
        y += ran;
    }
    v->yield_initial = 0;
    // the records into the compact arrays of the C ABI (on the engine stream,
    // ahead of the copies below and of any later reader)
    hipLaunchKernelGGL(vmc_unpack_kernel, dim3((unsigned)((W + BLOCK - 1) / BLOCK)),
                       dim3(BLOCK), 0, e->stream, v->rec, v->W, v->wf, v->ecarry,
                       v->sum_e, v->sum_e2, v->n_acc);
    HIP_TRY(hipGetLastError());
    bool need_sync = false;
    if (sum_e) { HIP_TRY(hipMemcpyAsync(sum_e, v->sum_e, W * sizeof(double),
                 hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (sum_e2) { HIP_TRY(hipMemcpyAsync(sum_e2, v->sum_e2, W * sizeof(double),
                  hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (n_acc) { HIP_TRY(hipMemcpyAsync(n_acc, v->n_acc, W * sizeof(int64_t),
                 hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (ser_wf) { HIP_TRY(hipMemcpyAsync(ser_wf, dwf, ny * W * sizeof(double),
                  hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (ser_e) { HIP_TRY(hipMemcpyAsync(ser_e, de, ny * W * sizeof(double),
                 hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (ser_stat) { HIP_TRY(hipMemcpyAsync(ser_stat, dst, ny * W,
                    hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (ser_pos) { HIP_TRY(hipMemcpyAsync(ser_pos, dpos,
                   ny * W * (size_t)e->dm.n * sizeof(double),
                   hipMemcpyDeviceToHost, e->stream)); need_sync = true; }
    if (need_sync) HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

// ----------------------------------------------------------------- DMC ----
// What a setter asks of a slot: K modes or bins (0: off) of C doubles each;
// `aux`: keep per-walker rows, of A doubles (0: as the output, K * C).
struct DmcEstSpec {
    int K, C, pure;
    long long pfw;
    bool aux;
    int A = 0;
    int stride = 1;              // (F(k, tau), g1(s); site statistics: P)
};

// One per-step estimator of a population: K modes or bins of C doubles each.
struct DmcEstSlot {
    int K = 0;                   // modes or bins; 0: off
    int C = 1;                   // doubles per mode or bin
    int A = 0;                   // doubles per walker in the rows; 0: as the
                                 // output, K * C
    int pure = 0;
    long long pfw = 1;           // forward-walking length; F(k, tau): lags
    int stride = 1;              // F(k, tau): time steps per lag; g1(s): time
                                 // steps per evaluation; site statistics: the
                                 // occupation bins P of the K = P + D
    DevBuf<double> aux[2];       // [maxw][aux_row()] per-walker rows (null: none kept)
    DevBuf<double> iter;         // [steps][K][C] per-step outputs, grown on demand
    DevBuf<double> tab;          // a table of the estimator's own (g1(s): the
                                 // shift rows), filled by its setter
    size_t row() const { return (size_t)K * C; }
    size_t aux_row() const { return A ? (size_t)A : row(); }
    bool on() const { return K > 0; }
    void drop()
    {
        aux[0].release();
        aux[1].release();
        iter.release();
        tab.release();
        K = 0; C = 1; A = 0; pure = 0; pfw = 1; stride = 1;
    }
    // on (K > 0), with the rows of `maxw` walkers if asked for; a failure
    // leaves it off
    int set(const DmcEstSpec &a, size_t maxw)
    {
        drop();
        if (a.K <= 0) return 0;
        K = a.K; C = a.C; A = a.A; pure = a.pure; pfw = a.pfw;
        stride = a.stride;
        for (int b = 0; b < 2 && a.aux; ++b)
            if (aux[b].alloc(maxw * aux_row())) {
                drop();
                return 1;
            }
        return 0;
    }
};
enum { EST_SSF, EST_DENS, EST_PD, EST_CM, EST_ISF, EST_OBDM, EST_SITE,
       EST_SLOTS };
// (the header's names of the slots: qmc_dmc_est_rows_dev)
static_assert(EST_SSF == QMC_EST_SSF && EST_DENS == QMC_EST_DENSITY &&
              EST_PD == QMC_EST_PAIR_DIST && EST_CM == QMC_EST_CM_DIFFUSION &&
              EST_ISF == QMC_EST_ISF && EST_OBDM == QMC_EST_OBDM &&
              EST_SITE == QMC_EST_SITE && EST_SLOTS == QMC_EST_SLOTS,
              "the estimator slots as include/qmcwalk.h names them");

struct qmc_dmc {
    qmc_engine *eng = nullptr;
    qmc_dmc_params p;
    long long maxw = 0;
    int nblocks = 0;
    // two population buffers: [0]/[1] alternate parent / child roles
    DevBuf<double> pos[2], drift[2];
    DevBuf<unsigned short> label[2];
    DevBuf<double> energy[2], weight[2];
    int cur = 0;                 // index of the parent buffer
    DevBuf<double> eslot;
    DevBuf<double> spare;        // (one particle per lane only: DmcSpare)
    DevBuf<long long> ref;
    DevBuf<int> count;
    DevBuf<long long> block_tot, block_off;
    DevBuf<double> block_esum;
    DevBuf<DmcCtl> ctl;
    // per-step series (device), capacity ser_cap steps: the five grow together
    DevBuf<double> ser_e, ser_w, ser_ref, ser_acc;
    DevBuf<unsigned long long> ser_nw;
    long long ser_cap = 0, ser_len = 0;
    // tapes (test only)
    DevBuf<double> u_tape, g_tape;
    std::vector<long long> u_off, g_off;
    long long tape_step = 0;
    bool stepped = false;        // a step has run since the last set_state
    std::vector<double> init_weight;   // weights of set_full_state as given (the
                                       // device keeps their logarithms)
    bool sums_pending = false;   // E_t partials still to be summed (by finish)
    double global_target = 0.0;
    // estimators, in launch order: S(k) (3 doubles per mode) and the density,
    // set together, the pair distribution (qmc_pairdist.h) and the
    // centre-of-mass diffusion (qmc_cmdiff.h: two sums per step, one double
    // per walker) and the imaginary-time density correlations (qmc_isf.h:
    // K modes of lags + 2 doubles), each set on its own, and the one-body
    // density matrix (qmc_obdm.h: K shifts, its shift table in the slot) and
    // the site occupation statistics (qmc_site.h: K = P + D counts)
    DmcEstSlot est[EST_SLOTS];
    DevBuf<double> est_partial;     // [EST_BLOCKS][widest row]
    long long est_block_steps = 0;  // steps of the estimator block in progress
    int est_last_act = 1;           // aux buffer the last estimator step wrote
    bool record_rows = false;       // the walker record carries every slot's
                                    // rows, not those of S(k) / density alone
    bool any_est() const
    {
        return std::any_of(est, est + EST_SLOTS,
                           [](const DmcEstSlot &s) { return s.on(); });
    }
};

// est_partial holds the block partial sums of one estimator at a time:
// [EST_BLOCKS][widest row of the estimators that are on].
static int dmc_size_est_partial(qmc_dmc *d)
{
    size_t kc = 0;
    for (const DmcEstSlot &s : d->est) kc = std::max(kc, s.row());
    d->est_partial.release();
    return kc ? d->est_partial.alloc(EST_BLOCKS * kc) : 0;
}

// Replace the settings of `count` slots from `first` on; the other slots stay
// as they are.  A failed allocation leaves these slots off and the others
// with partial sums of their own size; if even those cannot be had, every
// slot is off.  Nothing is ever on over a missing buffer.
static int dmc_set_est_slots(qmc_dmc *d, int first, int count,
                             const DmcEstSpec *spec)
{
    d->est_block_steps = 0;
    d->est_partial.release();
    for (int i = 0; i < count; ++i) d->est[first + i].drop();
    bool ok = true;
    for (int i = 0; i < count && ok; ++i)
        ok = d->est[first + i].set(spec[i], (size_t)d->maxw) == 0;
    if (ok && dmc_size_est_partial(d) == 0) return 0;
    for (int i = 0; i < count; ++i) d->est[first + i].drop();
    if (dmc_size_est_partial(d))
        for (DmcEstSlot &s : d->est) s.drop();
    return 1;            // (alloc has set the message)
}

static int dmc_reserve_series(qmc_dmc *d, long long nsteps)
{
    if (nsteps <= d->ser_cap) return 0;
    d->ser_cap = 0;             // (nothing is recorded into a partly grown set)
    const size_t ns = (size_t)nsteps;
    if (d->ser_e.alloc(ns) || d->ser_w.alloc(ns) || d->ser_ref.alloc(ns) ||
        d->ser_acc.alloc(ns) || d->ser_nw.alloc(ns))
        return 1;
    d->ser_cap = nsteps;
    return 0;
}

extern "C" int qmc_dmc_create(qmc_engine *e, const qmc_dmc_params *p,
                              qmc_dmc **out)
{
    if (!e || !p || !out) return fail("qmc_dmc_create: null argument");
    if (p->max_num_walkers <= 0 || p->target_num_walkers <= 0)
        return fail("qmc_dmc_create: walker counts must be positive");
    if (!(p->time_step > 0)) return fail("qmc_dmc_create: time_step <= 0");
    if (p->propagator != QMC_DMC_LINEAR && p->propagator != QMC_DMC_QUADRATIC)
        return fail("qmc_dmc_create: unknown propagator (0: linear, "
                    "1: second order)");
    HIP_TRY(hipSetDevice(e->device));
    std::unique_ptr<qmc_dmc> d(new qmc_dmc());
    d->eng = e;
    d->p = *p;
    d->maxw = p->max_num_walkers;
    d->nblocks = (int)((d->maxw + BR_TILE - 1) / BR_TILE);
    d->global_target = (double)p->target_num_walkers;
    const size_t W = (size_t)d->maxw, n = (size_t)e->dm.n;
    for (int b = 0; b < 2; ++b)
        if (d->pos[b].alloc(W * n) || d->drift[b].alloc(W * n) ||
            d->label[b].alloc(W * n) || d->energy[b].alloc(W) ||
            d->weight[b].alloc(W))
            return 1;
    // (the cached second Box-Muller normal: one particle per lane only,
    // qmc_kernels.h: DmcSpare)
    // (the second-order step uses both normals of a block at once: no cache)
    const bool need_spare = e->P == 1 && p->propagator == QMC_DMC_LINEAR;
    if (d->eslot.alloc(W) || (need_spare && d->spare.alloc(W * n)) ||
        d->ref.alloc(W) || d->count.alloc(W) ||
        d->block_tot.alloc(d->nblocks) || d->block_off.alloc(d->nblocks) ||
        d->block_esum.alloc(d->nblocks) || d->ctl.alloc(1))
        return 1;
    HIP_TRY(hipMemset(d->ctl, 0, sizeof(DmcCtl)));
    HIP_TRY(hipMemset(d->ref, 0, W * sizeof(long long)));
    HIP_TRY(hipMemset(d->eslot, 0, W * sizeof(double)));
    *out = d.release();
    return 0;
}

extern "C" void qmc_dmc_destroy(qmc_dmc *d)
{
    if (!d) return;
    (void)hipSetDevice(d->eng->device);
    delete d;
}

static int dmc_reset_ctl(qmc_dmc *d, long long nw, double ref_energy)
{
    DmcCtl c;
    memset(&c, 0, sizeof(c));
    c.prev_nw = nw;
    c.nw = nw;
    c.ref_energy = ref_energy;
    HIP_TRY(hipMemcpyAsync(d->ctl, &c, sizeof(c), hipMemcpyHostToDevice,
                           d->eng->stream));
    HIP_TRY(hipStreamSynchronize(d->eng->stream));
    d->cur = 0;
    d->stepped = false;
    d->tape_step = 0;
    d->ser_len = 0;
    return 0;
}

static int dmc_zero_population(qmc_dmc *d)
{
    d->init_weight.clear();
    qmc_engine *e = d->eng;
    const size_t n = (size_t)e->dm.n, W = (size_t)d->maxw;
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(hipMemsetAsync(d->pos[b], 0, W * n * sizeof(double), e->stream));
        HIP_TRY(hipMemsetAsync(d->drift[b], 0, W * n * sizeof(double), e->stream));
        HIP_TRY(hipMemsetAsync(d->energy[b], 0, W * sizeof(double), e->stream));
        HIP_TRY(hipMemsetAsync(d->weight[b], 0, W * sizeof(double), e->stream));
        hipLaunchKernelGGL(ident_labels_kernel,
                           dim3((unsigned)((W * n + 255) / 256)), dim3(256), 0,
                           e->stream, d->label[b], (long long)W, (int)n);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(d->eslot, 0, W * sizeof(double), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

// pos: host positions (sorted here) or device positions already in lane order
// with their labels (label_dev, may be null = identity).
static int dmc_set_state_impl(qmc_dmc *d, int64_t nw, const double *pos,
                              bool pos_on_device,
                              const unsigned short *label_dev, int use_ref,
                              double ref_energy, int64_t src_rows = 0)
{
    if (!d || !pos) return fail("qmc_dmc_set_state: null argument");
    if (nw <= 0 || nw > d->maxw)
        return fail("qmc_dmc_set_state: number of walkers out of range");
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n;
    if (dmc_zero_population(d)) return 1;
    if (pos_on_device && src_rows > 0 && src_rows < nw) {
        // more walkers than source rows: the rows are reused cyclically
        const long long tot = (long long)nw * (long long)n;
        const unsigned grid = (unsigned)((tot + 255) / 256);
        hipLaunchKernelGGL(tile_rows_kernel<double>, dim3(grid), dim3(256), 0,
                           e->stream, pos, (long long)src_rows, d->pos[0],
                           (long long)nw, (int)n);
        if (label_dev)
            hipLaunchKernelGGL(tile_rows_kernel<unsigned short>, dim3(grid),
                               dim3(256), 0, e->stream, label_dev,
                               (long long)src_rows, d->label[0], (long long)nw,
                               (int)n);
        HIP_TRY(hipGetLastError());
    } else if (pos_on_device) {
        HIP_TRY(hipMemcpyAsync(d->pos[0], pos, (size_t)nw * n * sizeof(double),
                               hipMemcpyDeviceToDevice, e->stream));
        if (label_dev)
            HIP_TRY(hipMemcpyAsync(d->label[0], label_dev,
                                   (size_t)nw * n * sizeof(unsigned short),
                                   hipMemcpyDeviceToDevice, e->stream));
    } else {
        std::vector<double> sorted;
        std::vector<unsigned short> label;
        sort_rows(pos, (size_t)nw, n, sorted, label);
        HIP_TRY(hipMemcpyAsync(d->pos[0], sorted.data(),
                               (size_t)nw * n * sizeof(double),
                               hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(d->label[0], label.data(),
                               (size_t)nw * n * sizeof(unsigned short),
                               hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    PrepArgs a{ d->pos[0], d->drift[0], d->energy[0], (long long)nw };
    int rc = dispatch_shape<LaunchPrep>(e, a);
    if (rc) return rc;
    std::vector<double> en((size_t)nw);
    // unit weights; the device keeps LOG weights (dmc_evolve_kernel)
    HIP_TRY(hipMemsetAsync(d->weight[0], 0, (size_t)nw * sizeof(double), e->stream));
    HIP_TRY(hipMemcpyAsync(en.data(), d->energy[0], (size_t)nw * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(d->eslot, d->energy[0], (size_t)nw * sizeof(double),
                           hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (!use_ref) {
        // mrbp_qmc/dmc.py:302-312: sum(E w) / sum(w) with unit weights
        double se = 0.0;
        for (size_t i = 0; i < (size_t)nw; ++i) se += en[i] * 1.0;
        ref_energy = se / (double)nw;
    }
    return dmc_reset_ctl(d, nw, ref_energy);
}

extern "C" int qmc_dmc_set_state(qmc_dmc *d, int64_t nw, const double *pos,
                                 int use_ref, double ref_energy)
{
    return dmc_set_state_impl(d, nw, pos, false, nullptr, use_ref, ref_energy);
}

extern "C" int qmc_dmc_set_state_dev(qmc_dmc *d, int64_t nw,
                                     const double *pos_dev, int use_ref,
                                     double ref_energy)
{
    return dmc_set_state_impl(d, nw, pos_dev, true, nullptr, use_ref,
                              ref_energy);
}

extern "C" int qmc_dmc_set_state_from_vmc(qmc_dmc *d, qmc_vmc *v, int64_t nw,
                                          int use_ref, double ref_energy)
{
    if (!d || !v) return fail("qmc_dmc_set_state_from_vmc: null argument");
    if (v->eng != d->eng)
        return fail("qmc_dmc_set_state_from_vmc: ensembles of different engines");
    // nw > num_chains: the chains are reused cyclically
    return dmc_set_state_impl(d, nw, v->pos, true, v->label, use_ref,
                              ref_energy, v->W);
}

extern "C" int qmc_dmc_set_full_state(qmc_dmc *d, int64_t nw,
                                      const double *confs,
                                      const double *energy,
                                      const double *weight,
                                      const double *slot_energy,
                                      double ref_energy)
{
    if (!d || !confs || !energy || !weight)
        return fail("qmc_dmc_set_full_state: null argument");
    if (nw <= 0 || nw > d->maxw)
        return fail("qmc_dmc_set_full_state: number of walkers out of range");
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, W = (size_t)d->maxw;
    // confs[s] = (pos row, drift row): sort by position, carry the drift along
    std::vector<double> hp, hd;
    std::vector<unsigned short> label;
    sort_rows(confs, (size_t)nw, n, hp, label, confs + n, &hd, 2 * n, 2 * n);
    if (dmc_zero_population(d)) return 1;
    HIP_TRY(hipMemcpyAsync(d->pos[0], hp.data(), hp.size() * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d->drift[0], hd.data(), hd.size() * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d->label[0], label.data(),
                           label.size() * sizeof(unsigned short),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d->energy[0], energy, (size_t)nw * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    // the device keeps LOG weights (dmc_evolve_kernel); a weight <= 0 has no
    // children either way
    std::vector<double> logw((size_t)nw);
    d->init_weight.assign(weight, weight + nw);
    for (size_t i = 0; i < (size_t)nw; ++i)
        logw[i] = weight[i] > 0.0 ? std::log(weight[i]) : -HUGE_VAL;
    HIP_TRY(hipMemcpyAsync(d->weight[0], logw.data(), (size_t)nw * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
    // the reference copies the whole props.energy array of the initial state
    // into its `actual` buffer (qmc_base/dmc.py:707-708), stale tail included
    if (slot_energy)
        HIP_TRY(hipMemcpyAsync(d->eslot, slot_energy, W * sizeof(double),
                               hipMemcpyHostToDevice, e->stream));
    else
        HIP_TRY(hipMemcpyAsync(d->eslot, energy, (size_t)nw * sizeof(double),
                               hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return dmc_reset_ctl(d, nw, ref_energy);
}

extern "C" int qmc_dmc_set_tape(qmc_dmc *d, const double *u, int64_t nu,
                                const double *g, int64_t ng,
                                const int64_t *u_off, const int64_t *g_off,
                                int64_t nsteps)
{
    if (!d) return fail("qmc_dmc_set_tape: null argument");
    HIP_TRY(hipSetDevice(d->eng->device));
    d->u_tape.release();
    d->g_tape.release();
    d->u_off.clear(); d->g_off.clear();
    d->tape_step = 0;
    if (!u || !g || nsteps <= 0) return 0;
    // pad so that a step may read up to maxw uniforms / maxw*N normals
    // (the second-order step: [slot][2][N], two rows per walker)
    const size_t rows = d->p.propagator == QMC_DMC_QUADRATIC ? 2 : 1;
    size_t upad = (size_t)nu + (size_t)d->maxw;
    size_t gpad = (size_t)ng + rows * (size_t)d->maxw * (size_t)d->eng->dm.n;
    if (d->u_tape.alloc(upad) || d->g_tape.alloc(gpad)) return 1;
    HIP_TRY(hipMemset(d->u_tape, 0, upad * sizeof(double)));
    HIP_TRY(hipMemset(d->g_tape, 0, gpad * sizeof(double)));
    HIP_TRY(hipMemcpy(d->u_tape, u, (size_t)nu * sizeof(double),
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->g_tape, g, (size_t)ng * sizeof(double),
                      hipMemcpyHostToDevice));
    d->u_off.assign(u_off, u_off + nsteps);
    d->g_off.assign(g_off, g_off + nsteps);
    return 0;
}

static FinishArgs dmc_finish_args(qmc_dmc *d, const double *total_dev,
                                  long long ser_idx)
{
    FinishArgs f;
    f.ctl = d->ctl; f.total = total_dev;
    f.block_esum = (!total_dev && d->sums_pending) ? d->block_esum.get() : nullptr;
    const bool rec = ser_idx >= 0;
    f.ser_e = rec ? d->ser_e.get() : nullptr; f.ser_w = d->ser_w;
    f.ser_ref = d->ser_ref; f.ser_acc = d->ser_acc; f.ser_nw = d->ser_nw;
    f.ser_idx = ser_idx;
    f.kappa = d->p.num_walkers_control_factor; f.dt = d->p.time_step;
    f.target = d->global_target;
    return f;
}

// Small populations run the whole branching step in one workgroup
// (branch_fused_kernel), which can also carry the previous step's bookkeeping.
static bool dmc_fused_branching(const qmc_dmc *d)
{
    return d->nblocks <= BR_FUSED_TILES;
}

// Enqueue the rank-local part of one time step.  `prev_fin`: the bookkeeping of
// the step before, to ride at the head of the fused branching kernel (only
// where dmc_fused_branching(d)).
// `prev_fin_done` (if given) is set once the fused branching kernel -- which
// applies the previous step's deferred bookkeeping `prev_fin` at its head --
// has been enqueued: a caller that sees an error must launch that bookkeeping
// itself only while the flag is still false.
static int dmc_enqueue_local(qmc_dmc *d, double *partial_dev,
                             const FinishArgs *prev_fin = nullptr,
                             bool *prev_fin_done = nullptr)
{
    qmc_engine *e = d->eng;
    const int par = d->cur, chi = 1 - d->cur;
    const double *ut = nullptr, *gt = nullptr;
    if (d->u_tape) {
        if (d->tape_step >= (long long)d->u_off.size())
            return fail("qmc_dmc: tape exhausted");
        ut = d->u_tape + d->u_off[(size_t)d->tape_step];
        gt = d->g_tape + d->g_off[(size_t)d->tape_step];
        d->tape_step += 1;
    }
    BranchArgs b;
    b.weight = d->weight[par]; b.energy = d->energy[par];
    b.count = d->count; b.block_tot = d->block_tot; b.block_off = d->block_off;
    b.block_esum = d->block_esum; b.ref = d->ref; b.ctl = d->ctl;
    b.u_tape = ut; b.maxw = d->maxw; b.seed = d->p.rng_seed;
    b.slot0 = d->p.slot0;
    if (dmc_fused_branching(d)) {
        d->sums_pending = false;
        FinishArgs none{};
        hipLaunchKernelGGL(branch_fused_kernel, dim3(1), dim3(BLOCK), 0,
                           e->stream, b, partial_dev,
                           prev_fin ? *prev_fin : none, prev_fin ? 1 : 0);
        if (prev_fin_done) *prev_fin_done = true;
    } else {
        if (prev_fin) return fail("qmc_dmc: internal: deferred bookkeeping "
                                  "needs the fused branching kernel");
        hipLaunchKernelGGL(branch_count_kernel, dim3(d->nblocks), dim3(BLOCK),
                           0, e->stream, b);
        hipLaunchKernelGGL(branch_scatter_kernel, dim3(d->nblocks),
                           dim3(BLOCK), 0, e->stream, b);
        // single GPU: the finish kernel sums the partials itself
        d->sums_pending = partial_dev == nullptr;
        if (partial_dev)
            hipLaunchKernelGGL(dmc_local_sums_kernel, dim3(1), dim3(BLOCK), 0,
                               e->stream, d->block_esum, d->ctl, partial_dev);
    }
    HIP_TRY(hipGetLastError());
    EvolveArgs a;
    a.ppos = d->pos[par]; a.pdrift = d->drift[par]; a.penergy = d->energy[par];
    a.cpos = d->pos[chi]; a.cdrift = d->drift[chi];
    a.plabel = d->label[par]; a.clabel = d->label[chi];
    a.cenergy = d->energy[chi]; a.cweight = d->weight[chi];
    a.eslot = d->eslot; a.ref = d->ref; a.ctl = d->ctl; a.g_tape = gt;
    a.spare = d->spare;
    a.maxw = d->maxw; a.dt = d->p.time_step;
    a.sigma = sqrt(2 * d->p.time_step);           // mrbp_qmc/dmc.py:178
    a.seed = d->p.rng_seed; a.slot0 = d->p.slot0;
    a.fix_stale = d->p.fix_stale_energy;
    if (d->p.propagator == QMC_DMC_QUADRATIC) {
        // two half diffusions of spread sqrt(dt) each around the drift
        a.sigma = sqrt(d->p.time_step);
        return dispatch_shape<LaunchEvolve2>(e, a);
    }
    int rc = dispatch_shape<LaunchEvolve>(e, a);
    if (rc) return rc;
    return 0;
}

static int dmc_enqueue_finish(qmc_dmc *d, const double *total_dev,
                              long long ser_idx)
{
    qmc_engine *e = d->eng;
    const FinishArgs f = dmc_finish_args(d, total_dev, ser_idx);
    hipLaunchKernelGGL(dmc_finish_kernel, dim3(1), dim3(BLOCK), 0, e->stream,
                       f);
    HIP_TRY(hipGetLastError());
    d->cur = 1 - d->cur;          // children become the parents
    d->stepped = true;
    return 0;
}

extern "C" int qmc_dmc_read_series(qmc_dmc *d, int64_t nsteps, double *energy,
                                   double *weight, uint64_t *num_walkers,
                                   double *ref_energy, double *accum_energy)
{
    if (!d) return fail("qmc_dmc_read_series: null argument");
    if (nsteps > d->ser_len) return fail("qmc_dmc_read_series: too many steps");
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t ns = (size_t)nsteps;
    if (energy) HIP_TRY(hipMemcpyAsync(energy, d->ser_e, ns * 8,
                                       hipMemcpyDeviceToHost, e->stream));
    if (weight) HIP_TRY(hipMemcpyAsync(weight, d->ser_w, ns * 8,
                                       hipMemcpyDeviceToHost, e->stream));
    if (num_walkers) HIP_TRY(hipMemcpyAsync(num_walkers, d->ser_nw, ns * 8,
                                            hipMemcpyDeviceToHost, e->stream));
    if (ref_energy) HIP_TRY(hipMemcpyAsync(ref_energy, d->ser_ref, ns * 8,
                                           hipMemcpyDeviceToHost, e->stream));
    if (accum_energy) HIP_TRY(hipMemcpyAsync(accum_energy, d->ser_acc, ns * 8,
                                             hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // a full read consumes the series (split-step drivers append to it)
    if (nsteps == d->ser_len) d->ser_len = 0;
    return 0;
}

extern "C" int qmc_dmc_run_block(qmc_dmc *d, int64_t nsteps, double *energy,
                                 double *weight, uint64_t *num_walkers,
                                 double *ref_energy, double *accum_energy)
{
    if (!d) return fail("qmc_dmc_run_block: null argument");
    if (nsteps <= 0) return fail("qmc_dmc_run_block: nsteps must be >= 1");
    if (d->p.external_reduce)
        return fail("qmc_dmc_run_block: ensemble was created for "
                    "external_reduce; drive it with step_local/step_finish");
    HIP_TRY(hipSetDevice(d->eng->device));
    if (dmc_reserve_series(d, nsteps)) return 1;
    d->ser_len = 0;
    if (dmc_fused_branching(d)) {
        // small population: a step costs the latency of its dependent
        // launches.  The bookkeeping of step t rides at the head of step
        // t + 1's branching kernel (same order on the stream as its own
        // launch would have); only the last step of the block launches it.
        FinishArgs pend{};
        bool have = false;
        for (long long t = 0; t < nsteps; ++t) {
            bool pend_done = false;
            int rc = dmc_enqueue_local(d, nullptr, have ? &pend : nullptr,
                                       &pend_done);
            if (rc) {
                // the step before still needs its bookkeeping -- unless this
                // step's branching kernel, which carries it, was enqueued
                // before the failure (then it has been applied, once)
                if (have && !pend_done) {
                    hipLaunchKernelGGL(dmc_finish_kernel, dim3(1), dim3(BLOCK),
                                       0, d->eng->stream, pend);
                    (void)hipGetLastError();   // the first error is reported
                }
                return rc;
            }
            pend = dmc_finish_args(d, nullptr, t);
            have = true;
            d->cur = 1 - d->cur;          // children become the parents
            d->stepped = true;
            d->ser_len = t + 1;
        }
        hipLaunchKernelGGL(dmc_finish_kernel, dim3(1), dim3(BLOCK), 0,
                           d->eng->stream, pend);
        HIP_TRY(hipGetLastError());
    } else {
        for (long long t = 0; t < nsteps; ++t) {
            int rc = dmc_enqueue_local(d, nullptr);
            if (rc) return rc;
            rc = dmc_enqueue_finish(d, nullptr, t);
            if (rc) return rc;
            d->ser_len = t + 1;
        }
    }
    if (energy || weight || num_walkers || ref_energy || accum_energy)
        return qmc_dmc_read_series(d, nsteps, energy, weight, num_walkers,
                                   ref_energy, accum_energy);
    return 0;
}

extern "C" int qmc_dmc_set_estimators(qmc_dmc *d, const qmc_dmc_est_params *p)
{
    if (!d || !p) return fail("qmc_dmc_set_estimators: null argument");
    if (p->num_modes < 0 || p->num_modes > EST_MAXK || p->num_bins < 0 ||
        p->num_bins > EST_MAXK)
        return fail("qmc_dmc_set_estimators: num_modes / num_bins must be in "
                    "[0, 256]");
    HIP_TRY(hipSetDevice(d->eng->device));
    d->est_last_act = 1;
    // Per-walker rows, pure or mixed.  The density kernel accumulates in them
    // in mixed mode as well.  The S(k) kernel does not touch them when mixed:
    // they are allocated all the same, so that the memory footprint and the
    // walker records of such a population stay what they were.
    const DmcEstSpec spec[2] = {
        { p->num_modes, 3, p->ssf_pure, p->ssf_pfw, true },
        { p->num_bins, 1, p->dens_pure, p->dens_pfw, true } };
    return dmc_set_est_slots(d, EST_SSF, 2, spec);
}

// The pair distribution estimator is set on its own: the S(k) / density
// settings and buffers stay as they are (and the other way round).
extern "C" int qmc_dmc_set_pair_dist_estimator(qmc_dmc *d, int32_t num_bins,
                                               int32_t pure, int64_t pfw)
{
    if (!d) return fail("qmc_dmc_set_pair_dist_estimator: null argument");
    if (num_bins < 0 || num_bins > EST_MAXK)
        return fail("qmc_dmc_set_pair_dist_estimator: num_bins must be in "
                    "[0, 256]");
    if (num_bins > 0 && pure && pfw < 1)
        return fail("qmc_dmc_set_pair_dist_estimator: pfw must be >= 1");
    static_assert(PD_EST_MAXN >= 512, "every engine's boson_number fits");
    HIP_TRY(hipSetDevice(d->eng->device));
    // per-walker rows only when pure: the mixed kernel keeps none
    const DmcEstSpec spec = { num_bins, 1, pure ? 1 : 0, pure ? pfw : 1,
                              pure != 0 };
    return dmc_set_est_slots(d, EST_PD, 1, &spec);
}

// The first `nsteps` rows of slot `k` in the last estimator block: what the
// read entry points of the slots that are set on their own share.
static int dmc_read_est_rows(qmc_dmc *d, int k, int64_t nsteps,
                             double *iter_out, const char *entry,
                             const char *estimator)
{
    const std::string who = std::string(entry) + ": ";
    if (!d || !iter_out) return fail(who + "null argument");
    const DmcEstSlot &s = d->est[k];
    if (!s.on())
        return fail(who + "the " + estimator + " estimator is not set");
    if (nsteps <= 0 || nsteps > d->est_block_steps)
        return fail(who + "nsteps outside the last estimator block");
    HIP_TRY(hipSetDevice(d->eng->device));
    return read_doubles(d->eng, iter_out, s.iter, (size_t)nsteps * s.row());
}

extern "C" int qmc_dmc_read_pair_dist(qmc_dmc *d, int64_t nsteps,
                                      double *iter_out)
{
    return dmc_read_est_rows(d, EST_PD, nsteps, iter_out,
                             "qmc_dmc_read_pair_dist", "pair distribution");
}

// The centre-of-mass diffusion estimator (qmc_cmdiff.h) is set on its own as
// well.  Its rows are one double per walker; begin_block zeroes them, which
// moves the time origin to the start of the block.
extern "C" int qmc_dmc_set_cm_diffusion_estimator(qmc_dmc *d, int32_t on)
{
    if (!d) return fail("qmc_dmc_set_cm_diffusion_estimator: null argument");
    HIP_TRY(hipSetDevice(d->eng->device));
    const DmcEstSpec spec = { on ? 1 : 0, 2, 0, 1, true, 1 };
    return dmc_set_est_slots(d, EST_CM, 1, &spec);
}

extern "C" int qmc_dmc_read_cm_diffusion(qmc_dmc *d, int64_t nsteps,
                                         double *iter_out)
{
    return dmc_read_est_rows(d, EST_CM, nsteps, iter_out,
                             "qmc_dmc_read_cm_diffusion",
                             "centre-of-mass diffusion");
}

// The imaginary-time density correlations F(k, tau) (qmc_isf.h) are set on
// their own as well.  A walker's row is what a step puts out, K modes of
// C = num_lags + 2 doubles; the first step of a block writes the origin, so
// begin_block moves it.  K (T + 2) <= ISF_MAXROW keeps a row within 16 indices
// per lane (8 KB per walker and buffer).
extern "C" int qmc_dmc_set_isf_estimator(qmc_dmc *d, int32_t num_modes,
                                         int32_t num_lags, int64_t lag_stride)
{
    if (!d) return fail("qmc_dmc_set_isf_estimator: null argument");
    if (num_modes < 0 || num_modes > 64)
        return fail("qmc_dmc_set_isf_estimator: num_modes must be in [0, 64]");
    if (num_modes > 0) {
        if (num_lags < 1 || num_lags > 64)
            return fail("qmc_dmc_set_isf_estimator: num_lags must be in "
                        "[1, 64]");
        if (lag_stride < 1 || lag_stride > INT32_MAX)
            return fail("qmc_dmc_set_isf_estimator: lag_stride must be in "
                        "[1, 2^31 - 1]");
        if (num_modes * (num_lags + 2) > ISF_MAXROW)
            return fail("qmc_dmc_set_isf_estimator: num_modes * (num_lags + 2) "
                        "must not exceed 1024");
    }
    HIP_TRY(hipSetDevice(d->eng->device));
    const bool on = num_modes > 0;  // (off: the unchecked rest is not read)
    const DmcEstSpec spec = { num_modes, on ? num_lags + 2 : 1, 0,
                              on ? num_lags : 1, true, 0,
                              on ? (int)lag_stride : 1 };
    return dmc_set_est_slots(d, EST_ISF, 1, &spec);
}

extern "C" int qmc_dmc_read_isf(qmc_dmc *d, int64_t nsteps, double *iter_out)
{
    return dmc_read_est_rows(d, EST_ISF, nsteps, iter_out, "qmc_dmc_read_isf",
                             "F(k, tau)");
}

// The one-body density matrix g1(s) (qmc_obdm.h) is set on its own as well:
// mixed, no per-walker rows.  The shift rows live in the slot, not in the
// engine's scratch table, which any qmc_obdm* call on the engine rewrites;
// the slot's drop releases them.  The shifts as given sit behind the rows
// (the shift kernel reads them there).  The estimator is evaluated at the
// steps of a block with step_idx % eval_stride == 0; the rows of the other
// steps stay zero.
extern "C" int qmc_dmc_set_obdm_estimator(qmc_dmc *d, int32_t nshift,
                                          const double *shifts,
                                          int64_t eval_stride)
{
    const char *who = "qmc_dmc_set_obdm_estimator";
    if (!d) return fail(std::string(who) + ": null argument");
    if (nshift < 0 || nshift > EST_MAXK)
        return fail(std::string(who) + ": nshift must be in [0, 256]");
    if (nshift > 0) {
        if (obdm_check_host_shifts(who, nshift, shifts)) return 1;
        if (eval_stride < 1 || eval_stride > INT32_MAX)
            return fail(std::string(who) +
                        ": eval_stride must be in [1, 2^31 - 1]");
    }
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    const bool on = nshift > 0;     // (off: the unchecked rest is not read)
    const DmcEstSpec spec = { nshift, 1, 0, 1, false, 0,
                              on ? (int)eval_stride : 1 };
    if (dmc_set_est_slots(d, EST_OBDM, 1, &spec)) return 1;
    if (!on) return 0;
    DmcEstSlot &s = d->est[EST_OBDM];
    const size_t K = (size_t)nshift;
    int rc = s.tab.alloc(K * (OBDM_SROW + 1));
    if (!rc) {
        double *dsh = s.tab + K * OBDM_SROW;
        hipError_t he = hipMemcpyAsync(dsh, shifts, K * sizeof(double),
                                       hipMemcpyHostToDevice, e->stream);
        if (he != hipSuccess)
            rc = fail(std::string(who) + ": " + hipGetErrorString(he));
        if (!rc) rc = obdm_fill_shift_table(e, nshift, dsh, s.tab);
        if (!rc && (he = hipStreamSynchronize(e->stream)) != hipSuccess)
            rc = fail(std::string(who) + ": " + hipGetErrorString(he));
    }
    if (rc) {
        // nothing is ever on over a missing table (the message stays)
        const std::string msg = g_err;
        const DmcEstSpec off = { 0, 1, 0, 1, false };
        (void)dmc_set_est_slots(d, EST_OBDM, 1, &off);
        return fail(msg);
    }
    return 0;
}

extern "C" int qmc_dmc_read_obdm(qmc_dmc *d, int64_t nsteps, double *iter_out)
{
    return dmc_read_est_rows(d, EST_OBDM, nsteps, iter_out,
                             "qmc_dmc_read_obdm", "one-body density");
}

// The site occupation statistics (qmc_site.h) are set on their own as well:
// K = num_occ + num_dist counts per step, per-walker rows only when pure.  The
// sites are the periods of the lattice, so the supercell must hold a whole
// number of them.
extern "C" int qmc_dmc_set_site_estimator(qmc_dmc *d, int32_t num_occ,
                                          int32_t num_dist, int32_t pure,
                                          int64_t pfw)
{
    const std::string who = "qmc_dmc_set_site_estimator: ";
    if (!d) return fail(who + "null argument");
    const bool on = num_occ != 0;   // (off: the unchecked rest is not read)
    if (on) {
        const double L = d->eng->dm.L;
        if (!(L >= 1.0 && L <= (double)SITE_MAXS && L == std::floor(L)))
            return fail(who + "supercell_size must be an integer in [1, 512] "
                        "(the sites are the periods of the lattice)");
        if (num_occ < 1 || num_dist < 0 || num_dist > (int32_t)L ||
            (int64_t)num_occ + num_dist > EST_MAXK)
            return fail(who + "num_occ >= 1, 0 <= num_dist <= supercell_size "
                        "and num_occ + num_dist <= 256 are needed");
        if (pure && pfw < 1) return fail(who + "pfw must be >= 1");
    }
    HIP_TRY(hipSetDevice(d->eng->device));
    // per-walker rows only when pure: the mixed kernel keeps none
    const DmcEstSpec spec = { on ? num_occ + num_dist : 0, 1,
                              on && pure ? 1 : 0, on && pure ? pfw : 1,
                              on && pure != 0, 0, on ? num_occ : 1 };
    return dmc_set_est_slots(d, EST_SITE, 1, &spec);
}

extern "C" int qmc_dmc_read_site(qmc_dmc *d, int64_t nsteps, double *iter_out)
{
    return dmc_read_est_rows(d, EST_SITE, nsteps, iter_out,
                             "qmc_dmc_read_site", "site occupation");
}

// g1(s) of the walkers of a step: lane groups of est_width(N), the dynamic LDS
// sized from N and K (beyond the default limit at large N: allow_lds).  (The
// caller checks the launch with the reduction that follows.)
static void launch_dmc_obdm(const qmc_engine *e, const double *stab,
                            const EstArgs &a)
{
    const size_t lds = dmc_obdm_lds_bytes(a.n, a.K);
    auto go = [&](auto g) {
        constexpr int G = decltype(g)::value;
        allow_lds(dmc_obdm_kernel<G>, lds);
        hipLaunchKernelGGL(dmc_obdm_kernel<G>, dim3(EST_BLOCKS), dim3(BLOCK),
                           lds, e->stream, e->dm_dev, stab, a);
    };
    switch (est_width(a.n)) {
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    case 32: go(std::integral_constant<int, 32>{}); break;
    default: go(std::integral_constant<int, 64>{}); break;
    }
}

// Evaluate the estimators on the population yielded by the step that has just
// been finished (its parents are the buffer that is not `cur`).
static int dmc_enqueue_estimators(qmc_dmc *d, long long step_idx)
{
    qmc_engine *e = d->eng;
    const int par = 1 - d->cur;
    const int act = (int)(step_idx % 2), prev = 1 - act;
    d->est_last_act = act;
    EstArgs a;
    a.ppos = d->pos[par]; a.ref = d->ref; a.ctl = d->ctl;
    a.maxw = d->maxw; a.step_idx = step_idx; a.n = e->dm.n;
    a.partial = d->est_partial;
    // (in slot order: they take turns at est_partial)
    for (int k = 0; k < EST_SLOTS; ++k) {
        const DmcEstSlot &s = d->est[k];
        if (!s.on()) continue;
        // g1(s): only every s.stride-th step of the block, the first included
        // (the rows of the others stay as begin_block zeroed them)
        if (k == EST_OBDM && step_idx % s.stride != 0) continue;
        // (null where no per-walker rows are kept: the mixed g2, g1)
        a.aux_prev = s.aux[prev]; a.aux_act = s.aux[act];
        a.K = s.K; a.pure = s.pure; a.pfw = s.pfw;
        a.scale2 = 0.0;
        switch (k) {
        case EST_SSF:
            a.scale = 4.0 / e->dm.L;
            launch_ssf(e, a);
            break;
        case EST_DENS:
            a.scale = e->dm.L / (double)s.K;      // bin size
            hipLaunchKernelGGL(dmc_density_kernel, dim3(EST_BLOCKS),
                               dim3(BLOCK), 0, e->stream, a);
            break;
        case EST_PD:
            a.scale = e->dm.L;
            a.scale2 = (double)s.K / (0.5 * e->dm.L);   // as pair_dist_launch
            hipLaunchKernelGGL(dmc_pair_dist_kernel, dim3(EST_BLOCKS),
                               dim3(BLOCK), 0, e->stream, a);
            break;
        case EST_CM:
            // the children of the step sit in the buffer that is `cur` now
            a.scale = e->dm.L;
            a.cpos = d->pos[d->cur];
            hipLaunchKernelGGL(dmc_cm_diffusion_kernel, dim3(EST_BLOCKS),
                               dim3(BLOCK), 0, e->stream, a);
            a.cpos = nullptr;
            break;
        case EST_OBDM:
            a.scale = 0.0;
            launch_dmc_obdm(e, s.tab, a);
            break;
        case EST_SITE:
            a.scale = e->dm.L;
            a.scale2 = 0.5 * (1.0 - e->dm.z_a);   // half a barrier
            a.stride = s.stride;                  // P (qmc_site.h)
            hipLaunchKernelGGL(dmc_site_kernel, dim3(EST_BLOCKS), dim3(BLOCK),
                               0, e->stream, a);
            a.stride = 1;
            break;
        default:
            a.scale = 4.0 / e->dm.L;              // as S(k)
            a.stride = s.stride;
            hipLaunchKernelGGL(dmc_isf_kernel, dim3(EST_BLOCKS), dim3(BLOCK),
                               0, e->stream, a);
            a.stride = 1;
        }
        const int row = (int)s.row();
        hipLaunchKernelGGL(est_reduce_kernel, dim3((row + 31) / 32), dim3(256),
                           0, e->stream, d->est_partial, EST_BLOCKS, row,
                           a.divisor(), s.iter + (size_t)step_idx * row);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// Start an estimator block of `nsteps` steps: per-block resets of the
// forward-walking buffers and of the per-step outputs (qmc_base/dmc.py:897-909).
static int dmc_est_begin_block(qmc_dmc *d, long long nsteps)
{
    qmc_engine *e = d->eng;
    for (DmcEstSlot &s : d->est) {
        if (!s.on()) continue;
        const size_t need = (size_t)nsteps * s.row();
        if (s.iter.reserve(need)) return 1;
        HIP_TRY(hipMemsetAsync(s.iter, 0, need * 8, e->stream));
        for (int k = 0; k < 2; ++k)
            if (s.aux[k])
                HIP_TRY(hipMemsetAsync(s.aux[k], 0,
                                       (size_t)d->maxw * s.aux_row() * 8,
                                       e->stream));
    }
    d->est_block_steps = nsteps;
    d->est_last_act = 1;
    return 0;
}

extern "C" int qmc_dmc_run_block_est(qmc_dmc *d, int64_t nsteps,
                                     int eval_estimators, double *energy,
                                     double *weight, uint64_t *num_walkers,
                                     double *ref_energy, double *accum_energy,
                                     double *iter_ssf, double *iter_density)
{
    if (!d) return fail("qmc_dmc_run_block_est: null argument");
    if (nsteps <= 0) return fail("qmc_dmc_run_block_est: nsteps must be >= 1");
    if (d->p.external_reduce)
        return fail("qmc_dmc_run_block_est: ensemble was created for "
                    "external_reduce; drive it with est_begin_block / "
                    "step_local / step_finish / step_estimators");
    if (!d->any_est())
        return qmc_dmc_run_block(d, nsteps, energy, weight, num_walkers,
                                 ref_energy, accum_energy);
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    if (dmc_reserve_series(d, nsteps)) return 1;
    if (dmc_est_begin_block(d, nsteps)) return 1;
    d->ser_len = 0;
    for (long long t = 0; t < nsteps; ++t) {
        int rc = dmc_enqueue_local(d, nullptr);
        if (rc) return rc;
        rc = dmc_enqueue_finish(d, nullptr, t);
        if (rc) return rc;
        d->ser_len = t + 1;
        if (eval_estimators) {
            rc = dmc_enqueue_estimators(d, t);
            if (rc) return rc;
        }
    }
    double *const host[2] = { iter_ssf, iter_density };
    for (int k = 0; k < 2; ++k)
        if (host[k] && d->est[k].on())
            HIP_TRY(hipMemcpyAsync(host[k], d->est[k].iter,
                                   (size_t)nsteps * d->est[k].row() * 8,
                                   hipMemcpyDeviceToHost, e->stream));
    return qmc_dmc_read_series(d, nsteps, energy, weight, num_walkers,
                               ref_energy, accum_energy);
}

// Split-step counterparts (multi-GPU, external_reduce): the caller opens an
// estimator block, calls step_estimators after every step_finish of a kept
// block, and sums the per-rank outputs (linear in the walkers) across ranks.
extern "C" int qmc_dmc_est_begin_block(qmc_dmc *d, int64_t nsteps)
{
    if (!d) return fail("qmc_dmc_est_begin_block: null argument");
    if (!d->any_est())
        return fail("qmc_dmc_est_begin_block: no estimators are set");
    if (nsteps <= 0) return fail("qmc_dmc_est_begin_block: nsteps must be >= 1");
    HIP_TRY(hipSetDevice(d->eng->device));
    return dmc_est_begin_block(d, nsteps);
}

extern "C" int qmc_dmc_step_estimators(qmc_dmc *d, int64_t step_idx)
{
    if (!d) return fail("qmc_dmc_step_estimators: null argument");
    if (!d->any_est())
        return fail("qmc_dmc_step_estimators: no estimators are set");
    if (step_idx < 0 || step_idx >= d->est_block_steps)
        return fail("qmc_dmc_step_estimators: step index outside the block "
                    "opened by qmc_dmc_est_begin_block");
    if (!d->stepped)
        return fail("qmc_dmc_step_estimators: no time step has run yet");
    HIP_TRY(hipSetDevice(d->eng->device));
    return dmc_enqueue_estimators(d, step_idx);
}

extern "C" int qmc_dmc_est_iter_dev(qmc_dmc *d, double **iter_ssf,
                                    double **iter_density)
{
    if (!d) return fail("qmc_dmc_est_iter_dev: null argument");
    // (a slot that is off holds no buffer)
    if (iter_ssf) *iter_ssf = d->est[EST_SSF].iter.get();
    if (iter_density) *iter_density = d->est[EST_DENS].iter.get();
    return 0;
}

extern "C" int qmc_dmc_est_rows_dev(qmc_dmc *d, int32_t slot, double **rows,
                                    int64_t *row_doubles)
{
    if (!d || !rows || !row_doubles)
        return fail("qmc_dmc_est_rows_dev: null argument");
    if (slot < 0 || slot >= EST_SLOTS)
        return fail("qmc_dmc_est_rows_dev: no such estimator slot");
    const DmcEstSlot &s = d->est[slot];
    // (a slot that is off holds no buffer; one that is on has none before its
    // first estimator block)
    *rows = s.on() ? s.iter.get() : nullptr;
    *row_doubles = s.on() ? (int64_t)s.row() : 0;
    return 0;
}

extern "C" int qmc_dmc_step_local(qmc_dmc *d, double *partial_dev)
{
    if (!d || !partial_dev) return fail("qmc_dmc_step_local: null argument");
    HIP_TRY(hipSetDevice(d->eng->device));
    return dmc_enqueue_local(d, partial_dev);
}

extern "C" int qmc_dmc_step_finish(qmc_dmc *d, const double *total_dev)
{
    if (!d || !total_dev) return fail("qmc_dmc_step_finish: null argument");
    HIP_TRY(hipSetDevice(d->eng->device));
    if (d->ser_len >= d->ser_cap) {
        // grow geometrically, keeping what was recorded
        long long ncap = d->ser_cap ? d->ser_cap * 2 : 1024;
        DevBuf<double> oe(std::move(d->ser_e)), ow(std::move(d->ser_w)),
            orf(std::move(d->ser_ref)), oa(std::move(d->ser_acc));
        DevBuf<unsigned long long> on(std::move(d->ser_nw));
        long long olen = d->ser_len;
        d->ser_cap = 0;
        if (dmc_reserve_series(d, ncap)) return 1;
        if (oe) {
            hipStream_t s = d->eng->stream;
            HIP_TRY(hipMemcpyAsync(d->ser_e, oe, olen * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(d->ser_w, ow, olen * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(d->ser_ref, orf, olen * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(d->ser_acc, oa, olen * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(d->ser_nw, on, olen * 8, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        // (the old series go here, after the copies)
    }
    int rc = dmc_enqueue_finish(d, total_dev, d->ser_len);
    if (rc) return rc;
    d->ser_len += 1;
    return 0;
}

extern "C" int qmc_dmc_num_walkers(qmc_dmc *d, int64_t *nw)
{
    if (!d || !nw) return fail("qmc_dmc_num_walkers: null argument");
    HIP_TRY(hipSetDevice(d->eng->device));
    DmcCtl c;
    HIP_TRY(hipMemcpyAsync(&c, d->ctl, sizeof(c), hipMemcpyDeviceToHost,
                           d->eng->stream));
    HIP_TRY(hipStreamSynchronize(d->eng->stream));
    *nw = c.prev_nw;
    return 0;
}

extern "C" int qmc_dmc_get_state(qmc_dmc *d, double *confs, double *energy,
                                 double *weight, uint8_t *mask,
                                 int64_t *cloning_ref, double *scalars)
{
    if (!d) return fail("qmc_dmc_get_state: null argument");
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)e->dm.n, W = (size_t)d->maxw;
    DmcCtl c;
    HIP_TRY(hipMemcpyAsync(&c, d->ctl, sizeof(c), hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const long long nw = d->stepped ? c.nw : c.prev_nw;
    std::vector<long long> href;
    if (cloning_ref) {
        href.assign(W, 0);
        if (d->stepped)
            HIP_TRY(hipMemcpy(href.data(), d->ref, W * sizeof(long long),
                              hipMemcpyDeviceToHost));
    }
    if (confs) {
        memset(confs, 0, W * 2 * n * sizeof(double));
        if (d->stepped) {
            // yielded walkers are the parents selected by the cloning table;
            // the parent buffer of the last step is the one that is not `cur`
            const int par = 1 - d->cur;
            DevBuf<double> tmp;
            if (tmp.alloc((size_t)nw * 2 * n)) return 1;
            long long tot = nw * (long long)n;
            hipLaunchKernelGGL(dmc_gather_state_kernel,
                               dim3((unsigned)((tot + 255) / 256)), dim3(256),
                               0, e->stream, d->pos[par], d->drift[par],
                               d->label[par], d->ref, nw, (int)n, tmp);
            HIP_TRY(hipMemcpyAsync(confs, tmp, (size_t)nw * 2 * n * 8,
                                   hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        } else {
            std::vector<double> hp((size_t)nw * n), hd((size_t)nw * n);
            std::vector<unsigned short> hl((size_t)nw * n);
            HIP_TRY(hipMemcpy(hp.data(), d->pos[d->cur], hp.size() * 8,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(hd.data(), d->drift[d->cur], hd.size() * 8,
                              hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(hl.data(), d->label[d->cur], hl.size() * 2,
                              hipMemcpyDeviceToHost));
            for (size_t s = 0; s < (size_t)nw; ++s)
                for (size_t i = 0; i < n; ++i) {
                    confs[(s * 2 + 0) * n + hl[s * n + i]] = hp[s * n + i];
                    confs[(s * 2 + 1) * n + hl[s * n + i]] = hd[s * n + i];
                }
        }
    }
    if (energy) {
        memset(energy, 0, W * sizeof(double));
        // after a step eslot[s] holds the parent's energy (actual.energy)
        HIP_TRY(hipMemcpy(energy, d->stepped ? d->eslot : d->energy[d->cur],
                          (size_t)nw * 8, hipMemcpyDeviceToHost));
    }
    if (weight) {
        for (size_t s = 0; s < W; ++s) weight[s] = s < (size_t)nw ? 1.0 : 0.0;
        if (!d->stepped && d->init_weight.size() == (size_t)nw) {
            std::copy(d->init_weight.begin(), d->init_weight.end(), weight);
        } else if (!d->stepped) {
            HIP_TRY(hipMemcpy(weight, d->weight[d->cur], (size_t)nw * 8,
                              hipMemcpyDeviceToHost));
            for (size_t s = 0; s < (size_t)nw; ++s) weight[s] = std::exp(weight[s]);
        }
    }
    if (mask)
        for (size_t s = 0; s < W; ++s) mask[s] = s < (size_t)nw ? 0 : 1;
    if (cloning_ref)
        for (size_t s = 0; s < W; ++s) cloning_ref[s] = (int64_t)href[s];
    if (scalars) {
        scalars[0] = c.e_t; scalars[1] = c.w_t; scalars[2] = c.ref_energy;
        scalars[3] = c.total_weight != 0.0 ? c.total_energy / c.total_weight
                                           : 0.0;
        scalars[4] = (double)nw;
    }
    return 0;
}

static_assert(REC_BASE_SEGS + EST_SLOTS <= REC_MAX_SEGS,
              "a record segment per estimator slot");

// The segment table of the walker records, from the slots as they are now.
static WalkerRecArgs walker_rec_args(qmc_dmc *d, long long first,
                                     long long count)
{
    WalkerRecArgs a;
    const int n = d->eng->dm.n, cur = d->cur;
    int k = 0, rec = 0;
    auto add = [&](void *base, int width, int kind) {
        a.seg[k].base = base; a.seg[k].width = width; a.seg[k].kind = kind;
        rec += width;
        ++k;
    };
    add(d->pos[cur].get(), n, REC_F64);
    add(d->drift[cur].get(), n, REC_F64);
    add(d->label[cur].get(), n, REC_U16);
    a.e_off = rec;
    add(d->energy[cur].get(), 1, REC_F64);
    add(d->weight[cur].get(), 1, REC_F64);
    // the rows the next estimator step reads as "previous": those of S(k) and
    // the density always, those of the other slots with record_rows (a slot
    // that is off or keeps no rows -- the mixed g2 and site statistics, g1 --
    // adds nothing)
    for (int e = 0; e < EST_SLOTS; ++e) {
        const DmcEstSlot &s = d->est[e];
        double *rows = s.aux[d->est_last_act].get();
        if (!s.on() || !rows || (e > EST_DENS && !d->record_rows)) continue;
        add(rows, (int)s.aux_row(), REC_F64);
    }
    for (int j = k; j < REC_MAX_SEGS; ++j) a.seg[j] = RecSeg{ nullptr, 0, 0 };
    a.nseg = k; a.rec = rec;
    a.eslot = d->eslot;
    a.first = first; a.count = count;
    return a;
}

// One wavefront per record; enough blocks to fill the device, the rest by
// the grid stride.
static unsigned walker_rec_blocks(long long count)
{
    const long long want = (count + REC_WAVES - 1) / REC_WAVES;
    return (unsigned)std::min<long long>(want, 4096);
}

extern "C" int qmc_dmc_set_record_rows(qmc_dmc *d, int32_t on)
{
    if (!d) return fail("qmc_dmc_set_record_rows: null argument");
    d->record_rows = on != 0;
    return 0;
}

extern "C" int qmc_dmc_walker_record_size(qmc_dmc *d, int64_t *doubles)
{
    if (!d || !doubles) return fail("qmc_dmc_walker_record_size: null argument");
    *doubles = walker_rec_args(d, 0, 0).rec;
    return 0;
}

extern "C" int qmc_dmc_export_walkers(qmc_dmc *d, int64_t first, int64_t count,
                                      double *buf_dev)
{
    if (!d || !buf_dev) return fail("qmc_dmc_export_walkers: null argument");
    if (count <= 0) return 0;
    if (first < 0 || first + count > d->maxw)
        return fail("qmc_dmc_export_walkers: slot range outside the population");
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    const WalkerRecArgs a = walker_rec_args(d, first, count);
    hipLaunchKernelGGL(pack_walkers_kernel, dim3(walker_rec_blocks(count)),
                       dim3(64 * REC_WAVES), 0, e->stream, a, buf_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Stream-ordered: nothing here reads the device back.  The caller knows the
// population size (it gathered the counts to plan the rebalance).
extern "C" int qmc_dmc_import_walkers_at(qmc_dmc *d, int64_t first,
                                         int64_t count, const double *buf_dev)
{
    if (!d || !buf_dev) return fail("qmc_dmc_import_walkers_at: null argument");
    if (count <= 0) return 0;
    if (first < 0 || first + count > d->maxw)
        return fail("qmc_dmc_import_walkers_at: population would exceed "
                    "max_num_walkers");
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    d->init_weight.clear();
    const WalkerRecArgs a = walker_rec_args(d, first, count);
    hipLaunchKernelGGL(unpack_walkers_kernel, dim3(walker_rec_blocks(count)),
                       dim3(64 * REC_WAVES), 0, e->stream, a, buf_dev);
    // imported slots must not consume a spare normal stored for another walker
    hipLaunchKernelGGL(dmc_set_nw_kernel, dim3(1), dim3(64), 0, e->stream,
                       d->ctl, (long long)(first + count), (long long)first);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int qmc_dmc_set_num_walkers(qmc_dmc *d, int64_t nw)
{
    if (!d) return fail("qmc_dmc_set_num_walkers: null argument");
    if (nw < 0 || nw > d->maxw)
        return fail("qmc_dmc_set_num_walkers: bad population size");
    d->init_weight.clear();
    qmc_engine *e = d->eng;
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(dmc_set_nw_kernel, dim3(1), dim3(64), 0, e->stream,
                       d->ctl, (long long)nw, (long long)nw);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int qmc_dmc_import_walkers(qmc_dmc *d, int64_t count,
                                      const double *buf_dev)
{
    if (!d || !buf_dev) return fail("qmc_dmc_import_walkers: null argument");
    if (count <= 0) return 0;
    int64_t nw = 0;
    int rc = qmc_dmc_num_walkers(d, &nw);       // synchronises
    if (rc) return rc;
    if (nw + count > d->maxw)
        return fail("qmc_dmc_import_walkers: population would exceed "
                    "max_num_walkers");
    return qmc_dmc_import_walkers_at(d, nw, count, buf_dev);
}

extern "C" int qmc_dmc_truncate(qmc_dmc *d, int64_t new_nw)
{
    if (!d) return fail("qmc_dmc_truncate: null argument");
    HIP_TRY(hipSetDevice(d->eng->device));
    int64_t nw = 0;
    int rc = qmc_dmc_num_walkers(d, &nw);       // synchronises
    if (rc) return rc;
    if (new_nw < 0 || new_nw > nw)
        return fail("qmc_dmc_truncate: bad population size");
    return qmc_dmc_set_num_walkers(d, new_nw);
}
