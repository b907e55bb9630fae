// qmc_obdm.h -- one-body density matrix g1(s) of the Bijl-Jastrow model
// (qmc_base/jastrow/model.py:859-965: ith_one_body_density, one_body_density).
//
//   ith(i, s) = exp( [log f1(z_i + s) - log f1(z_i)]
//                  + sum_{j != i} [log f2(|d(z_i + s, z_j)|) - log f2(|d(z_i, z_j)|)] )
//   g1(s)     = (1/N) sum_i ith(i, s)
//
// for nconf configurations and nshift shifts: nconf * nshift * N * (N - 1)
// shifted pair factors, the expensive estimator of the model.
//
// Layout.  One wavefront per (configuration, chunk of shifts).  The wavefront
// first publishes the per-particle angle tables of its configuration in LDS
// ({sin, cos}(pi z / L), {sin, cos}(k2 z), of the image inside the box: the
// same four numbers `PTab` holds) and computes, once, the logarithm of the
// UNSHIFTED row product of every particle (the denominator does not depend on
// the shift).  Then groups of G = min(64, 2^ceil(log2 N)) lanes take one shift
// each, lane = own particle i (N > 64: ceil(N / 64) passes), and every lane
// carries OBDM_U = 2 shifts at once, so that one broadcast read of a partner's
// table entry from LDS serves two pair factors.  The partner loop runs over all
// j in the caller's order; the entry is wave-uniform.  Nothing here is
// symmetric in (i, j), so no rows are rotated and no particle order is
// assumed: position-sorted rows of a VMC ensemble and caller-ordered rows give
// the same g1 (only the `ith` output follows the order of the row).
//
// No transcendental per pair.  The own particle moved by s has the tables
//   sin/cos(pi (z_i + s) / L), sin/cos(k2 (z_i + s))
// by one angle addition each from its own entry and the shift's entry
// (obdm_shift_kernel: the shift reduced to [-L/2, L/2], one sincos pair per
// shift for the whole batch); where z_i + s leaves [0, L) the image inside the
// box is taken (sign flip of the first pair, rotation by k2 L of the second),
// so that own and partner are both inside the box and the separation is in
// (-L, L), the situation `short_generic` handles.  Per pair:
//   S = sin(pi D / L), C = cos(pi D / L) by angle subtraction;
//   class  r < rm  <=>  |S| < sin(pi rm / L);   wrapped <=> C < 0;
//   long:  f2 = |S|^beta;   short: f2 = |a_m| cos(k2 r - phi)
//          = |a_m| (|sin k2 d| sin phi + cos k2 d cos phi).
// An own particle in the lower half of the box can only meet partners wrapped
// one way, one in the upper half only the other way, so the own k2-table
// rotated by -+k2 L is prepared once per (lane, shift) and a wrapped pair only
// selects it.
//
// The short / long class of the shifted pair changes lane by lane and shift by
// shift (with a cutoff of a quarter of the box half of all pairs are short), so
// it cannot be hoisted like the ZCLASS masks of the energy pass.  It is kept a
// SELECT: both factors are formed for every pair and two conditional moves
// route them into the long and the short product.  An exec-masked branch would
// run both sides in nearly every wavefront anyway and add its mask arithmetic
// (ISA census: DESIGN section 4).
//
// Products, not sums of logarithms: the long and the short factors are
// multiplied up separately (the long ones take the power beta at the end), the
// binary exponent is split off both products every OBDM_FOLD partners (q_fold),
// so neither can leave the fp64 range at any N, and each (lane, shift) takes
// two logarithms and one exponential at the end.  The shifted and the
// unshifted row go through the same code (obdm_rows / obdm_row_log), so that a
// zero shift reproduces the denominator bit for bit and g1(0) is exactly 1.
//
// fp64 only: a float row product underflows, and the estimator is a ratio of
// two such products.  qmc_engine_set_fast_math does not apply to this kernel.
#pragma once

#include "qmc_device.h"
#include "qmc_kernels_misc.h"
// (the pair arithmetic of a row: obdm_log_f1, obdm_wrap_tab, obdm_rows,
// obdm_row_log, shared with the single-particle VMC sweeps)
#include "qmc_obdm_rows.h"

static constexpr int OBDM_U = 2;        // shifts carried by a lane
static constexpr int OBDM_SROW = 8;     // doubles per row of the shift table
// LDS doubles per particle: the four table entries, the position as given
// (one-body factor), its image in the box, log of the unshifted row
static constexpr int OBDM_LDS_PER_PARTICLE = 7;

// Row of the shift table: {s, sin, cos(pi s' / L), sin, cos(k2 s'), s'}, s' the
// shift reduced to [-L/2, L/2] (the pair factors have the period L; the
// one-body factor takes the shift as given).
__global__ void __launch_bounds__(64)
obdm_shift_kernel(const DevModel *__restrict__ mp,
                  const double *__restrict__ shifts, int nshift,
                  double *__restrict__ stab)
{
    const DevModel &m = *mp;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nshift) return;
    const double s = shifts[k];
    const double sr = fma(-m.L, rint(s / m.L), s);
    double s1, c1, s2, c2;
    sincos_halfpi(sr * m.two_over_L, s1, c1);
    sincos_halfpi(sr * m.k2_2pi, s2, c2);
    double *row = stab + (size_t)k * OBDM_SROW;
    row[0] = s; row[1] = s1; row[2] = c1; row[3] = s2; row[4] = c2;
    row[5] = sr; row[6] = 0.0; row[7] = 0.0;
}

struct ObdmArgs {
    const double *pos;     // [nconf][N]
    const double *stab;    // [nshift][OBDM_SROW]
    double *g1;            // [nconf][nshift]
    double *ith;           // [nconf][nshift][N] or null
    long long nconf;
    int nshift;
    int chunk;             // shifts per wavefront (grid.y chunks)
};

// ---- the stages of one configuration, run by one wavefront ---------------
// obdm_kernel (a batch of configurations) and dmc_obdm_kernel (the walkers of
// a DMC step) call the same three stages, so a configuration's g1 carries the
// same bits from both.  The stages share the configuration's LDS region; the
// caller orders them (stage 2 reads what stage 1 wrote, stage 3 what both
// wrote): a block barrier where the block is the wavefront, wave-level fences
// where the region belongs to one wavefront of a larger block.  Every lane of
// the wavefront runs every stage: indices are clamped and stores masked.
struct ObdmLds {
    double *tab;       // [n][4] angle tables
    double *zraw;      // positions as given
    double *zbox;      // their images in [0, L)
    double *den;       // log of the unshifted row
    __device__ ObdmLds(double *base, int n)
        : tab(base), zraw(base + 4 * n), zbox(base + 5 * n), den(base + 6 * n)
    {
    }
};

// Stage 1: the tables of the configuration `row`.
__device__ __forceinline__ void obdm_fill_tables(const DevModel &m,
                                                 const double *__restrict__ row,
                                                 const ObdmLds &l, int lane)
{
    const int n = m.n;
    const int npass = (n + 63) / 64;
    for (int p = 0; p < npass; ++p) {
        const int i = lane + 64 * p;
        const double z1 = (i < n) ? row[i] : 0.0;
        const double z = wrap_box(z1, m.L);
        PTab t;
        sincos_halfpi(z * m.two_over_L, t.s, t.c);
        sincos_halfpi(z * m.k2_2pi, t.su, t.cu);
        if (i < n) {
            l.tab[4 * i] = t.s; l.tab[4 * i + 1] = t.c;
            l.tab[4 * i + 2] = t.su; l.tab[4 * i + 3] = t.cu;
            l.zraw[i] = z1; l.zbox[i] = z;
        }
    }
}

// Stage 2: the unshifted rows, once per configuration.
__device__ __forceinline__ void obdm_unshifted_rows(const DevModel &m,
                                                    const ObdmLds &l, int lane)
{
    const int n = m.n;
    const double *tab = l.tab;
    const bool pairs = !m.is_ideal, onebody = !m.is_free;
    const int npass = (n + 63) / 64;
    for (int p = 0; p < npass; ++p) {
        const int i = lane + 64 * p;
        const int ic = min(i, n - 1);
        PTab own[1];
        own[0].s = tab[4 * ic]; own[0].c = tab[4 * ic + 1];
        own[0].su = tab[4 * ic + 2]; own[0].cu = tab[4 * ic + 3];
        const int self[1] = { ic };
        ObdmRow r[1];
        r[0].PL = 0.5; r[0].PS = 0.5; r[0].eL = 1; r[0].eS = 1; r[0].cnt = 0;
        if (pairs) obdm_rows<1>(m, tab, n, own, self, r);
        const double lf = onebody ? obdm_log_f1(m, l.zraw[ic]) : 0.0;
        const double v = obdm_row_log(m, r[0], lf);
        if (i < n) l.den[i] = v;
    }
}

// Stage 3: the shifts [k0, k1) of the table `stab` (nshift rows).  Groups of
// G lanes take one shift each and every lane carries OBDM_U of them;
// out.ith(k, i, v) gets the ratio of particle i at shift k from its lane,
// out.g1(k, v) the mean over the particles from the leader of the group.
template <int G, typename Out>
__device__ __forceinline__ void obdm_shift_loop(const DevModel &m,
                                                const ObdmLds &l, int lane,
                                                const double *__restrict__ stab,
                                                int nshift, int k0, int k1,
                                                Out out)
{
    const int n = m.n;
    const double *tab = l.tab, *zraw = l.zraw, *zbox = l.zbox, *den = l.den;
    const bool pairs = !m.is_ideal, onebody = !m.is_free;
    const int npass = (n + 63) / 64;
    constexpr int GPW = 64 / G;                 // shift groups of a wavefront
    const int grp = lane / G, gl = lane % G;
    const double inv_guard = 700.0;             // domain of exp_bounded
    for (int kb = k0; kb < k1; kb += GPW * OBDM_U) {
        int ks[OBDM_U];
        double sh[OBDM_U][OBDM_SROW - 2];
#pragma unroll
        for (int u = 0; u < OBDM_U; ++u) {
            ks[u] = kb + GPW * u + grp;
            const double *srow =
                stab + (size_t)min(ks[u], nshift - 1) * OBDM_SROW;
#pragma unroll
            for (int q = 0; q < OBDM_SROW - 2; ++q) sh[u][q] = srow[q];
        }
        double acc[OBDM_U];
#pragma unroll
        for (int u = 0; u < OBDM_U; ++u) acc[u] = 0.0;
        for (int p = 0; p < npass; ++p) {
            const int i = gl + 64 * p;
            const int ic = min(i, n - 1);
            const double es = tab[4 * ic], ec = tab[4 * ic + 1];
            const double esu = tab[4 * ic + 2], ecu = tab[4 * ic + 3];
            const double zb = zbox[ic], zr = zraw[ic], dn = den[ic];
            PTab own[OBDM_U];
            int self[OBDM_U];
#pragma unroll
            for (int u = 0; u < OBDM_U; ++u) {
                const double s1 = sh[u][1], c1 = sh[u][2];
                const double s2 = sh[u][3], c2 = sh[u][4];
                // angle additions, then the image inside the box
                double ts = fma(es, c1, ec * s1), tc = fma(ec, c1, -(es * s1));
                double tsu = fma(esu, c2, ecu * s2);
                double tcu = fma(ecu, c2, -(esu * s2));
                const double zt = zb + sh[u][5];
                const bool over = zt >= m.L, under = zt < 0.0;
                if (over | under) {
                    // one period down (over) or up (under): the first pair
                    // changes sign, the second turns by -+k2 L
                    const double t = over ? m.sth_signed : -m.sth_signed;
                    const double rs = fma(tsu, m.cth, -(tcu * t));
                    const double rc = fma(tcu, m.cth, tsu * t);
                    ts = -ts; tc = -tc; tsu = rs; tcu = rc;
                }
                own[u].s = ts; own[u].c = tc; own[u].su = tsu; own[u].cu = tcu;
                self[u] = ic;
            }
            ObdmRow r[OBDM_U];
#pragma unroll
            for (int u = 0; u < OBDM_U; ++u) {
                r[u].PL = 0.5; r[u].PS = 0.5; r[u].eL = 1; r[u].eS = 1;
                r[u].cnt = 0;
            }
            if (pairs) obdm_rows<OBDM_U>(m, tab, n, own, self, r);
#pragma unroll
            for (int u = 0; u < OBDM_U; ++u) {
                const double lf =
                    onebody ? obdm_log_f1(m, zr + sh[u][0]) : 0.0;
                double x = obdm_row_log(m, r[u], lf) - dn;
                x = fmin(fmax(x, -inv_guard), inv_guard);
                const double v = exp_bounded(x);
                const bool ok = (i < n) & (ks[u] < k1);
                if (ok) {
                    acc[u] += v;
                    out.ith(ks[u], i, v);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < OBDM_U; ++u) {
            // sum over the lanes of the group: xor butterfly, a fixed order
            double t = acc[u];
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1)
                t += __shfl_xor(t, off, 64);
            if (gl == 0 && ks[u] < k1) out.g1(ks[u], t / (double)n);
        }
    }
}

// G: lanes of a shift group (8, 16, 32, 64; N <= G below 64).
template <int G>
__global__ void __launch_bounds__(64)
obdm_kernel(const DevModel *__restrict__ mp, ObdmArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    const int n = m.n;
    const ObdmLds l(smem, n);
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;

    obdm_fill_tables(m, a.pos + c * n, l, lane);
    __syncthreads();
    obdm_unshifted_rows(m, l, lane);
    __syncthreads();

    const int k0 = blockIdx.y * a.chunk;
    const int k1 = min(a.nshift, k0 + a.chunk);
    struct Out {
        double *g1v, *ithv;
        int n;
        __device__ __forceinline__ void ith(int k, int i, double v) const
        {
            if (ithv) ithv[(size_t)k * n + i] = v;
        }
        __device__ __forceinline__ void g1(int k, double v) const { g1v[k] = v; }
    };
    const Out out{ a.g1 + (size_t)c * a.nshift,
                   a.ith ? a.ith + (size_t)c * a.nshift * n : nullptr, n };
    obdm_shift_loop<G>(m, l, lane, a.stab, a.nshift, k0, k1, out);
}

// ---- g1(s) as a DMC block estimator --------------------------------------
// The mixed g1 of the yielded walkers of a time step, in the frame of the
// other DMC estimators (qmc_kernels_misc.h: EstArgs, est_reduce_kernel).
// Walker s carries the configuration of its parent, ppos[ref[s]]:
//
//   iter[t][k] = sum_{s < nw_t} g1_s(shift_k)        (a.K shifts, divisor 1)
//
// Mixed only (g1 is non-local: forward walking does not apply), the walkers
// unweighted as in the mixed g2, no per-walker rows.
//
// One wavefront per walker slot, grid-striding over the live slots.  Per walker
// it runs the three stages above on an LDS region of its own
// (OBDM_LDS_PER_PARTICLE * N doubles), all K shifts in one go.  The region is
// touched by that wavefront alone, so wave-level fences and wave barriers order
// the stages (as dmc_pair_dist_kernel); the wavefronts of a block go round the
// slot loop different numbers of times, so no block barrier may stand in it.
// A wave-private LDS row of K running sums takes the walkers in the wave's
// slot order: sum[k] is read and written by one lane only, the leader of the
// group that owns shift k, the same for every walker.  est_block_sum adds up
// the wavefronts of a block (its barrier is the only one of the block),
// est_reduce_kernel the blocks.  No floating-point atomics: the same bits on
// every run.  fp64 whatever fast_math says.
//
// Dynamic LDS: [NWAVE][K] sums, then [NWAVE][7 N] tables -- 120 KB at N = 512,
// K = 256 (one block per CU then).  The model and the shift table travel
// beside EstArgs, whose layout the other estimators share.
static size_t dmc_obdm_lds_bytes(int n, int K)
{
    return (size_t)(BLOCK / 64) * ((size_t)K + (size_t)n * OBDM_LDS_PER_PARTICLE) *
           sizeof(double);
}

template <int G>
__global__ void __launch_bounds__(BLOCK)
dmc_obdm_kernel(const DevModel *__restrict__ mp,
                const double *__restrict__ stab, EstArgs a)
{
    constexpr int NWAVE = BLOCK / 64;
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    const int n = m.n, K = a.K;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *sum = smem + (size_t)wave * K;                      // [NWAVE][K]
    const ObdmLds l(smem + (size_t)NWAVE * K +
                        (size_t)wave * n * OBDM_LDS_PER_PARTICLE, n);
    for (int k = lane; k < K; k += 64) sum[k] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    struct Out {
        double *sum;
        __device__ __forceinline__ void ith(int, int, double) const {}
        __device__ __forceinline__ void g1(int k, double v) const { sum[k] += v; }
    };
    const Out out{ sum };
    const long long nw = a.ctl->nw;
    const long long wstride = (long long)gridDim.x * NWAVE;
    for (long long s = (long long)blockIdx.x * NWAVE + wave; s < nw;
         s += wstride) {
        const long long par = a.ref[s];
        obdm_fill_tables(m, a.ppos + (size_t)par * n, l, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        obdm_unshifted_rows(m, l, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        obdm_shift_loop<G>(m, l, lane, stab, K, 0, K, out);
        __builtin_amdgcn_wave_barrier();    // the tables are rewritten next
    }
    est_block_sum(smem, K, K, a.partial);
}

// sums[k][0..1] (+)= sum_c w_c g1[c][k], sum_c w_c g1[c][k]^2 and, in the
// block after the last shift, wsum (+)= sum_c w_c (w null: 1).  One block per
// shift; thread t adds configurations t, t + 256, ... in index order, the 256
// partial sums are added by a fixed tree: the same bits on every run (no
// floating-point atomics).  `accumulate` adds to what is there (tiles of a
// large batch arrive in order).
__global__ void __launch_bounds__(256)
obdm_reduce_kernel(const double *__restrict__ g1, const double *__restrict__ w,
                   long long nconf, int nshift, int accumulate,
                   double *__restrict__ sums, double *__restrict__ wsum)
{
    __shared__ double s0[256], s1[256];
    const int k = blockIdx.x, t = threadIdx.x;
    double a0 = 0.0, a1 = 0.0;
    if (k < nshift) {
        for (long long c = t; c < nconf; c += 256) {
            const double g = g1[(size_t)c * nshift + k];
            const double wg = w ? w[c] * g : g;
            a0 += wg;
            a1 = fma(wg, g, a1);
        }
    } else {
        for (long long c = t; c < nconf; c += 256) a0 += w ? w[c] : 1.0;
    }
    s0[t] = a0; s1[t] = a1;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) { s0[t] += s0[t + h]; s1[t] += s1[t + h]; }
        __syncthreads();
    }
    if (t == 0) {
        if (k < nshift) {
            sums[2 * k] = accumulate ? sums[2 * k] + s0[0] : s0[0];
            sums[2 * k + 1] = accumulate ? sums[2 * k + 1] + s1[0] : s1[0];
        } else if (wsum) {
            wsum[0] = accumulate ? wsum[0] + s0[0] : s0[0];
        }
    }
}
