// qmc_pairdist.h -- pair distribution function g2(r): the histogram of the
// minimum-image pair distances of a configuration (the distance is
// `min_distance`, qmc_base/utils.py:35-51, reached through `_real_distance`,
// mrbp_qmc/model.py:555-562; the bin rule is the `int(z // bin_size)` of the
// density estimator, mrbp_qmc/dmc.py:522-545).
//
//   z_i    the position brought into [0, L) (wrap_box)
//   r_ij   = |z_i - z_j|, or L - |z_i - z_j| where that exceeds L/2
//   b_ij   = min(floor(r_ij / delta), B - 1),  delta = (L/2) / B
//   H[b]   = number of unordered pairs i < j with b_ij = b
//
// so that sum_b H[b] = N (N - 1) / 2 for every configuration and a pair at
// exactly r = L/2 counts in the last bin.  g2(r_b) = H[b] L / (N (N - 1) delta)
// is formed by the callers; the kernel hands out the integers.
//
// Layout.  One wavefront per configuration; where N <= 32, groups of
// G = 8, 16, 32 lanes take one configuration each (the host widens G again
// when 64 / G histograms would not fit the LDS budget).  A group publishes the
// wrapped positions of its configuration in LDS and clears a histogram of B
// 32-bit counters there.  The pair loop runs by rotation: the lane that owns
// particle i meets i + 1, i + 2, ..., i + floor((N - 1) / 2) (indices modulo
// N), and for an even N the particles i < N/2 meet i + N/2 as well: every
// unordered pair once, N (N - 1) / 2 in all.  N > G runs in passes over the
// own particles, i = lane + G p.  Per pair: one LDS read of the partner (the
// lanes of a group read consecutive doubles), one subtraction, the image
// select, one multiplication by 1 / delta, the conversion, one clamp and one
// LDS integer add.  The histogram leaves the wavefront with plain vector
// stores, as 32-bit counts or as doubles (exact: a count is below 2^17) for
// the reduction over configurations.
//
// Counts are integers, so the order in which the LDS adds arrive cannot change
// the result: the kernel is deterministic.  There is no floating-point atomic
// and no global atomic.  Positions and distances are fp64 whatever
// qmc_engine_set_fast_math says.
//
// The rounding of r / delta is the only freedom: the kernel multiplies by the
// host's 1 / delta where the definition divides, and forms L - |d| where the
// reference forms -L/2 + (d + L/2) % L.  Both differ from the definition by a
// few ulp of r, which moves a pair only if it sits within that of a bin edge
// (tests/_pairdist_restatement.py lists such pairs; with L and B powers of two
// and positions on a binary grid every operation is exact).
//
// The reduction over configurations is obdm_reduce_kernel (qmc_obdm.h) on the
// double-valued histograms: fixed summation order, and exact with unit weights
// since every partial sum is an integer below 2^53.
#pragma once

#include "qmc_device.h"
#include "qmc_kernels_misc.h"

static constexpr int PD_MAX_BINS = 4096;
// LDS a wavefront may take for positions and histograms of its groups
static constexpr size_t PD_LDS_BUDGET = 32768;

struct PairDistArgs {
    const double *pos;     // [nconf][n]
    void *out;             // [nconf][nbins], OutT
    long long nconf;
    int n, nbins;
    double L, half;        // supercell size, L / 2
    double inv_delta;      // nbins / (L / 2)
};

__device__ __forceinline__ void pd_count(unsigned *__restrict__ h, double zi,
                                         double zj, const PairDistArgs &a,
                                         bool active)
{
    const double ad = __builtin_fabs(zi - zj);
    const double r = (ad > a.half) ? a.L - ad : ad;
    int b = (int)(r * a.inv_delta);            // r >= 0: truncation is floor
    b = min(max(b, 0), a.nbins - 1);
    if (active) atomicAdd(&h[b], 1u);
}

// G: lanes of a configuration group (8, 16, 32, 64).
template <int G, typename OutT>
__global__ void __launch_bounds__(64)
pair_dist_kernel(PairDistArgs a)
{
    extern __shared__ double pd_smem[];
    constexpr int GPW = 64 / G;                 // configurations of a wavefront
    const int n = a.n, B = a.nbins;
    const int lane = threadIdx.x, grp = lane / G, gl = lane % G;
    double *z = pd_smem + grp * n;                               // [GPW][n]
    unsigned *h = (unsigned *)(pd_smem + GPW * n) + grp * B;     // [GPW][B]
    const long long c = (long long)blockIdx.x * GPW + grp;
    const bool live = c < a.nconf;
    const double *row = a.pos + (size_t)(live ? c : 0) * n;
    const int npass = (n + G - 1) / G;

    for (int p = 0; p < npass; ++p) {
        const int i = gl + G * p;
        const double zw = wrap_box((live && i < n) ? row[i] : 0.0, a.L);
        if (i < n) z[i] = zw;
    }
    for (int b = gl; b < B; b += G) h[b] = 0u;
    __syncthreads();

    const int kfull = (n - 1) / 2;              // offsets every particle takes
    for (int p = 0; p < npass; ++p) {
        const int i = gl + G * p;
        const int ic = min(i, n - 1);
        const bool own = live && i < n;
        const double zi = z[ic];
#pragma unroll 4
        for (int k = 1; k <= kfull; ++k) {
            int j = ic + k;
            j = (j >= n) ? j - n : j;
            pd_count(h, zi, z[j], a, own);
        }
        if (!(n & 1)) {
            // even N: the offset N/2 joins each pair from both ends; the
            // lower half of the particles takes it
            const int j = min(ic + n / 2, n - 1);
            pd_count(h, zi, z[j], a, own && i < n / 2);
        }
    }
    __syncthreads();

    OutT *out = (OutT *)a.out + (size_t)(live ? c : 0) * B;
    for (int b = gl; b < B; b += G)
        if (live) out[b] = (OutT)h[b];
}

// ---- g2(r) as a DMC block estimator ------------------------------------
// The pair histogram of every yielded walker of a time step, mixed or pure
// (forward walking), in the frame of the S(k) and density estimators
// (qmc_kernels_misc.h: EstArgs, est_reduce_kernel).  Walker s carries the
// configuration of its parent, parents[ref[s]]; H_s is its histogram as above.
//
//   mixed   iter[t][b] = sum_{s live} H_s[b]
//   pure    aux_t[s][b] = aux_{t-1}[ref_t[s]][b] + (t < pfw ? H_s[b] : 0)
//           iter[t][b] = sum_{s live} aux_t[s][b] / min(t + 1, pfw)
//
// The per-walker rows travel through the cloning table, as the S(k) parts do
// (a clone inherits the history of its parent, a dead walker's history ends);
// the slot-wise copy and the ever-growing mixed buffer of the density
// estimator are quirks reproduced there for parity and have no place here.
//
// One wavefront per walker slot, grid-striding over the live slots; particle
// i = lane + 64 p in pass p, the rotation pair loop of pair_dist_kernel<64>.
// Positions and histogram of a wavefront live in LDS and are only touched by
// that wavefront, so wave-level fences order them (as dmc_density_kernel).
// Every quantity is an integer held in a double, exact below 2^53: neither the
// lane sums, nor the block reduction, nor est_reduce_kernel can round, and the
// one division is of an integer by an integer.  fp64 whatever fast_math says.
static constexpr int PD_EST_MAXN = 512;     // particles (the engine's limit)

__global__ void __launch_bounds__(BLOCK) dmc_pair_dist_kernel(EstArgs a)
{
    constexpr int NWAVE = BLOCK / 64;
    static_assert(PD_EST_MAXN >= EST_MAXK,
                  "the block reduction reuses the position rows");
    __shared__ double zs[NWAVE][PD_EST_MAXN];
    __shared__ unsigned hs[NWAVE][EST_MAXK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.n, B = a.K;
    double *z = zs[wave];
    unsigned *h = hs[wave];
    PairDistArgs g;
    g.pos = nullptr; g.out = nullptr; g.nconf = 0;
    g.n = n; g.nbins = B;
    g.L = a.scale; g.half = 0.5 * a.scale; g.inv_delta = a.scale2;
    const long long nw = a.ctl->nw;
    const long long wstride = (long long)gridDim.x * NWAVE;
    double acc[EST_CH];
#pragma unroll
    for (int c = 0; c < EST_CH; ++c) acc[c] = 0.0;
    const bool count_now = a.counts_now();
    const int npass = (n + 63) / 64;
    const int kfull = (n - 1) / 2;              // offsets every particle takes
    for (long long s = (long long)blockIdx.x * NWAVE + wave; s < nw;
         s += wstride) {
        const long long par = a.ref[s];
        if (count_now) {
            const double *row = a.ppos + (size_t)par * n;
            for (int p = 0; p < npass; ++p) {
                const int i = lane + 64 * p;
                const double zw = wrap_box(i < n ? row[i] : 0.0, g.L);
                if (i < n) z[i] = zw;
            }
            for (int b = lane; b < B; b += 64) h[b] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int p = 0; p < npass; ++p) {
                const int i = lane + 64 * p;
                const int ic = min(i, n - 1);
                const bool own = i < n;
                const double zi = z[ic];
#pragma unroll 4
                for (int k = 1; k <= kfull; ++k) {
                    int j = ic + k;
                    j = (j >= n) ? j - n : j;
                    pd_count(h, zi, z[j], g, own);
                }
                if (!(n & 1)) {
                    // even N: the lower half of the particles takes the
                    // offset N/2 (pair_dist_kernel)
                    const int j = min(ic + n / 2, n - 1);
                    pd_count(h, zi, z[j], g, own && i < n / 2);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int c = 0; c < EST_CH; ++c) {
            const int b = c * 64 + lane;
            if (c * 64 >= B) break;
            if (b < B) {
                double v = count_now ? (double)h[b] : 0.0;
                if (a.pure) {
                    v += a.aux_prev[(size_t)par * B + b];
                    a.aux_act[(size_t)s * B + b] = v;
                }
                acc[c] += v;
            }
        }
        __builtin_amdgcn_wave_barrier();    // z and h are rewritten next
    }
    __syncthreads();                            // the position rows are free now
    double *red = &zs[0][0];                    // [NWAVE][EST_MAXK]
#pragma unroll
    for (int c = 0; c < EST_CH; ++c) red[wave * EST_MAXK + c * 64 + lane] = acc[c];
    est_block_sum(red, EST_MAXK, B, a.partial);
}
