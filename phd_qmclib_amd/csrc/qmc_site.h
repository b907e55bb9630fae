// qmc_site.h -- site occupation statistics of the lattice: how many particles
// sit on each lattice site of a configuration, as the occupation distribution
// P(n) and the site-site correlation <n_c n_{c+d}> (an extension: the
// reference has neither).  The lattice period is 1 and the supercell holds
// S = L sites (L integral, 1 <= S <= SITE_MAXS); a period is a well of width
// z_a followed by a barrier of width z_b = 1 - z_a (qmc_device.h).
//
//   site c  well c with half a barrier on each side: [c - z_b/2, c + 1 - z_b/2)
//   u_i     = wrap_box(z_i + z_b/2, L)
//   c_i     = min((int)u_i, S - 1)
//   n_c     = number of particles i with c_i = c            (sum_c n_c = N)
//   occ[n]  = number of sites c with min(n_c, P - 1) = n,  n = 0 .. P-1
//             (the last bin collects n_c >= P - 1; sum_n occ[n] = S)
//   corr[d] = sum_c n_c n_{(c + d) mod S},                 d = 0 .. D-1
//             (corr[0] = sum_c n_c^2, corr[d] = corr[S - d], and with D = S
//             sum_d corr[d] = N^2)
//
// A row is the K = P + D doubles [occ | corr].  P >= 1, 0 <= D <= S and
// P + D <= EST_MAXK; P = 0 switches the estimator off.  The callers form
// P(n) = occ[n] / (S W), the on-site variance corr[0] / (S W) - (N / S)^2 and
// the connected correlation C(d) = corr[d] / (S W) - (N / S)^2 over W walkers
// (engine.site_statistics); the kernel hands out the integers.
//
// Mixed and pure follow g2(r) exactly (qmc_pairdist.h: counts_now(), divisor(),
// the rows travelling through the cloning table).  Walker s carries the
// configuration of its parent, ppos[ref[s]]; R_s is its row as above.
//
//   mixed   iter[t][j] = sum_{s live} R_s[j]
//   pure    aux_t[s][j] = aux_{t-1}[ref_t[s]][j] + (t < pfw ? R_s[j] : 0)
//           iter[t][j] = sum_{s live} aux_t[s][j] / min(t + 1, pfw)
//
// The operator is local and diagonal, so the pure estimate needs no VMC
// extrapolation.
//
// Layout.  One wavefront per walker slot, grid-striding over the live slots,
// EST_BLOCKS x BLOCK as dmc_pair_dist_kernel.  The wavefront keeps the site
// counts in a row of its own in LDS, stored twice, n[0 .. 2S) with
// n[c + S] = n[c], so that the circular shift c + d needs no modulo.  Lane
// `lane` bins the particles i = lane + 64 p with two LDS integer adds each.
// Then lane `lane` owns the row entries j = lane + 64 q and, per entry, walks
// the sites c = 0 .. S-1 once: it reads n[c] (the same address in every lane:
// a broadcast) and, for a correlation entry d = j - P, n[c + d] (consecutive
// addresses over the lanes: conflict-free), counts the match
// min(n[c], P - 1) == j and adds the product, and keeps the one of the two sums
// that its entry is.  Nothing crosses lanes after the
// binning: no wave reduction and no second histogram.  The row of counts
// belongs to the wavefront alone, so wave-level fences and barriers order its
// reuse.  LDS: BLOCK / 64 rows of 2 SITE_MAXS 32-bit counters, 16 KB per
// workgroup, reused for the block reduction.
//
// EstArgs has no free field for P (its one padding slot went to `stride`), so
// P travels in `stride`, which only F(k, tau) reads; S is (int)scale
// (scale = L, integral as the host has checked), z_b / 2 comes in scale2 and
// D = K - P.
//
// Every quantity is an integer: a site count is at most N <= 512, a product
// sum at most N^2 < 2^18, held in 32-bit counters and then in doubles, exact
// below 2^53.  Neither the order of the LDS adds, nor the block reduction,
// nor est_reduce_kernel can round, and the one division is of an integer by an
// integer: the kernel is deterministic.  There is no floating-point atomic and
// no global atomic.  Positions are fp64 whatever qmc_engine_set_fast_math
// says.  The only freedom is a particle within a few ulp of a site boundary
// (u_i at an integer), where the rounding of z_i + z_b/2 decides the site
// (tests/_site_restatement.py lists such particles).
#pragma once

#include "qmc_device.h"
#include "qmc_kernels_misc.h"

static constexpr int SITE_MAXS = 512;       // sites of the supercell

__global__ void __launch_bounds__(BLOCK) dmc_site_kernel(EstArgs a)
{
    constexpr int NWAVE = BLOCK / 64;
    static_assert(2 * SITE_MAXS * sizeof(unsigned) >= EST_MAXK * sizeof(double),
                  "the block reduction reuses the site counts");
    __shared__ __attribute__((aligned(16))) unsigned ns[NWAVE][2 * SITE_MAXS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.n, K = a.K, P = a.stride;
    const int S = min(max((int)a.scale, 1), SITE_MAXS);
    const double L = a.scale, half_zb = a.scale2;
    unsigned *cnt = ns[wave];
    const long long nw = a.ctl->nw;
    const long long wstride = (long long)gridDim.x * NWAVE;
    double acc[EST_CH];
#pragma unroll
    for (int c = 0; c < EST_CH; ++c) acc[c] = 0.0;
    const bool count_now = a.counts_now();
    const int npass = (n + 63) / 64;
    for (long long s = (long long)blockIdx.x * NWAVE + wave; s < nw;
         s += wstride) {
        const long long par = a.ref[s];
        if (count_now) {
            const double *row = a.ppos + (size_t)par * n;
            for (int c = lane; c < 2 * S; c += 64) cnt[c] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int p = 0; p < npass; ++p) {
                const int i = lane + 64 * p;
                const double u = wrap_box((i < n ? row[i] : 0.0) + half_zb, L);
                const int c = min(max((int)u, 0), S - 1);
                if (i < n) {
                    atomicAdd(&cnt[c], 1u);
                    atomicAdd(&cnt[c + S], 1u);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int q = 0; q < EST_CH; ++q) {
            const int j = q * 64 + lane;
            if (q * 64 >= K) break;
            unsigned r = 0u;
            if (count_now) {
                // (a lane without an entry walks along with d = 0 and drops
                // its sum: c + d < 2 S for every lane)
                const bool is_corr = j >= P && j < K;
                const int d = is_corr ? j - P : 0;
                const unsigned top = (unsigned)(P - 1);
                // Both sums in every lane and one select at the end: a select
                // per site became a divergent branch around the second read,
                // with a wait on every read.  Unrolled, the reads of several
                // sites are in flight at once.
                unsigned prod = 0u, match = 0u;
#pragma unroll 8
                for (int c = 0; c < S; ++c) {
                    const unsigned nc = cnt[c];
                    const unsigned nd = cnt[c + d];
                    prod += nc * nd;
                    match += min(nc, top) == (unsigned)j ? 1u : 0u;
                }
                r = is_corr ? prod : match;
            }
            if (j < K) {
                double v = (double)r;
                if (a.pure) {
                    v += a.aux_prev[(size_t)par * K + j];
                    a.aux_act[(size_t)s * K + j] = v;
                }
                acc[q] += v;
            }
        }
        __builtin_amdgcn_wave_barrier();    // the counts are rewritten next
    }
    __syncthreads();                            // the site counts are free now
    double *red = (double *)&ns[0][0];          // [NWAVE][EST_MAXK]
#pragma unroll
    for (int c = 0; c < EST_CH; ++c) red[wave * EST_MAXK + c * 64 + lane] = acc[c];
    est_block_sum(red, EST_MAXK, K, a.partial);
}
