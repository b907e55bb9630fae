// qmc_tripledist.h -- three-body distribution g3(d): the histogram of the
// spans of all particle triples of a configuration on the ring of length L.
//
//   z_i     the position brought into [0, L) (wrap_box)
//   triple  {i, j, k}, i < j < k; a <= b <= c its three wrapped positions
//   gaps    b - a, c - b, L - (c - a)
//   span    d_ijk = L - (largest gap): the shortest arc that holds all three
//   delta   = D / B,  0 < D <= L/2 (max_span)
//   bin     d_ijk <  D:  min(floor(d_ijk / delta), B - 1)
//           d_ijk >= D:  B                          (the overflow bin)
//   T[b]    = number of triples in bin b,  b = 0 ... B
//
// so that sum_b T[b] = N (N - 1) (N - 2) / 6 for every configuration (all
// zeros for N < 3).  For independent uniform particles E T[b] =
// C(N,3) 3 (delta/L)^2 (2 b + 1), b < B; the callers form g3 from that, the
// kernel hands out the integers.
//
// The triple count as a pair walk.  Order the particles by (wrapped position,
// index) into ranks 0 ... N - 1, zs[rank] the ordered positions.  For rank a
// and m = 1 ... N - 1 let r = (a + m) mod N and
//
//   arc(a, m) = zs[r] - zs[a]          if a + m < N
//             = (zs[r] + L) - zs[a]    otherwise
//
// the forward arc from a to the m-th particle after it; whether it wraps is
// decided by the rank, not by the sign of a difference, so coincident
// particles are ordered by index all the way round.  Because D <= L/2 a triple
// of span below D has exactly one leftmost member, and its span is the forward
// arc from its first to its last member.  The m - 1 particles strictly between
// the two in rank order each complete one such triple:
//
//   T[b] = sum over (a, m), arc(a, m) < D, bin(arc) = b, of (m - 1),  b < B
//   T[B] = C(N,3) - sum_{b < B} T[b]
//
// and since the arc grows with m the walk of a rank stops at the first m with
// arc >= D: O(N^2 D / L) LDS reads and integer adds where the definition asks
// for O(N^3) triples.
//
// Layout.  One wavefront per configuration; where N <= 32, groups of
// G = 8, 16, 32 lanes take one configuration each (the host widens G when
// 64 / G configurations would not fit the LDS budget).  A group publishes the
// wrapped row z[N] in LDS, clears B + 1 32-bit counters (the overflow counter
// starts at C(N,3)), and every own particle counts the entries below it (ties
// by index; the lanes of a group read the same z[j]: a broadcast) and writes
// zs[rank].  After a wave-level fence the lane that owns rank a walks m = 1,
// 2, ... (the lanes of a group read consecutive doubles), adds m - 1 to its
// bin with an LDS integer add and keeps its own total, which it takes off the
// overflow counter at the end.  N > G runs in passes, i = lane + G p.  The row
// leaves with plain vector stores, as 32-bit counts (C(512,3) < 2^25) or as
// doubles for the reduction over configurations (obdm_reduce_kernel).
//
// All adds are integer, so their order cannot change the result: the kernel is
// deterministic.  No global atomic, no floating-point atomic.  fp64 whatever
// qmc_engine_set_fast_math says.  The rounding of arc / delta (the kernel
// multiplies by the host's 1 / delta) and of arc against D is the only
// freedom: a triple moves only if its span sits within a few ulp of a bin edge
// or of D (tests/_tripledist_restatement.py lists such triples; with L, delta
// and the positions on a binary grid every operation is exact).
#pragma once

#include "qmc_device.h"

static constexpr int TD_MAX_BINS = 4096;
// LDS a wavefront may take for the rows and histograms of its groups
static constexpr size_t TD_LDS_BUDGET = 32768;

struct TripleDistArgs {
    const double *pos;     // [nconf][n]
    void *out;             // [nconf][nbins + 1], OutT
    long long nconf;
    int n, nbins;
    unsigned ntriples;     // C(n, 3)
    double L, span;        // supercell size, max_span D
    double inv_delta;      // nbins / D
};

// LDS bytes of one configuration: z[n], zs[n] and nbins + 1 counters
static inline size_t td_lds_per_conf(int n, int nbins)
{
    return 2 * (size_t)n * sizeof(double) + ((size_t)nbins + 1) * sizeof(unsigned);
}

// wave-level ordering of the LDS traffic of one wavefront
__device__ __forceinline__ void td_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// G: lanes of a configuration group (8, 16, 32, 64).
template <int G, typename OutT>
__global__ void __launch_bounds__(64)
triple_dist_kernel(TripleDistArgs a)
{
    extern __shared__ double td_smem[];
    constexpr int GPW = 64 / G;                 // configurations of a wavefront
    const int n = a.n, B = a.nbins, B1 = B + 1;
    const int lane = threadIdx.x, grp = lane / G, gl = lane % G;
    double *z = td_smem + (size_t)grp * 2 * n;                    // [GPW][2][n]
    double *zs = z + n;
    unsigned *h = (unsigned *)(td_smem + (size_t)GPW * 2 * n) + (size_t)grp * B1;
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
    if (gl == 0) h[B] = a.ntriples;
    td_wave_sync();

    // rank of every own particle: the entries below it, ties by index
    for (int p = 0; p < npass; ++p) {
        const int i = gl + G * p;
        const double zi = z[min(i, n - 1)];
        int rank = 0;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const double zj = z[j];
            rank += (zj < zi || (zj == zi && j < i)) ? 1 : 0;
        }
        if (i < n) zs[rank] = zi;
    }
    td_wave_sync();

    unsigned taken = 0u;                        // triples this lane has binned
    for (int p = 0; p < npass; ++p) {
        const int r0 = gl + G * p;
        if (!live || r0 >= n) continue;
        const double za = zs[r0];
        for (int m = 1; m < n; ++m) {
            int r = r0 + m;
            const bool past = r >= n;           // the arc passes z = L
            r = past ? r - n : r;
            const double zr = zs[r];
            const double arc = (past ? zr + a.L : zr) - za;
            if (!(arc < a.span)) break;
            if (m >= 2) {
                const int b = min(max((int)(arc * a.inv_delta), 0), B - 1);
                atomicAdd(&h[b], (unsigned)(m - 1));
                taken += (unsigned)(m - 1);
            }
        }
    }
    if (taken) atomicSub(&h[B], taken);
    td_wave_sync();

    OutT *out = (OutT *)a.out + (size_t)(live ? c : 0) * B1;
    for (int b = gl; b < B1; b += G)
        if (live) out[b] = (OutT)h[b];
}
