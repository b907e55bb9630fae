// qmc_renyi_region.h -- replica-swap estimator of the Renyi-2 entropy of a
// region X made of up to two disjoint segments of the ring, with the charge
// (particle number) of the region resolved in the reduction (no counterpart
// in the reference).  It extends qmc_renyi.h, which describes the swap itself.
//
// Definitions.  Entry k of a call is a region X_k given by three doubles
// (l1, g, l2).  With t as qmc_renyi_swap defines it (images in [0, L), offset
// from `origin`, + L where negative) particle z is in X_k when
//
//   t < l1  or  (m1 <= t && t < m2),    m1 = l1 + g,  m2 = m1 + l2,
//
// the two marks formed in fp64 in exactly this order.  Limits: l1 > 0, g >= 0,
// l2 >= 0, m2 < L, all finite; l2 = 0 is a single segment (its g is not used
// but obeys the limits); 1 <= nreg <= 4096.  n_x[nconf][nreg] is the number
// of particles of each configuration in X_k (exact).  A pair is matched at k
// when its two replicas hold the same TOTAL number in X_k, however they split
// it between the two windows.  For a matched pair, with Y the complement,
//
//   R1' = X(R2) u Y(R1),   R2' = X(R1) u Y(R2),
//   log_ratio = ln|psi(R1')| + ln|psi(R2')| - ln|psi(R1)| - ln|psi(R2)|
//             = S(X2, Y1) + S(X1, Y2) - S(X1, Y1) - S(X2, Y2),
//
// the pair factors across the cut alone; -inf where the pair is unmatched,
// exactly 0 for a model without interactions and where either side is empty
// in both replicas.  fp64 whatever qmc_engine_set_fast_math says.
//
// Layout.  One wavefront per replica pair; stage 1 is that of qmc_renyi.h
// (renyi_order_replicas): each replica ordered by t once, the PTab angle
// table of the union and t in LDS.  In that order X_k is at most two index
// ranges of a replica's block and Y_k at most two:
//
//   [0, b1) prefix | [b1, b2) gap | [b2, b3) second window | [b3, N) tail
//        X                Y                  X                    Y
//
// b1, b2, b3 the numbers of particles with t < l1, t < m1, t < m2: the four
// boundaries of a replica are these and N, which is the same for every entry
// and is not stored.  (The tail runs to t = L, the wrap back to the origin.)
//
// Stage 2 counts b1, b2, b3 per replica and entry with wave ballots (exact
// integers), writes n_x = b1 + b3 - b2, finishes the unmatched and the trivial
// entries, and lists the others in LDS: three ints per listed entry, k and
// the boundaries of either replica, ten bits each (N <= 512).
//
// Stage 3, per listed entry: the side with fewer particles owns (X or Y: the
// totals agree between the replicas, the ranges do not), the other side is
// the partner.  For partner replica h = 0, 1 in turn, a lane takes one owner
// particle of either replica -- 2 min(n_X, N - n_X) items in passes of 64 --
// and walks the partner ranges of replica h with obdm_rows, the row arithmetic
// of g1 as it stands, once per range (one where the two ranges touch, as the
// gap and the tail of a single segment do, or one of them is empty), adds the
// logarithms of the ranges (obdm_row_log) and signs the sum: plus where owner
// and partner belong to different replicas.  The ranges of a pass are the
// same in every lane: the bounds are scalars, every LDS read of a partner is
// a broadcast, and no membership is looked at in the pair loop.  Only the
// cross pairs X x Y are formed, 4 n_X (N - n_X) of them, each once.  A fixed
// xor butterfly adds up the wavefront.
//
// LDS: 2N (4 + 1) doubles of tables and t, then the larger of 2N doubles (t
// as given, stage 1) and 3 ints per entry (the list): 40 KB + 48 KB at
// N = 512 with 4096 entries, inside the 160 KB of a gfx950 workgroup.
//
// Rows for the reduction, per tile of `stride` pairs and column by column so
// that the reduction reads them coalesced: rows[k][p] = swap (0 unmatched, the
// argument of exp clamped to +-700) and rows[K + k][p] = c0 + 1024 c1, the
// occupations of the two replicas (exact in a double).
// renyi_region_reduce_kernel adds them up in a fixed order, block (k, 0) the
// three columns of qmc_renyi_swap_reduce_dev and block (k, 1 + n) the two
// columns of charge n.
//
// No atomics of any kind, no scratch.  The same input gives the same bits.
#pragma once

#include <cstdint>

#include "qmc_device.h"
#include "qmc_obdm_rows.h"
#include "qmc_renyi.h"

static constexpr int RG_BND_BITS = 10;          // a boundary, 0 ... 512
static constexpr int RG_BND_MASK = (1 << RG_BND_BITS) - 1;
static constexpr int RG_MAX_N = 512;            // of every engine
static_assert(RG_MAX_N <= RG_BND_MASK, "packing of the boundaries");
static constexpr int RG_LIST_INTS = 3;          // k and a word per replica
static constexpr long long RG_MAX_SUMS = 1ll << 20;   // doubles of sums_dev

static size_t renyi_region_lds_bytes(int n, int K)
{
    const size_t tail = (size_t)2 * n * sizeof(double);
    const size_t list = (size_t)K * RG_LIST_INTS * sizeof(int);
    return (size_t)2 * n * RENYI_LDS_PER_ENTRY * sizeof(double) +
           (tail > list ? tail : list);
}

struct RegionArgs {
    const double *pos;       // [2 npair][N]
    const double *regions;   // [K][3] = l1, g, l2
    int32_t *n_x;            // [2 npair][K] or null
    double *log_ratio;       // [npair][K] or null
    double *rows;            // [2 K][stride] = swap[K], occupations[K], or null
    long long npair, stride;
    int K;
    double origin;
};

// The two index ranges of one side of a replica's block, (start, length)
// each, from its packed boundaries: ranges that touch are one, and an empty
// first range gives way to the second.
struct RgSide {
    int s0, l0, s1, l1;
};

__device__ __forceinline__ RgSide rg_side(int code, int n, bool want_x)
{
    const int b1 = code & RG_BND_MASK;
    const int b2 = (code >> RG_BND_BITS) & RG_BND_MASK;
    const int b3 = code >> (2 * RG_BND_BITS);
    RgSide r;
    r.s0 = want_x ? 0 : b1;  r.l0 = want_x ? b1 : b2 - b1;
    r.s1 = want_x ? b2 : b3; r.l1 = want_x ? b3 - b2 : n - b3;
    if (r.s0 + r.l0 == r.s1) { r.l0 += r.l1; r.l1 = 0; }
    if (r.l0 == 0) { r.s0 = r.s1; r.l0 = r.l1; r.l1 = 0; }
    return r;
}

__global__ void __launch_bounds__(64)
renyi_region_kernel(const DevModel *__restrict__ mp, RegionArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    const int n = m.n, n2 = 2 * n, K = a.K;
    double *tab = smem;                          // [2N][4], replicas by t
    double *ts = smem + 4 * n2;                  // [2N] t in that order
    double *traw = smem + RENYI_LDS_PER_ENTRY * n2;   // [2N] t as given
    int *mk = (int *)traw;                       // [K][3] the list (later)
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const int npass = (n2 + 63) / 64;

    // Stage 1: each replica ordered by t.
    renyi_order_replicas(m, a.pos + (size_t)p * n2, a.origin, tab, ts, traw,
                         lane);                  // traw is the list from here

    // Stage 2: the boundaries per replica and entry; the unmatched and the
    // trivial entries are finished here.
    const double ninf = -__builtin_inf();
    int nm = 0;                                  // listed entries (uniform)
    for (int k = 0; k < K; ++k) {
        const double l1 = a.regions[3 * k];
        const double m1 = l1 + a.regions[3 * k + 1];
        const double m2 = m1 + a.regions[3 * k + 2];
        int b[2][3] = { { 0, 0, 0 }, { 0, 0, 0 } };
        for (int pp = 0; pp < npass; ++pp) {
            const int q = lane + 64 * pp;
            const double tq = ts[min(q, n2 - 1)];
            const bool r0 = q < n, r1 = (q >= n) & (q < n2);
            const bool u1 = tq < l1, u2 = tq < m1, u3 = tq < m2;
            b[0][0] += __popcll(__ballot(u1 & r0));
            b[0][1] += __popcll(__ballot(u2 & r0));
            b[0][2] += __popcll(__ballot(u3 & r0));
            b[1][0] += __popcll(__ballot(u1 & r1));
            b[1][1] += __popcll(__ballot(u2 & r1));
            b[1][2] += __popcll(__ballot(u3 & r1));
        }
        const int c0 = b[0][0] + b[0][2] - b[0][1];
        const int c1 = b[1][0] + b[1][2] - b[1][1];
        const bool matched = c0 == c1;
        const bool done = !matched | (c0 == 0) | (c0 == n) | (m.is_ideal != 0);
        if (lane == 0) {
            if (a.n_x) {
                a.n_x[(size_t)(2 * p) * K + k] = c0;
                a.n_x[(size_t)(2 * p + 1) * K + k] = c1;
            }
            if (a.rows)
                a.rows[(size_t)(K + k) * a.stride + p] =
                    (double)(c0 + (c1 << RG_BND_BITS));
            if (done) {
                if (a.log_ratio)
                    a.log_ratio[(size_t)p * K + k] = matched ? 0.0 : ninf;
                if (a.rows)
                    a.rows[(size_t)k * a.stride + p] = matched ? 1.0 : 0.0;
            } else {
                mk[RG_LIST_INTS * nm] = k;
                for (int r = 0; r < 2; ++r)
                    mk[RG_LIST_INTS * nm + 1 + r] =
                        b[r][0] | (b[r][1] << RG_BND_BITS) |
                        (b[r][2] << (2 * RG_BND_BITS));
            }
        }
        nm += done ? 0 : 1;
    }
    __syncthreads();

    // Stage 3: the cross pairs of the listed entries, range by range.
    const double guard = 700.0;                  // domain of exp_bounded
    for (int kb = 0; kb < nm; ++kb) {
        // the same in every lane: scalars, so that the ranges are loop bounds
        // the compiler knows to be uniform
        const int k = __builtin_amdgcn_readfirstlane(mk[RG_LIST_INTS * kb]);
        const int e0 =
            __builtin_amdgcn_readfirstlane(mk[RG_LIST_INTS * kb + 1]);
        const int e1 =
            __builtin_amdgcn_readfirstlane(mk[RG_LIST_INTS * kb + 2]);
        const RgSide x0 = rg_side(e0, n, true);
        const int nx = x0.l0 + x0.l1;            // 0 < nx < N, of both replicas
        const bool own_x = 2 * nx <= n;          // the smaller side owns
        const int mo = own_x ? nx : n - nx;
        const RgSide o0 = rg_side(e0, n, own_x), o1 = rg_side(e1, n, own_x);
        const int items = 2 * mo;                // an owner of either replica
        double acc = 0.0;
        for (int h = 0; h < 2; ++h) {            // the partners' replica
            const RgSide pr = rg_side(h ? e1 : e0, n, !own_x);   // pr.l0 > 0
            const double *ptab = tab + 4 * (h * n);
            for (int w0 = 0; w0 < items; w0 += 64) {
                const int w = w0 + lane;
                const int wc = min(w, items - 1);
                const int ro = wc >= mo ? 1 : 0; // the owner's replica
                const int i = wc - ro * mo;      // its place on the owner side
                const int l0 = ro ? o1.l0 : o0.l0;
                const int at = i < l0 ? (ro ? o1.s0 : o0.s0) + i
                                      : (ro ? o1.s1 : o0.s1) + (i - l0);
                const int slot = ro * n + at;
                PTab own[1];
                own[0].s = tab[4 * slot]; own[0].c = tab[4 * slot + 1];
                own[0].su = tab[4 * slot + 2]; own[0].cu = tab[4 * slot + 3];
                const int self[1] = { -1 };      // nobody to leave out
                ObdmRow r[1];
                obdm_rows<1>(m, ptab + 4 * pr.s0, pr.l0, own, self, r);
                double lg = obdm_row_log(m, r[0], 0.0);
                if (pr.l1 > 0) {
                    obdm_rows<1>(m, ptab + 4 * pr.s1, pr.l1, own, self, r);
                    lg += obdm_row_log(m, r[0], 0.0);
                }
                const double v = (h != ro) ? lg : -lg;
                acc += (w < items) ? v : 0.0;
            }
        }
        // sum over the wavefront: xor butterfly, a fixed order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            acc += __shfl_xor(acc, off, 64);
        if (lane == 0) {
            if (a.log_ratio) a.log_ratio[(size_t)p * K + k] = acc;
            if (a.rows) {
                const double x = fmin(fmax(acc, -guard), guard);
                a.rows[(size_t)k * a.stride + p] = exp_bounded(x);
            }
        }
    }
}

// sums[K][3 + 2 Q] (+)= the sums over the npair pairs of a tile of rows.
// Block (k, 0): sum swap, sum swap^2, matched pairs; block (k, 1 + c):
// sum swap [c0 = c] and sum [c0 = c] + [c1 = c].  Thread t adds the pairs t,
// t + 256, ... in index order and the 256 partial sums are added by a fixed
// tree: the same bits on every run (no floating-point atomics).  `accumulate`
// adds to what is there (the tiles arrive in order).
__global__ void __launch_bounds__(256)
renyi_region_reduce_kernel(const double *__restrict__ rows, long long npair,
                           long long stride, int K, int Q, int accumulate,
                           double *__restrict__ sums)
{
    __shared__ double s0[256], s1[256], s2[256];
    const int k = blockIdx.x, y = blockIdx.y, t = threadIdx.x;
    const double *__restrict__ sw = rows + (size_t)k * stride;
    const double *__restrict__ occ = rows + (size_t)(K + k) * stride;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (long long p = t; p < npair; p += 256) {
        const double s = sw[p];
        const int code = (int)occ[p];
        const int c0 = code & RG_BND_MASK, c1 = code >> RG_BND_BITS;
        if (y == 0) {
            a0 += s;
            a1 = fma(s, s, a1);
            a2 += (c0 == c1) ? 1.0 : 0.0;
        } else {
            a0 += (c0 == y - 1) ? s : 0.0;
            a1 += (double)((c0 == y - 1 ? 1 : 0) + (c1 == y - 1 ? 1 : 0));
        }
    }
    s0[t] = a0; s1[t] = a1; s2[t] = a2;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) {
            s0[t] += s0[t + h]; s1[t] += s1[t + h]; s2[t] += s2[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        double *out = sums + (size_t)k * (3 + 2 * Q);
        const int c = y == 0 ? 0 : 3 + 2 * (y - 1);
        out[c] = accumulate ? out[c] + s0[0] : s0[0];
        out[c + 1] = accumulate ? out[c + 1] + s1[0] : s1[0];
        if (y == 0) out[2] = accumulate ? out[2] + s2[0] : s2[0];
    }
}
