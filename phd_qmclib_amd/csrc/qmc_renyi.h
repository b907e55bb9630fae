// qmc_renyi.h -- replica-swap estimator of the Renyi-2 entanglement entropy
// of a segment A = [a0, a0 + l) of the ring (no counterpart in the reference).
//
// Two independent configurations R1, R2 of |psi|^2 (a replica pair: the rows
// 2p and 2p + 1 of the batch) exchange their particles inside A:
//
//   R1' = A(R2) u B(R1),   R2' = A(R1) u B(R2),      B the complement of A,
//   swap = psi(R1') psi(R2') / (psi(R1) psi(R2)),    S2(l) = -ln <swap>,
//
// which needs both replicas to hold the same number of particles in A (a
// "matched" pair; swap = 0 otherwise).  Membership of a particle, per replica:
//
//   zw = wrap_box(z, L), a0w = wrap_box(a0, L), t = zw - a0w (+ L if < 0),
//   in A  <=>  t < l.
//
// Cross-pair form.  R1' u R2' and R1 u R2 are the same multiset of positions,
// so the one-body factors cancel, and so do the pairs inside A and inside B.
// With S(X, Y) = sum_{x in X, y in Y} ln f2(|min-image(x - y)|):
//
//   ln swap = S(A2, B1) + S(A1, B2) - S(A1, B1) - S(A2, B2).
//
// No f1 is evaluated, and a model without interactions gives exactly 0.
//
// Layout.  One wavefront per replica pair.  The two rows are contiguous, so
// the union of the pair is one row of 2N entries, entry q of replica q / N.
//
// Stage 1 orders every replica by t (rank by a broadcast count, ties by
// index) and publishes, in that order, the angle table of the union in LDS
// (the four numbers of `PTab`, filled as obdm_fill_tables does) and t.  Every
// segment starts at the same origin, so in this order A is a PREFIX of each
// replica's block and B the rest, at every length: no membership mask is left
// in the pair loop, and only the pairs across the cut are ever formed --
// 4 n_A (N - n_A) of them, N^2 at most, where a masked walk over the union
// forms 4 N^2.
//
// Stage 2 counts, per length, the particles of either replica in A with wave
// ballots (exact integers), writes them, and lists the matched lengths in
// LDS.  An unmatched length gets -inf there and then, a matched one with an
// empty side (or a model without interactions) 0, and neither reaches the
// pair loop.
//
// Stage 3, per matched length: the smaller side owns, the other side is the
// partner.  A lane takes one (owner, partner replica) item -- 4 min(n_A,
// N - n_A) items in passes of 64 -- and walks that replica's partner range
// with obdm_rows, the row arithmetic of g1 as it stands (angle subtraction,
// short / long as a select, the wrapped own k2-table, exponents split off
// every OBDM_FOLD partners), takes the logarithm in the obdm_row_log form,
// and signs it: plus where the partner range belongs to the other replica
// (the numerator), minus for its own (the denominator).  The items are laid
// out partner replica by partner replica, so the lanes of a pass read the
// same partner entry (a broadcast) except in the pass that holds the boundary.
// A fixed xor butterfly adds up the wavefront.  Every cross pair is formed
// once.
//
// No atomics of any kind, no scratch; fp64 whatever qmc_engine_set_fast_math
// says (a float row product underflows).  The same input gives the same bits.
#pragma once

#include <cstdint>

#include "qmc_device.h"
#include "qmc_obdm_rows.h"

static constexpr int RENYI_MAX_LEN = 4096;     // lengths of one call
static constexpr int RENYI_LEN_BITS = 12;      // (k, n_A) packed in the list
static_assert(RENYI_MAX_LEN == 1 << RENYI_LEN_BITS, "packing of the list");
// LDS doubles per entry of the union: the four table entries and t
static constexpr int RENYI_LDS_PER_ENTRY = 5;

// the tables, then a region that holds t in the caller's order while the
// replicas are ranked and the list of matched lengths afterwards
static constexpr size_t RENYI_LDS_LIMIT = 160 * 1024;   // of a gfx950 workgroup

static size_t renyi_lds_bytes(int n, int K)
{
    const size_t tail = (size_t)2 * n * sizeof(double);
    const size_t list = (size_t)K * sizeof(int);
    return (size_t)2 * n * RENYI_LDS_PER_ENTRY * sizeof(double) +
           (tail > list ? tail : list);
}

struct RenyiArgs {
    const double *pos;       // [2 npair][N]
    const double *lengths;   // [K]
    int32_t *n_a;            // [2 npair][K] or null
    double *log_ratio;       // [npair][K] or null
    double *rows;            // [npair][2 K] = swap[K], matched[K], or null
    long long npair;
    int K;
    double origin;
};

// Stage 1 of a wavefront's replica pair `row` (2N positions): t as given into
// traw, then every entry to its rank inside its replica, its table entry to
// tab and its t to ts.  Ends on a barrier: traw is free from there.
__device__ __forceinline__ void renyi_order_replicas(
    const DevModel &m, const double *__restrict__ row, double origin,
    double *tab, double *ts, double *traw, int lane)
{
    const int n = m.n, n2 = 2 * n;
    const int npass = (n2 + 63) / 64;
    const double a0w = wrap_box(origin, m.L);
    for (int pp = 0; pp < npass; ++pp) {
        const int q = lane + 64 * pp;
        const double z = wrap_box((q < n2) ? row[q] : 0.0, m.L);
        double d = z - a0w;
        if (d < 0.0) d += m.L;
        if (q < n2) traw[q] = d;
    }
    __syncthreads();
    for (int pp = 0; pp < npass; ++pp) {
        const int q = lane + 64 * pp;
        const int qc = min(q, n2 - 1);
        const double z = wrap_box(row[qc], m.L);
        PTab t;
        sincos_halfpi(z * m.two_over_L, t.s, t.c);
        sincos_halfpi(z * m.k2_2pi, t.su, t.cu);
        const double tq = traw[qc];
        const int base = qc >= n ? n : 0;        // the entry's replica block
        int rank = 0;
        for (int j = base; j < base + n; ++j) {
            const double tj = traw[j];
            rank += ((tj < tq) | ((tj == tq) & (j < qc))) ? 1 : 0;
        }
        if (q < n2) {
            const int dst = base + rank;         // in [base, base + N)
            tab[4 * dst] = t.s; tab[4 * dst + 1] = t.c;
            tab[4 * dst + 2] = t.su; tab[4 * dst + 3] = t.cu;
            ts[dst] = tq;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64)
renyi_swap_kernel(const DevModel *__restrict__ mp, RenyiArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    const int n = m.n, n2 = 2 * n, K = a.K;
    double *tab = smem;                          // [2N][4], replicas by t
    double *ts = smem + 4 * n2;                  // [2N] t in that order
    double *traw = smem + RENYI_LDS_PER_ENTRY * n2;   // [2N] t as given
    int *mk = (int *)traw;                       // [K] matched lengths (later)
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const int npass = (n2 + 63) / 64;

    // Stage 1: t as given, then every entry to its rank inside its replica.
    renyi_order_replicas(m, a.pos + (size_t)p * n2, a.origin, tab, ts, traw,
                         lane);                  // traw is the list from here

    // Stage 2: the occupation of A per replica and length; the unmatched and
    // the trivial lengths are finished here.
    const double ninf = -__builtin_inf();
    int nm = 0;                                  // listed lengths (uniform)
    for (int k = 0; k < K; ++k) {
        const double len = a.lengths[k];
        int c0 = 0, c1 = 0;
        for (int pp = 0; pp < npass; ++pp) {
            const int q = lane + 64 * pp;
            const bool in = (q < n2) && ts[min(q, n2 - 1)] < len;
            c0 += __popcll(__ballot(in & (q < n)));
            c1 += __popcll(__ballot(in & (q >= n)));
        }
        const bool matched = c0 == c1;
        const bool done = !matched | (c0 == 0) | (c0 == n) | (m.is_ideal != 0);
        if (lane == 0) {
            if (a.n_a) {
                a.n_a[(size_t)(2 * p) * K + k] = c0;
                a.n_a[(size_t)(2 * p + 1) * K + k] = c1;
            }
            if (done) {
                if (a.log_ratio)
                    a.log_ratio[(size_t)p * K + k] = matched ? 0.0 : ninf;
                if (a.rows) {
                    a.rows[(size_t)p * 2 * K + k] = matched ? 1.0 : 0.0;
                    a.rows[(size_t)p * 2 * K + K + k] = matched ? 1.0 : 0.0;
                }
            } else {
                mk[nm] = k | (c0 << RENYI_LEN_BITS);
            }
        }
        nm += done ? 0 : 1;
    }
    __syncthreads();

    // Stage 3: the cross pairs of the listed lengths.
    const double guard = 700.0;                  // domain of exp_bounded
    for (int kb = 0; kb < nm; ++kb) {
        const int code = mk[kb];
        const int k = code & (RENYI_MAX_LEN - 1);
        const int na = code >> RENYI_LEN_BITS;   // 0 < na < N
        const bool own_a = 2 * na <= n;          // the smaller side owns
        const int mo = own_a ? na : n - na, np = n - mo;
        const int bo = own_a ? 0 : na;           // offsets inside a block
        const int bp = own_a ? na : 0;
        const int items = 4 * mo;                // (owner, partner replica)
        double acc = 0.0;
        for (int w0 = 0; w0 < items; w0 += 64) {
            const int w = w0 + lane;
            const int wc = min(w, items - 1);
            // replica 0's partners for the first 2 mo items, replica 1's for
            // the rest: the lanes of a pass read one partner entry, two
            // where the pass holds the boundary
            const int h = wc >= 2 * mo ? 1 : 0;
            const int o = wc - 2 * mo * h;       // o in [0, 2 mo)
            const int ro = o >= mo ? 1 : 0;      // the owner's replica
            const int slot = ro * n + bo + (o - ro * mo);
            PTab own[1];
            own[0].s = tab[4 * slot]; own[0].c = tab[4 * slot + 1];
            own[0].su = tab[4 * slot + 2]; own[0].cu = tab[4 * slot + 3];
            const int self[1] = { -1 };          // nobody to leave out
            ObdmRow r[1];
            obdm_rows<1>(m, tab + 4 * (h * n + bp), np, own, self, r);
            const double lg = obdm_row_log(m, r[0], 0.0);
            const double v = (h != ro) ? lg : -lg;
            acc += (w < items) ? v : 0.0;
        }
        // sum over the wavefront: xor butterfly, a fixed order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            acc += __shfl_xor(acc, off, 64);
        if (lane == 0) {
            if (a.log_ratio) a.log_ratio[(size_t)p * K + k] = acc;
            if (a.rows) {
                const double x = fmin(fmax(acc, -guard), guard);
                a.rows[(size_t)p * 2 * K + k] = exp_bounded(x);
                a.rows[(size_t)p * 2 * K + K + k] = 1.0;
            }
        }
    }
}

// sums[K][3] = sum swap, sum swap^2, matched pairs from the column sums
// colsum[2 K][2] that obdm_reduce_kernel leaves of the rows above.
__global__ void __launch_bounds__(64)
renyi_pack_kernel(const double *__restrict__ colsum, int K,
                  double *__restrict__ sums)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    sums[3 * k] = colsum[2 * k];
    sums[3 * k + 1] = colsum[2 * k + 1];
    sums[3 * k + 2] = colsum[2 * (K + k)];
}
