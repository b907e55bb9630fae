// qmc_partent.h -- one-particle replica swap: the purity of the one-body
// density matrix and the particle-partition Renyi-2 entropy at n = 1 (no
// counterpart in the reference).
//
// Two independent configurations R1 = x1, R2 = x2 of |psi|^2 (a replica pair:
// the rows 2p and 2p + 1 of the batch) exchange ONE particle, x1_i <-> x2_j:
//
//   Tr rho1^2 = sum_k lambda_k^2 = < psi(R1') psi(R2') / (psi(R1) psi(R2)) >,
//   S2(n = 1) = -ln Tr rho1^2,                      rho1 of trace 1.
//
// The rows of a VMC ensemble are position-sorted, so no particular (i, j) is
// an unbiased choice; the kernel averages over all N^2 of them, which is a
// symmetric function of each row.  R1' u R2' and R1 u R2 are the same multiset
// of positions, so the one-body factors cancel: no f1 is evaluated, and a
// model without interactions gives exactly 0 everywhere and a mean of exactly
// 1.  With lf(x, y) = ln f2(|min-image(x - y)|) and F[i][j] = lf(x1_i, x2_j):
//
//   a_i = sum_k F[i][k] - sum_{k != i} lf(x1_i, x1_k)
//   b_j = sum_k F[k][j] - sum_{k != j} lf(x2_j, x2_k)
//   log_ratio[i][j] = a_i + b_j - 2 F[i][j]
//   mean = N^-2 sum_ij exp(log_ratio[i][j])
//
// Layout.  One wavefront per replica pair.  The two rows are contiguous, so
// the union of the pair is one row of 2N entries, entry q of replica q / N.
//
// Stage 1: obdm_fill_tables, once per replica, leaves the angle table of the
// union in LDS ([2N][4]).  (The positions it also publishes land in the 2N
// doubles that hold a and b from stage 2 on; nobody reads them.)
//
// Stage 2: a lane owns one entry of the union, 2N entries in passes of 64.  It
// walks the other replica's N entries and its own replica's N - 1 with
// obdm_rows<1> (a broadcast read per partner for N >= 64, two addresses
// below), takes both logarithms with obdm_row_log and leaves their difference,
// a_i or b_j, in LDS.  Lane groups are not used here: at N <= 16 part of the
// wavefront idles in this stage.
//
// Stage 3: F is not kept (2 MB at N = 512); f_ij is formed again, by
// obdm_rows<1> on a table of one partner, and the element is taken in the LOG
// form, x = a_i + b_j - 2 ln f_ij, exp(x) with x clamped to +-700.  The
// product form exp(a_i + b_j) f_ij^-2 would save the logarithm only for an
// integer beta, and its two factors leave the range of a double one by one
// where their product does not: a_i + b_j carries the whole row sums
// (|a_i| grows like N), while x, the logarithm of a ratio of wave functions
// that differ by one exchange, stays of order one.  A lane owns a particle j
// of replica 2 (the stores of a row of log_ratio are contiguous) and walks the
// particles i of replica 1; for N <= 32 the wavefront splits into 64 / G
// groups of G = 8, 16, 32 lanes that take 64 / G values of i at a time.  A
// fixed xor butterfly adds up the wavefront.
//
// Phases are ordered by wave-level fences and wave barriers (the LDS region
// belongs to the one wavefront of the block).  No atomics of any kind, no
// scratch; fp64 whatever qmc_engine_set_fast_math says.  The same input gives
// the same bits.
#pragma once

#include <cstdint>

#include "qmc_device.h"
#include "qmc_obdm.h"
#include "qmc_obdm_rows.h"

// LDS doubles per entry of the union: the four table entries and a / b
static constexpr int PARTENT_LDS_PER_ENTRY = 5;
static constexpr size_t PARTENT_LDS_LIMIT = 160 * 1024;   // of a gfx950 workgroup

static size_t partent_lds_bytes(int n)
{
    return (size_t)2 * n * PARTENT_LDS_PER_ENTRY * sizeof(double);
}

struct PartEntArgs {
    const double *pos;       // [2 npair][N]
    double *mean;            // [npair] or null
    double *log_ratio;       // [npair][N][N] or null
    long long npair;
};

// wave-level ordering of the LDS traffic of one wavefront
__device__ __forceinline__ void partent_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(64)
particle_swap_kernel(const DevModel *__restrict__ mp, PartEntArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    const int n = m.n, n2 = 2 * n;
    double *tab = smem;                          // [2N][4]
    double *ab = smem + 4 * n2;                  // [2N]: a, then b
    const long long p = blockIdx.x;
    const int lane = threadIdx.x;
    const double *__restrict__ row = a.pos + (size_t)p * n2;
    const bool pairs = !m.is_ideal;

    // Stage 1: the tables of the union, replica by replica.
    ObdmLds l(smem, n);
    l.zraw = ab; l.zbox = ab + n;                // not read
    obdm_fill_tables(m, row, l, lane);
    l.tab = tab + 4 * n;
    obdm_fill_tables(m, row + n, l, lane);
    partent_wave_sync();

    // Stage 2: a_i and b_j.
    const int none[1] = { -1 };                  // nobody to leave out
    for (int q0 = 0; q0 < n2; q0 += 64) {
        const int q = q0 + lane;
        const int qc = min(q, n2 - 1);
        const int r = qc >= n ? 1 : 0;           // the entry's replica
        PTab own[1];
        own[0].s = tab[4 * qc]; own[0].c = tab[4 * qc + 1];
        own[0].su = tab[4 * qc + 2]; own[0].cu = tab[4 * qc + 3];
        double v = 0.0;
        if (pairs) {
            const int self[1] = { qc - r * n };
            ObdmRow ro[1], rs[1];
            obdm_rows<1>(m, tab + 4 * (r ? 0 : n), n, own, none, ro);
            obdm_rows<1>(m, tab + 4 * (r ? n : 0), n, own, self, rs);
            v = obdm_row_log(m, ro[0], 0.0) - obdm_row_log(m, rs[0], 0.0);
        }
        // the last reads of the positions' region are long past: stage 1
        // only wrote there
        if (q < n2) ab[q] = v;
    }
    partent_wave_sync();

    // Stage 3: the N^2 exchanges.
    const int lg = n > 32 ? 6 : n > 16 ? 5 : n > 8 ? 4 : 3;   // G = 1 << lg
    const int G = 1 << lg, R = 64 >> lg;         // lanes, rows of a step
    const int grp = lane >> lg, gl = lane & (G - 1);
    const double guard = 700.0;                  // domain of exp_bounded
    double *__restrict__ out =
        a.log_ratio ? a.log_ratio + (size_t)p * n * n : nullptr;
    double acc = 0.0;
    for (int j0 = 0; j0 < n; j0 += G) {
        const int j = j0 + gl;
        const int jc = min(j, n - 1);
        const int e = n + jc;
        PTab own[1];
        own[0].s = tab[4 * e]; own[0].c = tab[4 * e + 1];
        own[0].su = tab[4 * e + 2]; own[0].cu = tab[4 * e + 3];
        const double bj = ab[e];
        for (int i0 = 0; i0 < n; i0 += R) {
            const int i = i0 + grp;
            const int ic = min(i, n - 1);
            double lf = 0.0;
            if (pairs) {
                ObdmRow rf[1];
                obdm_rows<1>(m, tab + 4 * ic, 1, own, none, rf);
                lf = obdm_row_log(m, rf[0], 0.0);
            }
            const double x = fma(-2.0, lf, ab[ic] + bj);
            const bool ok = (i < n) & (j < n);
            if (out && ok) out[(size_t)i * n + j] = x;
            const double v = exp_bounded(fmin(fmax(x, -guard), guard));
            acc += ok ? v : 0.0;
        }
    }
    // sum over the wavefront: xor butterfly, a fixed order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        acc += __shfl_xor(acc, off, 64);
    if (lane == 0 && a.mean) a.mean[p] = acc / ((double)n * (double)n);
}
