// qmc_obdm_grid.h -- the two-point one-body density matrix rho1(x, x') on a
// grid (no counterpart in the reference): what g1(s) of qmc_obdm.h integrates
// away.  In a lattice rho1 is not a function of x - x'; its eigenvalues are
// the occupations of the natural orbitals and the largest one, over N, the
// condensate fraction.
//
// M = num_points uniform cells of [0, L), delta = L / M, centres
// x_c = (c + 1/2) L / M.  For one configuration R, z_i the image of particle i
// in [0, L) and a(i) = min(floor(z_i / delta), M - 1) its row bin:
//
//   R_conf[a][c] = sum_{i : a(i) = a} psi(z_1 .. z_i -> x_c .. z_N) / psi(R)
//
// The row index follows the particle's actual position and the column is the
// cell centre, so the average over |psi|^2 is int_{bin a} rho1(x, x_c) dx with
// no bias inside the row bin.  The ratio is that of qmc_obdm.h: the one-body
// factor at x_c over the one at the position as given, and the N - 1 pair
// factors of the moved particle against the others, by obdm_rows / obdm_row_log
// on the tables of obdm_fill_tables with the denominator of
// obdm_unshifted_rows, so that a ratio carries the rounding of g1's and a
// particle that sits on a cell centre gives exactly 1 in its diagonal cell.
// M N (N - 1) pair factors per configuration: g1 at M shifts.
//
// M^2 doubles per configuration do not fit anywhere, so the kernel reduces
// over the configurations itself, into G = num_groups independent sums,
//
//   sums[g][a][c] = sum_{conf = g (mod G)} w_conf R_conf[a][c]
//   wsum[g]       = sum_{conf = g (mod G)} w_conf         (w null: 1)
//
// Layout: the transpose of obdm_kernel's.  LANE = COLUMN c: the moved
// particle's table (sin/cos(pi x_c / L), sin/cos(k2 x_c)) and log f1(x_c) are
// constants of the lane for the whole launch and stay in registers across the
// configurations; x_c is inside the box by construction, so there are no angle
// additions and no image fix-up.  The own particle i is wave-uniform, the
// partner loop reads broadcast entries of the configuration's table in LDS as
// before.  A lane carries OGRID_U = 2 OWN PARTICLES of its column at a time,
// not two columns: the two product chains are as independent and a partner's
// entry serves both, but the 64 lanes of a wavefront are all at work at
// M = 64, where two columns to a lane would leave half of them idle.
//
// Work decomposition.  A partial matrix p = s G + g (s < S) takes the members
// q = s, s + S, ... of group g (configuration g + G q) in rising order.  It is
// cut into tiles of 64 columns times `rows` row bins; one wavefront owns one
// tile of one partial matrix for the whole launch.  Per configuration it fills
// the tables and the denominators, lists the particles whose bin falls into
// its rows (ballot compaction, in row order of the particles) and walks the
// list two at a time.  For a fixed particle the row is wave-uniform and every
// lane owns its column, so acc[a(i)][c] += w v has no conflicts among lanes;
// the two particles of a lane are added one after the other.  Nothing depends
// on the particles being sorted.
//
// The partial matrices live in GLOBAL memory, not in LDS: a tile of M rows is
// 32 KB at M = 64 and 256 KB at M = 512, and holding it in LDS would leave one
// or two wavefronts to a CU under a partner loop that lives on LDS latency
// being hidden by other wavefronts.  A wavefront's tile is touched by nobody
// else and stays in cache; the old values are requested before the partner
// loop and added after it.  With S = 1 the partial matrices ARE sums[g]; with
// S > 1 they are an engine-owned scratch of S G M^2 doubles (bounded from M by
// the host: OGRID_SCRATCH_ELEMS) and obdm_grid_fold_kernel adds
// s = 0, 1, ..., S - 1 in that order.
//
// Summation order, then: inside a partial matrix configurations in rising
// index, particles in the order of the row; the partial matrices of a group in
// rising s; wsum[g] by 256 strided partial sums and a fixed tree
// (obdm_grid_wsum_kernel).  S depends on (nconf, M, G, N) alone.  No
// floating-point atomics: two calls give the same bits.
//
// fp64 only, as qmc_obdm.h; qmc_engine_set_fast_math does not apply.
#pragma once

#include "qmc_device.h"
#include "qmc_obdm.h"
#include "qmc_obdm_rows.h"

static constexpr int OGRID_U = 2;           // own particles carried by a lane
static constexpr int OGRID_MAX_POINTS = 512;
static constexpr int OGRID_MAX_GROUPS = 1024;

// LDS: the tables of obdm_kernel, then bin[N] and list[N] as ints
static size_t obdm_grid_lds_bytes(int n)
{
    return (size_t)n * OBDM_LDS_PER_PARTICLE * sizeof(double) +
           (size_t)2 * n * sizeof(int);
}

struct ObdmGridArgs {
    const double *pos;     // [nc][N]: the configurations c_base .. c_base + nc
    const double *w;       // [nc] or null
    double *part;          // [S G][M][M] partial matrices (S = 1: sums)
    long long c_base, nc;
    int M, G, S;
    int rows, nrt, nct;    // row bins of a tile, row tiles, column tiles
};

__global__ void __launch_bounds__(64)
obdm_grid_kernel(const DevModel *__restrict__ mp, ObdmGridArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    const int n = m.n, M = a.M;
    const ObdmLds l(smem, n);
    int *bin = (int *)(smem + (size_t)OBDM_LDS_PER_PARTICLE * n);
    int *list = bin + n;
    const int lane = threadIdx.x;
    const bool pairs = !m.is_ideal, onebody = !m.is_free;

    // block -> (partial matrix, row tile, column tile)
    long long b = blockIdx.x;
    const int ct = (int)(b % a.nct); b /= a.nct;
    const int rt = (int)(b % a.nrt); b /= a.nrt;
    const int p = (int)b;
    const int g = p % a.G, s = p / a.G;
    const int r0 = rt * a.rows, r1 = min(M, r0 + a.rows);

    // the lane's column: constants of the launch
    const int col = ct * 64 + lane;
    const bool col_ok = col < M;
    const double delta = m.L / (double)M;
    // (c + 1/2) L first, then the division: the rounding of
    // engine.one_body_matrix_points
    const double xc = ((double)min(col, M - 1) + 0.5) * m.L / (double)M;
    PTab own[OGRID_U];
    sincos_halfpi(xc * m.two_over_L, own[0].s, own[0].c);
    sincos_halfpi(xc * m.k2_2pi, own[0].su, own[0].cu);
    own[1] = own[0];
    const double lf_col = onebody ? obdm_log_f1(m, xc) : 0.0;
    double *__restrict__ acc = a.part + (size_t)p * M * M + min(col, M - 1);
    const double guard = 700.0;                 // domain of exp_bounded

    // members q = s, s + S, ... of group g; the first one inside this tile of
    // the batch
    const long long G = a.G, S = a.S, c_end = a.c_base + a.nc;
    long long q = a.c_base > g ? (a.c_base - g + G - 1) / G : 0;
    q += ((s - q) % S + S) % S;
    for (; g + G * q < c_end; q += S) {
        const long long c = g + G * q - a.c_base;
        const double wc = a.w ? a.w[c] : 1.0;
        __syncthreads();                        // the tables are rewritten
        obdm_fill_tables(m, a.pos + (size_t)c * n, l, lane);
        __syncthreads();
        obdm_unshifted_rows(m, l, lane);
        // the particles of this row tile, in the order of the row
        int cnt = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const int ic = min(i, n - 1);
            const int ai = min((int)floor(l.zbox[ic] / delta), M - 1);
            const bool in = (i < n) & (ai >= r0) & (ai < r1);
            const unsigned long long mask = __ballot(in);
            if (i < n) bin[i] = ai;
            if (in) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = i;
            cnt += __popcll(mask);
        }
        __syncthreads();
        for (int k = 0; k < cnt; k += OGRID_U) {
            int self[OGRID_U], row[OGRID_U];
            bool ok[OGRID_U];
            double dn[OGRID_U], old[OGRID_U];
#pragma unroll
            for (int u = 0; u < OGRID_U; ++u) {
                ok[u] = k + u < cnt;
                self[u] = __builtin_amdgcn_readfirstlane(
                    list[min(k + u, cnt - 1)]);
                row[u] = __builtin_amdgcn_readfirstlane(bin[self[u]]);
                dn[u] = l.den[self[u]];
                // requested here, added after the partner loop
                old[u] = col_ok ? acc[(size_t)row[u] * M] : 0.0;
            }
            ObdmRow r[OGRID_U];
#pragma unroll
            for (int u = 0; u < OGRID_U; ++u) {
                r[u].PL = 0.5; r[u].PS = 0.5; r[u].eL = 1; r[u].eS = 1;
                r[u].cnt = 0;
            }
            if (pairs) obdm_rows<OGRID_U>(m, l.tab, n, own, self, r);
            double v[OGRID_U];
#pragma unroll
            for (int u = 0; u < OGRID_U; ++u) {
                double x = obdm_row_log(m, r[u], lf_col) - dn[u];
                x = fmin(fmax(x, -guard), guard);
                v[u] = wc * exp_bounded(x);
            }
            // the second particle may fall into the first one's row
            const double t0 = old[0] + v[0];
            const double t1 = (row[1] == row[0] ? t0 : old[1]) + v[1];
            if (col_ok) {
                acc[(size_t)row[0] * M] = t0;
                if (ok[1]) acc[(size_t)row[1] * M] = t1;
            }
        }
    }
}

// sums[g][e] = part[0 G + g][e] + part[1 G + g][e] + ... in rising s, e < M^2
__global__ void __launch_bounds__(256)
obdm_grid_fold_kernel(const double *__restrict__ part, int G, int S,
                      long long mm, double *__restrict__ sums)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)G * mm) return;
    double t = 0.0;
    for (int s = 0; s < S; ++s) t += part[(size_t)s * G * mm + idx];
    sums[idx] = t;
}

// wsum[g] = sum of w over the members of group g (w null: their number).  One
// block per group; thread t adds members t, t + 256, ... in rising order, a
// fixed tree adds the 256 partial sums.
__global__ void __launch_bounds__(256)
obdm_grid_wsum_kernel(const double *__restrict__ w, long long nconf, int G,
                      double *__restrict__ wsum)
{
    __shared__ double s0[256];
    const int g = blockIdx.x, t = threadIdx.x;
    double a0 = 0.0;
    for (long long c = g + (long long)G * t; c < nconf; c += 256ll * G)
        a0 += w ? w[c] : 1.0;
    s0[t] = a0;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) s0[t] += s0[t + h];
        __syncthreads();
    }
    if (t == 0) wsum[g] = s0[0];
}
