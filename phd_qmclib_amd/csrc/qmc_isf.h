// qmc_isf.h -- imaginary-time density correlations of a DMC population (an
// extension: the reference has none),
//
//   F(k, tau) = <rho_k(tau) rho_-k(0)>,   rho_k = sum_i exp(i k z_i),
//
// which decays as sum_n |<n|rho_k|0>|^2 exp(-(E_n - E_0) tau): the excitation
// spectrum.  In the frame of the other DMC estimators (qmc_kernels_misc.h:
// EstArgs, est_reduce_kernel).
//
// Parameters: K modes k_m = 2 pi m / L, m = 0 .. K-1 (the mode set of S(k));
// T lags; lag stride q >= 1, lag l is tau_l = l q dt.  C = T + 2; a walker row
// has K C doubles, laid out [m][c].
//
// At step t of a block walker s carries R = ppos[ref_t[s]], rho_m = rho_m(R):
//
//   t = 0:  row = 0, then row[m][T] = Re rho_m, row[m][T+1] = Im rho_m (the
//           origin) and row[m][0] = (Re rho_m)^2 + (Im rho_m)^2; aux_prev is
//           not read.
//   t > 0:  row = aux_{t-1}[ref_t[s]]; if t % q == 0 and l = t / q < T,
//           row[m][l] = Re rho_m row[m][T] + Im rho_m row[m][T+1].
//   both:   aux_t[s] = row,  iter[t] = sum_{s < nw_t} row   (divisor 1).
//
// A clone inherits the row of its parent, a dead walker's row ends.  The
// walkers of step t are distributed as psi_T phi_0 and weighting an ancestor
// by its descendants makes the earlier end pure, so iter[t][m][l] / nw_t
// estimates F(k_m, tau_l) with projection time (t - l q) dt behind the later
// end: pure in the limit of a long block, read at the last step of the block;
// lags close to the end of the block are mixed at their later end.  Columns T
// and T+1 give the pure <rho_m> at the same projection.
//
// One wavefront per walker slot, grid-striding over the live slots.  At a step
// that measures (t = 0, or t = l q with l < T; uniform over the launch) the
// wavefront forms rho_m of its walker with the routine of the S(k) kernel for
// up to 64 modes (qmc_kernels_misc.h: rho_modes8, the factor tables, the
// matrix-core tile and its lane map are described there); any N.  Lane m then
// holds rho_m and hands it to the others through LDS.  At any other step no
// rho is formed.  Lanes take the row indices lane + 64 j for the coalesced
// copy aux_prev[par] -> aux_act[s], replace the measured column on the way and
// keep per-lane running sums; est_block_sum adds up the wavefronts of a block
// into partial[block][K C], est_reduce_kernel sums the blocks.  fp64 whatever
// fast_math says; no atomics.
static constexpr int ISF_MAXROW = 1024;          // K (T + 2) at most
static constexpr int ISF_NJ = ISF_MAXROW / 64;   // row indices per lane

__global__ void __launch_bounds__(BLOCK) dmc_isf_kernel(EstArgs a)
{
    using S = SsfShape<8>;
    constexpr int NWAVE = BLOCK / 64;
    static_assert(NWAVE * S::WAVE_DOUBLES >= NWAVE * ISF_MAXROW,
                  "the block reduction reuses the tables' LDS");
    __shared__ double smem[NWAVE * S::WAVE_DOUBLES];
    __shared__ double rho[NWAVE][2][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *X = smem + (size_t)wave * S::WAVE_DOUBLES;   // F_a (rows of D)
    double *Y = X + S::ROWS * S::RS;                     // E_b (columns of D)
    const int n = a.n;
    const int T = (int)a.pfw, C = T + 2, A = a.K * C;
    const long long t = a.step_idx;
    const bool first = t == 0;
    const long long lag = t / a.stride;
    const bool measure = first || (t % a.stride == 0 && lag < T);
    const int col = first ? 0 : (int)lag;       // the column measured now
    const long long nw = a.ctl->nw;
    const long long wstride = (long long)gridDim.x * NWAVE;
    // what this lane does to row index lane + 64 j at a measuring step:
    // 4 m + kind, kind 0 copy, 1 the measured column, 2 / 3 the origin (t = 0)
    int sel[ISF_NJ];
    double acc[ISF_NJ];
#pragma unroll
    for (int j = 0; j < ISF_NJ; ++j) {
        const int i = lane + 64 * j;
        const int m = i / C, c = i - m * C;
        int kind = 0;
        if (measure && i < A) {
            if (c == col) kind = 1;
            else if (first && c == T) kind = 2;
            else if (first && c == T + 1) kind = 3;
        }
        sel[j] = 4 * m + kind;
        acc[j] = 0.0;
    }
    for (long long s = (long long)blockIdx.x * NWAVE + wave; s < nw;
         s += wstride) {
        const long long par = a.ref[s];
        if (measure) {
            double re, im;                  // rho of mode `lane`
            rho_modes8(a.ppos + par * n, n, a.scale, X, Y, lane, re, im);
            rho[wave][0][lane] = re;
            rho[wave][1][lane] = im;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        const double *prow = a.aux_prev + (size_t)par * A;
        double *arow = a.aux_act + (size_t)s * A;
#pragma unroll
        for (int j = 0; j < ISF_NJ; ++j) {
            const int i = lane + 64 * j;
            if (64 * j >= A) break;
            if (i < A) {
                double v = first ? 0.0 : prow[i];
                const int kind = sel[j] & 3, m = sel[j] >> 2;
                if (kind) {
                    const double re = rho[wave][0][m], im = rho[wave][1][m];
                    if (kind == 2) v = re;
                    else if (kind == 3) v = im;
                    else if (first) v = fma(re, re, im * im);
                    else v = fma(re, prow[m * C + T], im * prow[m * C + T + 1]);
                }
                arow[i] = v;
                acc[j] += v;
            }
        }
        __builtin_amdgcn_wave_barrier();    // rho is rewritten next
    }
    __syncthreads();                       // the tables' LDS is reused
    double *red = smem;                    // [NWAVE][ISF_MAXROW]
#pragma unroll
    for (int j = 0; j < ISF_NJ; ++j)
        red[wave * ISF_MAXROW + lane + 64 * j] = acc[j];
    est_block_sum(red, ISF_MAXROW, A, a.partial);
}
