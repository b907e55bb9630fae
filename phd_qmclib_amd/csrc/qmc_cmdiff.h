// qmc_cmdiff.h -- centre-of-mass diffusion of a DMC population: the
// winding-number estimator of the superfluid fraction (an extension: the
// reference has none),
//
//   rho_s / rho = lim_{tau -> inf} N <(X_cm(tau) - X_cm(0))^2> / (2 D tau),
//
// D = 1 in these units (sigma = sqrt(2 dt)), in the frame of the other DMC
// estimators (qmc_kernels_misc.h: EstArgs, est_reduce_kernel).
//
// Walker s of step t carries the configuration of its parent,
// ppos[ref_t[s]]; when the estimators of step t run, row s of the child buffer
// holds the configuration evolved from that parent.
//
//   raw      = sum_i (cpos[s][i] - ppos[ref_t[s]][i])
//   d_t(s)   = raw - L rint(raw / L)
//   Y_t(s)   = aux_{t-1}[ref_t[s]]          (0 at the first step of a block)
//   aux_t[s] = Y_t(s) + d_t(s)
//   iter[t]  = (sum_{s live} Y_t(s), sum_{s live} Y_t(s)^2)
//
// Y_t(s) is N times the unwrapped centre-of-mass displacement of the yielded
// walker since the first yielded state of the block; the rows travel through
// the cloning table as the S(k) parts do (a clone inherits the history of its
// parent, a dead walker's history ends).  The sum over the particles does not
// change under a permutation of a row, and a wrap of a particle by L changes
// raw by L, which the minimum image takes out again: the sorted rows, the
// labels and the wrap convention of the stepping kernels do not matter.
//
// CONDITION: |sum_i displacement_i| < L / 2 in every time step, or the minimum
// image picks the wrong winding.  The sum is about sqrt(2 N dt) (0.3 at
// N = 64, dt = 1e-3) against L / 2 >= 4: far from binding.
//
// One wavefront per walker slot, grid-striding over the live slots; lane
// i + 64 p forms the difference at index i + 64 p, the passes add up in the
// lane in index order, the lanes in the fixed order of group_sum<64>.  Lane 0
// does the minimum image, the transport and the two sums of its wavefront; the
// wavefronts of a block add up in index order, est_reduce_kernel sums the
// blocks (divisor 1).  fp64 whatever fast_math says; any N.
__global__ void __launch_bounds__(BLOCK) dmc_cm_diffusion_kernel(EstArgs a)
{
    constexpr int NWAVE = BLOCK / 64;
    __shared__ double red[NWAVE][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = a.n;
    const double L = a.scale;
    const long long nw = a.ctl->nw;
    const long long wstride = (long long)gridDim.x * NWAVE;
    double sum_y = 0.0, sum_y2 = 0.0;           // (lane 0 only)
    for (long long s = (long long)blockIdx.x * NWAVE + wave; s < nw;
         s += wstride) {
        const long long par = a.ref[s];
        const double *prow = a.ppos + (size_t)par * n;
        const double *crow = a.cpos + (size_t)s * n;
        double diff = 0.0;
        for (int i = lane; i < n; i += 64) diff += crow[i] - prow[i];
        const double raw = group_sum<64>(diff);
        if (lane == 0) {
            const double y = a.aux_prev[par];
            a.aux_act[s] = y + (raw - L * rint(raw / L));
            sum_y += y;
            sum_y2 += y * y;
        }
    }
    if (lane == 0) {
        red[wave][0] = sum_y;
        red[wave][1] = sum_y2;
    }
    est_block_sum(&red[0][0], 2, 2, a.partial);
}
