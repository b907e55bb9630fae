// qmc_energy_parts.h -- the local energy of a configuration split into its
// kinetic, lattice and interaction parts, and Tan's contact in windows.
//
// With H = -sum d_i^2 + sum V(z_i) + g sum_{i<j} delta(z_ij) and a Jastrow
// factor that carries the exact contact cusp, the reference's local energy
// (qmc_base/jastrow/model.py:681-743) leaves the delta term out: the cusp
// accounts for it.  Integrating by parts, for any state sampled from |psi|^2
//     <sum_i F_i^2>               = T       the kinetic energy, F = d ln psi
//     <E_L - sum F_i^2 - sum V>   = E_int   = g <sum_{i<j} delta(z_ij)>
// with g = 4 kappa, kappa = f2'(0+) / f2(0) = k2 tan(k2 r_off).  The second
// route to E_int counts the pairs inside a window r_k and divides the cusp of
// the pair density out of them:
//     C_k = 1 / (2 r_k) sum_{i<j, d_ij < r_k}
//               [cos(k2 r_off) / cos(k2 (d_ij - r_off))]^2
// (d_ij the minimum-image distance, the compare strict): f2(0)^2 / f2(d)^2,
// which holds inside the contact cutoff only -- the host refuses a window
// beyond it.  On an ideal model the weight is 1 and C_k is the plain
// coincidence density.
//
// One row of 4 + K doubles per configuration, always in fp64:
//     E, T, V, I = (E - T) - V, C_0 .. C_{K-1}
// One lane group per configuration, as evaluate_kernel (qmc_kernels.h).  E and
// the drift come from eval_walker, i.e. from the pair sums the steppers use; V
// is the potential that energy contains (mrbp_qmc/model.py:533-551): the
// barrier test on the position as given, the defect cells by floor(z).  The
// windows are a second pass: the row of wrapped positions goes to LDS, in the
// region the pair tables have left, and every lane walks it for its own
// particles -- a broadcast read, a subtraction and a compare per pair; the
// cosine and the quotient run for the pairs inside the largest window only.
// The sums run in a fixed order: two calls return the same bits.
#pragma once

#include "qmc_kernels.h"

static constexpr int EP_COLS = 4;            // E, T, V, I
static constexpr int EP_MAX_RANGES = 16;

struct EnergyPartsArgs {
    const double *pos;   // [nconf][N]
    double *parts;       // [nconf][EP_COLS + K]
    long long nconf;
    int K;
    double rmax;                   // the largest window
    double r[EP_MAX_RANGES];       // the windows (entries from K on: 0)
};

// V(z) of one particle (mrbp_qmc/model.py:533-551), with the region test and
// the cell of one_body / one_body_kin_const
__device__ __forceinline__ double lattice_potential(const DevModel &m, double z)
{
    const double cell = floor(z);
    if (!(m.z_a < z - cell)) return 0.0;
    if (m.uniform_barrier) return m.v_barrier;
    int rr = (int)cell % m.defects_sep;
    if (rr < 0) rr += m.defects_sep;
    return (rr == 0) ? m.v0d : m.v0;
}

template <int G, int P, bool PAD, bool ZC>
__global__ void __launch_bounds__(WalkBlock<G>::N)
energy_parts_kernel(const DevModel *__restrict__ mp, EnergyPartsArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    constexpr int GPB = WalkBlock<G>::N / G;            // groups per block
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    double *lds = smem + (size_t)grp * GroupLds<G, P, ZC>::DOUBLES;
    const long long w = walker_of_block<GPB>(blockIdx.x, grp);
    const bool active = w < a.nconf;
    if (GPB == 1 && !active) return;      // (no one else in the workgroup)
    const long long wr = active ? w : 0;
    const int n = walker_n<G, P, PAD>(m);
    const int K = a.K;
    double z[P], z1[P], F[P], ei[P], E = 0.0, wf;
    int idx[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        idx[p] = lane_particle<G, P, PAD>(m, gl, p);
        // (pair tables and windows from the image inside the box, one-body
        // factor and V from the position as given -- evaluate_kernel)
        z1[p] = (idx[p] < n) ? a.pos[wr * n + idx[p]] : 0.0;
        z[p] = wrap_box(z1[p], m.L);
    }
    eval_walker<G, P, PAD, false, false, ZC, double>(m, z, z1, gl, lds, F, ei,
                                                     E, wf);
    double t_lane = 0.0, v_lane = 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (idx[p] < n) {
            t_lane = fma(F[p], F[p], t_lane);
            if (!m.is_free) v_lane += lattice_potential(m, z1[p]);
        }
    const double T = group_sum<G>(t_lane);
    const double V = group_sum<G>(v_lane);
    double *row = a.parts + (size_t)wr * (EP_COLS + K);
    if (active && gl == 0) {
        row[0] = E;
        row[1] = T;
        row[2] = V;
        row[3] = (E - T) - V;
    }
    if (K <= 0) return;

    // ---- the windows ----
    // every lane of the wave is done with the pair tables: the row of wrapped
    // positions takes their place (n <= GroupLds::ROW)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (idx[p] < n) lds[idx[p]] = z[p];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    double acc[EP_MAX_RANGES];
#pragma unroll
    for (int k = 0; k < EP_MAX_RANGES; ++k) acc[k] = 0.0;
    const double rmax = a.rmax, L = m.L;
    const bool ideal = m.is_ideal != 0;
    for (int j = 0; j < n; ++j) {
        const double zj = lds[j];             // one address per group
#pragma unroll
        for (int p = 0; p < P; ++p) {
            double d = fabs(z[p] - zj);
            d = fmin(d, L - d);
            // every pair once, from its lower index (an idle lane holds n)
            if (idx[p] < j && d < rmax) {
                double wgt = 1.0;
                if (!ideal) {
                    // cos(k2 (d - r_off)) by the angle addition: k2 d < pi/2
                    // inside the contact cutoff
                    double s, c;
                    sincos_halfpi(d * m.k2_2pi, s, c);
                    const double q =
                        fast_div(m.cphi, fma(c, m.cphi, s * m.sphi));
                    wgt = q * q;
                }
#pragma unroll
                for (int k = 0; k < EP_MAX_RANGES; ++k)
                    if (k < K && d < a.r[k]) acc[k] += wgt;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < EP_MAX_RANGES; ++k) {
        if (k < K) {          // (K is uniform: whole waves take the sum)
            const double c = group_sum<G>(acc[k]);
            if (active && gl == 0) row[EP_COLS + k] = c / (2.0 * a.r[k]);
        }
    }
}

// the instantiations: one translation unit (inst_EPARTS.hip); qmcwalk.hip sees
// them as `extern template` declarations (the shapes and their (PAD, ZC)
// variants follow qmc_inst.h)
#define QMC_INST_EPARTS(KW, G, P, PAD, ZC)                                    \
    KW template __global__ void energy_parts_kernel<G, P, PAD, ZC>(           \
        const DevModel *, EnergyPartsArgs);
#define QMC_INST_EPARTS_SMALL(KW, G, P)                                       \
    QMC_INST_EPARTS(KW, G, P, false, false)                                   \
    QMC_INST_EPARTS(KW, G, P, false, true)                                    \
    QMC_INST_EPARTS(KW, G, P, true, false)                                    \
    QMC_INST_EPARTS(KW, G, P, true, true)
#define QMC_INST_EPARTS_MASKED(KW, G, P)                                      \
    QMC_INST_EPARTS(KW, G, P, true, false) QMC_INST_EPARTS(KW, G, P, true, true)
#define QMC_TU_EPARTS(KW)                                                     \
    QMC_INST_EPARTS_SMALL(KW, 16, 1) QMC_INST_EPARTS_SMALL(KW, 16, 2)         \
    QMC_INST_EPARTS_SMALL(KW, 32, 2) QMC_INST_EPARTS_SMALL(KW, 64, 1)         \
    QMC_INST_EPARTS_SMALL(KW, 64, 2) QMC_INST_EPARTS_MASKED(KW, 64, 4)        \
    QMC_INST_EPARTS_MASKED(KW, 64, 8)
