// qmc_evolve2.h -- the second-order DMC propagator (qmc_dmc_params.propagator
// = 1): dmc_evolve2_kernel, next to dmc_evolve_kernel (qmc_kernels.h), which
// it leaves as it is.  An extension: the reference has the linear step only.
//
// One time step of child slot s with parent p = ref[s], step counter t, in the
// units of the rest of the library (hbar^2 / 2m = 1, F = grad log psi, velocity
// 2 F):
//
//     R_a = wrap(R_p + sqrt(dt) xi1)          half diffusion
//     R_m = wrap(R_a + dt F(R_a))             midpoint of the drift flow
//     R_b = wrap(R_a + 2 dt F(R_m))           full drift, RK2
//     R'  = wrap(R_b + sqrt(dt) xi2)          half diffusion
//     log w' = -dt ((E(R') + E_p) / 2 - E_ref)
//
// the symmetric composition branching/2 . diffusion/2 . drift . diffusion/2 .
// branching/2 with the drift flow integrated to second order: the time-step
// error of the mixed estimators is O(dt^2).  The parent's stored drift is not
// used (F(R') is stored all the same); the weight averages with the PARENT's
// energy whatever `fix_stale` says -- the stale-slot quirk would
// break the symmetry; `eslot` is maintained as the linear kernel does.
//
// xi1, xi2: the two Box-Muller normals of ONE Philox block, dmc_normal2(seed,
// slot0 + s, t, label) -- keyed with t, not t >> 1: in the oracle's terms
// dmc_normal(seed, slot, 2 t, label) and dmc_normal(seed, slot, 2 t + 1, label).
// No spare row: `spare` and `spare_nw` are neither read nor written.  A tape
// holds [slot][2][N] normals per step, the xi1 row, then the xi2 row.
//
// Three pair sums per walker, each on a freshly ordered row and each deciding
// `fast` (sorted rows or the general sum, counted in `diag`) for itself.  The
// three are ONE loop body run three times -- the body holds the sorted-row sum
// and its general fallback, the largest pieces of code in the library; unrolled
// it would be three copies of both -- so the two intermediate stages compute an
// energy nobody reads (the quotient sums the drift needs are the energy's).
// Between the stages only a lane's positions and labels are live in registers.
// Labels travel with the sorts, so what is addressed by PARTICLE waits in two
// rows behind the walker's pair tables in LDS, indexed by label: R_a (read back
// after the second sort) and xi2 (drawn with xi1, used after it).
#pragma once

#include "qmc_kernels.h"

// LDS doubles per lane group: the linear kernel's region (sorted rows or the
// general layout, whichever is larger) + R_a[G P] + xi2[G P]
template <int G, int P, bool PAD, bool ZC>
struct Step2Lds {
    static constexpr int TABLES = StepLds<G, P, PAD, ZC, true>::DOUBLES;
    static constexpr int DOUBLES = TABLES + 2 * G * P;
};

// Minimum waves per SIMD asked of the register allocator.  The loop keeps a
// lane's row, its labels and the stage across the pair sums, a handful of
// registers more than the linear kernel has live there: held to that kernel's
// figures (lb_waves: 7 waves at N <= 64, 5 on the sorted rows of N <= 128) the
// N <= 128 shape spills 48-68 bytes per lane and the padded position-classified
// N <= 64 shape 16.  One wave fewer for those: no instantiation of the shapes
// with one or two particles per lane uses scratch.  (6.5 KB of LDS per walker
// at N <= 128: the 16 walkers of four waves per SIMD fit with room to spare.)
constexpr int lb2_waves(int G, int P, bool ZC)
{
    return (G == 64 && P == 1) ? (ZC ? 6 : LB_P1)
           : (G == 64 && P == 2 && !ZC) ? 4 : 1;
}

// Lane order before a pair sum, as dmc_evolve_kernel establishes it: the exact
// sort and the once-per-walker condition of the sorted-row shapes (-> true: the
// sorted-row sum may run), the seam / transposition passes of the others.
template <int G, int P, bool PAD, bool ZC>
__device__ __forceinline__ bool evolve2_order(const DevModel &m, double (&z)[P],
                                              int (&lab)[P], int gl, int n,
                                              unsigned step, bool active)
{
    constexpr bool S64 = G == 64 && P == 1 && !ZC;
    constexpr bool S128 = G == 64 && P == 2 && !ZC;
    bool fast = false;
    if constexpr (S64) {
        fast = !m.is_ideal && sort_lanes64(z[0], lab[0], gl, PAD ? n : 64) &&
               (PAD ? far_partner_ok_ring(m, z[0], gl, n)
                    : far_partner_ok64(m, z[0], gl));
    } else if constexpr (S128) {
        fast = !m.is_ideal && (!PAD || (n & 1) == 0) &&
               sort_rows128(z, lab, gl, PAD ? n / 2 : 64) &&
               (PAD ? far_partner_ok_ring128(m, z, gl, n / 2)
                    : far_partner_ok128(m, z, gl));
    }
    if constexpr (S64 || S128) {
        // (diagnostic, cold path only: evaluations that leave the sorted rows)
        if (!fast && !m.is_ideal && gl == 0 && active)
            atomicAdd(m.diag, 1ull);
    } else if constexpr (G == 64 && P == 1) {
        anchor_seam(z[0], lab[0], n);
        if ((step % RESORT_EVERY) == 0)
            resort_linear<G>(z[0], lab[0], gl, step / RESORT_EVERY, n);
    } else if constexpr (SlotMap<G, P>::CONSECUTIVE) {
        anchor_seam_rows<P>(z, lab, n);
        if ((step % RESORT_EVERY) == 0)
            resort_linear_rows<P>(z, lab, gl, step / RESORT_EVERY, n);
    } else if ((step % RESORT_EVERY) == 0)
        resort_step<G, P>(z, lab, gl, step / RESORT_EVERY, n, m.L,
                          m.half_L, lanes_in_use<G, PAD>(m));
    return fast;
}

template <int G, int P, bool PAD, bool ZC, typename R = double>
__global__ void __launch_bounds__(WalkBlock<G>::N, lb2_waves(G, P, ZC))
dmc_evolve2_kernel(const DevModel *__restrict__ mp, EvolveArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    constexpr int GPB = WalkBlock<G>::N / G;
    constexpr int TABLES = Step2Lds<G, P, PAD, ZC>::TABLES;
    static_assert(TABLES >= GroupLds<G, P, ZC>::DOUBLES,
                  "eval_walker is the fallback on the same LDS region");
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    double *lds = smem + (size_t)grp * Step2Lds<G, P, PAD, ZC>::DOUBLES;
    // by particle label (< n <= G P), behind the pair tables
    double *l_ra = lds + TABLES, *l_xi = l_ra + G * P;
    const long long s = walker_of_block<GPB>(blockIdx.x, grp);
    const long long nw = a.ctl->nw;
    // whole block beyond the population: nothing to do
    if ((GPB == 1 ? s : (long long)blockIdx.x * GPB) >= nw) return;
    const bool active = s < nw;
    const long long sr = active ? s : 0;
    const int n = walker_n<G, P, PAD>(m);
    const unsigned int step = a.ctl->step;
    const double ref_energy = a.ctl->ref_energy;
    const long long su = (G == 64) ? qmc_uniform(sr) : sr;
    const long long par = a.ref[su];
    double e_par = 0.0;
    if (G == 64) e_par = a.penergy[par];
    // a.sigma: sqrt(dt), the spread of HALF the diffusion (qmcwalk.hip)
    const double half_spread = a.sigma;

    // ---- R_a = wrap(R_p + sqrt(dt) xi1); R_a and xi2 to their label's entry
    double z[P];
    int lab[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        int i = lane_particle<G, P, PAD>(m, gl, p);
        double zz = 0.0;
        lab[p] = i;
        if (i < n) {
            const double z0 = a.ppos[par * n + i];
            // random numbers belong to the particle (label), not to the lane
            const int li = (int)a.plabel[par * n + i];
            lab[p] = li;
            double g1, g2;
            if (a.g_tape) {
                g1 = a.g_tape[(sr * 2) * n + li];
                g2 = a.g_tape[(sr * 2 + 1) * n + li];
            } else {
                dmc_normal2(a.seed, a.slot0 + (unsigned)sr, step, (unsigned)li,
                            g1, g2);
            }
            zz = wrap_box(z0 + half_spread * g1, m.L);
            l_ra[li] = zz;
            l_xi[li] = g2;
        }
        z[p] = zz;
    }

    double F[P], ei[P], e_next = 0.0, wf;
    // (not unrolled: one copy of the pair sums, see the head of this file)
#pragma clang loop unroll(disable)
    for (int stage = 0; stage < 3; ++stage) {
        const bool fast =
            evolve2_order<G, P, PAD, ZC>(m, z, lab, gl, n, step, active);
        if (stage == 2) {
            // R' and its labels leave now: not live across the last pair sum
#pragma unroll
            for (int p = 0; p < P; ++p) {
                int i = lane_particle<G, P, PAD>(m, gl, p);
                if (active && i < n) {
                    a.cpos[s * n + i] = z[p];
                    a.clabel[s * n + i] = (unsigned short)lab[p];
                }
            }
        }
        constexpr bool S64 = G == 64 && P == 1 && !ZC;
        constexpr bool S128 = G == 64 && P == 2 && !ZC;
        if (S64 && fast) {
            if constexpr (S64)
                eval_sorted64<R, false, true, false, PAD>(m, z[0], gl, lds,
                                                          F[0], e_next, wf);
        } else if (S128 && fast) {
            if constexpr (S128)
                eval_sorted128<R, false, true, false, PAD>(m, z, gl, lds, F,
                                                           e_next, wf);
        } else
            eval_walker<G, P, PAD, false, false, ZC, R>(m, z, z, gl, lds, F, ei,
                                                        e_next, wf);
        if (stage == 2) break;
        // (the pair sums read their tables through LDS: every lane is past
        // them, and past the stores of R_a and xi2, before the rows are read)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int p = 0; p < P; ++p) {
            int i = lane_particle<G, P, PAD>(m, gl, p);
            double zz = 0.0;
            if (i < n) {
                if (stage == 0) {
                    // R_m = wrap(R_a + dt F_a): this lane still holds R_a
                    zz = wrap_box(z[p] + a.dt * F[p], m.L);
                } else {
                    // R' = wrap(wrap(R_a + 2 dt F_m) + sqrt(dt) xi2)
                    const double zb =
                        wrap_box(l_ra[lab[p]] + 2 * a.dt * F[p], m.L);
                    zz = wrap_box(zb + half_spread * l_xi[lab[p]], m.L);
                }
            }
            z[p] = zz;
        }
    }
    if (!active) return;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        int i = lane_particle<G, P, PAD>(m, gl, p);
        if (i < n) a.cdrift[s * n + i] = F[p];
    }
    if (gl == 0) {
        if (G != 64) e_par = a.penergy[par];
        // always the parent's energy (the symmetric split); the logarithm of
        // the weight, as dmc_evolve_kernel stores it
        const double mean_energy = (e_next + e_par) / 2;
        a.cenergy[s] = e_next;
        a.cweight[s] = -a.dt * (mean_energy - ref_energy);
        a.eslot[s] = e_par;
    }
}
