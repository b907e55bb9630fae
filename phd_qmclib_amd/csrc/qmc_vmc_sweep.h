// qmc_vmc_sweep.h -- single-particle Metropolis sweeps (qmc_vmc_params.gaussian
// = QMC_VMC_PARTICLE): vmc_sweep_kernel, next to vmc_step_kernel
// (qmc_kernels.h), which it leaves as it is.  An extension: the reference
// defines the one-particle ratio (delta_wf_abs_log_kth_move), never calls it.
//
// One yield = one sweep of chain c (Philox slot chain0 + c) at step counter t:
// the particles are visited in LABEL order k = 0 .. N - 1 (the label is the
// index of the particle in the caller's rows, so the chain does not depend on
// the order a row is kept in),
//
//     (w0, w1) = vmc_move_block(seed, slot, t, k)
//     z'       = wrap_box(z_k + vmc_move_unit(w0) * move_spread, L)
//     D        = log f1(z') - log f1(z_k)
//                + sum_{j != k} [log f2(|d(z', z_j)|) - log f2(|d(z_k, z_j)|)]
//     u        = (w1 + 1/2) 2^-32           accept  <=>  log u < 2 D
//
// with z_j the CURRENT positions, the moves accepted earlier in the sweep
// included.  Word 0 of a particle's block moves it, as in the all-particle
// step; word 1 of the same block is that move's accept draw.
//
// Layout.  A lane group (G, P) of the engine's shape owns one chain for all
// the yields of a launch.  Its row and labels stay in registers in slot order,
// as in the stepping kernels; what the sweep addresses by PARTICLE lives in
// LDS, indexed by label, behind the region of the pair sums:
//
//     tab [n][4]  {sin, cos}(pi z / L), {sin, cos}(k2 z) of the current row
//     ntab[n][4]  the same of the proposals         zl[n]  current positions
//     nz  [n]     proposed positions                lu [n]  log u
//     dlf [n]     log f1(z') - log f1(z)
//
// A particle is moved once per sweep, so everything that belongs to the move
// alone -- the Philox block, z', its four table entries (two sincos), both
// one-body logarithms and log u -- does not depend on the moves before it and
// is computed for all N particles at once before the serial part, lane gl
// taking the labels P gl .. P gl + P - 1.  The serial part, per k: every lane
// reads the moved particle's two table entries (one address: a broadcast) and
// forms the shifted and the unshifted pair factor against ITS P partners with
// obdm_rows<2> (qmc_obdm_rows.h: image inside the box, obdm_wrap_tab, short /
// long select, exponent folding -- nothing of it is restated here; one read of
// a partner's entry serves both factors).  A lane holds at most 8 partners and
// the products are folded as in g1(s): none can leave the fp64 range at any N
// or cutoff.  Each lane takes the logarithm of ITS shifted row over its
// unshifted row (obdm_row_log of the quotient: two logarithms, which cost a
// wavefront the same whether one lane or all of them take them), and ONE
// number per lane is summed over the group (group_sum: DPP rotations inside
// the rows of 16 lanes, two exchanges across them).  With the one-body
// difference that is D; the group takes the sum of its first lane, so the
// decision is the same in every lane.  An accepted move copies entry k of
// ntab / nz to tab / zl.  The sum and the logarithms before it are a dependent
// chain per move; what hides it is the other wavefronts of the SIMD (DESIGN
// section 4).
//
// The yielded log|psi| and local energy are computed IN FULL at the end of the
// sweep -- nothing accumulates the D -- by the routines of vmc_step_kernel:
// the lanes fetch their particles' positions by label, the row is put in
// ascending order (the exact in-register sorts and the sorted-row sums on their
// shapes; on the others eval_walker behind a rank count through LDS, which
// needs none of the dynamically indexed registers -- scratch -- of the seam /
// transposition passes the stepping kernels run at four and eight particles
// per lane), log|psi| pass and energy pass.  A sweep that accepted nothing
// carries both values over, and leaves the row as it is.  The rows leave the
// launch position-sorted with their labels, set_state's invariant (as in
// vmc_step_kernel a row given outside the box stays in the order given until
// the sweep that brings it in, and an ideal gas is not sorted on the
// sorted-row shapes: eval_walker takes any order).
//
// fp64 throughout: qmc_engine_set_fast_math does not apply (a float row
// product underflows, qmc_obdm.h).
#pragma once

#include "qmc_kernels.h"
#include "qmc_obdm_rows.h"

// doubles per particle slot behind the pair-sum region (see above)
static constexpr int SWEEP_LDS_PER_SLOT = 12;

template <int G, int P, bool PAD, bool ZC>
struct SweepLds {
    static constexpr int TABLES = StepLds<G, P, PAD, ZC>::DOUBLES;
    static constexpr int SLOTS = G * P;
    static constexpr int DOUBLES = TABLES + SWEEP_LDS_PER_SLOT * SLOTS;
};

// the LDS of a group is touched by its own wavefront only
__device__ __forceinline__ void sweep_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the value of the group's first lane, in every lane of the group
template <int G>
__device__ __forceinline__ double sweep_first(double v, int gl)
{
    if constexpr (G == 64) return qmc_uniform_f64(v);
    return __shfl(v, (int)(threadIdx.x & 63) - gl, 64);
}

// some lane of the group says so
template <int G>
__device__ __forceinline__ bool sweep_any(bool b, int gl)
{
    const unsigned long long bal = __ballot(b);
    if constexpr (G == 64) return bal != 0ull;
    const int base = (int)(threadIdx.x & 63) - gl;
    return ((bal >> base) & ((1ull << (G & 63)) - 1ull)) != 0ull;
}

// What a lane's partners contribute to D: the logarithm of its shifted row
// over its unshifted row.  Both rows hold the same partners, so the quotient of
// the folded mantissas stays within (1/2, 2) and the exponents, the short
// counts subtract: two logarithms per lane instead of four (a lane without
// partners gives exactly 0).
__device__ __forceinline__ double sweep_lane_log(const DevModel &m,
                                                 const ObdmRow (&r)[2])
{
    ObdmRow q;
    q.PL = r[0].PL * fast_rcp(r[1].PL);
    q.PS = r[0].PS * fast_rcp(r[1].PS);
    q.eL = r[0].eL - r[1].eL;
    q.eS = r[0].eS - r[1].eS;
    q.cnt = r[0].cnt - r[1].cnt;
    return obdm_row_log(m, q, 0.0);
}

// Put the row (z = zl[lab], just read) in ascending order and evaluate
// log|psi| and the local energy of it with the routines of vmc_step_kernel.
// The one-body factor sees the positions as they are stored; they differ from
// their images in the box only in a row given outside it, which is not
// reordered.  -> the values of the group's first lane.
template <int G, int P, bool PAD, bool ZC>
__device__ __forceinline__ void sweep_eval(const DevModel &m, double (&z)[P],
                                           int (&lab)[P], int gl, int n,
                                           bool active, double *lds,
                                           const double *zl, double *sz,
                                           double *sl, double &wf, double &en)
{
    constexpr bool S64 = G == 64 && P == 1 && !ZC;
    constexpr bool S128 = G == 64 && P == 2 && !ZC;
    constexpr bool TWO_PASS = G == 64;
    double zn[P];
    bool out = false;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        zn[p] = wrap_box(z[p], m.L);
        out = out || zn[p] != z[p];
    }
    const bool outside = sweep_any<G>(out, gl);
    bool fast = false;
    if (!outside) {
        if constexpr (S64) {
            fast = !m.is_ideal &&
                   sort_lanes64(z[0], lab[0], gl, PAD ? n : 64) &&
                   (PAD ? far_partner_ok_ring(m, z[0], gl, n)
                        : far_partner_ok64(m, z[0], gl));
        } else if constexpr (S128) {
            fast = !m.is_ideal && (!PAD || (n & 1) == 0) &&
                   sort_rows128(z, lab, gl, PAD ? n / 2 : 64) &&
                   (PAD ? far_partner_ok_ring128(m, z, gl, n / 2)
                        : far_partner_ok128(m, z, gl));
        } else {
            // No in-register sort on this shape: every particle counts the
            // row entries below it (ties go by label) and the row is handed
            // round through LDS, `sz` / `sl`: the proposal rows, free between
            // two sweeps.  Exactly ascending, as set_state leaves a row.
            int rk[P];
#pragma unroll
            for (int p = 0; p < P; ++p) rk[p] = 0;
            for (int j = 0; j < n; ++j) {
                const double zj = zl[j];
#pragma unroll
                for (int p = 0; p < P; ++p)
                    rk[p] += ((zj < z[p]) |
                              ((zj == z[p]) & (j < lab[p]))) ? 1 : 0;
            }
            int *sli = reinterpret_cast<int *>(sl);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if (lane_particle<G, P, PAD>(m, gl, p) < n) {
                    sz[rk[p]] = z[p];
                    sli[rk[p]] = lab[p];
                }
            }
            sweep_sync();
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int i = lane_particle<G, P, PAD>(m, gl, p);
                if (i < n) { z[p] = sz[i]; lab[p] = sli[i]; }
            }
            sweep_sync();
        }
#pragma unroll
        for (int p = 0; p < P; ++p) zn[p] = z[p];
    }
    if constexpr (S64 || S128) {
        // (diagnostic, cold path only: rows that leave the sorted-row path)
        if (!fast && !m.is_ideal && gl == 0 && active)
            atomicAdd(m.diag, 1ull);
    }
    double F[P], ei[P], e_new = 0.0, wf_new = 0.0, wf_unused;
    if (S64 && fast) {
        if constexpr (S64) {
            eval_sorted64<double, true, false, false, PAD>(m, zn[0], gl, lds,
                                                           F[0], e_new, wf_new);
            eval_sorted64<double, false, true, true, PAD>(m, zn[0], gl, lds,
                                                          F[0], e_new,
                                                          wf_unused);
        }
    } else if (S128 && fast) {
        if constexpr (S128) {
            eval_sorted128<double, true, false, false, PAD>(m, zn, gl, lds, F,
                                                            e_new, wf_new);
            eval_sorted128<double, false, true, true, PAD>(m, zn, gl, lds, F,
                                                           e_new, wf_unused);
        }
    } else if constexpr (TWO_PASS) {
        eval_walker<G, P, PAD, true, false, ZC, double, false, false>(
            m, zn, z, gl, lds, F, ei, e_new, wf_new);
        eval_walker<G, P, PAD, false, false, ZC, double, true, true>(
            m, zn, z, gl, lds, F, ei, e_new, wf_unused);
    } else {
        eval_walker<G, P, PAD, true, false, ZC, double>(m, zn, z, gl, lds, F,
                                                        ei, e_new, wf_new);
    }
    wf = sweep_first<G>(wf_new, gl);
    en = sweep_first<G>(e_new, gl);
}

// All a.nsteps yields of a block for the chains of the launch, from yield a.y
// = 0 on; a.forced: the first of them is the initial state itself (no sweep;
// it counts N accepted moves); a.step: the counter of the first sweep.
template <int G, int P, bool PAD, bool ZC>
__global__ void __launch_bounds__(WalkBlock<G>::N)
vmc_sweep_kernel(const DevModel *__restrict__ mp, VmcArgs a)
{
    const DevModel &m = *mp;
    extern __shared__ double smem[];
    typedef SweepLds<G, P, PAD, ZC> Lds;
    constexpr int GPB = WalkBlock<G>::N / G;
    constexpr int SLOTS = Lds::SLOTS;
    static_assert(Lds::TABLES >= GroupLds<G, P, ZC>::DOUBLES,
                  "eval_walker is the fallback on the same LDS region");
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    double *lds = smem + (size_t)grp * Lds::DOUBLES;
    double *tab = lds + Lds::TABLES, *ntab = tab + 4 * SLOTS;
    double *zl = ntab + 4 * SLOTS, *nz = zl + SLOTS, *dlf = nz + SLOTS,
           *lu = dlf + SLOTS;
    const long long w = walker_of_block<GPB>(blockIdx.x, grp);
    const bool active = w < a.W;
    if (GPB == 1 && !active) return;      // (no one else in the workgroup)
    const long long wr = active ? w : 0;
    const int n = walker_n<G, P, PAD>(m);
    const unsigned int slot = a.chain0 + (unsigned int)wr;
    const bool pairs = !m.is_ideal, onebody = !m.is_free;

    double wf_cur = a.rec[wr].wf, e_cur = a.rec[wr].ecarry;
    double se = 0.0, se2 = 0.0;
    long long na = 0;
    if (!a.reset_sums) {
        se = a.rec[wr].sum_e; se2 = a.rec[wr].sum_e2; na = a.rec[wr].n_acc;
    }

    // the row in slot order (registers) and by label (LDS)
    double z[P];
    int lab[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = lane_particle<G, P, PAD>(m, gl, p);
        z[p] = (i < n) ? a.pos[wr * n + i] : 0.0;
        lab[p] = (i < n) ? (int)a.label[wr * n + i] : i;
        if (i < n) zl[lab[p]] = z[p];
    }
    sweep_sync();
    // this lane's labels: P gl .. P gl + cnt - 1
    const int k0 = P * gl;
    const int cnt = max(0, min(P, n - k0));
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int k = k0 + p;
        const double zk = wrap_box(zl[min(k, n - 1)], m.L);
        PTab t;
        sincos_halfpi(zk * m.two_over_L, t.s, t.c);
        sincos_halfpi(zk * m.k2_2pi, t.su, t.cu);
        if (k < n) {
            tab[4 * k] = t.s; tab[4 * k + 1] = t.c;
            tab[4 * k + 2] = t.su; tab[4 * k + 3] = t.cu;
        }
    }
    sweep_sync();

    const unsigned int nyield = a.nsteps;
    for (unsigned int y = 0; y < nyield; ++y) {
        const bool forced = a.forced != 0 && y == 0;
        const unsigned int step =
            a.step + y - (a.forced != 0 && y > 0 ? 1u : 0u);
        int nacc = 0;
        if (!forced) {
            // ---- every particle's proposal, all at once
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int k = k0 + p;
                const int kc = min(k, n - 1);
                const double zk = zl[kc];
                uint32_t w0, w1;
                vmc_move_block(a.seed, slot, step, (unsigned)kc, w0, w1);
                double zs;
                {
                    // (the sum of the ROUNDED product, as defined)
#pragma clang fp contract(off)
                    zs = zk + vmc_move_unit(w0) * a.move_spread;
                }
                const double zp = wrap_box(zs, m.L);
                PTab t;
                sincos_halfpi(zp * m.two_over_L, t.s, t.c);
                sincos_halfpi(zp * m.k2_2pi, t.su, t.cu);
                const double dl =
                    onebody ? obdm_log_f1(m, zp) - obdm_log_f1(m, zk) : 0.0;
                // (w1 + 1/2) 2^-32 in (0, 1), exact
                const double lgu = log_pos(fma((double)w1, 0x1p-32, 0x1p-33));
                if (k < n) {
                    ntab[4 * k] = t.s; ntab[4 * k + 1] = t.c;
                    ntab[4 * k + 2] = t.su; ntab[4 * k + 3] = t.cu;
                    nz[k] = zp; dlf[k] = dl; lu[k] = lgu;
                }
            }
            sweep_sync();
            // ---- the moves, one after the other
            for (int k = 0; k < n; ++k) {
                PTab own[2];
                own[0].s = ntab[4 * k]; own[0].c = ntab[4 * k + 1];
                own[0].su = ntab[4 * k + 2]; own[0].cu = ntab[4 * k + 3];
                own[1].s = tab[4 * k]; own[1].c = tab[4 * k + 1];
                own[1].su = tab[4 * k + 2]; own[1].cu = tab[4 * k + 3];
                const double zp = nz[k], dl = dlf[k], lgu = lu[k];
                const int self[2] = { k - k0, k - k0 };
                // (the lanes add their partners' logarithms in different
                // orders: the group takes its first lane's sum)
                double x = 0.0;
                if (pairs) {
                    ObdmRow r[2];
                    obdm_rows<2>(m, tab + 4 * k0, cnt, own, self, r);
                    x = sweep_first<G>(group_sum<G>(sweep_lane_log(m, r)), gl);
                }
                const double delta = x + dl;
                const bool acc = lgu < 2.0 * delta;
                // (every lane of the group is past its reads of entry k)
                sweep_sync();
                if (acc) {
                    if (gl == 0) {
                        tab[4 * k] = own[0].s; tab[4 * k + 1] = own[0].c;
                        tab[4 * k + 2] = own[0].su; tab[4 * k + 3] = own[0].cu;
                        zl[k] = zp;
                    }
                    ++nacc;
                }
                sweep_sync();
            }
        }
        // ---- log|psi| and energy of the resulting row, in full
        const bool changed = forced || nacc > 0;
        if (__ballot(changed) != 0ull) {
            double zt[P];
            int labt[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int i = lane_particle<G, P, PAD>(m, gl, p);
                labt[p] = lab[p];
                zt[p] = (i < n) ? zl[lab[p]] : 0.0;
            }
            double wf_new, e_new;
            sweep_eval<G, P, PAD, ZC>(m, zt, labt, gl, n, active, lds, zl, nz,
                                      dlf, wf_new, e_new);
            // (a group that accepted nothing keeps its row and its values: a
            // chain does not depend on its neighbours in the wavefront)
            if (changed) {
#pragma unroll
                for (int p = 0; p < P; ++p) { z[p] = zt[p]; lab[p] = labt[p]; }
                wf_cur = wf_new;
                e_cur = e_new;
            }
        }
        na += forced ? (long long)n : (long long)nacc;
        se = se + e_cur;
        se2 = fma(e_cur, e_cur, se2);
        if (active) {
            const long long row = (a.y + (long long)y) * a.W + w;
            if (gl == 0) {
                if (a.ser_wf) a.ser_wf[row] = wf_cur;
                if (a.ser_e) a.ser_e[row] = e_cur;
                if (a.ser_stat) a.ser_stat[row] = changed ? 1 : 0;
            }
            if (a.ser_pos) {
                // series in the original particle order
                for (int p = 0; p < cnt; ++p)
                    a.ser_pos[row * n + k0 + p] = zl[k0 + p];
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = lane_particle<G, P, PAD>(m, gl, p);
        if (i < n) {
            a.pos[w * n + i] = z[p];
            a.label[w * n + i] = (unsigned short)lab[p];
        }
    }
    if (gl == 0) {
        VmcRec *r = a.rec + w;
        r->wf = wf_cur;
        r->ecarry = e_cur;
        r->sum_e = se;
        r->sum_e2 = se2;
        r->n_acc = na;
    }
}

// the instantiations: one translation unit (inst_SWEEP.hip); qmcwalk.hip sees
// them as `extern template` declarations (the shapes and their (PAD, ZC)
// variants follow qmc_inst.h)
#define QMC_INST_SWEEP(KW, G, P, PAD, ZC)                                     \
    KW template __global__ void vmc_sweep_kernel<G, P, PAD, ZC>(              \
        const DevModel *, VmcArgs);
#define QMC_INST_SWEEP_SMALL(KW, G, P)                                        \
    QMC_INST_SWEEP(KW, G, P, false, false)                                    \
    QMC_INST_SWEEP(KW, G, P, false, true)                                     \
    QMC_INST_SWEEP(KW, G, P, true, false) QMC_INST_SWEEP(KW, G, P, true, true)
#define QMC_INST_SWEEP_MASKED(KW, G, P)                                       \
    QMC_INST_SWEEP(KW, G, P, true, false) QMC_INST_SWEEP(KW, G, P, true, true)
#define QMC_TU_SWEEP(KW)                                                      \
    QMC_INST_SWEEP_SMALL(KW, 16, 1) QMC_INST_SWEEP_SMALL(KW, 16, 2)           \
    QMC_INST_SWEEP_SMALL(KW, 32, 2) QMC_INST_SWEEP_SMALL(KW, 64, 1)           \
    QMC_INST_SWEEP_SMALL(KW, 64, 2) QMC_INST_SWEEP_MASKED(KW, 64, 4)          \
    QMC_INST_SWEEP_MASKED(KW, 64, 8)
