// qmc_obdm_rows.h -- the row arithmetic of the one-body density matrix
// (qmc_obdm.h, which describes it): log f1 at a position as given, the row
// products of shifted own particles against a table of partners in LDS, and
// the logarithm of a row.  A header of its own, without kernels, so that the
// single-particle VMC sweeps (qmc_vmc_sweep.h, a translation unit of their
// own) form their one-particle ratios with the same code.
#pragma once

#include "qmc_device.h"

static constexpr int OBDM_FOLD = 32;    // partners between exponent folds

// log f1 at a position as given
__device__ __forceinline__ double obdm_log_f1(const DevModel &m, double z)
{
    if (m.ob_table) {
        double ldz, lf = 0.0;
        bool barrier;
        one_body_tab<true, false>(m, z, ldz, lf, barrier);
        return lf;
    }
    // The factor of `one_body` (qmc_device.h) without its derivatives, with
    // the two offsets inside the cell written as the fused operations the
    // batch kernel has always been compiled to: left to the compiler, a
    // kernel with a loop around this code gets the products 0.5 z_a, 0.5 z_b
    // hoisted out of it and rounded on their own, and the same configuration
    // would give other bits in obdm_kernel and in dmc_obdm_kernel.
    const double z_cell = z - floor(z);
    double f1, xoff;
    if (m.z_a < z_cell) {
        const double x = m.kp1 * fma(0.5, m.z_b, z_cell - 1.0);
        f1 = 0.5 * (exp_bounded(2.0 * x) + 1.0);
        xoff = x;
    } else {
        double sh, ch;
        sincos_kernel(m.k1_half * fma(-0.5, m.z_a, z_cell), sh, ch);
        f1 = m.cf * ((ch - sh) * (ch + sh));
        xoff = 0.0;
    }
    return log_pos(f1) - xoff;
}

// The own k2-table rotated for a wrapped partner: an own particle in the upper
// half of the box (cos(pi z / L) < 0) meets wrapped partners at D > L/2, whose
// image is d = D - L; one in the lower half at D < -L/2, d = D + L.
__device__ __forceinline__ void obdm_wrap_tab(const DevModel &m, const PTab &a,
                                              double &suw, double &cuw)
{
    const double t = (a.c < 0.0) ? m.sth_signed : -m.sth_signed;
    suw = fma(a.su, m.cth, -(a.cu * t));
    cuw = fma(a.cu, m.cth, a.su * t);
}

struct ObdmRow {
    double PL, PS;     // products of the long / short pair factors (mantissas)
    int eL, eS;        // binary exponents split off them
    int cnt;           // short pairs
};

// Row products of U own particles (tables a[u], excluded partner self[u])
// against the n entries of the configuration's table in LDS.
template <int U>
__device__ __forceinline__ void obdm_rows(const DevModel &m,
                                          const double *__restrict__ tab, int n,
                                          const PTab (&a)[U],
                                          const int (&self)[U],
                                          ObdmRow (&r)[U])
{
    double suw[U], cuw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        obdm_wrap_tab(m, a[u], suw[u], cuw[u]);
        r[u].PL = 1.0; r[u].PS = 1.0; r[u].eL = 0; r[u].eS = 0; r[u].cnt = 0;
    }
    const double sin_rm = m.sin_rm, sphi = m.sphi, cphi = m.cphi;
    for (int j0 = 0; j0 < n; j0 += OBDM_FOLD) {
        const int j1 = min(n, j0 + OBDM_FOLD);
        for (int j = j0; j < j1; ++j) {
            // the partner's entry: the same address in every lane (broadcast)
            const double bs = tab[4 * j], bc = tab[4 * j + 1];
            const double bsu = tab[4 * j + 2], bcu = tab[4 * j + 3];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double S = fma(a[u].s, bc, -(a[u].c * bs));
                const double C = fma(a[u].c, bc, a[u].s * bs);
                const double aS = __builtin_fabs(S);
                const bool live = j != self[u];
                const bool isshort = (aS < sin_rm) & live;
                const bool islong = !(aS < sin_rm) & live;
                const bool wrapped = C < 0.0;
                const double su = wrapped ? suw[u] : a[u].su;
                const double cu = wrapped ? cuw[u] : a[u].cu;
                const double Su = fma(su, bcu, -(cu * bsu));   // sin(k2 d)
                const double Cu = fma(cu, bcu, su * bsu);
                const double Y =
                    __builtin_fabs(fma(__builtin_fabs(Su), sphi, Cu * cphi));
                r[u].PL *= islong ? aS : 1.0;
                r[u].PS *= isshort ? Y : 1.0;
                r[u].cnt += isshort ? 1 : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q_fold(r[u].PL, r[u].eL);
            q_fold(r[u].PS, r[u].eS);
        }
    }
}

// log of a row: beta log PL + log PS + cnt log|a_m| + log f1, the operations
// pinned (explicit fma) so that the shifted and the unshifted row round alike.
__device__ __forceinline__ double obdm_row_log(const DevModel &m,
                                               const ObdmRow &r, double logf1)
{
    const double LN2 = 6.93147180559945309417e-01;
    const double lL = fma((double)r.eL, LN2, log_pos(r.PL));
    const double lS = fma((double)r.eS, LN2, log_pos(r.PS));
    double v = fma(m.beta, lL, lS);
    v = fma((double)r.cnt, m.log_am, v);
    return v + logf1;
}
