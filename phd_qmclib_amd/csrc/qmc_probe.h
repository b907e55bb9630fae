// qmc_probe.h -- diagnostic kernel that runs the production device primitives
// of qmc_math.h / qmc_device.h on caller-given inputs (qmc_engine_probe).
// Only qmcwalk.hip includes it.
//
// Every function id calls the __device__ function itself, with the engine's
// DevModel and its device tables (log, trig, one-body), never a restatement:
// a test of the probe is a test of what the stepping kernels execute.
//
// Layout: in[n][in_width], out[n][out_width] (qmc_probe_width).  Inputs go in
// order, 64 to a wavefront: inputs 64 w ... 64 w + 63 run in wavefront w.
// wrap_box and trig_tab_load decide with a wave-wide __ballot, so which inputs
// share a wavefront is part of what a test sets up.  Lanes past n repeat input
// n - 1 (which lies in their own wavefront) and store nothing, so they never
// change a ballot.
#pragma once
#include "qmc_device.h"
#include "../../include/qmcwalk.h"

// -> input / output doubles per item of function `fn` (0, 0: unknown id)
static inline void qmc_probe_width(int fn, int &nin, int &nout)
{
    nin = nout = 0;
    switch (fn) {
    case QMC_PROBE_FAST_DIV: case QMC_PROBE_PAIR_DIV:
    case QMC_PROBE_PAIR_DIV_F32:            nin = 2; nout = 1; break;
    case QMC_PROBE_FAST_RCP: case QMC_PROBE_FAST_SQRT:
    case QMC_PROBE_EXP_BOUNDED: case QMC_PROBE_LOG_POS:
    case QMC_PROBE_WRAP_BOX: case QMC_PROBE_VMC_MOVE_UNIT:
                                            nin = 1; nout = 1; break;
    case QMC_PROBE_SINCOS_KERNEL: case QMC_PROBE_SINCOS_HALFPI:
                                            nin = 1; nout = 2; break;
    case QMC_PROBE_TRIG_TAB:                nin = 1; nout = 5; break;
    case QMC_PROBE_ONE_BODY_TAB:            nin = 1; nout = 3; break;
    case QMC_PROBE_ONE_BODY:                nin = 1; nout = 4; break;
    case QMC_PROBE_NORMAL2_WORDS: case QMC_PROBE_NORMAL2_UNIFORMS:
                                            nin = 2; nout = 2; break;
    case QMC_PROBE_PHILOX2X32:              nin = 3; nout = 2; break;
    case QMC_PROBE_PHILOX4X32:              nin = 6; nout = 4; break;
    default: break;
    }
}

__global__ void __launch_bounds__(64)
probe_kernel(const DevModel *__restrict__ mp, int fn, long long n,
             const double *__restrict__ in, double *__restrict__ out, int nin,
             int nout)
{
    const DevModel &m = *mp;
    const long long i0 = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long i = i0 < n ? i0 : n - 1;
    const double *x = in + i * nin;
    double y[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    switch (fn) {
    case QMC_PROBE_FAST_DIV: y[0] = fast_div(x[0], x[1]); break;
    case QMC_PROBE_PAIR_DIV: y[0] = pair_div(x[0], x[1]); break;
    case QMC_PROBE_PAIR_DIV_F32:
        y[0] = (double)pair_div((float)x[0], (float)x[1]);
        break;
    case QMC_PROBE_FAST_RCP: y[0] = fast_rcp(x[0]); break;
    case QMC_PROBE_FAST_SQRT: y[0] = fast_sqrt(x[0]); break;
    case QMC_PROBE_SINCOS_KERNEL: sincos_kernel(x[0], y[0], y[1]); break;
    case QMC_PROBE_SINCOS_HALFPI: sincos_halfpi(x[0], y[0], y[1]); break;
    case QMC_PROBE_EXP_BOUNDED: y[0] = exp_bounded(x[0]); break;
    case QMC_PROBE_LOG_POS: y[0] = log_pos(x[0]); break;
    case QMC_PROBE_WRAP_BOX: y[0] = wrap_box(x[0], m.L); break;
    case QMC_PROBE_TRIG_TAB: {
        TrigRow t;
        PTab ta;
        const bool ok = trig_tab_load(m, x[0], t);
        if (ok) {
            trig_tab_finish(m, t, ta);
            y[0] = ta.s; y[1] = ta.c; y[2] = ta.su; y[3] = ta.cu;
        } else {
            y[0] = y[1] = y[2] = y[3] = __builtin_nan("");
        }
        y[4] = ok ? 1.0 : 0.0;
        break;
    }
    case QMC_PROBE_ONE_BODY_TAB: {
        bool barrier;
        one_body_tab<true, true>(m, x[0], y[0], y[1], barrier);
        y[2] = barrier ? 1.0 : 0.0;
        break;
    }
    case QMC_PROBE_ONE_BODY: one_body(m, x[0], y[0], y[1], y[2], y[3]); break;
    case QMC_PROBE_VMC_MOVE_UNIT: y[0] = vmc_move_unit((uint32_t)x[0]); break;
    case QMC_PROBE_NORMAL2_WORDS:
        normal2_from_words((uint32_t)x[0], (uint32_t)x[1], y[0], y[1]);
        break;
    case QMC_PROBE_NORMAL2_UNIFORMS:
        normal2_from_uniforms(x[0], x[1], y[0], y[1]);
        break;
    case QMC_PROBE_PHILOX2X32: {
        uint32_t c0 = (uint32_t)x[0], c1 = (uint32_t)x[1];
        philox2x32_10(c0, c1, (uint32_t)x[2]);
        y[0] = (double)c0; y[1] = (double)c1;
        break;
    }
    case QMC_PROBE_PHILOX4X32: {
        uint32_t c[4] = { (uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2],
                          (uint32_t)x[3] };
        philox4x32_10(c, (uint32_t)x[4], (uint32_t)x[5]);
        for (int k = 0; k < 4; ++k) y[k] = (double)c[k];
        break;
    }
    default: break;
    }
    if (i0 < n) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < nout) out[i0 * nout + k] = y[k];
    }
}
