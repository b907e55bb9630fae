// qmc_walker_record.h -- the walker records of the population rebalance
// (qmc_dmc_export_walkers / qmc_dmc_import_walkers_at): the segment table and
// the kernels that pack walkers into records and unpack them.  Needs nothing
// but the HIP runtime (tools/record_bench.hip times the pair on its own).
#pragma once

#include <hip/hip_runtime.h>

// Walker record of the population rebalance, a vector of doubles: pos[N],
// drift[N], label[N] (as doubles), energy, log-weight, then one segment per
// estimator slot whose per-walker rows travel (S(k) parts [M][3] and density
// [B] always; the rows of the other slots when the ensemble carries them:
// qmc_dmc_set_record_rows).  The host lists the segments in record order.
struct RecSeg {
    void *base;                     // [maxw][width] rows of the population
    int width;                      // doubles per walker
    int kind;                       // REC_F64, or REC_U16 <-> double
};
enum { REC_F64, REC_U16 };
constexpr int REC_BASE_SEGS = 5;    // pos, drift, label, energy, log-weight
constexpr int REC_MAX_SEGS = 12;    // the base and one per estimator slot
constexpr int REC_WAVES = 4;        // wavefronts (records in flight) per block

struct WalkerRecArgs {
    RecSeg seg[REC_MAX_SEGS];
    int nseg;
    int rec;                        // doubles per record: the widths summed
    int e_off;                      // where the energy sits in a record
    double *eslot;                  // slot energies
    long long first, count;
};

// One wavefront per record, grid-striding over the records; the lanes stride
// over each segment, so a row and its part of the record move in whole
// 512-byte lines.  The segment table is wave-uniform (scalar loads from the
// kernel arguments): no per-element index arithmetic beyond an add.
__global__ void __launch_bounds__(64 * REC_WAVES)
pack_walkers_kernel(WalkerRecArgs a, double *__restrict__ buf)
{
    const int lane = threadIdx.x & 63;
    const long long wstride = (long long)gridDim.x * REC_WAVES;
    for (long long s = (long long)blockIdx.x * REC_WAVES + (threadIdx.x >> 6);
         s < a.count; s += wstride) {
        const size_t src = (size_t)(a.first + s);
        double *rec = buf + (size_t)s * a.rec;
        for (int k = 0; k < a.nseg; ++k) {
            const int w = a.seg[k].width;
            if (a.seg[k].kind == REC_U16) {
                const unsigned short *row =
                    (const unsigned short *)a.seg[k].base + src * w;
                for (int j = lane; j < w; j += 64) rec[j] = (double)row[j];
            } else {
                const double *row = (const double *)a.seg[k].base + src * w;
                for (int j = lane; j < w; j += 64) rec[j] = row[j];
            }
            rec += w;
        }
    }
}

__global__ void __launch_bounds__(64 * REC_WAVES)
unpack_walkers_kernel(WalkerRecArgs a, const double *__restrict__ buf)
{
    const int lane = threadIdx.x & 63;
    const long long wstride = (long long)gridDim.x * REC_WAVES;
    for (long long s = (long long)blockIdx.x * REC_WAVES + (threadIdx.x >> 6);
         s < a.count; s += wstride) {
        const size_t dst = (size_t)(a.first + s);
        const double *rec = buf + (size_t)s * a.rec;
        // the slot's previous occupant is gone: its "stale" energy (the
        // reference's quirk D1 reads it) becomes the newcomer's own
        if (lane == 0) a.eslot[dst] = rec[a.e_off];
        for (int k = 0; k < a.nseg; ++k) {
            const int w = a.seg[k].width;
            if (a.seg[k].kind == REC_U16) {
                unsigned short *row = (unsigned short *)a.seg[k].base + dst * w;
                for (int j = lane; j < w; j += 64)
                    row[j] = (unsigned short)rec[j];
            } else {
                double *row = (double *)a.seg[k].base + dst * w;
                for (int j = lane; j < w; j += 64) row[j] = rec[j];
            }
            rec += w;
        }
    }
}
