// record_bench.hip -- cost of moving walker records: export + import of W
// records (pack_walkers_kernel + unpack_walkers_kernel of
// csrc/qmc_walker_record.h) against the pair they replaced, in one process.
// Development tool; the table is profiles/record_bench.txt.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/record_bench \
//       tools/record_bench.hip && tools/record_bench [W [N [rounds [reps]]]]
//
// Layouts at N particles: (a) the base record, 3 N + 2 doubles; (b) with the
// rows of S(k), 64 modes, and of the density, 64 bins; (c) with the rows of
// F(k, tau), 16 modes x (62 + 2), as well.  The replaced pair (`*_v0` below,
// kept here as it was: one thread per double, a 64-bit division and an `if`
// chain per element) knows (a) and (b) only.
//
// Every round times `reps` export + import pairs of each variant between two
// events on one stream, the variants taking turns within a round; the figure
// of a variant is the median over the rounds, its spread their minimum and
// maximum.  Before any timing the new pack must give the records of the old
// one bit for bit, and an export -> wipe -> import round trip must restore
// every array.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../phd_qmclib_amd/csrc/qmc_walker_record.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) {            \
    printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// ---- the replaced pair ------------------------------------------------------
struct WalkerRecArgsV0 {
    double *pos, *drift;
    unsigned short *label;
    double *energy, *weight;
    double *eslot;
    double *ssf_aux, *dens_aux;
    long long first, count;
    int n, m3, nb;
};

__device__ __forceinline__ int walker_rec_size_v0(const WalkerRecArgsV0 &a)
{
    return 3 * a.n + 2 + a.m3 + a.nb;
}

__global__ void pack_walkers_kernel_v0(WalkerRecArgsV0 a, double *buf)
{
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rec = walker_rec_size_v0(a), n = a.n;
    if (idx >= a.count * rec) return;
    long long s = idx / rec;
    int j = (int)(idx % rec);
    long long src = a.first + s;
    double v;
    if (j < n) v = a.pos[src * n + j];
    else if (j < 2 * n) v = a.drift[src * n + (j - n)];
    else if (j < 3 * n) v = (double)a.label[src * n + (j - 2 * n)];
    else if (j == 3 * n) v = a.energy[src];
    else if (j == 3 * n + 1) v = a.weight[src];
    else if (j < 3 * n + 2 + a.m3) v = a.ssf_aux[src * a.m3 + (j - 3 * n - 2)];
    else v = a.dens_aux[src * a.nb + (j - 3 * n - 2 - a.m3)];
    buf[idx] = v;
}

__global__ void unpack_walkers_kernel_v0(WalkerRecArgsV0 a, const double *buf)
{
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rec = walker_rec_size_v0(a), n = a.n;
    if (idx >= a.count * rec) return;
    long long s = idx / rec;
    int j = (int)(idx % rec);
    long long dst = a.first + s;
    double v = buf[idx];
    if (j < n) a.pos[dst * n + j] = v;
    else if (j < 2 * n) a.drift[dst * n + (j - n)] = v;
    else if (j < 3 * n) a.label[dst * n + (j - 2 * n)] = (unsigned short)v;
    else if (j == 3 * n) {
        a.energy[dst] = v;
        a.eslot[dst] = v;
    }
    else if (j == 3 * n + 1) a.weight[dst] = v;
    else if (j < 3 * n + 2 + a.m3) a.ssf_aux[dst * a.m3 + (j - 3 * n - 2)] = v;
    else a.dens_aux[dst * a.nb + (j - 3 * n - 2 - a.m3)] = v;
}

// ---- the population ---------------------------------------------------------
struct Arrays {
    long long W;
    int n, m3, nb, isf;
    double *pos, *drift, *energy, *weight, *eslot, *ssf, *dens, *frow, *buf;
    unsigned short *label;
};

static double *dev_doubles(size_t count, unsigned seed)
{
    std::vector<double> h(count);
    unsigned long long x = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (double &v : h) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.25;
    }
    double *d;
    CHECK(hipMalloc(&d, count * 8));
    CHECK(hipMemcpy(d, h.data(), count * 8, hipMemcpyHostToDevice));
    return d;
}

static std::vector<double> host_of(const double *d, size_t count)
{
    std::vector<double> h(count);
    CHECK(hipMemcpy(h.data(), d, count * 8, hipMemcpyDeviceToHost));
    return h;
}

static WalkerRecArgs args_new(const Arrays &p, int layout)
{
    WalkerRecArgs a;
    int k = 0, rec = 0;
    auto add = [&](void *base, int width, int kind) {
        a.seg[k].base = base; a.seg[k].width = width; a.seg[k].kind = kind;
        rec += width;
        ++k;
    };
    add(p.pos, p.n, REC_F64);
    add(p.drift, p.n, REC_F64);
    add(p.label, p.n, REC_U16);
    a.e_off = rec;
    add(p.energy, 1, REC_F64);
    add(p.weight, 1, REC_F64);
    if (layout >= 1) { add(p.ssf, p.m3, REC_F64); add(p.dens, p.nb, REC_F64); }
    if (layout >= 2) add(p.frow, p.isf, REC_F64);
    for (int j = k; j < REC_MAX_SEGS; ++j) a.seg[j] = RecSeg{ nullptr, 0, 0 };
    a.nseg = k; a.rec = rec;
    a.eslot = p.eslot;
    a.first = 0; a.count = p.W;
    return a;
}

static WalkerRecArgsV0 args_v0(const Arrays &p, int layout)
{
    WalkerRecArgsV0 a;
    a.pos = p.pos; a.drift = p.drift; a.label = p.label;
    a.energy = p.energy; a.weight = p.weight; a.eslot = p.eslot;
    a.ssf_aux = layout ? p.ssf : nullptr;
    a.dens_aux = layout ? p.dens : nullptr;
    a.first = 0; a.count = p.W;
    a.n = p.n; a.m3 = layout ? p.m3 : 0; a.nb = layout ? p.nb : 0;
    return a;
}

static void pair_new(const Arrays &p, const WalkerRecArgs &a, hipStream_t st)
{
    // (the launch shape of qmcwalk.hip: walker_rec_blocks)
    const unsigned blocks = (unsigned)std::min<long long>(
        (p.W + REC_WAVES - 1) / REC_WAVES, 4096);
    hipLaunchKernelGGL(pack_walkers_kernel, dim3(blocks), dim3(64 * REC_WAVES),
                       0, st, a, p.buf);
    hipLaunchKernelGGL(unpack_walkers_kernel, dim3(blocks),
                       dim3(64 * REC_WAVES), 0, st, a, p.buf);
}

static void pair_v0(const Arrays &p, const WalkerRecArgsV0 &a, hipStream_t st)
{
    const long long tot = p.W * (long long)(3 * a.n + 2 + a.m3 + a.nb);
    const unsigned blocks = (unsigned)((tot + 255) / 256);
    hipLaunchKernelGGL(pack_walkers_kernel_v0, dim3(blocks), dim3(256), 0, st,
                       a, p.buf);
    hipLaunchKernelGGL(unpack_walkers_kernel_v0, dim3(blocks), dim3(256), 0,
                       st, a, p.buf);
}

static bool same(const std::vector<double> &x, const std::vector<double> &y)
{
    return x.size() == y.size() &&
           memcmp(x.data(), y.data(), x.size() * 8) == 0;
}

int main(int argc, char **argv)
{
    Arrays p;
    p.W = argc > 1 ? atoll(argv[1]) : 1 << 14;
    p.n = argc > 2 ? atoi(argv[2]) : 64;
    const int rounds = argc > 3 ? atoi(argv[3]) : 21;
    const int reps = argc > 4 ? atoi(argv[4]) : 200;
    p.m3 = 3 * 64; p.nb = 64; p.isf = 16 * (62 + 2);
    const size_t W = (size_t)p.W, n = (size_t)p.n;
    const size_t rec_max = 3 * n + 2 + p.m3 + p.nb + p.isf;
    p.pos = dev_doubles(W * n, 1); p.drift = dev_doubles(W * n, 2);
    p.energy = dev_doubles(W, 3); p.weight = dev_doubles(W, 4);
    p.eslot = dev_doubles(W, 5); p.ssf = dev_doubles(W * p.m3, 6);
    p.dens = dev_doubles(W * p.nb, 7); p.frow = dev_doubles(W * p.isf, 8);
    p.buf = dev_doubles(W * rec_max, 9);
    {
        std::vector<unsigned short> h(W * n);
        for (size_t i = 0; i < h.size(); ++i)
            h[i] = (unsigned short)((i * 7 + i / n) % n);
        CHECK(hipMalloc(&p.label, h.size() * 2));
        CHECK(hipMemcpy(p.label, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));

    // ---- the same records, and a round trip that restores the arrays ------
    for (int layout = 0; layout < 3; ++layout) {
        const WalkerRecArgs a = args_new(p, layout);
        const size_t tot = W * (size_t)a.rec;
        if (layout < 2) {
            const WalkerRecArgsV0 b = args_v0(p, layout);
            CHECK(hipMemset(p.buf, 0xff, tot * 8));
            hipLaunchKernelGGL(pack_walkers_kernel_v0,
                               dim3((unsigned)((tot + 255) / 256)), dim3(256),
                               0, st, b, p.buf);
            CHECK(hipStreamSynchronize(st));
            const std::vector<double> old_rec = host_of(p.buf, tot);
            CHECK(hipMemset(p.buf, 0xff, tot * 8));
            pair_new(p, a, st);
            CHECK(hipStreamSynchronize(st));
            if (!same(old_rec, host_of(p.buf, tot))) {
                printf("layout %c: the records differ from the old pack's\n",
                       'a' + layout);
                return 1;
            }
        }
        const std::vector<double> pos = host_of(p.pos, W * n),
            ssf = host_of(p.ssf, W * p.m3), fr = host_of(p.frow, W * p.isf),
            en = host_of(p.energy, W);
        std::vector<unsigned short> lab(W * n), lab2(W * n);
        CHECK(hipMemcpy(lab.data(), p.label, lab.size() * 2,
                        hipMemcpyDeviceToHost));
        const unsigned blocks = (unsigned)std::min<long long>(
            (p.W + REC_WAVES - 1) / REC_WAVES, 4096);
        hipLaunchKernelGGL(pack_walkers_kernel, dim3(blocks),
                           dim3(64 * REC_WAVES), 0, st, a, p.buf);
        CHECK(hipMemsetAsync(p.pos, 0, W * n * 8, st));
        CHECK(hipMemsetAsync(p.label, 0, W * n * 2, st));
        CHECK(hipMemsetAsync(p.energy, 0, W * 8, st));
        if (layout >= 1) CHECK(hipMemsetAsync(p.ssf, 0, W * p.m3 * 8, st));
        if (layout >= 2) CHECK(hipMemsetAsync(p.frow, 0, W * p.isf * 8, st));
        hipLaunchKernelGGL(unpack_walkers_kernel, dim3(blocks),
                           dim3(64 * REC_WAVES), 0, st, a, p.buf);
        CHECK(hipStreamSynchronize(st));
        CHECK(hipMemcpy(lab2.data(), p.label, lab2.size() * 2,
                        hipMemcpyDeviceToHost));
        if (!same(pos, host_of(p.pos, W * n)) || lab != lab2 ||
            !same(ssf, host_of(p.ssf, W * p.m3)) ||
            !same(fr, host_of(p.frow, W * p.isf)) ||
            !same(en, host_of(p.energy, W)) ||
            !same(en, host_of(p.eslot, W))) {
            printf("layout %c: the round trip does not restore the arrays\n",
                   'a' + layout);
            return 1;
        }
    }
    CHECK(hipGetLastError());

    // ---- timing -----------------------------------------------------------
    printf("export + import of %lld walker records at N = %d; %d rounds of "
           "%d pairs per variant, variants alternating\n", p.W, p.n, rounds,
           reps);
    printf("%-50s %8s %10s %10s %10s %9s\n", "layout / kernels", "doubles",
           "median us", "min us", "max us", "GB/s");
    const char *names[3] = { "(a) base record",
                             "(b) + S(k) 64 modes, density 64 bins",
                             "(c) + F(k, tau) 16 x 64" };
    for (int layout = 0; layout < 3; ++layout) {
        const WalkerRecArgs a = args_new(p, layout);
        const WalkerRecArgsV0 b = args_v0(p, layout < 2 ? layout : 1);
        const int variants = layout < 2 ? 2 : 1;
        std::vector<float> us[2];
        for (int r = -2; r < rounds; ++r)           // two warm-up rounds
            for (int v = 0; v < variants; ++v) {
                CHECK(hipEventRecord(e0, st));
                for (int i = 0; i < reps; ++i) {
                    if (v == 0) pair_new(p, a, st);
                    else pair_v0(p, b, st);
                }
                CHECK(hipEventRecord(e1, st));
                CHECK(hipEventSynchronize(e1));
                float ms = 0.f;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 0) us[v].push_back(ms * 1e3f / reps);
            }
        CHECK(hipGetLastError());
        for (int v = 0; v < variants; ++v) {
            std::sort(us[v].begin(), us[v].end());
            const float med = us[v][us[v].size() / 2];
            // a pair reads and writes every double of the records twice
            // (arrays -> records -> arrays)
            const double bytes = 4.0 * 8.0 * (double)p.W * a.rec;
            char label[96];
            snprintf(label, sizeof label, "%s, %s", names[layout],
                     v == 0 ? "new" : "replaced");
            printf("%-50s %8d %10.2f %10.2f %10.2f %9.0f\n", label, a.rec,
                   med, us[v].front(), us[v].back(), bytes / med * 1e-3);
        }
    }
    return 0;
}
