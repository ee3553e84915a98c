// devunit_trend.hip — TEST-ONLY device build around the trend fit (never linked into the package).
//
// The product's trend unit (dsq_k_trend.hip) is linked into the test library unchanged and driven through its launchers
// (dsq_launch.h): launch_trend_fit with its memset, cooperative launch and crossover, launch_trend_glm,
// launch_trend_loss_grad.  The passes themselves - register genes, mailbox, the workgroups' exchange - are header code
// (dsq_trend_grid.h): k_probe instantiates trend_grid_run with a driver that runs single passes at given points and has
// EVERY workgroup's leader write its own copy of what it saw.  No function body of the product is restated here.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "devunit_host.h"
#include "dsq_launch.h"
#include "dsq_trend_grid.h"

using namespace dsq;
using devunit::Bufs;

namespace {

constexpr int kProbeRec = 32;     // doubles per (workgroup, point)
constexpr int kProbeMaxPoints = 8;

// Per point: init_keep, eval, filter, eval through the ops' own entry points, and after each of the three kinds of pass
// the same pass once more through ops.pass, which hands out the six totals.  Record:
//   [0..5] totals of the load pass   [6] init_keep()          [7..9] eval: f, g0, g1     [10..15] totals of that eval
//   [16] filter()                    [17..22] totals of a second filter pass (idempotent: it keeps what the first kept)
//   [23..25] eval after the filter   [26..31] its totals
// The driver reads only kernel arguments and the points: it is the same in every workgroup, and it never waits itself.
__global__ __launch_bounds__(64 * kTrendWaves) void k_probe(const double* __restrict__ disp,
                                                            const double* __restrict__ means, int n, double min_disp,
                                                            double max_disp, uint8_t* __restrict__ keep, TrendGridMem* Gm,
                                                            const double* __restrict__ pts, int npts,
                                                            double* __restrict__ out) {
    __shared__ TrendShared S;
    trend_grid_run(TrendData{disp, means, keep, n, min_disp, max_disp, 0}, Gm, S, [&](GridTrendOps& ops) {
        for (int p = 0; p < npts; ++p) {
            const double a0 = pts[2 * p], a1 = pts[2 * p + 1];
            double rec[kProbeRec];
            double tot[6], f, g[2];
            rec[6] = (double)ops.init_keep();
            ops.pass(3, 0.0, 0.0, tot);
            for (int q = 0; q < 6; ++q) rec[q] = tot[q];
            ops.eval(a0, a1, f, g);
            rec[7] = f; rec[8] = g[0]; rec[9] = g[1];
            ops.pass(1, a0, a1, tot);
            for (int q = 0; q < 6; ++q) rec[10 + q] = tot[q];
            rec[16] = (double)ops.filter(a0, a1);
            ops.pass(2, a0, a1, tot);
            for (int q = 0; q < 6; ++q) rec[17 + q] = tot[q];
            ops.eval(a0, a1, f, g);
            rec[23] = f; rec[24] = g[0]; rec[25] = g[1];
            ops.pass(1, a0, a1, tot);
            for (int q = 0; q < 6; ++q) rec[26 + q] = tot[q];
            if (threadIdx.x == 0) {
                double* o = out + ((size_t)blockIdx.x * npts + p) * kProbeRec;
                for (int q = 0; q < kProbeRec; ++q) o[q] = rec[q];
            }
        }
    });
}

}  // namespace

extern "C" {

int du_trend_grid_blocks() { return kTrendGridBlocks; }
int du_trend_threads() { return 64 * kTrendWaves; }
int du_trend_reg_genes() { return kTrendRegGenes; }
int du_trend_probe_rec() { return kProbeRec; }

// k launches of dsq::launch_trend_fit back to back on ONE TrendGridMem, one keep mask and one stream, none of them
// touched in between: case j is disp / means [off[j], off[j + 1]).  out5: [k][5].
int du_trend_fit_seq(const double* disp, const double* means, const int* off, int k, double min_disp, double max_disp,
                     int force_grid, double* out5) {
    if (!disp || !means || !off || !out5 || k < 1 || force_grid < -1 || force_grid > 1) return (int)hipErrorInvalidValue;
    int nmax = 0;
    for (int j = 0; j < k; ++j) {
        if (off[j + 1] <= off[j] || off[j] < 0) return (int)hipErrorInvalidValue;
        nmax = std::max(nmax, off[j + 1] - off[j]);
    }
    Bufs B;
    const double* dd = B.put(disp, (size_t)off[k]);
    const double* dm = B.put(means, (size_t)off[k]);
    double* dout = B.put(out5, (size_t)k * 5);
    uint8_t* keep = B.alloc<uint8_t>((size_t)nmax);
    void* gm = B.alloc<char>(trend_grid_mem_bytes());
    if (B.e != hipSuccess) return (int)B.e;
    B.chk(hipMemset(keep, 0xEE, (size_t)nmax));
    B.chk(hipMemset(gm, 0xEE, trend_grid_mem_bytes()));  // the launcher zeroes it
    for (int j = 0; j < k && B.e == hipSuccess; ++j)
        B.chk(launch_trend_fit(0, dd + off[j], dm + off[j], off[j + 1] - off[j], min_disp, max_disp, keep, dout + 5 * j,
                               gm, force_grid));
    B.done();
    B.get(out5, dout, (size_t)k * 5);
    return (int)B.e;
}

// dsq::launch_trend_glm (the raw one-fit mode), `repeats` launches on one keep mask.  out5: [repeats][5]
int du_trend_glm(const double* targets, const double* cov, int n, int repeats, double* out5) {
    if (!targets || !cov || !out5 || n < 1 || repeats < 1) return (int)hipErrorInvalidValue;
    Bufs B;
    const double* dt = B.put(targets, (size_t)n);
    const double* dc = B.put(cov, (size_t)n);
    double* dout = B.put(out5, (size_t)repeats * 5);
    uint8_t* keep = B.alloc<uint8_t>((size_t)n);
    if (B.e != hipSuccess) return (int)B.e;
    B.chk(hipMemset(keep, 0xEE, (size_t)n));
    for (int j = 0; j < repeats && B.e == hipSuccess; ++j) B.chk(launch_trend_glm(0, dt, dc, n, keep, dout + 5 * j));
    B.done();
    B.get(out5, dout, (size_t)repeats * 5);
    return (int)B.e;
}

// k_probe on `blocks` workgroups (1, or kTrendGridBlocks launched cooperatively as launch_trend_fit does).
// pts: [npts][2], out: [blocks][npts][kProbeRec], *timeout: the grid memory's flag after the launch
int du_trend_probe(int blocks, const double* disp, const double* means, int n, double min_disp, double max_disp,
                   const double* pts, int npts, double* out, unsigned int* timeout) {
    if (!disp || !means || !pts || !out || !timeout || n < 1 || npts < 1 || npts > kProbeMaxPoints ||
        (blocks != 1 && blocks != kTrendGridBlocks))
        return (int)hipErrorInvalidValue;
    Bufs B;
    const double* dd = B.put(disp, (size_t)n);
    const double* dm = B.put(means, (size_t)n);
    const double* dp = B.put(pts, (size_t)npts * 2);
    double* dout = B.put(out, (size_t)blocks * npts * kProbeRec);
    uint8_t* keep = B.alloc<uint8_t>((size_t)n);
    TrendGridMem* gm = B.alloc<TrendGridMem>(1);
    if (B.e != hipSuccess) return (int)B.e;
    B.chk(hipMemset(keep, 0xEE, (size_t)n));
    B.chk(hipMemset(gm, 0, sizeof(TrendGridMem)));
    if (B.e != hipSuccess) return (int)B.e;
    if (blocks == 1) {
        hipLaunchKernelGGL(k_probe, dim3(1), dim3(64 * kTrendWaves), 0, 0, dd, dm, n, min_disp, max_disp, keep, gm, dp,
                           npts, dout);
    } else {
        void* args[] = {(void*)&dd, (void*)&dm, (void*)&n,  (void*)&min_disp, (void*)&max_disp,
                        (void*)&keep, (void*)&gm, (void*)&dp, (void*)&npts,     (void*)&dout};
        B.chk(hipLaunchCooperativeKernel((const void*)k_probe, dim3(blocks), dim3(64 * kTrendWaves), args, 0, 0));
    }
    B.done();
    B.get(out, dout, (size_t)blocks * npts * kProbeRec);
    B.get(timeout, &gm->timeout, 1);
    return (int)B.e;
}

// dsq::launch_trend_loss_grad (k_trend).  keep may be null.  partials: [kTrendPartials][4]
int du_trend_loss_grad(const double* cov, const double* targets, const uint8_t* keep, int n, double a0, double a1,
                       double* partials) {
    if (!cov || !targets || !partials || n < 1) return (int)hipErrorInvalidValue;
    Bufs B;
    const double* dc = B.put(cov, (size_t)n);
    const double* dt = B.put(targets, (size_t)n);
    const uint8_t* dk = B.put(keep, (size_t)n);
    double* dp = B.put(partials, (size_t)kTrendPartials * 4);
    if (B.e != hipSuccess) return (int)B.e;
    B.chk(launch_trend_loss_grad(0, dc, dt, dk, n, a0, a1, dp));
    B.done();
    B.get(partials, dp, (size_t)kTrendPartials * 4);
    return (int)B.e;
}

int du_trend_partials() { return kTrendPartials; }

}  // extern "C"
