// devunit_shrink.hip — TEST-ONLY device build of the apeGLM objective (never linked into the package).
//
// dsq_shrink.h's shrink_fn and shrink_fn_wide are header templates and are called here from two small kernels at
// caller-given coefficients: one gene per wavefront and four per 256-thread block as k_shrink launches the register
// widths, one gene per 64-thread block as k_shrink_wide launches the run-time-p ones.  Every gene has its own counts,
// offsets, design, size, prior scales and shrink index, so one launch probes many corners of the objective.  Each kernel
// evaluates twice - the loss alone (g == nullptr, the grid search's and the scaling constant's call) and the loss with its
// gradient - and returns what EVERY lane holds.  No function body of the product is restated here.
#include <hip/hip_runtime.h>

#include "devunit_host.h"
#include "dsq_dispatch.h"
#include "dsq_launch.h"
#include "dsq_shrink.h"

using namespace dsq;
using devunit::Bufs;

namespace {

struct FnArgs {
    const int32_t* y;      // [G][ldx]
    const double* offset;  // [G][ldx]
    const double* Xt;      // [G][rows][ldx], rows = P (register widths) or PB (run-time p)
    int ldx, N, G;
    const double *size, *sigma0, *sigma;  // [G]
    const int32_t* sidx;                  // [G]
    const double* b;                      // [G][rows]
};

__device__ ShrinkArgs gene_args(const FnArgs& a, int gk, int rows) {
    ShrinkArgs A;
    A.y = a.y + (size_t)gk * a.ldx;
    A.offset = a.offset + (size_t)gk * a.ldx;
    A.Xt = a.Xt + (size_t)gk * rows * a.ldx;
    A.ldx = a.ldx; A.N = a.N;
    A.size = a.size[gk]; A.sigma0 = a.sigma0[gk]; A.sigma = a.sigma[gk]; A.shrink_index = a.sidx[gk];
    return A;
}

// f0 / f1: [G][64] (loss-only call, call with a gradient), g: [G][64][P]
template <int P>
__global__ void __launch_bounds__(kBlock) k_fn(FnArgs a, double* __restrict__ f0, double* __restrict__ f1,
                                               double* __restrict__ g) {
    const int lane = threadIdx.x & 63;
    const int gk = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (gk >= a.G) return;
    const ShrinkArgs A = gene_args(a, gk, P);
    double bb[P], gg[P];
#pragma unroll
    for (int j = 0; j < P; ++j) bb[j] = a.b[(size_t)gk * P + j];
    const size_t o = (size_t)gk * 64 + lane;
    f0[o] = shrink_fn<DeviceWave, P>(A, bb, nullptr);
    f1[o] = shrink_fn<DeviceWave, P>(A, bb, gg);
#pragma unroll
    for (int j = 0; j < P; ++j) g[o * P + j] = gg[j];
}

// the same for a run-time p <= PB; g: [G][64][PB], read before the call and written back whole, so that an entry the
// template leaves alone keeps what the caller put there
template <int PMAX, int PB>
__global__ void __launch_bounds__(64) k_fn_wide(FnArgs a, int p, double* __restrict__ f0, double* __restrict__ f1,
                                                double* __restrict__ g) {
    const int lane = threadIdx.x, gk = blockIdx.x;
    if (gk >= a.G) return;
    const ShrinkArgs A = gene_args(a, gk, PB);
    const double* xb = a.b + (size_t)gk * PB;
    const size_t o = (size_t)gk * 64 + lane;
    double gg[PB];
#pragma unroll
    for (int j = 0; j < PB; ++j) gg[j] = g[o * PB + j];
    f0[o] = shrink_fn_wide<DeviceWave, PMAX, PB>(A, p, xb, nullptr);
    f1[o] = shrink_fn_wide<DeviceWave, PMAX, PB>(A, p, xb, gg);
#pragma unroll
    for (int j = 0; j < PB; ++j) g[o * PB + j] = gg[j];
}

// rows: the rows of Xt and the entries of b and g per gene; p: the coefficients in use
int fn_run(int PMAX, int PB, int p, bool wide, const int32_t* y, const double* offset, const double* Xt, int ldx, int N,
           int G, const double* size, const double* sigma0, const double* sigma, const int32_t* sidx, const double* b,
           double* f0, double* f1, double* g) {
    const int rows = PB;
    if (N < 1 || G < 1 || ldx < N || p < 1 || p > rows) return (int)hipErrorInvalidValue;
    if (!y || !offset || !Xt || !size || !sigma0 || !sigma || !sidx || !b || !f0 || !f1 || !g)
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < G; ++k)
        if (sidx[k] < 0 || sidx[k] >= p) return (int)hipErrorInvalidValue;
    Bufs B;
    FnArgs a;
    a.y = B.put(y, (size_t)G * ldx);
    a.offset = B.put(offset, (size_t)G * ldx);
    a.Xt = B.put(Xt, (size_t)G * rows * ldx);
    a.ldx = ldx; a.N = N; a.G = G;
    a.size = B.put(size, G);
    a.sigma0 = B.put(sigma0, G);
    a.sigma = B.put(sigma, G);
    a.sidx = B.put(sidx, G);
    a.b = B.put(b, (size_t)G * rows);
    double* d0 = B.put(f0, (size_t)G * 64);
    double* d1 = B.put(f1, (size_t)G * 64);
    double* dg = B.put(g, (size_t)G * 64 * rows);
    if (B.e != hipSuccess) return (int)B.e;
    bool found = false;
    if (!wide) {
        DSQ_DISPATCH_P(p, hipLaunchKernelGGL((k_fn<P>), dim3(genes_to_blocks(G)), dim3(kBlock), 0, 0, a, d0, d1, dg);
                       found = true)
    } else {
#define DU_WIDE(M_, B_)                                                                                  \
    if (!found && PMAX == M_ && PB == B_) {                                                              \
        hipLaunchKernelGGL((k_fn_wide<M_, B_>), dim3(G), dim3(64), 0, 0, a, p, d0, d1, dg);              \
        found = true;                                                                                    \
    }
        DU_WIDE(16, 16) DU_WIDE(32, 24) DU_WIDE(32, 32) DU_WIDE(48, 40) DU_WIDE(48, 48)
#undef DU_WIDE
    }
    if (!found) return (int)hipErrorInvalidValue;
    B.done();
    B.get(f0, d0, (size_t)G * 64);
    B.get(f1, d1, (size_t)G * 64);
    B.get(g, dg, (size_t)G * 64 * rows);
    return (int)B.e;
}

}  // namespace

extern "C" {

// shrink_fn<DeviceWave, P>, P = 1 ... 12.  y / offset: [G][ldx], Xt: [G][P][ldx], size / sigma0 / sigma / sidx: [G],
// b: [G][P] -> f0 / f1: [G][64], g: [G][64][P]
int du_shrink_fn(int P, const int32_t* y, const double* offset, const double* Xt, int ldx, int N, int G,
                 const double* size, const double* sigma0, const double* sigma, const int32_t* sidx, const double* b,
                 double* f0, double* f1, double* g) {
    if (P < 1 || P > DSQ_REG_MAX_P) return (int)hipErrorInvalidValue;
    return fn_run(P, P, P, false, y, offset, Xt, ldx, N, G, size, sigma0, sigma, sidx, b, f0, f1, g);
}

// shrink_fn_wide<DeviceWave, PMAX, PB> at a run-time p <= PB, the launcher's five (PMAX, PB).  Xt: [G][PB][ldx],
// b: [G][PB], g: [G][64][PB] - full PB rows and entries whatever p is
int du_shrink_fn_wide(int PMAX, int PB, int p, const int32_t* y, const double* offset, const double* Xt, int ldx, int N,
                      int G, const double* size, const double* sigma0, const double* sigma, const int32_t* sidx,
                      const double* b, double* f0, double* f1, double* g) {
    return fn_run(PMAX, PB, p, true, y, offset, Xt, ldx, N, G, size, sigma0, sigma, sidx, b, f0, f1, g);
}

}  // extern "C"
