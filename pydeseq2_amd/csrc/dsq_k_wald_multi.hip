// dsq_k_wald_multi.hip — Wald tests of K contrasts of one fit in one launch (gfx950), designs of up to 12 columns: one
// gene per wavefront.  X^T W X is accumulated once per gene by the loop of k_wald<P> (lane-strided samples, butterfly
// sum: every lane ends up with M), M + ridge is factored once, and the contrasts run lane-parallel: lane l takes the
// contrasts l, l + 64, ... - its own triangular solves, quadratic form and alternative-hypothesis tail - and the 64
// lanes store 64 consecutive results of the gene's row of the [G][K] outputs.  Wider designs: k_wald_multi_wide
// (dsq_k_wide.hip).  A unit of its own so that the twelve instantiations build beside the other units.
#include "dsq_dispatch.h"
#include "dsq_launch.h"
#include "dsq_stats.h"

namespace dsq {

// waves per SIMD asked for (DSQ_WALD_MULTI_WAVES_MID: developer A/B builds, 5 ... 8 columns); from 9 columns on M, its
// factor and a lane's own solve vectors leave room for one
#ifndef DSQ_WALD_MULTI_WAVES_MID
#define DSQ_WALD_MULTI_WAVES_MID 2
#endif
constexpr int wald_multi_min_waves(int p) { return p <= 4 ? 3 : (p <= 8 ? DSQ_WALD_MULTI_WAVES_MID : 1); }

template <int P>
__global__ __launch_bounds__(kBlock, wald_multi_min_waves(P)) void k_wald_multi(
    const double* __restrict__ mu, int ldn, const double* __restrict__ sf, const double* __restrict__ Xt, int ldx, int N,
    int G, const double* __restrict__ disp, const double* __restrict__ beta, const double* __restrict__ ridge,
    const double* __restrict__ contrasts, int K, double lfc_null, int alt, double* __restrict__ pvals,
    double* __restrict__ stats, double* __restrict__ se) {
    const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= G) return;
    double b[P];
#pragma unroll
    for (int j = 0; j < P; ++j) b[j] = beta[(size_t)g * P + j];
    const size_t o = (size_t)g * K;
    wald_gene_multi<DeviceWave, P>(mu ? mu + (size_t)g * ldn : nullptr, sf, Xt, ldx, N, disp[g], b, ridge, contrasts, K,
                                   lfc_null, alt, pvals + o, stats + o, se + o);
}

hipError_t launch_wald_multi(hipStream_t st, const double* mu, int ldn, const double* sf, const double* Xt, int ldx,
                             int N, int G, int P_, const double* disp, const double* beta, const double* d_ridge,
                             const double* d_contrasts, int K, double lfc_null, int alt, double* pvals, double* stats,
                             double* se) {
    if (G <= 0) return hipSuccess;
    if (K < 1 || P_ < 1) return hipErrorInvalidValue;
    if (P_ > DSQ_REG_MAX_P)
        return launch_wide_wald_multi(st, mu, ldn, sf, Xt, ldx, N, G, P_, disp, beta, d_ridge, d_contrasts, K, lfc_null,
                                      alt, pvals, stats, se);
    const dim3 grid(genes_to_blocks(G)), block(kBlock);
    DSQ_DISPATCH_P(P_, hipLaunchKernelGGL(k_wald_multi<P>, grid, block, 0, st, mu, ldn, sf, Xt, ldx, N, G, disp, beta,
                                          d_ridge, d_contrasts, K, lfc_null, alt, pvals, stats, se))
    return hipGetLastError();
}

}  // namespace dsq
