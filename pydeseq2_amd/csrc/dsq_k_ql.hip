// dsq_k_ql.hip — quasi-likelihood F-test (gfx950, dsq_ql.h): k_ql_dev, the deviance difference of the two fits and the
// full model's residual deviance of a gene in one sweep over its row - one gene per wavefront, both coefficient vectors
// in wave-private LDS, run-time widths (P_full <= 128, 1 <= P_reduced < P_full) exactly as k_lrt; k_ql_score, F and its
// p-value from the moderated dispersions, one gene per lane; k_f_sf, the F distribution's survival function elementwise.
// Algorithmic HBM traffic of k_ql_dev: 4N bytes of counts per gene, 8 (P_f + P_r) + 8 read and 24 written; the two
// transposed designs and the size factors are shared by every gene and stay in L2.  No atomics, no scratch; the
// lane-strided loop and the butterfly of DeviceWave::sum fix the order of every addition.
// The file makes two objects (Makefile): with -DDSQ_QL_DEV and -ffp-contract=off k_ql_dev, which is held to the bits of
// its host build (dsq_ql.h); without, the two elementwise kernels under the flags of every other unit, so that the
// chi-square branch of k_ql_score is k_chisq_sf's arithmetic.
#include "dsq_launch.h"
#include "dsq_ql.h"

namespace dsq {

#if defined(DSQ_QL_DEV)

__global__ __launch_bounds__(kBlock) void k_ql_dev(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                   const double* __restrict__ Xf, int ldf, int Pf,
                                                   const double* __restrict__ Xr, int ldr, int Pr, int N, int G,
                                                   double df, const double* __restrict__ disp,
                                                   const double* __restrict__ beta_f, const double* __restrict__ beta_r,
                                                   double* __restrict__ num, double* __restrict__ dev,
                                                   double* __restrict__ s2) {
    __shared__ double coef[kWavesPerBlock][kLrtMaxCoef + 1];
    exp_tab_fill();  // the tables of fexp_t / flog1p_t (dsq_math.h)
    log_tab_fill();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWavesPerBlock + w;
    if (g < G) {
        for (int j = lane; j < Pf; j += 64) coef[w][j] = beta_f[(size_t)g * Pf + j];
        for (int j = lane; j < Pr; j += 64) coef[w][Pf + j] = beta_r[(size_t)g * Pr + j];
    }
    __syncthreads();
    if (g >= G) return;
    const QlOut o = ql_gene<DeviceWave>(y + (size_t)g * ldn, sf, Xf, ldf, Pf, Xr, ldr, Pr, coef[w], coef[w] + Pf,
                                        disp[g], N, df);
    if (lane == 0) {
        num[g] = o.num;
        dev[g] = o.dev;
        s2[g] = o.s2;
    }
}

hipError_t launch_ql_dev(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xf, int ldf, int Pf,
                         const double* Xr, int ldr, int Pr, int N, int G, double df, const double* disp,
                         const double* beta_f, const double* beta_r, double* num, double* dev, double* s2) {
    if (G <= 0) return hipSuccess;
    if (Pf < 2 || Pr < 1 || Pr >= Pf || Pf + Pr > kLrtMaxCoef) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ql_dev, dim3(genes_to_blocks(G)), dim3(kBlock), 0, st, y, ldn, sf, Xf, ldf, Pf, Xr, ldr, Pr, N, G,
                       df, disp, beta_f, beta_r, num, dev, s2);
    return hipGetLastError();
}

#else

__global__ __launch_bounds__(kBlock) void k_ql_score(const double* __restrict__ num, const double* __restrict__ s2_post,
                                                     int n, int df_test, double df_total, double* __restrict__ F,
                                                     double* __restrict__ pval) {
    exp_tab_fill();  // (chisq_sf of the df_total = inf branch)
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const QlScore o = ql_score(num[i], s2_post[i], df_test, df_total);
    F[i] = o.F;
    pval[i] = o.p;
}

hipError_t launch_ql_score(hipStream_t st, const double* num, const double* s2_post, int n, int df_test, double df_total,
                           double* F, double* pval) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ql_score, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, num, s2_post, n, df_test,
                       df_total, F, pval);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void k_f_sf(const double* __restrict__ F, int n, int d1, double d2,
                                                 double* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = f_sf(F[i], d1, d2);
}

hipError_t launch_f_sf(hipStream_t st, const double* F, int n, int d1, double d2, double* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_f_sf, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, F, n, d1, d2, out);
    return hipGetLastError();
}

#endif

}  // namespace dsq
