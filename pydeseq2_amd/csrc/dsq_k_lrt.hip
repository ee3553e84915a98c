// dsq_k_lrt.hip — likelihood-ratio statistic and p-value of a reduced design (gfx950): one gene per wavefront, the full
// and the reduced model's coefficients in wave-private LDS, run-time widths (P_full <= 128, 1 <= P_reduced < P_full).
// One sweep over the gene's row: algorithmic HBM traffic 4N bytes of counts per gene, 8 (P_f + P_r) + 8 read and 16
// written; the two transposed designs and the size factors are shared by every gene and stay in L2.  No atomics, no
// scratch; the lane-strided loop and the butterfly of DeviceWave::sum fix the order of every addition.
#include "dsq_launch.h"
#include "dsq_lrt.h"

namespace dsq {

__global__ __launch_bounds__(kBlock) void k_lrt(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                const double* __restrict__ Xf, int ldf, int Pf,
                                                const double* __restrict__ Xr, int ldr, int Pr, int N, int G,
                                                const double* __restrict__ disp, const double* __restrict__ beta_f,
                                                const double* __restrict__ beta_r, double* __restrict__ stat,
                                                double* __restrict__ pval) {
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
    const LrtOut o = lrt_gene<DeviceWave>(y + (size_t)g * ldn, sf, Xf, ldf, Pf, Xr, ldr, Pr, coef[w], coef[w] + Pf,
                                          disp[g], N);
    if (lane == 0) {
        stat[g] = o.stat;
        pval[g] = o.p;
    }
}

hipError_t launch_lrt(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xf, int ldf, int Pf,
                      const double* Xr, int ldr, int Pr, int N, int G, const double* disp, const double* beta_f,
                      const double* beta_r, double* stat, double* pval) {
    if (G <= 0) return hipSuccess;
    if (Pf < 2 || Pr < 1 || Pr >= Pf || Pf + Pr > kLrtMaxCoef) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lrt, dim3(genes_to_blocks(G)), dim3(kBlock), 0, st, y, ldn, sf, Xf, ldf, Pf, Xr, ldr, Pr, N, G,
                       disp, beta_f, beta_r, stat, pval);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void k_chisq_sf(const double* __restrict__ x, int n, int df,
                                                     double* __restrict__ out) {
    exp_tab_fill();
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = chisq_sf(x[i], df);
}

hipError_t launch_chisq_sf(hipStream_t st, const double* x, int n, int df, double* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_chisq_sf, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, x, n, df, out);
    return hipGetLastError();
}

}  // namespace dsq
