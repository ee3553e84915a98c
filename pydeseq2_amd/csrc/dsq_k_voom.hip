// dsq_k_voom.hip — limma-voom (gfx950, dsq_voom.h), one gene per wavefront, any row length (64-sample chunks, the counts
// re-read per pass), run-time design width P <= kWideMaxP:
//   k_voom_fit1  log-CPM, unweighted least squares through pinv(X), residual standard deviation and mean log-CPM; the
//                coefficients in wave-private static LDS.  Per gene 4N bytes of counts per pass (ceil(P / 8) + 1 passes,
//                the later ones from L2), 8 (P + 2) written.
//   k_voom_wls   precision weights from the knot table (in LDS, shared by the workgroup), X^T W X by the matrix cores in
//                the wave's segment of dynamic LDS (WideWork, as the run-time-P kernels of dsq_k_wide.hip: 4, 2 or 1 waves
//                per workgroup), Cholesky, a second sweep for the residual variance, inverse, K contrasts.  Per gene 8N
//                bytes of counts, 8 P read, 8 (P + 1 + 2K) written, 16N more when the layers E and w are asked for.
// The design, its pseudo-inverse, the per-sample offsets, the knots and the contrasts are shared by every gene and stay in
// L2.  No atomics, no scratch; vector stores only.  Built with -ffp-contract=off (Makefile): k_voom_fit1 and the layers of
// k_voom_wls are held to the bits of the host build (tests/hostvoom).
#include "dsq_launch.h"
#include "dsq_voom.h"

namespace dsq {

__global__ __launch_bounds__(kBlock) void k_voom_fit1(const int32_t* __restrict__ y, int ldn,
                                                      const double* __restrict__ off, const double* __restrict__ Xt,
                                                      const double* __restrict__ pinvXt, int ldx, int P, int N, int G,
                                                      double* __restrict__ beta1, double* __restrict__ amean,
                                                      double* __restrict__ sigma1) {
    __shared__ double coef[kWavesPerBlock][kWideMaxP];
    log_tab_fill();  // the table of flog_t (dsq_math.h)
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWavesPerBlock + w;
    if (g >= G) return;
    const VoomFit1 o = voom_fit1_row<DeviceWave>(y + (size_t)g * ldn, off, Xt, pinvXt, (size_t)ldx, P, N, coef[w]);
    DeviceWave::sync();
    for (int j = lane; j < P; j += 64) beta1[(size_t)g * P + j] = coef[w][j];
    if (lane == 0) {
        amean[g] = o.amean;
        sigma1[g] = o.sigma;
    }
}

hipError_t launch_voom_fit1(hipStream_t st, const int32_t* y, int ldn, const double* off, const double* Xt,
                            const double* pinvXt, int ldx, int P, int N, int G, double* beta1, double* amean,
                            double* sigma1) {
    if (G <= 0) return hipSuccess;
    if (P < 1 || P > kWideMaxP || N <= P) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_voom_fit1, dim3(genes_to_blocks(G)), dim3(kBlock), 0, st, y, ldn, off, Xt, pinvXt, ldx, P, N, G,
                       beta1, amean, sigma1);
    return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void k_voom_wls(const int32_t* __restrict__ y, int ldn,
                                                     const double* __restrict__ off, const double* __restrict__ Xt,
                                                     int ldx, int P, int N, int G, const double* __restrict__ beta1,
                                                     const double* __restrict__ knot_x,
                                                     const double* __restrict__ knot_f, int nk,
                                                     const double* __restrict__ contrasts, int K,
                                                     double* __restrict__ beta, double* __restrict__ sigma2,
                                                     double* __restrict__ est, double* __restrict__ u,
                                                     double* __restrict__ E_out, double* __restrict__ w_out, int ldl,
                                                     int per_wave_doubles) {
    extern __shared__ __attribute__((aligned(16))) double voom_lds[];
    __shared__ double kx[kVoomMaxKnots], kf[kVoomMaxKnots];
    log_tab_fill();  // the table of flog_t (dsq_math.h)
    for (int i = threadIdx.x; i < nk; i += blockDim.x) {
        kx[i] = knot_x[i];
        kf[i] = knot_f[i];
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * (blockDim.x >> 6) + w;
    if (g >= G) return;
    WideWork W;
    W.bind(voom_lds + (size_t)w * per_wave_doubles, P);
    for (int j = lane; j < P; j += 64) W.v(2)[j] = beta1[(size_t)g * P + j];
    DeviceWave::sync();
    const bool layers = E_out != nullptr && w_out != nullptr;
    double* Eg = layers ? E_out + (size_t)g * ldl : nullptr;
    double* wg = layers ? w_out + (size_t)g * ldl : nullptr;
    bool bad = false;  // a gene without counts (k_voom_fit1 left NaN): NaN everywhere
    for (int j = 0; j < P; ++j) bad = bad || W.v(2)[j] != W.v(2)[j];
    if (bad) {
        const double nan = __builtin_nan("");
        for (int j = lane; j < P; j += 64) beta[(size_t)g * P + j] = nan;
        for (int k = lane; k < K; k += 64) {
            est[(size_t)g * K + k] = nan;
            u[(size_t)g * K + k] = nan;
        }
        if (lane == 0) sigma2[g] = nan;
        if (layers)
            for (int n = lane; n < N; n += 64) {
                Eg[n] = nan;
                wg[n] = nan;
            }
        return;
    }
    const double s2 = voom_wls_row<DeviceWave>(y + (size_t)g * ldn, off, Xt, ldx, N, W, kx, kf, nk, contrasts, K,
                                               lane == 0, est + (size_t)g * K, u + (size_t)g * K, Eg, wg);
    for (int j = lane; j < P; j += 64) beta[(size_t)g * P + j] = W.v(0)[j];
    if (lane == 0) sigma2[g] = s2;
}

hipError_t launch_voom_wls(hipStream_t st, const int32_t* y, int ldn, const double* off, const double* Xt, int ldx, int P,
                           int N, int G, const double* beta1, const double* knot_x, const double* knot_f, int nk,
                           const double* contrasts, int K, double* beta, double* sigma2, double* est, double* u,
                           double* E_out, double* w_out, int ldl) {
    if (G <= 0) return hipSuccess;
    if (P < 1 || P > kWideMaxP || N <= P || K < 1 || nk < 2 || nk > kVoomMaxKnots) return hipErrorInvalidValue;
    // as many waves per workgroup (4, 2 or 1) as fit 64 KB of dynamic LDS (the plan of the run-time-P kernels)
    const size_t per_wave = (size_t)wide_work_doubles(P) * sizeof(double);
    const int wpb = per_wave * 4 <= 64 * 1024 ? 4 : (per_wave * 2 <= 64 * 1024 ? 2 : 1);
    const size_t smem = per_wave * wpb;
    if (smem > 48 * 1024) {
        (void)hipFuncSetAttribute((const void*)k_voom_wls, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(k_voom_wls, dim3((G + wpb - 1) / wpb), dim3(64 * wpb), smem, st, y, ldn, off, Xt, ldx, P, N, G,
                       beta1, knot_x, knot_f, nk, contrasts, K, beta, sigma2, est, u, E_out, w_out, ldl,
                       (int)(per_wave / 8));
    return hipGetLastError();
}

}  // namespace dsq
