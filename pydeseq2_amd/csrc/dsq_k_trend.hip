// dsq_k_trend.hip — the parametric dispersion trend on the device (gfx950): the fit (k_trend_fit: one workgroup, or
// kTrendGridBlocks cooperatively launched ones, dsq_trend_grid.h), its one-fit mode, the stand-alone loss / gradient
// (k_trend) and the fitted values a0 + a1 / mean.  The unit refers to no symbol of another kernel unit, so the test
// library (tests/devunit) links it unchanged.
#include <cstdio>

#include "dsq_launch.h"
#include "dsq_trend_grid.h"

namespace dsq {

// ---- O(G) glue between the per-gene stages (keeps the dispersion vectors on the device)
// fitted trend  a0 + a1 / normed_mean  (dds.py:826-833; a1 = 0 gives the mean trend, dds.py:1277-1299)
__global__ void k_trend_eval(const double* __restrict__ nm, int n, double a0, double a1,
                             double* __restrict__ fitted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fitted[i] = (a1 == 0.0) ? a0 : a0 + a1 / nm[i];
}

// the same with the coefficients where the trend-fit kernel left them on the device (coef[0], coef[1]): the fitted
// values and the prior can then be enqueued without the host seeing the coefficients first
__global__ void k_trend_eval_dev(const double* __restrict__ nm, int n, const double* __restrict__ coef,
                                 double* __restrict__ fitted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double a0 = coef[0], a1 = coef[1];
    if (i < n) fitted[i] = (a1 == 0.0) ? a0 : a0 + a1 / nm[i];
}

hipError_t launch_trend_eval(hipStream_t st, const double* nm, int n, double a0, double a1, double* fitted) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_trend_eval, dim3((n + 255) / 256), dim3(256), 0, st, nm, n, a0, a1, fitted);
    return hipGetLastError();
}
hipError_t launch_trend_eval_dev(hipStream_t st, const double* nm, int n, const double* coef, double* fitted) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_trend_eval_dev, dim3((n + 255) / 256), dim3(256), 0, st, nm, n, coef, fitted);
    return hipGetLastError();
}

// gamma-GLM trend loss/gradient partial sums, one row of 4 per block (summed by the host in a
// fixed order => run-to-run deterministic): {sum(t/m + log m), sum g0, sum g1, count}
constexpr int kTrendBlocks = 256;
__global__ __launch_bounds__(256) void k_trend(const double* __restrict__ cov,
                                               const double* __restrict__ targets,
                                               const uint8_t* __restrict__ keep, int n, double a0,
                                               double a1, double* __restrict__ partials) {
    __shared__ double red[4][4];
    double s = 0.0, g0 = 0.0, g1 = 0.0, cnt = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (keep != nullptr && keep[i] == 0) continue;
        const double c = cov[i], t = targets[i];
        const double m = a0 + a1 * c;
        const double v = t / m + log(m);
        if (v != v) continue;  // np.nanmean skips NaN terms
        s += v;
        const double r = (t / m - 1.0) / m;
        g0 += r;
        g1 += r * c;
        cnt += 1.0;
    }
    s = DeviceWave::sum(s); g0 = DeviceWave::sum(g0); g1 = DeviceWave::sum(g1); cnt = DeviceWave::sum(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = s; red[w][1] = g0; red[w][2] = g1; red[w][3] = cnt; }
    __syncthreads();
    if (threadIdx.x < 4) {
        partials[blockIdx.x * 4 + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
}

// partials: [kTrendBlocks][4] device doubles
hipError_t launch_trend_loss_grad(hipStream_t st, const double* cov, const double* targets,
                                  const uint8_t* keep, int n, double a0, double a1, double* partials) {
    hipLaunchKernelGGL(k_trend, dim3(kTrendBlocks), dim3(256), 0, st, cov, targets, keep, n, a0, a1,
                       partials);
    return hipGetLastError();
}

// ------------------------------------------------------------------ trend fit (the passes: dsq_trend_grid.h)
__global__ __launch_bounds__(64 * kTrendWaves) void k_trend_fit(const double* __restrict__ disp,
                                                                const double* __restrict__ means, int n,
                                                                double min_disp, double max_disp,
                                                                uint8_t* __restrict__ keep, TrendGridMem* Gm,
                                                                double* __restrict__ out5, int single) {
    __shared__ TrendShared S;
    trend_grid_run(TrendData{disp, means, keep, n, min_disp, max_disp, single}, Gm, S, [&](GridTrendOps& ops) {
        const TrendOut o = trend_fit_core(ops, S.W, single != 0);
        if (threadIdx.x == 0 && blockIdx.x == 0) {
            const bool timed_out =
                gridDim.x > 1 && __hip_atomic_load(&Gm->timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
            out5[0] = o.a0; out5[1] = o.a1; out5[2] = timed_out ? -1.0 : (double)o.ok;
            out5[3] = (double)o.n_outer; out5[4] = (double)o.n_kept;
#ifdef DSQ_TREND_PHASES
            printf("trend phases: evals %d  optimiser %lld  pass %lld cycles | build_B %lld cauchy %lld subsm %lld "
                   "ls-setup %lld fg %lld after-ls+update %lld\n", ops.n_eval, ops.c_opt, ops.c_pass, g_lbd_phase[0],
                   g_lbd_phase[1], g_lbd_phase[2], g_lbd_phase[3], g_lbd_phase[4], g_lbd_phase[5]);
            for (int q = 0; q < 8; ++q) g_lbd_phase[q] = 0;
#endif
        }
    });
}

size_t trend_grid_mem_bytes() { return sizeof(TrendGridMem); }

// out5: {a0, a1, ok (1 converged, 0 not, -1 the workgroups' exchange timed out), gamma-GLM fits, genes in the last fit}
hipError_t launch_trend_fit(hipStream_t st, const double* disp, const double* means, int n, double min_disp,
                            double max_disp, uint8_t* keep, double* out5, void* grid_mem, int force_grid) {
    TrendGridMem* gm = (TrendGridMem*)grid_mem;
    int single = 0;
    if (gm != nullptr && force_grid >= 0 && (force_grid > 0 || n >= 3072)) {  // (measured crossover of one workgroup against the grid: ~3000 genes)
        hipError_t e0 = hipMemsetAsync(gm, 0, sizeof(TrendGridMem), st);
        if (e0 != hipSuccess) return e0;
        void* args[] = {(void*)&disp, (void*)&means, (void*)&n,    (void*)&min_disp, (void*)&max_disp,
                        (void*)&keep, (void*)&gm,    (void*)&out5, (void*)&single};
        return hipLaunchCooperativeKernel((const void*)k_trend_fit, dim3(kTrendGridBlocks), dim3(64 * kTrendWaves), args,
                                          0, st);
    }
    hipLaunchKernelGGL(k_trend_fit, dim3(1), dim3(64 * kTrendWaves), 0, st, disp, means, n, min_disp, max_disp, keep,
                       (TrendGridMem*)nullptr, out5, 0);
    return hipGetLastError();
}

// Inference.dispersion_trend_gamma_glm (inference.py:284-308): ONE gamma-GLM fit of targets ~ a0 + a1 * cov
hipError_t launch_trend_glm(hipStream_t st, const double* targets, const double* cov, int n, uint8_t* keep,
                            double* out5) {
    hipLaunchKernelGGL(k_trend_fit, dim3(1), dim3(64 * kTrendWaves), 0, st, targets, cov, n, 0.0, 0.0, keep,
                       (TrendGridMem*)nullptr, out5, 1);
    return hipGetLastError();
}

}  // namespace dsq
