// dsq_k_ash.hip — adaptive shrinkage (gfx950), dsq_ash.h.
//   k_ash_fit: one workgroup of four waves per contrast.  Wave w walks the 64-gene chunks w, w + 4, ... (lane = gene:
//     M logarithms and exponentials, then the chunk's share of H on the fp64 matrix cores through WideGram); the four
//     partial H (each in the place of its wave's chunk buffer), d and the two sums are added in wave order by the whole
//     block; wave 0 runs the stop test, the QP and the step control.  LDS at M = 48: 4 x 26.4 KB of wave-private chunk
//     buffers and 42.4 KB for the block (H, the working set's factor, a dozen vectors): 148 KB.  No grid-wide
//     synchronisation, no atomics: a rerun gives the same bits.
//   k_ash_post: one thread per (contrast, gene).
#include "dsq_ash.h"
#include "dsq_launch.h"

namespace dsq {

constexpr int kAshWaves = kWavesPerBlock;

__global__ __launch_bounds__(kBlock) void k_ash_fit(const double* __restrict__ lfc, const double* __restrict__ se, int G,
                                                    int ldg, const double* __restrict__ sd, const int32_t* __restrict__ mk,
                                                    int ldm, int max_iter, double* __restrict__ pi,
                                                    int32_t* __restrict__ niter, uint8_t* __restrict__ conv,
                                                    double* __restrict__ kkt, double* __restrict__ loglik) {
    extern __shared__ __attribute__((aligned(16))) double ash_lds[];
    const int k = blockIdx.x;
    const int M = mk[k];
    if (M < 1 || M > kAshMaxM) return;
    const int tid = threadIdx.x, wv = tid >> 6;
    const double* b = lfc + (size_t)k * ldg;
    const double* s = se + (size_t)k * ldg;
    AshBlock B;
    B.bind(ash_lds, M, kAshWaves);
    double* wave_base = ash_lds + AshBlock::doubles(M, kAshWaves);
    const int wave_doubles = ash_wave_doubles(M, true);
    AshWave Q;
    Q.bind(wave_base + wv * wave_doubles, M, true);

    for (int m = tid; m < M; m += kBlock) {
        const double v = sd[(size_t)k * ldm + m];
        B.sd2[m] = v * v;
        B.xt[m] = 1.0 / (double)M;
    }
    if (tid == 0) { B.ctl[0] = 1; B.ctl[1] = 0; }
    wide_zero_pad_rows<DeviceWave>(Q.W);
    int* cnt = B.idx;  // (free until the first QP)
    const int c = ash_count<DeviceWave>(b, s, G, wv, kAshWaves);
    if ((tid & 63) == 0) cnt[wv] = c;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < kAshWaves; ++w) n += cnt[w];
    __syncthreads();
    if (n == 0) {  // no used gene: NaN in every output of the contrast
        for (int m = tid; m < M; m += kBlock) pi[(size_t)k * ldm + m] = NAN;
        if (tid == 0) { niter[k] = 0; conv[k] = 0; kkt[k] = NAN; loglik[k] = NAN; }
        return;
    }
    AshState S;
    S.begin(n, max_iter);
    for (;;) {
        const bool gram = B.ctl[0] != 0;
        ash_pass<DeviceWave>(B, Q, wv, b, s, G, B.xt, S.inv_n, gram);
        __syncthreads();
        ash_combine(B, wave_base, wave_doubles, gram, tid, kBlock);
        __syncthreads();
        if (wv == 0) ash_drive<DeviceWave>(B, S);
        __syncthreads();
        if (B.ctl[1] != 0) break;
    }
    if (wv == 0) {
        const AshFit o = ash_result<DeviceWave>(B, S, n, pi + (size_t)k * ldm);
        if (tid == 0) { niter[k] = o.n_iter; conv[k] = (uint8_t)o.converged; kkt[k] = o.kkt; loglik[k] = o.loglik; }
    }
}

__global__ __launch_bounds__(kBlock) void k_ash_post(const double* __restrict__ lfc, const double* __restrict__ se, int G,
                                                     int ldg, const double* __restrict__ sd, const int32_t* __restrict__ mk,
                                                     int ldm, const double* __restrict__ pi, double* __restrict__ post_mean,
                                                     double* __restrict__ post_sd, double* __restrict__ lfsr) {
    const int k = blockIdx.y;
    const int g = blockIdx.x * kBlock + threadIdx.x;
    const int M = mk[k];
    if (g >= G || M < 1 || M > kAshMaxM) return;
    const size_t at = (size_t)k * ldg + g;
    double pm, psd, fs;
    ash_posterior(lfc[at], se[at], sd + (size_t)k * ldm, pi + (size_t)k * ldm, M, pm, psd, fs);
    post_mean[at] = pm;
    post_sd[at] = psd;
    lfsr[at] = fs;
}

hipError_t launch_ash_fit(hipStream_t st, const double* lfc, const double* se, int G, int ldg, int K, const double* sd,
                          const int32_t* m, int ldm, int max_m, int max_iter, double* pi, int32_t* niter, uint8_t* conv,
                          double* kkt, double* loglik) {
    if (K <= 0 || G <= 0 || max_m <= 0) return hipSuccess;
    if (max_m > kAshMaxM || ldg < G || ldm < max_m || max_iter < 1) return hipErrorInvalidValue;
    const size_t bytes = sizeof(double) * (size_t)(AshBlock::doubles(max_m, kAshWaves) + kAshWaves * ash_wave_doubles(max_m, true));
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)k_ash_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ash_fit, dim3(K), dim3(kBlock), bytes, st, lfc, se, G, ldg, sd, m, ldm, max_iter, pi, niter, conv,
                       kkt, loglik);
    return hipGetLastError();
}

hipError_t launch_ash_post(hipStream_t st, const double* lfc, const double* se, int G, int ldg, int K, const double* sd,
                           const int32_t* m, int ldm, const double* pi, double* post_mean, double* post_sd, double* lfsr) {
    if (K <= 0 || G <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ash_post, dim3((G + kBlock - 1) / kBlock, K), dim3(kBlock), 0, st, lfc, se, G, ldg, sd, m, ldm, pi,
                       post_mean, post_sd, lfsr);
    return hipGetLastError();
}

}  // namespace dsq
