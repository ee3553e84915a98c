// dsq_k_proj.hip — hidden-batch factors and batch removal (gfx950), dsq_proj.h.  One gene per wavefront throughout.
//   k_log_counts: Y = log(y / sf + eps) of the gene-major counts; 4N bytes read and 8N written per gene.
//   k_nb_residuals: deviance / Pearson residuals from a finished fit, the gene's coefficients in wave-private LDS, the
//     transposed design and the size factors shared by every gene (L2); 4N bytes read and 8N written per gene, two
//     logarithms and one exponential per sample: transcendental-bound like k_lrt.
//   k_project_out<MODE>: out = x - (x P) B^T; one pass over the row per eight columns of P, one for the subtraction.
//     MODE 2 (N <= 1024): the row in registers, all its loads in flight at once; 1: the first pass leaves the row in the
//     wave's LDS and the later ones read that - either way 8N bytes read and 8N written per gene; 0: a row longer than the
//     plan stages (proj_plan: N > 16 320) is re-read from memory by every pass.  P^T and B^T are shared by every gene
//     (L2).  No atomics, no block-wide synchronisation after the table fill: a rerun gives the same bits.
#include "dsq_launch.h"
#include "dsq_proj.h"

namespace dsq {

__global__ __launch_bounds__(kBlock) void k_log_counts(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                       int N, int G, int normalized, double eps, double* __restrict__ out,
                                                       int ld) {
    log_tab_fill();
    __syncthreads();
    const int g = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6);
    if (g >= G) return;
    log_counts_row<DeviceWave>(y + (size_t)g * ldn, sf, N, normalized != 0, eps, out + (size_t)g * ld);
}

__global__ __launch_bounds__(kBlock) void k_nb_residuals(const int32_t* __restrict__ y, int ldn,
                                                         const double* __restrict__ sf, const double* __restrict__ Xt,
                                                         int ldx, int P, int N, int G, const double* __restrict__ disp,
                                                         const double* __restrict__ beta, int kind,
                                                         double* __restrict__ out, int ld) {
    __shared__ double coef[kWavesPerBlock][DSQ_MAX_P];
    exp_tab_fill();
    log_tab_fill();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWavesPerBlock + w;
    if (g < G)
        for (int j = lane; j < P; j += 64) coef[w][j] = beta[(size_t)g * P + j];
    __syncthreads();
    if (g >= G) return;
    nb_residuals_row<DeviceWave>(y + (size_t)g * ldn, sf, Xt, (size_t)ldx, P, coef[w], disp[g], N, kind,
                                 out + (size_t)g * ld);
}

// x and out may be the same matrix: no __restrict__ on either
// (four waves per SIMD asked for: at most 128 registers - the fully unrolled register path would take every one it can)
template <int MODE>
__global__ __launch_bounds__(kBlock, 4) void k_project_out(const double* x, int ld, const double* __restrict__ Pt,
                                                        const double* __restrict__ Bt, int ldp, int q, int N, int G,
                                                        int post, double eps, int stride, double* out, int ldo,
                                                        double* __restrict__ coef_out) {
    extern __shared__ __attribute__((aligned(16))) double proj_lds[];
    exp_tab_fill();
    __syncthreads();
    const int w = threadIdx.x >> 6;
    const int g = blockIdx.x * (int)(blockDim.x >> 6) + w;
    if (g >= G) return;
    double* mine = proj_lds + (size_t)w * stride;  // kProjMaxQ coefficients, then the row
    double* co = coef_out != nullptr ? coef_out + (size_t)g * q : nullptr;
    if constexpr (MODE == 2)
        project_row_reg<DeviceWave>(x + (size_t)g * ld, Pt, Bt, (size_t)ldp, q, N, post, eps, mine, out + (size_t)g * ldo, co);
    else
        project_row<DeviceWave, MODE == 1>(x + (size_t)g * ld, mine + kProjMaxQ, Pt, Bt, (size_t)ldp, q, N, post, eps, mine,
                                           out + (size_t)g * ldo, co);
}

hipError_t launch_log_counts(hipStream_t st, const int32_t* y, int ldn, const double* sf, int N, int G, int normalized,
                             double eps, double* out, int ld) {
    if (G <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_log_counts, dim3(genes_to_blocks(G)), dim3(kBlock), 0, st, y, ldn, sf, N, G, normalized, eps, out,
                       ld);
    return hipGetLastError();
}

hipError_t launch_nb_residuals(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xt, int ldx, int P,
                               int N, int G, const double* disp, const double* beta, int kind, double* out, int ld) {
    if (G <= 0) return hipSuccess;
    if (P < 1 || P > DSQ_MAX_P) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nb_residuals, dim3(genes_to_blocks(G)), dim3(kBlock), 0, st, y, ldn, sf, Xt, ldx, P, N, G, disp,
                       beta, kind, out, ld);
    return hipGetLastError();
}

hipError_t launch_project_out(hipStream_t st, const double* x, int ld, const double* Pt, const double* Bt, int ldp, int q,
                              int N, int G, int post, double eps, double* out, int ldo, double* coef_out) {
    if (G <= 0) return hipSuccess;
    const ProjPlan plan = proj_plan(N);
    if (plan.waves < 1 || q < 1 || q > kProjMaxQ || ld < N || ldo < N || ldp < N) return hipErrorInvalidValue;
    if (plan.lds_bytes > 48 * 1024) {  // (the LDS rows only)
        const hipError_t e = hipFuncSetAttribute((const void*)k_project_out<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)plan.lds_bytes);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((G + plan.waves - 1) / plan.waves), block(64 * plan.waves);
    if (plan.staged == 2)
        hipLaunchKernelGGL(k_project_out<2>, grid, block, plan.lds_bytes, st, x, ld, Pt, Bt, ldp, q, N, G, post, eps,
                           plan.stride, out, ldo, coef_out);
    else if (plan.staged == 1)
        hipLaunchKernelGGL(k_project_out<1>, grid, block, plan.lds_bytes, st, x, ld, Pt, Bt, ldp, q, N, G, post, eps,
                           plan.stride, out, ldo, coef_out);
    else
        hipLaunchKernelGGL(k_project_out<0>, grid, block, plan.lds_bytes, st, x, ld, Pt, Bt, ldp, q, N, G, post, eps,
                           plan.stride, out, ldo, coef_out);
    return hipGetLastError();
}

}  // namespace dsq
