// dsq_k_rlog.hip — regularized-log transformation (gfx950): one gene per wavefront, four per block; the ridge IRLS of
// dsq_rlog.h with the arrowhead normal equations in closed form.  Lanes own samples lane, lane + 64, ...
//   k_rlog<R>, R = 1, 2, 4, 8 (N <= 64 R): the lane's counts, log size factors, eta and the A, q of the pending solve stay
//     in registers; HBM traffic per gene 4N bytes of counts read once and 8N bytes of output written once.
//   k_rlog<0> (N > 512): eta lives in the gene's output row, the counts are read again every sweep (coalesced; a row of
//     12N bytes stays in L2 between the sweeps of its wavefront).
// One fused reduction of four values per sweep.  No LDS beyond the math tables, no atomics, no scratch; the lane-strided
// loops and the butterfly of DeviceWave fix the order of every addition: reruns are bit-identical.
#include "dsq_launch.h"
#include "dsq_rlog.h"

namespace dsq {

template <int R>
__global__ __launch_bounds__(kBlock) void k_rlog(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                 int N, int G, const double* __restrict__ disp,
                                                 const double* __restrict__ base_mean, double beta_prior_var,
                                                 double* out, double* __restrict__ intercept,
                                                 uint8_t* __restrict__ conv, int32_t* __restrict__ niter) {
    exp_tab_fill();  // the tables of fexp_t / flog_t / flog1p_t (dsq_math.h)
    log_tab_fill();
    __syncthreads();
    const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= G) return;
    const RlogOut o = rlog_gene<DeviceWave, R>(y + (size_t)g * ldn, sf, N, disp[g], base_mean[g], beta_prior_var,
                                               out + (size_t)g * N);
    if ((threadIdx.x & 63) == 0) {
        intercept[g] = o.intercept;
        conv[g] = (uint8_t)o.converged;
        niter[g] = o.n_iter;
    }
}

hipError_t launch_rlog(hipStream_t st, const int32_t* y, int ldn, const double* sf, int N, int G, const double* disp,
                       const double* base_mean, double beta_prior_var, double* out, double* intercept, uint8_t* conv,
                       int32_t* niter) {
    if (G <= 0) return hipSuccess;
    if (N < 1 || ldn < N) return hipErrorInvalidValue;
    const dim3 grid(genes_to_blocks(G)), block(kBlock);
#define DSQ_RLOG_LAUNCH(R_)                                                                                          \
    hipLaunchKernelGGL((k_rlog<R_>), grid, block, 0, st, y, ldn, sf, N, G, disp, base_mean, beta_prior_var, out,     \
                       intercept, conv, niter)
    if (N <= 64) DSQ_RLOG_LAUNCH(1);
    else if (N <= 128) DSQ_RLOG_LAUNCH(2);
    else if (N <= 256) DSQ_RLOG_LAUNCH(4);
    else if (N <= 512) DSQ_RLOG_LAUNCH(8);
    else DSQ_RLOG_LAUNCH(0);
#undef DSQ_RLOG_LAUNCH
    return hipGetLastError();
}

}  // namespace dsq
