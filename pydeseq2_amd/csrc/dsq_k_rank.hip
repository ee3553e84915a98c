// dsq_k_rank.hip — Wilcoxon rank-sum test of K comparisons on the normalised counts (gfx950), dsq_rank.h.
//   k_ranksum: one gene per wavefront, grid.y = the comparison.  The wave stages the used samples' y / sf stratum by
//     stratum in its private LDS row (`stride` doubles, the longest padded row of the K comparisons), sorts each stratum
//     with LdsSorter, takes the tested samples' midranks by binary search and the tie term from the run starts.  No
//     atomics, no block-wide synchronisation: a rerun gives the same bits, and so does a launch of one comparison alone.
//   The launch plan (waves per workgroup, dynamic LDS) is rank_plan(stride) of the header: 4 waves up to 5120 doubles,
//   2 up to 10 240, 1 up to 16 384 (128 KiB).
#include "dsq_launch.h"
#include "dsq_lds_sort.h"
#include "dsq_rank.h"

namespace dsq {

__global__ __launch_bounds__(kBlock) void k_ranksum(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                    int G, const int32_t* __restrict__ order, int ldo,
                                                    const int32_t* __restrict__ seg, const int32_t* __restrict__ pad,
                                                    int lds, const int32_t* __restrict__ nstrata,
                                                    const int8_t* __restrict__ labels, int ldl, int alt, int stride,
                                                    double* __restrict__ stat, double* __restrict__ pvalue,
                                                    double* __restrict__ usum, double* __restrict__ ties, int ldg) {
    extern __shared__ __attribute__((aligned(16))) double rank_lds[];
    const int w = threadIdx.x >> 6, k = blockIdx.y;
    const int g = blockIdx.x * (int)(blockDim.x >> 6) + w;
    if (g >= G) return;
    const RankLayout Q{order + (size_t)k * ldo, seg + (size_t)k * lds, pad + (size_t)k * lds, nstrata[k],
                       labels + (size_t)k * ldl};
    const RankOut o = ranksum_gene<DeviceWave>(y + (size_t)g * ldn, sf, Q, alt, rank_lds + (size_t)w * stride, LdsSorter());
    if ((threadIdx.x & 63) == 0) {
        const size_t at = (size_t)k * ldg + g;
        stat[at] = o.stat;
        pvalue[at] = o.pvalue;
        usum[at] = o.usum;
        ties[at] = o.ties;
    }
}

// L: the longest padded row of the K comparisons (the caller has checked every layout against it, rank_check_layout)
hipError_t launch_ranksum(hipStream_t st, const int32_t* y, int ldn, const double* sf, int G, int K, const int32_t* order,
                          int ldo, const int32_t* seg, const int32_t* pad, int lds, const int32_t* nstrata,
                          const int8_t* labels, int ldl, int alt, int L, double* stat, double* pvalue, double* usum,
                          double* ties, int ldg) {
    if (G <= 0 || K <= 0) return hipSuccess;
    const RankPlan plan = rank_plan(L);
    if (plan.waves < 1 || K > 65535 || ldg < G) return hipErrorInvalidValue;
    if (plan.lds_bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)k_ranksum, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)plan.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ranksum, dim3((G + plan.waves - 1) / plan.waves, K), dim3(64 * plan.waves), plan.lds_bytes, st, y,
                       ldn, sf, G, order, ldo, seg, pad, lds, nstrata, labels, ldl, alt, L, stat, pvalue, usum, ties, ldg);
    return hipGetLastError();
}

}  // namespace dsq
