// dsq_k_gram.hip — sample PCA / sample distances (gfx950), dsq_gram.h.
//   k_row_meanvar_gm: gene-major rows, one gene per wavefront, four per block.
//   k_row_meanvar_sm: sample-major, eight threads per gene walking the samples, 32 neighbouring genes per block
//     (coalesced across genes); the same order of the sums as the gene-major kernel (dsq_gram.h).
//   k_gram_pack: 32 x 32 tiles through LDS: the selected genes, centred, gene-major [K][pad16(N)], zero padding.
//   k_sample_gram: one workgroup per (lower-triangle macro tile, gene slice); 73.7 KB of LDS (two panels of 32 genes
//     x 128 samples, row stride 144), 32 accumulator fragments per lane (128 VGPRs).
//   k_gram_reduce: S[i][j] = sum of the slices' partial tiles in ascending order, both triangles.
//   k_gram_dist: D from S.
#include "dsq_gram.h"
#include "dsq_launch.h"

namespace dsq {

__global__ __launch_bounds__(kBlock) void k_row_meanvar_gm(const double* __restrict__ x, int N, int G, size_t ld,
                                                           double* __restrict__ mean, double* __restrict__ var) {
    const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= G) return;
    double m, v;
    row_meanvar_row<DeviceWave>(x + (size_t)g * ld, N, m, v);
    if ((threadIdx.x & 63) == 0) {
        mean[g] = m;
        if (var != nullptr) var[g] = v;
    }
}

constexpr int kRowQ = 8;                   // threads per gene of the sample-major kernel (row_sum_part)
constexpr int kRowGenes = kBlock / kRowQ;  // genes per block: 32 neighbours, 256 B of every sample's row

__global__ __launch_bounds__(kBlock) void k_row_meanvar_sm(const double* __restrict__ x, int N, int G, size_t ld,
                                                           double* __restrict__ mean, double* __restrict__ var) {
    __shared__ double part[kRowGenes][kRowQ + 1];
    __shared__ double mean_s[kRowGenes];
    const int tx = threadIdx.x & (kRowGenes - 1), q = threadIdx.x / kRowGenes;
    const int g = blockIdx.x * kRowGenes + tx;
    const bool mine = g < G;
    const double* col = x + (mine ? g : 0);  // (a thread beyond G walks gene 0 and writes nothing: it reaches the barriers)
    part[tx][q] = row_sum_part<kRowQ>(col, ld, N, 0.0, false, q);
    __syncthreads();
    if (q == 0) {
        double r[kRowQ];
#pragma unroll
        for (int i = 0; i < kRowQ; ++i) r[i] = part[tx][i];
        const double m = row_sum_join<kRowQ>(r) / (double)N;
        mean_s[tx] = m;
        if (mine) mean[g] = m;
    }
    __syncthreads();
    if (var == nullptr) return;
    part[tx][q] = row_sum_part<kRowQ>(col, ld, N, mean_s[tx], true, q);
    __syncthreads();
    if (q == 0 && mine) {
        double r[kRowQ];
#pragma unroll
        for (int i = 0; i < kRowQ; ++i) r[i] = part[tx][i];
        var[g] = row_sum_join<kRowQ>(r) / (double)(N - 1);  // N == 1: 0 / 0 = NaN (R's NA)
    }
}

constexpr int kPackTile = 32;

__global__ __launch_bounds__(kBlock) void k_gram_pack(const double* __restrict__ x, int layout, size_t ld, int N,
                                                      const int32_t* __restrict__ sel, const double* __restrict__ mean,
                                                      int K, int pad, double* __restrict__ xp) {
    __shared__ double tile[kPackTile][kPackTile + 1];
    const int k0 = blockIdx.x * kPackTile, s0 = blockIdx.y * kPackTile;
    const int tx = threadIdx.x & (kPackTile - 1), ty = threadIdx.x >> 5;  // 32 x 8
    if (layout == 1) {  // gene-major: rows are read as they are written
        for (int dk = ty; dk < kPackTile; dk += 8) {
            const int k = k0 + dk, s = s0 + tx;
            if (k < K && s < pad) xp[(size_t)k * (size_t)pad + (size_t)s] = gram_pack_value(x, 1, ld, N, sel, mean, k, s);
        }
        return;
    }
    for (int ds = ty; ds < kPackTile; ds += 8) {  // sample-major: lanes along the genes, transposed through LDS
        const int k = k0 + tx, s = s0 + ds;
        tile[ds][tx] = (k < K && s < pad) ? gram_pack_value(x, 0, ld, N, sel, mean, k, s) : 0.0;
    }
    __syncthreads();
    for (int dk = ty; dk < kPackTile; dk += 8) {
        const int k = k0 + dk, s = s0 + tx;
        if (k < K && s < pad) xp[(size_t)k * (size_t)pad + (size_t)s] = tile[tx][dk];
    }
}

__global__ __launch_bounds__(kBlock) void k_sample_gram(GramPlan P, const double* __restrict__ xp, double* __restrict__ part,
                                                        double* __restrict__ S, size_t lds_S) {
    extern __shared__ __attribute__((aligned(16))) double gram_lds[];
    gram_block<DeviceWave>(P, (int)blockIdx.x, (int)blockIdx.y, xp, part, S, lds_S, gram_lds);
}

__global__ __launch_bounds__(kBlock) void k_gram_reduce(GramPlan P, const double* __restrict__ part, double* __restrict__ S,
                                                        size_t lds_S) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= P.N || j > i) return;
    const double v = gram_reduce_entry(P, part, i, j);
    S[(size_t)i * lds_S + (size_t)j] = v;
    S[(size_t)j * lds_S + (size_t)i] = v;
}

__global__ __launch_bounds__(kBlock) void k_gram_dist(const double* __restrict__ S, int N, size_t lds_S,
                                                      double* __restrict__ D, size_t ldd) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= N || j >= N) return;
    D[(size_t)i * ldd + (size_t)j] = gram_dist_entry(S, lds_S, i, j);
}

size_t sample_gram_work_doubles(int N, int K) { return N < 1 || K < 0 ? 0 : gram_work_doubles(N, K); }

hipError_t launch_row_meanvar(hipStream_t st, const double* x, int layout, int N, int G, int ld, double* mean, double* var) {
    if (N <= 0 || G <= 0) return hipSuccess;
    if (layout == DSQ_GENE_MAJOR)
        hipLaunchKernelGGL(k_row_meanvar_gm, dim3(genes_to_blocks(G)), dim3(kBlock), 0, st, x, N, G, (size_t)ld, mean, var);
    else
        hipLaunchKernelGGL(k_row_meanvar_sm, dim3((G + kRowGenes - 1) / kRowGenes), dim3(kBlock), 0, st, x, N, G, (size_t)ld,
                           mean, var);
    return hipGetLastError();
}

hipError_t launch_sample_gram(hipStream_t st, const double* x, int layout, int N, int ld, const int32_t* sel, int K,
                              const double* mean, double* work, double* S, int lds_S) {
    if (N <= 0) return hipSuccess;
    const GramPlan P = gram_plan(N, K);
    const dim3 rgrid((N + 63) / 64, (N + 3) / 4);
    if (K <= 0) {  // no gene: S = 0 (the reduction of no slice)
        hipLaunchKernelGGL(k_gram_reduce, rgrid, dim3(kBlock), 0, st, P, (const double*)nullptr, S, (size_t)lds_S);
        return hipGetLastError();
    }
    double* xp = work;
    double* part = work + (size_t)K * (size_t)P.pad;
    hipLaunchKernelGGL(k_gram_pack, dim3((K + kPackTile - 1) / kPackTile, P.pad / kPackTile + (P.pad % kPackTile != 0)),
                       dim3(kBlock), 0, st, x, layout, (size_t)ld, N, sel, mean, K, P.pad, xp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t bytes = sizeof(double) * (size_t)kGramLdsDoubles;
    e = hipFuncSetAttribute((const void*)k_sample_gram, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sample_gram, dim3(P.ntiles, P.slices), dim3(kBlock), bytes, st, P, (const double*)xp, part, S,
                       (size_t)lds_S);
    e = hipGetLastError();
    if (e != hipSuccess || P.slices == 1) return e;
    hipLaunchKernelGGL(k_gram_reduce, rgrid, dim3(kBlock), 0, st, P, (const double*)part, S, (size_t)lds_S);
    return hipGetLastError();
}

hipError_t launch_gram_dist(hipStream_t st, const double* S, int N, int lds_S, double* D, int ldd) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gram_dist, dim3((N + 63) / 64, (N + 3) / 4), dim3(kBlock), 0, st, S, N, (size_t)lds_S, D, (size_t)ldd);
    return hipGetLastError();
}

}  // namespace dsq
