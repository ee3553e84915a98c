// dsq_gram.h — sample-space statistics of a transformed N x G matrix (DESeq2's plotPCA / dist):
// row means and variances per gene, the packed centred operand, the symmetric N x N Gram matrix S = X~ X~^T summed over a
// list of genes on the fp64 matrix cores, its reduction over gene slices and the Euclidean distances from it.
//
// The Gram is WideGram (dsq_wide.h) turned round: there p x p summed over the samples of one gene, here N x N summed over
// up to G genes.  One workgroup of four wavefronts owns one lower-triangle macro tile of kGramT x kGramT samples and one
// slice of the gene list; it stages chunks of kGramChunk genes of the two sample panels in LDS and accumulates 16 x 16
// fragments with v_mfma_f64_16x16x4_f64 (A = x~[sample i][4 genes], B = x~[4 genes][sample j]).  Everything that decides
// the order of the additions of an entry (slices, chunks, the four genes of a k-step) depends on N and K only - never on
// the tile the entry lies in: an entry takes its genes in list order, so S is symmetric by construction (computed once,
// mirrored), the same sample at two indices gives the same bits, and a rerun gives the same bits.  No atomics.
// The host build (tests/hostgram) runs the same plan, packing, partial layout and reduction with plain sums in the place
// of the MFMA fragments.
#pragma once
#include "dsq_wave.h"

namespace dsq {

constexpr int kGramT = 128;                  // samples per side of a macro tile
constexpr int kGramF = kGramT / 16;          // 16 x 16 fragments per side
constexpr int kGramChunk = 32;               // genes staged per chunk (eight k-steps of four)
// row stride of a staged panel xs[gene][sample]: the 32 lanes of one half of a ds_read_b64 read 16 consecutive samples of
// two consecutive genes; with the stride = 16 (mod 32) doubles they cover the 64 banks once
constexpr int kGramLd = kGramT + 16;
constexpr int kGramLdsDoubles = 2 * kGramChunk * kGramLd;
constexpr int kGramTargetBlocks = 512;       // (tile, slice) blocks the split over genes aims at
constexpr int kGramMinSliceChunks = 4;       // ... and the fewest chunks worth a slice (and a partial tile) of their own
constexpr int kGramTile2 =kGramT * kGramT;  // doubles of one partial tile in the workspace

DSQ_HD int gram_pad16(int n) { return (n + 15) & ~15; }

// The launch plan: a function of N and K alone.
//   macro tiles: t = ti (ti + 1) / 2 + tj for 0 <= tj <= ti < nt;  chunk c: genes [32 c, min(32 c + 32, K));
//   slice s: chunks [s cps, min((s + 1) cps, chunks)).
struct GramPlan {
    int N, K, pad, nt, ntiles, chunks, slices, cps;
};
DSQ_HD GramPlan gram_plan(int N, int K) {
    GramPlan p;
    p.N = N; p.K = K; p.pad = gram_pad16(N);
    p.nt = (N + kGramT - 1) / kGramT;
    p.ntiles = p.nt * (p.nt + 1) / 2;
    p.chunks = (K + kGramChunk - 1) / kGramChunk;
    int s = kGramTargetBlocks / (p.ntiles > 0 ? p.ntiles : 1);
    if (s < 1) s = 1;
    const int most = (p.chunks + kGramMinSliceChunks - 1) / kGramMinSliceChunks;
    if (s > most) s = most;
    p.cps = s > 0 ? (p.chunks + s - 1) / s : 0;
    p.slices = p.cps > 0 ? (p.chunks + p.cps - 1) / p.cps : 0;
    return p;
}
DSQ_HD void gram_tile_rc(int t, int& ti, int& tj) {
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti = i; tj = t - i * (i + 1) / 2;
}
// doubles of workspace: the packed panel [K][pad16(N)], then, with more than one slice, slices x ntiles partial tiles
DSQ_HD size_t gram_work_doubles(int N, int K) {
    const GramPlan p = gram_plan(N, K);
    return (size_t)K * (size_t)p.pad + (p.slices > 1 ? (size_t)p.slices * (size_t)p.ntiles * (size_t)kGramTile2 : 0);
}

// ------------------------------------------------------------------ row means and variances (two-pass, rowVars)
// ONE order of the sums whatever the layout and whoever runs it, so that both layouts (and the host build) give the same
// bits: 64 partial sums, partial l over the samples l, l + 64, ... in order, added as the butterfly of DeviceWave::sum
// adds the lanes of a wavefront (partners at distance 32, 16, 8, 4, 2, 1).  The squares are accumulated with an explicit
// fma, not left to the contraction setting of the build.
// Sample-major (stride ld) and the host: Q threads share a gene; thread q owns the partials l = q + Q j, j < 64 / Q, and
// adds them up to one value (the butterfly's steps at distance 32 ... Q); row_sum_join then takes the steps at distance
// Q / 2 ... 1 over the Q values.  Any Q gives the same bits (Q = 1: one lane, or the host, does it all).
// Pass 1 (sq = false) sums x, pass 2 (sq = true) sums (x - m)^2.  No branches: a partial never holds -0.0, so adding
// +0.0 (or 0 * 0) for a sample that is not there leaves its bits as they are.
template <int Q>
DSQ_HD double row_sum_part(const double* col, size_t ld, int N, double m, bool sq, int q) {
    constexpr int J = 64 / Q;
    double p[J];
#pragma unroll
    for (int j = 0; j < J; ++j) p[j] = 0.0;
    for (int n0 = 0; n0 < N; n0 += 64) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int n = n0 + q + Q * j;
            const bool there = n < N;
            const double v = col[(size_t)(there ? n : 0) * ld];
            const double d = there ? (sq ? v - m : v) : 0.0;
            p[j] = sq ? fma(d, d, p[j]) : p[j] + d;
        }
    }
#pragma unroll
    for (int s = J / 2; s >= 1; s >>= 1) {
#pragma unroll
        for (int j = 0; j < J / 2; ++j)
            if (j < s) p[j] += p[j + s];
    }
    return p[0];
}
template <int Q>
DSQ_HD double row_sum_join(double* r) {
#pragma unroll
    for (int s = Q / 2; s >= 1; s >>= 1) {
#pragma unroll
        for (int i = 0; i < Q / 2; ++i)
            if (i < s) r[i] += r[i + s];
    }
    return r[0];
}
DSQ_HD void row_meanvar_col(const double* col, size_t ld, int N, double& mean, double& var) {
    const double m = row_sum_part<1>(col, ld, N, 0.0, false, 0) / (double)N;
    mean = m;
    var = row_sum_part<1>(col, ld, N, m, true, 0) / (double)(N - 1);  // N == 1: 0 / 0 = NaN (R's NA)
}
// gene-major row: the 64 lanes of a wavefront are the 64 partial sums
template <class Wv>
DSQ_HD void row_meanvar_row(const double* row, int N, double& mean, double& var) {
    if constexpr (Wv::W != 64) {
        row_meanvar_col(row, 1, N, mean, var);
    } else {
        double s = 0.0;
        for (int n = Wv::lane(); n < N; n += 64) s += row[n];
        const double m = Wv::sum(s) / (double)N;
        double q = 0.0;
        for (int n = Wv::lane(); n < N; n += 64) q = fma(row[n] - m, row[n] - m, q);
        mean = m;
        var = Wv::sum(q) / (double)(N - 1);
    }
}

// ------------------------------------------------------------------ the canonical operand
// element (k, s) of the packed panel [K][pad16(N)]: gene sel[k] (k without a list) of sample s, centred; 0 in the padding
// layout: 0 sample-major [N][ld], 1 gene-major [G][ld]
DSQ_HD double gram_pack_value(const double* x, int layout, size_t ld, int N, const int32_t* sel, const double* mean, int k,
                              int s) {
    if (s >= N) return 0.0;
    const size_t g = sel != nullptr ? (size_t)sel[k] : (size_t)k;
    const double v = layout == 1 ? x[g * ld + (size_t)s] : x[(size_t)s * ld + g];
    return mean != nullptr ? v - mean[g] : v;
}

// ------------------------------------------------------------------ one (tile, slice) block of the Gram
// xp: the packed panel.  One slice: both triangles of S are written; several: the partial tile goes to
// part[(slice * ntiles + tile)][lr][lc] (entries of the lower triangle inside N only).
// Device: called by the 256 threads of a workgroup, lds = kGramLdsDoubles doubles of LDS.  Wave w owns the fragment rows w
// and 7 - w (nine fragments on a diagonal tile whichever the wave, sixteen elsewhere) and all eight fragment columns.
// Host: lds = kGramTile2 doubles of scratch.
template <class Wv>
DSQ_HD void gram_block(const GramPlan& P, int tile, int slice, const double* xp, double* part, double* S, size_t lds_S,
                       double* lds) {
    int ti, tj;
    gram_tile_rc(tile, ti, tj);
    const int i0 = ti * kGramT, j0 = tj * kGramT;
    const bool diag = ti == tj;
    const size_t ldp = (size_t)P.pad;
    const int na = P.pad - i0 < kGramT ? P.pad - i0 : kGramT;  // staged samples of the two panels (multiples of 16)
    const int nb = P.pad - j0 < kGramT ? P.pad - j0 : kGramT;
    const int c_begin = slice * P.cps;
    const int c_end = c_begin + P.cps < P.chunks ? c_begin + P.cps : P.chunks;
    double* out = P.slices > 1 ? part + ((size_t)slice * (size_t)P.ntiles + (size_t)tile) * (size_t)kGramTile2 : nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 15, kq = lane >> 4;
    double* xa = lds;
    double* xb = diag ? lds : lds + kGramChunk * kGramLd;
    const int rf0 = w, rf1 = kGramF - 1 - w;
    int cols = nb / 16;
    int cmax0 = 16 * rf0 < na ? cols : 0, cmax1 = 16 * rf1 < na ? cols : 0;
    if (diag) {
        cmax0 = cmax0 < rf0 + 1 ? cmax0 : rf0 + 1;
        cmax1 = cmax1 < rf1 + 1 ? cmax1 : rf1 + 1;
    }
    const bool full = cmax0 == kGramF && cmax1 == kGramF;
    d4 acc0[kGramF], acc1[kGramF];
#pragma unroll
    for (int c = 0; c < kGramF; ++c) { acc0[c] = d4{0.0, 0.0, 0.0, 0.0}; acc1[c] = d4{0.0, 0.0, 0.0, 0.0}; }
    // staging: thread (ss, gs) moves sample ss of the genes gs, gs + 2, ... of a chunk.  The next chunk is fetched into
    // registers before the current one is multiplied and stored to LDS after it, so the loads fly under the MFMAs.
    const int ss = tid & (kGramT - 1), gs = tid >> 7;
    constexpr int kStage = kGramChunk / 2;
    double ra[kStage], rb[kStage];
    const bool in_a = ss < na, in_b = !diag && ss < nb;
    auto fetch = [&](int ch) {
        const int g0 = ch * kGramChunk;
        const int kc = P.K - g0 < kGramChunk ? P.K - g0 : kGramChunk;
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int g = gs + 2 * u;  // (genes beyond the list: zeros, which fill the last k-step)
            const size_t at = (size_t)(g0 + g) * ldp;
            ra[u] = in_a && g < kc ? xp[at + (size_t)(i0 + ss)] : 0.0;
            rb[u] = in_b && g < kc ? xp[at + (size_t)(j0 + ss)] : 0.0;
        }
    };
    if (c_begin < c_end) fetch(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        const int g0 = ch * kGramChunk;
        const int kc = P.K - g0 < kGramChunk ? P.K - g0 : kGramChunk;
        const int kc4 = (kc + 3) & ~3;  // the last k-step is filled with zero genes
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
            const int g = gs + 2 * u;
            if (in_a) xa[g * kGramLd + ss] = ra[u];
            if (in_b) xb[g * kGramLd + ss] = rb[u];
        }
        __syncthreads();
        if (ch + 1 < c_end) fetch(ch + 1);
        const double* pa = xa + kq * kGramLd + r;
        const double* pb = xb + kq * kGramLd + r;
        if (full) {
            for (int k4 = 0; k4 < kc4; k4 += 4) {
                const double a0 = pa[k4 * kGramLd + 16 * rf0], a1 = pa[k4 * kGramLd + 16 * rf1];
#pragma unroll
                for (int c = 0; c < kGramF; ++c) {
                    const double b = pb[k4 * kGramLd + 16 * c];
                    acc0[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0[c], 0, 0, 0);
                    acc1[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1[c], 0, 0, 0);
                }
            }
        } else {
            // (fragment rows / columns beyond the staged samples are read as whatever the LDS holds and never used)
            for (int k4 = 0; k4 < kc4; k4 += 4) {
                const double a0 = pa[k4 * kGramLd + 16 * rf0], a1 = pa[k4 * kGramLd + 16 * rf1];
#pragma unroll
                for (int c = 0; c < kGramF; ++c) {
                    const double b = pb[k4 * kGramLd + 16 * c];
                    if (c < cmax0) acc0[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0[c], 0, 0, 0);
                    if (c < cmax1) acc1[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1[c], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < kGramF; ++c) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (c >= (h == 0 ? cmax0 : cmax1)) continue;
            const d4 v = h == 0 ? acc0[c] : acc1[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int lr = 16 * (h == 0 ? rf0 : rf1) + kq + 4 * q, lc = 16 * c + r;
                const int gi = i0 + lr, gj = j0 + lc;
                if (gi < P.N && gj < P.N && gj <= gi) {
                    if (out != nullptr) {
                        out[lr * kGramT + lc] = v[q];
                    } else {
                        S[(size_t)gi * lds_S + (size_t)gj] = v[q];
                        S[(size_t)gj * lds_S + (size_t)gi] = v[q];
                    }
                }
            }
        }
    }
#else
    (void)na; (void)nb; (void)lds;
    for (int lr = 0; lr < kGramT; ++lr)
        for (int lc = 0; lc < kGramT; ++lc) {
            const int gi = i0 + lr, gj = j0 + lc;
            if (gi >= P.N || gj >= P.N || gj > gi) continue;
            double s = 0.0;
            for (int ch = c_begin; ch < c_end; ++ch) {
                const int g0 = ch * kGramChunk;
                const int kc = P.K - g0 < kGramChunk ? P.K - g0 : kGramChunk;
                for (int g = g0; g < g0 + kc; ++g) s += xp[(size_t)g * ldp + (size_t)gi] * xp[(size_t)g * ldp + (size_t)gj];
            }
            if (out != nullptr) {
                out[lr * kGramT + lc] = s;
            } else {
                S[(size_t)gi * lds_S + (size_t)gj] = s;
                S[(size_t)gj * lds_S + (size_t)gi] = s;
            }
        }
#endif
}

// entry (i, j), i >= j, of S from the partial tiles: the slices in ascending order (no slice: 0)
DSQ_HD double gram_reduce_entry(const GramPlan& P, const double* part, int i, int j) {
    const int ti = i / kGramT, tj = j / kGramT;
    const size_t tile = (size_t)(ti * (ti + 1) / 2 + tj);
    const size_t at = (size_t)((i - ti * kGramT) * kGramT + (j - tj * kGramT));
    double s = 0.0;
#pragma unroll 8
    for (int sl = 0; sl < P.slices; ++sl) s += part[((size_t)sl * (size_t)P.ntiles + tile) * (size_t)kGramTile2 + at];
    return s;
}

// Euclidean distance of samples i and j from the Gram
DSQ_HD double gram_dist_entry(const double* S, size_t lds_S, int i, int j) {
    if (i == j) return 0.0;
    const double d2 = (S[(size_t)i * lds_S + (size_t)i] + S[(size_t)j * lds_S + (size_t)j]) - 2.0 * S[(size_t)i * lds_S + (size_t)j];
    return d2 < 0.0 ? 0.0 : sqrt(d2);  // (rounding may leave the difference of near-duplicates below 0)
}

}  // namespace dsq
