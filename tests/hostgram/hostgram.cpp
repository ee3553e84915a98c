// hostgram.cpp — TEST-ONLY host instantiation of the sample-Gram templates (dsq_gram.h).
// Built by tests/hostgram/build.py with g++ and -ffp-contract=off into tests/hostgram/_hostgram.so, loaded only by tests.
//
// hg_sample_gram composes the pieces as launch_sample_gram does: pack into the workspace, one gram_block per
// (tile, slice) of the plan, the reduction of the slices.  Only the sums inside a block differ from the device (plain sums
// in list order in the place of the MFMA fragments).
#include <cstdint>
#include <vector>

#include "dsq_gram.h"

using namespace dsq;

extern "C" {

void hg_consts(int* out) { out[0] = kGramT; out[1] = kGramChunk; out[2] = kGramLd; out[3] = kGramTargetBlocks; }

void hg_plan(int N, int K, int* out) {
    const GramPlan p = gram_plan(N, K);
    out[0] = p.pad; out[1] = p.nt; out[2] = p.ntiles; out[3] = p.chunks; out[4] = p.slices; out[5] = p.cps;
}

void hg_tile_rc(int t, int* rc) { gram_tile_rc(t, rc[0], rc[1]); }

size_t hg_work_doubles(int N, int K) { return gram_work_doubles(N, K); }

int hg_row_meanvar(const double* x, int layout, int N, int G, int ld, double* mean, double* var) {
    if (N < 1 || G < 0 || (layout != 0 && layout != 1) || ld < (layout == 1 ? N : G)) return -2;
    for (int g = 0; g < G; ++g) {
        double m, v;
        if (layout == 1) row_meanvar_row<HostWave>(x + (size_t)g * ld, N, m, v);
        else row_meanvar_col(x + g, (size_t)ld, N, m, v);
        mean[g] = m;
        if (var != nullptr) var[g] = v;
    }
    return 0;
}

int hg_sample_gram(const double* x, int layout, int N, int G, int ld, const int32_t* sel, int K, const double* mean,
                   double* work, double* S, int lds) {
    if (N < 1 || G < 0 || K < 0 || (sel == nullptr && K > G) || (layout != 0 && layout != 1) ||
        ld < (layout == 1 ? N : G) || lds < N)
        return -2;
    if (G == 0) K = 0;
    const GramPlan P = gram_plan(N, K);
    double* xp = work;
    double* part = work + (size_t)K * (size_t)P.pad;
    for (int k = 0; k < K; ++k)
        for (int s = 0; s < P.pad; ++s) xp[(size_t)k * P.pad + s] = gram_pack_value(x, layout, (size_t)ld, N, sel, mean, k, s);
    std::vector<double> scratch(kGramTile2);
    for (int sl = 0; sl < P.slices; ++sl)
        for (int t = 0; t < P.ntiles; ++t) gram_block<HostWave>(P, t, sl, xp, part, S, (size_t)lds, scratch.data());
    if (P.slices != 1)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j <= i; ++j) {
                const double v = gram_reduce_entry(P, part, i, j);
                S[(size_t)i * lds + j] = v;
                S[(size_t)j * lds + i] = v;
            }
    return 0;
}

int hg_gram_dist(const double* S, int N, int lds, double* D, int ldd) {
    if (N < 1 || lds < N || ldd < N) return -2;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) D[(size_t)i * ldd + j] = gram_dist_entry(S, (size_t)lds, i, j);
    return 0;
}

}  // extern "C"
