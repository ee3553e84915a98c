// hostrank.cpp — TEST-ONLY host instantiation of the rank-sum templates (dsq_rank.h).
// Built by tests/hostrank/build.py with g++ and -ffp-contract=off into tests/hostrank/_hostrank.so, loaded only by tests.
//
// hr_ranksum walks the genes and comparisons as k_ranksum does, one "wave" of one lane (HostWave) per gene; the sorter
// pads a stratum's segment to the next power of two with NaN as LdsSorter does, so a layout whose pads are too small
// writes outside its row here as it would on the device (the row is allocated with exactly pad[S] doubles).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "dsq_rank.h"

using namespace dsq;

namespace {
struct HostSorter {
    int operator()(double* buf, int n) const {
        const int L = rank_pow2(n);
        for (int k = n; k < L; ++k) buf[k] = NAN;
        std::sort(buf, buf + n, [](double a, double b) { return (a < b) || (a == a && b != b); });  // NaNs last
        return L;
    }
};
}  // namespace

extern "C" {

int hr_plan(int L, int* waves, size_t* lds_bytes) {
    const RankPlan p = rank_plan(L);
    *waves = p.waves;
    *lds_bytes = p.lds_bytes;
    return p.waves > 0 ? 0 : -2;
}

// 0: fine; otherwise -2 and *why = the launcher's message
int hr_check_layout(const int32_t* order, const int32_t* seg, const int32_t* pad, int S, int cap_strata, int cap_order, int N,
                    const char** why) {
    *why = rank_check_layout(order, seg, pad, S, cap_strata, cap_order, N);
    return *why == nullptr ? 0 : -2;
}

int hr_ranksum(const int32_t* y, int ldn, const double* sf, int N, int G, int K, const int32_t* order, int ldo,
               const int32_t* seg, const int32_t* pad, int lds, const int32_t* nstrata, const int8_t* labels, int ldl,
               int alt, double* stat, double* pvalue, double* usum, double* ties, int ldg) {
    if (N < 2 || G < 0 || K < 1 || ldn < N || ldl < N || ldo < 1 || lds < 2 || ldg < G) return -2;
    if (!(alt == 0 || alt == 3 || alt == 4)) return -2;
    for (int k = 0; k < K; ++k)
        if (rank_check_layout(order + (size_t)k * ldo, seg + (size_t)k * lds, pad + (size_t)k * lds, nstrata[k], lds - 1,
                              ldo, N) != nullptr)
            return -2;
    for (int k = 0; k < K; ++k) {
        const RankLayout Q{order + (size_t)k * ldo, seg + (size_t)k * lds, pad + (size_t)k * lds, nstrata[k],
                           labels + (size_t)k * ldl};
        std::vector<double> row((size_t)Q.pad[Q.S]);
        for (int g = 0; g < G; ++g) {
            std::fill(row.begin(), row.end(), -7.0);
            const RankOut o = ranksum_gene<HostWave>(y + (size_t)g * ldn, sf, Q, alt, row.data(), HostSorter());
            const size_t at = (size_t)k * ldg + g;
            stat[at] = o.stat; pvalue[at] = o.pvalue; usum[at] = o.usum; ties[at] = o.ties;
        }
    }
    return 0;
}

}  // extern "C"
