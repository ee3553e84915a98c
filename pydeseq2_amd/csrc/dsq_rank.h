// dsq_rank.h — Wilcoxon rank-sum test (Mann-Whitney, stratified: van Elteren) of one comparison on one gene's normalised
// counts.  One gene per wavefront, as the trimmed statistics of dsq_stats.h: the used samples' values
// v = (double)y / sf are staged stratum by stratum in a wave-private LDS segment and each stratum is sorted in place by the
// `Sorter` (device: LdsSorter, dsq_lds_sort.h).  Nothing is sorted along with the values: the midrank of a tested sample
// is lower / upper bound of its recomputed value in its stratum's sorted segment, the tie term one pass over the starts of
// the tie runs.  Rank sums are half-integers and tie terms integers below 2^53: every order of summation gives the same
// bits.  No atomics.  Templates over the wave policy (dsq_wave.h): tests/hostrank runs the same code on the host.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dsq_wave.h"

namespace dsq {

constexpr int kRankMaxL = 16384;            // LDS doubles per gene: 128 KiB of the 160 KiB of a workgroup (DSQ_RANK_MAX_L)
constexpr int kRankLdsBytes = 160 * 1024;   // what a workgroup of gfx950 may allocate

// ---- launch plan: a pure function of L = the padded row length (the sum over the strata of next_pow2(N_s))
struct RankPlan {
    int waves;         // wavefronts (= genes) per workgroup; 0: L is refused
    size_t lds_bytes;  // dynamic LDS of the workgroup
};
DSQ_HD RankPlan rank_plan(int L) {
    RankPlan p{0, 0};
    if (L < 1 || L > kRankMaxL) return p;
    const size_t per = (size_t)L * sizeof(double);
    p.waves = 4 * per <= (size_t)kRankLdsBytes ? 4 : (2 * per <= (size_t)kRankLdsBytes ? 2 : 1);
    p.lds_bytes = per * (size_t)p.waves;
    return p;
}

DSQ_HD int rank_pow2(int n) {
    int L = 1;
    while (L < n) L <<= 1;
    return L;
}

// ---- one comparison's layout.  order[seg[s] .. seg[s+1]): the sample indices of stratum s (used samples only, tested and
// reference in any order); pad[s]: where the stratum's segment starts in the gene's LDS row, pad[s+1] - pad[s] =
// next_pow2(N_s); label[n]: 1 tested, 0 reference (samples that are left out are not in `order`)
struct RankLayout {
    const int32_t* order;
    const int32_t* seg;
    const int32_t* pad;
    int S;
    const int8_t* label;
};

// the layout as the launcher must find it before a kernel may index with it (host arrays); nullptr: fine
inline const char* rank_check_layout(const int32_t* order, const int32_t* seg, const int32_t* pad, int S, int cap_strata,
                                     int cap_order, int N) {
    if (S < 1 || S > cap_strata) return "n_strata: between 1 and lds - 1 strata per comparison";
    if (seg[0] != 0 || pad[0] != 0) return "seg / pad: the first offset of a comparison is 0";
    for (int s = 0; s < S; ++s) {
        const int n = seg[s + 1] - seg[s];
        if (n < 1) return "seg: every stratum holds at least one sample";
        if (seg[s + 1] > cap_order || seg[s + 1] > N) return "seg: more used samples than ldo or N";
        if (pad[s + 1] - pad[s] != rank_pow2(n)) return "pad: the prefix sums of next_pow2(N_s)";
        if (pad[s + 1] > kRankMaxL)
            return "the padded row (sum of next_pow2(N_s)) is longer than DSQ_RANK_MAX_L = 16384 doubles";
    }
    for (int i = 0; i < seg[S]; ++i)
        if (order[i] < 0 || order[i] >= N) return "order: a sample index outside 0 ... N - 1";
    return nullptr;
}

struct RankOut {
    double stat, pvalue, usum, ties;
};

// IEEE division: the orderings and the ties of the test are those of these quotients (the fast reciprocal of dsq_math.h
// is one ulp off here and there, which would split or merge ties)
DSQ_HD double rank_value(int32_t y, double sf) { return (double)y / sf; }

// number of buf[0 .. n) below v
DSQ_HD int rank_lower(const double* buf, int n, double v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (buf[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first index in [lo, n) whose value is above v (n: none)
DSQ_HD int rank_upper(const double* buf, int lo, int n, double v) {
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (buf[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// alt: dsq_alt's codes - 0 two-sided, 3 "greater", 4 "less".  buf: the gene's LDS row, pad[S] doubles.
template <class Wv, class Sorter>
DSQ_HD RankOut ranksum_gene(const int32_t* y, const double* sf, const RankLayout& Q, int alt, double* buf, Sorter&& sorter) {
    const bool single = Q.S == 1;
    double W = 0.0, V = 0.0, usum = 0.0, ties = 0.0;
    for (int s = 0; s < Q.S; ++s) {
        const int b = Q.seg[s], n = Q.seg[s + 1] - b;
        double* row = buf + Q.pad[s];
        for (int i = Wv::lane(); i < n; i += Wv::W) {
            const int idx = Q.order[b + i];
            row[i] = rank_value(y[idx], sf[idx]);
        }
        sorter(row, n);  // (synchronises the wave before it reads and after it has written)
        double r = 0.0, t = 0.0;
        int n1 = 0;
        for (int i = Wv::lane(); i < n; i += Wv::W) {
            const int idx = Q.order[b + i];
            if (Q.label[idx] == 1) {  // midrank of a tested sample: the values below it, and half of its tie run + 1
                const double v = rank_value(y[idx], sf[idx]);
                const int lo = rank_lower(row, n, v);
                const int hi = rank_upper(row, lo, n, v);
                r += (double)lo + 0.5 * (double)(hi - lo + 1);
                n1 += 1;
            }
            // element i of the sorted row starts a tie run of t >= 2 values: t^3 - t
            if (i + 1 < n && row[i] == row[i + 1] && (i == 0 || row[i - 1] != row[i])) {
                const double tt = (double)(rank_upper(row, i + 1, n, row[i]) - i);
                t += tt * (tt * tt - 1.0);
            }
        }
        r = Wv::sum(r);
        t = Wv::sum(t);
        n1 = Wv::sumi(n1);
        const int n2 = n - n1;
        if (n1 == 0 || n2 == 0 || n < 2) continue;  // a stratum with one group only says nothing
        const double dn = (double)n, p = (double)n1 * (double)n2;
        const double U = r - 0.5 * ((double)n1 * (double)(n1 + 1));
        usum += U;
        ties += t;
        const double D = U - 0.5 * p;                 // exact (half-integers)
        const double B = (dn * dn * dn - dn) - t;     // exact (integers below 2^53)
        const double Vs = (p * B) / (12.0 * dn * (dn - 1.0));
        if (single) {
            W += D;
            V += Vs;
        } else {  // van Elteren's weights
            const double w = 1.0 / (dn + 1.0);
            W += w * D;
            V += (w * w) * Vs;
        }
    }
    RankOut o;
    o.usum = usum;
    o.ties = ties;
    if (!(V > 0.0)) {
        o.stat = 0.0;
        o.pvalue = 1.0;
        return o;
    }
    const double sd = sqrt(V), c = single ? 0.5 : 0.0;  // continuity correction: the plain test only
    if (alt == 3) {
        o.stat = (W - c) / sd;
        o.pvalue = norm_sf(o.stat);
    } else if (alt == 4) {
        o.stat = (W + c) / sd;
        o.pvalue = norm_sf(-o.stat);
    } else {
        const double z = dmax(fabs(W) - c, 0.0) / sd;
        o.stat = dsign(W) * z;
        o.pvalue = dmin(1.0, 2.0 * norm_sf(z));
    }
    return o;
}

}  // namespace dsq
