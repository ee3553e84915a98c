// dsq_lrt.h — likelihood-ratio test of a nested (reduced) design: DESeq2's nbinomLRT.
//
// Both models are fitted with the FINAL dispersions; per gene
//     stat = 2 (l_full - l_reduced)
//          = 2 sum_n [ y (eta_f - eta_r) - (y + r) (log(r + mu_f) - log(r + mu_r)) ],   r = 1 / alpha,
// mu = sf exp(X beta) unthresholded as the reference's solver returns it (utils.py:435-437).  The lgamma and alpha-only
// terms of utils.nb_nll (utils.py:216-234) are those of the other model and cancel analytically: the statistic is never
// formed as the difference of two likelihoods of 1e3 - 1e4.  pvalue = Q(df / 2, stat / 2), df = P_full - P_reduced.
//
// Written once and compiled twice like the other per-gene routines (DeviceWave in dsq_k_lrt.hip, a host policy in
// tests/hostlrt).  Every floating-point operation of the sample loop is either a single IEEE operation or an explicit
// fma, and the logarithm goes through flog1p_t and the exponential through fexp_t (explicit fmas only): the compiler's
// contraction setting cannot change a bit, so a host instantiation that walks the 64 lanes and adds them in the
// butterfly's order reproduces the device's statistic exactly (tests/hostlrt, tests/test_gpu_lrt.py).
#pragma once
#include "dsq_wave.h"

namespace dsq {

constexpr int kLrtMaxCoef = 255;  // P_full + P_reduced <= 128 + 127: both coefficient vectors of a gene

// Survival function of the chi-square distribution with an INTEGER number of degrees of freedom, Q(df / 2, x / 2)
// (scipy.stats.chi2.sf).  With h = x / 2 the regularised incomplete gamma function of a half-integer order is a finite
// sum of positive terms - nothing cancels:
//     df = 2 m     : e^-h sum_{j < m} h^j / j!
//     df = 2 m + 1 : erfc(sqrt h) + e^-h sum_{1 <= j <= m} h^(j - 1/2) / Gamma(j + 1/2)
// e^-h is applied as two factors e^(-h/2): the partial sum times the first stays in range, so the product is accurate
// down to the smallest normal number and no logarithm is needed where e^-h alone underflows (h > 708) while the
// p-value does not (the sum reaches e^255 at df = 127).  Beyond h = 1500 the result is below 1e-500 for every df <= 127.
// x <= 0: 1; NaN: NaN.  Relative error measured against 50-digit arithmetic: DESIGN.md 7b.
DSQ_HD double chisq_sf(double x, int df) {
    if (x != x) return x;
    if (!(x > 0.0)) return 1.0;
    const double h = 0.5 * x;
    if (h > 1500.0) return 0.0;
    const bool odd = (df & 1) != 0;
    const int m = df >> 1;  // either sum has m terms
    double lead = 0.0, t = 1.0, s = 0.0;
    if (odd) {
        const double a = sqrt(h);
        lead = erfc(a);
        t = a * 1.1283791670955125739;  // h^(1/2) / Gamma(3/2) = 2 sqrt(h / pi)
    }
    const double step = odd ? 1.5 : 1.0;  // term k + 1 = term k * h / (k + step)
    for (int k = 0; k < m; ++k) {
        s += t;
        t = t * h / ((double)k + step);
    }
    const double e = fexp_t(-0.5 * h);
    return lead + (s * e) * e;
}

// One lane's share of sum_n [ y (eta_f - eta_r) - (y + r) log((r + mu_f) / (r + mu_r)) ]: samples lane, lane + W, ...
// Xf / Xr: the transposed designs ([P][ld], one coalesced request per column and sweep); bf / br: the coefficient
// vectors (wave-private LDS on the device).
template <class Wv>
DSQ_HD double lrt_lane_sum(const int32_t* y, const double* sf, const double* Xf, int ldf, int Pf, const double* Xr,
                           int ldr, int Pr, const double* bf, const double* br, double r, int N) {
    double acc = 0.0;
    for (int n = Wv::lane(); n < N; n += Wv::W) {
        double ef = 0.0, er = 0.0;
        for (int j = 0; j < Pf; ++j) ef = fma(Xf[(size_t)j * ldf + n], bf[j], ef);
        for (int j = 0; j < Pr; ++j) er = fma(Xr[(size_t)j * ldr + n], br[j], er);
        const double s = sf[n], yy = (double)y[n];
        const double af = fma(s, fexp_t(ef), r), ar = fma(s, fexp_t(er), r);
        // log(af / ar) as +-log1p((hi - lo) / lo): exact for equal means, no rounding of a quotient near 1
        const bool up = af >= ar;
        const double hi = up ? af : ar, lo = up ? ar : af;
        const double u = (hi - lo) / lo;
        double lg;
        if (u < 1e300) {
            lg = flog1p_t(u, lo / hi);
        } else {  // a mean that overflowed, r = 0 with a vanished mean, NaN: whatever the library makes of it
            DSQ_NO_SPECULATE;
            lg = log1p(u);
        }
        acc = fma(yy, ef - er, acc);
        acc = fma(-(yy + r), up ? lg : -lg, acc);
    }
    return acc;
}

struct LrtOut {
    double stat, p;
};

template <class Wv>
DSQ_HD LrtOut lrt_gene(const int32_t* y, const double* sf, const double* Xf, int ldf, int Pf, const double* Xr, int ldr,
                       int Pr, const double* bf, const double* br, double disp, int N) {
    const double r = 1.0 / disp;
    LrtOut o;
    o.stat = 2.0 * Wv::sum(lrt_lane_sum<Wv>(y, sf, Xf, ldf, Pf, Xr, ldr, Pr, bf, br, r, N));
    o.p = chisq_sf(o.stat, Pf - Pr);  // (a negative statistic - the reduced fit ended above the full one - gives 1)
    return o;
}

}  // namespace dsq
