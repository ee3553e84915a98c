// dsq_ql.h — quasi-likelihood F-test of a contrast or a nested (reduced) design: edgeR's glmQLFit / glmQLFTest (Lund et
// al. 2012), DESIGN.md 6n.
//
// Both models are fitted at the TREND dispersion (r = 1 / alpha_trend).  Per gene
//     num = D_reduced - D_full = 2 sum_n [ y (eta_f - eta_r) - (y + r) log((r + mu_f) / (r + mu_r)) ]
// - the statistic of dsq_lrt.h, operation for operation, never a difference of two deviances - and the full model's
// residual deviance D_f = sum_n d(y, mu_f) with the NB unit deviance
//     d = 2 [ y log(y / mu) - (y + r) log((y + r) / (mu + r)) ]   (y > 0),        d = 2 r log1p(mu / r)   (y = 0),
// mu = sf exp(X beta) unthresholded.  s2 = D_f / (N - P) is the gene's quasi-likelihood dispersion; the host moderates it
// across genes (limma's squeezeVar, pydeseq2_amd/ql.py) and ql_score turns num and the moderated s2 into F and its
// p-value: the F distribution's survival function f_sf below, or chisq_sf when the prior degrees of freedom are infinite.
//
// Written once and compiled twice (DeviceWave in dsq_k_ql.hip, a host policy in tests/hostql).  As in dsq_lrt.h every
// floating-point operation of the sample loop is a single IEEE operation or an explicit fma, the logarithms go through
// flog1p_t and the exponential through fexp_t: a host instantiation that walks the 64 lanes and adds them in the
// butterfly's order reproduces num, D_f and s2 bit for bit (tests/hostql, tests/test_gpu_ql.py) - PROVIDED the device unit
// is compiled without contraction, as the host build is: under -ffp-contract=fast the backend fuses a product into a
// neighbouring sum or even into the addend of a written fma (p + fma(k, c, q * w) becomes fma(k, c, fma(q, w, p)) in
// flog1p_t; y - sf * e here), one rounding fewer than the host's.  The Makefile builds k_ql_dev with -ffp-contract=off.
#pragma once
#include "dsq_lrt.h"

namespace dsq {

constexpr int kQlBetaMaxIter = 200;  // hard cap of f_sf's continued fraction (most seen in any probe: 60)

namespace detail {
// log(hi / lo) = log1p(diff / lo) >= 0 for hi >= lo > 0 and diff = hi - lo (the caller has the difference without the
// rounding of hi and lo where it can): exactly 0 for diff = 0, no rounding of a quotient near 1.
DSQ_HD double ql_log_ratio(double diff, double lo, double hi) {
    const double u = diff / lo;
    if (u < 1e300) return flog1p_t(u, lo / hi);
    DSQ_NO_SPECULATE;  // a vanished or overflowed mean, NaN: whatever the library makes of it
    return log1p(u);
}
}  // namespace detail

// acc + HALF the NB unit deviance of a count yy with mean mu and size r;  amu = mu + r as the caller rounded it.
//   y > 0:  y log(y / mu) - (y + r) log((y + r) / (mu + r)),  both logarithms as +-log1p(|y - mu| / lo): (y + r) - (mu + r)
//           is y - mu, taken before r is added, so the second ratio keeps its accuracy when r is large (1e8: Poisson);
//   y = 0:  r log1p(mu / r).
// y = mu gives exactly acc.
DSQ_HD double nb_unit_deviance(double acc, double yy, double mu, double amu, double r) {
    if (yy > 0.0) {
        const double ay = yy + r;
        const bool up = yy >= mu;
        const double diff = up ? yy - mu : mu - yy;
        const double l1 = detail::ql_log_ratio(diff, up ? mu : yy, up ? yy : mu);
        const double l2 = detail::ql_log_ratio(diff, up ? amu : ay, up ? ay : amu);
        acc = fma(yy, up ? l1 : -l1, acc);
        acc = fma(-ay, up ? l2 : -l2, acc);
    } else {
        acc = fma(r, detail::ql_log_ratio(mu, r, amu), acc);
    }
    return acc;
}

struct QlLane {
    double num, dev;  // halves of the lane's share of D_r - D_f and of D_f
};

// One lane's share (samples lane, lane + W, ...) of both sums in one sweep; eta_f and mu_f are shared.  The num part is
// lrt_lane_sum of dsq_lrt.h operation for operation (tests/test_ql_host.py holds the two to the same bits).
template <class Wv>
DSQ_HD QlLane ql_lane_sums(const int32_t* y, const double* sf, const double* Xf, int ldf, int Pf, const double* Xr,
                           int ldr, int Pr, const double* bf, const double* br, double r, int N) {
    QlLane a{0.0, 0.0};
    for (int n = Wv::lane(); n < N; n += Wv::W) {
        double ef = 0.0, er = 0.0;
        for (int j = 0; j < Pf; ++j) ef = fma(Xf[(size_t)j * ldf + n], bf[j], ef);
        for (int j = 0; j < Pr; ++j) er = fma(Xr[(size_t)j * ldr + n], br[j], er);
        const double s = sf[n], yy = (double)y[n];
        const double xf = fexp_t(ef);
        const double af = fma(s, xf, r), ar = fma(s, fexp_t(er), r);
        const bool up = af >= ar;
        const double hi = up ? af : ar, lo = up ? ar : af;
        const double u = (hi - lo) / lo;
        double lg;
        if (u < 1e300) {
            lg = flog1p_t(u, lo / hi);
        } else {
            DSQ_NO_SPECULATE;
            lg = log1p(u);
        }
        a.num = fma(yy, ef - er, a.num);
        a.num = fma(-(yy + r), up ? lg : -lg, a.num);
        a.dev = nb_unit_deviance(a.dev, yy, s * xf, af, r);
    }
    return a;
}

struct QlOut {
    double num, dev, s2;
};

template <class Wv>
DSQ_HD QlOut ql_gene(const int32_t* y, const double* sf, const double* Xf, int ldf, int Pf, const double* Xr, int ldr,
                     int Pr, const double* bf, const double* br, double disp, int N, double df) {
    const QlLane a = ql_lane_sums<Wv>(y, sf, Xf, ldf, Pf, Xr, ldr, Pr, bf, br, 1.0 / disp, N);
    QlOut o;
    o.num = 2.0 * Wv::sum(a.num);
    o.dev = 2.0 * Wv::sum(a.dev);
    o.s2 = o.dev / df;
    return o;
}

namespace detail {
// b0 + a1 / (b1 + a2 / (b2 + ...)) with  I_x(a, b) = x^a y^b / (B(a, b) * this),  y = 1 - x given separately: the even
// part of the classical continued fraction of the incomplete beta function (DiDonato & Morris 1992, the fraction of
// their BFRAC), by the modified Lentz algorithm.  Converges for x < (a + 1) / (a + b + 2).  Its coefficients hold a only
// in quotients near 1 and in lambda = a y - b x: nothing cancels at the scale of a (the classical form's 1 + d_k lose
// a * eps: 3e-10 at a = 1.5e7), so the fraction is as accurate at 1e8 denominator degrees of freedom as at 10.
DSQ_HD double ql_beta_cf(double a, double b, double x, double y) {
    constexpr double tiny = 1e-300;
    const double lam1 = a * y - b * x + 1.0;
    double f = a * lam1 / (a + 1.0);
    if (fabs(f) < tiny) f = tiny;
    double C = f, D = 0.0;
    for (int m = 1; m <= kQlBetaMaxIter; ++m) {
        const double dm = (double)m;
        const double q = a + 2.0 * dm - 1.0;
        const double w = dm * (b - dm) * x;
        const double aN = ((a + dm - 1.0) / q) * ((a + b + dm - 1.0) / q) * w * x;
        const double bN = dm + w / q + (a + dm) * (lam1 + dm * (1.0 + y)) / (q + 2.0);
        D = bN + aN * D;
        if (fabs(D) < tiny) D = tiny;
        C = bN + aN / C;
        if (fabs(C) < tiny) C = tiny;
        D = 1.0 / D;
        const double del = C * D;
        f *= del;
        if (fabs(del - 1.0) <= 2.0 * kEps) break;
    }
    return f;
}

// log( x^a y^b / B(a, b) ), written for g = max(a, b), s = min(a, b) and their variables zg, zs (zg^g zs^s): the test has
// a = d2 / 2 anywhere up to 5e7 and b = d1 / 2 <= 63.5, either may be the larger.
//   - g log zg is g log1p(-zs) when zs < 1/2 (and likewise for zs): the logarithm of a number near 1 is never taken.
//   - From g = 10 upward - where stirling_tail's series is below 4e-17, the threshold of lgamma_digamma -
//         lgamma(g + s) - lgamma(g) = (g - 1/2) log1p(s / g) - s + s log(g + s) + corr(g + s) - corr(g)
//     is a stable difference (the two lgammas are ~g log g each, their difference only ~s log g), and s log(g + s) joins
//     s log zs as s log((g + s) zs), a logarithm of a moderate number.
//   - From s = 10 upward lgamma(s) is taken by Stirling's formula as well: its s log s joins that logarithm, which is
//     then log((g + s) zs / s) - zero at F = 1 -, and its s cancels the -s above in the formula, not in the arithmetic.
//   - Below g = 10 the three lgammas are small and taken as such.
DSQ_HD double ql_log_beta_power(double a, double b, double x, double y) {
    const bool abig = a >= b;
    const double g = abig ? a : b, s = abig ? b : a;
    const double zg = abig ? x : y, zs = abig ? y : x;
    const double lg = zs < 0.5 ? log1p(-zs) : log(zg);
    if (g < 10.0) {
        const double ls = zg < 0.5 ? log1p(-zg) : log(zs);
        return g * lg + s * ls + (lgamma(g + s) - lgamma(g) - lgamma(s));
    }
    const double corr = stirling_tail(1.0 / (g + s)) - stirling_tail(1.0 / g);
    const double grow = (g - 0.5) * log1p(s / g);
    if (s < 10.0) return g * lg + s * log((g + s) * zs) + (grow - s + corr) - lgamma(s);
    return g * lg + s * log((g + s) * zs / s) + grow + (0.5 * log(s) - kHalfLog2Pi + (corr - stirling_tail(1.0 / s)));
}
}  // namespace detail

// Survival function of the F distribution with d1 (an integer, 1 ... 127) and d2 (real, > 0, up to ~1e8) degrees of
// freedom (scipy.stats.f.sf):  p = I_x(d2 / 2, d1 / 2),  x = d2 / (d2 + d1 F),  y = 1 - x = d1 F / (d2 + d1 F), both
// formed as quotients.  Left of (a + 1) / (a + b + 2) the continued fraction of I_x(a, b) converges; right of it the one
// of I_y(b, a), and p = 1 - I_y(b, a) >= ~0.2 loses nothing.  F <= 0: 1; NaN (either argument): NaN.
// Relative error c eps (1 + |ln p|) down to p = 1e-300, c measured against 400-digit arithmetic: DESIGN.md 7.
DSQ_HD double f_sf(double F, int d1, double d2) {
    if (F != F) return F;
    if (d2 != d2) return d2;
    if (!(F > 0.0)) return 1.0;
    const double a = 0.5 * d2, b = 0.5 * (double)d1;
    const double t = (double)d1 * F, den = d2 + t;
    if (!(den < 1.79769313486231570815e308)) return 0.0;  // F = inf (or d1 F overflowed)
    const double x = d2 / den, y = t / den;
    const double L = detail::ql_log_beta_power(a, b, x, y);
    if ((a + b + 2.0) * y > b + 1.0) return exp(L) / detail::ql_beta_cf(a, b, x, y);
    return 1.0 - exp(L) / detail::ql_beta_cf(b, a, y, x);
}

struct QlScore {
    double F, p;
};

// F = max(num, 0) / (df_test * s2_post) and its p-value on (df_test, df_total) degrees of freedom; df_total = inf: F's
// limit, chisq_sf(df_test F, df_test).  The caller passes infinity when the moderation found no gene-specific variability
// (df0 = inf) - not squeeze_var's capped n_used df, which bounds a finite df0 + df (ql.score_df).  NaN in, NaN out.
DSQ_HD QlScore ql_score(double num, double s2_post, int df_test, double df_total) {
    QlScore o;
    const double top = (num != num) ? num : (num > 0.0 ? num : 0.0);
    o.F = top / ((double)df_test * s2_post);
    if (o.F != o.F) {
        o.p = o.F;
    } else if (df_total < 1.79769313486231570815e308) {
        o.p = f_sf(o.F, df_test, df_total);
    } else {
        o.p = chisq_sf((double)df_test * o.F, df_test);
    }
    return o;
}

}  // namespace dsq
