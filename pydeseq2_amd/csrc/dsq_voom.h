// dsq_voom.h — limma-voom (Law et al. 2014): the two per-gene sweeps over the count matrix.
//   voom_fit1_row   E_n = log2((y_n + 0.5) / (L_n + 1) 1e6), unweighted least squares beta1 = pinv(X) E (no solve), the
//                   residual standard deviation sigma1 and the mean Abar of E: the points of the mean-variance trend
//   voom_wls_row    per sample lambda_n = x_n beta1 + log2(L_n + 1) - log2(1e6), the precision weight w_n = f(lambda_n)^-4
//                   from the trend's knot table (piecewise linear, constant outside), then weighted least squares:
//                   X^T W X (matrix cores, dsq_wide.h) and X^T W E per 64-sample chunk, Cholesky, beta; a SECOND sweep for
//                   sigma2 = sum w (E - x beta)^2 / (N - P) (never E^T W E - beta^T X^T W E); (X^T W X)^-1; per contrast c
//                   est = c . beta and the exact unscaled standard deviation u = sqrt(c^T (X^T W X)^-1 c).
// The library size enters as off_n = log2(L_n + 1) - log2(1e6), computed once by the caller: E_n = log2(y_n + 0.5) - off_n.
// One gene per wavefront; templates over the wave policy (dsq_wave.h): tests/hostvoom runs the same code on the host.
//
// Every sum over the samples keeps ONE order (as dsq_proj.h): lane l takes n = l, l + 64, ... ascending, the 64 lanes are
// added as the butterfly of DeviceWave::sum adds them; a host policy walks the 64 partial sums itself (voom_sums).  With
// the logarithm through flog_t and every multiply-add written as an fma, voom_fit1_row and the per-sample part of
// voom_wls_row (E, lambda, w) have the same bits on the host and on the device - PROVIDED the device unit is compiled
// without contraction (the Makefile builds dsq_k_voom.hip with -ffp-contract=off, DESIGN.md 6n "Bits").  The Gram matrix
// of the device runs through the matrix cores in another order of additions: beta, sigma2, est and u agree within a bound
// (DESIGN.md 7h), not to the bit.  No atomics.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dsq_wide.h"

namespace dsq {

constexpr int kVoomMaxKnots = 256;  // capacity of the knot table (at delta = 1 % of the range lowess leaves <= 202 anchors)
constexpr double kVoomLog2e = 1.44269504088896340736;

// log2((y + 0.5) / (L + 1) 1e6) with off = log2(L + 1) - log2(1e6)
DSQ_HD double voom_logcpm(int32_t y, double off) { return fma(flog_t((double)y + 0.5), kVoomLog2e, -off); }

// the trend at lam: linear between the knots (kx strictly increasing, nk >= 2), the end values outside; exactly kf[i] on a
// knot.  At most 8 halvings for 256 knots.  NaN in, NaN out.
DSQ_HD double voom_lookup(const double* kx, const double* kf, int nk, double lam) {
    if (lam <= kx[0]) return kf[0];
    if (lam >= kx[nk - 1]) return kf[nk - 1];
    int lo = 0, hi = nk - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kx[mid] <= lam) lo = mid;
        else hi = mid;
    }
    const double t = (lam - kx[lo]) / (kx[hi] - kx[lo]);
    return fma(t, kf[hi] - kf[lo], kf[lo]);
}

// f^-4: the trend is sqrt(standard deviation)
DSQ_HD double voom_weight(double f) {
    const double f2 = f * f;
    return 1.0 / (f2 * f2);
}

// K sums over the samples in the fixed order; term(n, acc) adds sample n to the K running sums of its lane
template <class Wv, int K, class F>
DSQ_HD void voom_sums(int N, double (&out)[K], F term) {
    if constexpr (Wv::W == 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = 0.0;
        for (int n = Wv::lane(); n < N; n += 64) term(n, out);
        Wv::sum_n(out);
    } else {  // the host: the 64 partial sums and the butterfly's additions, by hand
        double p[K][64];
        for (int l = 0; l < 64; ++l) {
            double a[K];
            for (int k = 0; k < K; ++k) a[k] = 0.0;
            for (int n = l; n < N; n += 64) term(n, a);
            for (int k = 0; k < K; ++k) p[k][l] = a[k];
        }
        for (int k = 0; k < K; ++k) {
            for (int s = 32; s >= 1; s >>= 1)
                for (int l = 0; l < s; ++l) p[k][l] += p[k][l + s];
            out[k] = p[k][0];
        }
    }
}

// ------------------------------------------------------------------ first fit
// JB coefficients beta1_{j0 .. j0 + JB - 1}: one pass over the row (the logarithm is taken again in every pass)
template <class Wv, int JB>
DSQ_HD void voom_fit1_coef(const int32_t* y, const double* off, const double* pinvXt, size_t ldx, int& j0, int N,
                           double* coef) {
    double a[JB];
    voom_sums<Wv, JB>(N, a, [&](int n, double (&acc)[JB]) {
        const double E = voom_logcpm(y[n], off[n]);
#pragma unroll
        for (int k = 0; k < JB; ++k) acc[k] = fma(pinvXt[(size_t)(j0 + k) * ldx + n], E, acc[k]);
    });
    if (Wv::lane() == 0) {
#pragma unroll
        for (int k = 0; k < JB; ++k) coef[j0 + k] = a[k];
    }
    j0 += JB;
}

struct VoomFit1 {
    double amean, sigma;
};

// coef: P doubles of wave-private memory, the gene's beta1 on return.  A gene without counts: NaN everywhere.
template <class Wv>
DSQ_HD VoomFit1 voom_fit1_row(const int32_t* y, const double* off, const double* Xt, const double* pinvXt, size_t ldx,
                              int P, int N, double* coef) {
    bool some = false;
    for (int n = Wv::lane(); n < N; n += Wv::W) some = some || y[n] != 0;
    VoomFit1 o;
    if (!Wv::any(some)) {
        const double nan = __builtin_nan("");
        for (int j = Wv::lane(); j < P; j += Wv::W) coef[j] = nan;
        Wv::sync();
        o.amean = nan;
        o.sigma = nan;
        return o;
    }
    int j = 0;
    while (j + 8 <= P) voom_fit1_coef<Wv, 8>(y, off, pinvXt, ldx, j, N, coef);
    if (P - j >= 4) voom_fit1_coef<Wv, 4>(y, off, pinvXt, ldx, j, N, coef);
    if (P - j >= 2) voom_fit1_coef<Wv, 2>(y, off, pinvXt, ldx, j, N, coef);
    if (P - j >= 1) voom_fit1_coef<Wv, 1>(y, off, pinvXt, ldx, j, N, coef);
    Wv::sync();  // lane 0's coefficients -> every lane
    double s[2];
    voom_sums<Wv, 2>(N, s, [&](int n, double (&acc)[2]) {
        const double E = voom_logcpm(y[n], off[n]);
        double fit = 0.0;
        for (int k = 0; k < P; ++k) fit = fma(Xt[(size_t)k * ldx + n], coef[k], fit);
        const double r = E - fit;
        acc[0] = fma(r, r, acc[0]);
        acc[1] = acc[1] + E;
    });
    o.sigma = sqrt(s[0] / (double)(N - P));
    o.amean = s[1] / (double)N;
    return o;
}

// ------------------------------------------------------------------ weighted fit
// On entry W.v(2) = beta1 (no NaN: the caller has dealt with the genes without counts); on return W.v(0) = beta, W.inv =
// (X^T W X)^-1.  vec slots: 0 beta, 1 right-hand side, 2 beta1.  The lane for which `writer` holds stores est[K], u[K].
// E_out / w_out: the gene's rows of the two layers, or both null.  Returns sigma2.
template <class Wv, int MP>
DSQ_HD double voom_wls_row(const int32_t* y, const double* off, const double* Xt, int ldx, int N, const WideWorkT<MP>& W,
                           const double* kx, const double* kf, int nk, const double* contrasts, int K, bool writer,
                           double* est, double* u, double* E_out, double* w_out) {
    const int P = W.P, ld = W.ld;
    const double* b1 = W.v(2);
    WideGram<Wv, false, MP> gram;
    gram.begin(W);
    wide_zero_pad_rows<Wv>(W);
    double rpart = 0.0;  // device: lane j < P: (X^T W E)_j
#if !defined(__HIP_DEVICE_COMPILE__)
    for (int j = 0; j < P; ++j) W.v(1)[j] = 0.0;
#endif
    Wv::sync();
    const int n_end = ((N + 63) / 64) * 64;
    for (int n0 = 0; n0 < n_end; n0 += 64) {
        wide_stage_x<Wv>(W, Xt, ldx, N, n0);
        Wv::sync();
        for (int l = Wv::lane(); l < 64; l += Wv::W) {  // device: one iteration, lane = sample of the chunk
            const int n = n0 + l;
            double w = 0.0, wE = 0.0;
            if (n < N) {
                const double E = voom_logcpm(y[n], off[n]);
                double fit = 0.0;
                for (int j = 0; j < P; ++j) fit = fma(W.xs[j * kWideXsLd + l], b1[j], fit);
                w = voom_weight(voom_lookup(kx, kf, nk, fit + off[n]));
                wE = w * E;
                if (E_out != nullptr) {
                    E_out[n] = E;
                    w_out[n] = w;
                }
            }
            W.w[l] = w;
            W.w[64 + l] = wE;
        }
        Wv::sync();
        gram.add_chunk(W);
#if defined(__HIP_DEVICE_COMPILE__)
        const int j = threadIdx.x & 63;
        if (j < P)
            for (int n = 0; n < 64; ++n) rpart += W.xs[j * kWideXsLd + n] * W.w[64 + n];
#else
        for (int j = 0; j < P; ++j)
            for (int n = 0; n < 64; ++n) W.v(1)[j] += W.xs[j * kWideXsLd + n] * W.w[64 + n];
#endif
        Wv::sync();
    }
    gram.finish(W);
#if defined(__HIP_DEVICE_COMPILE__)
    if ((int)(threadIdx.x & 63) < P) W.v(1)[threadIdx.x & 63] = rpart;
#endif
    Wv::sync();
    wide_chol<Wv>(W, W.M, W.L, 0.0);
    wide_chol_solve<Wv>(W, W.L, W.v(1));
    for (int j = Wv::lane(); j < P; j += Wv::W) W.v(0)[j] = W.v(1)[j];
    Wv::sync();
    const double* b = W.v(0);
    double s[1];
    voom_sums<Wv, 1>(N, s, [&](int n, double (&acc)[1]) {  // the second sweep: the residuals themselves
        const double E = voom_logcpm(y[n], off[n]);
        double fit1 = 0.0, fit = 0.0;
        for (int j = 0; j < P; ++j) {
            const double x = Xt[(size_t)j * ldx + n];
            fit1 = fma(x, b1[j], fit1);
            fit = fma(x, b[j], fit);
        }
        const double w = voom_weight(voom_lookup(kx, kf, nk, fit1 + off[n]));
        const double r = E - fit;
        acc[0] = fma(w * r, r, acc[0]);
    });
    wide_inverse<Wv>(W, W.L, W.Li, W.inv);
    for (int k = 0; k < K; ++k) {
        const double* c = contrasts + (size_t)k * P;
        double e = 0.0;
        for (int j = 0; j < P; ++j) e = fma(c[j], b[j], e);
        double q = 0.0;
        for (int i = Wv::lane(); i < P; i += Wv::W) {
            double r = 0.0;
            for (int j = 0; j < P; ++j) r = fma(W.inv[i * ld + j], c[j], r);
            q = fma(c[i], r, q);
        }
        q = Wv::sum(q);
        if (writer) {
            est[k] = e;
            u[k] = sqrt(q);
        }
    }
    return s[0] / (double)(N - P);
}

}  // namespace dsq
