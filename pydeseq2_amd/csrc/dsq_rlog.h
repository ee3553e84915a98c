// dsq_rlog.h — regularized-log transformation: DESeq2's rlog() (rlogData -> fitNbinomGLMs -> fitBeta with the lambda
// ridge, betaTol 1e-4, minmu 0.5, maxit 100, useOptim = FALSE).  The reference project has none; DESIGN.md 6h is the
// statement of the algorithm, and parity with R is by construction from it, not measured.
//
// Per gene a ridge-penalised NB GLM with the design [1 | I_N]: an intercept beta0 and one coefficient b_j per sample,
// penalties lambda0 (intercept) and lambda (samples), on the natural-log scale.  X^T W X + Lambda is an arrowhead matrix
// (a dense first row / column, otherwise diagonal), so the normal equations of an IRLS iteration have a closed form.
// With w_j = mu_j / (1 + a mu_j), the working response z_j = ln(mu_j / s_j) + (y_j - mu_j) / mu_j and
//     q_j = w_j / (w_j + lambda),   A_j = w_j z_j / (w_j + lambda):
//     beta0 = (sum w z - sum w q z) / (sum w + lambda0 - sum w q) = sum A / (sum q + lambda0 / lambda),
//     b_j   = q_j (z_j - beta0)     = A_j - q_j beta0.
// The second form of beta0 is the first one with w (1 - q) = lambda q put in: it has no difference of two sums (which
// loses every digit of sum w - sum w q once the prior is wide and q -> 1).  w_j z_j = w_j ln(mu_j / s_j) +
// (y_j - mu_j) / (1 + a mu_j) needs no division by mu.  No p x p algebra, no factorisation, no limit on N.
//
// Deviance of the stopping rule: dev = -2 sum_j log NB(y_j; mu_j, size r = 1 / a), the full log-pmf
//     log NB = [lgamma(y + r) - lgamma(r) - lgamma(y + 1)] + y (ln mu - ln r - L1) - r L1,   L1 = log1p(a mu):
// the bracket is summed once per gene, log(r + mu) = ln r + L1 is taken as a log1p so that r ln r never meets
// r log(r + mu) (they cancel to O(mu); at a = 1e-8 the difference would carry 1e-7 of noise).
//
// One sweep per iteration (rlog_sweep_*): from the solution of the previous sweep's sums every sample's eta_j = beta0 + b_j,
// mu_j (one exponential), the deviance term (one log1p) and the A_j, q_j of the NEXT solve (two reciprocals), and one
// fused reduction of four values: the deviance sum, sum A, sum q and the number of |b_j| > 30.
// Written once over the wave policy: rlog_gene composes the pieces for a policy whose call is one lane (DeviceWave in
// dsq_k_rlog.hip, HostWave); a host build that steps 64 lanes in lockstep composes the same pieces (tests/hostrlog).
#pragma once
#include "dsq_alpha.h"
#include "dsq_wave.h"

namespace dsq {

constexpr int kRlogMaxIter = 100;
constexpr double kRlogTol = 1e-4, kRlogMinMu = 0.5, kRlogMaxBeta = 30.0;
constexpr double kLn2 = 0.69314718055994530942, kInvLn2 = 1.44269504088896340736;
constexpr double kLnHalf = -0.69314718055994530942;

struct RlogPar {
    double a, r, lr;  // dispersion, size 1 / a and its logarithm
    double lam;       // lambda of the sample coefficients, natural-log scale: 1 / (beta_prior_var ln^2 2)
    double k0;        // lambda0 / lambda, lambda0 = 1e-6 / ln^2 2
};

DSQ_HD RlogPar rlog_par(double disp, double beta_prior_var) {
    RlogPar p;
    p.a = disp;
    p.r = 1.0 / disp;
    p.lr = flog_t(p.r);
    p.lam = 1.0 / (beta_prior_var * kLn2 * kLn2);
    p.k0 = 1e-6 * beta_prior_var;
    return p;
}

// One sample at eta = beta0 + b_j (lns = ln s_j): its term of sum_j log NB less the per-gene constant, and the A, q of
// the next solve.  mu = max(s exp(eta), 0.5); ln mu is eta + lns, or ln 0.5 where the clamp is active.
DSQ_HD void rlog_terms(const RlogPar& p, double y, double lns, double eta, double& A, double& q, double& v) {
    const double e = eta + lns;
    const double m = fexp_t(e);
    const bool clamped = m < kRlogMinMu;
    const double mu = clamped ? kRlogMinMu : m, lm = clamped ? kLnHalf : e;
    const double u = p.a * mu;
    const double rw = frcp(1.0 + u);
    const double L1 = flog1p_t(u, rw);
    v = fma(y, (lm - p.lr) - L1, -(p.r * L1));
    const double w = mu * rw;
    const double wz = fma(w, lm - lns, (y - mu) * rw);
    const double inv = frcp(w + p.lam);
    A = wz * inv;
    q = w * inv;
}

// lgamma(y + r) - lgamma(r) - lgamma(y + 1): the part of log NB that no iteration changes (lga = lgamma(r))
template <class Wv>
DSQ_HD double rlog_const_term(int yi, double r, double lga) {
    double dl, dd;
    lgamma_digamma_diff<Wv, false>(yi, r, lga, 0.0, dl, dd);  // lgamma(r) - lgamma(y + r)
    const bool in_tab = yi < kLgammaIntN;
    double lg1 = kLgammaInt[in_tab ? yi : 0];
    if (Wv::any(!in_tab)) {
        const double z = in_tab ? 300.0 : (double)yi + 1.0;
        const double big = (z - 0.5) * flog_t(z) - z + kHalfLog2Pi + stirling_tail(frcp(z));
        if (!in_tab) lg1 = big;
    }
    return -dl - lg1;
}

// ---- a lane's samples in registers: R of them, n = lane + i W (N <= R W)
template <int R>
struct RlogRegs {
    double y[R], lns[R], eta[R], A[R], q[R];
    bool valid[R];
};

// loads the lane's samples, starts every eta at beta0 and returns the lane's share of the constant; s[]: the sums
template <class Wv, int R>
DSQ_HD double rlog_begin_regs(RlogRegs<R>& m, const RlogPar& p, const int32_t* y, const double* sf, int N, double lga,
                              double beta0, double (&s)[4]) {
    double cst = 0.0;
    s[0] = s[1] = s[2] = s[3] = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int n = Wv::lane() + i * Wv::W;
        m.valid[i] = n < N;
        const int yi = m.valid[i] ? y[n] : 0;
        m.y[i] = (double)yi;
        m.lns[i] = flog_t(m.valid[i] ? sf[n] : 1.0);
        m.eta[i] = beta0;
        const double c = rlog_const_term<Wv>(yi, p.r, lga);
        double v;
        rlog_terms(p, m.y[i], m.lns[i], beta0, m.A[i], m.q[i], v);
        if (m.valid[i]) {
            cst += c;
            s[1] += m.A[i];
            s[2] += m.q[i];
        }
    }
    return cst;
}

template <class Wv, int R>
DSQ_HD void rlog_sweep_regs(RlogRegs<R>& m, const RlogPar& p, double beta0, double (&s)[4]) {
    s[0] = s[1] = s[2] = s[3] = 0.0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const double b = fma(-m.q[i], beta0, m.A[i]);
        m.eta[i] = beta0 + b;
        double v;
        rlog_terms(p, m.y[i], m.lns[i], m.eta[i], m.A[i], m.q[i], v);
        if (m.valid[i]) {
            s[0] += v;
            s[1] += m.A[i];
            s[2] += m.q[i];
            s[3] += fabs(b) > kRlogMaxBeta ? 1.0 : 0.0;
        }
    }
}

template <class Wv, int R>
DSQ_HD void rlog_store_regs(const RlogRegs<R>& m, double* out, int N) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int n = Wv::lane() + i * Wv::W;
        if (n < N) out[n] = m.eta[i] * kInvLn2;
    }
}

// ---- any N: eta lives in the gene's output row (natural log until rlog_store_row), the counts are read again and the
// A, q of the previous sweep are recomputed from the eta it left (a second exponential and the logarithm of the size
// factor per sample and sweep: the price of holding nothing per sample - a solve-then-sweep order would recompute them
// just the same, b_j = A_j - q_j beta0 needs both and the row holds one value; 1.8 x the register path's time per sample
// and iteration)
template <class Wv>
DSQ_HD double rlog_begin_row(const RlogPar& p, const int32_t* y, const double* sf, double* row, int N, double lga,
                             double beta0, double (&s)[4]) {
    double cst = 0.0;
    s[0] = s[1] = s[2] = s[3] = 0.0;
    for (int n = Wv::lane(); n < N; n += Wv::W) {
        const int yi = y[n];
        cst += rlog_const_term<Wv>(yi, p.r, lga);
        double A, q, v;
        rlog_terms(p, (double)yi, flog_t(sf[n]), beta0, A, q, v);
        row[n] = beta0;
        s[1] += A;
        s[2] += q;
    }
    return cst;
}

template <class Wv>
DSQ_HD void rlog_sweep_row(const RlogPar& p, const int32_t* y, const double* sf, double* row, int N, double beta0,
                           double (&s)[4]) {
    s[0] = s[1] = s[2] = s[3] = 0.0;
    for (int n = Wv::lane(); n < N; n += Wv::W) {
        const double yy = (double)y[n], lns = flog_t(sf[n]);
        double A, q, v;
        rlog_terms(p, yy, lns, row[n], A, q, v);
        const double b = fma(-q, beta0, A);
        const double eta = beta0 + b;
        row[n] = eta;
        rlog_terms(p, yy, lns, eta, A, q, v);
        s[0] += v;
        s[1] += A;
        s[2] += q;
        s[3] += fabs(b) > kRlogMaxBeta ? 1.0 : 0.0;
    }
}

template <class Wv>
DSQ_HD void rlog_store_row(double* row, int N) {
    for (int n = Wv::lane(); n < N; n += Wv::W) row[n] *= kInvLn2;
}

// ---- the part every lane computes alike, from the reduced sums
struct RlogFit {
    double beta0, cst, dev_old;
    int n_iter, converged;
};

// the intercept of the iteration that begins, from the sums the previous sweep left; called at the top of every iteration
// and nowhere else, so f.beta0 is always the beta0 the eta in place were built from (the one reported), also at the cap
DSQ_HD void rlog_solve(RlogFit& f, const RlogPar& p, const double (&s)[4]) { f.beta0 = s[1] / (s[2] + p.k0); }

// after the sweep of iteration t (its coefficients are in place): true when the fit stops here
DSQ_HD bool rlog_check(RlogFit& f, const RlogPar& p, const double (&s)[4], int t) {
    if (fabs(f.beta0) > kRlogMaxBeta || s[3] > 0.0) {  // fitBeta: a coefficient beyond +-30: not converged
        f.n_iter = kRlogMaxIter;
        return true;
    }
    const double dev = -2.0 * (f.cst + s[0]);
    const double c = fabs(dev - f.dev_old) / (fabs(dev) + 0.1);
    if (c != c) {
        f.n_iter = kRlogMaxIter;
        return true;
    }
    if (t > 0 && c < kRlogTol) {
        f.n_iter = t + 1;
        f.converged = f.n_iter < kRlogMaxIter;
        return true;
    }
    f.dev_old = dev;
    return false;
}

DSQ_HD void rlog_fit_begin(RlogFit& f, double cst) {
    f.cst = cst;
    f.dev_old = 0.0;
    f.n_iter = kRlogMaxIter;
    f.converged = 0;
}

struct RlogOut {
    double intercept;  // log2
    int n_iter, converged;
};

// A gene whose base mean is not positive (no counts) is not fitted: a row of zeros, intercept 0, n_iter 0, not converged.
// R = 0: the row path.
template <class Wv, int R>
DSQ_HD RlogOut rlog_gene(const int32_t* y, const double* sf, int N, double disp, double base_mean, double beta_prior_var,
                         double* out) {
    RlogOut o;
    if (!(base_mean > 0.0)) {
        for (int n = Wv::lane(); n < N; n += Wv::W) out[n] = 0.0;
        o.intercept = 0.0;
        o.n_iter = 0;
        o.converged = 0;
        return o;
    }
    const RlogPar p = rlog_par(disp, beta_prior_var);
    double lga, dga;
    lgamma_digamma<false, true>(p.r, lga, dga);
    RlogFit f;
    f.beta0 = flog_t(base_mean);
    double s[4];
    if constexpr (R > 0) {
        RlogRegs<R> m;
        const double c = Wv::sum(rlog_begin_regs<Wv, R>(m, p, y, sf, N, lga, f.beta0, s));
        Wv::sum_n(s);
        rlog_fit_begin(f, c);
        for (int t = 0; t < kRlogMaxIter; ++t) {
            rlog_solve(f, p, s);
            rlog_sweep_regs<Wv, R>(m, p, f.beta0, s);
            Wv::sum_n(s);
            if (rlog_check(f, p, s, t)) break;
        }
        rlog_store_regs<Wv, R>(m, out, N);
    } else {
        const double c = Wv::sum(rlog_begin_row<Wv>(p, y, sf, out, N, lga, f.beta0, s));
        Wv::sum_n(s);
        rlog_fit_begin(f, c);
        for (int t = 0; t < kRlogMaxIter; ++t) {
            rlog_solve(f, p, s);
            rlog_sweep_row<Wv>(p, y, sf, out, N, f.beta0, s);
            Wv::sum_n(s);
            if (rlog_check(f, p, s, t)) break;
        }
        rlog_store_row<Wv>(out, N);
    }
    o.intercept = f.beta0 * kInvLn2;
    o.n_iter = f.n_iter;
    o.converged = f.converged;
    return o;
}

}  // namespace dsq
