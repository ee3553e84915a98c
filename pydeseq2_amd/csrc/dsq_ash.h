// dsq_ash.h — adaptive shrinkage of a contrast's log fold changes: Stephens' ashr as DESeq2's lfcShrink(type = "ashr") calls it
// (mixcompdist = "normal", method = "shrink": a zero-mean mixture of normals without a point mass, prior "uniform",
// optimiser mixSQP).  The reference project has none; DESIGN.md 6i is the statement of the algorithm, and parity with R is
// by construction from it, not measured.
//
// Per contrast, from (b_g, s_g) alone (a gene is used if both are finite and s_g > 0; n used genes), with the grid of
// standard deviations sd_m, m < M <= 48, given by the caller:
//     l_gm = -1/2 log(s_g^2 + sd_m^2) - 1/2 b_g^2 / (s_g^2 + sd_m^2),   L_gm = exp(l_gm - max_m l_gm)   (never stored),
//     minimise f(x) = -(1/n) sum_g log(sum_m L_gm x_m) + sum_m x_m over x >= 0   (its minimiser sums to 1: the ML pi).
// Newton steps on an active set: u = L x, d_m = (1/n) sum_g L_gm / u_g, grad = 1 - d, H = (1/n) sum_g (L_g / u_g)(L_g / u_g)^T
// + 1e-8 I; stop at min grad >= -1e-8; else y = argmin 1/2 y^T H y + (grad - H x)^T y over y >= 0 (ash_qp: Lawson-Hanson
// on the normal equations, started from the support of x), p = y - x, backtracking t = 1, 0.75, ... until
// f(x + t p) <= f(x) + 0.01 t grad^T p + 1e-14 (1 + |f(x)|) (kAshNoise; below t = 1e-8 the step is taken as it is).
//
// Genes are walked in chunks of 64, lane = gene: a wave takes the chunks wv, wv + nw, ...  For a chunk the lanes leave
// L in the wave's xs[m][lane], w = 1 / (n u^2), r = 1 / (n u), log u and the row maximum in four 64-vectors; H's share is
// WideGram's (dsq_wide.h: the fp64 matrix cores on the device, plain sums on the host), and lane j < M + 2 walks row j of
// xs (d_j), the logarithms (j = M) and the row maxima (j = M + 1) in gene order.  Unused genes and the lanes beyond G are
// masked (w = r = 0 and finite xs), not compacted.  The waves' partial sums are added in wave order (ash_combine).  So the
// order of every addition is fixed by (G, nw) alone - a rerun gives the same bits, and a host build that steps the waves
// one after the other (tests/hostash) adds in the device's order everywhere but inside a chunk of the Gram matrix.
// Wave 0 then runs ash_drive: the stop test, the QP and the step control, one call per pass.
#pragma once
#include <cfloat>

#include "dsq_wide.h"

namespace dsq {

constexpr int kAshMaxM = kWideMaxP;
constexpr int kAshVec = kAshMaxM + 4;  // a vector of the block: M values and the sums of log u and of the row maxima
constexpr double kAshConvTol = 1e-8, kAshDelta = 1e-8, kAshDecrease = 0.01, kAshStepCut = 0.75, kAshMinStep = 1e-8;
constexpr double kAshQpTol = 1e-10;
// Allowance for the rounding of f in the sufficient-decrease test, relative to 1 + |f(x)|.  f is a mean of n logarithms and
// carries a few 1e-16 sqrt(n) of rounding; within a step or two of the stop the decrease a Newton step promises is smaller
// than that, the exact test then fails at every step length and a search of 65 passes ends in a step of 1e-8 (one plain
// contrast of 60 000 genes in 28 needed 648 passes that way, 7 with the allowance).  45 ulp.
constexpr double kAshNoise = 1e-14;
constexpr double kLog2Pi = 1.83787706640934548356;

DSQ_HD bool ash_finite(double v) { return fabs(v) <= DBL_MAX; }
DSQ_HD bool ash_used(double b, double s) { return ash_finite(b) && ash_finite(s) && s > 0.0; }

// ---- workspace of one wave: the chunk (xs, four 64-vectors) and its partial H.  On the device the partial H is written
// once, from the accumulator registers after the last chunk, and takes the place of xs (alias_h); the host's WideGram adds
// into it chunk by chunk, so there it has a place of its own.
DSQ_HD int ash_rows(int M) { return ((M + 15) / 16) * 16; }
DSQ_HD int ash_wave_doubles(int M, bool alias_h) {
    return ash_rows(M) * kWideXsLd + 4 * 64 + (alias_h ? 0 : M * wide_ld(M));
}
struct AshWave {
    WideWork W;  // P = M, ld, rows, xs, w and M (the partial H) are bound; nothing else is used
    double *r, *lg, *mx;
    DSQ_HD void bind(double* base, int M, bool alias_h) {
        W.P = M; W.ld = wide_ld(M); W.rows = ash_rows(M);
        W.xs = base;
        W.w = W.xs + W.rows * kWideXsLd;
        r = W.w + 64; lg = r + 64; mx = lg + 64;
        W.M = alias_h ? W.xs : mx + 64;
        W.dM = W.L = W.Li = W.inv = W.vec = W.acc = W.tab = nullptr;
    }
};

// ---- workspace of the block (one contrast)
struct AshBlock {
    int M, ld, nw;
    double *H, *A;                             // M x ld: H, and the working set's block of it / its Cholesky factor
    double *sd2, *x, *xt, *y, *z, *q, *d, *p;  // [kAshVec]; d: d_m, then the sums of log u and of the row maxima
    double* part;                              // [nw][kAshVec] the waves' shares of d
    int *idx, *in_set, *ban, *ctl;             // [kAshMaxM] each; ctl[0]: the next pass builds H, ctl[1]: finished
    DSQ_HD static int doubles(int M, int nw) { return 2 * M * wide_ld(M) + (8 + nw) * kAshVec + 2 * kAshMaxM; }
    DSQ_HD void bind(double* base, int M_, int nw_) {
        M = M_; ld = wide_ld(M_); nw = nw_;
        H = base; A = H + M * ld;
        sd2 = A + M * ld; x = sd2 + kAshVec; xt = x + kAshVec; y = xt + kAshVec; z = y + kAshVec; q = z + kAshVec;
        d = q + kAshVec; p = d + kAshVec;
        part = p + kAshVec;
        idx = (int*)(part + nw * kAshVec);
        in_set = idx + kAshMaxM; ban = in_set + kAshMaxM; ctl = ban + kAshMaxM;
    }
};

// number of used genes among the chunks of wave wv
template <class Wv>
DSQ_HD int ash_count(const double* b, const double* s, int G, int wv, int nw) {
    int c = 0;
    for (int g0 = wv * 64; g0 < G; g0 += nw * 64)
        for (int l = Wv::lane(); l < 64; l += Wv::W) {
            const int g = g0 + l;
            if (g < G && ash_used(b[g], s[g])) c += 1;
        }
    return Wv::sumi(c);
}

// One pass of wave wv at the point xv: its share of d and of the two sums into B.part[wv], and with `gram` its share of
// H (already divided by n) into Q.W.M.  The rows of xs beyond M must be zero (wide_zero_pad_rows, once).
template <class Wv>
DSQ_HD void ash_pass(const AshBlock& B, const AshWave& Q, int wv, const double* b, const double* s, int G,
                     const double* xv, double inv_n, bool gram) {
    const int M = B.M;
    double* dp = B.part + wv * kAshVec;
    double* xs = Q.W.xs;
    WideGram<Wv, false> gr;
    if (gram) gr.begin(Q.W);
    for (int j = Wv::lane(); j < M + 2; j += Wv::W) dp[j] = 0.0;
    Wv::sync();
    for (int g0 = wv * 64; g0 < G; g0 += B.nw * 64) {
        for (int l = Wv::lane(); l < 64; l += Wv::W) {
            const int g = g0 + l;
            double bb = g < G ? b[g] : 0.0, ss = g < G ? s[g] : 0.0;
            const bool used = ash_used(bb, ss);
            if (!used) { bb = 0.0; ss = 1.0; }  // (finite xs in a masked lane)
            const double s2 = ss * ss, hb2 = 0.5 * bb * bb;
            double top = -DBL_MAX;
            for (int m = 0; m < M; ++m) {
                const double v = s2 + B.sd2[m];
                const double lm = -0.5 * log(v) - hb2 / v;
                xs[m * kWideXsLd + l] = lm;
                top = lm > top ? lm : top;
            }
            double u = 0.0;
            for (int m = 0; m < M; ++m) {
                const double Lm = exp(xs[m * kWideXsLd + l] - top);
                xs[m * kWideXsLd + l] = Lm;
                u += Lm * xv[m];
            }
            const double ru = 1.0 / u;
            Q.W.w[l] = used ? inv_n * ru * ru : 0.0;
            Q.r[l] = used ? inv_n * ru : 0.0;
            Q.lg[l] = used ? log(u) : 0.0;
            Q.mx[l] = used ? top : 0.0;
        }
        Wv::sync();
        if (gram) gr.add_chunk(Q.W);
        for (int j = Wv::lane(); j < M + 2; j += Wv::W) {
            double acc = dp[j];
            if (j < M) {
                for (int n = 0; n < 64; ++n) acc += xs[j * kWideXsLd + n] * Q.r[n];
            } else {
                const double* v = j == M ? Q.lg : Q.mx;
                for (int n = 0; n < 64; ++n) acc += v[n];
            }
            dp[j] = acc;
        }
        Wv::sync();
    }
    if (gram) gr.finish(Q.W);
}

// The waves' shares, added in wave order: thread tid of nt.  h0 + w * hstride: the partial H of wave w.
DSQ_HD void ash_combine(const AshBlock& B, const double* h0, int hstride, bool gram, int tid, int nt) {
    const int M = B.M, ld = B.ld;
    for (int j = tid; j < M + 2; j += nt) {
        double a = B.part[j];
        for (int w = 1; w < B.nw; ++w) a += B.part[w * kAshVec + j];
        B.d[j] = a;
    }
    if (!gram) return;
    for (int e = tid; e < M * M; e += nt) {
        const int i = e / M, j = e % M;
        double a = h0[i * ld + j];
        for (int w = 1; w < B.nw; ++w) a += h0[w * hstride + i * ld + j];
        B.H[i * ld + j] = a + (i == j ? kAshDelta : 0.0);
    }
}

// ---- the quadratic subproblem: y = argmin 1/2 y^T H y + q^T y over y >= 0, q = grad - H x, into B.y.  Lawson-Hanson's
// active-set scheme on the normal equations (what nnls does on the Cholesky factor of H), started from the support of x:
// solve on the working set; while a component of the solution is not positive, go as far towards it as feasibility allows
// and drop what reached zero; then add the zero component with the most negative gradient, until none is below -1e-10.
// A component whose own solve does not make it positive is set aside until y moves.  Uniform in the wave: every lane
// reads the same values from the block's workspace.
template <class Wv>
DSQ_HD void ash_qp(const AshBlock& B) {
    const int M = B.M, ld = B.ld;
    for (int m = Wv::lane(); m < M; m += Wv::W) {
        double r = 0.0;
        for (int j = 0; j < M; ++j) r += B.H[m * ld + j] * B.x[j];
        B.q[m] = (1.0 - B.d[m]) - r;
        B.y[m] = B.x[m];
        B.in_set[m] = B.x[m] > 0.0 ? 1 : 0;
        B.ban[m] = 0;
    }
    Wv::sync();
    bool solve = true;  // the first round solves on the support of x
    int added = -1;
    for (int round = 0; round < 8 * kAshMaxM; ++round) {
        if (!solve) {
            for (int m = Wv::lane(); m < M; m += Wv::W) {
                double r = B.q[m];
                for (int j = 0; j < M; ++j) r += B.H[m * ld + j] * B.y[j];
                B.z[m] = r;
            }
            Wv::sync();
            int best = -1;
            double gbest = -kAshQpTol;
            for (int m = 0; m < M; ++m)
                if (!B.in_set[m] && !B.ban[m] && B.z[m] < gbest) { gbest = B.z[m]; best = m; }
            if (best < 0) return;  // the subproblem's KKT conditions hold
            Wv::sync();
            if (Wv::lane() == 0) B.in_set[best] = 1;
            Wv::sync();
            added = best;
        }
        solve = false;
        for (;;) {
            int k = 0, at = -1;
            for (int m = 0; m < M; ++m)
                if (B.in_set[m]) {
                    if (m == added) at = k;
                    if (Wv::lane() == 0) B.idx[k] = m;
                    k += 1;
                }
            if (k == 0) break;
            Wv::sync();
            WideWork Wk;
            Wk.P = k; Wk.ld = wide_ld(k); Wk.rows = ash_rows(k);
            for (int e = Wv::lane(); e < k * k; e += Wv::W) {
                const int i = e / k, j = e % k;
                if (j <= i) B.A[i * Wk.ld + j] = B.H[B.idx[i] * ld + B.idx[j]];
            }
            for (int i = Wv::lane(); i < k; i += Wv::W) B.z[i] = -B.q[B.idx[i]];
            Wv::sync();
            wide_chol<Wv>(Wk, B.A, B.A, 0.0);  // (in place: column j is read before it is written)
            wide_chol_solve<Wv>(Wk, B.A, B.z);
            bool bad = false;
            double alpha = 2.0;
            for (int i = 0; i < k; ++i) {
                const double zi = B.z[i];
                bad = bad || !ash_finite(zi);
                if (zi <= 0.0) {
                    const double yi = B.y[B.idx[i]];
                    const double a = yi > 0.0 ? yi / (yi - zi) : 0.0;
                    alpha = a < alpha ? a : alpha;
                }
            }
            Wv::sync();
            if (bad) {  // the factorisation broke down: no step (ash_drive ends the fit)
                for (int m = Wv::lane(); m < M; m += Wv::W) B.y[m] = B.x[m];
                Wv::sync();
                return;
            }
            if (at >= 0 && B.z[at] <= 0.0) {  // the newcomer would not enter: aside with it
                if (Wv::lane() == 0) { B.in_set[added] = 0; B.ban[added] = 1; }
                Wv::sync();
                added = -1;
                break;
            }
            added = -1;
            if (alpha > 1.0) {  // every component positive: the working set's minimiser
                for (int i = Wv::lane(); i < k; i += Wv::W) B.y[B.idx[i]] = B.z[i];
                for (int m = Wv::lane(); m < M; m += Wv::W) B.ban[m] = 0;
                Wv::sync();
                break;
            }
            for (int i = Wv::lane(); i < k; i += Wv::W) {
                const int m = B.idx[i];
                const double yi = B.y[m], zi = B.z[i];
                double yn = yi + alpha * (zi - yi);
                if (zi <= 0.0 && (yi > 0.0 ? yi / (yi - zi) : 0.0) <= alpha) yn = 0.0;
                if (!(yn > 0.0)) { yn = 0.0; B.in_set[m] = 0; }
                B.y[m] = yn;
            }
            for (int m = Wv::lane(); m < M; m += Wv::W) B.ban[m] = 0;
            Wv::sync();
        }
    }
}

// ---- the stop test and the step control: one call after every pass, which was at B.xt
enum AshPhase { ASH_FIRST = 0, ASH_TRIAL = 1, ASH_SEARCH = 2, ASH_REFRESH = 3 };
struct AshState {
    double f, gp, t, inv_n, noise;  // f(x) and its rounding allowance; grad^T p and the step length of the search in progress
    int phase, it, max_iter, converged;
    DSQ_HD void begin(int n, int max_iter_) {
        f = gp = noise = 0.0; t = 1.0; inv_n = 1.0 / (double)n;
        phase = ASH_FIRST; it = 0; max_iter = max_iter_; converged = 0;
    }
};

template <class Wv>
DSQ_HD void ash_set_trial(const AshBlock& B, double t) {
    for (int m = Wv::lane(); m < B.M; m += Wv::W) B.xt[m] = B.x[m] + t * B.p[m];
    Wv::sync();
}

// Sets B.xt and B.ctl for the next pass; true when the fit has ended (B.x, B.d and S are the result).  The first trial of
// a search (t = 1) is a pass with H: accepted, as nearly always, it is the next iteration's evaluation.  The passes of a
// search that goes on skip H, and the point it ends at is evaluated once more, with H.
template <class Wv>
DSQ_HD bool ash_drive(const AshBlock& B, AshState& S) {
    const int M = B.M;
    double sx = 0.0;
    for (int m = 0; m < M; ++m) sx += B.xt[m];
    const double fe = -S.inv_n * B.d[M] + sx;
    bool gram = true;
    if (S.phase == ASH_TRIAL && !(fe <= S.f + kAshDecrease * S.gp + S.noise)) {
        S.t = kAshStepCut;
        S.phase = ASH_SEARCH;
        gram = false;
    } else if (S.phase == ASH_SEARCH) {
        if (fe <= S.f + kAshDecrease * S.t * S.gp + S.noise) {
            S.phase = ASH_REFRESH;  // (B.xt is set to the same x + t p again below)
        } else {
            S.t *= kAshStepCut;
            if (S.t < kAshMinStep) S.phase = ASH_REFRESH;
            else gram = false;
        }
    } else {  // an evaluation with H at the point that is now current
        Wv::sync();
        for (int m = Wv::lane(); m < M; m += Wv::W) B.x[m] = B.xt[m];
        Wv::sync();
        S.f = fe;
        S.noise = kAshNoise * (1.0 + fabs(fe));
        double gmin = DBL_MAX;
        for (int m = 0; m < M; ++m) gmin = dmin(gmin, 1.0 - B.d[m]);
        bool done = false;
        if (gmin >= -kAshConvTol) { S.converged = 1; done = true; }
        else if (S.it >= S.max_iter || !ash_finite(gmin)) done = true;
        if (!done) {
            ash_qp<Wv>(B);
            for (int m = Wv::lane(); m < M; m += Wv::W) B.p[m] = B.y[m] - B.x[m];
            Wv::sync();
            double gp = 0.0;
            for (int m = 0; m < M; ++m) gp += (1.0 - B.d[m]) * B.p[m];
            if (!(gp < 0.0)) done = true;  // no descent direction (the subproblem failed): not converged
            else {
                S.gp = gp; S.t = 1.0; S.it += 1; S.phase = ASH_TRIAL;
            }
        }
        if (done) {
            if (Wv::lane() == 0) { B.ctl[0] = 0; B.ctl[1] = 1; }
            Wv::sync();
            return true;
        }
    }
    Wv::sync();
    ash_set_trial<Wv>(B, S.t);
    if (Wv::lane() == 0) { B.ctl[0] = gram ? 1 : 0; B.ctl[1] = 0; }
    Wv::sync();
    return false;
}

struct AshFit {
    double kkt, loglik;
    int n_iter, converged;
};
// pi into pi_out (lanes of the calling wave), the rest returned
template <class Wv>
DSQ_HD AshFit ash_result(const AshBlock& B, const AshState& S, int n, double* pi_out) {
    const int M = B.M;
    double sx = 0.0, dtop = -DBL_MAX;
    for (int m = 0; m < M; ++m) { sx += B.x[m]; dtop = dmax(dtop, B.d[m]); }
    for (int m = Wv::lane(); m < M; m += Wv::W) pi_out[m] = B.x[m] / sx;
    AshFit o;
    o.kkt = dtop - 1.0;
    o.loglik = (B.d[M] + B.d[M + 1]) - 0.5 * (double)n * kLog2Pi;
    o.n_iter = S.it;
    o.converged = S.converged;
    return o;
}

// ---- posterior of one gene under the fitted mixture: mean, standard deviation and local false sign rate
DSQ_HD void ash_posterior(double b, double s, const double* sd, const double* pi, int M, double& pm, double& psd,
                          double& lfsr) {
    if (!ash_used(b, s)) {
        pm = psd = lfsr = NAN;
        return;
    }
    const double s2 = s * s, hb2 = 0.5 * b * b;
    double top = -DBL_MAX;
    for (int m = 0; m < M; ++m) {
        const double v = s2 + sd[m] * sd[m];
        const double lm = -0.5 * log(v) - hb2 / v;
        top = lm > top ? lm : top;
    }
    double sw = 0.0, s1 = 0.0, sq = 0.0, neg = 0.0, pos = 0.0;
    for (int m = 0; m < M; ++m) {
        if (!(pi[m] > 0.0)) continue;
        const double g2 = sd[m] * sd[m], v = s2 + g2;
        const double wl = pi[m] * exp((-0.5 * log(v) - hb2 / v) - top);
        const double t = g2 / v, mu = t * b, var = t * s2;
        const double zz = mu / sqrt(var);
        sw += wl;
        s1 += wl * mu;
        sq += wl * (var + mu * mu);
        neg += wl * norm_sf(zz);
        pos += wl * norm_sf(-zz);
    }
    pm = s1 / sw;
    psd = sqrt(dmax(sq / sw - pm * pm, 0.0));
    lfsr = dmin(neg, pos) / sw;
}

}  // namespace dsq
