// dsq_proj.h — hidden-batch factors and batch removal (RUVg / RUVr, limma's removeBatchEffect): the three
// per-gene operations the host side of pydeseq2_amd/ruv.py is built on.
//   log_counts_row    Y = log(v + eps), v = (double)y / sf by IEEE division (or v = y)
//   nb_residuals_row  deviance or Pearson residuals of the NB GLM, post hoc from beta, dispersion and size factors
//   project_row       c_j = sum_n x_n P_nj, out_n = x_n - sum_j c_j B_nj, then nothing / exp(.) - eps / its rounded clip
// One gene per wavefront; templates over the wave policy (dsq_wave.h): tests/hostruv runs the same code on the host.
//
// The projection keeps ONE order of the sums (as row_meanvar_row of dsq_gram.h): lane l sums n = l, l + 64, ... ascending
// with an explicit fma, the 64 lanes are added as the butterfly of DeviceWave::sum adds them (partners at distance 32, 16,
// 8, 4, 2, 1; sum_n is the same butterfly), and the subtraction is a chain of fma(-c_j, B_nj, .) with j ascending.  The
// host policy walks the 64 partial sums itself, so it reproduces the device bit for bit, and a rerun gives the same bits.
// (dsq_k_proj.hip is compiled with -ffp-contract=off, as the host build is: the only fused multiply-adds are the explicit
// ones, here and in flog_t / flog1p_t / fexp_t.)
// A lane only ever touches the samples n = lane (mod 64) of its row - while summing, in the LDS copy and when it writes -
// and a wave has finished all its sums before its first store: out may be x (in place).  No atomics.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dsq_wave.h"

namespace dsq {

constexpr int kProjMaxQ = 64;               // columns of P and B (DSQ_PROJ_MAX_Q)
constexpr int kProjLdsBytes = 152 * 1024;   // dynamic LDS of a workgroup: gfx950's 160 KiB less room for the tables of fexp_t
constexpr int kProjWaveMax = 128 * 1024;    // ... and the most one wavefront stages
constexpr int kProjRegs = 16;               // samples a lane keeps in registers: rows of up to 64 * 16 = 1024 samples

// ---- launch plan: a pure function of N.  A wavefront keeps its kProjMaxQ coefficients in LDS.  Its row: in registers up
// to 64 * kProjRegs samples (staged = 2: every load of the row is in flight at once, and the occupancy is not bounded by
// LDS); beyond, in LDS next to the coefficients (staged = 1); a row longer than that is re-read from memory by every pass.
struct ProjPlan {
    int waves;         // wavefronts (= genes) per workgroup; 0: N is refused (N < 1)
    int staged;        // where the row stays between the passes: 2 registers, 1 LDS, 0 nowhere
    int stride;        // LDS doubles per wavefront
    size_t lds_bytes;  // dynamic LDS of the workgroup
};
DSQ_HD ProjPlan proj_plan(int N) {
    ProjPlan p{0, 0, 0, 0};
    if (N < 1) return p;
    const size_t per = ((size_t)N + kProjMaxQ) * sizeof(double);
    if (N <= 64 * kProjRegs) { p.waves = 4; p.staged = 2; }                     // N <= 1024
    else if (4 * per <= (size_t)kProjLdsBytes) { p.waves = 4; p.staged = 1; }   // N <= 4800
    else if (2 * per <= (size_t)kProjLdsBytes) { p.waves = 2; p.staged = 1; }   // N <= 9664
    else if (per <= (size_t)kProjWaveMax) { p.waves = 1; p.staged = 1; }        // N <= 16 320
    else { p.waves = 4; p.staged = 0; }
    p.stride = kProjMaxQ + (p.staged == 1 ? N : 0);
    p.lds_bytes = (size_t)p.waves * (size_t)p.stride * sizeof(double);
    return p;
}

// ------------------------------------------------------------------ log counts
// flog_t wants a normal number; anything else (eps + v subnormal, inf, NaN) goes to the library
DSQ_HD double proj_log(double x) {
    if (x >= 2.2250738585072014e-308 && x < 1.7976931348623157e308) return flog_t(x);
    DSQ_NO_SPECULATE;
    return log(x);
}
// sf is read only when `normalized`: without it the caller may pass no size factors at all (a null pointer)
template <class Wv>
DSQ_HD void log_counts_row(const int32_t* y, const double* sf, int N, bool normalized, double eps, double* out) {
    if (normalized) {
        for (int n = Wv::lane(); n < N; n += Wv::W)
            out[n] = proj_log((double)y[n] / sf[n] + eps);  // IEEE division (6k): not the fast reciprocal
    } else {
        for (int n = Wv::lane(); n < N; n += Wv::W) out[n] = proj_log((double)y[n] + eps);
    }
}

// ------------------------------------------------------------------ NB residuals
// log(1 + d / lo) for d >= 0, lo > 0 (hi = lo + d as the caller has it): exactly 0 for d == 0 (6f)
DSQ_HD double proj_log1p_ratio(double d, double lo, double hi) {
    const double u = d / lo;
    if (u < 1e300) return flog1p_t(u, lo / hi);
    DSQ_NO_SPECULATE;  // a vanished or overflowed mean, NaN: whatever the library makes of it
    return log1p(u);
}
// kind 0: sign(y - mu) sqrt(max(D, 0)), D = 2 [y log(y / mu) - (y + r) log((y + r) / (mu + r))]  (y = 0: 2 r log1p(mu / r))
// kind 1: (y - mu) / sqrt(mu + alpha mu^2)
// Both logarithms of the deviance are +-log1p(|y - mu| / lo) with the SAME numerator |y - mu| (one rounding) and lo =
// min(y, mu), min(y, mu) + r: the second is never formed as the difference of y + r and mu + r, whose roundings - of the
// size of u r - would swamp y - mu at small dispersions.
DSQ_HD double nb_residual_value(double y, double mu, double alpha, double r, int kind) {
    if (kind == 1) {
        const double t = alpha * mu;
        return (y - mu) / sqrt(fma(t, mu, mu));
    }
    double h;  // D / 2
    if (y == 0.0) {
        const double u = mu / r;
        h = r * proj_log1p_ratio(u, 1.0, 1.0 + u);
    } else {
        const bool up = y >= mu;
        const double d = up ? y - mu : mu - y, lo = up ? mu : y, hi = up ? y : mu;
        const double A = y * proj_log1p_ratio(d, lo, hi);
        const double B = (y + r) * proj_log1p_ratio(d, lo + r, hi + r);
        h = up ? A - B : B - A;
    }
    const double D = 2.0 * h;
    if (D != D) return D;
    return dsign(y - mu) * sqrt(dmax(D, 0.0));
}
// Xt: the transposed design [P][ldx]; beta: the gene's P coefficients (natural log; wave-private LDS on the device).
// A gene without counts, or with a NaN coefficient or dispersion: a NaN row.
template <class Wv>
DSQ_HD void nb_residuals_row(const int32_t* y, const double* sf, const double* Xt, size_t ldx, int P, const double* beta,
                             double disp, int N, int kind, double* out) {
    bool some = false, bad = disp != disp;
    for (int n = Wv::lane(); n < N; n += Wv::W) some = some || y[n] != 0;
    for (int j = 0; j < P; ++j) bad = bad || beta[j] != beta[j];
    if (bad || !Wv::any(some)) {
        const double nan = __builtin_nan("");
        for (int n = Wv::lane(); n < N; n += Wv::W) out[n] = nan;
        return;
    }
    const double r = 1.0 / disp;
    for (int n = Wv::lane(); n < N; n += Wv::W) {
        double eta = 0.0;
        for (int j = 0; j < P; ++j) eta = fma(Xt[(size_t)j * ldx + n], beta[j], eta);
        const double mu = sf[n] * fexp_t(eta);
        out[n] = nb_residual_value((double)y[n], mu, disp, r, kind);
    }
}

// ------------------------------------------------------------------ projection
// JB coefficients c_{j0 .. j0 + JB - 1} of one gene: one pass over the row x.  FILL: x is the row in memory and the pass
// also leaves it in `fill`, the wave's LDS copy, for the passes after it (a lane reads back only what it wrote itself).
template <class Wv, int JB, bool FILL>
DSQ_HD void proj_coef_chunk(const double* x, double* fill, const double* Pt, size_t ldp, int j0, int N, double* coef) {
    if constexpr (Wv::W == 64) {
        double a[JB];
#pragma unroll
        for (int k = 0; k < JB; ++k) a[k] = 0.0;
#pragma unroll 4
        for (int n = Wv::lane(); n < N; n += 64) {
            const double xv = x[n];
            if constexpr (FILL) fill[n] = xv;
#pragma unroll
            for (int k = 0; k < JB; ++k) a[k] = fma(xv, Pt[(size_t)(j0 + k) * ldp + n], a[k]);
        }
        Wv::sum_n(a);
        if (Wv::lane() == 0) {
#pragma unroll
            for (int k = 0; k < JB; ++k) coef[j0 + k] = a[k];
        }
    } else {  // the host: the 64 partial sums and the butterfly's additions, by hand
        if constexpr (FILL)
            for (int n = 0; n < N; ++n) fill[n] = x[n];
        for (int k = 0; k < JB; ++k) {
            double p[64];
            for (int l = 0; l < 64; ++l) {
                double a = 0.0;
                for (int n = l; n < N; n += 64) a = fma(x[n], Pt[(size_t)(j0 + k) * ldp + n], a);
                p[l] = a;
            }
            for (int s = 32; s >= 1; s >>= 1)
                for (int l = 0; l < s; ++l) p[l] += p[l + s];
            coef[j0 + k] = p[0];
        }
    }
}
// the first chunk of a staged row reads memory and fills the copy, the others read the copy
template <class Wv, int JB, bool STAGE>
DSQ_HD void proj_coef_step(const double* xg, double* xs_w, const double* Pt, size_t ldp, int& j, int N, double* coef) {
    if (STAGE && j == 0)
        proj_coef_chunk<Wv, JB, STAGE>(xg, xs_w, Pt, ldp, j, N, coef);
    else
        proj_coef_chunk<Wv, JB, false>(STAGE ? xs_w : xg, nullptr, Pt, ldp, j, N, coef);
    j += JB;
}

// post: 0 nothing, 1 exp(v) - eps, 2 max(rint(exp(v) - eps), 0) (a NaN stays)
DSQ_HD double proj_post(double v, int post, double eps) {
    if (post == 0) return v;
    const double e = fexp_t(v) - eps;
    if (post == 1) return e;
    const double t = rint(e);
    return t < 0.0 ? 0.0 : t;
}

// xg: the gene's row in memory; STAGE: the first pass leaves the row in the wave's LDS copy xs_w (N doubles) and the later
// ones read that instead of xg; coef: q doubles of wave-private LDS; out may be xg; coef_out: the gene's q coefficients or
// null
template <class Wv, bool STAGE>
DSQ_HD void project_row(const double* xg, double* xs_w, const double* Pt, const double* Bt, size_t ldp, int q,
                        int N, int post, double eps, double* coef, double* out, double* coef_out) {
    const double* xs = STAGE ? xs_w : xg;
    int j = 0;
    while (j + 8 <= q) proj_coef_step<Wv, 8, STAGE>(xg, xs_w, Pt, ldp, j, N, coef);
    if (q - j >= 4) proj_coef_step<Wv, 4, STAGE>(xg, xs_w, Pt, ldp, j, N, coef);
    if (q - j >= 2) proj_coef_step<Wv, 2, STAGE>(xg, xs_w, Pt, ldp, j, N, coef);
    if (q - j >= 1) proj_coef_step<Wv, 1, STAGE>(xg, xs_w, Pt, ldp, j, N, coef);
    Wv::sync();  // lane 0's coefficients -> every lane
#pragma unroll 4
    for (int n = Wv::lane(); n < N; n += Wv::W) {
        double v = xs[n];
        for (int k = 0; k < q; ++k) v = fma(-coef[k], Bt[(size_t)k * ldp + n], v);
        out[n] = proj_post(v, post, eps);
    }
    if (coef_out != nullptr)
        for (int k = Wv::lane(); k < q; k += Wv::W) coef_out[k] = coef[k];
}

// The same with the row in registers (N <= 64 * kProjRegs; device only - the host runs project_row, whose sums take the
// samples in the same order): a lane's sample i is n = lane + 64 i; one beyond N counts as x = 0, P = 0, and fma(0, 0, a)
// leaves the bits of a partial sum as they are (a partial sum never holds -0.0).
template <class Wv, int JB>
DSQ_HD void proj_coef_chunk_reg(const double (&xv)[kProjRegs], const double* Pt, size_t ldp, int j0, int N, double* coef) {
    double a[JB];
#pragma unroll
    for (int k = 0; k < JB; ++k) a[k] = 0.0;
#pragma unroll
    for (int i = 0; i < kProjRegs; ++i) {
        const int n = Wv::lane() + 64 * i;
#pragma unroll
        for (int k = 0; k < JB; ++k) a[k] = fma(xv[i], n < N ? Pt[(size_t)(j0 + k) * ldp + n] : 0.0, a[k]);
    }
    Wv::sum_n(a);
    if (Wv::lane() == 0) {
#pragma unroll
        for (int k = 0; k < JB; ++k) coef[j0 + k] = a[k];
    }
}
template <class Wv>
DSQ_HD void project_row_reg(const double* xg, const double* Pt, const double* Bt, size_t ldp, int q, int N, int post,
                            double eps, double* coef, double* out, double* coef_out) {
    if constexpr (Wv::W != 64) {
        project_row<Wv, false>(xg, nullptr, Pt, Bt, ldp, q, N, post, eps, coef, out, coef_out);
    } else {
        double xv[kProjRegs];
#pragma unroll
        for (int i = 0; i < kProjRegs; ++i) {
            const int n = Wv::lane() + 64 * i;
            xv[i] = n < N ? xg[n] : 0.0;
        }
        int j = 0;
        // (two columns a pass: 32 loads of P in flight per lane next to the 16 values of the row; the row costs nothing to re-read)
        for (; j + 2 <= q; j += 2) proj_coef_chunk_reg<Wv, 2>(xv, Pt, ldp, j, N, coef);
        if (q - j >= 1) { proj_coef_chunk_reg<Wv, 1>(xv, Pt, ldp, j, N, coef); j += 1; }
        Wv::sync();  // lane 0's coefficients -> every lane
        for (int k = 0; k < q; ++k) {  // (per sample still a chain over k ascending; sixteen loads of B in flight)
            const double c = -coef[k];
#pragma unroll
            for (int i = 0; i < kProjRegs; ++i) {
                const int n = Wv::lane() + 64 * i;
                xv[i] = fma(c, n < N ? Bt[(size_t)k * ldp + n] : 0.0, xv[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kProjRegs; ++i) {
            const int n = Wv::lane() + 64 * i;
            if (n < N) out[n] = proj_post(xv[i], post, eps);
        }
        if (coef_out != nullptr)
            for (int k = Wv::lane(); k < q; k += Wv::W) coef_out[k] = coef[k];
    }
}

}  // namespace dsq
