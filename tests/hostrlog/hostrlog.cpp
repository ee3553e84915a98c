// hostrlog.cpp — TEST-ONLY host instantiation of the regularized-log templates (dsq_rlog.h).
// Built by tests/hostrlog/build.py with g++ and -ffp-contract=off into tests/hostrlog/_hostrlog.so, loaded only by tests.
//
// Two policies over the same pieces: HostWave (one lane walks every sample; rlog_gene as the kernel calls it, on the row
// path), and Lanes64 - 64 lanes stepped in lockstep through rlog_begin_* / rlog_sweep_* / rlog_check, their partial sums
// added in the order of DeviceWave's butterfly (partners 32, 16, 8, 4, 2, 1), with the samples in "registers"
// (RlogRegs<R>, R chosen as launch_rlog chooses it) or in the output row.
#include <cstdint>

#include "dsq_rlog.h"

using namespace dsq;

namespace {
struct Lanes64 {
    static constexpr int W = 64;
    static inline int cur = 0;
    static inline int lane() { return cur; }
    static inline bool any(bool) { return true; }  // (only guards work that is itself predicated per lane)
};

void butterfly(double (&v)[64]) {
    for (int m = 32; m >= 1; m >>= 1) {
        double t[64];
        for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ m];
        for (int l = 0; l < 64; ++l) v[l] = t[l];
    }
}

// the lanes' four partial sums -> s (every lane of a wavefront ends with the same totals)
void reduce4(double (&part)[64][4], double (&s)[4]) {
    for (int k = 0; k < 4; ++k) {
        double v[64];
        for (int l = 0; l < 64; ++l) v[l] = part[l][k];
        butterfly(v);
        s[k] = v[0];
    }
}

template <int R>
RlogOut gene64(const int32_t* y, const double* sf, int N, double disp, double bm, double bpv, double* out) {
    RlogOut o{0.0, 0, 0};
    if (!(bm > 0.0)) {
        for (int n = 0; n < N; ++n) out[n] = 0.0;
        return o;
    }
    const RlogPar p = rlog_par(disp, bpv);
    double lga, dga;
    lgamma_digamma<false, true>(p.r, lga, dga);
    RlogFit f;
    f.beta0 = flog_t(bm);
    static RlogRegs<(R > 0 ? R : 1)> m[64];
    double part[64][4], c[64], s[4];
    for (int l = 0; l < 64; ++l) {
        Lanes64::cur = l;
        if constexpr (R > 0) c[l] = rlog_begin_regs<Lanes64, R>(m[l], p, y, sf, N, lga, f.beta0, part[l]);
        else c[l] = rlog_begin_row<Lanes64>(p, y, sf, out, N, lga, f.beta0, part[l]);
    }
    butterfly(c);
    reduce4(part, s);
    rlog_fit_begin(f, c[0]);
    for (int t = 0; t < kRlogMaxIter; ++t) {
        rlog_solve(f, p, s);
        for (int l = 0; l < 64; ++l) {
            Lanes64::cur = l;
            if constexpr (R > 0) rlog_sweep_regs<Lanes64, R>(m[l], p, f.beta0, part[l]);
            else rlog_sweep_row<Lanes64>(p, y, sf, out, N, f.beta0, part[l]);
        }
        reduce4(part, s);
        if (rlog_check(f, p, s, t)) break;
    }
    for (int l = 0; l < 64; ++l) {
        Lanes64::cur = l;
        if constexpr (R > 0) rlog_store_regs<Lanes64, R>(m[l], out, N);
        else rlog_store_row<Lanes64>(out, N);
    }
    o.intercept = f.beta0 * kInvLn2;
    o.n_iter = f.n_iter;
    o.converged = f.converged;
    return o;
}
}  // namespace

extern "C" {

// mode 0: one lane; 1: 64 lanes, registers up to N = 512 and the row beyond (the kernel's choice); 2: 64 lanes, row path
int hr_rlog(const int32_t* y, int ldn, const double* sf, int N, int G, const double* disp, const double* base_mean,
            double beta_prior_var, int mode, double* out, double* intercept, uint8_t* conv, int32_t* niter) {
    if (N < 1 || G < 0 || ldn < N || !(beta_prior_var > 0.0) || mode < 0 || mode > 2) return -1;
    for (int g = 0; g < G; ++g) {
        const int32_t* yg = y + (size_t)g * ldn;
        double* og = out + (size_t)g * N;
        RlogOut o;
        if (mode == 0) o = rlog_gene<HostWave, 0>(yg, sf, N, disp[g], base_mean[g], beta_prior_var, og);
        else if (mode == 2 || N > 512) o = gene64<0>(yg, sf, N, disp[g], base_mean[g], beta_prior_var, og);
        else if (N <= 64) o = gene64<1>(yg, sf, N, disp[g], base_mean[g], beta_prior_var, og);
        else if (N <= 128) o = gene64<2>(yg, sf, N, disp[g], base_mean[g], beta_prior_var, og);
        else if (N <= 256) o = gene64<4>(yg, sf, N, disp[g], base_mean[g], beta_prior_var, og);
        else o = gene64<8>(yg, sf, N, disp[g], base_mean[g], beta_prior_var, og);
        intercept[g] = o.intercept;
        conv[g] = (uint8_t)o.converged;
        niter[g] = o.n_iter;
    }
    return 0;
}

}  // extern "C"
