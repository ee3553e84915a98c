// hostwide.cpp — TEST-ONLY host instantiation of the run-time-P templates (dsq_wide.h) over the workspace of the
// designs wider than 48 columns (dsq_wider.h: WiderWork, matrices bound apart from the small vectors as on the device).
// Built by tests/hostwide/build.py with g++ and -ffp-contract=off into tests/hostwide/_hostwide.so, loaded only by tests.
#include <cstdint>
#include <cstring>
#include <vector>

#include "dsq_wider.h"

using namespace dsq;

namespace {
// a gene's workspace: LDS part and device-memory slot, as SlotGeom (dsq_k_wide.hip) binds them
struct HostSlot {
    std::vector<double> lds, mem;
    WiderWork W;
    explicit HostSlot(int P) : lds((size_t)wider_lds_doubles(P)), mem(wider_slot_doubles(P)) {
        W.bind_split(lds.data(), mem.data(), P);
    }
};
}  // namespace

extern "C" {

int hw_max_p() { return kWiderMaxP; }

int hw_mom(const int32_t* y, int ldn, const double* sf, const double* Xt, const double* pinvXt, int ldx, int N, int G,
           int P_, double min_disp, double max_disp, double min_mu, double* normed_mean, double* rough, double* moments,
           double* mom, double* mu) {
    if (P_ <= kWideMaxP || P_ > kWiderMaxP) return -1;
    HostSlot S(P_);
    double smi = 0.0;
    for (int n = 0; n < N; ++n) smi += 1.0 / sf[n];
    smi /= N;
    for (int g = 0; g < G; ++g) {
        MomOut o = mom_wide<HostWave>(y + (size_t)g * ldn, sf, Xt, pinvXt, ldx, N, S.W, smi, min_disp, max_disp, min_mu,
                                      mu ? mu + (size_t)g * ldn : nullptr);
        normed_mean[g] = o.normed_mean; rough[g] = o.rough; moments[g] = o.moments; mom[g] = o.mom;
    }
    return 0;
}

int hw_alpha_mle(const int32_t* y, const double* mu, int ldn, const double* Xt, int ldx, int N, int G, int P_,
                 const double* alpha_hat, double min_disp, double max_disp, double prior_var, int cr_reg, int prior_reg,
                 double* alpha, uint8_t* conv) {
    if (P_ <= kWideMaxP || P_ > kWiderMaxP) return -1;
    HostSlot S(P_);
    Lbfgsb1d mach;
    for (int g = 0; g < G; ++g) {
        AlphaOut o = fit_alpha_wide<HostWave>(y + (size_t)g * ldn, mu + (size_t)g * ldn, Xt, ldx, N, S.W, nullptr,
                                              alpha_hat[g], min_disp, max_disp, prior_var, cr_reg != 0, prior_reg != 0,
                                              mach, nullptr, nullptr);
        alpha[g] = o.alpha; conv[g] = (uint8_t)o.converged;
    }
    return 0;
}

int hw_lfc_fit(const int32_t* y, int ldn, const double* sf, const double* Xt, const double* pinvXt, int ldx, int N,
               int G, int P_, const double* disp, double min_mu, double beta_tol, int full_rank,
               const double* robust_disp, const uint8_t* flags, double cutoff, double* cooks, uint8_t* any_all,
               uint8_t* any_use, uint8_t* any_use_nr, uint8_t* few_above, const double* ridge, const double* contrast,
               double lfc_null, int alt, double* beta, double* mu, double* H, uint8_t* conv, double* pv, double* st,
               double* se, int maxiter) {
    if (P_ <= kWideMaxP || P_ > kWiderMaxP) return -1;
    HostSlot S(P_);
    std::vector<double> xlu(3 * kWiderMaxP);
    std::vector<int> nbd(kWiderMaxP);
    static LbfgsbWork<kWiderMaxP> Lb;
    for (int g = 0; g < G; ++g) {
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = nullptr; A.Xt = Xt; A.pinvXt = pinvXt; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = beta_tol; A.min_beta = -30.0; A.max_beta = 30.0;
        A.maxiter = maxiter; A.full_rank = full_rank != 0;
        LfcEpilogue E;
        if (flags != nullptr) {
            E.flags = flags; E.robust_disp = robust_disp[g]; E.cutoff = cutoff;
            E.cooks_row = cooks ? cooks + (size_t)g * ldn : nullptr;
        }
        if (ridge != nullptr) { E.ridge = ridge; E.contrast = contrast; E.lfc_null = lfc_null; E.alt = alt; }
        double* mo = mu ? mu + (size_t)g * ldn : nullptr;
        double* ho = H ? H + (size_t)g * ldn : nullptr;
        IrlsOut o = irls_gene_wide<HostWave>(A, S.W, mo, ho, &E);
        if (o.fallback) {
            std::memset(&Lb, 0, sizeof(Lb));
            o = irls_rescue_wide<HostWave>(A, S.W, Lb, xlu.data(), nbd.data(), mo, ho, &E);
        }
        for (int j = 0; j < P_; ++j) beta[(size_t)g * P_ + j] = S.W.v(0)[j];
        conv[g] = (uint8_t)o.converged;
        if (flags != nullptr) {
            any_all[g] = E.cooks.any_gt_all; any_use[g] = E.cooks.any_gt_use; any_use_nr[g] = E.cooks.any_gt_use_nr;
            few_above[g] = E.cooks.few_above;
        }
        if (ridge != nullptr) { pv[g] = E.wald.p; st[g] = E.wald.stat; se[g] = E.wald.se; }
    }
    return 0;
}

}  // extern "C"
