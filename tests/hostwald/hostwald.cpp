// hostwald.cpp — TEST-ONLY host instantiation of the multi-contrast Wald templates: wald_gene_multi<HostWave, P>
// (dsq_stats.h, P = 1 ... 12) and wald_gene_multi_wide<HostWave> (dsq_wide.h) over both workspaces of the run-time-P
// path (WideWork up to 48 columns, WiderWork beyond, bound as the device kernels bind them).
// Built by tests/hostwald/build.py with g++ and -ffp-contract=off into tests/hostwald/_hostwald.so, loaded only by tests.
#include <cstdint>
#include <vector>

#include "dsq_dispatch.h"
#include "dsq_stats.h"
#include "dsq_wider.h"

using namespace dsq;

namespace {

template <int P>
void reg_gene(const double* mu, const double* sf, const double* Xt, int ldx, int N, double disp, const double* beta,
              const double* ridge, const double* contrasts, int K, double lfc_null, int alt, double* pv, double* st,
              double* se) {
    double b[P];
    for (int j = 0; j < P; ++j) b[j] = beta[j];
    wald_gene_multi<HostWave, P>(mu, sf, Xt, ldx, N, disp, b, ridge, contrasts, K, lfc_null, alt, pv, st, se);
}

template <class Work>
void wide_genes(const Work& W, const double* mu, int ldn, const double* sf, const double* Xt, int ldx, int N, int G,
                const double* disp, const double* beta, const double* ridge, const double* contrasts, int K,
                double lfc_null, int alt, double* pv, double* st, double* se) {
    const int P = W.P;
    for (int g = 0; g < G; ++g) {
        for (int j = 0; j < P; ++j) W.v(0)[j] = beta[(size_t)g * P + j];
        const size_t o = (size_t)g * K;
        wald_gene_multi_wide<HostWave>(mu ? mu + (size_t)g * ldn : nullptr, sf, Xt, ldx, N, disp[g], W, ridge, contrasts,
                                       K, lfc_null, alt, true, pv + o, st + o, se + o);
    }
}

}  // namespace

extern "C" {

// mu [G][ldn] or null (then sf is used); contrasts [K][P]; outputs [G][K].  wide != 0: the run-time-P templates at
// any P <= 128 (otherwise P <= 12: the register templates)
int hwm_wald_multi(const double* mu, int ldn, const double* sf, const double* Xt, int ldx, int N, int G, int P_,
                   const double* disp, const double* beta, const double* ridge, const double* contrasts, int K,
                   double lfc_null, int alt, int wide, double* pv, double* st, double* se) {
    if (K < 1 || P_ < 1 || alt < 0 || alt > 4) return -1;
    if (!wide) {
        if (P_ > DSQ_REG_MAX_P) return -1;
        for (int g = 0; g < G; ++g) {
            const size_t o = (size_t)g * K;
            DSQ_DISPATCH_P(P_, reg_gene<P>(mu ? mu + (size_t)g * ldn : nullptr, sf, Xt, ldx, N, disp[g],
                                           beta + (size_t)g * P_, ridge, contrasts, K, lfc_null, alt, pv + o, st + o,
                                           se + o))
        }
        return 0;
    }
    if (P_ > kWiderMaxP) return -1;
    if (P_ <= kWideMaxP) {
        std::vector<double> lds((size_t)wide_work_doubles(P_));
        WideWork W;
        W.bind(lds.data(), P_);
        wide_genes(W, mu, ldn, sf, Xt, ldx, N, G, disp, beta, ridge, contrasts, K, lfc_null, alt, pv, st, se);
    } else {
        std::vector<double> lds((size_t)wider_lds_doubles(P_)), mem(wider_slot_doubles(P_));
        WiderWork W;
        W.bind_split(lds.data(), mem.data(), P_);
        wide_genes(W, mu, ldn, sf, Xt, ldx, N, G, disp, beta, ridge, contrasts, K, lfc_null, alt, pv, st, se);
    }
    return 0;
}

}  // extern "C"
