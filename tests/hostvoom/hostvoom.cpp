// hostvoom.cpp — TEST-ONLY host instantiation of the voom row functions (dsq_voom.h).
// Built by tests/hostvoom/build.py with g++ and -ffp-contract=off into tests/hostvoom/_hostvoom.so, loaded only by tests.
//
// HostWave: one lane walks the chunk loops; every sum over the samples goes through voom_sums, whose host branch forms the
// 64 lane-strided partial sums of a wavefront and adds them in the order of DeviceWave::sum's butterfly.  That reproduces
// the device's beta1, Abar, sigma1 and the layers E and w bit for bit; the Gram matrix is summed sample by sample here and
// by the matrix cores there, so beta, sigma2, est and u agree within a bound only.
#include <cstdint>
#include <vector>

#include "dsq_voom.h"

using namespace dsq;

extern "C" {

int hv_lookup(const double* kx, const double* kf, int nk, const double* lam, int n, double* out) {
    if (nk < 2 || nk > kVoomMaxKnots) return -1;
    for (int i = 0; i < n; ++i) out[i] = voom_lookup(kx, kf, nk, lam[i]);
    return 0;
}

int hv_fit1(const int32_t* y, int ldn, const double* off, const double* Xt, const double* pinvXt, int ldx, int P, int N,
            int G, double* beta1, double* amean, double* sigma1) {
    if (P < 1 || P > kWideMaxP || N <= P) return -1;
    for (int g = 0; g < G; ++g) {
        const VoomFit1 o = voom_fit1_row<HostWave>(y + (size_t)g * ldn, off, Xt, pinvXt, (size_t)ldx, P, N,
                                                   beta1 + (size_t)g * P);
        amean[g] = o.amean;
        sigma1[g] = o.sigma;
    }
    return 0;
}

int hv_wls(const int32_t* y, int ldn, const double* off, const double* Xt, int ldx, int P, int N, int G,
           const double* beta1, const double* kx, const double* kf, int nk, const double* contrasts, int K, double* beta,
           double* sigma2, double* est, double* u, double* E, double* w, int ldl) {
    if (P < 1 || P > kWideMaxP || N <= P || K < 1 || nk < 2 || nk > kVoomMaxKnots) return -1;
    for (int i = 1; i < nk; ++i)
        if (!(kx[i] > kx[i - 1])) return -1;
    std::vector<double> mem((size_t)wide_work_doubles(P));
    WideWork W;
    W.bind(mem.data(), P);
    const double nan = __builtin_nan("");
    const bool layers = E != nullptr && w != nullptr;
    for (int g = 0; g < G; ++g) {
        bool bad = false;
        for (int j = 0; j < P; ++j) {
            W.v(2)[j] = beta1[(size_t)g * P + j];
            bad = bad || W.v(2)[j] != W.v(2)[j];
        }
        if (bad) {
            for (int j = 0; j < P; ++j) beta[(size_t)g * P + j] = nan;
            for (int k = 0; k < K; ++k) est[(size_t)g * K + k] = u[(size_t)g * K + k] = nan;
            sigma2[g] = nan;
            if (layers)
                for (int n = 0; n < N; ++n) E[(size_t)g * ldl + n] = w[(size_t)g * ldl + n] = nan;
            continue;
        }
        sigma2[g] = voom_wls_row<HostWave>(y + (size_t)g * ldn, off, Xt, ldx, N, W, kx, kf, nk, contrasts, K, true,
                                           est + (size_t)g * K, u + (size_t)g * K, layers ? E + (size_t)g * ldl : nullptr,
                                           layers ? w + (size_t)g * ldl : nullptr);
        for (int j = 0; j < P; ++j) beta[(size_t)g * P + j] = W.v(0)[j];
    }
    return 0;
}

}  // extern "C"
