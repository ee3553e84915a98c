// hostash.cpp — TEST-ONLY host instantiation of the adaptive-shrinkage templates (dsq_ash.h).
// Built by tests/hostash/build.py with g++ and -ffp-contract=off into tests/hostash/_hostash.so, loaded only by tests.
//
// ha_ash composes the pieces as k_ash_fit / k_ash_post do, with the waves of a workgroup stepped one after the other:
// nw = 1 is one wave that walks every chunk, nw = 4 the device's assignment of chunks to waves and its order of adding the
// waves' shares.  Inside a chunk the lanes are walked in order (HostWave); only WideGram's sums differ from the matrix
// cores' order of additions.
#include <cstdint>
#include <vector>

#include "dsq_ash.h"

using namespace dsq;

extern "C" {

int ha_ash(const double* lfc, const double* se, int G, int ldg, int K, const double* sd, const int32_t* mk, int ldm,
           int max_iter, int nw, double* pi, double* post_mean, double* post_sd, double* lfsr, int32_t* niter,
           uint8_t* conv, double* kkt, double* loglik, int32_t* passes) {
    if (K < 1 || G < 0 || ldg < G || max_iter < 1 || nw < 1 || nw > 8) return -1;
    for (int k = 0; k < K; ++k)
        if (mk[k] < 0 || mk[k] > kAshMaxM || ldm < mk[k]) return -1;
    for (int k = 0; k < K; ++k) {
        const int M = mk[k];
        if (G == 0 || M == 0) continue;
        const double* b = lfc + (size_t)k * ldg;
        const double* s = se + (size_t)k * ldg;
        const int wd = ash_wave_doubles(M, false);
        std::vector<double> mem((size_t)AshBlock::doubles(M, nw) + (size_t)nw * wd, 0.0);
        AshBlock B;
        B.bind(mem.data(), M, nw);
        double* wave_base = mem.data() + AshBlock::doubles(M, nw);
        std::vector<AshWave> Q(nw);
        int n = 0;
        for (int w = 0; w < nw; ++w) {
            Q[w].bind(wave_base + (size_t)w * wd, M, false);
            wide_zero_pad_rows<HostWave>(Q[w].W);
            n += ash_count<HostWave>(b, s, G, w, nw);
        }
        for (int m = 0; m < M; ++m) {
            const double v = sd[(size_t)k * ldm + m];
            B.sd2[m] = v * v;
            B.xt[m] = 1.0 / (double)M;
        }
        B.ctl[0] = 1;
        B.ctl[1] = 0;
        passes[k] = 0;
        if (n == 0) {
            for (int m = 0; m < M; ++m) pi[(size_t)k * ldm + m] = NAN;
            niter[k] = 0; conv[k] = 0; kkt[k] = NAN; loglik[k] = NAN;
        } else {
            AshState S;
            S.begin(n, max_iter);
            for (;;) {
                const bool gram = B.ctl[0] != 0;
                for (int w = 0; w < nw; ++w) ash_pass<HostWave>(B, Q[w], w, b, s, G, B.xt, S.inv_n, gram);
                ash_combine(B, Q[0].W.M, wd, gram, 0, 1);
                passes[k] += 1;
                if (ash_drive<HostWave>(B, S)) break;
            }
            const AshFit o = ash_result<HostWave>(B, S, n, pi + (size_t)k * ldm);
            niter[k] = o.n_iter; conv[k] = (uint8_t)o.converged; kkt[k] = o.kkt; loglik[k] = o.loglik;
        }
        for (int g = 0; g < G; ++g) {
            const size_t at = (size_t)k * ldg + g;
            ash_posterior(b[g], s[g], sd + (size_t)k * ldm, pi + (size_t)k * ldm, M, post_mean[at], post_sd[at], lfsr[at]);
        }
    }
    return 0;
}

}  // extern "C"
