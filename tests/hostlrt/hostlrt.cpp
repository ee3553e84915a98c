// hostlrt.cpp — TEST-ONLY host instantiation of the likelihood-ratio templates (dsq_lrt.h).
// Built by tests/hostlrt/build.py with g++ and -ffp-contract=off into tests/hostlrt/_hostlrt.so, loaded only by tests.
//
// Two instantiations of the same template: HostWave (one lane walks every sample), and Lanes64 - the 64 lane-strided
// partial sums of a wavefront, added in the order of DeviceWave::sum's butterfly (partners 32, 16, 8, 4, 2, 1).  The
// sample loop of dsq_lrt.h holds single IEEE operations and explicit fmas only, so the second one reproduces the
// device's statistic bit for bit.
#include <cstdint>

#include "dsq_lrt.h"

using namespace dsq;

namespace {
struct Lanes64 {
    static constexpr int W = 64;
    static inline int cur = 0;
    static inline int lane() { return cur; }
};
}  // namespace

extern "C" {

int hl_chisq_sf(const double* x, int n, int df, double* out) {
    if (df < 1 || df > 127) return -1;
    for (int i = 0; i < n; ++i) out[i] = chisq_sf(x[i], df);
    return 0;
}

// wave64 != 0: the device's order of additions
int hl_lrt(const int32_t* y, int ldn, const double* sf, const double* Xf, int ldf, int Pf, const double* Xr, int ldr,
           int Pr, int N, int G, const double* disp, const double* beta_f, const double* beta_r, int wave64, double* stat,
           double* pval) {
    if (Pr < 1 || Pr >= Pf || Pf + Pr > kLrtMaxCoef) return -1;
    for (int g = 0; g < G; ++g) {
        const int32_t* yg = y + (size_t)g * ldn;
        const double* bf = beta_f + (size_t)g * Pf;
        const double* br = beta_r + (size_t)g * Pr;
        if (!wave64) {
            const LrtOut o = lrt_gene<HostWave>(yg, sf, Xf, ldf, Pf, Xr, ldr, Pr, bf, br, disp[g], N);
            stat[g] = o.stat; pval[g] = o.p;
            continue;
        }
        double v[64];
        for (int l = 0; l < 64; ++l) {
            Lanes64::cur = l;
            v[l] = lrt_lane_sum<Lanes64>(yg, sf, Xf, ldf, Pf, Xr, ldr, Pr, bf, br, 1.0 / disp[g], N);
        }
        for (int m = 32; m >= 1; m >>= 1) {
            double t[64];
            for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ m];
            for (int l = 0; l < 64; ++l) v[l] = t[l];
        }
        stat[g] = 2.0 * v[0];
        pval[g] = chisq_sf(stat[g], Pf - Pr);
    }
    return 0;
}

}  // extern "C"
