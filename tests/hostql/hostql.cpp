// hostql.cpp — TEST-ONLY host instantiation of the quasi-likelihood templates (dsq_ql.h).
// Built by tests/hostql/build.py with g++ and -ffp-contract=off into tests/hostql/_hostql.so, loaded only by tests.
//
// As tests/hostlrt: HostWave (one lane walks every sample), and Lanes64 - the 64 lane-strided partial sums of a
// wavefront, added in the order of DeviceWave::sum's butterfly (partners 32, 16, 8, 4, 2, 1), which reproduces the
// device's num, deviance and s2 bit for bit.
#include <cstdint>

#include "dsq_ql.h"

using namespace dsq;

namespace {
struct Lanes64 {
    static constexpr int W = 64;
    static inline int cur = 0;
    static inline int lane() { return cur; }
};

double butterfly(double* v) {
    for (int m = 32; m >= 1; m >>= 1) {
        double t[64];
        for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ m];
        for (int l = 0; l < 64; ++l) v[l] = t[l];
    }
    return v[0];
}
}  // namespace

extern "C" {

int hq_f_sf(const double* F, int n, int d1, double d2, double* out) {
    if (d1 < 1 || d1 > 127) return -1;
    for (int i = 0; i < n; ++i) out[i] = f_sf(F[i], d1, d2);
    return 0;
}

int hq_score(const double* num, const double* s2_post, int n, int df_test, double df_total, double* F, double* p) {
    if (df_test < 1 || df_test > 127) return -1;
    for (int i = 0; i < n; ++i) {
        const QlScore o = ql_score(num[i], s2_post[i], df_test, df_total);
        F[i] = o.F; p[i] = o.p;
    }
    return 0;
}

// twice nb_unit_deviance of each (y, mu, r): the unit deviance itself
int hq_unit_deviance(const double* y, const double* mu, const double* r, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = 2.0 * nb_unit_deviance(0.0, y[i], mu[i], mu[i] + r[i], r[i]);
    return 0;
}

// wave64 != 0: the device's order of additions
int hq_deviance(const int32_t* y, int ldn, const double* sf, const double* Xf, int ldf, int Pf, const double* Xr, int ldr,
                int Pr, int N, int G, const double* disp, const double* beta_f, const double* beta_r, int wave64,
                double* num, double* dev, double* s2) {
    if (Pr < 1 || Pr >= Pf || Pf + Pr > kLrtMaxCoef) return -1;
    const double df = (double)(N - Pf);
    for (int g = 0; g < G; ++g) {
        const int32_t* yg = y + (size_t)g * ldn;
        const double* bf = beta_f + (size_t)g * Pf;
        const double* br = beta_r + (size_t)g * Pr;
        if (!wave64) {
            const QlOut o = ql_gene<HostWave>(yg, sf, Xf, ldf, Pf, Xr, ldr, Pr, bf, br, disp[g], N, df);
            num[g] = o.num; dev[g] = o.dev; s2[g] = o.s2;
            continue;
        }
        double a[64], b[64];
        for (int l = 0; l < 64; ++l) {
            Lanes64::cur = l;
            const QlLane q = ql_lane_sums<Lanes64>(yg, sf, Xf, ldf, Pf, Xr, ldr, Pr, bf, br, 1.0 / disp[g], N);
            a[l] = q.num; b[l] = q.dev;
        }
        num[g] = 2.0 * butterfly(a);
        dev[g] = 2.0 * butterfly(b);
        s2[g] = dev[g] / df;
    }
    return 0;
}

}  // extern "C"
