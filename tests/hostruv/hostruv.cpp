// hostruv.cpp — TEST-ONLY host instantiation of the hidden-batch templates (dsq_proj.h).
// Built by tests/hostruv/build.py with g++ and -ffp-contract=off into tests/hostruv/_hostruv.so, loaded only by tests.
//
// The entry points take the arguments of the C ABI calls (dsq_dev_log_counts, dsq_dev_nb_residuals, dsq_project_plan,
// dsq_dev_project_out), refuse what those refuse and walk the genes as the kernels do, one "wave" of one lane (HostWave)
// per gene; the projection's host branch adds the 64 partial sums in the butterfly's order itself.  The staged copy of a
// row is allocated with exactly N doubles and the coefficients with exactly q, so an index outside either shows here.
#include <cmath>
#include <cstdint>
#include <vector>

#include "dsq_proj.h"

using namespace dsq;

extern "C" {

int hv_plan(int N, int* waves, int* staged, size_t* lds_bytes) {
    const ProjPlan p = proj_plan(N);
    *waves = p.waves;
    *staged = p.staged;
    *lds_bytes = p.lds_bytes;
    return p.waves > 0 ? 0 : -2;
}

int hv_log_counts(const int32_t* y, int ldn, const double* sf, int N, int G, int normalized, double eps, double* out,
                  int ld) {
    if (N < 1 || G < 0 || ldn < N || ld < N || !(std::isfinite(eps) && eps > 0.0)) return -2;
    if (G > 0 && (y == nullptr || (sf == nullptr && normalized))) return -2;
    for (int g = 0; g < G; ++g)
        log_counts_row<HostWave>(y + (size_t)g * ldn, sf, N, normalized != 0, eps, out + (size_t)g * ld);
    return 0;
}

int hv_nb_residuals(const int32_t* y, int ldn, const double* sf, const double* Xt, int ldx, int P, int N, int G,
                    const double* disp, const double* beta, int kind, double* out, int ld) {
    if (N < 1 || G < 0 || P < 1 || P > 128 || ldn < N || ldx < N || ld < N || !(kind == 0 || kind == 1)) return -2;
    for (int g = 0; g < G; ++g)
        nb_residuals_row<HostWave>(y + (size_t)g * ldn, sf, Xt, (size_t)ldx, P, beta + (size_t)g * P, disp[g], N, kind,
                                   out + (size_t)g * ld);
    return 0;
}

int hv_project_out(const double* x, int ld, const double* Pt, const double* Bt, int ldp, int q, int N, int G, int post,
                   double eps, double* out, int ldo, double* coef_out) {
    if (N < 1 || G < 0 || q < 1 || q > kProjMaxQ || ld < N || ldo < N || ldp < N || post < 0 || post > 2) return -2;
    if (post != 0 && !(std::isfinite(eps) && eps > 0.0)) return -2;
    if (out == x && ldo != ld) return -2;
    const ProjPlan plan = proj_plan(N);
    std::vector<double> row((size_t)(plan.staged == 1 ? N : 0)), coef((size_t)q);
    for (int g = 0; g < G; ++g) {
        double* co = coef_out != nullptr ? coef_out + (size_t)g * q : nullptr;
        if (plan.staged == 1)
            project_row<HostWave, true>(x + (size_t)g * ld, row.data(), Pt, Bt, (size_t)ldp, q, N, post, eps, coef.data(),
                                        out + (size_t)g * ldo, co);
        else
            project_row<HostWave, false>(x + (size_t)g * ld, nullptr, Pt, Bt, (size_t)ldp, q, N, post, eps, coef.data(),
                                         out + (size_t)g * ldo, co);
    }
    return 0;
}

}  // extern "C"
