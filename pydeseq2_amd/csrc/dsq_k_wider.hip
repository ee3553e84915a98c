// dsq_k_wider.hip — kernels of the designs wider than kWideMaxP = 48 columns (up to kWiderMaxP = 128, dsq_wider.h).
// The launch_wide_* entry points of dsq_k_wide.hip hand P > 48 to the launchers here, so every caller of the run-time-P
// path takes these designs without a change.  Persistent grid: one gene per 64-lane workgroup, as many workgroups as
// can be resident (LDS-bound), each looping over the genes g = blockIdx.x, blockIdx.x + gridDim.x, ... with its own slot
// of device memory for the p x p matrices.  A gene's result does not depend on the slot that ran it.  The design's
// cell structure is not used here (general Gram accumulation at any P).
#include <mutex>
#include <vector>

#include "dsq_dispatch.h"
#include "dsq_launch.h"
#include "dsq_wider.h"

namespace dsq {

namespace {

constexpr size_t kLdsPerCu = 160 * 1024;

// device-memory slots per (device, stream): grown on demand, released by wider_release when the stream's owner
// (dsq_destroy) is done with it; launches on one stream run one at a time, so a stream's slots have one user
struct SlotPool {
    int device;
    hipStream_t stream;
    double* p;
    size_t doubles;
};
std::mutex g_pool_mu;
std::vector<SlotPool> g_pools;

// slots for a launch of `want` workgroups whose LDS takes `lds_bytes` each; *n_slots <= want
hipError_t wider_slots(hipStream_t st, int P, size_t lds_bytes, int want, double** out, int* n_slots) {
    const int cus = current_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    size_t per_cu = kLdsPerCu / (lds_bytes + 1024);
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    int n = (int)(cus * per_cu);
    if (n > want) n = want;
    const size_t need = (size_t)n * wider_slot_doubles(P);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    SlotPool* sp = nullptr;
    for (SlotPool& q : g_pools)
        if (q.device == dev && q.stream == st) sp = &q;
    if (sp == nullptr) {
        g_pools.push_back(SlotPool{dev, st, nullptr, 0});
        sp = &g_pools.back();
    }
    if (sp->doubles < need) {
        if (sp->p != nullptr) {  // earlier launches on this stream may still use the old block
            e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
            (void)hipFree(sp->p);
            sp->p = nullptr;
            sp->doubles = 0;
        }
        e = hipMalloc((void**)&sp->p, need * sizeof(double));
        if (e != hipSuccess) { sp->p = nullptr; return e; }
        sp->doubles = need;
    }
    *out = sp->p;
    *n_slots = n;
    return hipSuccess;
}

template <class K>
void set_smem(K kernel, size_t bytes) {
    if (bytes > 48 * 1024) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        (void)hipGetLastError();
    }
}

size_t lds_bytes(int P) { return (size_t)wider_lds_doubles(P) * sizeof(double); }

}  // namespace

void wider_release(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pools.size();) {
        if (g_pools[i].device == dev && g_pools[i].stream == st) {
            if (g_pools[i].p != nullptr) {
                (void)hipStreamSynchronize(st);
                (void)hipFree(g_pools[i].p);
            }
            g_pools.erase(g_pools.begin() + i);
        } else {
            ++i;
        }
    }
}

#define DSQ_WIDER_BIND()                                                          \
    extern __shared__ __attribute__((aligned(16))) double wider_lds[];            \
    WiderWork W;                                                                  \
    W.bind_split(wider_lds, slots + (size_t)blockIdx.x * slot_doubles, P)

// ------------------------------------------------------------------ MoM (+ linear-model mu_hat, OLS coefficients)
__global__ __launch_bounds__(64) void k_mom_wider(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                  const double* __restrict__ Xt, const double* __restrict__ pinvXt,
                                                  int ldx, int N, int G, int P, double* __restrict__ slots,
                                                  size_t slot_doubles, const double* __restrict__ s_mean_inv,
                                                  double min_disp, double max_disp, double min_mu,
                                                  double* __restrict__ normed_mean, double* __restrict__ rough,
                                                  double* __restrict__ moments, double* __restrict__ mom,
                                                  double* __restrict__ mu, double* __restrict__ coef) {
    DSQ_WIDER_BIND();
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const MomOut o = mom_wide<SlotWave>(y + (size_t)g * ldn, sf, Xt, pinvXt, ldx, N, W, s_mean_inv[0], min_disp,
                                            max_disp, min_mu, mu ? mu + (size_t)g * ldn : nullptr);
        if (threadIdx.x == 0) {
            if (normed_mean) normed_mean[g] = o.normed_mean;
            if (rough) rough[g] = o.rough;
            if (moments) moments[g] = o.moments;
            if (mom) mom[g] = o.mom;
        }
        if (coef != nullptr)
            for (int j = threadIdx.x; j < P; j += 64) coef[(size_t)g * P + j] = W.v(0)[j];
        SlotWave::sync();
    }
}

hipError_t launch_wider_mom(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xt,
                            const double* pinvXt, int ldx, int N, int G, int P, double min_disp, double max_disp,
                            double min_mu, double* normed_mean, double* rough, double* moments, double* mom,
                            double* mu, double* coef, const double* d_s_mean_inv) {
    if (G <= 0) return hipSuccess;
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem, G, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_mom_wider, smem);
    hipLaunchKernelGGL(k_mom_wider, dim3(n), dim3(64), smem, st, y, ldn, sf, Xt, pinvXt, ldx, N, G, P, slots,
                       wider_slot_doubles(P), d_s_mean_inv, min_disp, max_disp, min_mu, normed_mean, rough, moments,
                       mom, mu, coef);
    return hipGetLastError();
}

// rough dispersions from already-normalised counts (Inference.fit_rough_dispersions); as k_rough_normed_wide
__global__ __launch_bounds__(64) void k_rough_normed_wider(const double* __restrict__ normed, int ldn,
                                                           const double* __restrict__ Xt,
                                                           const double* __restrict__ pinvXt, int ldx, int N, int G,
                                                           int P, double* __restrict__ slots, size_t slot_doubles,
                                                           double* __restrict__ out) {
    DSQ_WIDER_BIND();
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const double* v = normed + (size_t)g * ldn;
        for (int j = 0; j < P; ++j) {
            double b = 0.0;
            for (int n = SlotWave::lane(); n < N; n += 64) b += pinvXt[j * ldx + n] * v[n];
            b = SlotWave::sum(b);
            if (threadIdx.x == 0) W.v(0)[j] = b;
        }
        SlotWave::sync();
        double rr = 0.0;
        const double dof = (double)(N - P);
        for (int n = SlotWave::lane(); n < N; n += 64) {
            double yh = 0.0;
            for (int j = 0; j < P; ++j) yh += Xt[j * ldx + n] * W.v(0)[j];
            yh = dmax(yh, 1.0);
            rr += ((v[n] - yh) * (v[n] - yh) - yh) / (dof * yh * yh);
        }
        rr = SlotWave::sum(rr);
        if (threadIdx.x == 0) out[g] = dmax(rr, 0.0);
        SlotWave::sync();
    }
}

hipError_t launch_wider_rough_normed(hipStream_t st, const double* normed, int ldn, const double* Xt,
                                     const double* pinvXt, int ldx, int N, int G, int P, double* out) {
    if (G <= 0) return hipSuccess;
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem, G, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_rough_normed_wider, smem);
    hipLaunchKernelGGL(k_rough_normed_wider, dim3(n), dim3(64), smem, st, normed, ldn, Xt, pinvXt, ldx, N, G, P, slots,
                       wider_slot_doubles(P), out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ dispersion fit (genes 0..G-1, or list[0..G-1])
__global__ __launch_bounds__(64) void k_alpha_wider(const int32_t* __restrict__ y, const double* __restrict__ mu,
                                                    int ldn, const double* __restrict__ Xt, int ldx, int N, int G,
                                                    int P, double* __restrict__ slots, size_t slot_doubles,
                                                    const double* __restrict__ alpha_hat, double min_disp,
                                                    double max_disp, double prior_var, int cr_reg, int prior_reg,
                                                    double* __restrict__ alpha, uint8_t* __restrict__ conv,
                                                    int32_t* __restrict__ nfev, double* __restrict__ nll_const,
                                                    int const_mode) {
    __shared__ Lbfgsb1d machine;
    log_tab_fill();  // the count memo takes its logarithms through the LDS table (flog_t, dsq_math.h)
    __syncthreads();
    DSQ_WIDER_BIND();
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const AlphaOut o = fit_alpha_wide<SlotWave>(
            y + (size_t)g * ldn, mu + (size_t)g * ldn, Xt, ldx, N, W, nullptr, alpha_hat[g], min_disp, max_disp,
            prior_var, cr_reg != 0, prior_reg != 0, machine, const_mode == DSQ_CONST_LOAD ? nll_const + g : nullptr,
            const_mode == DSQ_CONST_STORE ? nll_const + g : nullptr);
        if (threadIdx.x == 0) {
            alpha[g] = o.alpha;
            conv[g] = (uint8_t)o.converged;
            if (nfev != nullptr) nfev[g] = o.nfev;
        }
        SlotWave::sync();
    }
}

// grid_fit_alpha alone for listed genes: alpha[list[k]] = exp(best grid point); as k_alpha_grid_wide
__global__ __launch_bounds__(64) void k_alpha_grid_wider(const int32_t* __restrict__ y, const double* __restrict__ mu,
                                                         int ldn, const double* __restrict__ Xt, int ldx, int N, int P,
                                                         double* __restrict__ slots, size_t slot_doubles,
                                                         double min_disp, double max_disp, double* __restrict__ alpha,
                                                         const int32_t* __restrict__ list, int n_list) {
    log_tab_fill();
    __syncthreads();
    DSQ_WIDER_BIND();
    for (int k = blockIdx.x; k < n_list; k += gridDim.x) {
        const int g = list[k];
        WideAlphaArgs A;
        A.y = y + (size_t)g * ldn; A.mu = mu + (size_t)g * ldn; A.Xt = Xt; A.ldx = ldx; A.N = N; A.cells = nullptr;
        A.la_hat = 0.0; A.prior_var = 1.0;
        A.cst = alpha_const<SlotWave>(A.y, A.mu, N);
        double lohi[2] = {log(min_disp), log(max_disp)};
        double best_la = 0.0;
        for (int level = 0; level < 2; ++level) {
            double best = 0.0;
            int kbest = 0;
            bool best_nan = false;
            for (int i = 0; i < 100; ++i) {
                double f, gu;
                alpha_eval_wide<SlotWave, false>(A, W, linspace_at(lohi[0], lohi[1], 100, i), true, false, f, gu);
                const bool isn = (f != f);
                if (i == 0 || (!best_nan && (isn || f < best))) { best = f; kbest = i; best_nan = isn; }
            }
            const double c = linspace_at(lohi[0], lohi[1], 100, kbest);
            const double delta = linspace_at(lohi[0], lohi[1], 100, 1) - linspace_at(lohi[0], lohi[1], 100, 0);
            best_la = c;
            lohi[0] = c - delta; lohi[1] = c + delta;
        }
        if (threadIdx.x == 0) alpha[g] = exp(best_la);
        SlotWave::sync();
    }
}

hipError_t launch_wider_alpha(hipStream_t st, const int32_t* y, const double* mu, int ldn, const double* Xt, int ldx,
                              int N, int G, int P, const double* alpha_hat, double min_disp, double max_disp,
                              double prior_var, int cr_reg, int prior_reg, double* alpha, uint8_t* conv,
                              int32_t* nfev, double* nll_const, int const_mode) {
    if (G <= 0) return hipSuccess;
    if (nll_const == nullptr) const_mode = DSQ_CONST_COMPUTE;
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem + 2 * kLogTabN * sizeof(double) + sizeof(Lbfgsb1d), G, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_alpha_wider, smem);
    hipLaunchKernelGGL(k_alpha_wider, dim3(n), dim3(64), smem, st, y, mu, ldn, Xt, ldx, N, G, P, slots,
                       wider_slot_doubles(P), alpha_hat, min_disp, max_disp, prior_var, cr_reg, prior_reg, alpha, conv,
                       nfev, nll_const, const_mode);
    return hipGetLastError();
}

hipError_t launch_wider_alpha_grid(hipStream_t st, const int32_t* y, const double* mu, int ldn, const double* Xt,
                                   int ldx, int N, int P, double min_disp, double max_disp, double* alpha,
                                   const int32_t* list, int n_list) {
    if (n_list <= 0) return hipSuccess;
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem + 2 * kLogTabN * sizeof(double), n_list, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_alpha_grid_wider, smem);
    hipLaunchKernelGGL(k_alpha_grid_wider, dim3(n), dim3(64), smem, st, y, mu, ldn, Xt, ldx, N, P, slots,
                       wider_slot_doubles(P), min_disp, max_disp, alpha, list, n_list);
    return hipGetLastError();
}

// ------------------------------------------------------------------ IRLS (+ fused epilogue), rescue, layers, Wald
namespace {
__device__ __forceinline__ void wider_epilogue_begin(LfcEpilogue& E, const IrlsExtras& ex, int g, int ldn) {
    if (ex.flags != nullptr) {
        E.flags = ex.flags; E.robust_disp = ex.robust_disp[g]; E.cutoff = ex.cutoff;
        E.cooks_row = ex.cooks ? ex.cooks + (size_t)g * ldn : nullptr;
    }
    if (ex.ridge != nullptr) { E.ridge = ex.ridge; E.contrast = ex.contrast; E.lfc_null = ex.lfc_null; E.alt = ex.alt; }
}
__device__ __forceinline__ void wider_epilogue_store(const LfcEpilogue& E, const IrlsExtras& ex, int g) {
    if (ex.flags != nullptr) {
        ex.any_all[g] = (uint8_t)E.cooks.any_gt_all;
        ex.any_use[g] = (uint8_t)E.cooks.any_gt_use;
        ex.any_use_nr[g] = (uint8_t)E.cooks.any_gt_use_nr;
        ex.few_above[g] = (uint8_t)E.cooks.few_above;
    }
    if (ex.ridge != nullptr) { ex.pvals[g] = E.wald.p; ex.stats[g] = E.wald.stat; ex.se[g] = E.wald.se; }
}
}  // namespace

__global__ __launch_bounds__(64) void k_irls_wider(const int32_t* __restrict__ y, int ldn, const double* __restrict__ sf,
                                                   const double* __restrict__ lsf, const double* __restrict__ Xt,
                                                   const double* __restrict__ pinvXt, int ldx, int N, int G, int P,
                                                   double* __restrict__ slots, size_t slot_doubles, int full_rank,
                                                   const double* __restrict__ disp, double min_mu, double beta_tol,
                                                   double min_beta, double max_beta, int maxiter,
                                                   double* __restrict__ beta, double* __restrict__ mu,
                                                   double* __restrict__ hat, uint8_t* __restrict__ conv,
                                                   int32_t* __restrict__ iters, int32_t* __restrict__ fb_count,
                                                   int32_t* __restrict__ fb_list, IrlsExtras ex) {
    DSQ_WIDER_BIND();
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = lsf; A.Xt = Xt; A.pinvXt = pinvXt; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = beta_tol; A.min_beta = min_beta; A.max_beta = max_beta;
        A.maxiter = maxiter; A.full_rank = full_rank != 0;
        LfcEpilogue E;
        wider_epilogue_begin(E, ex, g, ldn);
        const IrlsOut o = irls_gene_wide<SlotWave>(A, W, mu ? mu + (size_t)g * ldn : nullptr,
                                                   hat ? hat + (size_t)g * ldn : nullptr, &E);
        if (!o.fallback)
            for (int j = threadIdx.x; j < P; j += 64) beta[(size_t)g * P + j] = W.v(0)[j];
        if (threadIdx.x == 0) {
            conv[g] = (uint8_t)o.converged;
            if (iters != nullptr) iters[g] = o.iters;
            if (o.fallback) fb_list[atomicAdd(fb_count, 1)] = g;
            else wider_epilogue_store(E, ex, g);
        }
        SlotWave::sync();
    }
}

__global__ __launch_bounds__(64) void k_irls_rescue_wider(const int32_t* __restrict__ y, int ldn,
                                                          const double* __restrict__ sf, const double* __restrict__ lsf,
                                                          const double* __restrict__ Xt,
                                                          const double* __restrict__ pinvXt, int ldx, int N, int P,
                                                          double* __restrict__ slots, size_t slot_doubles,
                                                          int full_rank, const double* __restrict__ disp,
                                                          double min_mu, double beta_tol, double min_beta,
                                                          double max_beta, int maxiter, double* __restrict__ beta,
                                                          double* __restrict__ mu, double* __restrict__ hat,
                                                          uint8_t* __restrict__ conv, int32_t* __restrict__ iters,
                                                          const int32_t* __restrict__ fb_list, int n_fb,
                                                          IrlsExtras ex) {
    __shared__ LbfgsbWork<kWiderMaxP> Lb;
    __shared__ double xlu[3 * kWiderMaxP];
    __shared__ int nbd[kWiderMaxP];
    DSQ_WIDER_BIND();
    for (int k = blockIdx.x; k < n_fb; k += gridDim.x) {
        const int g = fb_list[k];
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = lsf; A.Xt = Xt; A.pinvXt = pinvXt; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = beta_tol; A.min_beta = min_beta; A.max_beta = max_beta;
        A.maxiter = maxiter; A.full_rank = full_rank != 0;
        // beta_init of the gene (the first kernel's W is gone): recompute as irls_gene_wide does
        for (int j = 0; j < P; ++j) {
            double b0 = 0.0;
            for (int n = SlotWave::lane(); n < N; n += 64) {
                const double yv = (double)A.y[n];
                if (A.full_rank) b0 += pinvXt[j * ldx + n] * log(yv / sf[n] + 0.1);
                else if (j == 0) b0 += log(yv / sf[n]);
            }
            b0 = SlotWave::sum(b0);
            if (!A.full_rank) b0 = j == 0 ? b0 / (double)N : 0.0;
            if (threadIdx.x == 0) W.v(2)[j] = b0;
        }
        SlotWave::sync();
        LfcEpilogue E;
        wider_epilogue_begin(E, ex, g, ldn);
        if (ex.cooks_ld != 0 && E.cooks_row != nullptr) E.cooks_row = ex.cooks_tmp + (size_t)k * ldn;  // (see k_irls_rescue)
        const IrlsOut o = irls_rescue_wide<SlotWave>(A, W, Lb, xlu, nbd, mu ? mu + (size_t)g * ldn : nullptr,
                                                     hat ? hat + (size_t)g * ldn : nullptr, &E);
        for (int j = threadIdx.x; j < P; j += 64) beta[(size_t)g * P + j] = W.v(0)[j];
        if (threadIdx.x == 0) {
            conv[g] = (uint8_t)o.converged;
            if (iters != nullptr) iters[g] = o.iters;
            wider_epilogue_store(E, ex, g);
        }
        SlotWave::sync();
    }
}

hipError_t launch_wider_irls(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* lsf,
                             const double* Xt, const double* pinvXt, int ldx, int N, int G, int P, int full_rank,
                             const double* disp, double min_mu, double beta_tol, double min_beta, double max_beta,
                             int maxiter, double* beta, double* mu, double* hat, uint8_t* conv, int32_t* iters,
                             int32_t* fb_count, int32_t* fb_list, const IrlsExtras* extras) {
    if (G <= 0) return hipSuccess;
    IrlsExtras ex{};
    if (extras != nullptr) ex = *extras;
    ex.cells = CellDesign{};
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem, G, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_irls_wider, smem);
    hipLaunchKernelGGL(k_irls_wider, dim3(n), dim3(64), smem, st, y, ldn, sf, lsf, Xt, pinvXt, ldx, N, G, P, slots,
                       wider_slot_doubles(P), full_rank, disp, min_mu, beta_tol, min_beta, max_beta, maxiter, beta, mu,
                       hat, conv, iters, fb_count, fb_list, ex);
    return hipGetLastError();
}

hipError_t launch_wider_irls_rescue(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* lsf,
                                    const double* Xt, const double* pinvXt, int ldx, int N, int P, int full_rank,
                                    const double* disp, double min_mu, double beta_tol, double min_beta,
                                    double max_beta, int maxiter, double* beta, double* mu, double* hat, uint8_t* conv,
                                    int32_t* iters, const int32_t* fb_list, int n_fb, const IrlsExtras* extras) {
    if (n_fb <= 0) return hipSuccess;
    IrlsExtras ex{};
    if (extras != nullptr) ex = *extras;
    ex.cells = CellDesign{};
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    const size_t stat = sizeof(LbfgsbWork<kWiderMaxP>) + 3 * kWiderMaxP * sizeof(double) + kWiderMaxP * sizeof(int);
    hipError_t e = wider_slots(st, P, smem + stat, n_fb, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_irls_rescue_wider, smem);
    hipLaunchKernelGGL(k_irls_rescue_wider, dim3(n), dim3(64), smem, st, y, ldn, sf, lsf, Xt, pinvXt, ldx, N, P, slots,
                       wider_slot_doubles(P), full_rank, disp, min_mu, beta_tol, min_beta, max_beta, maxiter, beta, mu,
                       hat, conv, iters, fb_list, n_fb, ex);
    return hipGetLastError();
}

// layers (mu, hat) of a finished fit from beta
__global__ __launch_bounds__(64) void k_irls_layers_wider(const int32_t* __restrict__ y, int ldn,
                                                          const double* __restrict__ sf, const double* __restrict__ Xt,
                                                          int ldx, int N, int G, int P, double* __restrict__ slots,
                                                          size_t slot_doubles, const double* __restrict__ disp,
                                                          const double* __restrict__ beta, double min_mu,
                                                          double* __restrict__ mu, double* __restrict__ hat) {
    DSQ_WIDER_BIND();
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = nullptr; A.Xt = Xt; A.pinvXt = nullptr; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = 0.0; A.min_beta = 0.0; A.max_beta = 0.0; A.maxiter = 0;
        A.full_rank = false;
        for (int j = threadIdx.x; j < P; j += 64) W.v(0)[j] = beta[(size_t)g * P + j];
        SlotWave::sync();
        double S;
        irls_sweep_wide<SlotWave>(A, W, 1.0 / A.disp, S);
        irls_finish_wide<SlotWave>(A, W, mu ? mu + (size_t)g * ldn : nullptr, hat ? hat + (size_t)g * ldn : nullptr,
                                   nullptr);
        SlotWave::sync();
    }
}

hipError_t launch_wider_irls_layers(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xt,
                                    int ldx, int N, int G, int P, const double* disp, const double* beta,
                                    double min_mu, double* mu, double* hat) {
    if (G <= 0) return hipSuccess;
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem, G, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_irls_layers_wider, smem);
    hipLaunchKernelGGL(k_irls_layers_wider, dim3(n), dim3(64), smem, st, y, ldn, sf, Xt, ldx, N, G, P, slots,
                       wider_slot_doubles(P), disp, beta, min_mu, mu, hat);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void k_wald_wider(const double* __restrict__ mu, int ldn,
                                                   const double* __restrict__ sf, const double* __restrict__ Xt,
                                                   int ldx, int N, int G, int P, double* __restrict__ slots,
                                                   size_t slot_doubles, const double* __restrict__ disp,
                                                   const double* __restrict__ beta, const double* __restrict__ ridge,
                                                   const double* __restrict__ contrast, double lfc_null, int alt,
                                                   double* __restrict__ pvals, double* __restrict__ stats,
                                                   double* __restrict__ se) {
    DSQ_WIDER_BIND();
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        for (int j = threadIdx.x; j < P; j += 64) W.v(0)[j] = beta[(size_t)g * P + j];
        SlotWave::sync();
        const WaldOut o = wald_gene_wide<SlotWave>(mu ? mu + (size_t)g * ldn : nullptr, sf, Xt, ldx, N, disp[g], W,
                                                   ridge, contrast, lfc_null, alt);
        if (threadIdx.x == 0) {
            pvals[g] = o.p;
            stats[g] = o.stat;
            se[g] = o.se;
        }
        SlotWave::sync();
    }
}

hipError_t launch_wider_wald(hipStream_t st, const double* mu, int ldn, const double* sf, const double* Xt, int ldx,
                             int N, int G, int P, const double* disp, const double* beta, const double* d_ridge,
                             const double* d_contrast, double lfc_null, int alt, double* pvals, double* stats,
                             double* se) {
    if (G <= 0) return hipSuccess;
    const size_t smem = lds_bytes(P);
    double* slots;
    int n;
    hipError_t e = wider_slots(st, P, smem, G, &slots, &n);
    if (e != hipSuccess) return e;
    set_smem(k_wald_wider, smem);
    hipLaunchKernelGGL(k_wald_wider, dim3(n), dim3(64), smem, st, mu, ldn, sf, Xt, ldx, N, G, P, slots,
                       wider_slot_doubles(P), disp, beta, d_ridge, d_contrast, lfc_null, alt, pvals, stats, se);
    return hipGetLastError();
}

}  // namespace dsq
