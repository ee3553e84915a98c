// dsq_k_wide.hip — kernels of the run-time-P path (dsq_wide.h, dsq_wider.h): designs wider than the register path's 12
// columns, up to kWiderMaxP = 128, and — optionally — narrower designs without cell structure, whose p(p+1) register
// accumulators spill.  Every kernel and every launcher is written once, over one of two geometry policies:
//   * LdsGeom  (P <= kWideMaxP = 48): one gene per wavefront; the wave's p x p matrices, the staged design chunk and the
//     small vectors live in a wave-private segment of dynamic LDS whose size follows P (1, 2 or 4 waves per workgroup);
//   * SlotGeom (P = 49 ... 128): persistent grid, one gene per 64-lane workgroup, as many workgroups as can be resident
//     (LDS-bound), each looping over the genes g = blockIdx.x, blockIdx.x + gridDim.x, ... with its own slot of device
//     memory for the p x p matrices.  A gene's result does not depend on the slot that ran it.  The design's cell
//     structure is not used (general Gram accumulation at any P).
// X^T W X is accumulated by v_mfma_f64_16x16x4_f64 (or from per-cell sums for cell designs).
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

// ------------------------------------------------------------------ the two geometries
// All that differs between the families.  A kernel binds its workspace once (work) and hands the body of one gene to
// each(n, body), which runs it for the wave's items k < n.  plan (host) shapes a launch over `items` items: grid, block,
// dynamic LDS and the policy object the kernel gets.  Two constraints, both checked with tools/kernel_resources.py
// (k_irls_layers_wide shows either at once: 128 VGPR for LdsGeom, 96 for SlotGeom):
//   * LdsGeom::each carries no loop, not even one whose step the compiler folds;
//   * the policy is the kernels' LAST argument.
struct WideLaunch {
    int grid, block;
    size_t smem;
};

struct LdsGeom {
    using Wave = DeviceWave;
    using Work = WideWork;
    static constexpr int kThreads = 256;  // launch bound
    static constexpr int kWaves = 4;      // waves (genes) per workgroup at most
    static constexpr bool kCells = true;  // k_irls_wide takes the design's cells when the launcher passes them
    int per_wave_doubles;

    static __device__ __forceinline__ int wave() { return threadIdx.x >> 6; }
    static __device__ __forceinline__ bool lane0() { return (threadIdx.x & 63) == 0; }
    __device__ __forceinline__ Work work(int P) const {
        extern __shared__ __attribute__((aligned(16))) double wide_lds[];
        Work W;
        W.bind(wide_lds + (size_t)wave() * per_wave_doubles, P);
        return W;
    }
    // item(k) for the wave's items k < n: it has one
    template <class F>
    static __device__ __forceinline__ void each(int n, F item) {
        const int k = blockIdx.x * (blockDim.x >> 6) + wave();
        if (k < n) item(k);
    }

    // as many waves per workgroup (4, 2 or 1, at most max_waves) as fit 64 KB of LDS
    static hipError_t plan(hipStream_t, int P, int items, size_t, int max_waves, WideLaunch& L, LdsGeom& geo) {
        const size_t per_wave = (size_t)wide_work_doubles(P) * sizeof(double);
        int wpb = per_wave * 4 <= 64 * 1024 ? 4 : (per_wave * 2 <= 64 * 1024 ? 2 : 1);
        if (wpb > max_waves) wpb = max_waves;
        L.grid = (items + wpb - 1) / wpb;
        L.block = 64 * wpb;
        L.smem = per_wave * wpb;
        geo.per_wave_doubles = (int)(per_wave / 8);
        return hipSuccess;
    }
};

struct SlotGeom {
    using Wave = SlotWave;
    using Work = WiderWork;
    static constexpr int kThreads = 64;
    static constexpr int kWaves = 1;
    static constexpr bool kCells = false;
    double* slots;
    size_t slot_doubles;

    static __device__ __forceinline__ int wave() { return 0; }
    static __device__ __forceinline__ bool lane0() { return threadIdx.x == 0; }
    __device__ __forceinline__ Work work(int P) const {
        extern __shared__ __attribute__((aligned(16))) double wide_lds[];
        Work W;
        W.bind_split(wide_lds, slots + (size_t)blockIdx.x * slot_doubles, P);
        return W;
    }
    // persistent grid; the barrier keeps the next gene's writes to the slot behind this gene's reads
    template <class F>
    static __device__ __forceinline__ void each(int n, F item) {
        for (int k = blockIdx.x; k < n; k += gridDim.x) {
            item(k);
            SlotWave::sync();
        }
    }

    // as many workgroups as can be resident with the kernel's static_lds besides the dynamic LDS, a slot each
    static hipError_t plan(hipStream_t st, int P, int items, size_t static_lds, int, WideLaunch& L, SlotGeom& geo) {
        L.block = 64;
        L.smem = (size_t)wider_lds_doubles(P) * sizeof(double);
        geo.slot_doubles = wider_slot_doubles(P);
        return wider_slots(st, P, L.smem + static_lds, items, &geo.slots, &L.grid);
    }
};

namespace {

// kernel(args..., geo) over `items` items; static_lds: the kernel's static LDS
template <class Geo, class K, class... Args>
hipError_t wide_run(Geo geo, K kernel, hipStream_t st, int P, int items, size_t static_lds, int max_waves,
                    Args... args) {
    WideLaunch L;
    const hipError_t e = Geo::plan(st, P, items, static_lds, max_waves, L, geo);
    if (e != hipSuccess) return e;
    set_smem(kernel, L.smem);
    hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(L.block), L.smem, st, args..., geo);
    return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------ MoM (+ linear-model mu_hat, OLS coefficients)
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_mom_wide(const int32_t* __restrict__ y, int ldn,
                                                            const double* __restrict__ sf,
                                                            const double* __restrict__ Xt,
                                                            const double* __restrict__ pinvXt, int ldx, int N, int G,
                                                            int P, const double* __restrict__ s_mean_inv,
                                                            double min_disp, double max_disp, double min_mu,
                                                            double* __restrict__ normed_mean,
                                                            double* __restrict__ rough,
                                                            double* __restrict__ moments, double* __restrict__ mom,
                                                            double* __restrict__ mu, double* __restrict__ coef,
                                                            Geo geo) {
    using Wv = typename Geo::Wave;
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        const MomOut o = mom_wide<Wv>(y + (size_t)g * ldn, sf, Xt, pinvXt, ldx, N, W, s_mean_inv[0], min_disp, max_disp,
                                      min_mu, mu ? mu + (size_t)g * ldn : nullptr);
        if (Geo::lane0()) {
            if (normed_mean) normed_mean[g] = o.normed_mean;
            if (rough) rough[g] = o.rough;
            if (moments) moments[g] = o.moments;
            if (mom) mom[g] = o.mom;
        }
        if (coef != nullptr)
            for (int j = Wv::lane(); j < P; j += 64) coef[(size_t)g * P + j] = W.v(0)[j];
    });
}

hipError_t launch_wide_mom(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xt,
                           const double* pinvXt, int ldx, int N, int G, int P, double min_disp, double max_disp,
                           double min_mu, double* normed_mean, double* rough, double* moments, double* mom,
                           double* mu, double* coef, const double* d_s_mean_inv) {
    if (G <= 0) return hipSuccess;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_mom_wide<decltype(geo)>, st, P, G, 0, LdsGeom::kWaves, y, ldn, sf, Xt, pinvXt, ldx, N, G,
                        P, d_s_mean_inv, min_disp, max_disp, min_mu, normed_mean, rough, moments, mom, mu, coef);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

// rough dispersions from already-normalised counts (Inference.fit_rough_dispersions)
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_rough_normed_wide(const double* __restrict__ normed,
                                                                     int ldn, const double* __restrict__ Xt,
                                                                     const double* __restrict__ pinvXt, int ldx, int N,
                                                                     int G, int P, double* __restrict__ out, Geo geo) {
    using Wv = typename Geo::Wave;
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        const double* v = normed + (size_t)g * ldn;
        for (int j = 0; j < P; ++j) {
            double b = 0.0;
            for (int n = Wv::lane(); n < N; n += 64) b += pinvXt[j * ldx + n] * v[n];
            b = Wv::sum(b);
            if (Geo::lane0()) W.v(0)[j] = b;
        }
        Wv::sync();
        double rr = 0.0;
        const double dof = (double)(N - P);
        for (int n = Wv::lane(); n < N; n += 64) {
            double yh = 0.0;
            for (int j = 0; j < P; ++j) yh += Xt[j * ldx + n] * W.v(0)[j];
            yh = dmax(yh, 1.0);
            rr += ((v[n] - yh) * (v[n] - yh) - yh) / (dof * yh * yh);
        }
        rr = Wv::sum(rr);
        if (Geo::lane0()) out[g] = dmax(rr, 0.0);
    });
}

hipError_t launch_wide_rough_normed(hipStream_t st, const double* normed, int ldn, const double* Xt,
                                    const double* pinvXt, int ldx, int N, int G, int P, double* out) {
    if (G <= 0) return hipSuccess;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_rough_normed_wide<decltype(geo)>, st, P, G, 0, LdsGeom::kWaves, normed, ldn, Xt, pinvXt,
                        ldx, N, G, P, out);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

// ------------------------------------------------------------------ dispersion fit
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_alpha_wide(const int32_t* __restrict__ y,
                                                              const double* __restrict__ mu, int ldn,
                                                              const double* __restrict__ Xt, int ldx, int N, int G,
                                                              int P, const double* __restrict__ alpha_hat,
                                                              double min_disp, double max_disp, double prior_var,
                                                              int cr_reg, int prior_reg, double* __restrict__ alpha,
                                                              uint8_t* __restrict__ conv, int32_t* __restrict__ nfev,
                                                              double* __restrict__ nll_const, int const_mode,
                                                              CellDesign cells, Geo geo) {
    __shared__ Lbfgsb1d machine[Geo::kWaves];
    log_tab_fill();  // the count memo takes its logarithms through the LDS table (flog_t, dsq_math.h)
    __syncthreads();
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        const AlphaOut o = fit_alpha_wide<typename Geo::Wave>(
            y + (size_t)g * ldn, mu + (size_t)g * ldn, Xt, ldx, N, W, cells.C > 0 ? &cells : nullptr, alpha_hat[g],
            min_disp, max_disp, prior_var, cr_reg != 0, prior_reg != 0, machine[Geo::wave()],
            const_mode == DSQ_CONST_LOAD ? nll_const + g : nullptr,
            const_mode == DSQ_CONST_STORE ? nll_const + g : nullptr);
        if (Geo::lane0()) {
            alpha[g] = o.alpha;
            conv[g] = (uint8_t)o.converged;
            if (nfev != nullptr) nfev[g] = o.nfev;
        }
    });
}

// The slot family's dispersion kernel stays written out: k_alpha_wide<SlotGeom> computes the same bits with the same
// registers, scratch and LDS, but its schedule came out 0.2 - 0.4 % slower per deseq2() pass at p = 65 (this kernel is
// 85 % of that pass), whichever way the policy was shaped (item loop as for / do-while / each, policy first or last, the
// slots as a __restrict__ argument).
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
    extern __shared__ __attribute__((aligned(16))) double wider_lds[];
    WiderWork W;
    W.bind_split(wider_lds, slots + (size_t)blockIdx.x * slot_doubles, P);
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

// grid_fit_alpha alone for listed genes: alpha[list[k]] = exp(best grid point)
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_alpha_grid_wide(const int32_t* __restrict__ y,
                                                                   const double* __restrict__ mu, int ldn,
                                                                   const double* __restrict__ Xt, int ldx, int N, int P,
                                                                   double min_disp, double max_disp,
                                                                   double* __restrict__ alpha,
                                                                   const int32_t* __restrict__ list, int n_list,
                                                                   Geo geo) {
    using Wv = typename Geo::Wave;
    log_tab_fill();  // the count memo takes its logarithms through the LDS table (flog_t, dsq_math.h)
    __syncthreads();
    const typename Geo::Work W = geo.work(P);
    geo.each(n_list, [&](int k) {
        const int g = list[k];
        WideAlphaArgs A;
        A.y = y + (size_t)g * ldn; A.mu = mu + (size_t)g * ldn; A.Xt = Xt; A.ldx = ldx; A.N = N; A.cells = nullptr;
        A.la_hat = 0.0; A.prior_var = 1.0;
        A.cst = alpha_const<Wv>(A.y, A.mu, N);
        const double best_la = grid_alpha_wide<Wv>(A, W, log(min_disp), log(max_disp));
        if (Geo::lane0()) alpha[g] = exp(best_la);
    });
}

hipError_t launch_wide_alpha(hipStream_t st, const int32_t* y, const double* mu, int ldn, const double* Xt, int ldx,
                             int N, int G, int P, const double* alpha_hat, double min_disp, double max_disp,
                             double prior_var, int cr_reg, int prior_reg, double* alpha, uint8_t* conv,
                             int32_t* nfev, double* nll_const, int const_mode, const CellDesign* cells) {
    if (G <= 0) return hipSuccess;
    if (nll_const == nullptr) const_mode = DSQ_CONST_COMPUTE;
    const size_t static_lds = 2 * kLogTabN * sizeof(double) + sizeof(Lbfgsb1d);
    if (P > kWideMaxP) {  // k_alpha_wider (no cells)
        WideLaunch L;
        SlotGeom geo;
        const hipError_t e = SlotGeom::plan(st, P, G, static_lds, 1, L, geo);
        if (e != hipSuccess) return e;
        set_smem(k_alpha_wider, L.smem);
        hipLaunchKernelGGL(k_alpha_wider, dim3(L.grid), dim3(L.block), L.smem, st, y, mu, ldn, Xt, ldx, N, G, P,
                           geo.slots, geo.slot_doubles, alpha_hat, min_disp, max_disp, prior_var, cr_reg, prior_reg,
                           alpha, conv, nfev, nll_const, const_mode);
        return hipGetLastError();
    }
    CellDesign cd{};
    if (cells != nullptr) cd = *cells;
    return wide_run(LdsGeom{}, k_alpha_wide<LdsGeom>, st, P, G, static_lds, LdsGeom::kWaves, y, mu, ldn, Xt, ldx, N, G,
                    P, alpha_hat, min_disp, max_disp, prior_var, cr_reg, prior_reg, alpha, conv, nfev, nll_const,
                    const_mode, cd);
}

hipError_t launch_wide_alpha_grid(hipStream_t st, const int32_t* y, const double* mu, int ldn, const double* Xt,
                                  int ldx, int N, int P, double min_disp, double max_disp, double* alpha,
                                  const int32_t* list, int n_list) {
    if (n_list <= 0) return hipSuccess;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_alpha_grid_wide<decltype(geo)>, st, P, n_list, 2 * kLogTabN * sizeof(double),
                        LdsGeom::kWaves, y, mu, ldn, Xt, ldx, N, P, min_disp, max_disp, alpha, list, n_list);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

// ------------------------------------------------------------------ IRLS (+ fused epilogue), rescue, layers, Wald
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_irls_wide(const int32_t* __restrict__ y, int ldn,
                                                             const double* __restrict__ sf,
                                                             const double* __restrict__ lsf,
                                                             const double* __restrict__ Xt,
                                                             const double* __restrict__ pinvXt, int ldx, int N, int G,
                                                             int P, int full_rank, const double* __restrict__ disp,
                                                             double min_mu, double beta_tol, double min_beta,
                                                             double max_beta, int maxiter, double* __restrict__ beta,
                                                             double* __restrict__ mu, double* __restrict__ hat,
                                                             uint8_t* __restrict__ conv, int32_t* __restrict__ iters,
                                                             int32_t* __restrict__ fb_count,
                                                             int32_t* __restrict__ fb_list, IrlsExtras ex, Geo geo) {
    using Wv = typename Geo::Wave;
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = lsf; A.Xt = Xt; A.pinvXt = pinvXt; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = beta_tol; A.min_beta = min_beta; A.max_beta = max_beta;
        A.maxiter = maxiter; A.full_rank = full_rank != 0;
        if (Geo::kCells && ex.cells.C > 0) A.cells = &ex.cells;
        LfcEpilogue E;
        epilogue_begin(E, ex, g, ldn);
        const IrlsOut o = irls_gene_wide<Wv>(A, W, mu ? mu + (size_t)g * ldn : nullptr,
                                             hat ? hat + (size_t)g * ldn : nullptr, &E);
        if (!o.fallback)
            for (int j = Wv::lane(); j < P; j += 64) beta[(size_t)g * P + j] = W.v(0)[j];
        if (Geo::lane0()) {
            conv[g] = (uint8_t)o.converged;
            if (iters != nullptr) iters[g] = o.iters;
            if (o.fallback) fb_list[atomicAdd(fb_count, 1)] = g;
            else epilogue_store(E, ex, g);
        }
    });
}

// the L-BFGS-B rescue of the genes of fb_list: one gene per 64-thread workgroup in either family
template <class Geo>
__global__ __launch_bounds__(64) void k_irls_rescue_wide(const int32_t* __restrict__ y, int ldn,
                                                         const double* __restrict__ sf, const double* __restrict__ lsf,
                                                         const double* __restrict__ Xt,
                                                         const double* __restrict__ pinvXt, int ldx, int N, int P,
                                                         int full_rank, const double* __restrict__ disp, double min_mu,
                                                         double beta_tol, double min_beta, double max_beta, int maxiter,
                                                         double* __restrict__ beta, double* __restrict__ mu,
                                                         double* __restrict__ hat, uint8_t* __restrict__ conv,
                                                         int32_t* __restrict__ iters,
                                                         const int32_t* __restrict__ fb_list, int n_fb, IrlsExtras ex,
                                                         Geo geo) {
    using Wv = typename Geo::Wave;
    constexpr int kMaxP = Geo::Work::kMaxP;
    __shared__ LbfgsbWork<kMaxP> Lb;
    __shared__ double xlu[3 * kMaxP];
    __shared__ int nbd[kMaxP];
    const typename Geo::Work W = geo.work(P);
    geo.each(n_fb, [&](int k) {
        const int g = fb_list[k];
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = lsf; A.Xt = Xt; A.pinvXt = pinvXt; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = beta_tol; A.min_beta = min_beta; A.max_beta = max_beta;
        A.maxiter = maxiter; A.full_rank = full_rank != 0;
        // beta_init of the gene (the first kernel's W is gone): recompute as irls_gene_wide does
        for (int j = 0; j < P; ++j) {
            double b0 = 0.0;
            for (int n = Wv::lane(); n < N; n += 64) {
                const double yv = (double)A.y[n];
                if (A.full_rank) b0 += pinvXt[j * ldx + n] * log(yv / sf[n] + 0.1);
                else if (j == 0) b0 += log(yv / sf[n]);
            }
            b0 = Wv::sum(b0);
            if (!A.full_rank) b0 = j == 0 ? b0 / (double)N : 0.0;
            if (Geo::lane0()) W.v(2)[j] = b0;
        }
        Wv::sync();
        LfcEpilogue E;
        epilogue_begin(E, ex, g, ldn);
        if (ex.cooks_ld != 0 && E.cooks_row != nullptr) E.cooks_row = ex.cooks_tmp + (size_t)k * ldn;  // (see k_irls_rescue)
        const IrlsOut o = irls_rescue_wide<Wv>(A, W, Lb, xlu, nbd, mu ? mu + (size_t)g * ldn : nullptr,
                                               hat ? hat + (size_t)g * ldn : nullptr, &E);
        for (int j = Wv::lane(); j < P; j += 64) beta[(size_t)g * P + j] = W.v(0)[j];
        if (Geo::lane0()) {
            conv[g] = (uint8_t)o.converged;
            if (iters != nullptr) iters[g] = o.iters;
            epilogue_store(E, ex, g);
        }
    });
}

hipError_t launch_wide_irls(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* lsf,
                            const double* Xt, const double* pinvXt, int ldx, int N, int G, int P, int full_rank,
                            const double* disp, double min_mu, double beta_tol, double min_beta, double max_beta,
                            int maxiter, double* beta, double* mu, double* hat, uint8_t* conv, int32_t* iters,
                            int32_t* fb_count, int32_t* fb_list, const IrlsExtras* extras) {
    if (G <= 0) return hipSuccess;
    IrlsExtras ex{};
    if (extras != nullptr) ex = *extras;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_irls_wide<decltype(geo)>, st, P, G, 0, LdsGeom::kWaves, y, ldn, sf, lsf, Xt, pinvXt, ldx,
                        N, G, P, full_rank, disp, min_mu, beta_tol, min_beta, max_beta, maxiter, beta, mu, hat, conv,
                        iters, fb_count, fb_list, ex);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

hipError_t launch_wide_irls_rescue(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* lsf,
                                   const double* Xt, const double* pinvXt, int ldx, int N, int P, int full_rank,
                                   const double* disp, double min_mu, double beta_tol, double min_beta,
                                   double max_beta, int maxiter, double* beta, double* mu, double* hat, uint8_t* conv,
                                   int32_t* iters, const int32_t* fb_list, int n_fb, const IrlsExtras* extras) {
    if (n_fb <= 0) return hipSuccess;
    IrlsExtras ex{};
    if (extras != nullptr) ex = *extras;
    ex.cells = CellDesign{};  // the rescue of a diverged gene runs the general evaluation
    const auto go = [&](auto geo) {
        constexpr int kMaxP = decltype(geo)::Work::kMaxP;
        constexpr size_t stat = sizeof(LbfgsbWork<kMaxP>) + 3 * kMaxP * sizeof(double) + kMaxP * sizeof(int);
        return wide_run(geo, k_irls_rescue_wide<decltype(geo)>, st, P, n_fb, stat, 1, y, ldn, sf, lsf, Xt, pinvXt, ldx,
                        N, P, full_rank, disp, min_mu, beta_tol, min_beta, max_beta, maxiter, beta, mu, hat, conv, iters,
                        fb_list, n_fb, ex);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

// layers (mu, hat) of a finished fit from beta
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_irls_layers_wide(const int32_t* __restrict__ y, int ldn,
                                                                    const double* __restrict__ sf,
                                                                    const double* __restrict__ Xt, int ldx, int N,
                                                                    int G, int P, const double* __restrict__ disp,
                                                                    const double* __restrict__ beta, double min_mu,
                                                                    double* __restrict__ mu, double* __restrict__ hat,
                                                                    Geo geo) {
    using Wv = typename Geo::Wave;
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        IrlsArgs A;
        A.y = y + (size_t)g * ldn; A.sf = sf; A.lsf = nullptr; A.Xt = Xt; A.pinvXt = nullptr; A.ldx = ldx; A.N = N;
        A.disp = disp[g]; A.min_mu = min_mu; A.beta_tol = 0.0; A.min_beta = 0.0; A.max_beta = 0.0; A.maxiter = 0;
        A.full_rank = false;
        for (int j = Wv::lane(); j < P; j += 64) W.v(0)[j] = beta[(size_t)g * P + j];
        Wv::sync();
        double S;
        irls_sweep_wide<Wv>(A, W, 1.0 / A.disp, S);
        irls_finish_wide<Wv>(A, W, mu ? mu + (size_t)g * ldn : nullptr, hat ? hat + (size_t)g * ldn : nullptr, nullptr);
    });
}

hipError_t launch_wide_irls_layers(hipStream_t st, const int32_t* y, int ldn, const double* sf, const double* Xt,
                                   int ldx, int N, int G, int P, const double* disp, const double* beta, double min_mu,
                                   double* mu, double* hat) {
    if (G <= 0) return hipSuccess;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_irls_layers_wide<decltype(geo)>, st, P, G, 0, LdsGeom::kWaves, y, ldn, sf, Xt, ldx, N, G,
                        P, disp, beta, min_mu, mu, hat);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_wald_wide(const double* __restrict__ mu, int ldn,
                                                             const double* __restrict__ sf,
                                                             const double* __restrict__ Xt, int ldx, int N, int G,
                                                             int P, const double* __restrict__ disp,
                                                             const double* __restrict__ beta,
                                                             const double* __restrict__ ridge,
                                                             const double* __restrict__ contrast, double lfc_null,
                                                             int alt, double* __restrict__ pvals,
                                                             double* __restrict__ stats, double* __restrict__ se,
                                                             Geo geo) {
    using Wv = typename Geo::Wave;
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        for (int j = Wv::lane(); j < P; j += 64) W.v(0)[j] = beta[(size_t)g * P + j];
        Wv::sync();
        const WaldOut o = wald_gene_wide<Wv>(mu ? mu + (size_t)g * ldn : nullptr, sf, Xt, ldx, N, disp[g], W, ridge,
                                             contrast, lfc_null, alt);
        if (Geo::lane0()) {
            pvals[g] = o.p;
            stats[g] = o.stat;
            se[g] = o.se;
        }
    });
}

hipError_t launch_wide_wald(hipStream_t st, const double* mu, int ldn, const double* sf, const double* Xt, int ldx,
                            int N, int G, int P, const double* disp, const double* beta, const double* d_ridge,
                            const double* d_contrast, double lfc_null, int alt, double* pvals, double* stats,
                            double* se) {
    if (G <= 0) return hipSuccess;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_wald_wide<decltype(geo)>, st, P, G, 0, LdsGeom::kWaves, mu, ldn, sf, Xt, ldx, N, G, P,
                        disp, beta, d_ridge, d_contrast, lfc_null, alt, pvals, stats, se);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

// K contrasts ([K][P]) of one fit: one Gram matrix and one factorisation per gene, the tail per contrast; results [G][K]
template <class Geo>
__global__ __launch_bounds__(Geo::kThreads) void k_wald_multi_wide(const double* __restrict__ mu, int ldn,
                                                                   const double* __restrict__ sf,
                                                                   const double* __restrict__ Xt, int ldx, int N, int G,
                                                                   int P, const double* __restrict__ disp,
                                                                   const double* __restrict__ beta,
                                                                   const double* __restrict__ ridge,
                                                                   const double* __restrict__ contrasts, int K,
                                                                   double lfc_null, int alt, double* __restrict__ pvals,
                                                                   double* __restrict__ stats, double* __restrict__ se,
                                                                   Geo geo) {
    using Wv = typename Geo::Wave;
    const typename Geo::Work W = geo.work(P);
    geo.each(G, [&](int g) {
        for (int j = Wv::lane(); j < P; j += 64) W.v(0)[j] = beta[(size_t)g * P + j];
        Wv::sync();
        const size_t o = (size_t)g * K;
        wald_gene_multi_wide<Wv>(mu ? mu + (size_t)g * ldn : nullptr, sf, Xt, ldx, N, disp[g], W, ridge, contrasts, K,
                                 lfc_null, alt, Geo::lane0(), pvals + o, stats + o, se + o);
    });
}

hipError_t launch_wide_wald_multi(hipStream_t st, const double* mu, int ldn, const double* sf, const double* Xt, int ldx,
                                  int N, int G, int P, const double* disp, const double* beta, const double* d_ridge,
                                  const double* d_contrasts, int K, double lfc_null, int alt, double* pvals,
                                  double* stats, double* se) {
    if (G <= 0) return hipSuccess;
    if (K < 1) return hipErrorInvalidValue;
    const auto go = [&](auto geo) {
        return wide_run(geo, k_wald_multi_wide<decltype(geo)>, st, P, G, 0, LdsGeom::kWaves, mu, ldn, sf, Xt, ldx, N, G,
                        P, disp, beta, d_ridge, d_contrasts, K, lfc_null, alt, pvals, stats, se);
    };
    return P > kWideMaxP ? go(SlotGeom{}) : go(LdsGeom{});
}

// the width from which the register / cell kernels hand over to this path (DSQ_WIDE_MIN_P: measurements)
int wide_min_p() {
    static const int v = [] {
        const char* e = getenv("DSQ_WIDE_MIN_P");
        const int x = e ? atoi(e) : DSQ_REG_MAX_P + 1;
        return x < 1 ? 1 : (x > DSQ_REG_MAX_P + 1 ? DSQ_REG_MAX_P + 1 : x);
    }();
    return v;
}

bool wide_with_cells() {
    static const bool v = getenv("DSQ_WIDE_CELLS") != nullptr;
    return v;
}

}  // namespace dsq
