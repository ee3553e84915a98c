// devunit.hip — TEST-ONLY device build of the scalar math and wave policies (never linked into the package).
//
// tests/hostsim compiles the per-gene headers with g++, so it runs the host branch of every
// `#if defined(__HIP_DEVICE_COMPILE__)` in dsq_math.h and the one-lane HostWave.  This library compiles the same headers
// with hipcc for gfx950 and the product's CXXFLAGS (tests/devunit/build.py reads them from csrc/Makefile), and calls
// their functions from small kernels: v_rcp_f64 / v_rsq_f64 + Newton, the LDS log / exp tables, the constant-memory
// count tables, DeviceWave's permlane / DPP butterflies and RowWave's row-scoped reductions.  No function body of the
// headers is restated here: a change to a header changes what is tested.
//
// Every launch is 256-thread blocks over n % 256 == 0 elements (whole waves, whole RowWave rows); every thread reaches
// the table fills and the one __syncthreads() before anything else.  Each entry point allocates, copies, launches,
// synchronises and frees on its own and returns the first hipError_t (hipErrorInvalidValue for a bad argument).
#include <hip/hip_runtime.h>

#include "devunit_host.h"
#include "dsq_alpha.h"
#include "dsq_alpha_rows.h"
#include "dsq_irls.h"
#include "dsq_math.h"
#include "dsq_stats.h"
#include "dsq_wave.h"

using namespace dsq;
using devunit::Bufs;

namespace {

constexpr int kB = 256;  // threads per block

bool bad_n(int n) { return n <= 0 || n % kB != 0; }

// ------------------------------------------------------------------------------------------------ scalar functions
enum MathOp {
    kFrcp = 0, kFrsq, kFrcpG, kFdiv, kFlog, kFlogT, kFlog1p, kFlog1pT, kFexpT, kLgammaPos, kDigammaPos,
    kLgDg00, kLgDg10, kLgDg01, kLgDg11,  // lgamma_digamma<WANT_DG, TAB>
    kNormSf, kStirlingBig, kLogCount, kMathOps
};

__global__ void __launch_bounds__(kB) k_math(int op, const double* x, const double* y, double* o1, double* o2, int n) {
    log_tab_fill();
    exp_tab_fill();
    __syncthreads();
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r1 = 0.0, r2 = 0.0;
    switch (op) {
        case kFrcp: r1 = frcp(v); break;
        case kFrsq: r1 = frsq(v); break;
        case kFrcpG: r1 = frcp_g(v); break;
        case kFdiv: r1 = fdiv(v, y[i]); break;
        case kFlog: r1 = flog(v); break;
        case kFlogT: r1 = flog_t(v); break;
        case kFlog1p: r1 = flog1p(v); break;
        case kFlog1pT: r1 = flog1p_t(v, frcp(1.0 + v)); break;  // as the kernels call it
        case kFexpT: r1 = fexp_t(v); break;
        case kLgammaPos: r1 = lgamma_pos(v); break;
        case kDigammaPos: r1 = digamma_pos(v); break;
        case kLgDg00: lgamma_digamma<false, false>(v, r1, r2); r2 = 0.0; break;
        case kLgDg10: lgamma_digamma<true, false>(v, r1, r2); break;
        case kLgDg01: lgamma_digamma<false, true>(v, r1, r2); r2 = 0.0; break;
        case kLgDg11: lgamma_digamma<true, true>(v, r1, r2); break;
        case kNormSf: r1 = norm_sf(v); break;
        case kStirlingBig: stirling_big(v, r1, r2); break;
        case kLogCount: r1 = log_count((int)v); break;
        default: break;
    }
    o1[i] = r1;
    if (o2 != nullptr) o2[i] = r2;
}

// the count / log tables as the device reads them: kLgammaInt, kLogInt (constant memory), then the LDS copies of
// kLogTab and kExpTab that log_tab_fill / exp_tab_fill made
constexpr int kTabOut = 256 + 256 + 2 * kLogTabN + kExpTabN;
__global__ void __launch_bounds__(kB) k_tables(double* o) {
    log_tab_fill();
    exp_tab_fill();
    __syncthreads();
    const int t = threadIdx.x;
    if (t < kLgammaIntN) o[t] = kLgammaInt[t];
    if (t < 256) o[256 + t] = kLogInt[t];
#if defined(__HIP_DEVICE_COMPILE__)  // (the LDS tables exist in the device pass only)
    for (int j = t; j < 2 * kLogTabN; j += kB) o[512 + j] = g_log_tab[j];
    for (int j = t; j < kExpTabN; j += kB) o[512 + 2 * kLogTabN + j] = g_exp_tab[j];
#endif
}

// ---------------------------------------------------------------------- lgamma(a) - lgamma(y + a), digamma likewise
// one gene (= one a) per Wv::W lanes, lga / dga from the table lgamma_digamma, as alpha_eval_body computes them
template <class Wv, bool GRAD, bool BIG>
__global__ void __launch_bounds__(kB) k_lgdiff(const int* y, const double* a_gene, double* dl, double* dd, int n) {
    log_tab_fill();
    __syncthreads();
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const double a = a_gene[i / Wv::W];
    double lga, dga;
    lgamma_digamma<true, true>(a, lga, dga);
    double l, d;
    lgamma_digamma_diff<Wv, GRAD, BIG>(y[i], a, lga, dga, l, d);
    dl[i] = l;
    dd[i] = d;
}

// irls_init's cst = -sum[(lgamma(a) - lgamma(y+a)) + log(y!)] over one sample per gene (lane 0 of a DeviceWave):
// the wave memo of the gamma differences and the log-factorial's switch from kLgammaInt to Stirling at count 256
__global__ void __launch_bounds__(kB) k_irls_cst(const int* y, const double* a_gene, double* cst, int n) {
    log_tab_fill();
    __syncthreads();
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    const int g = i / 64;
    const double sf = 1.0, px = 1.0;
    IrlsArgs A{};
    A.y = y + g;
    A.sf = &sf;
    A.lsf = nullptr;
    A.Xt = &px;
    A.pinvXt = &px;
    A.ldx = 1;
    A.N = 1;
    A.full_rank = true;
    double b0[1], c;
    irls_init<DeviceWave, 1>(A, a_gene[g], b0, c);
    if (DeviceWave::lane() == 0) cst[g] = c;
}

// ------------------------------------------------------------------------------------------------ wave policies
enum WaveOp {
    kSum = 0, kSumi, kMaxi, kMax, kExclScan, kFromLane, kUniform, kReadlane, kRowBcast, kAny, kHist, kSlotAll,
    kSlotThird, kCellAdd, kWaveOps
};

template <int L>
__device__ __forceinline__ void row_bcast_all(double v, double* o, int i, int n) {
    if constexpr (L < 16) {
        o[(size_t)L * n + i] = RowWave::row_bcast<L>(v);
        row_bcast_all<L + 1>(v, o, i, n);
    }
}

// even_only (RowWave): rows 1 and 3 of every wavefront leave the kernel before the operation
template <class Wv>
__global__ void __launch_bounds__(kB) k_wave(int op, int even_only, const double* x, const int* xi, double* o, int* oi,
                                             int n) {
    constexpr int G = kB / Wv::W;  // genes per block
    __shared__ unsigned int s_cnt[G * 8];
    __shared__ unsigned int s_slot[G];
    __shared__ double s_acc[G];
    for (int t = threadIdx.x; t < G * 8; t += kB) s_cnt[t] = 0u;
    if (threadIdx.x < G) {
        s_slot[threadIdx.x] = 0u;
        s_acc[threadIdx.x] = 0.0;
    }
    __syncthreads();
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    if constexpr (Wv::W == 16) {
        if (even_only && ((threadIdx.x >> 4) & 1) != 0) return;
    }
    const int g = threadIdx.x / Wv::W, ln = Wv::lane();
    switch (op) {
        case kSum: o[i] = Wv::sum(x[i]); break;
        case kSumi: oi[i] = Wv::sumi(xi[i]); break;
        case kMaxi: oi[i] = Wv::maxi(xi[i]); break;
        case kMax: o[i] = Wv::max(x[i]); break;
        case kExclScan: oi[i] = Wv::excl_scan_i(xi[i]); break;
        case kFromLane:
            for (int s = 0; s < Wv::W; ++s) o[(size_t)s * n + i] = Wv::from_lane(x[i], s);
            break;
        case kUniform: o[i] = Wv::uniform(x[i]); break;
        case kReadlane:
            if constexpr (Wv::W == 64) {
                for (int s = 0; s < 64; ++s) o[(size_t)s * n + i] = detail::readlane_d(x[i], s);
            }
            break;
        case kRowBcast:
            if constexpr (Wv::W == 16) row_bcast_all<0>(x[i], o, i, n);
            break;
        case kAny: oi[i] = Wv::any(xi[i] != 0) ? 1 : 0; break;
        case kHist:
            Wv::hist_add(&s_cnt[g * 8 + (xi[i] & 7)]);
            Wv::sync();
            oi[i] = (int)s_cnt[g * 8 + (ln & 7)];
            break;
        case kSlotAll: oi[i] = (int)Wv::slot_add(&s_slot[g]); break;
        case kSlotThird:
            if (ln % 3 == 0) oi[i] = (int)Wv::slot_add(&s_slot[g]);
            break;
        case kCellAdd:
            Wv::cell_add(&s_acc[g], x[i]);
            Wv::sync();
            o[i] = s_acc[g];
            break;
        default: break;
    }
}

// K sums at once: o = sum_n<K>, oref = sum() of each value; x, o, oref are [K][n]
template <class Wv, int K>
__global__ void __launch_bounds__(kB) k_sumn(int even_only, const double* x, double* o, double* oref, int n) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    if constexpr (Wv::W == 16) {
        if (even_only && ((threadIdx.x >> 4) & 1) != 0) return;
    }
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = x[(size_t)k * n + i];
#pragma unroll
    for (int k = 0; k < K; ++k) oref[(size_t)k * n + i] = Wv::sum(v[k]);
    Wv::template sum_n<K>(v);
#pragma unroll
    for (int k = 0; k < K; ++k) o[(size_t)k * n + i] = v[k];
}

// a KSum per lane over T terms (x: [T][n]), then sum_comp; ls / lc: the lane's (s, c) before the reduction
template <class Wv>
__global__ void __launch_bounds__(kB) k_ksum(int T, int even_only, const double* x, double* ls, double* lc, double* o,
                                             int n) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n) return;
    if constexpr (Wv::W == 16) {
        if (even_only && ((threadIdx.x >> 4) & 1) != 0) return;
    }
    KSum k;
    for (int t = 0; t < T; ++t) k.add(x[(size_t)t * n + i]);
    ls[i] = k.s;
    lc[i] = k.c;
    o[i] = Wv::sum_comp(k);
}

template <class Wv, int K>
void launch_sumn(int even_only, const double* x, double* o, double* oref, int n) {
    hipLaunchKernelGGL((k_sumn<Wv, K>), dim3(n / kB), dim3(kB), 0, 0, even_only, x, o, oref, n);
}

template <class Wv>
bool dispatch_sumn(int K, int even_only, const double* x, double* o, double* oref, int n) {
    switch (K) {
#define DU_K(k) \
    case k: launch_sumn<Wv, k>(even_only, x, o, oref, n); return true;
        DU_K(1) DU_K(2) DU_K(3) DU_K(4) DU_K(5) DU_K(6) DU_K(7) DU_K(8) DU_K(9) DU_K(12) DU_K(13) DU_K(16) DU_K(24)
        DU_K(48)
#undef DU_K
        default: return false;
    }
}

}  // namespace

extern "C" {

// op: MathOp; y only for fdiv, o2 only for the functions with a second result (may be null otherwise)
int du_math(int op, const double* x, const double* y, double* o1, double* o2, int n) {
    if (bad_n(n) || op < 0 || op >= kMathOps || x == nullptr || o1 == nullptr || (op == kFdiv && y == nullptr))
        return (int)hipErrorInvalidValue;
    Bufs B;
    const double* dx = B.put(x, n);
    const double* dy = B.put(y, op == kFdiv ? n : 0);
    double* d1 = B.put(o1, n);
    double* d2 = B.put(o2, n);
    if (B.e != hipSuccess) return (int)B.e;
    hipLaunchKernelGGL(k_math, dim3(n / kB), dim3(kB), 0, 0, op, dx, op == kFdiv ? dy : nullptr, d1, d2, n);
    B.done();
    B.get(o1, d1, n);
    B.get(o2, d2, n);
    return (int)B.e;
}

int du_tables_n() { return kTabOut; }

int du_tables(double* o) {
    if (o == nullptr) return (int)hipErrorInvalidValue;
    Bufs B;
    double* d = B.put(o, kTabOut);
    if (B.e != hipSuccess) return (int)B.e;
    hipLaunchKernelGGL(k_tables, dim3(1), dim3(kB), 0, 0, d);
    B.done();
    B.get(o, d, kTabOut);
    return (int)B.e;
}

// wave: 64 (DeviceWave) or 16 (RowWave); a: one value per gene (n / wave of them); big: every y >= 256
int du_lgdiff(int wave, int grad, int big, const int* y, const double* a, double* dl, double* dd, int n) {
    if (bad_n(n) || (wave != 64 && wave != 16) || !y || !a || !dl || !dd) return (int)hipErrorInvalidValue;
    Bufs B;
    const int* dy = B.put(y, n);
    const double* da = B.put(a, n / wave);
    double* ddl = B.put(dl, n);
    double* ddd = B.put(dd, n);
    if (B.e != hipSuccess) return (int)B.e;
    const dim3 g(n / kB), b(kB);
#define DU_LG(W, G, Bg) hipLaunchKernelGGL((k_lgdiff<W, G, Bg>), g, b, 0, 0, dy, da, ddl, ddd, n)
    if (wave == 64) {
        if (grad) { if (big) DU_LG(DeviceWave, true, true); else DU_LG(DeviceWave, true, false); }
        else { if (big) DU_LG(DeviceWave, false, true); else DU_LG(DeviceWave, false, false); }
    } else {
        if (grad) { if (big) DU_LG(RowWave, true, true); else DU_LG(RowWave, true, false); }
        else { if (big) DU_LG(RowWave, false, true); else DU_LG(RowWave, false, false); }
    }
#undef DU_LG
    B.done();
    B.get(dl, ddl, n);
    B.get(dd, ddd, n);
    return (int)B.e;
}

// n / 64 genes of one sample each: y[g], a[g] -> cst[g]
int du_irls_cst(const int* y, const double* a, double* cst, int n) {
    if (bad_n(n) || !y || !a || !cst) return (int)hipErrorInvalidValue;
    const int G = n / 64;
    Bufs B;
    const int* dy = B.put(y, G);
    const double* da = B.put(a, G);
    double* dc = B.put(cst, G);
    if (B.e != hipSuccess) return (int)B.e;
    hipLaunchKernelGGL(k_irls_cst, dim3(n / kB), dim3(kB), 0, 0, dy, da, dc, n);
    B.done();
    B.get(cst, dc, G);
    return (int)B.e;
}

// op: WaveOp; o / oi hold n * nout entries (nout = 64 for from_lane / readlane_d on DeviceWave, 16 for from_lane and
// row_bcast on RowWave, else 1); x / xi / o / oi may be null where the op does not use them
int du_wave(int wave, int op, int even_only, const double* x, const int* xi, double* o, int* oi, int n, int nout) {
    if (bad_n(n) || (wave != 64 && wave != 16) || op < 0 || op >= kWaveOps || nout < 1 || nout > 64)
        return (int)hipErrorInvalidValue;
    const size_t no = (size_t)n * nout;
    Bufs B;
    const double* dx = B.put(x, n);
    const int* dxi = B.put(xi, n);
    double* d_o = B.put(o, no);
    int* d_oi = B.put(oi, no);
    if (B.e != hipSuccess) return (int)B.e;
    const bool wide = op == kFromLane || op == kReadlane || op == kRowBcast;
    const bool dbl_in = op == kSum || op == kMax || op == kFromLane || op == kUniform || op == kReadlane ||
                        op == kRowBcast || op == kCellAdd;
    const bool dbl_out = dbl_in;
    if ((dbl_in ? dx == nullptr : dxi == nullptr) && op != kSlotAll && op != kSlotThird) return (int)hipErrorInvalidValue;
    if (dbl_out ? d_o == nullptr : d_oi == nullptr) return (int)hipErrorInvalidValue;
    if (wide && nout != (op == kReadlane ? 64 : (op == kRowBcast ? 16 : wave))) return (int)hipErrorInvalidValue;
    if ((op == kReadlane && wave != 64) || (op == kRowBcast && wave != 16)) return (int)hipErrorInvalidValue;
    if (wave == 64)
        hipLaunchKernelGGL(k_wave<DeviceWave>, dim3(n / kB), dim3(kB), 0, 0, op, 0, dx, dxi, d_o, d_oi, n);
    else
        hipLaunchKernelGGL(k_wave<RowWave>, dim3(n / kB), dim3(kB), 0, 0, op, even_only, dx, dxi, d_o, d_oi, n);
    B.done();
    B.get(o, d_o, no);
    B.get(oi, d_oi, no);
    return (int)B.e;
}

// x, o, oref: [K][n]
int du_sumn(int wave, int K, int even_only, const double* x, double* o, double* oref, int n) {
    if (bad_n(n) || (wave != 64 && wave != 16) || K < 1 || !x || !o || !oref) return (int)hipErrorInvalidValue;
    const size_t nk = (size_t)n * K;
    Bufs B;
    const double* dx = B.put(x, nk);
    double* d_o = B.put(o, nk);
    double* d_r = B.put(oref, nk);
    if (B.e != hipSuccess) return (int)B.e;
    const bool ok = wave == 64 ? dispatch_sumn<DeviceWave>(K, 0, dx, d_o, d_r, n)
                               : dispatch_sumn<RowWave>(K, even_only, dx, d_o, d_r, n);
    if (!ok) return (int)hipErrorInvalidValue;
    B.done();
    B.get(o, d_o, nk);
    B.get(oref, d_r, nk);
    return (int)B.e;
}

// x: [T][n]
int du_ksum(int wave, int T, int even_only, const double* x, double* ls, double* lc, double* o, int n) {
    if (bad_n(n) || (wave != 64 && wave != 16) || T < 1 || !x || !ls || !lc || !o) return (int)hipErrorInvalidValue;
    Bufs B;
    const double* dx = B.put(x, (size_t)n * T);
    double* d_s = B.put(ls, n);
    double* d_c = B.put(lc, n);
    double* d_o = B.put(o, n);
    if (B.e != hipSuccess) return (int)B.e;
    if (wave == 64)
        hipLaunchKernelGGL(k_ksum<DeviceWave>, dim3(n / kB), dim3(kB), 0, 0, T, 0, dx, d_s, d_c, d_o, n);
    else
        hipLaunchKernelGGL(k_ksum<RowWave>, dim3(n / kB), dim3(kB), 0, 0, T, even_only, dx, d_s, d_c, d_o, n);
    B.done();
    B.get(ls, d_s, n);
    B.get(lc, d_c, n);
    B.get(o, d_o, n);
    return (int)B.e;
}

}  // extern "C"
