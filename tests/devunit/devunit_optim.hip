// devunit_optim.hip — TEST-ONLY device build of the lane-parallel L-BFGS-B optimisers (never linked into the package).
//
// The body of lbfgsb_wave (dsq_lbfgsb_wave.h) exists only under __HIP_DEVICE_COMPILE__, and the two forks of lbfgsb_nd
// (dsq_lbfgsb.h) that move WN1 / SS / SY by read-barrier-write compile only for a 64-lane policy: tests/hostsim cannot
// execute either.  This unit instantiates them under the product's CXXFLAGS and calls them from small kernels:
//   * the 8-, 16- and 32-lane group sums wv8 / wv16 / wv32 rowsum and colsum, one value per lane;
//   * lbfgsb_wave_direction<R> on given pairs;
//   * lbfgsb_wave<P, R> and lbfgsb_nd<NMAX, ., 10, OneLane | DeviceWave> on a test objective whose every evaluation
//     (x, f, g) lane 0 records into a global trace of at most 256 evaluations;
//   * lbp::dpofa / lbp::dtrsl_upper / a batch of lbp::dtrsl_upper_t_own with OneLane and with DeviceWave.
// No function body of the headers is restated here.  The objective is the unit's own: a __noinline__ function that every
// lane evaluates redundantly in scalar code, so that every optimiser instantiation sees the same function bits.
//
// One problem per wavefront, on a wave-private workspace in LDS which the wavefront first fills with a 64-bit pattern
// given by the caller (NaN unless a test says otherwise).  Every entry point allocates, copies, launches, synchronises
// and frees on its own and returns the first hipError_t (hipErrorInvalidValue for a bad argument).
#include <hip/hip_runtime.h>
#include <math.h>

#include "devunit_host.h"
#include "dsq_lbfgsb_wave.h"

using namespace dsq;

namespace du_optim {  // (named: the assembly check reads all units as one translation unit)

constexpr int kTraceCap = 256;
constexpr unsigned long long kNaNBits = 0x7ff8000000000000ull;

template <class T>
__device__ __forceinline__ void fill_words(T& W, unsigned long long pattern) {
    static_assert(sizeof(T) % 8 == 0, "whole 64-bit words");
    unsigned long long* raw = (unsigned long long*)&W;
    for (int i = threadIdx.x & 63; i < (int)(sizeof(T) / 8); i += 64) raw[i] = pattern;
    DeviceWave::sync();
}

// ---------------------------------------------------------------------------------------------- group sums
// R: 8 / 16 / 32, col: 0 rowsum, 1 colsum.  n is a multiple of 256: every lane of every wavefront is active.
__global__ __launch_bounds__(256) void k_groupsum(int R, int col, const double* __restrict__ v, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const double x = v[t];
    double r = x;
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass only needs the kernel's name)
    if (R == 8) r = col ? wv8::colsum(x) : wv8::rowsum(x);
    else if (R == 16) r = col ? wv16::colsum(x) : wv16::rowsum(x);
    else r = col ? wv32::colsum(x) : wv32::rowsum(x);
#endif
    out[t] = r;
}

// ---------------------------------------------------------------------------------------------- the direction
// S, Y: [n_prob][10][R], RHO: [n_prob][10], g, x, d, z: [n_prob][R]
template <int R>
__global__ __launch_bounds__(256) void k_direction(int n_prob, const int* __restrict__ col, const int* __restrict__ head,
                                                   const double* __restrict__ theta, const double* __restrict__ S,
                                                   const double* __restrict__ Y, const double* __restrict__ RHO,
                                                   const double* __restrict__ g, const double* __restrict__ x,
                                                   double* __restrict__ d, double* __restrict__ z) {
    __shared__ LbfgsbWaveWorkT<R> Ws[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + w;
    if (p >= n_prob) return;
    LbfgsbWaveWorkT<R>& W = Ws[w];
    fill_words(W, kNaNBits);
    for (int k = lane; k < 10 * R; k += 64) {
        (&W.S[0][0])[k] = S[(size_t)p * 10 * R + k];
        (&W.Y[0][0])[k] = Y[(size_t)p * 10 * R + k];
    }
    if (lane < 10) W.RHO[lane] = RHO[p * 10 + lane];
    if (lane < R) { W.g[lane] = g[p * R + lane]; W.x[lane] = x[p * R + lane]; }
    DeviceWave::sync();
#if defined(__HIP_DEVICE_COMPILE__)
    lbfgsb_wave_direction<R>(W, col[p], head[p], theta[p]);
#endif
    if (lane < R) { d[p * R + lane] = W.d[lane]; z[p * R + lane] = W.z[lane]; }
}

// ---------------------------------------------------------------------------------------------- the test objective
// f = 1/2 d' Q d + sum exp(clip(w d, -50, 50)), d = x - c (the family of tests/test_hostsim.py's scipy comparisons)
__device__ __noinline__ void objective(const double* __restrict__ Q, const double* __restrict__ c,
                                       const double* __restrict__ w, int n, const double* x, double* f, double* g) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const double di = x[i] - c[i];
        double qd = 0.0;
        for (int j = 0; j < n; ++j) qd += Q[i * n + j] * (x[j] - c[j]);
        double a = w[i] * di;
        a = a < -50.0 ? -50.0 : (a > 50.0 ? 50.0 : a);
        const double e = exp(a);
        s += 0.5 * di * qd + e;
        g[i] = qd + w[i] * e;
    }
    *f = s;
}

struct OptArgs {
    int n, n_prob;
    unsigned long long pattern;
    const double *Q, *c, *w, *x0, *l, *u;  // Q: [n_prob][n][n], the others [n_prob][n]
    const int* nbd;                        // [n_prob][n]
    double *tx, *tf, *tg;                  // [n_prob][256][n], [n_prob][256], [n_prob][256][n]
    double *xout, *fout;                   // [n_prob][n], [n_prob]
    int* res;                              // [n_prob][5]: success, nfev, nit, status, evaluations seen
};

// the objective of problem p with the trace behind it; pad: components n .. pad-1 of the gradient are written as 0
struct Traced {
    const OptArgs& a;
    int p, pad, nev;
    __device__ __forceinline__ void operator()(const double* x, double& f, double* g) {
        const int n = a.n;
        double fv;
        objective(a.Q + (size_t)p * n * n, a.c + (size_t)p * n, a.w + (size_t)p * n, n, x, &fv, g);
        f = fv;
        for (int k = n; k < pad; ++k) g[k] = 0.0;
        if ((threadIdx.x & 63) == 0 && nev < kTraceCap) {
            const size_t e = (size_t)p * kTraceCap + nev;
            for (int k = 0; k < n; ++k) { a.tx[e * n + k] = x[k]; a.tg[e * n + k] = g[k]; }
            a.tf[e] = fv;
        }
        nev += 1;
    }
};

__device__ __forceinline__ void store_result(const OptArgs& a, int p, const LbfgsbResult& r, int nev, const double* x) {
    DeviceWave::sync();
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < a.n; ++k) a.xout[(size_t)p * a.n + k] = x[k];
        a.fout[p] = r.f;
        int* o = a.res + p * 5;
        o[0] = r.success; o[1] = r.nfev; o[2] = r.nit; o[3] = r.status; o[4] = nev;
    }
}

// blockDim.x / 64 wavefronts, one problem each (blockDim.x: 64 or 256)
template <int P, int R>
__global__ __launch_bounds__(256) void k_wave_opt(OptArgs a) {
    __shared__ LbfgsbWaveWorkT<R> Ws[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = blockIdx.x * (blockDim.x >> 6) + w;
    if (p >= a.n_prob) return;
    LbfgsbWaveWorkT<R>& W = Ws[w];
    fill_words(W, a.pattern);
    if (lane < P) W.x[lane] = lane < a.n ? a.x0[(size_t)p * a.n + lane] : 0.0;
    DeviceWave::sync();
    Traced fg{a, p, P, 0};
    const LbfgsbResult r = lbfgsb_wave<P, R>(fg, W);
    store_result(a, p, r, fg.nev, W.x);
}

template <int NMAX>
struct NdWork {
    LbfgsbWork<NMAX> lb;
    double x[NMAX], l[NMAX], u[NMAX];
    int nbd[NMAX + (NMAX & 1)];
};

template <int NMAX, class Wv>
__global__ __launch_bounds__(64) void k_nd_opt(OptArgs a) {
    __shared__ NdWork<NMAX> W;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x;
    if (p >= a.n_prob) return;
    fill_words(W, a.pattern);
    if (lane < NMAX) {
        const bool in = lane < a.n;
        const size_t q = (size_t)p * a.n + lane;
        W.x[lane] = in ? a.x0[q] : 0.0;
        W.l[lane] = in ? a.l[q] : 0.0;
        W.u[lane] = in ? a.u[q] : 0.0;
        W.nbd[lane] = in ? a.nbd[q] : 0;
    }
    DeviceWave::sync();
    Traced fg{a, p, a.n, 0};
    const LbfgsbResult r = lbfgsb_nd<NMAX, Traced&, 10, Wv>(fg, a.n, W.x, W.l, W.u, W.nbd, W.lb);
    store_result(a, p, r, fg.nev, W.x);
}

// ---------------------------------------------------------------------------------------------- lbp
// op 0: dpofa, 1: dtrsl_upper job 01, 2: dtrsl_upper job 11, 3: the batch of formk - the right-hand sides are the columns
// n + 1 .. 2 n of the array itself, a lane each (2 n <= lda).  a: [n_prob][lda][lda], b, sacc: [n_prob][lda], all
// copied in and back whole; ret: [n_prob][64], what every lane returned.
constexpr int kLdaMax = 20;
template <class Wv>
__global__ __launch_bounds__(64) void k_lbp(int op, int lda, const int* __restrict__ n_, double* __restrict__ a_,
                                            double* __restrict__ b_, double* __restrict__ sacc_, int* __restrict__ ret) {
    __shared__ double a[kLdaMax * kLdaMax], b[kLdaMax], sacc[kLdaMax];
    const int lane = threadIdx.x & 63, p = blockIdx.x, n = n_[p];
    for (int k = lane; k < lda * lda; k += 64) a[k] = a_[(size_t)p * lda * lda + k];
    if (lane < lda) { b[lane] = b_[p * lda + lane]; sacc[lane] = sacc_[p * lda + lane]; }
    DeviceWave::sync();
    int r = 0;
    if (op == 0) r = lbp::dpofa<Wv>(a, lda, n, sacc);
    else if (op == 1) r = lbp::dtrsl_upper<Wv>(a, lda, n, b, 1, sacc);
    else if (op == 2) r = lbp::dtrsl_upper<Wv>(a, lda, n, b, 11, sacc);
    else {
        for (int js = n + 1 + Wv::lane(); js <= 2 * n; js += Wv::W) lbp::dtrsl_upper_t_own(a, lda, n, &a[(js - 1) * lda]);
        Wv::sync();
    }
    DeviceWave::sync();
    for (int k = lane; k < lda * lda; k += 64) a_[(size_t)p * lda * lda + k] = a[k];
    if (lane < lda) { b_[p * lda + lane] = b[lane]; sacc_[p * lda + lane] = sacc[lane]; }
    ret[p * 64 + lane] = r;
}

template <class K, class... A>
void launch(K kernel, dim3 grid, dim3 block, A... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, 0, args...);
}

}  // namespace du_optim

using namespace du_optim;

extern "C" {

int du_groupsum(int R, int col, const double* v, double* out, int n) {
    if ((R != 8 && R != 16 && R != 32) || (col != 0 && col != 1) || n < 256 || n % 256) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    const double* dv = B.put(v, (size_t)n);
    double* dout = B.put(out, (size_t)n);
    if (B.e == hipSuccess) launch(k_groupsum, dim3(n / 256), dim3(256), R, col, dv, dout);
    B.done();
    B.get(out, dout, (size_t)n);
    return (int)B.e;
}

int du_direction(int R, int n_prob, const int* col, const int* head, const double* theta, const double* S, const double* Y,
                 const double* RHO, const double* g, const double* x, double* d, double* z) {
    if ((R != 8 && R != 16 && R != 32) || n_prob < 1) return (int)hipErrorInvalidValue;
    for (int p = 0; p < n_prob; ++p)
        if (col[p] < 0 || col[p] > 10 || head[p] < 0 || head[p] > 9) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    const size_t np = (size_t)n_prob;
    const int *dcol = B.put(col, np), *dhead = B.put(head, np);
    const double *dth = B.put(theta, np), *dS = B.put(S, np * 10 * R), *dY = B.put(Y, np * 10 * R), *dRHO = B.put(RHO, np * 10);
    const double *dg = B.put(g, np * R), *dx = B.put(x, np * R);
    double *dd = B.put(d, np * R), *dz = B.put(z, np * R);
    if (B.e == hipSuccess) {
        const dim3 grid((n_prob + 3) / 4), block(256);
        if (R == 8) launch(k_direction<8>, grid, block, n_prob, dcol, dhead, dth, dS, dY, dRHO, dg, dx, dd, dz);
        else if (R == 16) launch(k_direction<16>, grid, block, n_prob, dcol, dhead, dth, dS, dY, dRHO, dg, dx, dd, dz);
        else launch(k_direction<32>, grid, block, n_prob, dcol, dhead, dth, dS, dY, dRHO, dg, dx, dd, dz);
    }
    B.done();
    B.get(d, dd, np * R);
    B.get(z, dz, np * R);
    return (int)B.e;
}

// form 0: lbfgsb_wave<P, R> (block_threads 64 or 256: one or four problems per block); form 1 / 2:
// lbfgsb_nd<R, ., 10, OneLane / DeviceWave> (P ignored, R = NMAX in {8, 16, 32, 48}; 64-thread blocks)
int du_optimise(int form, int P, int R, int block_threads, int n, int n_prob, unsigned long long pattern, const double* Q,
             const double* c, const double* w, const double* x0, const double* l, const double* u, const int* nbd,
             double* tx, double* tf, double* tg, double* xout, double* fout, int* res) {
    if (n < 1 || n_prob < 1 || (block_threads != 64 && block_threads != 256)) return (int)hipErrorInvalidValue;
    if (form == 0 ? (n > P || P > R || (P < R && n != P)) : (n > R || block_threads != 64)) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    const size_t np = (size_t)n_prob, nn = (size_t)n;
    OptArgs a;
    a.n = n; a.n_prob = n_prob; a.pattern = pattern;
    a.Q = B.put(Q, np * nn * nn); a.c = B.put(c, np * nn); a.w = B.put(w, np * nn); a.x0 = B.put(x0, np * nn);
    a.l = B.put(l, np * nn); a.u = B.put(u, np * nn); a.nbd = B.put(nbd, np * nn);
    a.tx = B.put(tx, np * kTraceCap * nn); a.tf = B.put(tf, np * kTraceCap); a.tg = B.put(tg, np * kTraceCap * nn);
    a.xout = B.put(xout, np * nn); a.fout = B.put(fout, np); a.res = B.put(res, np * 5);
    bool found = false;
    if (B.e == hipSuccess) {
        const int per = block_threads / 64;
        const dim3 gw((n_prob + per - 1) / per), bw(block_threads), gn(n_prob), bn(64);
#define DU_WAVE(P_, R_) if (form == 0 && P == P_ && R == R_) { launch(k_wave_opt<P_, R_>, gw, bw, a); found = true; }
        DU_WAVE(5, 8) DU_WAVE(7, 8) DU_WAVE(8, 8) DU_WAVE(9, 16) DU_WAVE(12, 16) DU_WAVE(16, 16) DU_WAVE(32, 32)
#undef DU_WAVE
#define DU_ND(R_) \
        if (form == 1 && R == R_) { launch(k_nd_opt<R_, OneLane>, gn, bn, a); found = true; } \
        if (form == 2 && R == R_) { launch(k_nd_opt<R_, DeviceWave>, gn, bn, a); found = true; }
        DU_ND(8) DU_ND(16) DU_ND(32) DU_ND(48)
#undef DU_ND
    }
    if (B.e == hipSuccess && !found) return (int)hipErrorInvalidValue;
    B.done();
    B.get(tx, a.tx, np * kTraceCap * nn); B.get(tf, a.tf, np * kTraceCap); B.get(tg, a.tg, np * kTraceCap * nn);
    B.get(xout, a.xout, np * nn); B.get(fout, a.fout, np); B.get(res, a.res, np * 5);
    return (int)B.e;
}

int du_lbp(int wave64, int op, int lda, int n_prob, const int* n, double* a, double* b, double* sacc, int* ret) {
    if (op < 0 || op > 3 || lda < 1 || lda > kLdaMax || n_prob < 1) return (int)hipErrorInvalidValue;
    for (int p = 0; p < n_prob; ++p)
        if (n[p] < 1 || (op == 3 ? 2 * n[p] : n[p]) > lda) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    const size_t np = (size_t)n_prob;
    const int* dn = B.put(n, np);
    double *da = B.put(a, np * lda * lda), *db = B.put(b, np * lda), *ds = B.put(sacc, np * lda);
    int* dr = B.put(ret, np * 64);
    if (B.e == hipSuccess) {
        if (wave64) launch(k_lbp<DeviceWave>, dim3(n_prob), dim3(64), op, lda, dn, da, db, ds, dr);
        else launch(k_lbp<OneLane>, dim3(n_prob), dim3(64), op, lda, dn, da, db, ds, dr);
    }
    B.done();
    B.get(a, da, np * lda * lda); B.get(b, db, np * lda); B.get(sacc, ds, np * lda); B.get(ret, dr, np * 64);
    return (int)B.e;
}

}  // extern "C"
