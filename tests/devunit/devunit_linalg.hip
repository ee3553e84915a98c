// devunit_linalg.hip — TEST-ONLY device build of the p x p algebra and the fp64 MFMA Gram (never linked into the package).
//
// tests/hostsim and tests/hostwide compile dsq_wide.h with g++ and the one-lane HostWave: the plain-sum branch of
// WideGram, empty barriers, `i += Wv::W` = `++i`.  This unit compiles dsq_wide.h / dsq_wider.h / dsq_linalg.h with hipcc
// for gfx950 under the product's CXXFLAGS and calls, from small kernels, what only the device build has: the three
// v_mfma_f64_16x16x4_f64 layouts of WideGram, the lane-parallel Cholesky / solve / inverse / Frobenius product with 64
// lanes and real barriers, the rpart / rpart2 right-hand side of the IRLS sweep, and row_chol_solve on sixteen-lane rows.
// No function body of the headers is restated here: a change to a header changes what is tested.
//
// Workspaces are bound as the product binds them:
//   MP = 48  (DeviceWave, WideWork::bind):      one gene per wavefront on a wave-private segment of dynamic LDS, 4 / 2 / 1
//                                               waves per block by the 64 KB rule of dsq_k_wide.hip;
//   MP = 128 (SlotWave, WiderWork::bind_split): one gene per 64-thread block at a time, LDS plus one slot of
//                                               wider_slot_doubles(P) of device memory per block, blocks looping over genes.
// Before every gene the whole workspace is filled with NaN, so that stale contents cannot pass for a result.
// Every entry point allocates, copies, launches, synchronises and frees on its own and returns the first hipError_t
// (hipErrorInvalidValue for a bad argument).
#include <hip/hip_runtime.h>

#include "devunit_host.h"
#include "dsq_dispatch.h"
#include "dsq_linalg.h"
#include "dsq_wave.h"
#include "dsq_wider.h"

using namespace dsq;

namespace {

template <int MP>
struct Fam;
template <>
struct Fam<kWideMaxP> {
    using Wv = DeviceWave;
    using Work = WideWork;
};
template <>
struct Fam<kWiderMaxP> {
    using Wv = SlotWave;
    using Work = WiderWork;
};

// where a launch puts its genes (host) and what the kernels need to bind their workspaces (device)
struct Geom {
    int P, G;
    int per_wave_doubles;  // MP = 48: doubles of LDS per wave
    double* slots;         // MP = 128: device memory, one slot per block
    size_t slot_doubles;
};
struct Launch {
    Geom g;
    dim3 grid, block;
    size_t lds;
};

// false: bad argument.  blocks: MP = 128 only, workgroups (= slots) that share the G genes (<= 0: one per gene)
bool make_launch(int mp, int P, int G, int blocks, devunit::Bufs& B, Launch& L) {
    if ((mp != kWideMaxP && mp != kWiderMaxP) || P < 1 || P > mp || G < 1) return false;
    L.g = Geom{P, G, 0, nullptr, 0};
    if (mp == kWideMaxP) {
        const size_t per_wave = (size_t)wide_work_doubles(P) * sizeof(double);
        const int wpb = per_wave * 4 <= 64 * 1024 ? 4 : (per_wave * 2 <= 64 * 1024 ? 2 : 1);
        L.g.per_wave_doubles = wide_work_doubles(P);
        L.grid = dim3((G + wpb - 1) / wpb);
        L.block = dim3(64 * wpb);
        L.lds = per_wave * wpb;
    } else {
        const int n = blocks <= 0 || blocks > G ? G : blocks;
        L.g.slot_doubles = wider_slot_doubles(P);
        L.g.slots = B.alloc<double>((size_t)n * L.g.slot_doubles);
        L.grid = dim3(n);
        L.block = dim3(64);
        L.lds = (size_t)wider_lds_doubles(P) * sizeof(double);
    }
    return true;
}

template <class K>
void raise_lds(K kernel, size_t bytes, devunit::Bufs& B) {
    if (bytes > 48 * 1024) B.chk(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// every lane writes its share of NaN over the gene's whole workspace
template <class Wv>
__device__ __forceinline__ void poison(double* p, size_t n) {
    for (size_t i = Wv::lane(); i < n; i += 64) p[i] = __builtin_nan("");
}

// f(W, g) for every gene of this wavefront (MP = 48: one) / workgroup (MP = 128: g = blockIdx.x, + gridDim.x, ...)
template <int MP, class F>
__device__ __forceinline__ void each_gene(const Geom& ge, F&& f) {
    extern __shared__ __attribute__((aligned(16))) double du_lds[];
    using Wv = typename Fam<MP>::Wv;
    typename Fam<MP>::Work W;
    if constexpr (MP == kWideMaxP) {
        const int wv = threadIdx.x >> 6;
        const int g = blockIdx.x * (blockDim.x >> 6) + wv;
        if (g >= ge.G) return;
        W.bind(du_lds + (size_t)wv * ge.per_wave_doubles, ge.P);
        poison<Wv>(W.M, wide_work_doubles(ge.P));
        Wv::sync();
        f(W, g);
    } else {
        W.bind_split(du_lds, ge.slots + (size_t)blockIdx.x * ge.slot_doubles, ge.P);
        for (int g = blockIdx.x; g < ge.G; g += gridDim.x) {
            poison<Wv>(W.xs, wider_lds_doubles(ge.P));
            poison<Wv>(W.gacc, wider_slot_doubles(ge.P));
            Wv::sync();
            f(W, g);
            Wv::sync();
        }
    }
}

template <int MP>
constexpr int kThreads = MP > kWideMaxP ? 64 : 256;

// the whole P x ld array, pad column included
template <class Wv, class Work>
__device__ __forceinline__ void store_mat(const Work& W, const double* src, double* dst) {
    for (int e = Wv::lane(); e < W.P * W.ld; e += 64) dst[e] = src[e];
}

// ------------------------------------------------------------------------------------------------ WideGram
// Xt: [G][P][ldx], w0 / w1: [G][N] -> M / dM: [G][P][ld]; the call sequence of alpha_eval_wide / irls_sweep_wide
template <int MP, bool TWO>
__global__ void __launch_bounds__(kThreads<MP>) k_gram(Geom ge, int N, int ldx, const double* Xt, const double* w0,
                                                       const double* w1, double* M, double* dM) {
    using Wv = typename Fam<MP>::Wv;
    each_gene<MP>(ge, [&](const typename Fam<MP>::Work& W, int g) {
        const double* X = Xt + (size_t)g * ge.P * ldx;
        WideGram<Wv, TWO, MP> gram;
        gram.begin(W);
        wide_zero_pad_rows<Wv>(W);
        Wv::sync();
        const int n_end = ((N + 63) / 64) * 64;
        for (int n0 = 0; n0 < n_end; n0 += 64) {
            wide_stage_x<Wv>(W, X, ldx, N, n0);
            Wv::sync();
            const int l = Wv::lane(), n = n0 + l;
            W.w[l] = n < N ? w0[(size_t)g * N + n] : 0.0;
            if (TWO) W.w[64 + l] = n < N ? w1[(size_t)g * N + n] : 0.0;
            Wv::sync();
            gram.add_chunk(W);
            Wv::sync();
        }
        gram.finish(W);
        store_mat<Wv>(W, W.M, M + (size_t)g * W.P * W.ld);
        store_mat<Wv>(W, W.dM, dM + (size_t)g * W.P * W.ld);
    });
}

// ------------------------------------------------------------------------------------------------ LDS / slot algebra
enum LinOp { kChol = 0, kLogdet, kSolve, kInverse, kFrob, kQuadXs, kCells, kLinOps };

// in0: [G][n0], in1: [G][n1] (null where the op has one input), out: [G][nout].  Matrices come in dense, row major
// (P x P) and go out as the workspace holds them (P x ld).  A factor or a matrix to factor is loaded as its lower
// triangle only: the strict upper triangle keeps the NaN.
template <int MP>
__global__ void __launch_bounds__(kThreads<MP>) k_linalg(Geom ge, int op, int C, double diag_add, const double* in0,
                                                         int n0, const double* in1, int n1, double* out, int nout) {
    using Wv = typename Fam<MP>::Wv;
    each_gene<MP>(ge, [&](const typename Fam<MP>::Work& W, int g) {
        const int P = W.P, ld = W.ld, lane = Wv::lane();
        const double* a = in0 + (size_t)g * n0;
        const double* b = in1 != nullptr ? in1 + (size_t)g * n1 : nullptr;
        double* o = out + (size_t)g * nout;
        auto load = [&](double* dst, const double* src, bool lower) {
            for (int e = lane; e < P * P; e += 64) {
                const int i = e / P, j = e % P;
                if (!lower || j <= i) dst[i * ld + j] = src[e];
            }
        };
        switch (op) {
            case kChol:  // a: A -> L
                load(W.M, a, true);
                Wv::sync();
                wide_chol<Wv>(W, W.M, W.L, diag_add);
                store_mat<Wv>(W, W.L, o);
                break;
            case kLogdet:  // a: L -> the value every lane got
                load(W.L, a, true);
                Wv::sync();
                o[lane] = wide_logdet<Wv>(W, W.L);
                break;
            case kSolve:  // a: L, b: right-hand side -> x
                load(W.L, a, true);
                for (int j = lane; j < P; j += 64) W.v(1)[j] = b[j];
                Wv::sync();
                wide_chol_solve<Wv>(W, W.L, W.v(1));
                for (int j = lane; j < P; j += 64) o[j] = W.v(1)[j];
                break;
            case kInverse:  // a: L -> Li, inv
                load(W.L, a, true);
                Wv::sync();
                wide_inverse<Wv>(W, W.L, W.Li, W.inv);
                store_mat<Wv>(W, W.Li, o);
                store_mat<Wv>(W, W.inv, o + P * ld);
                break;
            case kFrob:  // a, b: symmetric matrices -> the value every lane got
                load(W.inv, a, false);
                load(W.dM, b, false);
                Wv::sync();
                o[lane] = wide_frob<Wv>(W, W.inv, W.dM);
                break;
            case kQuadXs:  // a: symmetric matrix, b: xs as [P][64] -> lane = column
                load(W.inv, a, false);
                for (int j = 0; j < P; ++j) W.xs[j * kWideXsLd + lane] = b[j * 64 + lane];
                Wv::sync();
                o[lane] = wide_quad_xs(W, W.inv, lane);
                break;
            case kCells: {  // a: Xc [C][P] (device memory, as the product keeps it), b: cell sums [C] -> M
                CellDesign D;
                D.cell_of = nullptr; D.Xc = a; D.XX = nullptr; D.C = C;
                for (int c = lane; c < C; c += 64) W.acc[c] = b[c];
                Wv::sync();
                wide_gram_from_cells<Wv>(W, D, W.acc, W.M);
                Wv::sync();
                store_mat<Wv>(W, W.M, o);
                break;
            }
            default: break;
        }
    });
}

// ------------------------------------------------------------------------------------------------ IRLS right-hand side
// one irls_sweep_wide (general Gram path, cells == nullptr) at the given beta: W.v(1) = X^T (w z) from rpart / rpart2
// and W.M = X^T W X.  Xt: [G][P][ldx], y / sf: [G][N], beta: [G][P] -> v1: [G][P], M: [G][P][ld]
template <int MP>
__global__ void __launch_bounds__(kThreads<MP>) k_irls_rhs(Geom ge, int N, int ldx, const double* Xt, const int32_t* y,
                                                           const double* sf, const double* beta, double disp,
                                                           double min_mu, double a, double* v1, double* M) {
    using Wv = typename Fam<MP>::Wv;
    each_gene<MP>(ge, [&](const typename Fam<MP>::Work& W, int g) {
        const int P = W.P;
        IrlsArgs A{};
        A.y = y + (size_t)g * N;
        A.sf = sf + (size_t)g * N;
        A.lsf = nullptr;
        A.Xt = Xt + (size_t)g * P * ldx;
        A.pinvXt = nullptr;
        A.ldx = ldx;
        A.N = N;
        A.disp = disp;
        A.min_mu = min_mu;
        A.full_rank = false;
        for (int j = Wv::lane(); j < P; j += 64) W.v(0)[j] = beta[(size_t)g * P + j];
        Wv::sync();
        double S;
        irls_sweep_wide<Wv>(A, W, a, S);
        for (int j = Wv::lane(); j < P; j += 64) v1[(size_t)g * P + j] = W.v(1)[j];
        store_mat<Wv>(W, W.M, M + (size_t)g * P * W.ld);
    });
}

// ------------------------------------------------------------------------------------------------ row_chol_solve
// sixteen genes per 256-thread block, four per wavefront: ent: [G][T + P] (packed lower triangle, then b) through LDS
// -> x: [G][16 lanes][P].  even_only: rows 1 and 3 of every wavefront leave before the solve (as k_wave, devunit.hip)
constexpr int kRowB = 256;
template <int P>
__global__ void __launch_bounds__(kRowB) k_row_solve(int G, int even_only, const double* ent, double ridge, double* x) {
    constexpr int E = Tri<P>::N + P;
    __shared__ double s_ent[(kRowB / 16) * E];
    const int g0 = blockIdx.x * (kRowB / 16);
    for (int t = threadIdx.x; t < (kRowB / 16) * E; t += kRowB)
        s_ent[t] = g0 + t / E < G ? ent[(size_t)g0 * E + t] : 1.0;
    __syncthreads();
    const int row = threadIdx.x >> 4, g = g0 + row;
    if (g >= G) return;
    if (even_only && (row & 1) != 0) return;
    const double* e = s_ent + row * E;
    double xs[P];
    row_chol_solve<RowWave, P>(e, ridge, xs);
#pragma unroll
    for (int j = 0; j < P; ++j) x[((size_t)g * 16 + RowWave::lane()) * P + j] = xs[j];
}

}  // namespace

extern "C" {

// mp: 48 or 128; two: also X^T diag(w1) X into dM (w1 may be null otherwise); blocks: see make_launch
int du_gram(int mp, int two, int P, int N, int ldx, int G, int blocks, const double* Xt, const double* w0,
            const double* w1, double* M, double* dM) {
    if (N < 1 || ldx < N || !Xt || !w0 || (two && !w1) || !M || !dM) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    Launch L;
    if (!make_launch(mp, P, G, blocks, B, L)) return (int)hipErrorInvalidValue;
    const size_t nm = (size_t)G * P * wide_ld(P);
    const double* dX = B.put(Xt, (size_t)G * P * ldx);
    const double* d0 = B.put(w0, (size_t)G * N);
    const double* d1 = B.put(w1, two ? (size_t)G * N : 0);
    double* dMm = B.put(M, nm);
    double* ddM = B.put(dM, nm);
    if (B.e != hipSuccess) return (int)B.e;
#define DU_GRAM(MP_, TWO_)                                                                                           \
    do {                                                                                                             \
        raise_lds(k_gram<MP_, TWO_>, L.lds, B);                                                                      \
        if (B.e == hipSuccess)                                                                                       \
            hipLaunchKernelGGL((k_gram<MP_, TWO_>), L.grid, L.block, L.lds, 0, L.g, N, ldx, dX, d0, d1, dMm, ddM);   \
    } while (0)
    if (mp == kWideMaxP) { if (two) DU_GRAM(kWideMaxP, true); else DU_GRAM(kWideMaxP, false); }
    else { if (two) DU_GRAM(kWiderMaxP, true); else DU_GRAM(kWiderMaxP, false); }
#undef DU_GRAM
    B.done();
    B.get(M, dMm, nm);
    B.get(dM, ddM, nm);
    return (int)B.e;
}

// op: LinOp; in0: [G][n0], in1: [G][n1] or null, out: [G][nout] (sizes per op: see k_linalg and tests/devunit/__init__.py)
int du_wide_linalg(int mp, int op, int P, int G, int blocks, int C, double diag_add, const double* in0, int n0,
                   const double* in1, int n1, double* out, int nout) {
    if (op < 0 || op >= kLinOps || !in0 || !out) return (int)hipErrorInvalidValue;
    if (P < 1 || P > kWiderMaxP) return (int)hipErrorInvalidValue;
    const int ld = wide_ld(P);
    const bool two_in = op == kSolve || op == kFrob || op == kQuadXs || op == kCells;
    const int need0 = op == kCells ? C * P : P * P;
    const int need1 = op == kSolve ? P : (op == kFrob ? P * P : (op == kQuadXs ? P * 64 : (op == kCells ? C : 0)));
    const int needo = op == kChol || op == kCells ? P * ld : (op == kInverse ? 2 * P * ld : (op == kSolve ? P : 64));
    if (op == kCells && (C < 1 || C > kMaxCells)) return (int)hipErrorInvalidValue;
    if (n0 != need0 || nout != needo || (two_in && (!in1 || n1 != need1))) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    Launch L;
    if (!make_launch(mp, P, G, blocks, B, L)) return (int)hipErrorInvalidValue;
    const double* d0 = B.put(in0, (size_t)G * n0);
    const double* d1 = B.put(in1, two_in ? (size_t)G * n1 : 0);
    double* d_o = B.put(out, (size_t)G * nout);
    if (B.e != hipSuccess) return (int)B.e;
    if (mp == kWideMaxP) {
        raise_lds(k_linalg<kWideMaxP>, L.lds, B);
        if (B.e == hipSuccess)
            hipLaunchKernelGGL(k_linalg<kWideMaxP>, L.grid, L.block, L.lds, 0, L.g, op, C, diag_add, d0, n0,
                               two_in ? d1 : nullptr, n1, d_o, nout);
    } else {
        raise_lds(k_linalg<kWiderMaxP>, L.lds, B);
        if (B.e == hipSuccess)
            hipLaunchKernelGGL(k_linalg<kWiderMaxP>, L.grid, L.block, L.lds, 0, L.g, op, C, diag_add, d0, n0,
                               two_in ? d1 : nullptr, n1, d_o, nout);
    }
    B.done();
    B.get(out, d_o, (size_t)G * nout);
    return (int)B.e;
}

int du_irls_rhs(int mp, int P, int N, int ldx, int G, int blocks, const double* Xt, const int32_t* y, const double* sf,
                const double* beta, double disp, double min_mu, double a, double* v1, double* M) {
    if (N < 1 || ldx < N || !Xt || !y || !sf || !beta || !v1 || !M) return (int)hipErrorInvalidValue;
    devunit::Bufs B;
    Launch L;
    if (!make_launch(mp, P, G, blocks, B, L)) return (int)hipErrorInvalidValue;
    const size_t nm = (size_t)G * P * wide_ld(P);
    const double* dX = B.put(Xt, (size_t)G * P * ldx);
    const int32_t* dy = B.put(y, (size_t)G * N);
    const double* dsf = B.put(sf, (size_t)G * N);
    const double* db = B.put(beta, (size_t)G * P);
    double* dv = B.put(v1, (size_t)G * P);
    double* dMm = B.put(M, nm);
    if (B.e != hipSuccess) return (int)B.e;
    if (mp == kWideMaxP) {
        raise_lds(k_irls_rhs<kWideMaxP>, L.lds, B);
        if (B.e == hipSuccess)
            hipLaunchKernelGGL(k_irls_rhs<kWideMaxP>, L.grid, L.block, L.lds, 0, L.g, N, ldx, dX, dy, dsf, db, disp,
                               min_mu, a, dv, dMm);
    } else {
        raise_lds(k_irls_rhs<kWiderMaxP>, L.lds, B);
        if (B.e == hipSuccess)
            hipLaunchKernelGGL(k_irls_rhs<kWiderMaxP>, L.grid, L.block, L.lds, 0, L.g, N, ldx, dX, dy, dsf, db, disp,
                               min_mu, a, dv, dMm);
    }
    B.done();
    B.get(v1, dv, (size_t)G * P);
    B.get(M, dMm, nm);
    return (int)B.e;
}

// P: 3 .. 12 (what k_irls_row instantiates) or 16; ent: [G][P (P + 1) / 2 + P], x: [G][16][P]
int du_row_solve(int P, int G, int even_only, const double* ent, double ridge, double* x) {
    if (G < 1 || !ent || !x) return (int)hipErrorInvalidValue;
    if (!((P >= 3 && P <= DSQ_REG_MAX_P) || P == 16)) return (int)hipErrorInvalidValue;
    const int E = P * (P + 1) / 2 + P;
    devunit::Bufs B;
    const double* de = B.put(ent, (size_t)G * E);
    double* dx = B.put(x, (size_t)G * 16 * P);
    if (B.e != hipSuccess) return (int)B.e;
    const dim3 grid((G + kRowB / 16 - 1) / (kRowB / 16)), block(kRowB);
    switch (P) {
#define DU_ROW(p) \
    case p: hipLaunchKernelGGL(k_row_solve<p>, grid, block, 0, 0, G, even_only, de, ridge, dx); break;
        DU_ROW(3) DU_ROW(4) DU_ROW(5) DU_ROW(6) DU_ROW(7) DU_ROW(8) DU_ROW(9) DU_ROW(10) DU_ROW(11) DU_ROW(12)
        DU_ROW(16)
#undef DU_ROW
        default: return (int)hipErrorInvalidValue;
    }
    B.done();
    B.get(x, dx, (size_t)G * 16 * P);
    return (int)B.e;
}

}  // extern "C"
