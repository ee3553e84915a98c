// devunit_alpha.hip — TEST-ONLY device build of the dispersion objective (never linked into the package).
//
// dsq_alpha.h's alpha_eval / alpha_const / alpha_const_max are header templates and are called here from small kernels,
// one gene per wavefront and four per 256-thread block, as k_alpha calls them: the count memo (NB = 1, 2, 4), the
// LDS-staged padded rows (PAD), the per-cell accumulation (CELL) and the software-pipelined loop exist in the 64-lane
// build only.  The row kernels (dsq_k_alpha_rows.hip, dsq_k_alpha_rowsc.hip) carry their own restatement of the
// objective; the two units are linked into the test library unchanged and launched through dsq_launch.h with a
// caller-given evaluation cap, which leaves the k-th evaluation's (f, g) and the next point in every parked gene's
// optimiser state.  No function body of the product is restated here.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "devunit_host.h"
#include "dsq_alpha.h"
#include "dsq_alpha_rows.h"
#include "dsq_launch.h"

using namespace dsq;
using devunit::Bufs;

namespace dsq {
size_t alpha_rows_smem(int N);  // dsq_k_alpha_rows.hip
}

namespace {

// ------------------------------------------------------------------------------------------------ alpha_eval
// y / mu: [G][ldn], la / la_hat: [G] (la_hat = log alpha_hat as AlphaArgs holds it) -> f / g: [G][64] (every lane's
// result), cst: [G] (alpha_const of the rows the evaluation read).  The rows of a PAD instantiation are staged in the
// wave's LDS segment with k_alpha's layout - mu [npad], then the counts [npad] - padded with (0, 0.0); the cells' tables
// of a CELL instantiation lie behind the four segments, a CellWork<P> and a CellCtx per wave, as in k_alpha<P, true, true>.
template <int P, bool GRAD, bool PAD, int NB, bool CELL>
__global__ void __launch_bounds__(kBlock) k_eval(const int32_t* __restrict__ y, const double* __restrict__ mu, int ldn,
                                                 const double* __restrict__ Xt, int ldx, int N, int G,
                                                 const double* __restrict__ la, const double* __restrict__ la_hat,
                                                 double prior_var, int cr_reg, int prior_reg, CellDesign cells,
                                                 double* __restrict__ f, double* __restrict__ g,
                                                 double* __restrict__ cst) {
    __shared__ typename std::conditional<CELL, CellWork<P>, char>::type cellw[kWavesPerBlock];
    __shared__ CellCtx cellctx[kWavesPerBlock];
    extern __shared__ __attribute__((aligned(16))) double stage[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gk = blockIdx.x * kWavesPerBlock + w;
    const int npad = (N + 63) & ~63;
    log_tab_fill();
    if (CELL) {
        constexpr int T = Tri<P>::N;
        double* sXX = stage + (size_t)kWavesPerBlock * (npad + npad / 2);
        double* sXc = sXX + cells.C * T;
        for (int i = threadIdx.x; i < cells.C * T; i += kBlock) sXX[i] = cells.XX[i];
        for (int i = threadIdx.x; i < cells.C * P; i += kBlock) sXc[i] = cells.Xc[i];
        cells.XX = sXX;
        cells.Xc = sXc;
    }
    __syncthreads();
    if (gk >= G) return;
    if (CELL && lane == 0) {
        cellctx[w].D = cells;
        cellctx[w].ws = (void*)&cellw[w];
    }
    const int32_t* yg = y + (size_t)gk * ldn;
    const double* mg = mu + (size_t)gk * ldn;
    if (PAD) {
        double* ms = stage + (size_t)w * (npad + npad / 2);
        int32_t* ys = (int32_t*)(ms + npad);
        for (int n = lane; n < npad; n += 64) {
            ms[n] = n < N ? mg[n] : 0.0;
            ys[n] = n < N ? yg[n] : 0;
        }
        yg = ys;
        mg = ms;
    }
    DeviceWave::sync();
    AlphaArgs A;
    A.y = yg; A.mu = mg; A.Xt = Xt; A.ldx = ldx; A.N = N;
    A.la_hat = la_hat[gk];
    A.prior_var = prior_var;
    A.cell = CELL ? &cellctx[w] : nullptr;
    A.cst = alpha_const<DeviceWave>(yg, mg, N);
    double fv, gv;
    alpha_eval<DeviceWave, P, GRAD, PAD, NB, CELL>(A, la[gk], cr_reg != 0, prior_reg != 0, fv, gv);
    f[(size_t)gk * 64 + lane] = fv;
    g[(size_t)gk * 64 + lane] = gv;
    if (lane == 0) cst[gk] = A.cst;
}

// (P, GRAD, PAD, NB, CELL): the staged evaluation of k_alpha at every width; the un-staged one (rows too long for the
// LDS) at a narrow and a split-sweep width; the loss-only form of the grid search; the cell path at an out-of-line and
// an inlined width.  tests/devunit/__init__.py (EVAL_INST) holds the same list.
#define DU_NB(X, P_, G_, D_, C_) X(P_, G_, D_, 1, C_) X(P_, G_, D_, 2, C_) X(P_, G_, D_, 4, C_)
#define DU_EVAL_LIST(X)                                                                                            \
    DU_NB(X, 1, 1, 1, 0) DU_NB(X, 2, 1, 1, 0) DU_NB(X, 3, 1, 1, 0) DU_NB(X, 4, 1, 1, 0) DU_NB(X, 8, 1, 1, 0)         \
    DU_NB(X, 9, 1, 1, 0) DU_NB(X, 12, 1, 1, 0) DU_NB(X, 2, 1, 0, 0) DU_NB(X, 9, 1, 0, 0) DU_NB(X, 2, 0, 0, 0)        \
    DU_NB(X, 8, 0, 0, 0) DU_NB(X, 3, 1, 1, 1) DU_NB(X, 8, 1, 1, 1)

// alpha_const and alpha_const_max on the same rows: c / cm [G][64], mx [G][64]
__global__ void __launch_bounds__(kBlock) k_const(const int32_t* __restrict__ y, const double* __restrict__ mu, int ldn,
                                                  int N, int G, double* __restrict__ c, double* __restrict__ cm,
                                                  int* __restrict__ mx) {
    log_tab_fill();
    __syncthreads();
    const int gk = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gk >= G) return;
    const int32_t* yg = y + (size_t)gk * ldn;
    const double* mg = mu + (size_t)gk * ldn;
    int m = -1;
    c[(size_t)gk * 64 + lane] = alpha_const<DeviceWave>(yg, mg, N);
    cm[(size_t)gk * 64 + lane] = alpha_const_max<DeviceWave>(yg, mg, N, m);
    mx[(size_t)gk * 64 + lane] = m;
}

struct RowsArgs {
    int route;  // 0: k_alpha_rows (P = C <= 4), 1: k_alpha_rows_c from coefficients, 2: k_alpha_rows_c from cell_mu
    int wg;     // != 0: then k_alpha_wg on the parked states
    const int32_t* y; int ldn, N, G;
    const int32_t* list; int n_list;
    const double *coef, *cell_mu, *sf;
    const int32_t* cell_of; const double *Xc, *XX; int C, P;
    double min_mu; const double* alpha_hat; double min_disp, max_disp, prior_var; int prior_reg, const_mode, eval_cap;
};

}  // namespace

extern "C" {

int du_cus() { return current_device_cus(); }
int du_rowsc_tail(int N, int P, int C) { return alpha_rowsc_tail(N, P, C); }
int du_row_tail() { return kRowTail; }

int du_alpha_eval(int P, int grad, int pad, int nb, int cell, const int32_t* y, const double* mu, int ldn,
                  const double* Xt, int ldx, int N, int G, const double* la, const double* la_hat, double prior_var,
                  int cr_reg, int prior_reg, const int32_t* cell_of, const double* Xc, const double* XX, int C, double* f,
                  double* g, double* cst) {
    if (N < 1 || G < 1 || ldn < N || ldx < N || !y || !mu || !Xt || !la || !la_hat || !f || !g || !cst)
        return (int)hipErrorInvalidValue;
    if (cell && (!cell_of || !Xc || !XX || C < 1 || C > kMaxCells || !pad)) return (int)hipErrorInvalidValue;
    const int T = P * (P + 1) / 2;
    Bufs B;
    const int32_t* dy = B.put(y, (size_t)G * ldn);
    const double* dmu = B.put(mu, (size_t)G * ldn);
    const double* dX = B.put(Xt, (size_t)P * ldx);
    const double* dla = B.put(la, G);
    const double* dlh = B.put(la_hat, G);
    CellDesign D{};
    if (cell) {
        D.cell_of = B.put(cell_of, ldx);
        D.Xc = B.put(Xc, (size_t)C * P);
        D.XX = B.put(XX, (size_t)C * T);
        D.C = C;
    }
    double* df = B.put(f, (size_t)G * 64);
    double* dg = B.put(g, (size_t)G * 64);
    double* dc = B.put(cst, G);
    if (B.e != hipSuccess) return (int)B.e;
    const int npad = (N + 63) & ~63;
    size_t smem = pad ? (size_t)kWavesPerBlock * (npad + npad / 2) * sizeof(double) : 0;
    if (cell) smem += (size_t)C * (T + P) * sizeof(double);
    if (smem > 48 * 1024) return (int)hipErrorInvalidValue;
    bool found = false;
#define DU_X(P_, G_, D_, N_, C_)                                                                                       \
    if (!found && P == P_ && (grad != 0) == (G_ != 0) && (pad != 0) == (D_ != 0) && nb == N_ && (cell != 0) == (C_ != 0)) { \
        hipLaunchKernelGGL((k_eval<P_, G_ != 0, D_ != 0, N_, C_ != 0>), dim3(genes_to_blocks(G)), dim3(kBlock), smem, 0,   \
                           dy, dmu, ldn, dX, ldx, N, G, dla, dlh, prior_var, cr_reg, prior_reg, D, df, dg, dc);        \
        found = true;                                                                                                  \
    }
    DU_EVAL_LIST(DU_X)
#undef DU_X
    if (!found) return (int)hipErrorInvalidValue;
    B.done();
    B.get(f, df, (size_t)G * 64);
    B.get(g, dg, (size_t)G * 64);
    B.get(cst, dc, G);
    return (int)B.e;
}

int du_alpha_const(const int32_t* y, const double* mu, int ldn, int N, int G, double* c, double* cm, int* mx) {
    if (N < 1 || G < 1 || ldn < N || !y || !mu || !c || !cm || !mx) return (int)hipErrorInvalidValue;
    Bufs B;
    const int32_t* dy = B.put(y, (size_t)G * ldn);
    const double* dmu = B.put(mu, (size_t)G * ldn);
    double* dc = B.put(c, (size_t)G * 64);
    double* dcm = B.put(cm, (size_t)G * 64);
    int* dmx = B.put(mx, (size_t)G * 64);
    if (B.e != hipSuccess) return (int)B.e;
    hipLaunchKernelGGL(k_const, dim3(genes_to_blocks(G)), dim3(kBlock), 0, 0, dy, dmu, ldn, N, G, dc, dcm, dmx);
    B.done();
    B.get(c, dc, (size_t)G * 64);
    B.get(cm, dcm, (size_t)G * 64);
    B.get(mx, dmx, (size_t)G * 64);
    return (int)B.e;
}

}  // extern "C"

namespace {

// One launch of a row kernel with its own zeroed queue, grid and park counters.  Every output holds the caller's
// sentinels where the kernels did not write.  st_d [G][5]: x, f, g, xold, fold and st_i [G][5]: nfev, it, col, done,
// status of the parked genes' optimiser states, read through the struct.
int rows_run(const RowsArgs& a, double* nll_const, double* alpha, uint8_t* conv, int32_t* nfev, int32_t* grid_list,
             int32_t* grid_count, int32_t* park_list, int32_t* park_count, double* st_d, int32_t* st_i, double* wg_alpha,
             uint8_t* wg_conv, int32_t* wg_nfev, int32_t* wg_grid_list, int32_t* wg_grid_count) {
    const int G = a.G, P = a.P, C = a.C, T = P * (P + 1) / 2;
    if (G < 1 || a.N < 1 || a.N > 65535 || a.ldn < a.N || a.n_list < 1 || a.n_list > G || P < 1 || C < 1 || a.eval_cap < 0)
        return (int)hipErrorInvalidValue;
    if (!a.y || !a.sf || !a.cell_of || !a.Xc || !a.XX || !a.alpha_hat || !nll_const || !alpha || !conv || !nfev ||
        !grid_list || !grid_count || !park_list || !park_count || !st_d || !st_i)
        return (int)hipErrorInvalidValue;
    if (a.route == 0 ? (P != C || P > 4 || !a.coef || alpha_rows_smem(a.N) > 160 * 1024)
                     : (a.route == 1 ? !a.coef : (a.route == 2 ? !a.cell_mu : true)))
        return (int)hipErrorInvalidValue;
    if (a.route != 0 && alpha_rowsc_tail(a.N, P, C) == 0) return (int)hipErrorInvalidValue;
    if (a.wg && (a.route != 0 || a.eval_cap < 1 || a.const_mode == DSQ_CONST_COMPUTE || !alpha_wg_eligible(a.N) ||
                 !wg_alpha || !wg_conv || !wg_nfev || !wg_grid_list || !wg_grid_count))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < a.n_list && a.list != nullptr; ++k)
        if (a.list[k] < 0 || a.list[k] >= G) return (int)hipErrorInvalidValue;
    for (int n = 0; n < a.N; ++n)
        if (a.cell_of[n] < 0 || a.cell_of[n] >= C) return (int)hipErrorInvalidValue;
    Bufs B;
    const int32_t* dy = B.put(a.y, (size_t)G * a.ldn);
    const int32_t* dlist = B.put(a.list, a.n_list);
    const double* dcoef = a.route != 2 ? B.put(a.coef, (size_t)G * P) : nullptr;
    const double* dcm = a.route == 2 ? B.put(a.cell_mu, (size_t)G * C) : nullptr;
    const double* dsf = B.put(a.sf, a.N);
    CellDesign D{};
    D.cell_of = B.put(a.cell_of, a.N);
    D.Xc = B.put(a.Xc, (size_t)C * P);
    D.XX = B.put(a.XX, (size_t)C * T);
    D.C = C;
    const double* dah = B.put(a.alpha_hat, G);
    double* dnc = B.put(nll_const, G);
    double* dal = B.put(alpha, G);
    uint8_t* dcv = B.put(conv, G);
    int32_t* dnf = B.put(nfev, G);
    int32_t* dgl = B.put(grid_list, G);
    int32_t* dpl = B.put(park_list, G);
    int32_t* cnt = B.alloc<int32_t>(8);  // queue [0 .. 3], grid count [4], park count [5], k_alpha_wg's grid count [6]
    Lbfgsb1d* dst = B.alloc<Lbfgsb1d>(G);
    double* dwa = a.wg ? B.put(wg_alpha, G) : nullptr;
    uint8_t* dwc = a.wg ? B.put(wg_conv, G) : nullptr;
    int32_t* dwn = a.wg ? B.put(wg_nfev, G) : nullptr;
    int32_t* dwl = a.wg ? B.put(wg_grid_list, G) : nullptr;
    if (B.e != hipSuccess) return (int)B.e;
    B.chk(hipMemset(cnt, 0, 8 * sizeof(int32_t)));
    B.chk(hipMemset(dst, 0xFF, (size_t)G * sizeof(Lbfgsb1d)));
    if (B.e != hipSuccess) return (int)B.e;
    if (a.route == 0)
        B.chk(launch_alpha_rows(0, dy, a.ldn, a.N, dlist, a.n_list, cnt, dcoef, dsf, D, P, a.min_mu, dah, a.min_disp,
                                a.max_disp, a.prior_var, 1, a.prior_reg, dal, dcv, dnf, cnt + 4, dgl, dnc, a.const_mode,
                                a.eval_cap, dst, cnt + 5, dpl));
    else
        B.chk(launch_alpha_rows_c(0, dy, a.ldn, a.N, dlist, a.n_list, cnt, dcoef, dcm, dsf, D, P, a.min_mu, dah,
                                  a.min_disp, a.max_disp, a.prior_var, a.prior_reg, dal, dcv, dnf, cnt + 4, dgl, dnc,
                                  a.const_mode, a.eval_cap, dst, cnt + 5, dpl));
    if (B.e == hipSuccess && a.wg)
        B.chk(launch_alpha_wg(0, dy, a.ldn, a.N, dpl, cnt + 5, a.n_list, dcoef, dsf, D, P, a.min_mu, dah, a.prior_var,
                              a.prior_reg, dwa, dwc, dwn, cnt + 6, dwl, dnc, dst));
    B.done();
    int32_t hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    B.get(hc, cnt, 8);
    B.get(nll_const, dnc, G);
    B.get(alpha, dal, G);
    B.get(conv, dcv, G);
    B.get(nfev, dnf, G);
    B.get(grid_list, dgl, G);
    B.get(park_list, dpl, G);
    std::vector<Lbfgsb1d> st(G);
    B.get(st.data(), dst, G);
    if (a.wg) {
        B.get(wg_alpha, dwa, G);
        B.get(wg_conv, dwc, G);
        B.get(wg_nfev, dwn, G);
        B.get(wg_grid_list, dwl, G);
    }
    if (B.e != hipSuccess) return (int)B.e;
    *grid_count = hc[4];
    *park_count = hc[5];
    if (a.wg) *wg_grid_count = hc[6];
    for (int k = 0; k < hc[5] && k < G; ++k) {
        const int g = park_list[k];
        if (g < 0 || g >= G) continue;
        const Lbfgsb1d& m = st[g];
        double* d = st_d + (size_t)g * 5;
        int32_t* i = st_i + (size_t)g * 5;
        d[0] = m.x; d[1] = m.f; d[2] = m.g; d[3] = m.xold; d[4] = m.fold;
        i[0] = m.nfev; i[1] = m.it; i[2] = m.col; i[3] = m.done ? 1 : 0; i[4] = m.status;
    }
    return (int)B.e;
}

}  // namespace

extern "C" {

int du_rows_trace(int route, const int32_t* y, int ldn, int N, int G, const int32_t* list, int n_list, const double* coef,
                  const double* cell_mu, const double* sf, const int32_t* cell_of, const double* Xc, const double* XX,
                  int C, int P, double min_mu, const double* alpha_hat, double min_disp, double max_disp,
                  double prior_var, int prior_reg, int const_mode, int eval_cap, double* nll_const, double* alpha,
                  uint8_t* conv, int32_t* nfev, int32_t* grid_list, int32_t* grid_count, int32_t* park_list,
                  int32_t* park_count, double* st_d, int32_t* st_i) {
    const RowsArgs a{route, 0, y, ldn, N, G, list, n_list, coef, cell_mu, sf, cell_of, Xc, XX, C, P, min_mu, alpha_hat,
                     min_disp, max_disp, prior_var, prior_reg, const_mode, eval_cap};
    return rows_run(a, nll_const, alpha, conv, nfev, grid_list, grid_count, park_list, park_count, st_d, st_i, nullptr,
                    nullptr, nullptr, nullptr, nullptr);
}

// the row launch of du_rows_trace (route 0, eval_cap >= 1, the constants stored or loaded), then k_alpha_wg on what it
// parked; the wg_* arrays are what k_alpha_wg wrote
int du_alpha_wg(const int32_t* y, int ldn, int N, int G, const int32_t* list, int n_list, const double* coef,
                const double* sf, const int32_t* cell_of, const double* Xc, const double* XX, int P, double min_mu,
                const double* alpha_hat, double min_disp, double max_disp, double prior_var, int prior_reg,
                int const_mode, int eval_cap, double* nll_const, double* alpha, uint8_t* conv, int32_t* nfev,
                int32_t* grid_list, int32_t* grid_count, int32_t* park_list, int32_t* park_count, double* st_d,
                int32_t* st_i, double* wg_alpha, uint8_t* wg_conv, int32_t* wg_nfev, int32_t* wg_grid_list,
                int32_t* wg_grid_count) {
    const RowsArgs a{0, 1, y, ldn, N, G, list, n_list, coef, nullptr, sf, cell_of, Xc, XX, P, P, min_mu, alpha_hat,
                     min_disp, max_disp, prior_var, prior_reg, const_mode, eval_cap};
    return rows_run(a, nll_const, alpha, conv, nfev, grid_list, grid_count, park_list, park_count, st_d, st_i, wg_alpha,
                    wg_conv, wg_nfev, wg_grid_list, wg_grid_count);
}

}  // extern "C"
