// devunit_stats.hip — TEST-ONLY device build of the trimmed statistics and the Cook's bookkeeping (never linked into the
// package).
//
// tests/hostsim compiles dsq_stats.h with the one-lane HostWave: one lane owns every histogram bin, the prefix scan
// returns 0, barriers are empty and list slots are handed out sequentially.  This unit instantiates the same templates
// with DeviceWave under the product's CXXFLAGS and calls them from small kernels: trimmed_sum_select, bucket_rank_sum and
// select_rank_sum (over a plain LDS buffer and over a NormedValues accessor), seg_trimmed_variances, CooksAcc, and the
// product's LdsSorter (dsq_lds_sort.h).  No function body of the headers is restated here.
//
// Every kernel runs 256 threads - four wavefronts, one problem each - on wave-private segments of dynamic LDS laid out
// as the product kernels lay them out: `cap` doubles of values with a BucketWork behind them.  (Where four such segments
// exceed the 160 KB of a workgroup, the last wavefronts of a block stay idle.)  Before anything else the block fills its
// whole LDS with a byte pattern given by the caller: no result may depend on it.
// Problems are rows of different lengths, concatenated, with offsets off[0 .. n_prob].  Every entry point allocates,
// copies, launches, synchronises and frees on its own and returns the first hipError_t (hipErrorInvalidValue for a bad
// argument).
#include <hip/hip_runtime.h>

#include "devunit_host.h"
#include "dsq_lds_sort.h"
#include "dsq_stats.h"

using namespace dsq;

namespace du_stats {  // (named: the assembly check reads all units as one translation unit)

using Wv = DeviceWave;
constexpr int kWorkDoubles = (int)((sizeof(BucketWork) + 7) / 8);
constexpr size_t kLdsMax = 160 * 1024;

struct Carve {
    int cap;     // doubles of values per wavefront
    int active;  // wavefronts of a block that take a problem
    int n_prob;
    unsigned long long pattern;
};

// fills the block's LDS; false: this wavefront has no problem
__device__ __forceinline__ bool carve(const Carve& c, double*& buf, BucketWork*& W, int& p) {
    extern __shared__ __attribute__((aligned(16))) double du_lds[];
    const int stride = c.cap + kWorkDoubles;
    unsigned long long* raw = (unsigned long long*)du_lds;
    for (int i = threadIdx.x; i < c.active * stride; i += blockDim.x) raw[i] = c.pattern;
    __syncthreads();
    const int w = threadIdx.x >> 6;
    p = blockIdx.x * c.active + w;
    if (w >= c.active || p >= c.n_prob) return false;
    buf = du_lds + (size_t)w * stride;
    W = (BucketWork*)(buf + c.cap);
    return true;
}

struct Launch {
    Carve c;
    dim3 grid;
    size_t lds;
};

bool make_launch(int cap, int n_prob, int fill, Launch& L) {
    if (cap < 2 || n_prob < 1 || fill < 0 || fill > 255) return false;
    cap = (cap + 1) & ~1;  // the BucketWork behind the values stays 16-byte aligned
    const size_t per_wave = (size_t)(cap + kWorkDoubles) * sizeof(double);
    const int active = per_wave * 4 <= kLdsMax ? 4 : (int)(kLdsMax / per_wave);
    if (active < 1) return false;
    L.c = Carve{cap, active, n_prob, 0x0101010101010101ull * (unsigned long long)fill};
    L.grid = dim3((n_prob + active - 1) / active);
    L.lds = per_wave * active;
    return true;
}

template <class K>
void raise_lds(K kernel, size_t bytes, devunit::Bufs& B) {
    if (bytes > 48 * 1024) B.chk(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

int next_pow2(int n) {
    int L = 1;
    while (L < n) L <<= 1;
    return L;
}
int max_len(const int* off, int n_prob) {
    int m = 0;
    for (int p = 0; p < n_prob; ++p) {
        if (off[p + 1] < off[p]) return -1;
        m = off[p + 1] - off[p] > m ? off[p + 1] - off[p] : m;
    }
    return m;
}

// ---------------------------------------------------------------------------------------------- LdsSorter
__global__ __launch_bounds__(256) void k_sort(Carve c, int merge, const double* __restrict__ v,
                                              const int* __restrict__ off, double* __restrict__ out) {
    double* buf; BucketWork* W; int p;
    if (!carve(c, buf, W, p)) return;
    const int b = off[p], n = off[p + 1] - b;
    for (int k = Wv::lane(); k < n; k += 64) buf[k] = v[b + k];
    LdsSorter sorter;
    if (merge == 2) {  // robust_disp_gene's sequence: sort, squared errors around a value inside the row, merge
        sorter(buf, n);
        const double tm = buf[n / 3];
        Wv::sync();
        for (int k = Wv::lane(); k < n; k += 64) {
            const double d = buf[k] - tm;
            buf[k] = d * d;
        }
        sorter.merge(buf, n);
    } else if (merge) {  // (what the preceding sort leaves behind the row: NaN up to the power of two)
        int L = 1;
        while (L < n) L <<= 1;
        for (int k = n + Wv::lane(); k < L; k += 64) buf[k] = NAN;
        sorter.merge(buf, n);
    } else {
        sorter(buf, n);
    }
    for (int k = Wv::lane(); k < n; k += 64) out[b + k] = buf[k];
}

// ---------------------------------------------------------------------------------------------- trimmed_sum_select
__global__ __launch_bounds__(256) void k_select(Carve c, const double* __restrict__ v, const int* __restrict__ off,
                                                const int* __restrict__ nt, double* __restrict__ out) {
    double* buf; BucketWork* W; int p;
    if (!carve(c, buf, W, p)) return;
    const int b = off[p], n = off[p + 1] - b;
    for (int k = Wv::lane(); k < n; k += 64) buf[k] = v[b + k];
    Wv::sync();
    const double s = trimmed_sum_select<Wv>(buf, n, nt[p], (unsigned int*)W);
    if (Wv::lane() == 0) out[p] = s;
}

// ---------------------------------------------------------------------------------------------- rank sums
// ip[4 p ..]: n_act, j_lo, j_hi, mode.  mode bit 0: select_rank_sum (else bucket_rank_sum), bit 1: pass `range`,
// bit 2: over a NormedValues accessor (else the LDS buffer), bit 3: squared errors around tm[p], bit 4: through idx.
// `range` is found on the device as the product finds it (one pass over the same accessor): the buckets are indexed
// relative to it.
struct RankIn {
    const double* v;     // buffer mode: the rows
    const int32_t* y;    // accessor mode: counts and size factors of the row's samples (same offsets)
    const double* sf;
    const int32_t* idx;  // the row's index list (same offsets; entries < n)
    const double* tm;
    const int* off;
    const int* ip;
};

template <class Buf>
__device__ __forceinline__ void rank_sum(const Buf& B, int n, const int* q, BucketWork& W, double& res, int& ok) {
    const int n_act = q[0], j_lo = q[1], j_hi = q[2], mode = q[3];
    double range[2] = {0.0, 0.0};
    if (mode & 3) {
        double lo = INFINITY, hi = -INFINITY;
        for_each_batched<Wv>(B, n, [&](double x) {
            if (x >= 0.0) {
                lo = x < lo ? x : lo;
                hi = x > hi ? x : hi;
            }
        });
        range[0] = -Wv::max(-lo);
        range[1] = Wv::max(hi);
    }
    ok = 1;
    if (mode & 1) res = select_rank_sum<Wv>(B, n, n_act, j_lo, j_hi, (unsigned int*)W.sum, range);
    else ok = bucket_rank_sum<Wv>(B, n, n_act, j_lo, j_hi, W, res, (mode & 2) ? range : nullptr) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_rank(Carve c, RankIn in, double* __restrict__ out, int* __restrict__ accepted) {
    double* buf; BucketWork* W; int p;
    if (!carve(c, buf, W, p)) return;
    const int b = in.off[p], n = in.off[p + 1] - b;
    const int* q = in.ip + 4 * p;
    double res = 0.0;
    int ok = 0;
    if (q[3] & 4) {
        const NormedValues V{in.y + b, in.sf + b, (q[3] & 16) ? in.idx + b : nullptr, in.tm[p], (q[3] & 8) != 0};
        rank_sum(V, n, q, *W, res, ok);
    } else {
        for (int k = Wv::lane(); k < n; k += 64) buf[k] = in.v[b + k];
        Wv::sync();
        rank_sum(buf, n, q, *W, res, ok);
    }
    if (Wv::lane() == 0) {
        out[p] = res;
        accepted[p] = ok;
    }
}

// ---------------------------------------------------------------------------------------------- batched cells
// problem p = (gene p / nb, batch p % nb): one seg_trimmed_variances pass from vmax = -inf; lane q's result is the
// trimmed variance of cell c0 + q
__global__ __launch_bounds__(256) void k_seg(Carve c, const int32_t* __restrict__ y, int N, const double* __restrict__ sf,
                                             const int32_t* __restrict__ cell_offsets,
                                             const int32_t* __restrict__ cell_index, int n_cells, int L, int nb,
                                             double* __restrict__ out) {
    double* buf; BucketWork* W; int p;
    if (!carve(c, buf, W, p)) return;
    const CellPlan C{cell_offsets, cell_index, n_cells, 0};
    const int g = p / nb, c0 = (p % nb) * (kSegBatch / L);
    out[(size_t)p * 64 + Wv::lane()] =
        seg_trimmed_variances<Wv>(y + (size_t)g * N, sf, C, c0, L, buf, buf + kSegBatch, -INFINITY);
}

// ---------------------------------------------------------------------------------------------- CooksAcc
// one gene per wavefront; iout[6 g ..]: any_gt_all, any_gt_use, any_gt_use_nr, few_above, winning index, its count
__global__ __launch_bounds__(256) void k_cooks_acc(Carve c, int counted, const int32_t* __restrict__ y,
                                                   const double* __restrict__ mu, const double* __restrict__ hat,
                                                   const uint8_t* __restrict__ flags, int N, int P,
                                                   const double* __restrict__ ar, double cutoff,
                                                   double* __restrict__ ck, int* __restrict__ iout) {
    double* buf; BucketWork* W; int p;
    if (!carve(c, buf, W, p)) return;
    const int32_t* yr = y + (size_t)p * N;
    CooksAcc<Wv> acc(ar[p], cutoff, P);
    for (int n = Wv::lane(); n < N; n += 64)
        ck[(size_t)p * N + n] = acc.add(n, (double)yr[n], mu[(size_t)p * N + n], hat[(size_t)p * N + n], flags[n]);
    CooksAcc<Wv> probe = acc;  // reduce() alone: the winner's index and count
    CooksOut o0;
    int bi;
    double yref;
    probe.reduce(o0, bi, yref);
    const CooksOut o = counted ? acc.finish_counted(N, [&](int ref) {
        int above = 0;
        for (int n = Wv::lane(); n < N; n += 64) above += yr[n] > ref ? 1 : 0;
        return above;
    }) : acc.finish(yr, N);
    if (Wv::lane() == 0) {
        int* io = iout + 6 * p;
        io[0] = o.any_gt_all; io[1] = o.any_gt_use; io[2] = o.any_gt_use_nr; io[3] = o.few_above;
        io[4] = bi; io[5] = (int)yref;
    }
}

extern "C" {  // (C linkage holds inside the namespace)

// mode 0: LdsSorter::operator(), 1: ::merge on a row as the sort leaves it, 2: sort, (v - v[n/3])^2, merge
static int lds_sort_impl(int merge, const double* v, const int* off, int n_prob, int fill, double* out) {
    if (v == nullptr || off == nullptr || out == nullptr || n_prob < 1) return hipErrorInvalidValue;
    const int m = max_len(off, n_prob);
    Launch L;
    if (m < 1 || !make_launch(next_pow2(m < 2 ? 2 : m), n_prob, fill, L)) return hipErrorInvalidValue;
    devunit::Bufs B;
    const size_t tot = (size_t)off[n_prob];
    const double* d_v = B.put(v, tot);
    const int* d_off = B.put(off, (size_t)n_prob + 1);
    double* d_out = B.put(out, tot);
    raise_lds(k_sort, L.lds, B);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_sort, L.grid, dim3(256), L.lds, 0, L.c, merge, d_v, d_off, d_out);
    B.done();
    B.get(out, d_out, tot);
    return (int)B.e;
}

int du_lds_sort(const double* v, const int* off, int n_prob, int fill, double* out) {
    return lds_sort_impl(0, v, off, n_prob, fill, out);
}
int du_lds_merge(const double* v, const int* off, int n_prob, int fill, double* out) {
    return lds_sort_impl(1, v, off, n_prob, fill, out);
}
int du_lds_sort_merge(const double* v, const int* off, int n_prob, int fill, double* out) {
    return lds_sort_impl(2, v, off, n_prob, fill, out);
}

int du_trimmed_select(const double* v, const int* off, const int* nt, int n_prob, int fill, double* out) {
    if (v == nullptr || off == nullptr || nt == nullptr || out == nullptr || n_prob < 1) return hipErrorInvalidValue;
    const int m = max_len(off, n_prob);
    for (int p = 0; p < n_prob; ++p)
        if (nt[p] < 0 || off[p + 1] - off[p] - 2 * nt[p] < 1) return hipErrorInvalidValue;
    Launch L;
    if (m < 1 || !make_launch((m + 15) & ~15, n_prob, fill, L)) return hipErrorInvalidValue;
    devunit::Bufs B;
    const double* d_v = B.put(v, (size_t)off[n_prob]);
    const int* d_off = B.put(off, (size_t)n_prob + 1);
    const int* d_nt = B.put(nt, (size_t)n_prob);
    double* d_out = B.put(out, (size_t)n_prob);
    raise_lds(k_select, L.lds, B);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_select, L.grid, dim3(256), L.lds, 0, L.c, d_v, d_off, d_nt, d_out);
    B.done();
    B.get(out, d_out, (size_t)n_prob);
    return (int)B.e;
}

// v: buffer-mode rows; y / sf / idx: accessor-mode rows (all with the offsets `off`; whichever a problem does not use
// may hold anything, and a pointer no problem uses may be null).  ip: 4 ints per problem, see RankIn.
static int rank_sum_impl(const double* v, const int32_t* y, const double* sf, const int32_t* idx, const double* tm, const int* off,
                const int* ip, int n_prob, int fill, double* out, int* accepted) {
    if (off == nullptr || ip == nullptr || tm == nullptr || out == nullptr || accepted == nullptr || n_prob < 1)
        return hipErrorInvalidValue;
    const int m = max_len(off, n_prob);
    for (int p = 0; p < n_prob; ++p) {
        const int n = off[p + 1] - off[p], mode = ip[4 * p + 3];
        const int n_act = ip[4 * p], j_lo = ip[4 * p + 1], j_hi = ip[4 * p + 2];
        if (n_act < 0 || n_act > n || j_lo < 0 || j_hi >= n_act + (n_act == 0) || j_hi < j_lo - 1) return hipErrorInvalidValue;
        if ((mode & 4) ? (y == nullptr || sf == nullptr || ((mode & 16) && idx == nullptr)) : v == nullptr)
            return hipErrorInvalidValue;
        if ((mode & 16) && idx != nullptr)
            for (int k = 0; k < n; ++k)
                if (idx[off[p] + k] < 0 || idx[off[p] + k] >= n) return hipErrorInvalidValue;
    }
    Launch L;
    if (m < 1 || !make_launch((m + 15) & ~15, n_prob, fill, L)) return hipErrorInvalidValue;
    devunit::Bufs B;
    const size_t tot = (size_t)off[n_prob];
    RankIn in;
    in.v = B.put(v, tot);
    in.y = B.put(y, tot);
    in.sf = B.put(sf, tot);
    in.idx = B.put(idx, tot);
    in.tm = B.put(tm, (size_t)n_prob);
    in.off = B.put(off, (size_t)n_prob + 1);
    in.ip = B.put(ip, (size_t)4 * n_prob);
    double* d_out = B.put(out, (size_t)n_prob);
    int* d_acc = B.put(accepted, (size_t)n_prob);
    raise_lds(k_rank, L.lds, B);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_rank, L.grid, dim3(256), L.lds, 0, L.c, in, d_out, d_acc);
    B.done();
    B.get(out, d_out, (size_t)n_prob);
    B.get(accepted, d_acc, (size_t)n_prob);
    return (int)B.e;
}

// (mode bit 0 of every problem must name the routine)
int du_bucket_rank_sum(const double* v, const int32_t* y, const double* sf, const int32_t* idx, const double* tm,
                       const int* off, const int* ip, int n_prob, int fill, double* out, int* accepted) {
    for (int p = 0; ip != nullptr && p < n_prob; ++p)
        if (ip[4 * p + 3] & 1) return hipErrorInvalidValue;
    return rank_sum_impl(v, y, sf, idx, tm, off, ip, n_prob, fill, out, accepted);
}
int du_select_rank_sum(const double* v, const int32_t* y, const double* sf, const int32_t* idx, const double* tm,
                       const int* off, const int* ip, int n_prob, int fill, double* out, int* accepted) {
    for (int p = 0; ip != nullptr && p < n_prob; ++p)
        if (!(ip[4 * p + 3] & 1)) return hipErrorInvalidValue;
    return rank_sum_impl(v, y, sf, idx, tm, off, ip, n_prob, fill, out, accepted);
}

// y: [G][N]; cells as a CellPlan (offsets [n_cells + 1], index [offsets[n_cells]]); out: [G][nb][64], nb = the number
// of passes of kSegBatch / L cells that cover n_cells
int du_seg_variances(const int32_t* y, const double* sf, const int32_t* cell_offsets, const int32_t* cell_index,
                     int n_cells, int N, int G, int L, int fill, double* out) {
    if (y == nullptr || sf == nullptr || cell_offsets == nullptr || cell_index == nullptr || out == nullptr) return hipErrorInvalidValue;
    if (N < 1 || G < 1 || n_cells < 1 || L < 2 || L > kSegMaxCell || (L & (L - 1))) return hipErrorInvalidValue;
    for (int c = 0; c < n_cells; ++c) {
        const int n = cell_offsets[c + 1] - cell_offsets[c];
        if (n < 1 || n > L) return hipErrorInvalidValue;
    }
    for (int k = 0; k < cell_offsets[n_cells]; ++k)
        if (cell_index[k] < 0 || cell_index[k] >= N) return hipErrorInvalidValue;
    const int per = kSegBatch / L, nb = (n_cells + per - 1) / per;
    Launch Lc;
    if (!make_launch(kSegBatch + kSegBatch / 2, G * nb, fill, Lc)) return hipErrorInvalidValue;
    devunit::Bufs B;
    const int32_t* d_y = B.put(y, (size_t)G * N);
    const double* d_sf = B.put(sf, (size_t)N);
    const int32_t* d_co = B.put(cell_offsets, (size_t)n_cells + 1);
    const int32_t* d_ci = B.put(cell_index, (size_t)cell_offsets[n_cells]);
    double* d_out = B.put(out, (size_t)G * nb * 64);
    raise_lds(k_seg, Lc.lds, B);
    if (B.e == hipSuccess)
        hipLaunchKernelGGL(k_seg, Lc.grid, dim3(256), Lc.lds, 0, Lc.c, d_y, N, d_sf, d_co, d_ci, n_cells, L, nb, d_out);
    B.done();
    B.get(out, d_out, (size_t)G * nb * 64);
    return (int)B.e;
}

// y / mu / hat: [G][N], flags: [N], ar: [G]; ck: [G][N], iout: [G][6]
int du_cooks_acc(int counted, const int32_t* y, const double* mu, const double* hat, const uint8_t* flags, int N, int G,
                 int P, const double* ar, double cutoff, int fill, double* ck, int* iout) {
    if (y == nullptr || mu == nullptr || hat == nullptr || flags == nullptr || ar == nullptr || ck == nullptr || iout == nullptr)
        return hipErrorInvalidValue;
    if (N < 1 || G < 1 || P < 1) return hipErrorInvalidValue;
    Launch L;
    if (!make_launch(16, G, fill, L)) return hipErrorInvalidValue;
    devunit::Bufs B;
    const size_t tot = (size_t)G * N;
    const int32_t* d_y = B.put(y, tot);
    const double* d_mu = B.put(mu, tot);
    const double* d_hat = B.put(hat, tot);
    const uint8_t* d_fl = B.put(flags, (size_t)N);
    const double* d_ar = B.put(ar, (size_t)G);
    double* d_ck = B.put(ck, tot);
    int* d_io = B.put(iout, (size_t)6 * G);
    raise_lds(k_cooks_acc, L.lds, B);
    if (B.e == hipSuccess)
        hipLaunchKernelGGL(k_cooks_acc, L.grid, dim3(256), L.lds, 0, L.c, counted, d_y, d_mu, d_hat, d_fl, N, P, d_ar, cutoff,
                           d_ck, d_io);
    B.done();
    B.get(ck, d_ck, tot);
    B.get(iout, d_io, (size_t)6 * G);
    return (int)B.e;
}

}  // extern "C"

}  // namespace du_stats
