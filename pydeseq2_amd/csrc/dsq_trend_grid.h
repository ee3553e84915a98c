// dsq_trend_grid.h — the trend fit's data passes on one or many workgroups (device only): the register genes, the
// mailbox between a workgroup's leader wave and its helper waves, and the workgroups' exchange of partial sums.
// dsq_k_trend.hip instantiates it with the optimiser (trend_fit_core, dsq_trend.h); the test library instantiates it
// with a driver that records the totals of single passes.
//
// The fit is a CHAIN of dependent data passes - one per L-BFGS-B evaluation (about 20 per gamma-GLM fit), one per
// outlier filter - over two doubles per gene: its duration is (number of passes) x (latency of a pass), nearly
// independent of the number of genes (r03: 0.39 ms at 7 500 genes, 0.47 ms at 60 000).  Everything here serves that
// latency:
//   - the genes live in REGISTERS: kTrendGridBlocks x 64 kTrendWaves threads hold kTrendRegGenes genes each (clipped
//     dispersion, 1 / mean, keep bit), loaded once by the first pass; a pass reads no memory (genes beyond that
//     capacity - more than 65 536 - go through the arrays, as before);
//   - one cross-lane butterfly per reduction level for the six sums of a pass (loss, two gradient sums and their three
//     NaN-free counts, carried as doubles): lanes -> wave, the waves of a workgroup (through LDS), the workgroups;
//   - EVERY workgroup's wave 0 runs the same deterministic optimiser on the same totals (bit-identical: fixed butterfly
//     order), so nothing is broadcast, and the workgroups exchange their partial sums through SELF-VALIDATING words:
//     every 64-bit word carries 32 bits of payload and the pass number.  A reader polls the words of all workgroups
//     until every tag is the current pass: one store and one (polled) load per pass and workgroup - no arrival counter,
//     no fence, no second round trip for the data (the arrival-counter barrier this replaces cost three dependent
//     memory round trips per pass).  Words are double-buffered by pass parity: a workgroup can be at most one pass
//     ahead of the slowest reader (it needs that reader's words of pass p to leave pass p).
// Launched cooperatively (all workgroups resident); a bounded poll sets a flag instead of hanging the GPU.
#pragma once
#include "dsq_trend.h"

namespace dsq {

#ifndef DSQ_TREND_WAVES
#define DSQ_TREND_WAVES 8
#endif
constexpr int kTrendWaves = DSQ_TREND_WAVES;
#ifndef DSQ_TREND_GRID_BLOCKS
#define DSQ_TREND_GRID_BLOCKS 32
#endif
constexpr int kTrendGridBlocks = DSQ_TREND_GRID_BLOCKS;  // <= 64: one lane of the leader wave per workgroup
constexpr int kTrendRegGenes = 4;
constexpr int kTrendWords = 12;  // six doubles, two tagged words each

struct TrendGridMem {  // device global memory, zeroed before every launch (pass numbers start at 1)
    unsigned int timeout;
    unsigned int pad[31];
    unsigned long long word[2][64][16];  // [pass parity][workgroup][word]
};

struct TrendShared {
    TrendWork W;
    double a0, a1;  // mailbox: leader wave -> helper waves of this workgroup
    int cmd;        // 1 eval, 2 filter, 3 load + initial mask, 0 done
    double part[kTrendWaves][6];
};

// loss / gradient terms of one gene (trend_eval_partial's arithmetic, dsq_trend.h)
__device__ __forceinline__ void trend_eval_one(double cov, double t, double a0, double a1, TrendPartial& P) {
    const double mu = a0 + a1 * cov;
    const double rmu = frcp(mu);
    const double tm = t * rmu;
    const double v = tm + flog(mu);
    if (v == v) { P.s.add(v); P.cf += 1; }
    const double r = tm - 1.0;
    const double v0 = r * rmu, v1 = (r * cov) * rmu;
    if (v0 == v0) { P.g0.add(v0); P.c0 += 1; }
    if (v1 == v1) { P.g1.add(v1); P.c1 += 1; }
}

struct GridTrendOps {
    TrendData D;
    TrendGridMem* Gm;
    TrendShared* S;  // LDS of this workgroup
    unsigned int seq = 0;
    // this thread's genes (i = tid + k * NT)
    double cov_e[kTrendRegGenes], cov_f[kTrendRegGenes], tg[kTrendRegGenes];
    unsigned int kbits = 0;
#ifdef DSQ_TREND_PHASES
    long long t_last = 0, c_opt = 0, c_pass = 0;
    int n_eval = 0;
#endif

    // every thread of every workgroup, once per pass: this thread's share -> wave sums -> LDS
    __device__ void work(int cmd, double a0, double a1) {
        const int w = threadIdx.x >> 6;
        const int tid = blockIdx.x * (64 * kTrendWaves) + threadIdx.x, NT = gridDim.x * 64 * kTrendWaves;
        double v[6];
        if (cmd == 1) {
            TrendPartial P;
#pragma unroll
            for (int k = 0; k < kTrendRegGenes; ++k)
                if (kbits & (1u << k)) trend_eval_one(cov_e[k], tg[k], a0, a1, P);
            trend_eval_partial(D, tid + kTrendRegGenes * NT, NT, a0, a1, P);
            v[0] = P.s.value(); v[1] = P.g0.value(); v[2] = P.g1.value();
            v[3] = (double)P.cf; v[4] = (double)P.c0; v[5] = (double)P.c1;
        } else {
            int kept = 0;
            if (cmd == 3) {
#pragma unroll
                for (int k = 0; k < kTrendRegGenes; ++k) {
                    const int i = tid + k * NT;
                    cov_e[k] = 0.0; cov_f[k] = 0.0; tg[k] = 0.0;
                    if (i < D.n) {
                        const double m = D.means[i], d = D.disp[i];
                        const double c = D.raw ? 0.0 : 1.0 / m;
                        const bool bad = (c != c) || (c == INFINITY) || (c == -INFINITY);  // dds.py:1225-1231
                        cov_e[k] = D.raw ? m : frcp(m);
                        cov_f[k] = c;
                        tg[k] = D.raw ? d : trend_clip(d, D.min_disp, D.max_disp);
                        if (!bad) { kbits |= 1u << k; kept += 1; }
                    }
                }
                kept += trend_init_keep(D, tid + kTrendRegGenes * NT, NT);
            } else {
#pragma unroll
                for (int k = 0; k < kTrendRegGenes; ++k)
                    if (kbits & (1u << k)) {
                        const double ratio = tg[k] / (a0 + a1 * cov_f[k]);
                        if (ratio < 1e-4 || ratio >= 15.0) kbits &= ~(1u << k);  // dds.py:1254-1264
                        else kept += 1;
                    }
                kept += trend_filter(D, tid + kTrendRegGenes * NT, NT, a0, a1);
            }
            v[0] = (double)kept; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0; v[4] = 0.0; v[5] = 0.0;
        }
        DeviceWave::sum_n<6>(v);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) S->part[w][q] = v[q];
        }
    }

    // leader wave: the workgroup's sums -> its words of this pass; poll everybody's; combine.  tot[] is identical in
    // every lane of every workgroup's leader wave.
    __device__ void exchange(double (&tot)[6]) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int q = 0; q < 6; ++q) tot[q] = (lane < kTrendWaves) ? S->part[lane][q] : 0.0;
        DeviceWave::sum_n<6>(tot);
        if (gridDim.x == 1) return;
        seq += 1;
        unsigned long long(*words)[16] = Gm->word[seq & 1];
        if (lane < kTrendWords) {
            double mine = tot[0];
#pragma unroll
            for (int q = 1; q < 6; ++q) mine = (lane >> 1) == q ? tot[q] : mine;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(mine);
            const unsigned long long half = (lane & 1) ? (bits >> 32) : (bits & 0xffffffffull);
            __hip_atomic_store(&words[blockIdx.x][lane], (half << 32) | seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool on = lane < (int)gridDim.x;
        unsigned long long wd[kTrendWords];
        unsigned int spins = 0;
        for (;;) {
            bool ok = true;
            if (on) {
#pragma unroll
                for (int j = 0; j < kTrendWords; ++j)
                    wd[j] = __hip_atomic_load(&words[lane][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int j = 0; j < kTrendWords; ++j) ok = ok && ((unsigned int)wd[j] == seq);
            }
            if (__all(ok)) break;
            if (++spins > 20000000u) {
                __hip_atomic_store(&Gm->timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const unsigned long long bits = (wd[2 * q] >> 32) | (wd[2 * q + 1] & 0xffffffff00000000ull);
            tot[q] = on ? __longlong_as_double((long long)bits) : 0.0;
        }
        DeviceWave::sum_n<6>(tot);
    }

    __device__ void pass(int cmd, double a0, double a1, double (&tot)[6]) {  // wave 0 of every workgroup
        if ((threadIdx.x & 63) == 0) { S->a0 = a0; S->a1 = a1; S->cmd = cmd; }
        __syncthreads();  // A: the mailbox is visible to the helper waves
        work(cmd, a0, a1);
        __syncthreads();  // B: the waves' sums are in LDS
        exchange(tot);
    }
    __device__ int init_keep() {
        double tot[6];
        pass(3, 0.0, 0.0, tot);
        return (int)tot[0];
    }
    __device__ void eval(double a0, double a1, double& f, double* g) {
#ifdef DSQ_TREND_PHASES
        const long long t0 = clock64();
        if (t_last) c_opt += t0 - t_last;
#endif
        double tot[6];
        pass(1, a0, a1, tot);
        f = fdiv(tot[0], tot[3]);
        g[0] = -fdiv(tot[1], tot[4]);
        g[1] = -fdiv(tot[2], tot[5]);
#ifdef DSQ_TREND_PHASES
        t_last = clock64();
        c_pass += t_last - t0;
        n_eval += 1;
#endif
    }
    __device__ int filter(double a0, double a1) {
        double tot[6];
        pass(2, a0, a1, tot);
        return (int)tot[0];
    }
};

// The body of a trend kernel (64 * kTrendWaves threads per workgroup, S in the workgroup's LDS): the leader wave of
// every workgroup runs drive(ops) - the same sequence of ops.init_keep / eval / filter calls in every workgroup, and
// nothing else that waits on another wave or workgroup -, the helper waves serve its passes until it has returned.
template <class Driver>
__device__ __forceinline__ void trend_grid_run(const TrendData& D, TrendGridMem* Gm, TrendShared& S, Driver&& drive) {
    GridTrendOps ops;
    ops.D = D;
    ops.Gm = Gm;
    ops.S = &S;
    if ((threadIdx.x >> 6) == 0) {  // the leader wave of every workgroup runs the optimiser
        drive(ops);
        if (threadIdx.x == 0) S.cmd = 0;
        __syncthreads();  // release this workgroup's helper waves
    } else {
        for (;;) {
            __syncthreads();  // A: wait for the leader's next command
            const int cmd = S.cmd;
            if (cmd == 0) break;
            ops.work(cmd, S.a0, S.a1);
            __syncthreads();  // B
        }
    }
}

}  // namespace dsq
