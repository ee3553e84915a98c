// dsq_lds_sort.h — the bitonic sorter of a wavefront's private LDS segment (device only): what dsq_k_stats.hip hands to
// the trimmed statistics of dsq_stats.h as their `Sorter`.  A header of its own so that the device unit tests
// (tests/devunit) run this code and not a copy of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace dsq {

// ------------------------------------------------------------------ wave-private LDS sort
// Bitonic sort of n doubles (padded to L = next pow2 with NaN, which the comparison below puts last: a
// padding of +inf would sort in front of the row's own NaNs and push them out of buf[0..n)) held in a
// wave-private LDS segment; lanes stride over compare-exchange pairs.  Only this wave touches the segment,
// LDS operations of one wave execute in order, so a wave-level fence is sufficient.
struct LdsSorter {
    __device__ __forceinline__ static void wave_sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __device__ __forceinline__ int operator()(double* buf, int n) const {
        int L = 1;
        while (L < n) L <<= 1;
        const int lane = threadIdx.x & 63;
        for (int k = n + lane; k < L; k += 64) buf[k] = NAN;
        wave_sync();
        for (int k = 2; k <= L; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < (L >> 1); i += 64) {
                    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                    const int hi = lo | j;
                    const bool up = ((lo & k) == 0);
                    const double a = buf[lo], b = buf[hi];
                    // NaNs sort last (numpy.sort semantics)
                    const bool gt = (a > b) || (a != a && b == b);
                    if (gt == up) { buf[lo] = b; buf[hi] = a; }
                }
                wave_sync();
            }
        }
        return L;
    }
    // buf[0..n) bitonic (here: decreasing then increasing), buf[n..L) = NaN from the preceding sort:
    // the final merge phase of the network alone leaves it ascending
    __device__ __forceinline__ void merge(double* buf, int n) const {
        int L = 1;
        while (L < n) L <<= 1;
        const int lane = threadIdx.x & 63;
        wave_sync();
        for (int j = L >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < (L >> 1); i += 64) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const int hi = lo | j;
                const double a = buf[lo], b = buf[hi];
                const bool gt = (a > b) || (a != a && b == b);
                if (gt) { buf[lo] = b; buf[hi] = a; }
            }
            wave_sync();
        }
    }
};

}  // namespace dsq
