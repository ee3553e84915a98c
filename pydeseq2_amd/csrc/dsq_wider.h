// dsq_wider.h — designs of kWideMaxP + 1 = 49 ... kWiderMaxP = 128 columns.
//
// Five p x p matrices of a gene take 660 KB at p = 128: more than a CU's 160 KB of LDS.  This family runs the very
// templates of dsq_wide.h (same formulas, same optimisers, same per-entry operation order of the Cholesky / inverse /
// solves) over WiderWork = WideWorkT<128>, bound with bind_split:
//   * device memory, one slot per resident workgroup (SlotGeom, dsq_k_wide.hip): the Gram tile accumulators `gacc` and the five
//     p x p matrices M, dM, L, L^-1, inverse;
//   * LDS: the staged design chunk xs (rows x 65), the chunk's weights and the small vectors (8 x 128).
// The Gram matrices are still built by v_mfma_f64_16x16x4_f64 on 16 x 16 lower-triangle tiles (up to 36 per matrix),
// tile by tile: a lane's accumulator fragment goes to gacc after each 64-sample chunk and comes back for the next one
// (WideGram, MP > kWideMaxP), so every entry sums its samples in the same order as a register accumulator would.
// One gene per 64-lane workgroup; the matrices are read and written by other lanes of the same wavefront through
// device memory, so the wave policy's barrier (SlotWave::sync) is a workgroup-scope fence.
#pragma once
#include "dsq_wide.h"

namespace dsq {

constexpr int kWiderMaxP = 128;  // DSQ_MAX_P
using WiderWork = WideWorkT<kWiderMaxP>;

// doubles of LDS per gene (xs, w, vec, acc / tab), and of device memory per slot (gacc + five matrices, 32-byte
// multiples so that every slot's gacc stays aligned)
DSQ_HD int wider_lds_doubles(int P) {
    const int rows = ((P + 15) / 16) * 16;
    return rows * kWideXsLd + 2 * 64 + 8 * kWiderMaxP + 4 * kMaxCells;
}
DSQ_HD size_t wider_slot_doubles(int P) {
    const size_t d = (size_t)WiderWork::kGaccDoubles + 5 * (size_t)P * wide_ld(P);
    return (d + 3) & ~(size_t)3;
}

#if defined(__HIPCC__)
// DeviceWave whose barrier also orders device memory between the lanes (the slot's matrices)
struct SlotWave : DeviceWave {
    static __device__ __forceinline__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};
#endif

}  // namespace dsq
