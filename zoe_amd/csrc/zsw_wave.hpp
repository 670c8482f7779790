// zsw_wave.hpp — what the one-wavefront-per-item kernels share (zsw_annotate.hip, zsw_sam.hip, zsw_pileup.hip, zsw_fastq.hip,
// zsw_samtext.hip, zsw_text.hip): scalar copies of wavefront-uniform values, the wavefront's LDS hand-over, the prefix sum across
// its lanes, a byte copy by its lanes, the 16-byte vector the text kernels load and store through. Device code only.
#pragma once
#include <stdint.h>

namespace zsw {
namespace wave {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((may_alias)) u32x4_alias;

// A value every lane of the wavefront holds, moved to a scalar register. Records, ciglets, offsets and newline positions are loaded
// from wavefront-uniform addresses, but by vector loads (the kernels write memory, so the compiler cannot prove them invariant), and
// a walk on vector registers pays a mask and a vector instruction for every scalar step and branch of its cursors.
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) { return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32); }

// within a wavefront: what its lanes stored to LDS is there for every lane's loads behind this point
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum of x over lanes 0 .. lane
__device__ __forceinline__ uint32_t lane_prefix_sum(uint32_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint64_t n, int lane) {
    for (uint64_t j = (uint32_t)lane; j < n; j += 64) dst[j] = src[j];
}

}  // namespace wave
}  // namespace zsw
