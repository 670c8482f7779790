// zsw_handback_split.hip — the one-thread kernel behind the seed kernel that freezes the co-scheduled part of the hand-back list:
// *n0 = the count the seed kernel left, and, where the call plans slices (zsw_handback.hpp: handback_slices), the bounds of the
// three parts. The rule is the header's, the text the host model tests; the launches behind read their ranges from these words.
#include <hip/hip_runtime.h>

#include "zsw_handback.hpp"
#include "zsw_score_seed.hpp"

namespace zsw {

namespace {

__global__ void handback_split_kernel(const uint32_t* count, uint32_t* n0, uint32_t* bounds, HandbackSliceRule rule) {
    const uint32_t n = *count;
    *n0 = n;
    if (bounds) {
        const HandbackSlices s = handback_slices(n, rule);
        bounds[0] = s.shared.end;
        bounds[1] = s.head.end;
    }
}

}  // namespace

hipError_t launch_handback_split(const uint32_t* count, uint32_t* n0, uint32_t* bounds, const HandbackSliceRule& rule, hipStream_t stream) {
    hipLaunchKernelGGL(handback_split_kernel, dim3(1), dim3(1), 0, stream, count, n0, bounds, rule);
    return hipGetLastError();
}

}  // namespace zsw
