// bioinfo1_amd/csrc/tm_ends.hip -- the reversed-bytes gather of the mapper's
// end extension (--extend-ends, tm_api.cpp): the left end of a read is aligned
// backwards from its window, so its query and target bytes are written in
// reverse order into a staging buffer the anchored plan reads.
#include <hip/hip_runtime.h>

#include "tm_internal.h"
#include "tm_match.h"

namespace tmap {
namespace {

constexpr int kGatherBlock = 256;

// Segment s: dst[dst_off[s] + k] = src[src_end[s] - 1 - k], k < len[s].  One block per segment.
__global__ __launch_bounds__(kGatherBlock) void reverse_gather_kernel(uint32_t n, const uint8_t* __restrict__ src,
                                                                      const uint64_t* __restrict__ src_end,
                                                                      const uint32_t* __restrict__ len,
                                                                      const uint64_t* __restrict__ dst_off,
                                                                      uint8_t* __restrict__ dst) {
    const uint32_t s = blockIdx.x;
    if (s >= n) return;
    const uint32_t L = len[s];
    const uint8_t* from = src + src_end[s];
    uint8_t* to = dst + dst_off[s];
    for (uint32_t k = threadIdx.x; k < L; k += kGatherBlock) to[k] = from[-(int64_t)k - 1];
}

}  // namespace

int reverse_gather(tm_context* ctx, uint32_t n, const uint8_t* d_src, const uint64_t* d_src_end, const uint32_t* d_len,
                   const uint64_t* d_dst_off, uint8_t* d_dst) {
    if (!n) return TM_OK;
    hipLaunchKernelGGL(reverse_gather_kernel, dim3(n), dim3(kGatherBlock), 0, ctx->stream, n, d_src, d_src_end, d_len,
                       d_dst_off, d_dst);
    TM_HIP(ctx, hipGetLastError());
    return TM_OK;
}

}  // namespace tmap
