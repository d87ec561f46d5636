// recursion.hip -- the tail of Aligner::Recursion (Aligner.cpp:1211-1218) for the B lists of a batch
// in one pass (mums_recursion_batch / mums_recursion_tail_batch): EliminateOverlaps
// (v1), MultiplicityFilter, LengthFilter.
//
// anchor.hip's shape: one lane per problem, the reference replayed literally (recursion_lane.h).
// v1 appends the cut-off overlap of a pair as a new match, so a list grows: problem p owns the
// slice [soff[p], soff[p + 1]) of the work arrays, its input in the first nrow[p] rows.
//   gather  anchor.hip's: a lane problem's table becomes the first rows of its slice
//   tail    one lane per problem; cnt[p] = surviving rows, their ids in V's slice in list order;
//           flag[p] = 1 and cnt[p] = 0 when a copy did not fit the slice (the caller runs p alone)
//   emit    anchor.hip's: one workgroup per problem copies the surviving rows to its rows of the
//           MatchList (a slice's base is all it reads of the offsets)
#include <hip/hip_runtime.h>

#include "mums_internal.h"
#include "recursion_lane.h"

namespace mums {

namespace {

constexpr int kRecursionBlock = 64;   // tail: lanes (= problems) per workgroup

__global__ __launch_bounds__(kRecursionBlock) void recursion_tail_kernel(RecursionTail a) {
    const uint32_t t = blockIdx.x * kRecursionBlock + threadIdx.x;
    if (t >= a.B) return;
    const uint32_t p = a.order[t];
    a.flag[p] = 0;
    if (a.skip[p]) {   // the caller runs this list alone
        a.cnt[p] = 0;
        return;
    }
    const uint64_t d = a.soff[p];
    const uint64_t cap = a.soff[p + 1] - d;
    const uint32_t n = a.nrow[p];
    if (n > cap) {   // never planned so; nothing is touched
        a.cnt[p] = 0;
        a.flag[p] = 1;
        return;
    }
    lane::V1Counts c;
    const uint32_t kept = lane::recursion_tail(a.K + d, a.V + d, a.wlen + d, a.ws + d * a.G, n, (uint32_t)cap, (int)a.G,
                                               a.multiplicity, a.min_length, &c);
    a.cnt[p] = c.overflow ? 0 : kept;
    a.flag[p] = c.overflow ? 1 : 0;
}

}  // namespace

uint64_t recursion_slice_rows(uint64_t n, uint32_t G) { return lane::slice_rows((uint32_t)n, (int)G); }

hipError_t launch_recursion_tail(const RecursionTail& a, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    hipLaunchKernelGGL(recursion_tail_kernel, dim3((a.B + kRecursionBlock - 1) / kRecursionBlock), dim3(kRecursionBlock), 0,
                       st, a);
    return hipGetLastError();
}

}  // namespace mums
