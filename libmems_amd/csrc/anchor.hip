// anchor.hip -- the tail of ProgressiveAligner::pairwiseAnchorSearch (ProgressiveAligner.cpp:655-659)
// for the B lists of a batch in one pass (mums_anchor_batch / mums_anchor_tail_batch):
// EliminateOverlaps_v2(list, eliminate_both) over every sequence, then LengthFilter(min_length).
//
// The lists are a few tens of entries, so the batch keeps batch.hip's shape: one lane per problem,
// the reference replayed literally (anchor_lane.h: libstdc++'s std::sort on ids, the matchI / nextI
// walk, the filter) in the problem's slice [toff[p], toff[p + 1]) of global work arrays.
//   gather  a lane problem's table, bucket-major (batch.hip's ord / pool), becomes its slice's rows
//   tail    one lane per problem; cnt[p] = surviving rows, their ids in V's slice in list order
//   emit    one workgroup per problem copies the surviving rows to its rows of the MatchList
#include <hip/hip_runtime.h>

#include "anchor_lane.h"
#include "mums_internal.h"

namespace mums {

namespace {

constexpr int kAnchorBlock = 64;   // tail: lanes (= problems) per workgroup

// rows [toff[p], toff[p + 1]) of wlen / ws = problem p's table in GetMatchList order (ord slice at
// obase[p]); with nrow the table has nrow[p] rows (recursion.hip: a slice wider than its input)
__global__ void anchor_gather_kernel(const uint64_t* __restrict__ ord, const uint32_t* __restrict__ obase,
                                     const int64_t* __restrict__ pool, const uint64_t* __restrict__ toff, uint32_t G,
                                     int64_t* __restrict__ wlen, int64_t* __restrict__ ws,
                                     const uint32_t* __restrict__ nrow) {
    const uint32_t p = blockIdx.x;
    const uint64_t d = toff[p];
    const uint32_t n = nrow ? nrow[p] : (uint32_t)(toff[p + 1] - d);
    const uint64_t* o = ord + obase[p];
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        const int64_t* row = pool + (uint64_t)(uint32_t)o[k] * (uint64_t)(G + 2);
        wlen[d + k] = row[0];
        for (uint32_t g = 0; g < G; ++g) ws[(d + k) * G + g] = row[2 + g];
    }
}

__global__ __launch_bounds__(kAnchorBlock) void anchor_tail_kernel(AnchorTail a) {
    const uint32_t t = blockIdx.x * kAnchorBlock + threadIdx.x;
    if (t >= a.B) return;
    const uint32_t p = a.order[t];
    if (a.skip[p]) {   // the caller runs this list alone
        a.cnt[p] = 0;
        return;
    }
    const uint64_t d = a.toff[p];
    const uint32_t n = (uint32_t)(a.toff[p + 1] - d);
    a.cnt[p] = lane::anchor_tail(a.K + d, a.V + d, a.wlen + d, a.ws + d * a.G, n, (int)a.G, a.eliminate_both,
                                 a.min_length);
}

// rows [doff[p], doff[p] + cnt[p]) of the MatchList = the rows V names, in V's order
__global__ void anchor_emit_kernel(const uint32_t* __restrict__ V, const int64_t* __restrict__ wlen,
                                   const int64_t* __restrict__ ws, const uint64_t* __restrict__ toff,
                                   const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ doff, uint32_t G,
                                   uint64_t* __restrict__ out_len, int64_t* __restrict__ out_s) {
    const uint32_t p = blockIdx.x;
    const uint32_t n = cnt[p];
    const uint64_t b = toff[p], d = doff[p];
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        const uint64_t r = b + V[b + k];
        out_len[d + k] = (uint64_t)wlen[r];
        for (uint32_t g = 0; g < G; ++g) out_s[(d + k) * G + g] = ws[r * G + g];
    }
}

}  // namespace

hipError_t launch_anchor_gather(const uint64_t* ord, const uint32_t* obase, const int64_t* pool, const uint64_t* toff,
                                uint32_t B, uint32_t G, int64_t* wlen, int64_t* ws, hipStream_t st,
                                const uint32_t* nrow) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(anchor_gather_kernel, dim3(B), dim3(64), 0, st, ord, obase, pool, toff, G, wlen, ws, nrow);
    return hipGetLastError();
}

hipError_t launch_anchor_tail(const AnchorTail& a, hipStream_t st) {
    if (a.B == 0) return hipSuccess;
    hipLaunchKernelGGL(anchor_tail_kernel, dim3((a.B + kAnchorBlock - 1) / kAnchorBlock), dim3(kAnchorBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_anchor_emit(const uint32_t* V, const int64_t* wlen, const int64_t* ws, const uint64_t* toff,
                              const uint32_t* cnt, const uint64_t* doff, uint32_t B, uint32_t G, uint64_t* out_len,
                              int64_t* out_s, hipStream_t st) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(anchor_emit_kernel, dim3(B), dim3(64), 0, st, V, wlen, ws, toff, cnt, doff, G, out_len, out_s);
    return hipGetLastError();
}

}  // namespace mums
