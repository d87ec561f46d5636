// TEST INFRASTRUCTURE ONLY: libmems_amd/csrc/anchor_lane.h compiled for the host, so the lane's
// sort, walk and filter (what anchor.hip runs per problem) are held to tests/eo2_model.cpp and
// oracle.std_sort_ids without a device.
#include <cstdint>
#include <vector>

#include "../libmems_amd/csrc/anchor_lane.h"

// the tail of one list; out arrays hold at least n rows; returns the surviving rows
extern "C" uint64_t lane_anchor_tail(int G, uint64_t n, const uint64_t* len, const int64_t* s, int eliminate_both,
                                     uint64_t min_length, uint64_t* len_out, int64_t* s_out) {
    std::vector<uint64_t> K(n + 1);
    std::vector<uint32_t> V(n + 1);
    std::vector<int64_t> plen(len, len + n), ps(s, s + n * (uint64_t)G);
    plen.push_back(0);
    ps.push_back(0);
    const uint32_t kept = mums::lane::anchor_tail(K.data(), V.data(), plen.data(), ps.data(), (uint32_t)n, G,
                                                  eliminate_both, min_length);
    for (uint32_t k = 0; k < kept; ++k) {
        len_out[k] = (uint64_t)plen[V[k]];
        for (int g = 0; g < G; ++g) s_out[(uint64_t)k * G + g] = ps[(uint64_t)V[k] * G + g];
    }
    return kept;
}

// ids[0, n) = the std::sort order of 0 .. n-1 by keys (depth < 0: the library's limit)
extern "C" void lane_std_sort_ids(const uint64_t* keys, uint64_t n, int depth, uint32_t* ids) {
    std::vector<uint64_t> K(keys, keys + n);
    for (uint64_t i = 0; i < n; ++i) ids[i] = (uint32_t)i;
    K.push_back(0);
    mums::lane::std_sort_kv(K.data(), ids, (uint32_t)n, depth);
}
