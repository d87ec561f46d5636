// TEST INFRASTRUCTURE ONLY: libmems_amd/csrc/recursion_lane.h compiled for the host, so the lane's
// sort, v1 walk and filters (what recursion.hip runs per problem) are held to
// oracle.eliminate_overlaps and tests/eo_model.cpp without a device.  With RECURSION_LANE_MAIN the
// file is a stand-alone program over lists read from a file (the sanitizer run of
// test_recursion_batch_cpu.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../libmems_amd/csrc/recursion_lane.h"

extern "C" uint64_t lane_slice_rows(uint64_t n, int G) { return mums::lane::slice_rows((uint32_t)n, G); }

// The tail of one list in a slice of cap rows (cap < n: refused as an overflow).  out arrays hold at
// least cap rows; info[0..3] = deleted, appended, overflow.  Returns the surviving rows.  The work
// arrays are exactly cap rows long, so a sanitizer sees a write past the slice.
extern "C" uint64_t lane_recursion_tail(int G, uint64_t n, uint64_t cap, const uint64_t* len, const int64_t* s,
                                        uint32_t multiplicity, uint64_t min_length, uint64_t* len_out, int64_t* s_out,
                                        uint64_t* info) {
    info[0] = info[1] = 0;
    info[2] = 1;
    if (n > cap) return 0;
    std::vector<uint64_t> K(cap);
    std::vector<uint32_t> V(cap);
    std::vector<int64_t> plen(cap, 0), ps(cap * (uint64_t)G, 0);
    for (uint64_t i = 0; i < n; ++i) plen[i] = (int64_t)len[i];
    for (uint64_t i = 0; i < n * (uint64_t)G; ++i) ps[i] = s[i];
    mums::lane::V1Counts c;
    const uint32_t kept = mums::lane::recursion_tail(K.data(), V.data(), plen.data(), ps.data(), (uint32_t)n, (uint32_t)cap,
                                                     G, multiplicity, min_length, &c);
    info[0] = c.dels;
    info[1] = c.apps;
    info[2] = c.overflow ? 1 : 0;
    if (c.overflow) return 0;
    for (uint32_t k = 0; k < kept; ++k) {
        len_out[k] = (uint64_t)plen[V[k]];
        for (int g = 0; g < G; ++g) s_out[(uint64_t)k * G + g] = ps[(uint64_t)V[k] * G + g];
    }
    return kept;
}

#ifdef RECURSION_LANE_MAIN
// argv[1]: a file of u64 words: per list G, n, cap, multiplicity, min_length, n lengths, n * G
// starts.  Prints per list "kept appended overflow checksum".
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[5];
    while (fread(h, 8, 5, f) == 5) {
        const uint64_t G = h[0], n = h[1], cap = h[2];
        std::vector<uint64_t> len(n + 1), lo(cap + 1), info(3);
        std::vector<int64_t> s(n * G + 1), so(cap * G + 1);
        if (fread(len.data(), 8, n, f) != n || fread(s.data(), 8, n * G, f) != n * G) return 3;
        const uint64_t k = lane_recursion_tail((int)G, n, cap, len.data(), s.data(), (uint32_t)h[3], h[4], lo.data(),
                                               so.data(), info.data());
        uint64_t sum = 0;
        for (uint64_t i = 0; i < k; ++i) {
            sum = sum * 1000003u + lo[i];
            for (uint64_t g = 0; g < G; ++g) sum = sum * 1000003u + (uint64_t)so[i * G + g];
        }
        printf("%llu %llu %llu %llu\n", (unsigned long long)k, (unsigned long long)info[1], (unsigned long long)info[2],
               (unsigned long long)sum);
    }
    fclose(f);
    return 0;
}
#endif
