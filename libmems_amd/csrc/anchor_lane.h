// anchor_lane.h -- the sequential pieces of pairwiseAnchorSearch's tail (ProgressiveAligner.cpp:655-659)
// as one lane runs them: libstdc++'s std::sort on (key, id) pairs, EliminateOverlaps_v2's matchI /
// nextI walk (ProgressiveAligner.h:319-382) and LengthFilter (MatchList.h:652-664).
//
// overlaps.hip replays one cluster of a large list per lane with the walk below; anchor.hip replays a
// whole small list per lane (sort, walk and filter), one list per problem of a batch.  Everything is
// plain C++ on caller-owned arrays, so tests/anchor_lane_shim.cpp compiles this header for the host
// and holds it to tests/eo2_model.cpp (the toolchain's real std::sort) without a device.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MUMS_HD __host__ __device__ inline __attribute__((always_inline))
#define MUMS_HD_FN __host__ __device__ inline
#else
#define MUMS_HD inline
#define MUMS_HD_FN inline
#endif

namespace mums {
namespace lane {

constexpr uint32_t kDeleted = 0xFFFFFFFFu;   // a deleted match's slot in the id array
constexpr uint32_t kSortLeaf = 16;           // libstdc++ _S_threshold
constexpr int kSortStack = 64;               // segments waiting: one per level, depth limit 2 * lg n < 64

MUMS_HD int mult_of(const int64_t* s, int G) {
    int m = 0;
    for (int g = 0; g < G; ++g) m += s[g] != 0;
    return m;
}
MUMS_HD void crop_start(int64_t* len, int64_t* s, int G, int64_t a) {   // UngappedLocalAlignment.h:138
    *len -= a;
    for (int g = 0; g < G; ++g)
        if (s[g] > 0) s[g] += a;
}
MUMS_HD void crop_end(int64_t* len, int64_t* s, int G, int64_t a) {     // :147
    *len -= a;
    for (int g = 0; g < G; ++g)
        if (s[g] < 0) s[g] -= a;
}

// checkConsistent (ProgressiveAligner.h:272-291): the same b->Start - a->Start in every
// sequence where both are defined, and more than one such sequence
MUMS_HD bool check_consistent(const int64_t* a, const int64_t* b, int G) {
    bool consistent = true, have = false;
    int64_t o = 0;
    int inter = 0;
    for (int g = 0; g < G; ++g) {
        if (a[g] == 0 || b[g] == 0) continue;
        ++inter;
        if (!have) {
            o = b[g] - a[g];
            have = true;
        }
        if (o != b[g] - a[g]) consistent = false;
    }
    return consistent && inter > 1;
}

// EliminateOverlaps_v2's matchI / nextI loops (ProgressiveAligner.h:319-382) over V[a, b): ids of
// matches (lengths plen[id], starts ps[id * G ..]) that are all defined in seqI, sorted by
// SingleStartComparator(seqI).  Length(seqI) (UngappedLocalAlignment.h:48-55) is m_length for them.
// CropRight / CropLeft(diff, seqI) (:169-184) take the orientation of seqI.  processNewMatch
// (:260-271) sets Start(seqI) to NO_MATCH and then asks for Length(seqI) > 0, which is 0 for a
// Match: the cut-off copy is never kept, so none is made.  A deleted match's slot becomes kDeleted;
// returns the number of deleted matches.
MUMS_HD_FN uint64_t v2_walk(uint32_t* V, int64_t* plen, int64_t* ps, int G, int seqI, int64_t a, int64_t b,
                                  int eliminate_both) {
    uint64_t dels = 0;
    for (int64_t mi = a; mi < b; mi++) {
        if (V[mi] == kDeleted) continue;
        for (int64_t nj = mi + 1; nj < b; nj++) {
            if (V[nj] == kDeleted) continue;
            bool deleted_i = false;
            const uint64_t I = V[mi], J = V[nj];
            int64_t* sI = ps + I * G;
            int64_t* sJ = ps + J * G;
            const int64_t startI = sI[seqI], lenI = plen[I], startJ = sJ[seqI];
            int64_t diff = (startJ < 0 ? -startJ : startJ) - (startI < 0 ? -startI : startI) - lenI;
            if (diff >= 0) break;   // there are no more overlaps
            diff = -diff;
            // both decided before any crop of the pair
            const int mJ = mult_of(sJ, G), mI = mult_of(sI, G);
            const bool i_smaller = mJ > mI || (mJ == mI && plen[J] > lenI);
            const bool both = eliminate_both && !check_consistent(sI, sJ, G);
            if (both || i_smaller) {   // :345
                if (diff >= lenI) {
                    V[mi] = kDeleted;
                    deleted_i = true;
                    ++dels;
                } else if (startI > 0) {
                    crop_end(&plen[I], sI, G, diff);     // CropRight, forward
                } else {
                    crop_start(&plen[I], sI, G, diff);   // CropRight, reverse
                }
            }
            if (both || !i_smaller) {   // :363 (runs on nextI also after matchI was deleted)
                if (diff >= plen[J]) {
                    V[nj] = kDeleted;
                    ++dels;
                } else if (startJ > 0) {
                    crop_start(&plen[J], sJ, G, diff);   // CropLeft, forward
                } else {
                    crop_end(&plen[J], sJ, G, diff);     // CropLeft, reverse
                }
            }
            if (deleted_i) break;
        }
    }
    return dels;
}

MUMS_HD void swap_kv(uint64_t* K, uint32_t* V, uint32_t a, uint32_t b) {
    const uint64_t k = K[a];
    K[a] = K[b];
    K[b] = k;
    const uint32_t v = V[a];
    V[a] = V[b];
    V[b] = v;
}

// stl_heap.h __adjust_heap + __push_heap on (K, V)[0, len)
MUMS_HD void adjust_heap(uint64_t* K, uint32_t* V, int64_t hole, int64_t len, uint64_t vk, uint32_t vv) {
    const int64_t top = hole;
    int64_t child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (K[child] < K[child - 1]) child--;
        K[hole] = K[child];
        V[hole] = V[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        K[hole] = K[child - 1];
        V[hole] = V[child - 1];
        hole = child - 1;
    }
    int64_t parent = (hole - 1) / 2;
    while (hole > top && K[parent] < vk) {
        K[hole] = K[parent];
        V[hole] = V[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    K[hole] = vk;
    V[hole] = vv;
}

// std::__partial_sort(first, last, last) of (K, V)[0, len), len >= 2: make_heap, then __pop_heap
// from the back
MUMS_HD void heap_sort(uint64_t* K, uint32_t* V, int64_t len) {
    for (int64_t parent = (len - 2) / 2;; --parent) {
        adjust_heap(K, V, parent, len, K[parent], V[parent]);
        if (parent == 0) break;
    }
    while (len > 1) {
        --len;
        const uint64_t vk = K[len];
        const uint32_t vv = V[len];
        K[len] = K[0];
        V[len] = V[0];
        adjust_heap(K, V, 0, len, vk, vv);
    }
}

// libstdc++ std::sort (bits/stl_algo.h) of the pairs (K, V)[0, n) by K, literally: the order of
// equal keys is part of the result.  __introsort_loop's recursion on [cut, last) becomes a push on
// an explicit stack (one segment per level: at most 2 * lg n < kSortStack of them wait at a time);
// depth < 0: the library's 2 * __lg(n).  __final_insertion_sort's two forms (__insertion_sort with
// its move_backward for a new minimum, __unguarded_linear_insert) both put an element behind the
// last one that is not greater, which is the one loop below.
MUMS_HD_FN void std_sort_kv(uint64_t* K, uint32_t* V, uint32_t n, int depth) {
    if (n < 2) return;
    if (n > kSortLeaf) {
        uint32_t sf[kSortStack], sl[kSortStack];
        int sd[kSortStack];
        int top = 0;
        sf[0] = 0;
        sl[0] = n;
        sd[0] = depth >= 0 ? depth : 2 * (31 - __builtin_clz(n));
        top = 1;
        while (top > 0) {
            --top;
            uint32_t first = sf[top], last = sl[top];
            int d = sd[top];
            while (last - first > kSortLeaf) {
                if (d == 0) {
                    heap_sort(K + first, V + first, (int64_t)(last - first));
                    break;
                }
                --d;
                // __move_median_to_first(first, first + 1, mid, last - 1)
                const uint32_t a = first + 1, b = first + (last - first) / 2, c = last - 1;
                const uint64_t ka = K[a], kb = K[b], kc = K[c];
                uint32_t m;
                if (ka < kb) m = kb < kc ? b : (ka < kc ? c : a);
                else m = ka < kc ? a : (kb < kc ? c : b);
                swap_kv(K, V, first, m);
                // __unguarded_partition(first + 1, last, first)
                const uint64_t pv = K[first];
                uint32_t lo = first + 1, hi = last;
                for (;;) {
                    while (K[lo] < pv) ++lo;
                    --hi;
                    while (pv < K[hi]) --hi;
                    if (!(lo < hi)) break;
                    swap_kv(K, V, lo, hi);
                    ++lo;
                }
                // __introsort_loop(cut, last, depth_limit); last = cut
                if (top < kSortStack) {
                    sf[top] = lo;
                    sl[top] = last;
                    sd[top] = d;
                    ++top;
                }
                last = lo;
            }
        }
    }
    for (uint32_t i = 1; i < n; ++i) {
        const uint64_t vk = K[i];
        const uint32_t vv = V[i];
        uint32_t j = i;
        while (j > 0 && vk < K[j - 1]) {
            K[j] = K[j - 1];
            V[j] = V[j - 1];
            --j;
        }
        K[j] = vk;
        V[j] = vv;
    }
}

// One list's tail: EliminateOverlaps_v2(list, eliminate_both) over every sequence in order (the
// two-argument overload, ProgressiveAligner.h:397-406), then LengthFilter(min_length).  The list is
// rows [0, n) of plen / ps (ps: n x G starts, changed in place by the crops), K and V are n words of
// scratch each.  Afterwards V[0, returned count) holds the surviving rows' ids in list order.
// Like the reference's vector, the id array keeps the order of one sequence's pass as the input
// order of the next one's sort.
MUMS_HD_FN uint32_t anchor_tail(uint64_t* K, uint32_t* V, int64_t* plen, int64_t* ps, uint32_t n, int G,
                                      int eliminate_both, uint64_t min_length) {
    for (uint32_t i = 0; i < n; ++i) V[i] = i;
    if (n >= 2) {   // if( ml.size() < 2 ) return;
        for (int seqI = 0; seqI < G && n > 0; ++seqI) {
            for (uint32_t i = 0; i < n; ++i) {   // SingleStartComparator (AbstractMatch.h:324-351): |start|, NO_MATCH first
                const int64_t s = ps[(uint64_t)V[i] * G + seqI];
                K[i] = (uint64_t)(s < 0 ? -s : s);
            }
            std_sort_kv(K, V, n, -1);
            uint32_t a = 0;
            while (a < n && K[a] == 0) ++a;
            const uint64_t dels = v2_walk(V, plen, ps, G, seqI, (int64_t)a, (int64_t)n, eliminate_both);
            if (dels > 0) {
                uint32_t cur = 0;
                for (uint32_t i = 0; i < n; ++i)
                    if (V[i] != kDeleted) V[cur++] = V[i];
                n = cur;
            }
        }
    }
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n; ++i)
        if ((uint64_t)plen[V[i]] >= min_length) V[kept++] = V[i];
    return kept;
}

}  // namespace lane
}  // namespace mums
