// recursion_lane.h -- the sequential pieces of Aligner::Recursion's tail (Aligner.cpp:1211-1218) as
// one lane runs them: EliminateOverlaps (the v1 of Aligner.cpp:62-176: libstdc++'s std::sort per
// sequence, the matchI / nextI walk that appends the cut-off overlap of a pair as a new match),
// MultiplicityFilter (MatchList.h:636-649) and LengthFilter (:652-664).
//
// recursion.hip replays a whole small list per lane, one list per problem of a batch.  The list
// grows: a problem owns a slice of `cap` rows (lengths, G starts per row, one K and one V word per
// row); rows [0, n) are the input, every kept copy becomes the next free row and rows are never
// freed, so the live id list (V) is never longer than the rows in use.  Plain C++ on caller-owned
// arrays: tests/recursion_lane_shim.cpp compiles this header for the host and holds it to
// tests/eo_model.cpp (the toolchain's real std::sort on Match*) without a device.
#pragma once

#include "anchor_lane.h"

namespace mums {
namespace lane {

// Rows of the slice of a list of n input rows over G sequences (DESIGN.md §4f has the reasoning and
// the counts behind it).  A list below 2 rows is returned as it is, and a copy needs a source of
// multiplicity 3, so G = 2 never appends: such lists get their input rows.  The others get
// slice_factor(G) rows per input row, which grows with G because a copy of multiplicity m can be
// copied again in each later pass, and kSliceSlack on top, so that a short list with a few copies is
// not the one that runs alone.
constexpr uint32_t kSliceSlack = 32;
constexpr uint32_t kSliceFactorMax = 16;
MUMS_HD uint32_t slice_factor(int G) {
    const uint32_t f = G <= 3 ? 2u : 2u * (uint32_t)(G - 2);
    return f < kSliceFactorMax ? f : kSliceFactorMax;
}
MUMS_HD uint32_t slice_rows(uint32_t n, int G) { return n < 2 || G <= 2 ? n : slice_factor(G) * n + kSliceSlack; }

struct V1Counts {
    uint32_t dels = 0;       // matches deleted by the walks
    uint32_t apps = 0;       // copies kept (rows appended)
    bool overflow = false;   // a copy did not fit the slice: nothing was written past it, the result is void
};

// EliminateOverlaps' matchI / nextI loops (Aligner.cpp:76-160) over V[a, b): ids of matches that are
// all defined in seqI, sorted by SingleStartComparator(seqI).  The decisions and their order are
// cluster_sim_kernel's (overlaps.hip).  Every overlapping pair copies its smaller match before the
// crop (:97, :126), keeps of the copy what the crop cuts off, drops seqI from it (:152) and keeps it
// when Multiplicity() > 1 && Length() > 0 (:153).  The copy has one sequence less than its source,
// so a source of multiplicity <= 2 is never copied here; a kept copy is row *rows, in creation
// order.  Returns the deleted matches of this walk; c->overflow set: stopped in front of a copy
// that has no row.
MUMS_HD_FN uint32_t v1_walk(uint32_t* V, int64_t* plen, int64_t* ps, int G, int seqI, int64_t a, int64_t b,
                            uint32_t* rows, uint32_t cap, V1Counts* c) {
    uint32_t dels = 0;
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
            const int mJ = mult_of(sJ, G), mI = mult_of(sI, G);
            const bool i_smaller = mJ > mI || (mJ == mI && plen[J] > lenI);
            const uint64_t src = i_smaller ? I : J;
            const bool copy = (i_smaller ? mI : mJ) > 2;
            int64_t* sN = nullptr;
            int64_t lenN = plen[src];
            if (copy) {
                if (*rows >= cap) {
                    c->overflow = true;
                    c->dels += dels;
                    return dels;
                }
                sN = ps + (uint64_t)*rows * G;
                for (int g = 0; g < G; ++g) sN[g] = ps[src * G + g];
            }
            if (i_smaller) {
                if (diff >= lenI) {
                    V[mi] = kDeleted;
                    deleted_i = true;
                    ++dels;
                } else if (startI > 0) {
                    crop_end(&plen[I], sI, G, diff);
                    if (copy) crop_start(&lenN, sN, G, lenN - diff);
                } else {
                    crop_start(&plen[I], sI, G, diff);
                    if (copy) crop_end(&lenN, sN, G, lenN - diff);
                }
            } else {
                if (diff >= plen[J]) {
                    V[nj] = kDeleted;
                    ++dels;
                } else if (startJ > 0) {
                    crop_start(&plen[J], sJ, G, diff);
                    if (copy) crop_end(&lenN, sN, G, lenN - diff);
                } else {
                    crop_end(&plen[J], sJ, G, diff);
                    if (copy) crop_start(&lenN, sN, G, lenN - diff);
                }
            }
            if (copy) {
                sN[seqI] = 0;   // new_match->SetStart( seqI, 0 )
                if (lenN > 0) {
                    plen[*rows] = lenN;
                    ++*rows;
                    ++c->apps;
                }
            }
            if (deleted_i) break;   // (matchI-- then ++ in the reference: the same index, now NULL)
        }
    }
    c->dels += dels;
    return dels;
}

// One list's tail: EliminateOverlaps(list), then MultiplicityFilter(multiplicity) (0: none) and
// LengthFilter(min_length).  The list is rows [0, n) of plen / ps, n <= cap; plen has cap words, ps
// cap x G, K and V cap words each.  Afterwards V[0, returned count) holds the surviving rows' ids in
// list order.  Like the reference's vector, the id array keeps the order of one sequence's pass
// (the survivors, then the pass's new matches: :162-171) as the input order of the next one's sort.
MUMS_HD_FN uint32_t recursion_tail(uint64_t* K, uint32_t* V, int64_t* plen, int64_t* ps, uint32_t n, uint32_t cap,
                                   int G, uint32_t multiplicity, uint64_t min_length, V1Counts* c) {
    uint32_t rows = n;
    for (uint32_t i = 0; i < n; ++i) V[i] = i;
    if (n >= 2) {   // if( ml.size() < 2 ) return;
        for (int seqI = 0; seqI < G && n > 0; ++seqI) {
            for (uint32_t i = 0; i < n; ++i) {   // SingleStartComparator: |start|, NO_MATCH first
                const int64_t s = ps[(uint64_t)V[i] * G + seqI];
                K[i] = (uint64_t)(s < 0 ? -s : s);
            }
            std_sort_kv(K, V, n, -1);
            uint32_t a = 0;
            while (a < n && K[a] == 0) ++a;
            const uint32_t first_new = rows;
            const uint32_t dels = v1_walk(V, plen, ps, G, seqI, (int64_t)a, (int64_t)n, &rows, cap, c);
            if (c->overflow) return 0;
            if (dels > 0) {
                uint32_t cur = 0;
                for (uint32_t i = 0; i < n; ++i)
                    if (V[i] != kDeleted) V[cur++] = V[i];
                n = cur;
            }
            for (uint32_t r = first_new; r < rows; ++r) V[n++] = r;   // ml.insert( ml.end(), new_matches )
        }
    }
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t id = V[i];
        if (multiplicity != 0 && (uint32_t)mult_of(ps + (uint64_t)id * G, G) != multiplicity) continue;
        if ((uint64_t)plen[id] >= min_length) V[kept++] = id;
    }
    return kept;
}

}  // namespace lane
}  // namespace mums
