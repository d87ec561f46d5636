// batch_plan.h -- the host plan of a batched find (mums_find_batch, mums_anchor_batch; DESIGN.md
// §4d / §4e): which problems the lanes take, in what order, and where their slices of the record
// index space and of the carried table start.  Host only, no HIP: mums_capi.hip and
// tests/batch_plan_shim.cpp compile the same code.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace mums {
namespace batch {

inline int ceil_log2(uint64_t x) {
    int b = 0;
    while ((1ull << b) < x) ++b;
    return b;
}

constexpr uint64_t kIndexLimit = 0xFFFFFFF0ull;   // record and table indices are 32-bit

enum Status { kOk = 0, kTooManySequences, kTooManySeedMers, kTooManySlots };

struct Round {
    int L;       // seed length
    int kbits;   // bits of the canonical key, 2w + 1
};

// The size rule's constants: the lanes run side by side, so their pass lasts as long as its
// largest problem, about lane_us per seed-mer (of all its rounds), while a problem run alone
// costs about alone_us whatever its size.
struct Cost {
    double lane_us, alone_us;
};

struct Plan {
    Status status = kOk;
    bool lanes = true;                  // the sort key (problem id above the canonical key) fits 64 bits in every round
    std::vector<uint64_t> recs, tot;    // seed-mers: recs[r * B + p]; tot[p] = their sum over the rounds
    std::vector<uint8_t> routed;        // the problem runs alone
    std::vector<uint32_t> order;        // lane order: the routed problems, then by tot descending (stable)
    std::vector<uint64_t> aoff, nlen;   // nseg + 1 each: a sequence's offset from the batch's first base, its length
    std::vector<std::vector<uint32_t>> mbase;   // per round, nseg + 1: running sum of the lane problems' seed-mers
    std::vector<uint64_t> N, Nall;      // per round: the lanes' records, all records
    uint64_t Nmax = 0, Nsum = 0;        // of N over the rounds
    // problem p's slice of the carried table: an entry needs a probe and a probe two records of its
    // round, so the table after the last round has at most the sum over the rounds of half the
    // round's records
    std::vector<uint32_t> obase, ocap;
    uint64_t ord_words = 0;
};

inline bool too_many_sequences(uint32_t B, uint32_t G) { return (uint64_t)B * G + 1 >= (1ull << 32); }

// seq_off: B * G + 1 non-decreasing offsets.  cap: seed-mers of one problem in one round the lanes take.
inline Plan make_plan(uint32_t B, uint32_t G, const uint64_t* seq_off, const std::vector<Round>& rounds, uint64_t cap,
                      bool no_split, Cost cost) {
    Plan pl;
    if (too_many_sequences(B, G)) {
        pl.status = kTooManySequences;
        return pl;
    }
    const uint64_t nseg = (uint64_t)B * G;
    const size_t R = rounds.size();
    const int pbits = ceil_log2(B ? B : 1);
    for (const Round& x : rounds) pl.lanes = pl.lanes && x.kbits + pbits <= 64;
    auto mers = [](uint64_t n, uint64_t L) { return n < L ? 0 : n - L + 1; };
    pl.recs.assign((size_t)B * R, 0);
    pl.tot.assign(B, 0);
    pl.routed.assign(B, 0);
    pl.N.assign(R, 0);
    pl.Nall.assign(R, 0);
    for (size_t r = 0; r < R; ++r) {
        for (uint32_t p = 0; p < B; ++p) {
            uint64_t k = 0;
            for (uint32_t g = 0; g < G; ++g)
                k += mers(seq_off[(uint64_t)p * G + g + 1] - seq_off[(uint64_t)p * G + g], (uint64_t)rounds[r].L);
            pl.recs[r * B + p] = k;
            pl.tot[p] += k;
            pl.Nall[r] += k;
            if (!pl.lanes || k > cap) pl.routed[p] = 1;
            if (pl.Nall[r] >= kIndexLimit) {
                pl.status = kTooManySeedMers;
                return pl;
            }
        }
    }
    // the size rule: the k largest problems run alone, k minimising the sum of the two costs
    pl.order.resize(B);
    for (uint32_t p = 0; p < B; ++p) pl.order[p] = p;
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](uint32_t x, uint32_t y) {
        return (pl.routed[x] ? ~0ull : pl.tot[x]) > (pl.routed[y] ? ~0ull : pl.tot[y]);
    });
    if (pl.lanes && !no_split) {
        uint32_t k0 = 0, best = 0;
        while (k0 < B && pl.routed[pl.order[k0]]) ++k0;
        double best_cost = -1;
        for (uint32_t k = k0; k <= B; ++k) {
            const double c = cost.lane_us * (double)(k < B ? pl.tot[pl.order[k]] : 0) + cost.alone_us * (double)(k - k0);
            if (best_cost < 0 || c < best_cost) { best_cost = c; best = k; }
        }
        for (uint32_t k = k0; k < best; ++k) pl.routed[pl.order[k]] = 1;
    }
    pl.aoff.assign(nseg + 1, 0);
    pl.nlen.assign(nseg + 1, 0);
    for (uint64_t s = 0; s < nseg; ++s) {
        pl.aoff[s] = seq_off[s] - seq_off[0];
        pl.nlen[s] = seq_off[s + 1] - seq_off[s];
    }
    pl.mbase.assign(R, std::vector<uint32_t>(nseg + 1, 0));
    for (size_t r = 0; r < R; ++r) {
        uint64_t n = 0;
        for (uint64_t s = 0; s < nseg; ++s) {
            pl.mbase[r][s] = (uint32_t)n;
            if (!pl.routed[s / G]) n += mers(pl.nlen[s], (uint64_t)rounds[r].L);
        }
        pl.mbase[r][nseg] = (uint32_t)n;
        pl.N[r] = n;
        pl.Nmax = std::max(pl.Nmax, n);
        pl.Nsum += n;
    }
    pl.obase.assign(B, 0);
    pl.ocap.assign(B, 0);
    for (uint32_t p = 0; p < B; ++p) {
        uint64_t c = 0;
        for (size_t r = 0; r < R && !pl.routed[p]; ++r) c += pl.recs[r * B + p] >> 1;
        if (pl.ord_words + c >= kIndexLimit) {
            pl.status = kTooManySlots;
            return pl;
        }
        pl.obase[p] = (uint32_t)pl.ord_words;
        pl.ocap[p] = (uint32_t)c;
        pl.ord_words += c;
    }
    return pl;
}

}  // namespace batch
}  // namespace mums
