// TEST INFRASTRUCTURE ONLY: EliminateOverlaps_v2 (libMems/ProgressiveAligner.h:300-406) over
// Match* vectors sorted by this toolchain's real std::sort, statement by statement: Length(seqI)
// (UngappedLocalAlignment.h:48-55), CropLeft / CropRight (:169-184), checkConsistent
// (ProgressiveAligner.h:272-291) and processNewMatch (:260-271) with its push of a kept match,
// so that "v2 never appends to a list of ungapped matches" is a counted result, not a premise.
#include <algorithm>
#include <cstdint>
#include <limits>
#include <vector>

namespace {
struct M {
    int64_t len;              // m_length
    std::vector<int64_t> s;   // Start(seqI): signed, NO_MATCH = 0
    int64_t Start(unsigned seqI) const { return s[seqI]; }
    int64_t LeftEnd(unsigned seqI) const { return s[seqI] < 0 ? -s[seqI] : s[seqI]; }
    void SetStart(unsigned seqI, int64_t v) { s[seqI] = v; }
    bool Forward(unsigned seqI) const { return s[seqI] > 0; }   // Orientation(seqI) == forward
    int64_t Length(unsigned seqI) const {                        // UngappedLocalAlignment.h:48-55
        if (LeftEnd(seqI) == 0) return 0;
        return len;
    }
    unsigned Multiplicity() const {
        unsigned k = 0;
        for (int64_t v : s) k += v != 0;
        return k;
    }
    M* Copy() const { return new M(*this); }
    void CropStart(int64_t a) {   // :138: m_length -= a; MoveStart(a)
        len -= a;
        for (auto& v : s)
            if (v > 0) v += a;
    }
    void CropEnd(int64_t a) {     // :147: m_length -= a; MoveEnd(a)
        len -= a;
        for (auto& v : s)
            if (v < 0) v -= a;
    }
    void CropLeft(int64_t a, unsigned seqI) {    // :169
        if (Forward(seqI)) CropStart(a);
        else CropEnd(a);
    }
    void CropRight(int64_t a, unsigned seqI) {   // :178
        if (Forward(seqI)) CropEnd(a);
        else CropStart(a);
    }
};

int64_t absolut(int64_t x) { return x < 0 ? -x : x; }

// ProgressiveAligner.h:260-271; returns 1 when the match was kept
int processNewMatch(unsigned seqI, std::vector<M*>& new_matches, M*& new_match) {
    new_match->SetStart(seqI, 0);
    if (new_match->Multiplicity() > 1 && new_match->Length(seqI) > 0) {
        new_matches.push_back(new_match);
        return 1;
    }
    delete new_match;
    new_match = nullptr;
    return 0;
}

// ProgressiveAligner.h:272-291
bool checkConsistent(const M* a, const M* b) {
    bool consistent_overlap = true;
    int64_t o = (std::numeric_limits<int64_t>::max)();
    int64_t inter = 0;
    const size_t seq_count = a->s.size();
    for (size_t seqI = 0; seqI < seq_count; seqI++) {
        if (b->LeftEnd(seqI) == 0 || a->LeftEnd(seqI) == 0) continue;
        inter++;
        if (o == (std::numeric_limits<int64_t>::max)()) o = b->Start(seqI) - a->Start(seqI);
        if (o != b->Start(seqI) - a->Start(seqI)) consistent_overlap = false;
    }
    consistent_overlap = consistent_overlap && inter > 1;
    return consistent_overlap;
}

enum { kPairs, kConsistent, kDelI, kDelJ, kCropI, kCropJ, kKept, kCounters };
}  // namespace

// seq_ids == NULL: every sequence in order (:397-406).  counters[7]: overlapping pairs,
// consistent pairs, matchI deleted, nextI deleted, matchI cropped, nextI cropped, new matches kept.
extern "C" uint64_t model_eliminate_overlaps_v2(int G, uint64_t n, const uint64_t* len, const int64_t* s,
                                                const uint32_t* seq_ids_in, uint32_t nids, int eliminate_both_in,
                                                uint64_t* len_out, int64_t* s_out, uint64_t cap, uint64_t* counters) {
    std::vector<M*> ml;
    for (uint64_t i = 0; i < n; ++i) ml.push_back(new M{(int64_t)len[i], std::vector<int64_t>(s + i * G, s + i * G + G)});
    std::vector<unsigned> seq_ids;
    if (seq_ids_in) seq_ids.assign(seq_ids_in, seq_ids_in + nids);
    else
        for (int g = 0; g < G; ++g) seq_ids.push_back((unsigned)g);
    const bool eliminate_both = eliminate_both_in != 0;
    uint64_t cnt[kCounters] = {};
    if (ml.size() >= 2) {
        for (unsigned sidI = 0; sidI < seq_ids.size(); sidI++) {
            const unsigned seqI = seq_ids[sidI];
            std::sort(ml.begin(), ml.end(), [seqI](const M* a, const M* b) {   // SingleStartComparator
                const int64_t x = a->LeftEnd(seqI), y = b->LeftEnd(seqI);
                if (x == 0 || y == 0) return y != 0;
                return x < y;
            });
            int64_t matchI = 0, nextI = 0, deleted_count = 0;
            std::vector<M*> new_matches;
            for (; matchI != (int64_t)ml.size(); matchI++)
                if (ml[matchI]->Start(seqI) != 0) break;
            for (; matchI < (int64_t)ml.size(); matchI++) {
                if (ml[matchI] == nullptr) continue;
                for (nextI = matchI + 1; nextI < (int64_t)ml.size(); nextI++) {
                    if (ml[nextI] == nullptr) continue;
                    bool deleted_matchI = false;
                    const int64_t startI = ml[matchI]->Start(seqI);
                    const int64_t lenI = ml[matchI]->Length(seqI);
                    const int64_t startJ = ml[nextI]->Start(seqI);
                    int64_t diff = absolut(startJ) - absolut(startI) - lenI;
                    if (diff >= 0) break;
                    diff = -diff;
                    cnt[kPairs]++;
                    M* new_match;
                    const bool mem_iter_smaller =
                        (ml[nextI]->Multiplicity() > ml[matchI]->Multiplicity()) ||
                        (ml[nextI]->Multiplicity() == ml[matchI]->Multiplicity() &&
                         ml[nextI]->Length(seqI) > ml[matchI]->Length(seqI));
                    const bool consistent_overlap = checkConsistent(ml[matchI], ml[nextI]);
                    cnt[kConsistent] += consistent_overlap;
                    if ((!consistent_overlap && eliminate_both) || mem_iter_smaller) {
                        new_match = ml[matchI]->Copy();
                        if (diff >= lenI) {
                            delete ml[matchI];
                            ml[matchI] = nullptr;
                            matchI--;
                            deleted_matchI = true;
                            deleted_count++;
                            cnt[kDelI]++;
                        } else {
                            ml[matchI]->CropRight(diff, seqI);
                            new_match->CropLeft(new_match->Length(seqI) - diff, seqI);
                            cnt[kCropI]++;
                        }
                        cnt[kKept] += processNewMatch(seqI, new_matches, new_match);
                    }
                    if ((!consistent_overlap && eliminate_both) || !mem_iter_smaller) {
                        new_match = ml[nextI]->Copy();
                        if (diff >= ml[nextI]->Length(seqI)) {
                            delete ml[nextI];
                            ml[nextI] = nullptr;
                            deleted_count++;
                            cnt[kDelJ]++;
                        } else {
                            ml[nextI]->CropLeft(diff, seqI);
                            new_match->CropRight(new_match->Length(seqI) - diff, seqI);
                            cnt[kCropJ]++;
                        }
                        cnt[kKept] += processNewMatch(seqI, new_matches, new_match);
                    }
                    if (deleted_matchI) break;
                }
            }
            if (deleted_count > 0) {
                size_t cur = 0;
                for (size_t mI = 0; mI < ml.size(); ++mI)
                    if (ml[mI] != nullptr) ml[cur++] = ml[mI];
                ml.erase(ml.begin() + cur, ml.end());
            }
            ml.insert(ml.end(), new_matches.begin(), new_matches.end());
            new_matches.clear();
        }
    }
    if (counters)
        for (int k = 0; k < kCounters; ++k) counters[k] = cnt[k];
    uint64_t k = 0;
    for (M* m : ml) {
        if (k < cap) {
            len_out[k] = (uint64_t)m->len;
            for (int g = 0; g < G; ++g) s_out[k * G + g] = m->s[g];
        }
        ++k;
        delete m;
    }
    return k;
}
