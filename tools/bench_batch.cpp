// bench_batch -- many small gap searches: mums_find_batch against a loop of single finds.
//
// Through the C ABI only (no interpreter in either number), the library loaded at run time so
// that one binary times a build without mums_find_batch too:
//   bench_batch --lib PATH [--workload w1|w2] [--reps 5] [--mode loop|batch|both|anchor-loop|anchor-batch|anchor]
//               [--oracle PATH]
// Workloads (fixed generator seed, default seed per problem as pairwiseAnchorSearch chooses it,
// ProgressiveAligner.cpp:615-616, table size 40000), measured from host ASCII to host MatchList:
//   w1  4096 problems, two sequences, lengths uniform in [200, 4000], the partner a copy with 5 %
//       substitutions, every second partner reverse-complemented
//   w2  256 problems of 2 x 50000 bases, the same otherwise
// loop  = mums_clear / mums_add_genome x2 / mums_find / mums_result_copy per problem on one context
// batch = problems grouped by seed pattern, one mums_find_batch + mums_result_copy per pattern
// The anchor modes time the whole of pairwiseAnchorSearch with seed families (ranks 0-2 of each
// problem's default weight, eliminate_both 0, min_length 12):
// anchor-loop  = per problem mums_clear; per rank mums_clear_sequences / mums_set_seed / mums_add_genome x2 /
//                mums_find; mums_eliminate_overlaps_v2(NULL, 0, 0); mums_length_filter(12); mums_result_copy
// anchor-batch = problems grouped by weight, one mums_anchor_batch + mums_result_copy per weight
// anchor       = both, and the lists compared row by row
// --oracle: the CPU oracle (oracle/build/libmums_oracle.so) on one thread, timed once, and every
// list compared with it.
// Prints one JSON object per line: the repetitions' milliseconds, their median and spread
// (max - min), a hash of all lists, and for the batch the phase split of mums_get_stats.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../include/mums.h"
#include "../oracle/mums_oracle.h"

namespace {

struct Api {
    decltype(&mums_ctx_create) ctx_create;
    decltype(&mums_ctx_destroy) ctx_destroy;
    decltype(&mums_set_seed) set_seed;
    decltype(&mums_set_params) set_params;
    decltype(&mums_clear) clear;
    decltype(&mums_add_genome) add_genome;
    decltype(&mums_find) find;
    decltype(&mums_result_count) result_count;
    decltype(&mums_result_copy) result_copy;
    decltype(&mums_get_stats) get_stats;
    decltype(&mums_last_error) last_error;
    decltype(&mums_get_seed) get_seed;
    decltype(&mums_default_seed_weight) default_seed_weight;
    decltype(&mums_find_batch) find_batch;   // null in a build without it
    decltype(&mums_batch_info) batch_info;
    decltype(&mums_clear_sequences) clear_sequences;
    decltype(&mums_eliminate_overlaps_v2) eliminate_overlaps_v2;
    decltype(&mums_length_filter) length_filter;
    decltype(&mums_anchor_batch) anchor_batch;   // null in a build without it
    decltype(&mums_anchor_batch_info) anchor_batch_info;
};

constexpr int kFamilyRanks = 3;          // --seed-family: ranks 0, 1, 2 (ProgressiveAligner.cpp:619-653)
constexpr uint64_t kAnchorMinLength = 12;   // MIN_ANCHOR_LENGTH + 3 (:659)

template <typename F>
bool sym(void* h, const char* name, F* f, bool required = true) {
    *f = (F)dlsym(h, name);
    if (!*f && required) fprintf(stderr, "bench_batch: %s missing in the library\n", name);
    return *f || !required;
}

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

struct Workload {
    std::string ascii;               // all sequences, problem-major
    std::vector<uint64_t> off;       // 2 B + 1
    std::vector<uint64_t> pattern;   // per problem (0: default weight 0, no search)
    std::vector<uint32_t> weight;    // per problem: its default seed weight
    uint32_t B = 0;
};

Workload make_workload(const Api& a, const std::string& name) {
    Workload w;
    Rng r{name == "w1" ? 20261020ull : 20261021ull};
    w.B = name == "w1" ? 4096 : 256;
    static const char acgt[4] = {'A', 'C', 'G', 'T'};
    w.off.push_back(0);
    for (uint32_t p = 0; p < w.B; ++p) {
        const uint64_t n = name == "w1" ? 200 + r.next() % 3801 : 50000;
        std::string s0(n, 'A'), s1;
        for (auto& c : s0) c = acgt[r.next() & 3];
        s1 = s0;
        for (auto& c : s1)
            if (r.next() % 100 < 5) c = acgt[r.next() & 3];
        if (p & 1) {
            std::reverse(s1.begin(), s1.end());
            for (auto& c : s1) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
        }
        w.ascii += s0;
        w.off.push_back(w.ascii.size());
        w.ascii += s1;
        w.off.push_back(w.ascii.size());
        const uint32_t wt = a.default_seed_weight((s0.size() + s1.size()) / 2);
        w.pattern.push_back(wt ? (uint64_t)a.get_seed((int)wt, 0) : 0);
        w.weight.push_back(wt);
    }
    return w;
}

struct Lists {   // every problem's MatchList, problem order
    std::vector<uint64_t> moff, len;
    std::vector<int64_t> st;
    uint64_t hash() const {
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
        for (uint64_t v : moff) mix(v);
        for (uint64_t v : len) mix(v);
        for (int64_t v : st) mix((uint64_t)v);
        return h;
    }
    bool operator==(const Lists& o) const { return moff == o.moff && len == o.len && st == o.st; }
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

#define CK(call)                                                                              \
    do {                                                                                      \
        const int rc_ = (call);                                                               \
        if (rc_ != MUMS_OK) {                                                                 \
            fprintf(stderr, "bench_batch: %s -> %d (%s)\n", #call, rc_, a.last_error(ctx));  \
            return false;                                                                     \
        }                                                                                     \
    } while (0)

bool run_loop(const Api& a, mums_ctx* ctx, const Workload& w, Lists* out) {
    out->moff.assign(1, 0);
    out->len.clear();
    out->st.clear();
    for (uint32_t p = 0; p < w.B; ++p) {
        if (w.pattern[p]) {
            CK(a.clear(ctx));
            CK(a.set_seed(ctx, w.pattern[p]));
            for (int g = 0; g < 2; ++g)
                CK(a.add_genome(ctx, w.ascii.data() + w.off[2 * p + g], w.off[2 * p + g + 1] - w.off[2 * p + g]));
            CK(a.find(ctx));
            uint64_t M = 0;
            CK(a.result_count(ctx, &M, nullptr));
            const size_t l0 = out->len.size();
            out->len.resize(l0 + M);
            out->st.resize((l0 + M) * 2);
            if (M) CK(a.result_copy(ctx, out->len.data() + l0, out->st.data() + l0 * 2));
        }
        out->moff.push_back(out->len.size());
    }
    return true;
}

bool run_batch(const Api& a, mums_ctx* ctx, const Workload& w, Lists* out, mums_stats* phases) {
    std::map<uint64_t, std::vector<uint32_t>> groups;
    for (uint32_t p = 0; p < w.B; ++p)
        if (w.pattern[p]) groups[w.pattern[p]].push_back(p);
    std::vector<std::vector<uint64_t>> plen(w.B);
    std::vector<std::vector<int64_t>> pst(w.B);
    *phases = mums_stats{};
    for (const auto& kv : groups) {
        const std::vector<uint32_t>& idx = kv.second;
        std::string blob;
        std::vector<uint64_t> off(1, 0);
        for (uint32_t p : idx)
            for (int g = 0; g < 2; ++g) {
                blob.append(w.ascii, w.off[2 * p + g], w.off[2 * p + g + 1] - w.off[2 * p + g]);
                off.push_back(blob.size());
            }
        CK(a.set_seed(ctx, kv.first));
        CK(a.find_batch(ctx, (uint32_t)idx.size(), 2, blob.data(), off.data()));
        uint64_t M = 0;
        CK(a.result_count(ctx, &M, nullptr));
        std::vector<uint64_t> len(M), mo(idx.size() + 1);
        std::vector<int64_t> st(M * 2);
        if (M) CK(a.result_copy(ctx, len.data(), st.data()));
        CK(a.batch_info(ctx, mo.data(), nullptr, nullptr, nullptr));
        for (size_t j = 0; j < idx.size(); ++j) {
            plen[idx[j]].assign(len.begin() + mo[j], len.begin() + mo[j + 1]);
            pst[idx[j]].assign(st.begin() + 2 * mo[j], st.begin() + 2 * mo[j + 1]);
        }
        mums_stats s;
        CK(a.get_stats(ctx, &s));
        phases->ms_keys += s.ms_keys;
        phases->ms_sort += s.ms_sort;
        phases->ms_replay += s.ms_replay;
        phases->ms_output += s.ms_output;
        phases->ms_total += s.ms_total;
        phases->restarts += s.restarts;
    }
    out->moff.assign(1, 0);
    out->len.clear();
    out->st.clear();
    for (uint32_t p = 0; p < w.B; ++p) {
        out->len.insert(out->len.end(), plen[p].begin(), plen[p].end());
        out->st.insert(out->st.end(), pst[p].begin(), pst[p].end());
        out->moff.push_back(out->len.size());
    }
    return true;
}

bool take_list(const Api& a, mums_ctx* ctx, Lists* out) {
    uint64_t M = 0;
    CK(a.result_count(ctx, &M, nullptr));
    const size_t l0 = out->len.size();
    out->len.resize(l0 + M);
    out->st.resize((l0 + M) * 2);
    if (M) CK(a.result_copy(ctx, out->len.data() + l0, out->st.data() + l0 * 2));
    return true;
}

bool run_anchor_loop(const Api& a, mums_ctx* ctx, const Workload& w, Lists* out) {
    out->moff.assign(1, 0);
    out->len.clear();
    out->st.clear();
    for (uint32_t p = 0; p < w.B; ++p) {
        if (w.weight[p]) {
            CK(a.clear(ctx));
            for (int r = 0; r < kFamilyRanks; ++r) {
                CK(a.clear_sequences(ctx));
                CK(a.set_seed(ctx, (uint64_t)a.get_seed((int)w.weight[p], r)));
                for (int g = 0; g < 2; ++g)
                    CK(a.add_genome(ctx, w.ascii.data() + w.off[2 * p + g], w.off[2 * p + g + 1] - w.off[2 * p + g]));
                CK(a.find(ctx));
            }
            CK(a.eliminate_overlaps_v2(ctx, nullptr, 0, 0));
            CK(a.length_filter(ctx, kAnchorMinLength));
            if (!take_list(a, ctx, out)) return false;
        }
        out->moff.push_back(out->len.size());
    }
    return true;
}

bool run_anchor_batch(const Api& a, mums_ctx* ctx, const Workload& w, Lists* out, mums_stats* phases) {
    std::map<uint32_t, std::vector<uint32_t>> groups;
    for (uint32_t p = 0; p < w.B; ++p)
        if (w.weight[p]) groups[w.weight[p]].push_back(p);
    std::vector<std::vector<uint64_t>> plen(w.B);
    std::vector<std::vector<int64_t>> pst(w.B);
    *phases = mums_stats{};
    for (const auto& kv : groups) {
        const std::vector<uint32_t>& idx = kv.second;
        std::string blob;
        std::vector<uint64_t> off(1, 0);
        for (uint32_t p : idx)
            for (int g = 0; g < 2; ++g) {
                blob.append(w.ascii, w.off[2 * p + g], w.off[2 * p + g + 1] - w.off[2 * p + g]);
                off.push_back(blob.size());
            }
        uint64_t pats[kFamilyRanks];
        for (int r = 0; r < kFamilyRanks; ++r) pats[r] = (uint64_t)a.get_seed((int)kv.first, r);
        CK(a.anchor_batch(ctx, (uint32_t)idx.size(), 2, blob.data(), off.data(), pats, kFamilyRanks, 0, kAnchorMinLength));
        uint64_t M = 0;
        CK(a.result_count(ctx, &M, nullptr));
        std::vector<uint64_t> len(M), mo(idx.size() + 1);
        std::vector<int64_t> st(M * 2);
        if (M) CK(a.result_copy(ctx, len.data(), st.data()));
        CK(a.anchor_batch_info(ctx, mo.data(), nullptr, nullptr, nullptr, nullptr));
        for (size_t j = 0; j < idx.size(); ++j) {
            plen[idx[j]].assign(len.begin() + mo[j], len.begin() + mo[j + 1]);
            pst[idx[j]].assign(st.begin() + 2 * mo[j], st.begin() + 2 * mo[j + 1]);
        }
        mums_stats s;
        CK(a.get_stats(ctx, &s));
        phases->ms_keys += s.ms_keys;
        phases->ms_sort += s.ms_sort;
        phases->ms_replay += s.ms_replay;
        phases->ms_output += s.ms_output;
        phases->ms_total += s.ms_total;
        phases->restarts += s.restarts;
        phases->mem_count += s.mem_count;
    }
    out->moff.assign(1, 0);
    out->len.clear();
    out->st.clear();
    for (uint32_t p = 0; p < w.B; ++p) {
        out->len.insert(out->len.end(), plen[p].begin(), plen[p].end());
        out->st.insert(out->st.end(), pst[p].begin(), pst[p].end());
        out->moff.push_back(out->len.size());
    }
    return true;
}

void report(const char* what, const std::string& wl, const std::string& lib, std::vector<double> ms, uint64_t hash,
            uint64_t matches, const char* extra) {
    std::vector<double> s = ms;
    std::sort(s.begin(), s.end());
    const double med = s[s.size() / 2], spread = s.back() - s.front();
    printf("{\"what\": \"%s\", \"workload\": \"%s\", \"lib\": \"%s\", \"ms\": [", what, wl.c_str(), lib.c_str());
    for (size_t i = 0; i < ms.size(); ++i) printf("%s%.3f", i ? ", " : "", ms[i]);
    printf("], \"median_ms\": %.3f, \"spread_ms\": %.3f, \"matches\": %llu, \"hash\": \"%016llx\"%s}\n", med, spread,
           (unsigned long long)matches, (unsigned long long)hash, extra);
    fflush(stdout);
}

}  // namespace

int main(int argc, char** argv) {
    std::string lib, wl = "w1", mode = "both", oracle;
    int reps = 5;
    for (int i = 1; i < argc; ++i) {
        const std::string k = argv[i];
        if (k == "--lib" && i + 1 < argc) lib = argv[++i];
        else if (k == "--workload" && i + 1 < argc) wl = argv[++i];
        else if (k == "--reps" && i + 1 < argc) reps = atoi(argv[++i]);
        else if (k == "--mode" && i + 1 < argc) mode = argv[++i];
        else if (k == "--oracle" && i + 1 < argc) oracle = argv[++i];
        else { fprintf(stderr, "usage: bench_batch --lib PATH [--workload w1|w2] [--reps N] [--mode loop|batch|both|anchor-loop|anchor-batch|anchor] [--oracle PATH]\n"); return 2; }
    }
    if (lib.empty() || (wl != "w1" && wl != "w2") || reps < 1) { fprintf(stderr, "bench_batch: --lib PATH and --workload w1|w2 required\n"); return 2; }
    void* h = dlopen(lib.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "bench_batch: %s\n", dlerror()); return 2; }
    Api a{};
    bool ok = sym(h, "mums_ctx_create", &a.ctx_create) && sym(h, "mums_ctx_destroy", &a.ctx_destroy) &&
              sym(h, "mums_set_seed", &a.set_seed) && sym(h, "mums_set_params", &a.set_params) &&
              sym(h, "mums_clear", &a.clear) && sym(h, "mums_add_genome", &a.add_genome) && sym(h, "mums_find", &a.find) &&
              sym(h, "mums_result_count", &a.result_count) && sym(h, "mums_result_copy", &a.result_copy) &&
              sym(h, "mums_get_stats", &a.get_stats) && sym(h, "mums_last_error", &a.last_error) &&
              sym(h, "mums_get_seed", &a.get_seed) && sym(h, "mums_default_seed_weight", &a.default_seed_weight);
    sym(h, "mums_find_batch", &a.find_batch, false);
    sym(h, "mums_batch_info", &a.batch_info, false);
    if (!ok) return 2;
    sym(h, "mums_clear_sequences", &a.clear_sequences, false);
    sym(h, "mums_eliminate_overlaps_v2", &a.eliminate_overlaps_v2, false);
    sym(h, "mums_length_filter", &a.length_filter, false);
    sym(h, "mums_anchor_batch", &a.anchor_batch, false);
    sym(h, "mums_anchor_batch_info", &a.anchor_batch_info, false);
    if (mode.rfind("anchor", 0) == 0) {
        const bool a_loop = mode != "anchor-batch", a_batch = mode != "anchor-loop";
        if (a_loop && !(a.clear_sequences && a.eliminate_overlaps_v2 && a.length_filter)) {
            fprintf(stderr, "bench_batch: the library lacks mums_clear_sequences / mums_eliminate_overlaps_v2\n");
            return 2;
        }
        if (a_batch && !(a.anchor_batch && a.anchor_batch_info)) {
            fprintf(stderr, "bench_batch: the library has no mums_anchor_batch\n");
            return 2;
        }
        const Workload w = make_workload(a, wl);
        mums_ctx* ctx = nullptr;
        if (a.ctx_create(0, &ctx) != MUMS_OK) { fprintf(stderr, "bench_batch: no HIP device\n"); return 3; }
        a.set_params(ctx, 0, 1, 40000);
        Lists loop, batch;
        if (a_loop) {
            std::vector<double> ms;
            if (!run_anchor_loop(a, ctx, w, &loop)) return 1;   // warm-up: buffers, code objects
            for (int r = 0; r < reps; ++r) {
                const double t0 = now_ms();
                if (!run_anchor_loop(a, ctx, w, &loop)) return 1;
                ms.push_back(now_ms() - t0);
            }
            report("anchor_loop", wl, lib, ms, loop.hash(), loop.len.size(), "");
        }
        if (a_batch) {
            std::vector<double> ms;
            mums_stats last{};
            if (!run_anchor_batch(a, ctx, w, &batch, &last)) return 1;
            for (int r = 0; r < reps; ++r) {
                const double t0 = now_ms();
                if (!run_anchor_batch(a, ctx, w, &batch, &last)) return 1;
                ms.push_back(now_ms() - t0);
            }
            char extra[320];
            snprintf(extra, sizeof extra,
                     ", \"phase_ms\": {\"upload_keys\": %.3f, \"sort\": %.3f, \"replay\": %.3f, \"single_tail_emit\": %.3f, "
                     "\"pass_total\": %.3f}, \"restarts\": %llu, \"table_entries\": %llu",
                     last.ms_keys, last.ms_sort, last.ms_replay, last.ms_output, last.ms_total,
                     (unsigned long long)last.restarts, (unsigned long long)last.mem_count);
            report("anchor_batch", wl, lib, ms, batch.hash(), batch.len.size(), extra);
        }
        int status = 0;
        if (a_loop && a_batch) {
            const bool eq = loop == batch;
            printf("{\"what\": \"compare\", \"workload\": \"%s\", \"anchor_batch_equals_loop\": %s}\n", wl.c_str(),
                   eq ? "true" : "false");
            if (!eq) status = 1;
        }
        a.ctx_destroy(ctx);
        return status;
    }
    const bool want_loop = mode != "batch", want_batch = mode != "loop";
    if (want_batch && !a.find_batch) {
        if (mode == "batch") { fprintf(stderr, "bench_batch: the library has no mums_find_batch\n"); return 2; }
        fprintf(stderr, "bench_batch: the library has no mums_find_batch, timing the loop only\n");
    }
    const Workload w = make_workload(a, wl);
    mums_ctx* ctx = nullptr;
    if (a.ctx_create(0, &ctx) != MUMS_OK) { fprintf(stderr, "bench_batch: no HIP device\n"); return 3; }
    a.set_params(ctx, 0, 1, 40000);
    Lists loop, batch;
    bool have_loop = false, have_batch = false;
    if (want_loop) {
        std::vector<double> ms;
        if (!run_loop(a, ctx, w, &loop)) return 1;   // warm-up: buffers, code objects
        for (int r = 0; r < reps; ++r) {
            const double t0 = now_ms();
            if (!run_loop(a, ctx, w, &loop)) return 1;
            ms.push_back(now_ms() - t0);
        }
        have_loop = true;
        report("loop", wl, lib, ms, loop.hash(), loop.len.size(), "");
    }
    if (want_batch && a.find_batch) {
        std::vector<double> ms;
        mums_stats ph{}, last{};
        if (!run_batch(a, ctx, w, &batch, &ph)) return 1;
        for (int r = 0; r < reps; ++r) {
            const double t0 = now_ms();
            if (!run_batch(a, ctx, w, &batch, &last)) return 1;
            ms.push_back(now_ms() - t0);
        }
        have_batch = true;
        char extra[256];
        snprintf(extra, sizeof extra,
                 ", \"phase_ms\": {\"upload_keys\": %.3f, \"sort\": %.3f, \"replay\": %.3f, \"single_and_emit\": %.3f, "
                 "\"pass_total\": %.3f}, \"restarts\": %llu",
                 last.ms_keys, last.ms_sort, last.ms_replay, last.ms_output, last.ms_total, (unsigned long long)last.restarts);
        report("batch", wl, lib, ms, batch.hash(), batch.len.size(), extra);
    }
    int status = 0;
    if (have_loop && have_batch) {
        const bool eq = loop == batch;
        printf("{\"what\": \"compare\", \"workload\": \"%s\", \"batch_equals_loop\": %s}\n", wl.c_str(), eq ? "true" : "false");
        if (!eq) status = 1;
    }
    if (!oracle.empty()) {
        void* oh = dlopen(oracle.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!oh) { fprintf(stderr, "bench_batch: %s\n", dlerror()); return 2; }
        decltype(&oracle_find_matches) ofind;
        decltype(&oracle_result_count) ocount;
        decltype(&oracle_result_copy) ocopy;
        decltype(&oracle_result_free) ofree;
        if (!sym(oh, "oracle_find_matches", &ofind) || !sym(oh, "oracle_result_count", &ocount) ||
            !sym(oh, "oracle_result_copy", &ocopy) || !sym(oh, "oracle_result_free", &ofree))
            return 2;
        Lists ref;
        ref.moff.assign(1, 0);
        const double t0 = now_ms();
        for (uint32_t p = 0; p < w.B; ++p) {
            if (w.pattern[p]) {
                const char* seqs[2] = {w.ascii.data() + w.off[2 * p], w.ascii.data() + w.off[2 * p + 1]};
                const uint64_t lens[2] = {w.off[2 * p + 1] - w.off[2 * p], w.off[2 * p + 2] - w.off[2 * p + 1]};
                oracle_params prm{};
                prm.seed = w.pattern[p];
                prm.enum_tol = 1;
                prm.table_size = 40000;
                oracle_result* r = ofind(2, seqs, lens, &prm);
                if (!r) { fprintf(stderr, "bench_batch: the oracle refused problem %u\n", p); return 1; }
                const uint64_t M = ocount(r);
                const size_t l0 = ref.len.size();
                ref.len.resize(l0 + M);
                ref.st.resize((l0 + M) * 2);
                if (M) ocopy(r, ref.len.data() + l0, ref.st.data() + l0 * 2);
                ofree(r);
            }
            ref.moff.push_back(ref.len.size());
        }
        const double t = now_ms() - t0;
        const bool eq = (!have_batch || ref == batch) && (!have_loop || ref == loop);
        printf("{\"what\": \"oracle\", \"workload\": \"%s\", \"threads\": 1, \"ms\": %.3f, \"matches\": %llu, \"hash\": \"%016llx\", "
               "\"equals_gpu\": %s}\n", wl.c_str(), t, (unsigned long long)ref.len.size(), (unsigned long long)ref.hash(),
               eq ? "true" : "false");
        if (!eq) status = 1;
    }
    a.ctx_destroy(ctx);
    return status;
}
