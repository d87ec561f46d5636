// mums_find.cpp -- C++ host driver over include/mums_memhash.hpp (the reference-language
// host path).  Generates the SURVEY Appendix-C synthetic genomes (std::mt19937_64) or reads
// one raw/FASTA sequence per file, runs mums::MemHash / MaskedMemHash on the GPU and prints
// the MatchList text (UngappedLocalAlignment.h:200-206), one match per line.
//   mums_find gen G n weight p [mask]        (mask > 0 selects MaskedMemHash)
//   mums_find files weight f1 f2 ...
//   mums_find sml G n weight p [mask]        the drop-in path of Aligner.cpp:1181-1184 /
//       CreateMemorySMLs (MatchList.h:409-435): HipSML::Create per genome (deferred), then
//       MemHash::FindMatches from ml.sml_table; stderr reports the SMLs materialised (0)
//   mums_find family G n weight p            progressiveMauve's seed family: Clear, then seed ranks
//       0-2 each ClearSequences + FindMatches on one MemHash (ProgressiveAligner.cpp:619-653)
//   mums_find batch B n p [mask]             B problems of two sequences (lengths n / (k + 1), the
//       Appendix-C generator seeded per problem): "# problem k" + its MatchList text, first from
//       MemHash::FindMatchesBatch (default seeds), then after "== loop" from a loop of
//       Clear + FindMatches with the same seeds on the same object
//   mums_find anchor B n p | anchor files a0 b0 a1 b1 ...   B gap problems as in `batch`, or one per pair of
//       files: "# problem k" + its anchor list,
//       first from MemHash::AnchorSearchBatch (seed families, default weights), then after "== loop"
//       from the loop of pairwiseAnchorSearch (Clear; per rank ClearSequences + FindMatches;
//       EliminateOverlaps_v2; LengthFilter(12)) on the same object, then after "== tail" from
//       AnchorTailBatch over the problems' family tables
//   mums_find recursion files G nway weights f0_0 .. f0_G-1 f1_0 ...   one gap problem of Aligner::Recursion
//       per G files; nway: 0 / 1 (nway_only); weights: w0,w1,...,wG-1 for every problem's sequences or
//       "default" (getDefaultSeedWeight of each length).  "# problem k" + its list, first from
//       MemHash::RecursionBatch, then after "== loop" from the loop of Recursion's calls (Clear; per
//       round ClearSequences + FindMatches; EliminateOverlaps; MultiplicityFilter when nway;
//       LengthFilter(9)) on the same object, then after "== tail" from RecursionTailBatch over the
//       problems' tables
//   mums_find smldump G n weight p g stride  genome g's deferred SML read back: every entry
//       (position, mer) through operator[], then FindMer of every stride-th entry's mer
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>

#include "mums_memhash.hpp"

static std::vector<std::string> generate(int G, uint64_t n, double p, uint64_t seed) {
    std::mt19937_64 rng(seed);
    const char* acgt = "ACGT";
    std::vector<std::string> g(G);
    g[0].resize(n);
    for (uint64_t i = 0; i < n; ++i) g[0][i] = acgt[rng() & 3];
    for (int k = 1; k < G; ++k) {
        g[k] = g[0];
        for (uint64_t i = 0; i < n; ++i)
            if ((rng() % 1000000) < p * 1e6) g[k][i] = acgt[rng() & 3];
        if (k == 2) {
            std::string r(g[k].rbegin(), g[k].rend());
            for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
            g[k] = r;
        }
    }
    return g;
}

static std::string read_seq(const std::string& path) {
    std::ifstream f(path);
    std::string line, s;
    while (std::getline(f, line)) {
        if (!line.empty() && line[0] == '>') continue;
        for (char c : line)
            if (c != '\n' && c != '\r' && c != ' ') s.push_back(c);
    }
    return s;
}

int main(int argc, char** argv) {
    int gpus = 0;        // --gpus N: ShardedMemHash over devices 0..N-1 (RCCL); --local N: one GPU, N ranks
    bool local = false, slices = false;   // --slices: position slices per rank (else genome blocks)
    if (argc > 2 && (std::string(argv[1]) == "--gpus" || std::string(argv[1]) == "--local")) {
        local = std::string(argv[1]) == "--local";
        gpus = atoi(argv[2]);
        argv += 2;
        argc -= 2;
        if (argc > 1 && std::string(argv[1]) == "--slices") {
            slices = true;
            ++argv;
            --argc;
        }
    }
    uint64_t compat_chunk = 0;   // --compat CHUNK: ParallelMemHash (CHUNK_SIZE = CHUNK)
    if (argc > 2 && std::string(argv[1]) == "--compat") {
        compat_chunk = strtoull(argv[2], nullptr, 10);
        argv += 2;
        argc -= 2;
    }
    if (argc < 3) {
        std::cerr << "usage: mums_find [--gpus N | --local N] [--slices] [--compat CHUNK] gen G n weight p [mask] | "
                     "files weight f1 f2 ...\n";
        return 2;
    }
    std::string mode = argv[1];
    if ((mode == "sml" || mode == "smldump") && argc >= 6) {
        const int G = atoi(argv[2]);
        const uint64_t n = strtoull(argv[3], nullptr, 10);
        const int weight = atoi(argv[4]);
        const double p = atof(argv[5]);
        try {
            mums::MatchList ml;
            ml.seq_table = generate(G, n, p, 12345);
            auto t0 = std::chrono::steady_clock::now();
            ml.CreateMemorySMLs((uint32_t)weight);   // Create per genome: no keys, no sort
            auto t1 = std::chrono::steady_clock::now();
            if (mode == "smldump") {
                const uint32_t g = argc > 6 ? (uint32_t)atoi(argv[6]) : 0;
                const uint64_t stride = argc > 7 ? strtoull(argv[7], nullptr, 10) : 1000;
                mums::HipSML& sml = *ml.sml_table.at(g);
                std::ostringstream os;
                const uint64_t m = sml.SMLLength();
                for (uint64_t i = 0; i < m; ++i) {
                    const mums::bmer b = sml[i];
                    os << b.position << '\t' << b.mer << '\n';
                }
                for (uint64_t i = 0; i < m; i += stride) {   // FindMer (SortedMerList.cpp:170-179)
                    uint64_t r = 0;
                    const bool f = sml.FindMer(sml[i].mer, r);
                    os << "find\t" << i << '\t' << f << '\t' << r << '\n';
                }
                std::vector<mums::bmer> rv;   // MemorySML::Read past the end returns false
                const bool ok = sml.Read(rv, 10, m > 5 ? m - 5 : 0);
                os << "read\t" << ok << '\t' << rv.size() << '\n';
                std::cout << os.str();
                std::cerr << "sml length " << m << " materialized " << mums::HipSML::Materializations() << "\n";
                return 0;
            }
            mums::MaskedMemHash mh(0);
            const uint64_t mask = argc > 6 ? strtoull(argv[6], nullptr, 0) : 0;
            if (mask) mh.SetMask(mask);
            else mums_set_mask(mh.handle(), 0, 0);
            mh.FindMatches(ml);   // genomes and seed pattern from ml.sml_table
            auto t2 = std::chrono::steady_clock::now();
            std::ostringstream os;
            for (const auto& m : ml) os << m << '\n';
            std::cout << os.str();
            std::cerr << "matches " << ml.size() << " create ms "
                      << std::chrono::duration<double, std::milli>(t1 - t0).count() << " find ms "
                      << std::chrono::duration<double, std::milli>(t2 - t1).count() << " materialized "
                      << mums::HipSML::Materializations() << "\n";
        } catch (const std::exception& e) {
            std::cerr << "error: " << e.what() << "\n";
            return 1;
        }
        return 0;
    }
    if (mode == "batch" && argc >= 5) {
        const int B = atoi(argv[2]);
        const uint64_t n = strtoull(argv[3], nullptr, 10);
        const double p = atof(argv[4]);
        const uint64_t mask = argc > 5 ? strtoull(argv[5], nullptr, 0) : 0;
        try {
            std::vector<std::vector<std::string>> problems;
            for (int k = 0; k < B; ++k) problems.push_back(generate(2, n / (uint64_t)(k + 1), p, 12345 + (uint64_t)k));
            std::unique_ptr<mums::MemHash> mh;
            if (mask) {
                auto* m = new mums::MaskedMemHash(0);
                m->SetMask(mask);
                mh.reset(m);
            } else {
                mh.reset(new mums::MemHash(0));
            }
            std::vector<mums::MatchList> lists;
            mh->FindMatchesBatch(problems, lists);
            std::ostringstream os;
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                for (const auto& m : lists[k]) os << m << '\n';
            }
            os << "== loop\n";
            uint64_t probes = 0;
            for (uint64_t v : mh->BatchInfo().probes) probes += v;
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                const uint32_t w = mums_default_seed_weight((problems[k][0].size() + problems[k][1].size()) / 2);
                if (!w) continue;
                mh->Clear();
                mh->SetSeed((uint64_t)mums_get_seed((int)w, 0));
                mums::MatchList ml;
                ml.seq_table = problems[k];
                mh->FindMatches(ml);
                for (const auto& m : ml) os << m << '\n';
            }
            std::cout << os.str();
            std::cerr << "problems " << B << " probes " << probes << "\n";
        } catch (const std::exception& e) {
            std::cerr << "error: " << e.what() << "\n";
            return 1;
        }
        return 0;
    }
    if (mode == "anchor" && argc >= 5) {
        const bool files = std::string(argv[2]) == "files";   // anchor files a0 b0 a1 b1 ...: one problem per pair
        const int B = files ? (argc - 3) / 2 : atoi(argv[2]);
        const uint64_t n = files ? 0 : strtoull(argv[3], nullptr, 10);
        const double p = files ? 0 : atof(argv[4]);
        try {
            std::vector<std::vector<std::string>> problems;
            for (int k = 0; k < B; ++k) {
                if (files) problems.push_back({read_seq(argv[3 + 2 * k]), read_seq(argv[4 + 2 * k])});
                else problems.push_back(generate(2, n / (uint64_t)(k + 1), p, 12345 + (uint64_t)k));
            }
            mums::MemHash mh(0);
            std::vector<mums::MatchList> lists, tables((size_t)B), tails;
            mh.AnchorSearchBatch(problems, lists);
            std::ostringstream os;
            uint64_t entries = 0;
            for (uint64_t v : mh.AnchorBatchInfo().table_entries) entries += v;
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                for (const auto& m : lists[k]) os << m << '\n';
            }
            os << "== loop\n";
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                const uint32_t w = mums_default_seed_weight((problems[k][0].size() + problems[k][1].size()) / 2);
                if (!w) continue;
                mh.Clear();
                mums::MatchList ml;
                for (int seed_rank = 0; seed_rank < 3; ++seed_rank) {
                    mh.ClearSequences();
                    mh.SetSeed((uint64_t)mums_get_seed((int)w, seed_rank));
                    ml.clear();
                    ml.seq_table = problems[k];
                    mh.FindMatches(ml);
                }
                mh.GetMatchList(tables[(size_t)k]);
                mh.EliminateOverlaps_v2(false);
                mh.LengthFilter(12);
                mh.GetMatchList(ml);
                for (const auto& m : ml) os << m << '\n';
            }
            os << "== tail\n";
            mh.AnchorTailBatch(tables, 2, tails);
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                for (const auto& m : tails[k]) os << m << '\n';
            }
            std::cout << os.str();
            std::cerr << "problems " << B << " table entries " << entries << "\n";
        } catch (const std::exception& e) {
            std::cerr << "error: " << e.what() << "\n";
            return 1;
        }
        return 0;
    }
    if (mode == "recursion" && argc >= 7 && std::string(argv[2]) == "files") {
        const int G = atoi(argv[3]);
        const bool nway = atoi(argv[4]) != 0;
        const std::string wspec = argv[5];
        if (G < 2 || (argc - 6) % G != 0) {
            std::cerr << "error: recursion files G nway weights, then G files per problem\n";
            return 2;
        }
        const int B = (argc - 6) / G;
        try {
            std::vector<std::vector<std::string>> problems((size_t)B);
            for (int k = 0; k < B; ++k)
                for (int g = 0; g < G; ++g) problems[(size_t)k].push_back(read_seq(argv[6 + k * G + g]));
            std::vector<std::vector<uint32_t>> weights((size_t)B);
            for (int k = 0; k < B; ++k) {
                if (wspec == "default") {
                    for (const std::string& q : problems[(size_t)k]) weights[(size_t)k].push_back(mums_default_seed_weight(q.size()));
                } else {
                    std::stringstream ws(wspec);
                    std::string tok;
                    while (std::getline(ws, tok, ',')) weights[(size_t)k].push_back((uint32_t)atoi(tok.c_str()));
                }
            }
            mums::MemHash mh(0);
            std::vector<mums::MatchList> lists, tables((size_t)B), tails;
            mh.RecursionBatch(problems, lists, nway, 9, weights);
            std::ostringstream os;
            uint64_t entries = 0;
            for (uint64_t v : mh.AnchorBatchInfo().table_entries) entries += v;
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                for (const auto& m : lists[(size_t)k]) os << m << '\n';
            }
            os << "== loop\n";
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                const std::vector<uint32_t> rounds = mums::MemHash::recursion_rounds(weights[(size_t)k], nway);
                if (rounds.empty()) continue;
                mh.Clear();
                mums::MatchList ml;
                for (uint32_t w : rounds) {
                    mh.ClearSequences();
                    mh.SetSeed((uint64_t)mums_get_seed((int)w, 0));
                    ml.clear();
                    ml.seq_table = problems[(size_t)k];
                    mh.FindMatches(ml);
                }
                mh.GetMatchList(tables[(size_t)k]);
                mh.EliminateOverlaps();
                if (nway) mh.MultiplicityFilter((unsigned)G);
                mh.LengthFilter(9);
                mh.GetMatchList(ml);
                for (const auto& m : ml) os << m << '\n';
            }
            os << "== tail\n";
            mh.RecursionTailBatch(tables, (uint32_t)G, tails, nway ? (uint32_t)G : 0, 9);
            for (int k = 0; k < B; ++k) {
                os << "# problem " << k << '\n';
                for (const auto& m : tails[(size_t)k]) os << m << '\n';
            }
            std::cout << os.str();
            std::cerr << "problems " << B << " table entries " << entries << "\n";
        } catch (const std::exception& e) {
            std::cerr << "error: " << e.what() << "\n";
            return 1;
        }
        return 0;
    }
    if (mode == "family" && argc >= 6) {
        // pairwiseAnchorSearch's seed-family loop (ProgressiveAligner.cpp:619-653): Clear, then per
        // seed rank ClearSequences + FindMatches on the one MemHash; the MatchList is the whole table
        const int G = atoi(argv[2]);
        const uint64_t n = strtoull(argv[3], nullptr, 10);
        const int weight = atoi(argv[4]);
        const double p = atof(argv[5]);
        try {
            const std::vector<std::string> seq_table = generate(G, n, p, 12345);
            mums::MemHash gap_mh(0);
            mums::MatchList ml;
            gap_mh.Clear();
            for (int seed_rank = 0; seed_rank < 3; ++seed_rank) {
                gap_mh.ClearSequences();
                gap_mh.SetSeed((uint64_t)mums_get_seed(weight, seed_rank));
                ml.clear();
                ml.seq_table = seq_table;
                gap_mh.FindMatches(ml);
            }
            ml.clear();
            gap_mh.GetMatchList(ml);
            std::ostringstream os;
            for (const auto& m : ml) os << m << '\n';
            std::cout << os.str();
            std::cerr << "matches " << ml.size() << " mems " << gap_mh.MemCount() << " collisions "
                      << gap_mh.MemCollisionCount() << "\n";
        } catch (const std::exception& e) {
            std::cerr << "error: " << e.what() << "\n";
            return 1;
        }
        return 0;
    }
    std::vector<std::string> seqs;
    int weight = 0;
    uint64_t mask = 0;
    if (mode == "gen") {
        int G = atoi(argv[2]);
        uint64_t n = strtoull(argv[3], nullptr, 10);
        weight = atoi(argv[4]);
        double p = atof(argv[5]);
        if (argc > 6) mask = strtoull(argv[6], nullptr, 0);
        seqs = generate(G, n, p, 12345);
    } else {
        weight = atoi(argv[2]);
        for (int i = 3; i < argc; ++i) seqs.push_back(read_seq(argv[i]));
    }
    if (gpus > 0) {
        try {
            std::vector<int> devs(gpus, 0);
            for (int r = 0; r < gpus; ++r) devs[r] = local ? 0 : r;
            // RCCL prints its version banner on stdout during communicator setup: keep the
            // MatchList alone on stdout
            std::fflush(stdout);
            const int saved = dup(1);
            dup2(2, 1);
            mums::ShardedMemHash sh(devs, local, slices);
            std::fflush(stdout);
            dup2(saved, 1);
            close(saved);
            sh.SetSeed(weight ? (uint64_t)mums_get_seed(weight, 0) : 0);
            if (compat_chunk) sh.SetParallelCompat(true, compat_chunk);
            for (const auto& s : seqs) sh.AddSequence(s);
            mums::MatchList ml;
            auto t0 = std::chrono::steady_clock::now();
            sh.FindMatches(ml);
            auto t1 = std::chrono::steady_clock::now();
            std::ostringstream os;
            for (const auto& m : ml) os << m << '\n';
            std::cout << os.str();
            std::cerr << "matches " << ml.size() << " ranks " << gpus << " ms "
                      << std::chrono::duration<double, std::milli>(t1 - t0).count() << "\n";
        } catch (const std::exception& e) {
            std::cerr << "error: " << e.what() << "\n";
            return 1;
        }
        return 0;
    }
    try {
        mums::MaskedMemHash mh(0);   // mask 0 behaves exactly like MemHash
        if (compat_chunk && mums_set_parallel_compat(mh.handle(), 1, compat_chunk) != MUMS_OK)
            throw mums::InvalidData(mums_last_error(mh.handle()));
        if (mask) mh.SetMask(mask);
        else mums_set_mask(mh.handle(), 0, 0);
        mh.SetSeed(weight ? (uint64_t)mums_get_seed(weight, 0) : 0);
        mums::MatchList ml;
        ml.seq_table = seqs;
        auto t0 = std::chrono::steady_clock::now();
        mh.FindMatches(ml);
        auto t1 = std::chrono::steady_clock::now();
        std::ostringstream os;
        for (const auto& m : ml) os << m << '\n';
        std::cout << os.str();
        auto st = mh.stats();
        std::cerr << "matches " << ml.size() << " collisions " << st.collision_count << " ms "
                  << std::chrono::duration<double, std::milli>(t1 - t0).count() << "\n";
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
