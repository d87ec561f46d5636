// TEST INFRASTRUCTURE ONLY: runs libMems itself on a case file and prints what it computed.
//
// This program is ours; it links the reference's own translation units (oracle/Makefile, target
// `ref`) and calls their public entry points.  tests/golden/make_ref_golden.py records its
// output in tests/golden/ref_cases.json, the fixture that pins the C oracle and the HIP path to
// the reference (tests/test_ref_pinning_cpu.py, tests/test_gpu_ref_pinning.py).
//
//   ref_driver CASE_FILE [OUT_FILE]
//
// Case file: text lines `key value...` up to a line `data`, then the raw sequence bytes of all
// genomes back to back.  Keys:
//   mode       seeds | sml | find | family | recursion | eo1 | eo2 | occurrence | compat
//   finder     memhash | masked | pairwise                      (find, family, recursion)
//   weight W, rank R                                              (sml, find, occurrence, compat)
//   rounds W:R W:R ...   the seed of every round on one table   (family, recursion)
//   nway_only 0|1        recursion without `rounds`: the reference's own weight loop and tail
//   repeat_tol, enum_tol, table_size, mask
//   start_points p0 .. pG-1                                       (FindMatchesFromPosition)
//   match_log 0|1, offset_log 0|1
//   filter mult M | filter len L      applied in the order given, each printed
//   eliminate_both 0|1, seq_ids i j ..                            (eo2, family)
//   row len s0 .. sG-1                                            (eo1, eo2: the input MatchList)
//   G, lengths n0 .. nG-1
// Output: sections `@name count` followed by that many lines; a match is `len\ts0\t..\tsG-1`,
// lists are in GetMatchList order.
#include <omp.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "libMems/DNAMemorySML.h"
#include "libMems/MaskedMemHash.h"
#include "libMems/MatchList.h"
#include "libMems/MemHash.h"
#include "libMems/PairwiseMatchFinder.h"
#include "libMems/ParallelMemHash.h"
#include "libMems/SeedMasks.h"
#include "libMems/SeedOccurrenceList.h"

// The two overlap eliminators, as line ranges of the reference files (oracle/Makefile writes
// them at build time; neither file compiles whole here).
using namespace std;
using namespace genome;
namespace mems {
#include "min_anchor_length.inc"
#include "eo1_extract.inc"
#include "eo2_extract.inc"
}

using namespace mems;

namespace {

struct Case {
	map<string, vector<string> > kv;
	vector<pair<string, string> > filters;
	vector<vector<long long> > rows;
	vector<string> seqs;

	bool has(const string& k) const { return kv.count(k) != 0; }
	string str(const string& k, const string& def = "") const {
		map<string, vector<string> >::const_iterator it = kv.find(k);
		return it == kv.end() || it->second.empty() ? def : it->second[0];
	}
	long long num(const string& k, long long def = 0) const {
		string s = str(k);
		return s.empty() ? def : strtoll(s.c_str(), NULL, 0);
	}
	vector<long long> nums(const string& k) const {
		vector<long long> out;
		map<string, vector<string> >::const_iterator it = kv.find(k);
		if (it != kv.end())
			for (size_t i = 0; i < it->second.size(); i++)
				out.push_back(strtoll(it->second[i].c_str(), NULL, 0));
		return out;
	}
};

void fail(const string& msg) {
	cerr << "ref_driver: " << msg << endl;
	exit(2);
}

Case read_case(const char* path) {
	ifstream in(path, ios::binary);
	if (!in.is_open())
		fail(string("cannot open ") + path);
	Case c;
	string line;
	bool data = false;
	while (getline(in, line)) {
		if (line == "data") {
			data = true;
			break;
		}
		istringstream ls(line);
		string key, tok;
		if (!(ls >> key) || key[0] == '#')
			continue;
		vector<string> vals;
		while (ls >> tok)
			vals.push_back(tok);
		if (key == "filter") {
			if (vals.size() != 2)
				fail("filter takes a kind and a value");
			c.filters.push_back(make_pair(vals[0], vals[1]));
		} else if (key == "row") {
			vector<long long> r;
			for (size_t i = 0; i < vals.size(); i++)
				r.push_back(strtoll(vals[i].c_str(), NULL, 10));
			c.rows.push_back(r);
		} else
			c.kv[key] = vals;
	}
	vector<long long> lens = c.nums("lengths");
	if ((long long)lens.size() != c.num("G"))
		fail("lengths does not list G values");
	if (!data && !lens.empty())
		fail("no data section");
	for (size_t g = 0; g < lens.size(); g++) {
		string s((size_t)lens[g], '\0');
		in.read(&s[0], lens[g]);
		if (in.gcount() != lens[g])
			fail("data section is short");
		c.seqs.push_back(s);
	}
	return c;
}

ostream* out = &cout;

void print_list(const string& name, const MatchList& ml) {
	*out << '@' << name << ' ' << ml.size() << '\n';
	for (size_t i = 0; i < ml.size(); i++)
		*out << *ml[i] << '\n';
}

void print_text(const string& name, const string& text) {
	size_t n = 0;
	for (size_t i = 0; i < text.size(); i++)
		n += text[i] == '\n';
	*out << '@' << name << ' ' << n << '\n' << text;
}

void apply_filters(const Case& c, MatchList& ml) {
	for (size_t f = 0; f < c.filters.size(); f++) {
		long long v = strtoll(c.filters[f].second.c_str(), NULL, 10);
		if (c.filters[f].first == "mult")
			ml.MultiplicityFilter((unsigned)v);
		else if (c.filters[f].first == "len")
			ml.LengthFilter((gnSeqI)v);
		else
			fail("unknown filter " + c.filters[f].first);
		print_list("filter_" + c.filters[f].first + "_" + c.filters[f].second, ml);
	}
}

void free_matches(MatchList& ml) {
	for (size_t i = 0; i < ml.size(); i++)
		ml[i]->Free();
	ml.clear();
}

void fill_tables(const Case& c, MatchList& ml) {
	for (size_t g = 0; g < c.seqs.size(); g++) {
		ostringstream name;
		name << "seq" << g;
		ml.seq_filename.push_back(name.str());
		ml.seq_table.push_back(new gnSequence(c.seqs[g]));
		ml.sml_table.push_back(new DNAMemorySML());
	}
}

void create_smls(MatchList& ml, uint64 seed) {
	for (size_t g = 0; g < ml.sml_table.size(); g++) {
		ml.sml_table[g]->Clear();
		ml.sml_table[g]->Create(*ml.seq_table[g], seed);
	}
}

void release_tables(MatchList& ml) {
	for (size_t g = 0; g < ml.seq_table.size(); g++) {
		delete ml.seq_table[g];
		delete ml.sml_table[g];
	}
	ml.seq_table.clear();
	ml.sml_table.clear();
}

MemHash* new_finder(const Case& c) {
	string kind = c.str("finder", "memhash");
	MemHash* mh;
	if (kind == "memhash")
		mh = new MemHash();
	else if (kind == "masked") {
		MaskedMemHash* m = new MaskedMemHash();
		m->SetMask((uint64)c.num("mask"));
		mh = m;
	} else if (kind == "pairwise")
		mh = new PairwiseMatchFinder();
	else if (kind == "parallel")
		mh = new ParallelMemHash();
	else {
		fail("unknown finder " + kind);
		return NULL;
	}
	if (c.has("table_size"))
		mh->SetTableSize((uint32)c.num("table_size"));
	mh->SetRepeatTolerance((uint32)c.num("repeat_tol", DEFAULT_REPEAT_TOLERANCE));
	mh->SetEnumerationTolerance((uint32)c.num("enum_tol", DEFAULT_ENUMERATION_TOLERANCE));
	return mh;
}

void print_counters(MemHash& mh) {
	*out << "@counters 2\n";
	*out << "mem_count " << mh.MemCount() << '\n';
	*out << "collision_count " << mh.MemCollisionCount() << '\n';
}

void mode_seeds() {
	ostringstream t;
	for (int w = 1; w <= 33; w++)
		for (int r = 0; r <= 2; r++) {
			int64 s = getSeed(w, r);
			t << w << '\t' << r << '\t' << (uint64)s << '\t' << getSeedLength(s) << '\t' << getSeedWeight(s) << '\n';
		}
	print_text("seeds", t.str());
	ostringstream d;
	for (uint64 n = 0; n <= 64; n++)
		d << n << '\t' << getDefaultSeedWeight(n) << '\n';
	for (int e = 7; e <= 40; e++)
		for (int k = -1; k <= 1; k++) {
			uint64 n = ((uint64)1 << e) + k;
			d << n << '\t' << getDefaultSeedWeight(n) << '\n';
		}
	for (uint64 n = 100; n <= 10000000000ull; n *= 10)
		for (uint64 m = 1; m <= 9; m += 2)
			d << n * m << '\t' << getDefaultSeedWeight(n * m) << '\n';
	print_text("default_weight", d.str());
}

void mode_sml(const Case& c) {
	uint64 seed = (uint64)getSeed((int)c.num("weight"), (int)c.num("rank"));
	for (size_t g = 0; g < c.seqs.size(); g++) {
		gnSequence seq(c.seqs[g]);
		DNAMemorySML sml;
		sml.Create(seq, seed);
		ostringstream name;
		name << "sml" << g;
		*out << '@' << name.str() << ' ' << sml.SMLLength() << '\n';
		for (gnSeqI i = 0; i < sml.SMLLength(); i++) {
			bmer b = sml[i];
			*out << b.position << '\t' << (uint64)b.mer << '\n';
		}
	}
}

void mode_occurrence(const Case& c) {
	uint64 seed = (uint64)getSeed((int)c.num("weight"), (int)c.num("rank"));
	for (size_t g = 0; g < c.seqs.size(); g++) {
		gnSequence seq(c.seqs[g]);
		DNAMemorySML sml;
		sml.Create(seq, seed);
		SeedOccurrenceList sol;
		sol.construct(sml);
		ostringstream name;
		name << "occurrence" << g;
		*out << '@' << name.str() << ' ' << c.seqs[g].size() << '\n';
		for (size_t i = 0; i < c.seqs[g].size(); i++) {
			float f = sol.getFrequency(i);
			uint32 bits;
			memcpy(&bits, &f, sizeof bits);
			*out << bits << '\n';
		}
	}
}

// MemHash / MaskedMemHash / PairwiseMatchFinder / ParallelMemHash: FindMatches or
// FindMatchesFromPosition, with the logs, then the filters.
void mode_find(const Case& c) {
	MatchList ml;
	fill_tables(c, ml);
	create_smls(ml, (uint64)getSeed((int)c.num("weight"), (int)c.num("rank")));
	MemHash* mh = new_finder(c);
	ostringstream match_log, offset_log;
	if (c.num("match_log"))
		mh->SetMatchLog(&match_log);
	if (c.num("offset_log"))
		mh->SetOffsetLog(&offset_log);
	if (c.has("start_points")) {
		vector<long long> sp = c.nums("start_points");
		vector<gnSeqI> start_points(sp.begin(), sp.end());
		mh->FindMatchesFromPosition(ml, start_points);
	} else
		mh->FindMatches(ml);
	print_list("list", ml);
	print_counters(*mh);
	if (c.num("offset_log"))
		print_text("offset_log", offset_log.str());
	if (c.num("match_log"))
		print_text("match_log", match_log.str());
	apply_filters(c, ml);
	free_matches(ml);
	release_tables(ml);
	delete mh;
}

// The searches of pairwiseAnchorSearch (ProgressiveAligner.cpp:615-659) and of the gap search in
// Aligner::Recursion (Aligner.cpp:1178-1220): several seeds on one table, each round a fresh
// SML per sequence, ClearSequences, FindMatches into a list that is freed; the table's list is
// fetched once at the end.  The list is printed after every round and after each tail step.
void mode_rounds(const Case& c, bool family) {
	MatchList gap_list;
	fill_tables(c, gap_list);
	MemHash* mh = new_finder(c);
	vector<string> rounds;
	if (c.has("rounds"))
		rounds = c.kv.find("rounds")->second;
	else if (family) {
		if (c.seqs.size() != 2)
			fail("family takes two sequences unless it is given its rounds");
		gnSeqI avg_len = (c.seqs[0].size() + c.seqs[1].size()) / 2;   // ProgressiveAligner.cpp:615
		uint w = getDefaultSeedWeight(avg_len);
		for (int r = 0; r < 3; r++) {
			ostringstream t;
			t << w << ':' << r;
			rounds.push_back(t.str());
		}
	}
	mh->Clear();
	if (c.has("table_size"))
		mh->SetTableSize((uint32)c.num("table_size"));
	bool searched = true;
	for (size_t r = 0; r < rounds.size(); r++) {
		int w = 0, rank = 0;
		if (sscanf(rounds[r].c_str(), "%d:%d", &w, &rank) != 2)
			fail("round is not W:R");
		if ((uint)w < MIN_DNA_SEED_WEIGHT) {
			searched = false;
			break;
		}
		create_smls(gap_list, (uint64)getSeed(w, rank));
		mh->ClearSequences();
		MatchList cur_list = gap_list;
		cur_list.clear();
		mh->FindMatches(cur_list);
		ostringstream name;
		name << "round" << r;
		print_list(name.str(), cur_list);
		free_matches(cur_list);
	}
	if (searched) {
		mh->GetMatchList(gap_list);
		print_list("table", gap_list);
		print_counters(*mh);
		if (family) {
			if (c.has("seq_ids")) {
				vector<long long> ids = c.nums("seq_ids");
				vector<uint> seq_ids(ids.begin(), ids.end());
				EliminateOverlaps_v2(gap_list, seq_ids, c.num("eliminate_both") != 0);
			} else
				EliminateOverlaps_v2(gap_list, c.num("eliminate_both") != 0);
		} else
			EliminateOverlaps(gap_list);
		print_list("overlaps", gap_list);
		apply_filters(c, gap_list);
	}
	free_matches(gap_list);
	release_tables(gap_list);
	delete mh;
}

// The gap search of Aligner::Recursion as the reference wrote it, weight loop included: the two
// line ranges of Aligner.cpp run on the names they use there.  gap_mh is the MemHash of
// Aligner.h:197, nway_mh the MaskedMemHash of :198 with the mask Aligner.cpp:2208-2212 gives it.
void mode_recursion_literal(const Case& c) {
	const bool nway_only = c.num("nway_only") != 0;
	uint seq_count = (uint)c.seqs.size();
	uint seqI = 0;
	MatchList gap_list;
	fill_tables(c, gap_list);
	TLS<MemHash> gap_mh;
	MaskedMemHash nway_mh;
	uint64 nway_mask = 1;
	nway_mask <<= seq_count;
	nway_mask--;
	nway_mh.SetMask(nway_mask);
#include "recursion_search.inc"
	print_list("table", gap_list);
	print_counters(nway_only ? (MemHash&)nway_mh : gap_mh.get());
#include "recursion_tail.inc"
	print_list("final", gap_list);
	free_matches(gap_list);
	release_tables(gap_list);
}

void mode_eo(const Case& c, bool v2) {
	MatchList ml;
	uint G = (uint)c.num("G");
	for (size_t i = 0; i < c.rows.size(); i++) {
		if (c.rows[i].size() != G + 1)
			fail("row does not hold a length and G starts");
		Match m(G);
		for (uint g = 0; g < G; g++)
			m.SetStart(g, c.rows[i][g + 1]);
		m.SetLength((gnSeqI)c.rows[i][0]);
		ml.push_back(m.Copy());
	}
	if (!v2)
		EliminateOverlaps(ml);
	else if (c.has("seq_ids")) {
		vector<long long> ids = c.nums("seq_ids");
		vector<uint> seq_ids(ids.begin(), ids.end());
		EliminateOverlaps_v2(ml, seq_ids, c.num("eliminate_both") != 0);
	} else
		EliminateOverlaps_v2(ml, c.num("eliminate_both") != 0);
	print_list("overlaps", ml);
	apply_filters(c, ml);
	free_matches(ml);
}

}  // namespace

int main(int argc, char** argv) {
	if (argc < 2)
		fail("usage: ref_driver CASE_FILE [OUT_FILE]");
	// One thread: ParallelMemHash's chunks then run in order, and nothing races on its counters.
	omp_set_num_threads(1);
	Case c = read_case(argv[1]);
	ostringstream buf;
	out = &buf;
	string mode = c.str("mode");
	try {
		if (mode == "seeds")
			mode_seeds();
		else if (mode == "sml")
			mode_sml(c);
		else if (mode == "occurrence")
			mode_occurrence(c);
		else if (mode == "find" || mode == "compat")
			mode_find(c);
		else if (mode == "recursion" && !c.has("rounds"))
			mode_recursion_literal(c);
		else if (mode == "family" || mode == "recursion")
			mode_rounds(c, mode == "family");
		else if (mode == "eo1" || mode == "eo2")
			mode_eo(c, mode == "eo2");
		else
			fail("unknown mode " + mode);
	} catch (gnException& e) {
		fail(string("libMems threw ") + e.what());
	}
	if (argc > 2) {
		ofstream f(argv[2], ios::binary);
		f << buf.str();
		if (!f.good())
			fail(string("cannot write ") + argv[2]);
	} else
		cout << buf.str();
	return 0;
}
