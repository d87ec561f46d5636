"""The HIP path against answers recorded from libMems itself (tests/golden/ref_cases.json).

Every case of tests/ref_cases.py runs through the Python classes of libmems_amd -- MemHash,
MaskedMemHash, PairwiseMatchFinder, ParallelMemHash, FindMatchesFromPosition, the tolerances, the
table size, ClearSequences seed families, the filters, EliminateOverlaps (v1 and v2) on loaded
lists, SeedOccurrence, SortedMerList and SeedKeys, AnchorSearchBatch and RecursionBatch -- and is
compared bit for bit with what the reference printed: the list in GetMatchList order, MemCount,
the collision count, the offset log, the match log, the float32 bit patterns.  Only the fixtures
and the seeded generators are read; neither the oracle's answer nor a tolerance comes into it."""
import numpy as np
import pytest

import ref_cases as rc

pytestmark = pytest.mark.gpu

NAMES = list(rc.CASES)
SINGLE = [n for n in NAMES if rc.CASES[n]["mode"] not in ("family", "recursion")]
FAMILY = [n for n in NAMES if rc.CASES[n]["mode"] == "family"]
RECURSION = [n for n in NAMES if rc.CASES[n]["mode"] == "recursion" and not rc.CASES[n].get("whole")]
WHOLE = [n for n in NAMES if rc.CASES[n].get("whole")]


def lines(ml):
    return rc.lines_of(ml.lengths, ml.starts)


def make_finder(lm, c):
    kind = c.get("finder", "memhash")
    mh = {"memhash": lm.MemHash, "masked": lm.MaskedMemHash, "pairwise": lm.PairwiseMatchFinder,
          "parallel": lm.ParallelMemHash}[kind](0)
    if kind == "masked":
        mh.SetMask(c["mask"])
    if "table_size" in c:
        mh.SetTableSize(c["table_size"])
    mh.SetRepeatTolerance(c.get("repeat_tol", 0))
    mh.SetEnumerationTolerance(c.get("enum_tol", 1))
    return mh


def device_filters(c, out, mh):
    for kind, v in c.get("filters", ()):
        (mh.MultiplicityFilter if kind == "mult" else mh.LengthFilter)(v)
        out[f"filter_{kind}_{v}"] = lines(mh.GetMatchList())


def seeds_sections(lm):
    seeds = []
    for w in range(1, 34):
        for r in range(3):
            s = lm.getSeed(w, r)
            seeds.append(f"{w}\t{r}\t{s}\t{lm.getSeedLength(s)}\t{lm.getSeedWeight(s)}")
    ns = list(range(65)) + [(1 << e) + k for e in range(7, 41) for k in (-1, 0, 1)]
    n = 100
    while n <= 10_000_000_000:
        ns += [n * m for m in (1, 3, 5, 7, 9)]
        n *= 10
    return dict(seeds=seeds, default_weight=[f"{n}\t{lm.getDefaultSeedWeight(n)}" for n in ns])


def rounds_of(lm, name):
    c, seqs = rc.CASES[name], rc.case_seqs(name)
    if c["mode"] == "family":
        w = lm.getDefaultSeedWeight((len(seqs[0]) + len(seqs[1])) // 2)   # ProgressiveAligner.cpp:615
        return [(w, r) for r in range(3)]
    if c.get("whole"):   # the package's restatement of the weight loop, Aligner.cpp:1142-1177
        return [(w, 0) for w in lm.recursion_rounds([len(s) for s in seqs], c["nway_only"])]
    return rc.case_rounds(name)


def gpu_sections(lm, name):
    c = rc.CASES[name]
    mode, seqs = c["mode"], list(rc.case_seqs(name))
    if mode == "seeds":
        return seeds_sections(lm)
    out = {}
    if mode in ("sml", "occurrence"):
        seed = lm.getSeed(c["weight"], c["rank"])
        with lm.MemHash(0) as mh:
            mh.SetSeed(seed)
            for s in seqs:
                mh.AddSequence(s)
            mh.FindStage(lm.STAGE_SEEDS)
            for g, s in enumerate(seqs):
                if mode == "occurrence":
                    out[f"occurrence{g}"] = [str(int(b)) for b in mh.SeedOccurrence(g, len(s)).view(np.uint32)]
                    continue
                m = max(len(s) - lm.getSeedLength(seed) + 1, 0)
                pos, keys = mh.SortedMerList(g, m), mh.SeedKeys(g, m)
                out[f"sml{g}"] = [f"{int(p)}\t{int(keys[p])}" for p in pos]
    elif mode in ("find", "compat"):
        with make_finder(lm, c) as mh:
            mh.SetSeed(lm.getSeed(c["weight"], c["rank"]))
            if c.get("match_log"):
                mh.SetMatchLog(True)
            if "start_points" in c:
                ml = mh.FindMatchesFromPosition(seqs, c["start_points"])
            else:
                ml = mh.FindMatches(seqs)
            out["list"] = lines(ml)
            if mode == "find":
                out["counters"] = rc.counters_section(mh.MemCount(), mh.MemCollisionCount())
                if c.get("offset_log"):
                    out["offset_log"] = ["\t".join(str(int(x)) for x in row) for row in mh.OffsetLog()]
                if c.get("match_log"):
                    out["match_log"] = lines(mh.MatchLog())
                device_filters(c, out, mh)
    elif mode in ("family", "recursion"):
        with make_finder(lm, c) as mh:
            mh.Clear()
            for i, (w, r) in enumerate(rounds_of(lm, name)):
                mh.ClearSequences()
                mh.SetSeed(lm.getSeed(w, r))
                out[f"round{i}"] = lines(mh.FindMatches(seqs))
            out["table"] = lines(mh.GetMatchList())
            out["counters"] = rc.counters_section(mh.MemCount(), mh.MemCollisionCount())
            if mode == "family":
                mh.EliminateOverlaps_v2(None, bool(c.get("eliminate_both", 0)))
            else:
                mh.EliminateOverlaps()
            if c.get("whole"):
                if c["nway_only"]:
                    mh.MultiplicityFilter(len(seqs))
                mh.LengthFilter(9)   # MIN_ANCHOR_LENGTH
                return dict(table=out["table"], counters=out["counters"], final=lines(mh.GetMatchList()))
            out["overlaps"] = lines(mh.GetMatchList())
            device_filters(c, out, mh)
    elif mode in ("eo1", "eo2"):
        l, s = rc.case_rows(name)
        with lm.MemHash(0) as mh:
            mh.LoadMatches(lm.MatchList(l, s))
            if mode == "eo1":
                mh.EliminateOverlaps()
            else:
                mh.EliminateOverlaps_v2(list(c["seq_ids"]) if "seq_ids" in c else None, bool(c.get("eliminate_both", 0)))
            out["overlaps"] = lines(mh.GetMatchList())
    return out


@pytest.mark.parametrize("name", SINGLE + FAMILY + RECURSION + WHOLE)
def test_hip_gives_what_the_reference_recorded(gpu_lib, name):
    assert rc.input_sha256(name) == rc.fixture()[name]["sha256"]   # the input the reference answered
    rc.check_case(name, gpu_sections(gpu_lib, name))


@pytest.mark.parametrize("name", [n for n in NAMES if rc.CASES[n]["mode"] in ("eo1", "eo2")])
def test_overlap_functions_on_a_caller_list(gpu_lib, name):
    """libmems_amd.EliminateOverlaps / EliminateOverlaps_v2, the functions that take a MatchList."""
    c = rc.CASES[name]
    ml = gpu_lib.MatchList(*rc.case_rows(name))
    if c["mode"] == "eo1":
        got = gpu_lib.EliminateOverlaps(ml)
    else:
        got = gpu_lib.EliminateOverlaps_v2(ml, list(c["seq_ids"]) if "seq_ids" in c else None, bool(c.get("eliminate_both", 0)))
    rc.check_case(name, dict(overlaps=lines(got)))


def final_section(name):
    kind, v = rc.CASES[name]["filters"][-1]
    return f"filter_{kind}_{v}"


def test_anchor_search_batch(gpu_lib):
    """The family problems as one AnchorSearchBatch: per problem the reference's list after
    EliminateOverlaps_v2 and LengthFilter(MIN_ANCHOR_LENGTH + 3), and its table's entry count."""
    fx = rc.fixture()
    with gpu_lib.MemHash(0) as mh:
        got = mh.AnchorSearchBatch([rc.case_seqs(n) for n in FAMILY])
        info = mh.AnchorBatchInfo()
    for p, name in enumerate(FAMILY):
        sec = final_section(name)
        rc.check_section(name, sec, fx[name]["sections"][sec], lines(got[p]))
        assert int(info["table_entries"][p]) == fx[name]["sections"]["table"]["count"]
        assert int(info["collisions"][p]) == fx[name]["counters"]["collision_count"]


@pytest.mark.parametrize("variant,nway_only", [("m0", False), ("mG", True)])
def test_recursion_batch(gpu_lib, variant, nway_only):
    """The recursion problems as one RecursionBatch on the finder the reference uses (gap_mh, a
    MemHash; under nway_only nway_mh, a MaskedMemHash with every genome in its mask,
    Aligner.cpp:1190-1195, 2208-2212): per problem the reference's list after the v1
    EliminateOverlaps, MultiplicityFilter(G) when nway_only, and LengthFilter(MIN_ANCHOR_LENGTH)."""
    fx = rc.fixture()
    names = [n for n in RECURSION if n.endswith("_" + variant)]
    whole = [n for n in WHOLE if n.endswith("_" + variant)]
    assert len(names) == 3 and len(whole) == 3 and all(rc.CASES[n]["nway_only"] == nway_only for n in names + whole)
    assert [rc.case_seqs(n) for n in names] == [rc.case_seqs(n) for n in whole]
    with make_finder(gpu_lib, rc.CASES[names[0]]) as mh:   # nway_mh, the all-genomes mask, under nway_only; else gap_mh
        assert isinstance(mh, gpu_lib.MaskedMemHash) == nway_only
        got = mh.RecursionBatch([rc.case_seqs(n) for n in names], nway_only=nway_only)
        info = mh.RecursionBatchInfo()
    for p, (name, wname) in enumerate(zip(names, whole)):
        sec = final_section(name)
        rc.check_section(name, sec, fx[name]["sections"][sec], lines(got[p]))
        # ... and the reference's own weight loop and tail (RecursionBatch chose the rounds itself)
        rc.check_section(wname, "final", fx[wname]["sections"]["final"], lines(got[p]))
        for rec in (fx[name], fx[wname]):
            assert int(info["table_entries"][p]) == rec["sections"]["table"]["count"]
            assert int(info["collisions"][p]) == rec["counters"]["collision_count"]
