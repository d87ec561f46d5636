"""The CPU oracle and its models against answers recorded from libMems itself.

tests/golden/ref_cases.json holds, for every case of tests/ref_cases.py, what the reference
computed (oracle/ref_driver.cpp linked with libMems' own translation units; recorded by
golden/make_ref_golden.py).  Here the oracle (oracle/mums_oracle.c, eliminate_overlaps.c) and the
models the other fixtures are generated from (tests/seed_family_model.c, tests/eo2_model.cpp) must
give exactly that: lists in GetMatchList order, MemCount, collision count, offset log, match log,
SML order, seed table, float32 bit patterns.  No tolerance anywhere.

Where oracle/_ref/ref_driver exists (the libMems tree was present at build time) the live driver
must reproduce every fixture and the nine md5 sums of SURVEY.md Appendix C, which came from a
build whose recipe was never committed: the committed recipe is that recipe.  Without the driver
those tests skip; the others never do (a missing C compiler for the models is a failure)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import recursion_batch_cases as rb
import ref_cases as rc
import seed_family_cases as sf
import test_eliminate_overlaps_v2_cpu as eo2
from conftest import GOLDEN
from oracle import oracle

NAMES = list(rc.CASES)
needs_driver = pytest.mark.skipif(not rc.have_driver(), reason="oracle/_ref/ref_driver is not built (no libMems tree)")


# ---- the oracle's answer to a case, in the driver's sections ------------------------------------
def seeds_sections():
    L = oracle.lib()
    seeds = []
    for w in range(1, 34):
        for r in range(3):
            s = oracle.get_seed(w, r)
            seeds.append(f"{w}\t{r}\t{s}\t{L.oracle_seed_length(s)}\t{L.oracle_seed_weight(s)}")
    ns = list(range(65)) + [(1 << e) + k for e in range(7, 41) for k in (-1, 0, 1)]
    n = 100
    while n <= 10_000_000_000:
        ns += [n * m for m in (1, 3, 5, 7, 9)]
        n *= 10
    return dict(seeds=seeds, default_weight=[f"{n}\t{L.oracle_default_seed_weight(n)}" for n in ns])


def find_kwargs(c):
    kw = dict(repeat_tol=c.get("repeat_tol", 0), enum_tol=c.get("enum_tol", 1), table_size=c.get("table_size", 40000))
    if c.get("finder") == "masked":
        kw.update(masked=True, seq_mask=c["mask"])
    if c.get("finder") == "pairwise":
        kw.update(pairwise=True)
    if c.get("finder") == "parallel":
        kw.update(parallel_compat=True)
    if "start_points" in c:
        kw.update(start_points=c["start_points"])
    return kw


@functools.lru_cache(maxsize=None)
def models():
    return sf.load_model(), eo2.load_model()


def oracle_sections(name):
    c = rc.CASES[name]
    mode, seqs = c["mode"], list(rc.case_seqs(name))
    if mode == "seeds":
        return seeds_sections()
    seed = oracle.get_seed(c["weight"], c["rank"]) if "weight" in c else None
    out = {}
    if mode == "sml":
        for g, s in enumerate(seqs):
            pos, keys = oracle.build_sml(s, seed), oracle.seed_keys(s, seed)
            out[f"sml{g}"] = [f"{int(p)}\t{int(keys[p])}" for p in pos]
    elif mode == "occurrence":
        for g, s in enumerate(seqs):
            out[f"occurrence{g}"] = [str(int(b)) for b in oracle.seed_occurrence(s, seed).view(np.uint32)]
    elif mode in ("find", "compat"):
        l, s, st = oracle.find_matches(seqs, seed, **find_kwargs(c))
        out["list"] = rc.lines_of(l, s)
        if mode == "find":
            out["counters"] = rc.counters_section(st["mem_count"], st["collision_count"])
            if c.get("offset_log"):
                out["offset_log"] = ["\t".join(str(int(x)) for x in row) for row in st["offset_log"]]
            if c.get("match_log"):
                out["match_log"] = rc.lines_of(*st["match_log"])
            rc.filter_sections(c, out, l, s)
    elif mode in ("family", "recursion"):
        if mode == "family":
            w = int(oracle.lib().oracle_default_seed_weight((len(seqs[0]) + len(seqs[1])) // 2))   # ProgressiveAligner.cpp:615
            rounds = [(w, r) for r in range(3)]
        elif c.get("whole"):   # the rounds the project's restatement of Aligner.cpp:1142-1177 gives
            rounds = rc.recursion_rounds(seqs, c["nway_only"])
        else:
            rounds = rc.case_rounds(name)
        kw = dict(masked=True, seq_mask=c["mask"]) if c.get("finder") == "masked" else {}
        res = sf.run_model(models()[0], [(seqs, oracle.get_seed(w, r), kw) for w, r in rounds])
        for i, rnd in enumerate(res):
            out[f"round{i}"] = rc.lines_of(rnd["lengths"], rnd["starts"])
        l, s = res[-1]["lengths"], res[-1]["starts"]
        out["table"] = rc.lines_of(l, s)
        out["counters"] = rc.counters_section(res[-1]["mem_count"], res[-1]["collisions"])
        if mode == "family":
            l, s, _ = eo2.model_eo2(models()[1], l, s, None, bool(c.get("eliminate_both", 0)))
        else:
            l, s = oracle.eliminate_overlaps(l, s)
        s = np.asarray(s).reshape(len(l), len(seqs))
        if c.get("whole"):
            out = dict(table=out["table"], counters=out["counters"])
            l, s = rb.filters(l, s, len(seqs) if c["nway_only"] else 0, rb.MIN_LENGTH)
            out["final"] = rc.lines_of(l, s)
            return out
        out["overlaps"] = rc.lines_of(l, s)
        rc.filter_sections(c, out, l, s)
    elif mode in ("eo1", "eo2"):
        l, s = rc.case_rows(name)
        if mode == "eo1":
            l, s = oracle.eliminate_overlaps(l, s)
        else:
            l, s, _ = eo2.model_eo2(models()[1], l, s, list(c["seq_ids"]) if "seq_ids" in c else None,
                                    bool(c.get("eliminate_both", 0)))
        out["overlaps"] = rc.lines_of(l, s)
    return out


check_case = rc.check_case


# ---- the fixture itself ---------------------------------------------------------------------------
def test_fixture_holds_exactly_the_cases():
    assert set(rc.fixture()) == set(rc.CASES)


def test_fixture_file_is_small():
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                  if f not in ("ref_cases.json",) and os.path.isfile(os.path.join(GOLDEN, f)))
    assert os.path.getsize(rc.FIXTURE) <= largest


@pytest.mark.parametrize("name", NAMES)
def test_input_is_the_recorded_one(name):
    assert rc.input_sha256(name) == rc.fixture()[name]["sha256"]


def test_cases_reach_what_they_are_for():
    """Restart cases restart, the tolerance cases enumerate, the masks are not "all genomes", a
    recursion tail appends rows, the tied list has more than 16 equal sort keys."""
    fx = rc.fixture()
    for name in ("restart_n_gapped", "restart_high_copy", "restart_high_copy_tandem", "restart_from_position"):
        assert fx[name]["sections"]["offset_log"]["count"] > 0, name
    assert sum(fx[f"restart_mixed_{s}"]["sections"]["offset_log"]["count"] > 0 for s in range(6)) >= 3
    for G in (3, 4):
        counts = [fx[f"find_tol_G{G}_rt{rt}_et{et}"]["sections"]["list"]["count"] for rt, et in ((0, 1), (1, 1), (1, 2), (2, 3))]
        assert counts[0] < counts[1] <= counts[2] and counts[-1] > counts[0], counts
    for name, c in rc.CASES.items():
        if c.get("finder") == "masked" and c["mode"] == "find":
            assert c["mask"] != (1 << len(rc.case_seqs(name))) - 1 and fx[name]["sections"]["list"]["count"] > 20, name
        for kind, v in c.get("filters", ()):
            if c["mode"] == "find":
                secs = fx[name]["sections"]
                assert 0 < secs[f"filter_{kind}_{v}"]["count"] < secs["list"]["count"], (name, kind)
    appended = 0
    for i in range(3):
        secs = fx[f"recursion_{i}_m0"]["sections"]
        table = set(secs["table"]["text"].splitlines())
        appended += any(ln not in table and ln.split("\t").count("0") == 1 for ln in secs["overlaps"]["text"].splitlines())
    assert appended >= 1
    # the table size shows: three sizes, three orders of one set of matches
    orders = [fx[n]["sections"]["list"] for n in ("table_T7", "table_T1009", "rearranged")]
    assert rc.case_bytes("table_T7").split(b"data\n", 1)[1] == rc.case_bytes("rearranged").split(b"data\n", 1)[1]
    assert len({o["count"] for o in orders}) == 1 and len({o["list_md5"] for o in orders}) == 3, orders
    assert len({fx[n]["sections"]["match_log"]["list_md5"] for n in ("table_T7", "table_T1009")}) == 1
    # nway_only searches with the all-genomes mask: fewer table entries than the plain finder's
    for i in range(3):
        assert rc.CASES[f"recursion_{i}_mG"]["finder"] == "masked" and rc.CASES[f"recursion_{i}_mG"]["mask"] == 7
        assert fx[f"recursion_{i}_mG"]["sections"]["table"]["count"] < fx[f"recursion_{i}_m0"]["sections"]["round0"]["count"]
    # the reference's own weight loop searched with the rounds the cases with given rounds name
    for i in range(3):
        for v in ("m0", "mG"):
            a, b = fx[f"recursion_whole_{i}_{v}"], fx[f"recursion_{i}_{v}"]
            assert all(a["sections"]["table"][k] == b["sections"]["table"][k] for k in ("count", "list_md5"))
            assert a["counters"] == b["counters"]
            assert a["sections"]["final"]["list_md5"] == b["sections"]["filter_len_9"]["list_md5"]
    l, s = rc.tied_list()
    assert max(np.unique(np.abs(s[:, g]), return_counts=True)[1].max() for g in range(2)) > 16


# ---- the oracle against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_gives_what_the_reference_recorded(oracle_mod, name):
    check_case(name, oracle_sections(name))


# ---- the committed recipe against the fixture and Appendix C ---------------------------------------------
@needs_driver
@pytest.mark.parametrize("name", NAMES)
def test_live_driver_reproduces_the_fixture(name):
    check_case(name, rc.run_driver(name))


APPENDIX_C = json.load(open(os.path.join(GOLDEN, "appendix_c.json")))
APPENDIX_C_CASES = [dict(c, finder={"MemHash": "memhash", "MaskedMemHash": "masked"}[c["mode"]]) for c in APPENDIX_C["cases"]] + \
                   [dict(c, finder="parallel") for c in APPENDIX_C["parallel_compat"]]


def appendix_c_id(c):
    return f"G{c['G']}_n{c['n']}_p{c['p']}_{c['finder']}"


def appendix_c_param(c):
    return pytest.param(c, id=appendix_c_id(c), marks=[pytest.mark.slow] if c["G"] * c["n"] >= 40_000_000 else [])


@needs_driver
@pytest.mark.parametrize("case", [appendix_c_param(c) for c in APPENDIX_C_CASES])
def test_live_driver_reproduces_appendix_c(oracle_mod, tmp_path, case):
    """The md5 sums of SURVEY.md Appendix C, recorded from a build that was never committed."""
    import subprocess
    seqs = oracle_mod.generate(case["G"], case["n"], case["p"], 12345)
    head = f"mode find\nfinder {case['finder']}\nweight {case['w']}\nrank 0\n"
    if case["finder"] == "masked":
        head += f"mask {case['mask']}\n"
    head += f"G {len(seqs)}\nlengths " + " ".join(str(len(s)) for s in seqs) + "\ndata\n"
    path, outp = tmp_path / "case", tmp_path / "out"
    path.write_bytes(head.encode() + b"".join(seqs))
    subprocess.run([rc.DRIVER, str(path), str(outp)], check=True)
    secs = rc.parse_output(outp.read_text())
    txt = "".join(ln + "\n" for ln in secs["list"])
    assert len(secs["list"]) == case["matches"]
    assert hashlib.md5(txt.encode()).hexdigest() == case["md5"]
    if "collisions" in case:
        assert int(secs["counters"][1].split(" ")[1]) == case["collisions"]
