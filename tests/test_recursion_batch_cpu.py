"""mums_recursion_batch / mums_recursion_tail_batch without a device: the ABI surface, the mirror's
rounds and grouping as host logic, the fixture against the live CPU models, the conditions the cases
of tests/recursion_batch_cases.py exist for (counted, not assumed), and the lane's code
(libmems_amd/csrc/recursion_lane.h, what recursion.hip runs per problem) compiled for the host
against oracle.eliminate_overlaps and tests/eo_model.cpp, once more under the sanitizers as a
stand-alone program."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import recursion_batch_cases as rb
from conftest import ROOT

CALLS = ("mums_recursion_batch", "mums_recursion_tail_batch")
needs_compiler = pytest.mark.skipif(not rb.have_compiler(), reason="the CPU models need gcc / g++")

# Aligner.cpp:1142-1203 on the per-sequence default weights: (weights, nway_only, rounds)
WORKED = [((13, 11, 11, 9), False, [11, 9]), ((11, 11), False, [11]), ((13, 0), False, []), ((9, 9, 0), False, [9]),
          ((9, 9, 0), True, []), ((13, 11, 9), True, [9])]


def test_header_declares_the_two_calls():
    hdr = open(os.path.join(ROOT, "include", "mums.h")).read()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(mums_ctx\* ctx," % name, hdr), name
    assert re.search(r"#define MUMS_ABI_VERSION 6\b", hdr)


def test_symbols_and_null_context(gpu_lib):
    lib = gpu_lib.load_library()
    for name in CALLS:
        assert name in gpu_lib.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.mums_abi_version() == 6
    assert lib.mums_recursion_batch(None, 0, 2, None, None, None, 1, 0, 9) == -1
    assert lib.mums_recursion_tail_batch(None, 0, 2, None, None, None, 0, 9) == -1
    for name in ("RecursionBatch", "RecursionTailBatch", "RecursionBatchInfo"):
        assert callable(getattr(gpu_lib.MemHash, name))


@pytest.mark.parametrize("weights,nway,want", WORKED)
def test_recursion_rounds_worked_answers(gpu_lib, weights, nway, want):
    assert gpu_lib.recursion_rounds([0] * len(weights), nway, weights) == want
    assert rb.rounds_model(weights, nway) == want


def test_recursion_rounds_sweep_against_the_second_restatement(gpu_lib):
    rng = np.random.default_rng(7100)
    seen = set()
    for _ in range(4000):
        G = int(rng.integers(1, 7))
        ws = [int(w) for w in rng.choice([0, 3, 5, 7, 9, 11, 13, 15], size=G)]
        for nway in (False, True):
            got = gpu_lib.recursion_rounds([0] * G, nway, ws)
            assert got == rb.rounds_model(ws, nway), (ws, nway)
            assert got == sorted(got, reverse=True) and all(w >= rb.MIN_DNA_SEED_WEIGHT for w in got)
            seen.add(len(got))
    assert seen >= {0, 1, 2, 3}
    # the default weights come from the sequences' lengths (:1145)
    lens = [3000, 400, 20, 2500]
    ws = [gpu_lib.getDefaultSeedWeight(n) for n in lens]
    assert gpu_lib.recursion_rounds(lens) == rb.rounds_model(ws, False) != []


def test_mirror_grouping_is_host_logic(gpu_lib):
    problems = [(b"A" * 30, b"C" * 30, b"G" * 30), (b"A" * 30, b"", b"C" * 2), (b"A" * 30, b"C" * 31, b"G" * 29), (b"",) * 3]
    ws = [(13, 11, 9), (9, 0, 0), (13, 11, 9), (0, 0, 0)]
    calls = []

    def get_seed(w, r):
        calls.append((w, r))
        return 1000 * w + 1

    pats, groups = gpu_lib.recursion_groups(problems, False, ws, None, get_seed)
    assert pats == [(11001, 9001), (), (11001, 9001), ()] and groups == {(11001, 9001): [0, 2]}
    assert sorted(calls) == [(9, 0), (11, 0)]
    pats, groups = gpu_lib.recursion_groups(problems, True, ws, None, get_seed)
    assert pats == [(9001,), (), (9001,), ()] and groups == {(9001,): [0, 2]}
    with pytest.raises(ValueError):
        gpu_lib.recursion_groups(problems, False, ws[:2])


@needs_compiler
@pytest.mark.parametrize("name", list(rb.FIND_CASES))
def test_fixture_equals_the_live_models(name):
    assert rb.fixture()["find"][name] == rb.digest_case(name)


@needs_compiler
def test_tail_fixture_equals_the_live_model():
    fx = rb.fixture()
    assert fx["min_length"] == rb.MIN_LENGTH == 9
    assert set(fx["tail"]) == set(rb.tail_cases())
    for name in rb.tail_cases():
        assert fx["tail"][name] == rb.digest_tail(name), name


@needs_compiler
def test_r200_conditions():
    """Every G >= 3 problem appends, no G = 2 problem does, the multiplicity filter drops rows in
    most G >= 3 problems under nway_only, the length filter drops rows; at least 90 % of the
    appending problems run their appends inside the lane (below the row cap, inside their slice)."""
    k = rb.source_constants()
    assert k["tail_cap"] == 1024
    c = rb.find_case("r200")
    assert len(c["problems"]) == 200
    assert sorted({len(p) for p in c["problems"]}) == [2, 3, 4, 8]
    assert {len(pats) for pats in c["patterns"]} == {1, 2, 3}
    assert all(300 <= len(s) <= 3000 for p in c["problems"] for s in p)
    appending = in_lane = mult_drops = len_drops = wide = 0
    for prob, m in zip(c["problems"], rb.model_case("r200")):
        G = len(prob)
        tl, ts = m["table"]
        el, es, info = rb.lane_tail(tl, ts, 0, 0)
        assert not info["overflow"]
        if G == 2:
            assert info["apps"] == 0
            continue
        wide += 1
        assert info["apps"] >= 1, "a G >= 3 problem that does not append"
        appending += 1
        n = len(tl)
        in_lane += n <= k["tail_cap"] and not rb.lane_tail(tl, ts, 0, 0, cap=rb.slice_rows(n, G, k))[2]["overflow"]
        mult_drops += len(rb.filters(el, es, G, 0)[0]) < len(el)
        len_drops += bool((el < rb.MIN_LENGTH).any())
    assert wide == 150 and appending == 150
    assert mult_drops > wide // 2 and len_drops > 0, (mult_drops, len_drops)
    assert in_lane >= 0.9 * appending, (in_lane, appending)


@needs_compiler
def test_overflow_and_cap_conditions():
    k = rb.source_constants()
    l, s = rb.overflow_list()
    n, G = s.shape
    _, _, free = rb.lane_tail(l, s, 0, 0)
    assert n <= k["tail_cap"] and n + free["apps"] > rb.slice_rows(n, G, k)
    kept_l, kept_s, info = rb.lane_tail(l, s, 0, 0, cap=rb.slice_rows(n, G, k))
    assert info["overflow"] and len(kept_l) == 0
    t = rb.tail_cases()
    assert [len(l) for l, _ in t["tail_cap"]] == [k["tail_cap"], k["tail_cap"] + 1]
    # G = 3 is the smallest shape that appends, 16 / 17 rows straddle the sort's insertion threshold
    for M, (l, s) in zip(rb.ab.TAIL_MS, t["random_g3"]):
        assert len(l) == M and (M < 2 or rb.lane_tail(l, s, 0, 0)[2]["apps"] > 0)
    assert all(rb.lane_tail(l, s, 0, 0)[2]["apps"] == 0 for l, s in t["random_g2"])
    for G in (1, 2, 3, 4, 8, 9, 64):
        for n in (0, 1, 2, 17, 1024):
            assert rb.lane_shim().lane_slice_rows(n, G) == rb.slice_rows(n, G, k) >= n


@needs_compiler
def test_other_case_conditions():
    for m in rb.model_case("g3_mask101"):
        assert ((m["table"][1] != 0) == np.array([True, False, True])[None, :]).all() and m["table_entries"] > 0
        assert len(m["final"]["mG"][0]) == 0 and len(m["final"]["m2"][0]) == len(m["final"]["m0"][0]) > 0
    assert all(len(p) == 9 for p in rb.find_case("g9")["problems"])
    assert [m["restarts"] > 0 for m in rb.model_case("restart")] == [False, True, False]
    tables = {k: [m["table"] for m in rb.model_case(f"ranks_{k}")] for k in rb.RANK_ORDERS}

    def same(x, y):
        return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(tables[x], tables[y]))

    assert not same("w9_7", "w7_9") and not same("w9", "w9_7")
    for m3, m2 in zip(rb.model_case("ranks_w9_7_9"), rb.model_case("ranks_w9_7")):
        assert m3["probes"] > m2["probes"] and m3["collisions"] > m2["collisions"]
    d = rb.model_case("degenerate")
    assert [m["table_entries"] for m in d][0] == 0 and d[2]["table_entries"] == 0 and d[4]["table_entries"] == 1


def tail_inputs():
    for name, lists in rb.tail_cases().items():
        for l, s in lists:
            yield name, l, s
    for name in ("g9", "ranks_w9_7", "restart"):
        for m in rb.model_case(name):
            yield name, m["table"][0], m["table"][1]


@needs_compiler
def test_lane_code_on_the_host_equals_the_models():
    """recursion_lane.h with g++: sort, walk and filters of every tail list (the adversarial sort
    orders among them) and of tables of the find cases against the oracle and against the real
    std::sort on Match* (eo_model.cpp)."""
    for name, l, s in tail_inputs():
        G = s.shape[1]
        for mult in (0, 2, G):
            for ml in rb.TAIL_MIN_LENGTHS:
                a = rb.model_tail(l, s, mult, ml)
                b = rb.lane_tail(l, s, mult, ml)
                e = rb.eo_model_tail(l, s, mult, ml)
                assert not b[2]["overflow"]
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, len(l), mult, ml)
                assert np.array_equal(e[0], b[0]) and np.array_equal(e[1], b[1]), (name, len(l), mult, ml, "eo_model")
    for prob, m in zip(rb.find_case("r200")["problems"], rb.model_case("r200")):
        for v in ("m0", "mG"):
            b = rb.lane_tail(m["table"][0], m["table"][1], rb.VARIANTS[v](len(prob)))
            assert np.array_equal(m["final"][v][0], b[0]) and np.array_equal(m["final"][v][1], b[1]), v


@needs_compiler
def test_lane_under_the_sanitizers_as_a_program(tmp_path):
    """The shim and its own main, built with -fsanitize=address,undefined, over every tail list in
    a slice of exactly its planned size (the overflow list runs full) and once with room for all."""
    k = rb.source_constants()
    exe = f"{rb.LANE_MAIN}.{os.getpid()}"
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DRECURSION_LANE_MAIN", "-o", exe, rb.SHIM], check=True)
    jobs, want = [], []
    for name, l, s in tail_inputs():
        n, G = s.shape
        for cap in (rb.slice_rows(n, G, k), 64 * n + 64):
            jobs.append((G, cap, G if name == "g9" else 0, rb.MIN_LENGTH, l, s))
            el, es, info = rb.lane_tail(l, s, jobs[-1][2], rb.MIN_LENGTH, cap=cap)
            want.append((len(el), info["apps"], int(info["overflow"]), rb.lane_main_checksum(el, es)))
    path = str(tmp_path / "lists.bin")
    rb.lane_main_input(path, jobs)
    try:
        r = subprocess.run([exe, path], capture_output=True, text=True)
    finally:
        os.remove(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert got == want
    assert any(w[2] for w in want) and any(w[1] and not w[2] for w in want)
