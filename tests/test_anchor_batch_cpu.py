"""mums_anchor_batch / mums_anchor_tail_batch / mums_anchor_batch_info without a device: the ABI
surface, the mirror's grouping as host logic, the fixture against the live CPU models, the
conditions the cases of tests/anchor_batch_cases.py exist for, and the lane's code
(libmems_amd/csrc/anchor_lane.h, what anchor.hip runs per problem) compiled for the host against
tests/eo2_model.cpp and the oracle's std::sort restatement."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import anchor_batch_cases as ab
from conftest import ROOT
from oracle import oracle

CALLS = ("mums_anchor_batch", "mums_anchor_tail_batch", "mums_anchor_batch_info")
needs_compiler = pytest.mark.skipif(not ab.have_compiler(), reason="the CPU models need gcc / g++")


def test_header_declares_the_three_calls():
    hdr = open(os.path.join(ROOT, "include", "mums.h")).read()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(mums_ctx\* ctx," % name, hdr), name
    assert re.search(r"#define MUMS_ABI_VERSION 6\b", hdr)


def test_symbols_and_null_context(gpu_lib):
    lib = gpu_lib.load_library()
    for name in CALLS:
        assert name in gpu_lib.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.mums_abi_version() == 6
    assert lib.mums_anchor_batch(None, 0, 2, None, None, None, 1, 0, 12) == -1
    assert lib.mums_anchor_tail_batch(None, 0, 2, None, None, None, 0, 12) == -1
    assert lib.mums_anchor_batch_info(None, None, None, None, None, None) == -1
    for name in ("AnchorSearchBatch", "AnchorTailBatch", "AnchorBatchInfo"):
        assert callable(getattr(gpu_lib.MemHash, name))


def test_mirror_grouping_is_host_logic(gpu_lib):
    problems = [(b"A" * 300, b"C" * 300), (b"A" * 3, b"C" * 3), (b"A" * 3000, b"C" * 2000), (b"", b""),
                (b"A" * 280, b"C" * 320)]
    calls = []

    def get_seed(w, r):
        calls.append((w, r))
        return 1000 * w + r + 1

    ws, groups, pats = gpu_lib.anchor_seed_groups(problems, True, None, lambda n: {300: 7, 3: 0, 2500: 9, 0: 0}[n], get_seed)
    assert ws == [7, 0, 9, 0, 7] and groups == {7: [0, 4], 9: [2]}
    assert pats == {7: [7001, 7002, 7003], 9: [9001, 9002, 9003]} and 0 not in pats
    assert sorted(calls) == [(7, 0), (7, 1), (7, 2), (9, 0), (9, 1), (9, 2)]
    ws, groups, pats = gpu_lib.anchor_seed_groups(problems, False, [5, 5, 0, 11, 5], None, get_seed)
    assert ws == [5, 5, 0, 11, 5] and groups == {5: [0, 1, 4], 11: [3]} and pats == {5: [5001], 11: [11001]}
    with pytest.raises(ValueError):
        gpu_lib.anchor_seed_groups(problems, True, [5, 5])
    # the real tables: the mirror's default weights are the cases' (pairwiseAnchorSearch's choice)
    a = ab.find_case("a200")
    ws, groups, pats = gpu_lib.anchor_seed_groups(a["problems"])
    assert [tuple(pats[w]) if w else () for w in ws] == a["patterns"]


@needs_compiler
@pytest.mark.parametrize("name", list(ab.FIND_CASES))
def test_fixture_equals_the_live_models(name):
    assert ab.fixture()["find"][name] == ab.digest_case(name)


@needs_compiler
def test_tail_fixture_equals_the_live_model():
    fx = ab.fixture()
    assert fx["min_length"] == ab.MIN_LENGTH == 12
    assert set(fx["tail"]) == set(ab.tail_cases())
    for name in ab.tail_cases():
        assert fx["tail"][name] == ab.digest_tail(name), name


@needs_compiler
@pytest.mark.parametrize("name", list(ab.FIND_CASES))
def test_round_0_equals_the_oracle(name):
    c = ab.find_case(name)
    for p, (prob, pats, m) in enumerate(zip(c["problems"], c["patterns"], ab.model_case(name))):
        if not pats:
            continue
        rl, rs, st = oracle.find_matches(list(prob), pats[0], table_size=c["table_size"], masked=c["mask"] is not None,
                                         seq_mask=c["mask"] or 0)
        r0 = m["rounds"][0]
        assert np.array_equal(rl, r0["lengths"]) and np.array_equal(rs, r0["starts"]), (name, p)
        assert st["probes"] == r0["probes"] and st["collision_count"] == r0["collisions"], (name, p)


@needs_compiler
def test_a200_conditions():
    c = ab.find_case("a200")
    assert len(c["problems"]) == 200
    assert {len(pats) for pats in c["patterns"]} == {0, 3}
    assert {ab.default_weight(p) for p in c["problems"]} >= {0, 5, 7, 9}
    fam = v2 = both = filt = largest = 0
    for m, pats in zip(ab.model_case("a200"), c["patterns"]):
        if not pats:
            assert m["table_entries"] == 0
            continue
        r0, (tl, ts) = m["rounds"][0], m["table"]
        fam += not (np.array_equal(r0["lengths"], tl) and np.array_equal(r0["starts"], ts))
        el, es = ab.model_tail(tl, ts, False, 0)
        bl, bs = ab.model_tail(tl, ts, True, 0)
        v2 += len(el) < len(tl)
        both += not (np.array_equal(el, bl) and np.array_equal(es, bs))
        filt += bool((el < ab.MIN_LENGTH).any())
        largest = max(largest, len(tl))
    assert fam >= 150 and v2 >= 150 and both >= 100 and filt >= 20, (fam, v2, both, filt)
    assert largest > 16, "no table leaves the sort's insertion-only path"


@needs_compiler
def test_crowded_and_rank_order_conditions():
    for name in ("crowded_T7", "crowded_T1"):
        c = ab.find_case(name)
        assert len(c["problems"]) == 20 and c["table_size"] in (7, 1)
        assert max(m["table_entries"] for m in ab.model_case(name)) > c["table_size"]
    lists = {k: [m["table"] for m in ab.model_case(f"ranks_{k}")] for k in ab.RANK_ORDERS}

    def same(x, y):
        return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(lists[x], lists[y]))

    assert not same("r012", "r201"), "the order of the ranks goes unnoticed"
    assert not same("r0", "r012")
    # a repeated rank probes again: every probe of rounds 3 and 4 meets the table
    for m5, m3 in zip(ab.model_case("ranks_r01201"), ab.model_case("ranks_r012")):
        assert m5["probes"] > m3["probes"] and m5["collisions"] > m3["collisions"]


@needs_compiler
def test_wider_degenerate_and_restart_conditions():
    for name in ("g3", "g9"):
        starts = np.concatenate([m["table"][1] for m in ab.model_case(name)])
        assert (starts == 0).any() and (starts < 0).any(), name
    c = ab.find_case("g3_mask101")
    assert c["mask"] == 0b101
    for m in ab.model_case("g3_mask101"):
        assert ((m["table"][1] != 0) == np.array([True, False, True])[None, :]).all() and m["table_entries"] > 0
    d, dm = ab.find_case("degenerate"), ab.model_case("degenerate")
    L0, L1 = (ab.seed_length(s) for s in d["patterns"][0][:2])
    assert [m["table_entries"] for m in dm] == [0, dm[1]["table_entries"], 0, 1, 1, 1, dm[6]["table_entries"], 0]
    assert L0 <= len(d["problems"][3][1]) < L1 and d["problems"][4][0] == d["problems"][4][1]
    assert int(dm[5]["table"][0].max()) == 300   # the match ends with the sequences, not behind them
    r = ab.model_case("restart")
    assert [m["restarts"] for m in r] == [0, 3, 0, 3, 0]


@needs_compiler
def test_cap_and_pool_conditions():
    k = ab.source_constants()
    assert k["cap"] == 200000 and k["pool_floor"] == 1 << 16 and k["tail_cap"] == 1024
    c = ab.find_case("cap")
    largest = [max(ab.seedmers(p, s) for s in c["patterns"][0]) for p in c["problems"]]
    assert largest[1:4] == [k["cap"] - 1, k["cap"], k["cap"] + 1] and largest[0] < 2000 and largest[4] < 2000
    # the pool runs full in round 1, by the model's per-round entries and the formula in the source
    pc = ab.pool_case()
    pats, B = pc["patterns"][0], len(pc["problems"])
    per_round = [[len(r["lengths"]) for r in ab.model_rounds((x, x), pats)] for x in pc["classes"]]
    assert all(e == [0, 1] for e in per_round)
    nsum = sum(sum(ab.seedmers(p, s) for s in pats) for p in pc["problems"][:ab.POOL_CLASSES]) * (B // ab.POOL_CLASSES)
    assert nsum == 2 * B
    cap = ab.pool_cap(nsum, k["pool_floor"])
    assert cap == k["pool_floor"] and B - cap == 64


@needs_compiler
def test_tail_lists_and_the_heap_fallback():
    k = ab.source_constants()
    t = ab.tail_cases()
    assert [len(l) for l, _ in t["tail_cap"]] == [k["tail_cap"], k["tail_cap"] + 1]
    for G in ab.TAIL_GS:
        assert [len(l) for l, _ in t[f"random_g{G}"]] == list(ab.TAIL_MS)
        assert all(s.shape[1] == G for _, s in t[f"random_g{G}"])
    assert sum(len(ab.model_tail(l, s, False)[0]) for l, s in t["random_wide_g3"]) > 600
    i = 0
    for order in ab.SORT_ORDERS:
        for M in ab.ADVERSARIAL_MS:
            l, s = t["adversarial"][i]
            i += 1
            keys = ab.adversarial_keys(order, M)
            assert np.array_equal(np.abs(s[:, 0]).astype(np.uint64), keys)
            if order == "organ_pipe" and M >= 500:   # the depth limit is reached and shows in the order
                assert not np.array_equal(oracle.std_sort_ids(keys), oracle.std_sort_ids(keys, depth=10000))


@needs_compiler
def test_lane_code_on_the_host_equals_the_models():
    """anchor_lane.h with g++: sort, walk and filter of every tail list and every table of the
    find cases, and the sort alone at the depths the oracle's restatement is pinned at."""
    for name, lists in ab.tail_cases().items():
        for v, eb in ab.VARIANTS.items():
            for l, s in lists:
                for ml in (0, ab.MIN_LENGTH):
                    a, b = ab.model_tail(l, s, eb, ml), ab.lane_tail(l, s, eb, ml)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, v, len(l), ml)
    for name in ("a200", "g9", "crowded_T1"):
        for m in ab.model_case(name):
            for v in ab.find_case(name)["variants"]:
                b = ab.lane_tail(m["table"][0], m["table"][1], ab.VARIANTS[v])
                assert np.array_equal(m["final"][v][0], b[0]) and np.array_equal(m["final"][v][1], b[1]), (name, v)
    for order in ab.SORT_ORDERS:
        for n in (17, 500, 1000, 65536):
            keys = ab.adversarial_keys(order, n)
            for depth in (-1, 0, 3):
                assert np.array_equal(ab.lane_sort_ids(keys, depth), oracle.std_sort_ids(keys, depth=depth)), (order, n, depth)
