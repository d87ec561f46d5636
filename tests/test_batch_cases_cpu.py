"""The cases of tests/batch_cases.py reach the paths of the batched replay they exist for: reach
conditions on the inputs, from the oracle and the constants parsed out of mums_internal.h,
mums_capi.hip and batch.hip alone.  A case that drifts off its path, or a constant that moves
under it, fails here; test_gpu_batch_paths.py runs the same cases on the device."""
from __future__ import annotations

import re

import numpy as np
import pytest

import batch_cases as bc


@pytest.fixture(scope="module")
def consts():
    return bc.source_constants()


def oracle_of(case):
    return [bc.find(p, case["seed"], case["table_size"], case["mask"]) for p in case["problems"]]


def test_parsed_constants(consts):
    """The values the cases were chosen for; the ladder is what DESIGN §4d states."""
    assert consts["repeat_limit"] == 1000 and consts["cap"] == 200000 and consts["pool_floor"] == 1 << 16
    assert consts["ladder"] == [(2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (64, 64)]
    assert [bc.ceil_log2(b) for b in (1, 2, 3, 8, 9, 65600)] == [0, 1, 2, 3, 4, 17]


def test_a_alphabet_problems_stay_in_the_lanes_and_judge_the_table(consts):
    case = bc.alphabet()
    assert len(case["problems"]) == 255 and ord("-") not in case["bytes"] and {0, 0x80, 0xFF} <= set(case["bytes"])
    B = len(case["problems"])
    for v, prob, (rl, _, st) in zip(case["bytes"], case["problems"], oracle_of(case)):
        assert bc.in_lanes(prob, case["seed"], B, consts, st), v
        assert st["restarts"] == 0 and len(rl) >= 1, v
        # density: v stands at about half of the ~100 positions of its letter
        assert prob[0].count(bytes([v])) >= (25 if bytes([v]) not in b"ACGT" else 60), v
        assert b"-" not in prob[0] + prob[1]
    # a lane's table that folds v to any other letter gives another answer on v's problem
    assert bc.unnoticed_foldings(case["problems"], case["bytes"], case["seed"]) == []


@pytest.mark.parametrize("G,table_size", bc.INSTANTIATION_CASES)
def test_b_every_instantiation(consts, G, table_size):
    case = bc.instantiation_case(G, table_size)
    assert bc.instantiation(G, consts["ladder"]) == bc.INSTANTIATION_OF[G]
    assert {bc.instantiation(g, consts["ladder"]) for g, _ in bc.INSTANTIATION_CASES} == {8, 16, 32, 64}
    refs = oracle_of(case)
    B = len(case["problems"])
    assert all(bc.in_lanes(p, case["seed"], B, consts, r[2]) for p, r in zip(case["problems"], refs))
    starts = np.concatenate([r[1] for r in refs])
    assert len(starts) > 0 and (starts == 0).any(), "no NO_MATCH column"
    if G in (8, 16, 32, 64):
        assert (starts[:, G - 1] != 0).any()
    if G >= 33:
        assert (starts[:, 32:] < 0).any(), "no reverse strand in a genome >= 32"
    if G == 64:
        # (at G = 33 no entry can start at genome 32: an entry holds two genomes)
        first = np.argmax(starts != 0, axis=1)
        assert (first >= 32).sum() >= 5


@pytest.mark.parametrize("name", list(bc.MASK_CASES))
def test_c_masks_at_33_and_64_genomes(consts, name):
    case = bc.mask_case(name)
    G, S = case["G"], case["S"]
    assert bc.instantiation(G, consts["ladder"]) == 64
    if case["mask"]:
        assert case["mask"] == sum(1 << (G - 1 - g) for g in S) and case["mask"] < 1 << 64
    if name in ("g64_20_63", "g64_all"):
        assert case["mask"] & 1                       # genome 63 is bit 0
    if name in ("g64_0_5_40", "g64_all"):
        assert case["mask"] >> 63                     # genome 0 is bit 63
    B = len(case["problems"])
    for prob in case["problems"]:
        rl, rs, st = bc.find(prob, case["seed"], case["table_size"], case["mask"])
        assert bc.in_lanes(prob, case["seed"], B, consts, st)
        assert len(rl) >= 3
        present = rs != 0
        if case["mask"]:
            assert (present == np.isin(np.arange(G), S)[None, :]).all()
            al, as_, _ = bc.find(prob, case["seed"], case["table_size"], 0)
            assert len(al) > len(rl)                  # the mask rejects
        else:
            assert len({tuple(row) for row in present.tolist()}) > 10   # every subset is accepted
        if case["mask"] and case["reversed_mask"] != case["mask"]:
            wl, ws, _ = bc.find(prob, case["seed"], case["table_size"], case["reversed_mask"])
            assert not (np.array_equal(wl, rl) and np.array_equal(ws, rs)), "the bit order goes unnoticed"


@pytest.mark.parametrize("name", list(bc.SORT_WIDTH_CASES))
def test_d_sort_width_at_and_over_64_bits(consts, name):
    case = bc.sort_width_case(name)
    w, B, bits = bc.SORT_WIDTH_CASES[name]
    assert bc.seed_weight(case["seed"]) == w and len(case["problems"]) == B
    assert bc.sort_bits(case["seed"], B) == 2 * w + 1 + bc.ceil_log2(B) == bits
    assert bits in (64, 65)
    for prob, (rl, _, st) in zip(case["problems"], oracle_of(case)):
        assert len(rl) >= 1
        assert bc.in_lanes(prob, case["seed"], B, consts, st) == (bits == 64)


def test_e_the_entry_pool_runs_full(consts):
    floor = consts["pool_floor"]
    case = bc.pool_case()
    B = len(case["problems"])
    assert B == bc.POOL_PROBLEMS and len(set(case["classes"])) == bc.POOL_CLASSES
    L = bc.seed_length(case["seed"])
    per_class = []
    for x in case["classes"]:
        assert len(x) == L
        rl, rs, st = bc.find((x, x), case["seed"])
        assert rl.tolist() == [L] and rs.tolist() == [[1, 1]] and st["probes"] == 1 and st["collision_count"] == 0
        assert bc.in_lanes((x, x), case["seed"], B, consts, st)
        per_class.append(len(rl))
    N = sum(bc.seedmers(p, case["seed"]) for p in case["problems"])
    assert N == 2 * B
    cap = bc.pool_cap(N, floor)
    entries = sum(per_class[p % bc.POOL_CLASSES] for p in range(B))
    # more entries than the pool holds, by few enough that the single finds of the lanes that
    # find it full stay cheap
    assert cap < entries <= cap + 256, (cap, entries)
    assert cap == floor and entries - cap == 64


def test_f_repeat_limit_edge(consts):
    case = bc.repeat_limit_case()
    B = len(case["problems"])
    assert bc.seed_length(case["seed"]) == 15
    for p, (prob, (_, _, st)) in enumerate(zip(case["problems"], oracle_of(case))):
        lanes = bc.in_lanes(prob, case["seed"], B, consts, st)
        if p in case["expect"]:
            assert (int(st["max_group"]), int(st["restarts"]), lanes) == case["expect"][p], p
        else:
            assert lanes and st["restarts"] == 0 and st["max_group"] < 100
    groups = sorted(g for g, _, _ in case["expect"].values())
    assert groups[0] == consts["repeat_limit"] and groups[1] == consts["repeat_limit"] + 1
    # the same three runs in two genome orders: only one of them restarts
    runs = {p: sorted(max(len(r) for r in re.findall(rb"A+", s)) for s in case["problems"][p]) for p in (4, 6)}
    assert runs[4] == runs[6] == [100 + 14, 450 + 14, 600 + 14]
    assert case["expect"][4][1] == 1 and case["expect"][6][1] == 0


def test_g_degenerate_sequences_in_wider_problems(consts):
    case = bc.degenerate_case()
    L = bc.seed_length(case["seed"])
    B = len(case["problems"])
    for p, (prob, (rl, rs, st)) in enumerate(zip(case["problems"], oracle_of(case))):
        assert len(prob) == 4 and len(rl) >= 1 and bc.in_lanes(prob, case["seed"], B, consts, st)
        for g in case["empty"].get(p, ()):
            assert len(prob[g]) < L and (rs[:, g] == 0).all()
        for g in case["one_seed"].get(p, ()):
            assert len(prob[g]) == L
    assert set(case["empty"]) == {1, 2, 3, 5}
    assert [len(s) for s in case["problems"][3]][1::2] == [L, L - 1]


@pytest.mark.parametrize("table_size", [40000, 7])
def test_h_repeat_rich_problems_stay_in_the_lanes(consts, table_size):
    case = bc.repeat_rich_case(table_size)
    B = len(case["problems"])
    refs = oracle_of(case)
    for p, (prob, (rl, _, st)) in enumerate(zip(case["problems"], refs)):
        assert bc.in_lanes(prob, case["seed"], B, consts, st) and st["restarts"] == 0 and len(rl) >= 1
        if p in case["rich"]:
            assert st["collision_count"] > 0.9 * st["probes"] and st["probes"] > 5000
        if p in case["big_groups"]:
            assert 500 <= st["max_group"] <= consts["repeat_limit"]


def test_i_context_sequence_changes_shape():
    seq = bc.context_sequence()
    Gs = [len(c["problems"][0]) for c in seq]
    assert Gs == [64, 2, 2, 2, 2]
    bits = [bc.sort_bits(c["seed"], len(c["problems"])) for c in seq]
    assert bits[2] == 65 and all(b <= 64 for i, b in enumerate(bits) if i != 2)
    assert all(bc.seedmers(p, seq[3]["seed"]) == 0 for p in seq[3]["problems"])
    assert len(seq[4]["problems"]) == 40
