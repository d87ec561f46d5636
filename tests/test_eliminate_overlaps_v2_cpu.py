"""EliminateOverlaps_v2 (ProgressiveAligner.h:300-406), CPU side: the literal C++ model over
Match* vectors sorted by this toolchain's real std::sort (tests/eo2_model.cpp), its branch
counters on the inputs the GPU test replays, the processNewMatch claim (:260-271: nothing is
ever appended to a list of ungapped matches), and the recorded results of
tests/golden/eo_v2_cases.json against the live model."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from test_eliminate_overlaps_cpu import EDGE_LISTS, random_matchlist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libeo2_model.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "eo_v2_cases.json")

# (M, G, span, seed) before the shifted copies are appended
CASES = [(2, 2, 50, 1), (10, 2, 100, 2), (200, 3, 2000, 3), (3000, 4, 30000, 4), (5000, 8, 20000, 5),
         (3000, 3, 300, 7),            # nearly one cluster
         (3000, 4, 3_000_000, 9),      # sparse: many clusters of size 1-2
         (20000, 5, 400000, 6)]
SUBSET_CASE = (3000, 4, 30000, 4)      # the subset runs: [G - 1, 0] and [0, 0]
CHAIN_GS = (2, 4)                      # FindMatches -> v2 -> LengthFilter on the repeat-rich input
CHAIN_MIN_LENGTH = 30
COUNTERS = ("pairs", "consistent", "del_i", "del_j", "crop_i", "crop_j", "kept")


def load_model():
    """Builds tests/eo2_model.cpp (aside, then renamed: parallel workers never load a partial file)."""
    os.makedirs(BUILD, exist_ok=True)
    tmp = f"{SO}.{os.getpid()}"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, os.path.join(ROOT, "tests", "eo2_model.cpp")],
                   check=True)
    os.replace(tmp, SO)
    L = ctypes.CDLL(SO)
    L.model_eliminate_overlaps_v2.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.model_eliminate_overlaps_v2.restype = ctypes.c_uint64
    return L


@pytest.fixture(scope="module")
def model():
    return load_model()


def v2_matchlist(M, G, span, seed):
    """random_matchlist plus 30 % shifted copies: a random row with every defined start moved by
    one common signed amount in 1..199 (a reverse start that would cross zero becomes NO_MATCH, a
    forward one stops at 1) and a fresh random length.  A copy and its source overlap with the
    same offset in every sequence, which independent random starts almost never do."""
    rng = np.random.default_rng(seed)
    lengths, starts = random_matchlist(rng, M, G, start_span=span)
    k = (3 * M) // 10
    if k == 0:
        return lengths, starts
    rows = rng.integers(0, M, size=k)
    shift = rng.integers(1, 200, size=k) * rng.choice(np.array([-1, 1]), size=k)
    src = starts[rows]
    moved = src + shift[:, None]
    fwd = np.maximum(moved, 1)
    rev = np.where(moved < 0, moved, 0)
    copies = np.where(src > 0, fwd, np.where(src < 0, rev, 0)).astype(np.int64)
    copy_len = rng.integers(1, 300, size=k).astype(np.uint64)
    return np.concatenate([lengths, copy_len]), np.concatenate([starts, copies])


def model_eo2(L, lengths, starts, seq_ids=None, eliminate_both=False):
    """(lengths, starts, counters) of the model; the output can never be larger than cap."""
    M, G = starts.shape
    cap = 8 * M + 64
    lo = np.zeros(cap, dtype=np.uint64)
    so = np.zeros(cap * G, dtype=np.int64)
    cnt = np.zeros(len(COUNTERS), dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    ids = None if seq_ids is None else np.ascontiguousarray(list(seq_ids) + [0], dtype=np.uint32)   # never empty
    k = L.model_eliminate_overlaps_v2(G, M, lengths.ctypes.data, starts.ctypes.data,
                                      None if ids is None else ids.ctypes.data, 0 if ids is None else len(ids) - 1,
                                      int(eliminate_both), lo.ctypes.data, so.ctypes.data, cap, cnt.ctypes.data)
    assert k <= cap
    return lo[:k], so[:k * G].reshape(k, G), dict(zip(COUNTERS, (int(c) for c in cnt)))


def digest(lengths, starts):
    return hashlib.md5(np.asarray(lengths).astype("<u8").tobytes() + np.asarray(starts).astype("<i8").tobytes()).hexdigest()


def build_input(case):
    """The MatchList of a run: v2_matchlist of a CASES tuple, or an edge list of
    test_eliminate_overlaps_cpu.py by name (a cluster head carried across tiles, coordinates
    above 2^32), taken as it is."""
    return EDGE_LISTS[case]() if isinstance(case, str) else v2_matchlist(*case)


def all_inputs():
    return {c: build_input(c) for c in list(CASES) + sorted(EDGE_LISTS)}


def edge_key(name, eliminate_both):
    return f"edge_{name}_both{int(eliminate_both)}_idsall"


def case_key(M, G, span, seed, eliminate_both, seq_ids=None):
    ids = "all" if seq_ids is None else "-".join(str(i) for i in seq_ids)
    return f"M{M}_G{G}_span{span}_seed{seed}_both{int(eliminate_both)}_ids{ids}"


def repeat_rich(G):
    """The input of test_eliminate_overlaps_on_findmatches_output, for G genomes."""
    seqs = oracle.generate(G, 400_000, 0.02, 99)
    rep = seqs[0][1000:3000]
    return [s[:50_000] + rep + s[50_000:200_000] + rep + s[200_000:] for s in seqs]


def fixture_runs():
    """Every recorded run: (key, input builder, seq_ids, eliminate_both)."""
    runs = []
    for c in CASES:
        for both in (False, True):
            runs.append((case_key(*c, both), c, None, both))
    G = SUBSET_CASE[1]
    for ids in ([G - 1, 0], [0, 0]):
        for both in (False, True):
            runs.append((case_key(*SUBSET_CASE, both, ids), SUBSET_CASE, ids, both))
    for name in sorted(EDGE_LISTS):
        for both in (False, True):
            runs.append((edge_key(name, both), name, None, both))
    return runs


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["runs"]


@pytest.fixture(scope="module")
def inputs():
    return all_inputs()


@pytest.fixture(scope="module")
def results(model, inputs):
    """The model's result of every recorded run, computed once."""
    return {key: model_eo2(model, *inputs[c], ids, both) for key, c, ids, both in fixture_runs()}


@pytest.mark.parametrize("case", [c for c in CASES if c[0] >= 200], ids=str)
@pytest.mark.parametrize("both", [False, True])
def test_every_branch_is_taken(results, case, both):
    cnt = results[case_key(*case, both)][2]
    for name in COUNTERS[:6]:
        assert cnt[name] > 0, (name, cnt)


@pytest.mark.parametrize("key,case,ids,both", fixture_runs(), ids=[r[0] for r in fixture_runs()])
def test_no_new_match_is_kept(results, inputs, key, case, ids, both):
    ol, _, cnt = results[key]
    assert cnt["kept"] == 0
    assert len(ol) <= len(inputs[case][0])


@pytest.mark.parametrize("name", sorted(EDGE_LISTS))
@pytest.mark.parametrize("both", [False, True])
def test_edge_lists_have_work(results, inputs, name, both):
    ol, os_, cnt = results[edge_key(name, both)]
    lengths, starts = inputs[name]
    assert cnt["pairs"] > 0 and cnt["del_i"] + cnt["del_j"] + cnt["crop_i"] + cnt["crop_j"] > 0
    assert len(ol) < len(lengths) or not np.array_equal(os_, starts)


def test_v2_is_not_v1(results, inputs):
    differs = 0
    for c in CASES:
        vl, vs, _ = results[case_key(*c, False)]
        ol, os_ = oracle.eliminate_overlaps(*inputs[c])
        differs += not (np.array_equal(vl, ol) and np.array_equal(vs, os_))
    assert differs > 0


def test_subsets(model, results, inputs):
    G = SUBSET_CASE[1]
    lengths, starts = inputs[SUBSET_CASE]
    for both in (False, True):
        full = results[case_key(*SUBSET_CASE, both)]
        last_first = results[case_key(*SUBSET_CASE, both, [G - 1, 0])]
        twice = results[case_key(*SUBSET_CASE, both, [0, 0])]
        digests = {digest(*r[:2]) for r in (full, last_first, twice)}
        assert len(digests) == 3   # each its own result
        l1, s1, _ = model_eo2(model, lengths, starts, [0], both)
        l2, s2, _ = model_eo2(model, l1, s1, [0], both)
        assert np.array_equal(l2, twice[0]) and np.array_equal(s2, twice[1])
        le, se, cnt = model_eo2(model, lengths, starts, [], both)   # no id: no pass
        assert np.array_equal(le, lengths) and np.array_equal(se, starts) and cnt["pairs"] == 0


@pytest.mark.parametrize("key", [r[0] for r in fixture_runs()])
def test_fixture_matches_model(results, recorded, key):
    ol, os_, _ = results[key]
    assert recorded[key] == {"count": len(ol), "md5": digest(ol, os_)}


def test_fixture_holds_exactly_the_runs(recorded):
    chain = {f"chain_G{G}_both{b}_min{CHAIN_MIN_LENGTH}" for G in CHAIN_GS for b in (0, 1)}
    assert set(recorded) == {r[0] for r in fixture_runs()} | chain


@pytest.mark.parametrize("G", CHAIN_GS)
def test_v2_on_findmatches_output(model, recorded, G):
    # repeat-rich related genomes: MemHash MatchLists with overlapping entries, then LengthFilter
    lengths, starts, _ = oracle.find_matches(repeat_rich(G), oracle.get_seed(11))
    for both in (False, True):
        ol, os_, cnt = model_eo2(model, lengths, starts, None, both)
        assert cnt["pairs"] > 0 and cnt["kept"] == 0 and len(ol) <= len(lengths)
        assert len(ol) != len(lengths) or not np.array_equal(os_, starts)   # something was cropped
        keep = ol >= CHAIN_MIN_LENGTH
        assert recorded[f"chain_G{G}_both{int(both)}_min{CHAIN_MIN_LENGTH}"] == {
            "count": int(keep.sum()), "md5": digest(ol[keep], os_[keep])}
