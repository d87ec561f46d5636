"""mums_recursion_batch / mums_recursion_tail_batch (batch.hip's carried rounds, recursion.hip's v1 tail;
DESIGN.md §4f): the cases shared by test_recursion_batch_cpu.py, test_gpu_recursion_batch.py and
golden/make_recursion_batch_golden.py, the composition of the project's CPU models that gives their
expected values, and the digests golden/recursion_batch_cases.json records.

Expected values: tests/seed_family_model.c gives a problem's table round by round
(anchor_batch_cases.model_rounds), oracle.eliminate_overlaps the v1 EliminateOverlaps on it, numpy
the multiplicity and length filters.  Seeded generators, no files, no GPU.  A find case is a dict:
problems (tuples of bytes), patterns (per problem the seed patterns in round order; empty: no round,
no search), table_size, mask (None: MemHash), variants (names of VARIANTS: the multiplicity)."""
from __future__ import annotations

import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np

import anchor_batch_cases as ab
import seed_family_cases as sf
from oracle import oracle
from test_eliminate_overlaps_cpu import random_matchlist

ROOT = ab.ROOT
CSRC = ab.CSRC
FIXTURE = os.path.join(ROOT, "tests", "golden", "recursion_batch_cases.json")
LANE_SO = os.path.join(sf.BUILD, "librecursion_lane_shim.so")
LANE_MAIN = os.path.join(sf.BUILD, "recursion_lane_asan")
EO_SO = os.path.join(sf.BUILD, "libeo_model_recursion.so")
SHIM = os.path.join(ROOT, "tests", "recursion_lane_shim.cpp")
MIN_LENGTH = 9             # MIN_ANCHOR_LENGTH (Aligner.h:266, Aligner.cpp:1218)
MIN_DNA_SEED_WEIGHT = 5    # SeedMasks.h:375
# the multiplicity of MultiplicityFilter: none, 2, the problem's G (nway_only)
VARIANTS = {"m0": lambda G: 0, "m2": lambda G: 2, "mG": lambda G: G}
TAIL_MIN_LENGTHS = (0, MIN_LENGTH)


# ---- constants read out of the sources -------------------------------------------------------
def source_constants():
    """tail_cap (rows of one list the tail's lane takes) and the slice formula of recursion_lane.h:
    slice_rows(n, G) = n below 2 rows or at G <= 2, else min(factor_max, max(2, 2 * (G - 2))) * n + slack."""
    lane = open(os.path.join(CSRC, "recursion_lane.h")).read()
    factor_max = int(re.search(r"constexpr uint32_t kSliceFactorMax = (\d+);", lane).group(1))
    slack = int(re.search(r"constexpr uint32_t kSliceSlack = (\d+);", lane).group(1))
    assert "const uint32_t f = G <= 3 ? 2u : 2u * (uint32_t)(G - 2);" in lane
    assert "return f < kSliceFactorMax ? f : kSliceFactorMax;" in lane
    assert "{ return n < 2 || G <= 2 ? n : slice_factor(G) * n + kSliceSlack; }" in lane
    return dict(tail_cap=ab.source_constants()["tail_cap"], factor_max=factor_max, slack=slack)


def slice_rows(n, G, k=None):
    k = k or source_constants()
    return n if n < 2 or G <= 2 else min(k["factor_max"], max(2, 2 * (G - 2))) * n + k["slack"]


# ---- Aligner.cpp:1142-1203, a second restatement (the mirror's recursion_rounds is the first) ----
def rounds_model(weights, nway_only):
    """The seed weights one problem is searched with, in order: the reference's loop written over
    the descending weight list with an index, not over the multimap with an iterator.  (The last
    sequence taken does not set prev_mer, :1160-1164: two sequences of different weights are
    searched at the larger one.)"""
    desc = sorted((int(w) for w in weights), reverse=True)
    G, i, taken, out = len(desc), 0, 0, []
    while i < G:
        prev = desc[i]
        while desc[i] >= MIN_DNA_SEED_WEIGHT and (desc[i] == prev or taken < 2):
            taken += 1
            if i == G - 1:
                i = G
                break
            prev = desc[i]
            i += 1
        if taken < 2 or prev < MIN_DNA_SEED_WEIGHT:
            break
        if nway_only and taken < G:
            continue
        out.append(prev)
    return out


def default_weights(problem):
    return [int(oracle.lib().oracle_default_seed_weight(len(s))) for s in problem]


def patterns_of(weights):
    return tuple(oracle.get_seed(w, 0) for w in weights)


# ---- the find cases ---------------------------------------------------------------------------
def _case(problems, patterns, table_size=40000, mask=None, variants=("m0", "mG")):
    if not isinstance(patterns, list):
        patterns = [tuple(patterns)] * len(problems)
    return dict(problems=[tuple(p) for p in problems], patterns=[tuple(x) for x in patterns], table_size=table_size,
                mask=mask, variants=tuple(variants))


R200_GS = (2, 3, 4, 8)
R200_ROUNDS = ((7,), (9, 7), (11, 9, 7))


R200_FLANK = 40
# the ancestor's largest length per G: the lanes' rounds cost about the largest problem's seed-mers
# times a figure that grows with G, so the wide problems are the short ones
R200_NMAX = {2: 2960, 3: 2960, 4: 1500, 8: 800}


@functools.lru_cache(maxsize=None)
def r200():
    """200 gap problems, 50 each at G = 2, 3, 4 and 8: G copies (3 % substitutions, every third
    reverse-complemented) of at least three quarters of an ancestor X Y of 400 .. R200_NMAX[G] bp (sequences of 300 .. 3000 bp).  R200_FLANK bases on either
    side of the junction are left unmutated, and every copy but the first gets the inserted repeat
    Y[:k] X[-k:] (k = 12 .. 20) at the junction: the match X Y[:k] and the match X[-k:] Y are in
    every sequence and overlap in the first one alone by 2 k bases, so v1 cuts a copy of
    multiplicity G - 1 off.  Searched with 1 to 3 descending rounds."""
    rng = np.random.default_rng(6200)
    probs, pats = [], []
    for p in range(200):
        G = R200_GS[p % 4]
        n = int(rng.integers(400, R200_NMAX[G] + 1))
        anc = ab.rand_seq(rng, n)
        c = int(rng.integers(n // 2 - 20, n // 2 + 21))
        k = int(rng.integers(12, 21))
        seqs = []
        for g in range(G):
            lo = int(rng.integers(0, n // 8))
            hi = int(rng.integers(7 * n // 8, n + 1))
            s = bytearray(ab.mutate(rng, anc, 0.03))
            s[c - R200_FLANK:c + R200_FLANK] = anc[c - R200_FLANK:c + R200_FLANK]
            if g > 0:
                s[c:c] = anc[c:c + k] + anc[c - k:c]
            s = bytes(s[lo:len(s) - (n - hi)])
            seqs.append(ab.rc(s) if g % 3 == 2 else s)
        probs.append(tuple(seqs))
        pats.append(patterns_of(R200_ROUNDS[(p // 4) % 3]))
    return _case(probs, pats)


def masked_g3():
    c = ab.more_sequences(3, 0b101)
    return _case(c["problems"], patterns_of((9, 7)), mask=0b101, variants=("m0", "m2", "mG"))


def g9():
    c = ab.more_sequences(9)
    return _case(c["problems"], patterns_of((9, 7)))


RANK_ORDERS = {"w9": (9,), "w9_7": (9, 7), "w7_9": (7, 9), "w9_7_9": (9, 7, 9), "w7_7": (7, 7)}


def rank_order(name):
    rng = np.random.default_rng(6300)
    probs = [ab.partial_problem(rng, 3, 2400), ab.partial_problem(rng, 3, 1500), ab.partial_problem(rng, 3, 900)]
    return _case(probs, patterns_of(RANK_ORDERS[name]), variants=("m0",))


def degenerate():
    """G = 3: empty sequences, a sequence shorter than the longer seed but not the shorter one,
    identical sequences."""
    rng = np.random.default_rng(6400)
    pats = patterns_of((9, 7))
    L9, L7 = ab.seed_length(pats[0]), ab.seed_length(pats[1])
    assert L7 < L9
    x = ab.rand_seq(rng, 600)
    short = x[100:100 + L9 - 1]
    probs = [(b"", ab.rand_seq(rng, 500), b""), ab.partial_problem(rng, 3, 700), (b"", b"", b""), (x, short, x[50:400]),
             (x, x, x), (ab.rand_seq(rng, 400), b"", ab.rand_seq(rng, 30))]
    return _case(probs, pats)


def restart():
    """G = 3, a poly-A run of 1500 in every sequence of problem 1: MER_REPEAT_LIMIT restarts, the
    problem runs alone, rounds and v1 tail."""
    rng = np.random.default_rng(6500)
    a = ab.partial_problem(rng, 3, 900)
    probs = [ab.partial_problem(rng, 3, 1000), tuple(s[:200 + 50 * g] + b"A" * 1500 + s[200 + 50 * g:] for g, s in enumerate(a)),
             ab.partial_problem(rng, 3, 600)]
    return _case(probs, patterns_of((11, 9)))


FIND_CASES = {
    "r200": r200,
    "g3_mask101": masked_g3,
    "g9": g9,
    **{f"ranks_{k}": (lambda k=k: rank_order(k)) for k in RANK_ORDERS},
    "degenerate": degenerate,
    "restart": restart,
}


@functools.lru_cache(maxsize=None)
def find_case(name):
    return FIND_CASES[name]()


# ---- the tail-only lists -------------------------------------------------------------------------
OVERFLOW_ROWS = 120


def overflow_list():
    """G = 8, every match defined everywhere, starts so close that a match overlaps many others in
    every sequence: each pass appends about as many rows as it reads, the slice runs full."""
    rng = np.random.default_rng(6600)
    l, s = random_matchlist(rng, OVERFLOW_ROWS, 8, max_len=200, p_absent=0.0, start_span=400)
    return l, s.reshape(OVERFLOW_ROWS, 8)


@functools.lru_cache(maxsize=None)
def tail_cases():
    """name -> [(lengths, starts)] of one mums_recursion_tail_batch call (the same G in a call):
    anchor_batch_cases' lists (0, 1, 2, 16, 17, 200, 1000 rows at G = 2, 3, 8; the adversarial sort
    orders at 17, 500, 1000 rows; the row cap and one above) and the list that outgrows its slice."""
    out = dict(ab.tail_cases())
    out["overflow"] = [overflow_list()]
    return out


def tail_variants(G):
    return [(v, ml) for v in VARIANTS for ml in TAIL_MIN_LENGTHS]


# ---- the models ----------------------------------------------------------------------------------
def have_compiler():
    return sf.have_compiler()


def filters(lengths, starts, multiplicity, min_length):
    keep = lengths >= min_length
    if multiplicity:
        keep &= (starts != 0).sum(axis=1) == multiplicity
    return lengths[keep], starts[keep]


def model_tail(lengths, starts, multiplicity, min_length=MIN_LENGTH):
    starts = np.asarray(starts, dtype=np.int64)
    G = starts.shape[1]
    el, es = oracle.eliminate_overlaps(np.asarray(lengths, dtype=np.uint64), starts)
    return filters(el, np.asarray(es).reshape(len(el), G), multiplicity, min_length)


def model_problem(problem, patterns, table_size=40000, mask=None, variants=("m0", "mG"), min_length=MIN_LENGTH):
    """One problem through the models: rounds, table, the counters mums_anchor_batch_info reports
    and per variant the final list."""
    G = len(problem)
    if not patterns:
        empty = (np.zeros(0, dtype=np.uint64), np.zeros((0, G), dtype=np.int64))
        return dict(rounds=[], table=empty, table_entries=0, probes=0, collisions=0, restarts=0,
                    final={v: empty for v in variants})
    rounds = ab.model_rounds(problem, patterns, table_size, mask)
    table = (rounds[-1]["lengths"], np.asarray(rounds[-1]["starts"]).reshape(-1, G))
    return dict(rounds=rounds, table=table, table_entries=len(table[0]), probes=sum(r["probes"] for r in rounds),
                collisions=rounds[-1]["collisions"], restarts=ab.oracle_restarts(problem, patterns, table_size, mask),
                final={v: model_tail(table[0], table[1], VARIANTS[v](G), min_length) for v in variants})


@functools.lru_cache(maxsize=None)
def model_case(name):
    c = find_case(name)
    return [model_problem(p, pats, c["table_size"], c["mask"], c["variants"]) for p, pats in zip(c["problems"], c["patterns"])]


def digest_problem(m, variant):
    l, s = m["final"][variant]
    return dict(count=int(len(l)), list_md5=sf.list_md5(l, s), table_entries=int(m["table_entries"]),
                probes=int(m["probes"]), collisions=int(m["collisions"]), restarts=int(m["restarts"]))


def digest_case(name):
    ms = model_case(name)
    return {v: [digest_problem(m, v) for m in ms] for v in find_case(name)["variants"]}


def tail_key(variant, min_length):
    return f"{variant}_len{min_length}"


def digest_tail(name):
    out = {}
    for li, st in tail_cases()[name]:
        G = st.shape[1]
        el, es = model_tail(li, st, 0, 0)
        for v in VARIANTS:
            for ml in TAIL_MIN_LENGTHS:
                l, s = filters(el, es, VARIANTS[v](G), ml)
                out.setdefault(tail_key(v, ml), []).append(dict(count=int(len(l)), list_md5=sf.list_md5(l, s)))
    return out


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- tests/eo_model.cpp: the real std::sort on Match* ------------------------------------------------
@functools.lru_cache(maxsize=None)
def eo_model():
    os.makedirs(sf.BUILD, exist_ok=True)
    tmp = f"{EO_SO}.{os.getpid()}"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, os.path.join(ROOT, "tests", "eo_model.cpp")],
                   check=True)
    os.replace(tmp, EO_SO)
    L = ctypes.CDLL(EO_SO)
    L.model_eliminate_overlaps.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.model_eliminate_overlaps.restype = ctypes.c_uint64
    return L


def eo_model_tail(lengths, starts, multiplicity, min_length):
    M, G = starts.shape
    cap = 64 * M + 64
    lo = np.zeros(cap, dtype=np.uint64)
    so = np.zeros(cap * G, dtype=np.int64)
    l = np.ascontiguousarray(lengths, dtype=np.uint64)
    s = np.ascontiguousarray(starts, dtype=np.int64)
    k = eo_model().model_eliminate_overlaps(G, M, l.ctypes.data, s.ctypes.data, lo.ctypes.data, so.ctypes.data, cap)
    assert k <= cap
    return filters(lo[:k], so[:k * G].reshape(k, G), multiplicity, min_length)


# ---- recursion_lane.h on the host --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lane_shim():
    """tests/recursion_lane_shim.cpp: the header the device lanes run, compiled with g++."""
    os.makedirs(sf.BUILD, exist_ok=True)
    tmp = f"{LANE_SO}.{os.getpid()}"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, SHIM], check=True)
    os.replace(tmp, LANE_SO)
    L = ctypes.CDLL(LANE_SO)
    L.lane_slice_rows.restype = ctypes.c_uint64
    L.lane_slice_rows.argtypes = [ctypes.c_uint64, ctypes.c_int]
    L.lane_recursion_tail.restype = ctypes.c_uint64
    L.lane_recursion_tail.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def lane_tail(lengths, starts, multiplicity, min_length=MIN_LENGTH, cap=None):
    """The lane on one list in a slice of cap rows (None: room for everything):
    (lengths, starts, dict(dels, apps, overflow))."""
    n, G = starts.shape
    cap = 64 * n + 64 if cap is None else cap
    l = np.ascontiguousarray(lengths, dtype=np.uint64)
    s = np.ascontiguousarray(starts, dtype=np.int64)
    lo = np.zeros(cap + 1, dtype=np.uint64)
    so = np.zeros((cap + 1) * G, dtype=np.int64)
    info = np.zeros(3, dtype=np.uint64)
    k = lane_shim().lane_recursion_tail(G, n, cap, l.ctypes.data, s.ctypes.data, multiplicity, min_length, lo.ctypes.data,
                                        so.ctypes.data, info.ctypes.data)
    return lo[:k], so[:k * G].reshape(k, G), dict(dels=int(info[0]), apps=int(info[1]), overflow=bool(info[2]))


def lane_main_input(path, lists):
    """The stand-alone program's input: lists = [(G, cap, multiplicity, min_length, lengths, starts)]."""
    with open(path, "wb") as f:
        for G, cap, mult, ml, l, s in lists:
            np.array([G, len(l), cap, mult, ml], dtype=np.uint64).tofile(f)
            np.ascontiguousarray(l, dtype=np.uint64).tofile(f)
            np.ascontiguousarray(s, dtype=np.int64).tofile(f)


def lane_main_checksum(lengths, starts):
    h = 0
    for i in range(len(lengths)):
        h = (h * 1000003 + int(lengths[i])) % (1 << 64)
        for v in starts[i]:
            h = (h * 1000003 + (int(v) % (1 << 64))) % (1 << 64)
    return h


# ---- the device calls (test_gpu_recursion_batch.py) ---------------------------------------------------
def run_find_case(mh, case, multiplicity, min_length=MIN_LENGTH):
    """The case through mums_recursion_batch, one call per sequence count and distinct pattern
    tuple: (lists, info).  multiplicity: a number, or a function of G (VARIANTS)."""
    import libmems_amd
    problems, B = case["problems"], len(case["problems"])
    out = [None] * B
    info = {k: np.zeros(B, dtype=np.uint64) for k in ("matches", "table_entries", "probes", "collisions", "restarts")}
    groups = {}
    for p, pats in enumerate(case["patterns"]):
        groups.setdefault((len(problems[p]), pats), []).append(p)
    for (G, pats), idx in groups.items():
        if not pats:
            for p in idx:
                out[p] = libmems_amd.MatchList(np.zeros(0, dtype=np.uint64), np.zeros((0, G), dtype=np.int64))
            continue
        blob = b"".join(s for p in idx for s in problems[p])
        off = np.zeros(len(idx) * G + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for p in idx for s in problems[p]], dtype=np.uint64)
        pa = np.asarray(pats, dtype=np.uint64)
        mult = multiplicity(G) if callable(multiplicity) else int(multiplicity)
        mh._check(mh._lib.mums_recursion_batch(mh._ctx, len(idx), G, blob, off.ctypes.data, pa.ctypes.data, len(pa),
                                               mult, min_length))
        mh._batch_collect(idx, G, out, info)
    return out, info
