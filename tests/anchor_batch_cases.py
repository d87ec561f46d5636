"""mums_anchor_batch / mums_anchor_tail_batch (batch.hip's carried rounds, anchor.hip's tail; DESIGN.md
§4e): the cases shared by test_anchor_batch_cpu.py, test_gpu_anchor_batch.py and
golden/make_anchor_batch_golden.py, the composition of the project's CPU models that gives their
expected values, and the digests golden/anchor_batch_cases.json records.

Expected values: tests/seed_family_model.c gives a problem's table round by round,
tests/eo2_model.cpp EliminateOverlaps_v2 on it, a numpy `>= min_length` the filter
(seed_family_cases.chain_of_model is this composition for one list).  Seeded generators, no files,
no GPU.  A find case is a dict: problems (tuples of bytes), patterns (per problem the seed patterns
in round order; empty: seed weight 0, no search), table_size, mask (None: MemHash)."""
from __future__ import annotations

import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np

import seed_family_cases as sf
import test_eliminate_overlaps_v2_cpu as eo2
from oracle import oracle
from test_eliminate_overlaps_cpu import SORT_ORDERS, adversarial_keys, random_matchlist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmems_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "anchor_batch_cases.json")
LANE_SO = os.path.join(sf.BUILD, "libanchor_lane_shim.so")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
MIN_LENGTH = sf.CHAIN_MIN_LENGTH   # MIN_ANCHOR_LENGTH + 3 (ProgressiveAligner.cpp:659)
VARIANTS = {"eb0": False, "eb1": True}   # eliminate_both


# ---- constants read out of the sources -------------------------------------------------------
def source_constants():
    """tail_cap (rows of one list the tail's lane takes), cap (seed-mers of one problem and round
    the lanes take), pool_floor (the floor of the entry pool; the pool of an anchor batch is
    pool_cap(sum over the rounds of the lanes' seed-mers))."""
    capi = open(os.path.join(CSRC, "mums_capi.hip")).read()
    tail_cap = int(re.search(r"constexpr uint64_t kAnchorTailCap = (\d+);", capi).group(1))
    body = capi[capi.index("static uint64_t batch_problem_cap()"):]
    cap = int(re.search(r"strtoull\(e, nullptr, 10\) : (\d+)ull;", body[:body.index("}")]).group(1))
    m = re.search(r"const uint64_t pool_cap64 = std::min<uint64_t>\(Nsum / 2 \+ 1, std::max<uint64_t>\(Nsum / 8, "
                  r"1ull << (\d+)\)\);", capi)
    return dict(tail_cap=tail_cap, cap=cap, pool_floor=1 << int(m.group(1)))


def pool_cap(nsum, pool_floor):
    return min(nsum // 2 + 1, max(nsum // 8, pool_floor))


def seed_length(seed):
    return int(oracle.lib().oracle_seed_length(seed))


def seedmers(problem, seed):
    L = seed_length(seed)
    return sum(max(len(s) - L + 1, 0) for s in problem)


def default_weight(problem):
    """getDefaultSeedWeight of the mean length (ProgressiveAligner.cpp:615-616)."""
    return int(oracle.lib().oracle_default_seed_weight(sum(len(s) for s in problem) // max(len(problem), 1)))


def family(w, ranks=(0, 1, 2)):
    return tuple(oracle.get_seed(w, r) for r in ranks) if w else ()


# ---- sequence generators (restated from test_gpu_batch.py: a gpu module is not imported) ------
def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    hit = rng.random(len(a)) < rate
    a[hit] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
    return a.tobytes()


def rc(seq):
    return seq.translate(COMP)[::-1]


def pair(rng, n, rate=0.1, flip=False):
    a = rand_seq(rng, n)
    b = mutate(rng, a, rate)
    return (a, rc(b) if flip else b)


def partial_problem(rng, G, n):
    """G sequences sharing parts of one ancestor: subset matches with NO_MATCH columns."""
    anc = rand_seq(rng, n)
    out = []
    for g in range(G):
        lo = int(rng.integers(0, n // 3))
        hi = int(rng.integers(2 * n // 3, n))
        s = mutate(rng, anc[lo:hi], 0.03)
        out.append(rc(s) if g % 3 == 2 else s)
    return tuple(out)


# ---- the find cases ---------------------------------------------------------------------------
def _case(problems, patterns, table_size=40000, mask=None, variants=("eb0", "eb1")):
    if not isinstance(patterns, list):
        patterns = [tuple(patterns)] * len(problems)
    return dict(problems=[tuple(p) for p in problems], patterns=[tuple(x) for x in patterns], table_size=table_size,
                mask=mask, variants=tuple(variants))


@functools.lru_cache(maxsize=None)
def a200_problems():
    """200 gap pairs of 0 .. 4000 bp, 5 % substitutions, every second pair with a planted 100-bp
    repeat, half of the partners reverse-complemented."""
    rng = np.random.default_rng(4200)
    out = []
    for p in range(200):
        n = int(rng.integers(0, 4001))
        a = bytearray(rand_seq(rng, n))
        if p % 2 == 1 and n >= 400:
            i, j = int(rng.integers(0, n // 2 - 100)), int(rng.integers(n // 2, n - 100))
            a[j:j + 100] = a[i:i + 100]
        a = bytes(a)
        b = mutate(rng, a, 0.05)
        out.append((a, rc(b) if (p // 2) % 2 == 1 else b))
    return out


def a200():
    probs = a200_problems()
    return _case(probs, [family(default_weight(p)) for p in probs])


def crowded(table_size):
    probs = a200_problems()[40:60]
    return _case(probs, [family(default_weight(p)) for p in probs], table_size=table_size, variants=("eb0",))


RANK_ORDERS = {"r0": (0,), "r012": (0, 1, 2), "r201": (2, 0, 1), "r01201": (0, 1, 2, 0, 1)}


def rank_order(name):
    rng = np.random.default_rng(4300)
    probs = [pair(rng, 3000, 0.05), pair(rng, 2500, 0.05, flip=True), pair(rng, 1800, 0.08), pair(rng, 900, 0.05)]
    return _case(probs, family(9, RANK_ORDERS[name]), variants=("eb0",))


def more_sequences(G, mask=None):
    rng = np.random.default_rng(4400 + G)
    probs = [partial_problem(rng, G, 1200), partial_problem(rng, G, 700), partial_problem(rng, G, 1500)]
    return _case(probs, family(7), mask=mask)


def degenerate():
    """Empty sequences; a sequence shorter than rank 1's seed but not rank 0's; two identical
    sequences; a match ending at the junction between two problems (the bytes after each sequence
    continue the same bases)."""
    rng = np.random.default_rng(4500)
    pats = family(7)
    L0, L1 = seed_length(pats[0]), seed_length(pats[1])
    assert L0 < L1
    x = rand_seq(rng, 600)
    short = x[100:100 + L1 - 1]
    r = rand_seq(rng, 900)
    probs = [(b"", rand_seq(rng, 500)), pair(rng, 700), (b"", b""), (x, short), (x, x), (r[0:300], r[300:400] + r[0:300]),
             (r[300:700], mutate(rng, r[300:700], 0.03)), (rand_seq(rng, 400), b"")]
    return _case(probs, pats)


def restart():
    """A poly-A run of 1500 and an N run of 1200 in both sequences: MER_REPEAT_LIMIT restarts."""
    rng = np.random.default_rng(4600)
    a, b = pair(rng, 800)
    c, d = pair(rng, 900)
    probs = [pair(rng, 1000), (a[:400] + b"A" * 1500 + a[400:], b[:300] + b"A" * 1500 + b[300:]), pair(rng, 500),
             (c[:200] + b"N" * 1200 + c[200:], d[:500] + b"N" * 1200 + d[500:]), pair(rng, 1200, flip=True)]
    return _case(probs, family(9), variants=("eb0",))


CAP_EXTRAS = (-1, 0, 1)


def cap_case(cap=200000):
    """Problems just under, at and over the seed-mer cap in their largest round (the shortest seed
    of the family), among small ones."""
    rng = np.random.default_rng(4700)
    pats = family(11)
    L = min(seed_length(s) for s in pats)
    base = rand_seq(rng, cap // 2 + 200)
    mut = mutate(rng, base, 0.05)
    probs = [pair(rng, 800)]
    for extra in CAP_EXTRAS:
        n0 = cap // 2 + (L - 1)
        n1 = cap - (n0 - L + 1) + (L - 1) + extra
        probs.append((base[:n0], mut[:n1]))
    probs.append(pair(rng, 600, flip=True))
    return _case(probs, pats, variants=("eb0",))


POOL_CLASSES = 16
POOL_PROBLEMS = (1 << 16) + 64


@functools.lru_cache(maxsize=None)
def pool_case():
    """POOL_PROBLEMS problems (x, x) with x as long as the family's rank-0 seed, run in the rank
    order (1, 0): round 0's seed is longer than x (no seed-mer, no entry), round 1 gives every
    problem two seed-mers, one probe and one entry, so the pool (its floor) runs full in round 1
    for exactly 64 lanes.  x rotates over 16 strings (`classes`)."""
    pats = family(5, (1, 0))
    L = seed_length(pats[1])
    assert seed_length(pats[0]) > L
    rng = np.random.default_rng(4800)
    classes = []
    while len(classes) < POOL_CLASSES:
        x = rand_seq(rng, L)
        if x not in classes:
            classes.append(x)
    probs = [(classes[p % POOL_CLASSES],) * 2 for p in range(POOL_PROBLEMS)]
    return dict(_case(probs, pats, variants=("eb0",)), classes=classes)


FIND_CASES = {
    "a200": a200,
    "crowded_T7": lambda: crowded(7),
    "crowded_T1": lambda: crowded(1),
    **{f"ranks_{k}": (lambda k=k: rank_order(k)) for k in RANK_ORDERS},
    "g3": lambda: more_sequences(3),
    "g9": lambda: more_sequences(9),
    "g3_mask101": lambda: more_sequences(3, 0b101),
    "degenerate": degenerate,
    "restart": restart,
    "cap": cap_case,
}


@functools.lru_cache(maxsize=None)
def find_case(name):
    return FIND_CASES[name]()


# ---- the tail-only lists -------------------------------------------------------------------------
TAIL_MS = (0, 1, 2, 16, 17, 200, 1000)
TAIL_GS = (2, 3, 8)
ADVERSARIAL_MS = (17, 500, 1000)


def adversarial_list(order, M, seed=0):
    """A G = 2 list whose sequence-0 LeftEnds are adversarial_keys(order, M) (half of them on the
    reverse strand), short lengths so that neighbours overlap but the walk stays short."""
    rng = np.random.default_rng(5000 + M + seed)
    lengths = rng.integers(1, 40, size=M).astype(np.uint64)
    starts = np.zeros((M, 2), dtype=np.int64)
    starts[:, 0] = adversarial_keys(order, M).astype(np.int64) * np.where(rng.random(M) < 0.5, -1, 1)
    starts[:, 1] = rng.integers(1, 50 * M + 2, size=M) * np.where(rng.random(M) < 0.3, -1, 1)
    return lengths, starts


@functools.lru_cache(maxsize=None)
def tail_cases(tail_cap=None):
    """name -> [(lengths, starts)] of one mums_anchor_tail_batch call (the same G in a call)."""
    tail_cap = tail_cap or source_constants()["tail_cap"]
    out = {}
    for G in TAIL_GS:
        lists = []
        for M in TAIL_MS:
            rng = np.random.default_rng(5100 + 10 * M + G)
            l, s = random_matchlist(rng, M, G, start_span=max(4 * M, 40))
            lists.append((l, s.reshape(M, G)))
        out[f"random_g{G}"] = lists
    wide = []   # few overlaps: most rows survive, the order of the last pass shows in the result
    for M in (17, 200, 1000):
        rng = np.random.default_rng(5300 + M)
        l, s = random_matchlist(rng, M, 3, max_len=60, start_span=100 * M)
        wide.append((l, s.reshape(M, 3)))
    out["random_wide_g3"] = wide
    out["adversarial"] = [adversarial_list(o, M) for o in SORT_ORDERS for M in ADVERSARIAL_MS]
    caps = []
    for M in (tail_cap, tail_cap + 1):
        rng = np.random.default_rng(5200 + M)
        l, s = random_matchlist(rng, M, 3, start_span=6 * M)
        caps.append((l, s.reshape(M, 3)))
    out["tail_cap"] = caps
    return out


# ---- the models ----------------------------------------------------------------------------------
def have_compiler():
    return sf.have_compiler()


@functools.lru_cache(maxsize=None)
def models():
    return sf.load_model(), eo2.load_model()


def model_tail(lengths, starts, eliminate_both, min_length=MIN_LENGTH):
    el, es, _ = eo2.model_eo2(models()[1], np.asarray(lengths, dtype=np.uint64), np.asarray(starts, dtype=np.int64), None,
                              eliminate_both)
    keep = el >= min_length
    return el[keep], es[keep]


def model_rounds(problem, patterns, table_size=40000, mask=None):
    kw = dict(table_size=table_size, masked=mask is not None, seq_mask=mask or 0)
    return sf.run_model(models()[0], [(list(problem), pat, kw) for pat in patterns])


def oracle_restarts(problem, patterns, table_size=40000, mask=None):
    return sum(int(oracle.find_matches(list(problem), pat, table_size=table_size, masked=mask is not None,
                                       seq_mask=mask or 0)[2]["restarts"]) for pat in patterns)


def model_problem(problem, patterns, table_size=40000, mask=None, variants=("eb0", "eb1"), min_length=MIN_LENGTH):
    """One problem through the models: rounds (seed_family_model's per-round dicts), table, the
    counters mums_anchor_batch_info reports and per variant the final list."""
    G = len(problem)
    if not patterns:
        empty = (np.zeros(0, dtype=np.uint64), np.zeros((0, G), dtype=np.int64))
        return dict(rounds=[], table=empty, table_entries=0, probes=0, collisions=0, restarts=0,
                    final={v: empty for v in variants})
    rounds = model_rounds(problem, patterns, table_size, mask)
    table = (rounds[-1]["lengths"], rounds[-1]["starts"])
    return dict(rounds=rounds, table=table, table_entries=len(table[0]), probes=sum(r["probes"] for r in rounds),
                collisions=rounds[-1]["collisions"], restarts=oracle_restarts(problem, patterns, table_size, mask),
                final={v: model_tail(table[0], table[1], VARIANTS[v], min_length) for v in variants})


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


def digest_tail(name):
    return {v: [dict(count=int(len(l)), list_md5=sf.list_md5(l, s)) for l, s in
                (model_tail(li, st, VARIANTS[v]) for li, st in tail_cases()[name])] for v in VARIANTS}


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- anchor_lane.h on the host --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lane_shim():
    """tests/anchor_lane_shim.cpp: the header the device lanes run, compiled with g++."""
    os.makedirs(sf.BUILD, exist_ok=True)
    tmp = f"{LANE_SO}.{os.getpid()}"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp,
                    os.path.join(ROOT, "tests", "anchor_lane_shim.cpp")], check=True)
    os.replace(tmp, LANE_SO)
    L = ctypes.CDLL(LANE_SO)
    L.lane_anchor_tail.restype = ctypes.c_uint64
    L.lane_anchor_tail.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    L.lane_std_sort_ids.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    return L


def lane_tail(lengths, starts, eliminate_both, min_length=MIN_LENGTH):
    n, G = starts.shape
    l = np.ascontiguousarray(lengths, dtype=np.uint64)
    s = np.ascontiguousarray(starts, dtype=np.int64)
    lo = np.zeros(n + 1, dtype=np.uint64)
    so = np.zeros((n + 1) * G, dtype=np.int64)
    k = lane_shim().lane_anchor_tail(G, n, l.ctypes.data, s.ctypes.data, int(eliminate_both), min_length, lo.ctypes.data,
                                     so.ctypes.data)
    return lo[:k], so[:k * G].reshape(k, G)


def lane_sort_ids(keys, depth=-1):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    ids = np.zeros(len(keys), dtype=np.uint32)
    lane_shim().lane_std_sort_ids(keys.ctypes.data, len(keys), depth, ids.ctypes.data)
    return ids


# ---- the device calls (test_gpu_anchor_batch.py) ----------------------------------------------------
def run_find_case(mh, case, eliminate_both, min_length=MIN_LENGTH):
    """The case through mums_anchor_batch, one call per distinct pattern tuple: (lists, info)."""
    problems, B = case["problems"], len(case["problems"])
    G = len(problems[0])
    out = [None] * B
    info = {k: np.zeros(B, dtype=np.uint64) for k in ("matches", "table_entries", "probes", "collisions", "restarts")}
    groups = {}
    for p, pats in enumerate(case["patterns"]):
        groups.setdefault(pats, []).append(p)
    for pats, idx in groups.items():
        if not pats:   # seed weight 0: no search (ProgressiveAligner.cpp:626-633)
            import libmems_amd
            for p in idx:
                out[p] = libmems_amd.MatchList(np.zeros(0, dtype=np.uint64), np.zeros((0, G), dtype=np.int64))
            continue
        blob = b"".join(s for p in idx for s in problems[p])
        off = np.zeros(len(idx) * G + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for p in idx for s in problems[p]], dtype=np.uint64)
        pa = np.asarray(pats, dtype=np.uint64)
        mh._check(mh._lib.mums_anchor_batch(mh._ctx, len(idx), G, blob, off.ctypes.data, pa.ctypes.data, len(pa),
                                            int(eliminate_both), min_length))
        mh._anchor_collect(idx, G, out, info)
    return out, info
