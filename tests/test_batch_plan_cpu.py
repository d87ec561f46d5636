"""libmems_amd/csrc/batch_plan.h, the host plan of mums_find_batch and mums_anchor_batch, compiled
with g++ (tests/batch_plan_shim.cpp) and held to a restatement of DESIGN.md §4d / §4e in Python:
which problems the lanes take, their order, and where their slices start.  No device."""
from __future__ import annotations

import ctypes
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import seed_family_cases as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(sf.BUILD, "libbatch_plan_shim.so")
pytestmark = pytest.mark.skipif(not sf.have_compiler(), reason="the plan is compiled with g++")

FIND = (10.0, lambda rounds: 1000.0)                    # kLaneUs, the cost of a problem run alone
ANCHOR = (18.0, lambda rounds: 915.0 * rounds + 380.0)  # kSingleUs * rounds + kTailUs
CAP = 200000
OK, TOO_MANY_SEQUENCES, TOO_MANY_SEED_MERS, TOO_MANY_SLOTS = range(4)


@functools.lru_cache(maxsize=None)
def shim():
    os.makedirs(sf.BUILD, exist_ok=True)
    tmp = f"{SO}.{os.getpid()}"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", tmp,
                    os.path.join(ROOT, "tests", "batch_plan_shim.cpp")], check=True)
    os.replace(tmp, SO)
    lib = ctypes.CDLL(SO)
    lib.batch_plan_run.restype = ctypes.c_int
    lib.batch_plan_run.argtypes = ([ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_double]
                                   + [ctypes.c_void_p] * 9)
    return lib


def header_plan(lens, G, rounds, cap, no_split, cost, first=7):
    """batch_plan.h on B = len(lens) / G problems; rounds = [(L, kbits)]."""
    B, R = len(lens) // G, len(rounds)
    seq_off = np.cumsum([first] + list(lens)).astype(np.uint64)
    L = np.array([r[0] for r in rounds], dtype=np.int32)
    kb = np.array([r[1] for r in rounds], dtype=np.int32)
    out = dict(recs=np.zeros(R * B, np.uint64), routed=np.zeros(B, np.uint8), order=np.zeros(B, np.uint32),
               mbase=np.zeros(R * (B * G + 1), np.uint32), N=np.zeros(R, np.uint64), Nall=np.zeros(R, np.uint64),
               obase=np.zeros(B, np.uint32), ocap=np.zeros(B, np.uint32), scalars=np.zeros(2, np.uint64))
    status = shim().batch_plan_run(B, G, seq_off.ctypes.data, R, L.ctypes.data, kb.ctypes.data, cap, int(no_split),
                                   cost[0], cost[1](R), *[a.ctypes.data for a in out.values()])
    assert status == OK
    got = {k: v.tolist() for k, v in out.items() if k != "scalars"}
    got["mbase"] = out["mbase"].reshape(R, B * G + 1).tolist()
    got["recs"] = out["recs"].reshape(R, B).tolist()
    got["lanes"] = bool(out["scalars"][0])
    got["ord_words"] = int(out["scalars"][1])
    return got


def stated_plan(lens, G, rounds, cap, no_split, cost):
    """The rule as DESIGN.md states it.  A sequence of n bases has max(n - L + 1, 0) seed-mers.  The
    sort key is the problem id above the 2w + 1 key bits; when it does not fit 64 bits in some
    round, or a problem has more than cap seed-mers in some round, the problem runs alone.  The
    others are taken largest first (all rounds' seed-mers, input order among equals), and the k
    largest of them run alone too, k the first minimum of lane cost x (size of the largest problem
    left) + alone cost x k.  Lane problems get consecutive record ranges per round and consecutive
    table slices of sum over rounds of floor(records / 2) words."""
    B, R = len(lens) // G, len(rounds)
    mers = lambda n, L: max(n - L + 1, 0)
    seq = lambda p: lens[p * G:(p + 1) * G]
    recs = [[sum(mers(n, L) for n in seq(p)) for p in range(B)] for L, _ in rounds]
    size = [sum(recs[r][p] for r in range(R)) for p in range(B)]
    id_bits = (max(B, 1) - 1).bit_length()
    lanes = all(kbits + id_bits <= 64 for _, kbits in rounds)
    alone = [not lanes or any(recs[r][p] > cap for r in range(R)) for p in range(B)]
    order = [p for p in range(B) if alone[p]] + sorted((p for p in range(B) if not alone[p]), key=lambda p: -size[p])
    if lanes and not no_split:
        k0 = sum(alone)
        left = [size[p] for p in order[k0:]] + [0]
        costs = [cost[0] * left[k] + cost[1](R) * k for k in range(len(left))]
        for p in order[k0:k0 + costs.index(min(costs))]:
            alone[p] = True
    mbase, N = [], []
    for L, _ in rounds:
        row = [0]
        for p in range(B):
            for n in seq(p):
                row.append(row[-1] + (0 if alone[p] else mers(n, L)))
        mbase.append(row)
        N.append(row[-1])
    ocap = [0 if alone[p] else sum(recs[r][p] // 2 for r in range(R)) for p in range(B)]
    obase = [sum(ocap[:p]) for p in range(B)]
    return dict(recs=recs, routed=[int(a) for a in alone], order=order, mbase=mbase, N=N,
                Nall=[sum(recs[r]) for r in range(R)], obase=obase, ocap=ocap, lanes=lanes, ord_words=sum(ocap))


def check(lens, G, rounds, cap=CAP, no_split=False, cost=FIND):
    got = header_plan(lens, G, rounds, cap, no_split, cost)
    want = stated_plan(lens, G, rounds, cap, no_split, cost)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k], lens, G, rounds, cap, no_split)
    return got


W5 = (5, 11)    # a solid seed of weight 5: L, 2w + 1
W11 = (11, 23)


def test_empty_and_single():
    assert check([], 2, [W5])["order"] == []
    assert check([], 2, [W5, W11], cost=ANCHOR)["N"] == [0, 0]
    for cost in (FIND, ANCHOR):
        assert check([14, 15], 2, [W5], cost=cost)["routed"] == [0]
        # every sequence shorter than the seed: no record anywhere
        got = check([4, 3, 0, 4], 2, [W5], cost=cost)
        assert got["N"] == [0] and got["Nall"] == [0] and got["mbase"] == [[0] * 5] and got["ord_words"] == 0


def test_a_round_without_records_beside_one_with():
    got = check([7, 10, 9, 8, 10, 10], 2, [W11, W5], cost=ANCHOR)
    assert got["N"] == [0, 9 + 9 + 12] and got["ocap"] == [4, 4, 6]
    got = check([7, 10, 9, 8, 10, 10], 2, [W5, W11], cost=ANCHOR)
    assert got["N"] == [30, 0] and got["mbase"][1] == [0] * 7


def test_equal_sizes_keep_input_order():
    assert check([30, 30] * 6, 2, [W5])["order"] == list(range(6))
    # (12 + 20 = 16 + 16 seed-mers; the larger problem 2 goes first)
    assert check([16, 24, 20, 20, 40, 40, 24, 16], 2, [W5], no_split=True)["order"] == [2, 0, 1, 3]
    assert check([30, 30] * 5, 2, [W5, W11], cost=ANCHOR)["order"] == list(range(5))


def pair(size, L=5):
    """two sequences with `size` seed-mers of length L between them"""
    return [size // 2 + L - 1, size - size // 2 + L - 1]


def test_first_minimum_of_the_cost_wins():
    # k = 0 and k = 1 both cost 1500 (k = 2: 2000): nothing runs alone
    assert check(pair(150) + pair(50), 2, [W5])["routed"] == [0, 0]
    assert check(pair(50) + pair(150), 2, [W5])["routed"] == [0, 0]
    # k = 1 and k = B = 2 both cost 2000 (k = 0: 2500): the smallest stays in the lanes
    assert check(pair(100) + pair(250), 2, [W5])["routed"] == [0, 1]
    # k = B is the only minimum (4000, 4000, 2000): everything runs alone
    got = check(pair(400) + pair(300), 2, [W5])
    assert got["routed"] == [1, 1] and got["N"] == [0]
    # k = k0 = 1, a problem above the cap in front: 10 x 99 against 10 x 1 + 1000
    got = check(pair(99) + pair(300) + pair(1), 2, [W5], cap=299)
    assert got["routed"] == [0, 1, 0] and got["order"] == [1, 0, 2]
    # the anchor constants, two rounds (alone: 2210): k = 0 and k = 9 both cost 21690, k = 1 ... 8 and 10 more.
    # Sizes over both rounds: 2 (a + b) - 18 for sequences of 6 and more, 2 b - 9 beside a sequence of 4.
    two = [(5, 11), (6, 13)]
    lens = [306, 306] + [305, 306] * 8 + [4, 55]
    got = check(lens, 2, two, cost=ANCHOR)
    assert [got["recs"][0][p] + got["recs"][1][p] for p in (0, 1, 9)] == [1206, 1204, 101]
    assert got["routed"] == [0] * 10
    # one seed-mer more in the largest: k = 9 is the only minimum
    assert check([306, 307] + lens[2:], 2, two, cost=ANCHOR)["routed"] == [1] * 9 + [0]
    # k = B alone: two problems of 400 and 300 per round cost 18 x 800 in the lanes, 2 x 2210 alone
    assert check(pair(400) + pair(300), 2, [W5, W5], cost=ANCHOR)["routed"] == [1, 1]
    # k = k0 = 0 alone, one round (alone: 1295): 18 x 60 is less than anything with a problem alone
    assert check(pair(60) + pair(50), 2, [W5], cost=ANCHOR)["routed"] == [0, 0]


@pytest.mark.parametrize("cost", [FIND, ANCHOR])
def test_problem_above_the_cap(cost):
    small = [5, 4]   # one seed-mer
    got = check(small + pair(40) + small + [4, 4], 2, [W5], cap=1, cost=cost)
    assert got["routed"] == [0, 1, 0, 0] and got["order"] == [1, 0, 2, 3] and got["N"] == [2]
    got = check(small + pair(40) + small + [4, 4], 2, [W5], cap=0, cost=cost)
    assert got["routed"] == [1, 1, 1, 0] and got["order"] == [0, 1, 2, 3] and got["N"] == [0]
    # above the cap in the second round only
    got = check([12, 12, 30, 30], 2, [W11, W5], cap=4, cost=cost)
    assert got["routed"] == [1, 1] and got["recs"] == [[4, 40], [16, 52]]


def test_no_split_keeps_every_problem_up_to_the_cap():
    lens = pair(400) + pair(300) + pair(30000)
    for cost, rounds in ((FIND, [W5]), (ANCHOR, [W5, W11])):
        assert check(lens, 2, rounds, cost=cost)["routed"] == [1, 1, 1]
        assert check(lens, 2, rounds, no_split=True, cost=cost)["routed"] == [0, 0, 0]
        assert check(lens, 2, rounds, cap=20000, no_split=True, cost=cost)["routed"] == [0, 0, 1]


def test_keys_that_do_not_fit_64_bits():
    w31 = (31, 63)
    got = check([40, 40] * 3, 2, [w31])   # two id bits: 65
    assert not got["lanes"] and got["routed"] == [1, 1, 1] and got["N"] == [0] and got["Nall"] == [60]
    got = check([40, 40] * 2, 2, [w31])   # one id bit: 64
    assert got["lanes"] and got["routed"] == [0, 0]
    got = check([40, 40] * 3, 2, [W5, w31], cost=ANCHOR)   # one round is enough
    assert not got["lanes"] and got["routed"] == [1, 1, 1]


def test_random_sweep():
    rng = random.Random(20261021)
    seeds = [(5, 11), (7, 11), (9, 15), (11, 23), (15, 27), (31, 63)]
    for _ in range(400):
        B, G, R = rng.randint(0, 12), rng.randint(2, 4), rng.randint(1, 3)
        top = rng.choice([8, 20, 60])
        lens = [rng.randint(0, top) for _ in range(B * G)]
        rounds = [rng.choice(seeds[:5] if rng.random() < 0.9 else seeds) for _ in range(R)]
        cost = (rng.choice([10.0, 18.0, 500.0]), rng.choice(FIND[1:] + ANCHOR[1:] + (lambda r: 20.0 * r,)))
        check(lens, G, rounds, cap=rng.choice([CAP, 0, 1, 30, 100]), no_split=rng.random() < 0.3, cost=cost)


def test_size_refusals():
    """The statuses, on inputs that need no large arrays: B * G + 1 >= 2^32 before seq_off is read."""
    lib, nul, scal = shim(), None, np.zeros(2, np.uint64)
    L, kb = np.array([5], np.int32), np.array([11], np.int32)
    run = lambda B, G, off: lib.batch_plan_run(B, G, off, 1, L.ctypes.data, kb.ctypes.data, CAP, 0, 10.0, 1000.0, nul, nul,
                                               nul, nul, nul, nul, nul, nul, scal.ctypes.data)
    assert run(1 << 26, 64, None) == TOO_MANY_SEQUENCES
    # two sequences of 2^31 bases each: 2^32 - 8 seed-mers is past the 32-bit index space
    off = np.array([0, 1 << 31, 1 << 32], np.uint64)
    assert run(1, 2, off.ctypes.data) == TOO_MANY_SEED_MERS
