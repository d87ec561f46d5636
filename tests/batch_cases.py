"""mums_find_batch (batch.hip, host side in mums_capi.hip): the inputs that reach the parts of the
lanes' replay no random ACGT pair does.  The lanes restate the reference a second time (their
own nucleotide table, MheCompare / Contains / lower_bound, ExtendMatch, HashMatch and
MaskedMemHash acceptance, their own routing, pool and buffers), so the inputs that pin the
single-find path say nothing about them.  Shared by test_batch_cases_cpu.py, which holds every
case to the path it exists for with the oracle and the constants parsed out of the sources, and
test_gpu_batch_paths.py, which compares the device with the oracle bit for bit.

Plain data and code, fixed seeds, no GPU.  A case is a dict: problems (tuples of bytes), seed
(pattern), table_size, mask (None: MemHash) and what its reach conditions need.

Two branches of batch_replay_kernel are left alone on purpose: `n >= ord_cap` and `flag = 4`.
Both are unreachable by construction (an entry needs a probe and a probe two records, so a
problem of r records never holds more than r / 2 entries; maxlen keeps ExtendMatch's seed inside
its sequence), and no input is built to provoke them."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

import repeat_inputs
from oracle import oracle
from test_gpu_batch import mutate, pair, partial_problem, rand_seq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libmems_amd", "csrc")
ACGT = b"ACGT"


# ---- the constants the cases were chosen for, read out of the sources -----------------------
def source_constants(capi_text=None):
    """repeat_limit (kRepeatLimit), cap (seed-mers of one problem the lanes take), pool_floor
    (the floor of the entry pool) and ladder ([(largest G, instantiation)], the last entry the
    `else`) as mums_internal.h, mums_capi.hip and batch.hip state them.  A constant that moves
    fails the CPU reach tests instead of leaving a GPU case off its path."""
    internal = open(os.path.join(CSRC, "mums_internal.h")).read()
    capi = capi_text if capi_text is not None else open(os.path.join(CSRC, "mums_capi.hip")).read()
    batch = open(os.path.join(CSRC, "batch.hip")).read()
    repeat_limit = int(re.search(r"constexpr int kRepeatLimit\s*=\s*(\d+);", internal).group(1))
    body = capi[capi.index("static uint64_t batch_problem_cap()"):]
    cap = int(re.search(r"strtoull\(e, nullptr, 10\) : (\d+)ull;", body[:body.index("}")]).group(1))
    m = re.search(r"const uint64_t pool_cap64 = std::min<uint64_t>\(N / 2 \+ 1, std::max<uint64_t>\(N / 8, "
                  r"1ull << (\d+)\)\);", capi)
    pool_floor = 1 << int(m.group(1))
    launch = batch[batch.index("hipError_t launch_batch_replay("):]
    launch = launch[:launch.index("return hipGetLastError();")]
    ladder = [(int(g), int(mg)) for g, mg in
              re.findall(r"if \(b\.G <= (\d+)\) hipLaunchKernelGGL\(batch_replay_kernel<(\d+)>", launch)]
    last = re.search(r"else hipLaunchKernelGGL\(batch_replay_kernel<(\d+)>", launch)
    ladder.append((int(last.group(1)), int(last.group(1))))
    assert "gs > (uint32_t)kRepeatLimit" in batch and "const bool lanes = kbits + pbits <= 64;" in capi
    return dict(repeat_limit=repeat_limit, cap=cap, pool_floor=pool_floor, ladder=ladder)


def instantiation(G, ladder):
    """The MG of batch_replay_kernel<MG> launch_batch_replay takes for G sequences."""
    for top, mg in ladder:
        if G <= top:
            return mg
    raise ValueError(f"G = {G} above the ladder")


def ceil_log2(n):
    return 0 if n <= 1 else (n - 1).bit_length()


def seed_length(seed):
    return int(oracle.lib().oracle_seed_length(seed))


def seed_weight(seed):
    return bin(seed).count("1")


def seedmers(problem, seed):
    L = seed_length(seed)
    return sum(max(len(s) - L + 1, 0) for s in problem)


def sort_bits(seed, B):
    """Bits of the batch's sort key: 2w + 1 of the seed key and the problem id above it."""
    return 2 * seed_weight(seed) + 1 + ceil_log2(B)


def pool_cap(N, pool_floor):
    """The entry pool of a lanes' pass over N seed-mers (pool_cap64 of mums_find_batch)."""
    return min(N // 2 + 1, max(N // 8, pool_floor))


def find(problem, seed, table_size=40000, mask=None):
    return oracle.find_matches(list(problem), seed, table_size=table_size, masked=mask is not None, seq_mask=mask or 0)


def in_lanes(problem, seed, B, consts, stats=None):
    """Under MUMS_DEV_BATCH_NO_SPLIT=1 a lane replays the problem to its end iff it is within the
    cap, the sort key fits 64 bits and no masked-key group is above the repeat limit (the
    largest group is the same for every table size and mask)."""
    if stats is None:
        stats = find(problem, seed)[2]
    return (seedmers(problem, seed) <= consts["cap"] and sort_bits(seed, B) <= 64 and
            int(stats["max_group"]) <= consts["repeat_limit"])


# ---- A. the lanes' nucleotide table ----------------------------------------------------------
FOLD = bytearray(b"A" * 256)   # BasicDNATable, SortedMerList.cpp:29-47
for _c in b"cCbByY":
    FOLD[_c] = ord("C")
for _c in b"gGsSkK":
    FOLD[_c] = ord("G")
for _c in b"tT":
    FOLD[_c] = ord("T")
FOLD = bytes(FOLD)
ALPHABET_BYTES = [v for v in range(256) if v != ord("-")]


def alphabet_problem(v, n=400, density=0.5, positions=None):
    """(base with byte v at `density` of the positions holding the letter v folds to -- or at
    `positions` of them --, base with 2 % substitutions)."""
    rng = np.random.default_rng(2000 + v)
    base = rand_seq(rng, n)
    other = mutate(rng, base, 0.02)
    a = np.frombuffer(base, dtype=np.uint8).copy()
    at = np.flatnonzero(a == FOLD[v])
    if positions is None:
        at = at[rng.random(len(at)) < density]
    else:
        at = rng.choice(at, size=positions, replace=False)
    a[at] = v
    return (a.tobytes(), other)


@functools.lru_cache(maxsize=None)
def alphabet():
    return dict(problems=[alphabet_problem(v) for v in ALPHABET_BYTES], seed=oracle.get_seed(7), table_size=40000,
                mask=None, bytes=ALPHABET_BYTES)


def wrong_foldings(problem, v):
    """The problem with v folded beforehand to each of the three letters it does not fold to."""
    return [(chr(w), (problem[0].replace(bytes([v]), bytes([w])), problem[1])) for w in ACGT if w != FOLD[v]]


def unnoticed_foldings(problems, byte_values, seed):
    """[(v, wrong letter)] whose answer (list and counters) equals the right one."""
    out = []
    for v, prob in zip(byte_values, problems):
        rl, rs, st = find(prob, seed)
        for letter, wrong in wrong_foldings(prob, v):
            wl, ws, wst = find(wrong, seed)
            if (np.array_equal(rl, wl) and np.array_equal(rs, ws) and wst["probes"] == st["probes"] and
                    wst["collision_count"] == st["collision_count"]):
                out.append((v, letter))
    return out


# ---- B. every instantiation of batch_replay_kernel --------------------------------------------
INSTANTIATION_CASES = [(5, 40000), (8, 40000), (8, 7), (16, 40000), (17, 40000), (32, 40000), (33, 40000), (64, 40000),
                       (64, 7)]
INSTANTIATION_OF = {5: 8, 8: 8, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}
# ancestor lengths of the three problems: 600 up to 8 sequences, shorter above (the lanes of one
# wave run one after the other, and a GPU test of this suite stays under half a second)
INSTANTIATION_SIZES = {5: (600, 560, 640), 8: (600, 560, 640), 16: (300, 280, 320), 17: (250, 230, 270),
                       32: (150, 140, 160), 33: (150, 140, 160), 64: (120, 100, 110)}


@functools.lru_cache(maxsize=None)
def instantiation_case(G, table_size=40000):
    """Three problems of G sequences cut from one ancestor each, 3 % substitutions, every third
    sequence reverse-complemented (so are 32, 35, ... of the wide ones)."""
    rng = np.random.default_rng(300 + G)
    problems = [partial_problem(rng, G, n) for n in INSTANTIATION_SIZES[G]]
    return dict(problems=problems, seed=oracle.get_seed(7), table_size=table_size, mask=None, G=G)


# ---- C. MaskedMemHash acceptance at 33 and 64 genomes -----------------------------------------
def mask_of(S, G):
    """Genome 0 is the most significant of the G bits (MaskedMemHash.cpp:38-63)."""
    return sum(1 << (G - 1 - g) for g in S)


def reversed_mask_of(S, G):
    return sum(1 << g for g in S)


def masked_problem(rng, G, S, n, rate, n_other):
    anc = rand_seq(rng, n)
    return tuple(mutate(rng, anc, rate) if g in S else rand_seq(rng, n_other) for g in range(G))


# (rate: the extension steps over single substitutions under the seed's don't-care positions, so
# the related genomes need 8 % of them to come apart into several matches; 64 genomes that all
# have to agree need 0.6 %)
MASK_CASES = {
    "g33_0_1_32": dict(G=33, S=(0, 1, 32), rate=0.08, rng=401, n=(900, 800), n_other=300),
    "g64_0_5_40": dict(G=64, S=(0, 5, 40), rate=0.08, rng=402, n=(900, 800), n_other=150),
    "g64_20_63": dict(G=64, S=(20, 63), rate=0.08, rng=402, n=(900, 800), n_other=150),
    "g64_all": dict(G=64, S=tuple(range(64)), rate=0.006, rng=402, n=(300, 260), n_other=0),
    "g64_accept_all": dict(G=64, S=(0, 5, 40), rate=0.08, rng=402, n=(300, 260), n_other=40, mask=0),
}


@functools.lru_cache(maxsize=None)
def mask_case(name):
    c = MASK_CASES[name]
    rng = np.random.default_rng(c["rng"])
    problems = [masked_problem(rng, c["G"], c["S"], n, c["rate"], c["n_other"]) for n in c["n"]]
    return dict(problems=problems, seed=oracle.get_seed(7), table_size=40000, G=c["G"], S=c["S"],
                mask=c.get("mask", mask_of(c["S"], c["G"])), reversed_mask=reversed_mask_of(c["S"], c["G"]))


# ---- D. the sort key at and over 64 bits ------------------------------------------------------
SORT_WIDTH_CASES = {"w31_b2": (31, 2, 64), "w31_b3": (31, 3, 65), "w30_b8": (30, 8, 64), "w30_b9": (30, 9, 65)}


@functools.lru_cache(maxsize=None)
def sort_width_case(name):
    w, B, bits = SORT_WIDTH_CASES[name]
    rng = np.random.default_rng(500 + w + B)
    problems = [pair(rng, 800, 0.01, flip=bool(p & 1)) for p in range(B)]
    return dict(problems=problems, seed=oracle.get_seed(w), table_size=40000, mask=None, bits=bits)


# ---- E. the entry pool running full -----------------------------------------------------------
POOL_CLASSES = 16
POOL_PROBLEMS = (1 << 16) + 64   # 64 above the pool's floor (test_batch_cases_cpu.py holds the parsed floor to it)


@functools.lru_cache(maxsize=None)
def pool_case():
    """POOL_PROBLEMS problems (x, x), x one seed long: two seed-mers, one probe, one entry each,
    so exactly 64 lanes find the pool full.  x rotates over 16 strings (`classes`)."""
    seed = oracle.get_seed(5)
    L = seed_length(seed)
    rng = np.random.default_rng(600)
    classes = []
    while len(classes) < POOL_CLASSES:
        x = rand_seq(rng, L)
        if x not in classes:
            classes.append(x)
    problems = [(classes[p % POOL_CLASSES],) * 2 for p in range(POOL_PROBLEMS)]
    return dict(problems=problems, seed=seed, table_size=40000, mask=None, classes=classes)


# ---- F. MER_REPEAT_LIMIT ----------------------------------------------------------------------
def poly_a_pair(r0, r1, rng_seed=700):
    rng = np.random.default_rng(rng_seed)
    a, b = pair(rng, 800)
    return (a[:400] + b"C" + b"A" * r0 + b"C" + a[400:], b[:300] + b"G" + b"A" * r1 + b"G" + b[300:])


def poly_a_triple(windows, rng_seed=701, L=15):
    """Three related sequences, sequence g with a run of A giving windows[g] all-A seed windows."""
    rng = np.random.default_rng(rng_seed)
    a = rand_seq(rng, 800)
    out = []
    for g, wn in enumerate(windows):
        s = mutate(rng, a, 0.03)
        cut = 300 + 100 * g
        out.append(s[:cut] + b"C" + b"A" * (wn + L - 1) + b"G" + s[cut:])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def repeat_limit_case():
    """G = 3 (the pairs carry an empty third sequence, which adds no seed-mer), one batch.
    expect: problem -> (largest group, restarts, in the lanes)."""
    rng = np.random.default_rng(702)
    seed = oracle.get_seed(9)

    def ordinary(n):
        return partial_problem(rng, 3, n)

    problems = [ordinary(700), poly_a_pair(514, 514) + (b"",), ordinary(500), poly_a_pair(514, 515) + (b"",),
                poly_a_triple((600, 450, 100)), ordinary(900), poly_a_triple((450, 100, 600))]
    # (problem 4 restarts with 600 + 450 records collected and genome 2's head still on the key;
    # in problem 6 the 1150 all-A windows and one more window of the same masked key are all
    # collected before the check sees them, and no head is left on the key: no restart)
    expect = {1: (1000, 0, True), 3: (1001, 0, False), 4: (1050, 1, False), 6: (1151, 0, False)}
    return dict(problems=problems, seed=seed, table_size=40000, mask=None, expect=expect)


# ---- G. degenerate sequences inside wider problems --------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_case():
    """empty: problem -> the columns that hold no seed-mer."""
    rng = np.random.default_rng(800)
    seed = oracle.get_seed(7)
    L = seed_length(seed)

    def rel():
        a = rand_seq(rng, 700)
        return a, mutate(rng, a, 0.03)

    (a0, b0), (a1, b1), (a2, b2), (a3, b3) = rel(), rel(), rel(), rel()
    problems = [partial_problem(rng, 4, 700),
                (a0, b"", b0, b"ACG"),
                (b"", a1, b"", b1),
                (a2, rand_seq(rng, L), b2, rand_seq(rng, L - 1)),
                partial_problem(rng, 4, 500),
                (b"", b"", a3, b3)]
    return dict(problems=problems, seed=seed, table_size=40000, mask=None,
                empty={1: (1, 3), 2: (0, 2), 3: (3,), 5: (0, 1)}, one_seed={3: (1,)})


# ---- H. repeat-rich problems that stay in the lanes -------------------------------------------
@functools.lru_cache(maxsize=None)
def repeat_rich_case(table_size=40000):
    rng = np.random.default_rng(900)
    problems = [tuple(repeat_inputs.high_copy(G=3, n=6000, copies=300, unit=60, seed=5)),
                partial_problem(rng, 3, 600),
                tuple(repeat_inputs.high_copy(G=3, n=6000, copies=300, unit=60, seed=5, tandem=True)),
                tuple(repeat_inputs.high_copy(G=3, n=6000, copies=2, unit=300, seed=6, only_genome=1)),
                partial_problem(rng, 3, 800)]
    return dict(problems=problems, seed=oracle.get_seed(9), table_size=table_size, mask=None, rich=(0, 2, 3),
                big_groups=(0, 2))


# ---- I. one context, many shapes --------------------------------------------------------------
def context_sequence():
    """The batches one object runs in this order: G 64 -> 2, lanes -> every problem alone -> no
    seed-mer at all -> lanes again (grow-only buffers, per-problem words, the pool's row stride)."""
    rng = np.random.default_rng(1000)
    small = dict(problems=[pair(rng, 300), pair(rng, 450, flip=True), pair(rng, 200)], seed=oracle.get_seed(7),
                 table_size=40000, mask=None)
    empty = dict(problems=[(b"", b"")] * 5, seed=oracle.get_seed(7), table_size=40000, mask=None)
    alpha = alphabet()
    first40 = dict(alpha, problems=alpha["problems"][:40])
    return [instantiation_case(64), small, sort_width_case("w31_b3"), empty, first40]
