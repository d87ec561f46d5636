"""Seed families (ClearSequences keeps the MemHash table, ProgressiveAligner.cpp:619-653): the
cases shared by test_seed_family_cpu.py, test_gpu_seed_family.py and
golden/make_seed_family_golden.py, the loader of tests/seed_family_model.c and the digests the
fixture golden/seed_family_cases.json records.  A case may take its sequences from a generator of
tests/repeat_inputs.py (`gen`, the same sequences in every round) and may replace the sequences
of single rounds by those of a function of this module (`seqs`)."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

import repeat_inputs
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libseed_family_model.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "seed_family_cases.json")

# name -> G, n, p, w (seed weight), T (table size), ranks (seed ranks in round order); optional:
#   mode: dict(masked=, seq_mask=, pairwise=, repeat_tol=, enum_tol=)
#   alt: {round: (n, rng_seed)} -- that round runs on other sequences of the same G and p
#   gen: (generator of repeat_inputs.py, its keywords) -- the sequences of every round (n and p unused)
#   seqs: {round: name of a function of this module} -- that round runs on the sequences it returns
# The k cases exist for the paths of replay_carried_kernel / launch_replay_carried they reach
# (test_seed_family_cpu.py::test_cases_reach_the_carried_replays_paths holds them to it).
CASES = {
    "c1_pairwise_anchor": dict(G=2, n=30000, p=0.05, w=11, T=40000, ranks=(0, 1, 2)),
    "c1_order_201": dict(G=2, n=30000, p=0.05, w=11, T=40000, ranks=(2, 0, 1)),
    "c2_crowded_T7": dict(G=2, n=30000, p=0.05, w=11, T=7, ranks=(0, 1, 2)),
    "c3_g3_revcomp_T64": dict(G=3, n=20000, p=0.03, w=9, T=64, ranks=(0, 1, 2)),
    "c4_one_bucket_spill": dict(G=2, n=50000, p=1.0, w=9, T=1, ranks=(0, 1, 2)),
    "c5_g4_diagonal": dict(G=4, n=20000, p=0.08, w=11, T=40000, ranks=(0, 1, 2)),
    "c6_g34_dense_blocks": dict(G=34, n=2000, p=0.05, w=9, T=40000, ranks=(0, 1, 2)),
    "c7_masked7": dict(G=3, n=20000, p=0.03, w=9, T=64, ranks=(0, 1, 2), mode=dict(masked=True, seq_mask=7)),
    "c7_pairwise": dict(G=3, n=20000, p=0.03, w=9, T=64, ranks=(0, 1, 2), mode=dict(pairwise=True)),
    "c7_rt1_et2": dict(G=3, n=20000, p=0.03, w=9, T=64, ranks=(0, 1, 2), mode=dict(repeat_tol=1, enum_tol=2)),
    "c8_other_sequences": dict(G=2, n=30000, p=0.05, w=11, T=40000, ranks=(0, 1, 2), alt={2: (25000, 777)}),
    "c9_five_rounds": dict(G=2, n=30000, p=0.05, w=11, T=40000, ranks=(0, 1, 2, 0, 1)),
    "k1_spill_mid_replay": dict(G=2, n=40000, p=1.0, w=9, T=1, ranks=(0, 1, 2)),
    "k2_lds_carried_T3": dict(G=2, n=40000, p=1.0, w=9, T=3, ranks=(0, 1, 2)),
    "k3_small_edge_T300": dict(G=2, n=50000, p=1.0, w=9, T=300, ranks=(0, 1, 2)),
    "k4_g6": dict(G=6, n=4000, p=0.05, w=9, T=64, ranks=(0, 1, 2)),
    "k5_g12": dict(G=12, n=3000, p=0.05, w=9, T=64, ranks=(0, 1, 2)),
    "k6_g24": dict(G=24, n=2000, p=0.05, w=9, T=40000, ranks=(0, 1, 2)),
    "k7_g32": dict(G=32, n=2000, p=0.05, w=9, T=64, ranks=(0, 1, 2)),
    "k8_g33": dict(G=33, n=2000, p=0.05, w=9, T=64, ranks=(0, 1, 2)),
    "k9_w21": dict(G=2, n=30000, p=0.02, w=21, T=40000, ranks=(0, 1, 2)),
    "k10_n_gapped": dict(G=3, w=9, T=64, ranks=(0, 1, 2),
                         gen=("n_gapped", dict(G=3, n=20000, gaps=((5000, 1500),), p=0.02, seed=7, shift=40))),
    "k11_high_copy": dict(G=3, w=11, T=40000, ranks=(0, 1, 2),
                          gen=("high_copy", dict(G=3, n=15000, copies=600, unit=100, seed=11))),
    "k12_one_probe": dict(G=2, n=30000, p=0.05, w=11, T=40000, ranks=(0, 1), seqs={1: "one_probe_pair"}),
}
FIRST = "c1_pairwise_anchor"
SPILL = "k1_spill_mid_replay"   # its bucket outgrows the replay's LDS vector during round 1
RNG_SEED = 12345

_seq_cache = {}


def sequences(G, n, p, rng=RNG_SEED):
    key = (G, n, p, rng)
    if key not in _seq_cache:
        _seq_cache[key] = oracle.generate(G, n, p, rng)
    return _seq_cache[key]


def generated(gen, kw):
    key = (gen, repr(sorted(kw.items())))
    if key not in _seq_cache:
        _seq_cache[key] = getattr(repeat_inputs, gen)(**kw)
    return _seq_cache[key]


def one_probe_pair(run=19):
    """Two unrelated 300-bp sequences that share one run of `run` bases (the bases on either side
    of it differ).  19 is the length of the w11 rank-1 seed pattern, found by a search on the
    model: 18 gives no AddHashEntry call under that seed, 20 gives two, 19 exactly one
    (test_cases_reach_the_carried_replays_paths asserts it on the model)."""
    a = bytearray(oracle.generate(1, 300, 0.0, 5)[0])
    b = bytearray(oracle.generate(1, 300, 0.0, 6)[0])
    b[180:180 + run] = a[100:100 + run]
    for ia, ib in ((99, 179), (100 + run, 180 + run)):
        if b[ib] == a[ia]:
            b[ib] = b"ACGT"[(b"ACGT".index(a[ia]) + 1) % 4]
    return [bytes(a), bytes(b)]


def rounds_of(case):
    """[(sequences, seed pattern, oracle.find_matches keywords)] of a case, in round order."""
    c = CASES[case] if isinstance(case, str) else case
    mode = dict(c.get("mode", {}))
    out = []
    for r, rank in enumerate(c["ranks"]):
        if r in c.get("seqs", {}):
            seqs = globals()[c["seqs"][r]]()
        elif "gen" in c:
            seqs = generated(*c["gen"])
        else:
            n, rng = c.get("alt", {}).get(r, (c["n"], RNG_SEED))
            seqs = sequences(c["G"], n, c["p"], rng)
        assert len(seqs) == c["G"]
        out.append((seqs, oracle.get_seed(c["w"], rank), dict(table_size=c["T"], **mode)))
    return out


class _Round(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64), ("mem_count", ctypes.c_uint64), ("collisions", ctypes.c_uint64),
                ("probes", ctypes.c_uint64), ("log_n", ctypes.c_uint64), ("lengths", ctypes.c_void_p),
                ("starts", ctypes.c_void_p), ("table_counts", ctypes.c_void_p), ("log_len", ctypes.c_void_p),
                ("log_s", ctypes.c_void_p)]


def have_compiler():
    return shutil.which("gcc") is not None


def load_model():
    """Builds tests/seed_family_model.c with gcc (aside, then renamed: parallel workers never
    load a partial file)."""
    os.makedirs(BUILD, exist_ok=True)
    tmp = f"{SO}.{os.getpid()}"
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-fopenmp", "-w", "-o", tmp,
                    os.path.join(ROOT, "tests", "seed_family_model.c"), "-lm"], check=True)
    os.replace(tmp, SO)
    L = ctypes.CDLL(SO)
    L.seed_family_run.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                  ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(oracle._Params),
                                  ctypes.POINTER(_Round)]
    L.seed_family_free.argtypes = [ctypes.POINTER(_Round), ctypes.c_int]
    return L


def _copy(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


def run_model(L, rounds):
    """The model over rounds = [(sequences, seed, keywords)]: per round a dict with lengths,
    starts, mem_count, collisions, probes, table_counts, log = (lengths, starts)."""
    R = len(rounds)
    G = len(rounds[0][0])
    T = rounds[0][2].get("table_size", 40000)
    flat = [s for seqs, _, _ in rounds for s in seqs]
    arr = (ctypes.c_char_p * len(flat))(*flat)
    lens = (ctypes.c_uint64 * len(flat))(*[len(s) for s in flat])
    prms = (oracle._Params * R)()
    for r, (_, seed, kw) in enumerate(rounds):
        assert kw.get("table_size", 40000) == T
        prms[r] = oracle._Params(seed, kw.get("repeat_tol", 0), kw.get("enum_tol", 1), T, int(kw.get("masked", False)),
                                 kw.get("seq_mask", 0), 0, 0, 0, 0, int(kw.get("pairwise", False)), None)
    out = (_Round * R)()
    rc = L.seed_family_run(G, T, R, arr, lens, prms, out)
    assert rc == 0, "the model rejected the input"
    res = []
    try:
        for o in out:
            res.append(dict(
                lengths=_copy(o.lengths, o.count, np.uint64),
                starts=_copy(o.starts, o.count * G, np.int64).reshape(o.count, G),
                mem_count=int(o.mem_count), collisions=int(o.collisions), probes=int(o.probes),
                table_counts=_copy(o.table_counts, T, np.uint32),
                log=(_copy(o.log_len, o.log_n, np.uint64), _copy(o.log_s, o.log_n * G, np.int64).reshape(o.log_n, G))))
    finally:
        L.seed_family_free(out, R)
    return res


def list_md5(lengths, starts):
    return hashlib.md5(np.ascontiguousarray(lengths, dtype="<u8").tobytes() +
                       np.ascontiguousarray(starts, dtype="<i8").tobytes()).hexdigest()


def log_set_md5(log):
    """md5 of the match log's lines in lexicographic order (what was inserted, whatever the order)."""
    lengths, starts = log
    rows = np.concatenate([np.asarray(lengths, dtype=np.int64).reshape(-1, 1), np.asarray(starts, dtype=np.int64)], axis=1)
    rows = rows[np.lexsort(rows.T[::-1])] if len(rows) else rows
    return hashlib.md5(np.ascontiguousarray(rows, dtype="<i8").tobytes()).hexdigest()


def digest(rnd):
    """What the fixture records of one round."""
    return dict(log_set_md5=log_set_md5(rnd["log"]), count=int(len(rnd["lengths"])), list_md5=list_md5(rnd["lengths"], rnd["starts"]),
                mem_count=int(rnd["mem_count"]), collisions=int(rnd["collisions"]), probes=int(rnd["probes"]),
                table_md5=hashlib.md5(np.ascontiguousarray(rnd["table_counts"], dtype="<u4").tobytes()).hexdigest(),
                log_count=int(len(rnd["log"][0])), log_md5=list_md5(*rnd["log"]))


CHAIN_MIN_LENGTH = 9 + 3   # MIN_ANCHOR_LENGTH (Aligner.h:266) + 3: ProgressiveAligner.cpp:659


def chain_of_model(eo2, eo2_lib, family_round):
    """pairwiseAnchorSearch's tail (ProgressiveAligner.cpp:658-659) on a family list:
    tests/eo2_model.cpp, then LengthFilter on the host."""
    el, es, _ = eo2.model_eo2(eo2_lib, family_round["lengths"], family_round["starts"], None, False)
    keep = el >= CHAIN_MIN_LENGTH
    return el[keep], es[keep]


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def fixture_chain(key="chain"):
    with open(FIXTURE) as f:
        return json.load(f)[key]
