"""Seed families (ClearSequences keeps the MemHash table, ProgressiveAligner.cpp:619-653): the
cases shared by test_seed_family_cpu.py, test_gpu_seed_family.py and
golden/make_seed_family_golden.py, the loader of tests/seed_family_model.c and the digests the
fixture golden/seed_family_cases.json records."""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libseed_family_model.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "seed_family_cases.json")

# name -> G, n, p, w (seed weight), T (table size), ranks (seed ranks in round order); optional:
#   mode: dict(masked=, seq_mask=, pairwise=, repeat_tol=, enum_tol=)
#   alt: {round: (n, rng_seed)} -- that round runs on other sequences of the same G and p
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
}
FIRST = "c1_pairwise_anchor"
RNG_SEED = 12345

_seq_cache = {}


def sequences(G, n, p, rng=RNG_SEED):
    key = (G, n, p, rng)
    if key not in _seq_cache:
        _seq_cache[key] = oracle.generate(G, n, p, rng)
    return _seq_cache[key]


def rounds_of(case):
    """[(sequences, seed pattern, oracle.find_matches keywords)] of a case, in round order."""
    c = CASES[case] if isinstance(case, str) else case
    mode = dict(c.get("mode", {}))
    out = []
    for r, rank in enumerate(c["ranks"]):
        n, rng = c.get("alt", {}).get(r, (c["n"], RNG_SEED))
        out.append((sequences(c["G"], n, c["p"], rng), oracle.get_seed(c["w"], rank),
                    dict(table_size=c["T"], **mode)))
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


def fixture_chain():
    with open(FIXTURE) as f:
        return json.load(f)["chain"]
