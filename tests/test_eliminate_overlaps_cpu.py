"""EliminateOverlaps (Aligner.cpp:62-176), CPU side: the oracle's restatement of libstdc++'s
std::sort (introsort: tie order of SingleStartComparator) against the real std::sort /
std::partial_sort of this toolchain, and the oracle's EliminateOverlaps against a C++ model
over Match* vectors sorted by the real std::sort (tests/eo_model.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SO = os.path.join(BUILD, "libeo_model.so")


@pytest.fixture(scope="module")
def model():
    os.makedirs(BUILD, exist_ok=True)
    tmp = f"{SO}.{os.getpid()}"   # build aside, then rename: parallel workers never load a partial file
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, os.path.join(ROOT, "tests", "eo_model.cpp")],
                   check=True)
    os.replace(tmp, SO)
    L = ctypes.CDLL(SO)
    L.model_std_sort.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    L.model_eliminate_overlaps.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.model_eliminate_overlaps.restype = ctypes.c_uint64
    return L


def model_sort(L, keys, heap_only=False):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    ids = np.arange(len(keys), dtype=np.uint32)
    L.model_std_sort(ids.ctypes.data, len(keys), keys.ctypes.data, int(heap_only))
    return ids


@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 18, 33, 100, 1000, 5000, 40000])
@pytest.mark.parametrize("span", [1, 3, 50, 1 << 40])
def test_std_sort_restatement_matches_libstdcxx(model, n, span):
    rng = np.random.default_rng(n * 7 + span % 1000)
    keys = rng.integers(0, span, size=n, dtype=np.uint64)
    if n > 10:
        keys[rng.integers(0, n, size=n // 3)] = 0      # NO_MATCH group
    assert np.array_equal(oracle.std_sort_ids(keys), model_sort(model, keys))


@pytest.mark.parametrize("n", [17, 64, 1000, 4097])
def test_heap_fallback_matches_partial_sort(model, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 20, size=n, dtype=np.uint64)
    assert np.array_equal(oracle.std_sort_ids(keys, depth=0), model_sort(model, keys, heap_only=True))


def random_matchlist(rng, M, G, n=20000, max_len=300, p_absent=0.3, p_rev=0.3, start_span=None):
    """Matches with overlaps, reverse components, NO_MATCH and tied starts."""
    span = start_span or n
    lengths = rng.integers(1, max_len, size=M).astype(np.uint64)
    starts = rng.integers(1, span, size=(M, G)).astype(np.int64)
    starts[rng.random((M, G)) < p_rev] *= -1
    starts[rng.random((M, G)) < p_absent] = 0
    starts[:, 0] = np.where(starts[:, 0] == 0, 1 + rng.integers(0, span, size=M), starts[:, 0])
    return lengths, starts


EO_TILE = 1024   # overlaps.hip kEoTile: heads_kernel's tiles, tile_prefix_kernel's max-scan over them


def carried_head_matchlist(M=20000, G=3, span=2_000_000, seed=21, left=300_000, length=400_000):
    """random_matchlist (every length below 300: the running maximum of the ends always comes
    from the neighbouring entries) plus one match defined in every genome that spans several
    tiles of the sorted order: behind it only the tile prefix carries the cluster on."""
    rng = np.random.default_rng(seed)
    lengths, starts = random_matchlist(rng, M, G, start_span=span)
    big = np.array([[left + 17 * g for g in range(G)]], dtype=np.int64)
    return np.concatenate([lengths, np.array([length], dtype=np.uint64)]), np.concatenate([starts, big])


def above_2p32_matchlist(M=3000, G=4, span=30000, seed=22, shift=5_000_000_000):
    """random_matchlist with 5e9 added to every forward start and subtracted from every reverse
    one: coordinates and ends that do not fit 32 bits."""
    rng = np.random.default_rng(seed)
    lengths, starts = random_matchlist(rng, M, G, start_span=span)
    return lengths, starts + np.sign(starts) * shift


EDGE_LISTS = {"carried_head": carried_head_matchlist, "above_2p32": above_2p32_matchlist}
SORT_ORDERS = ("ascending", "descending", "organ_pipe", "sawtooth16", "all_equal_but_one")
SORT_SIZES = (17, 1000, 65536)


def adversarial_keys(order, n):
    """Key orders that drive introsort's median-of-three / depth limit differently from random keys."""
    i = np.arange(n, dtype=np.uint64)
    if order == "ascending":
        return i + 1
    if order == "descending":
        return n - i
    if order == "organ_pipe":
        return np.minimum(i, n - 1 - i) + 1
    if order == "sawtooth16":
        return i % 16 + 1
    keys = np.full(n, 7, dtype=np.uint64)
    keys[n // 2] = 3
    return keys


def model_eo(L, lengths, starts):
    M, G = starts.shape
    cap = 8 * M + 64
    lo = np.zeros(cap, dtype=np.uint64)
    so = np.zeros(cap * G, dtype=np.int64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    k = L.model_eliminate_overlaps(G, M, lengths.ctypes.data, starts.ctypes.data, lo.ctypes.data, so.ctypes.data, cap)
    assert k <= cap
    return lo[:k], so[:k * G].reshape(k, G)


@pytest.mark.parametrize("M,G,span,seed", [(2, 2, 50, 1), (10, 2, 100, 2), (200, 3, 2000, 3), (3000, 4, 30000, 4),
                                           (5000, 8, 20000, 5), (20000, 5, 400000, 6), (3000, 3, 300, 7)])
def test_eliminate_overlaps_oracle_matches_model(model, M, G, span, seed):
    rng = np.random.default_rng(seed)
    lengths, starts = random_matchlist(rng, M, G, start_span=span)
    ol, os_ = oracle.eliminate_overlaps(lengths, starts)
    ml, ms = model_eo(model, lengths, starts)
    assert np.array_equal(ol, ml) and np.array_equal(os_, ms)


def test_eliminate_overlaps_on_findmatches_output(model):
    # repeat-rich related genomes: MemHash MatchLists with overlapping entries
    seqs = oracle.generate(4, 400_000, 0.02, 99)
    rep = seqs[0][1000:3000]
    seqs = [s[:50_000] + rep + s[50_000:200_000] + rep + s[200_000:] for s in seqs]
    lengths, starts, _ = oracle.find_matches(seqs, oracle.get_seed(11))
    ol, os_ = oracle.eliminate_overlaps(lengths, starts)
    ml, ms = model_eo(model, lengths, starts)
    assert len(ol) != len(lengths) or not np.array_equal(os_, starts)   # something was cropped
    assert np.array_equal(ol, ml) and np.array_equal(os_, ms)


def test_carried_head_precondition():
    """In pass 0's sort order (LeftEnd in sequence 0) the long match alone carries the running
    maximum of the ends across at least 3 tile boundaries: behind each of them lies an entry that
    starts before the long match ends but at or after every other earlier end (a cluster head
    without it), and for one boundary the long match is not even in the previous tile."""
    lengths, starts = carried_head_matchlist()
    k = np.abs(starts[:, 0]).astype(np.uint64)
    assert (k != 0).all()
    order = oracle.std_sort_ids(k)
    K = k[order].astype(np.int64)
    ends = K + lengths[order].astype(np.int64)
    pos = int(np.nonzero(order == len(k) - 1)[0][0])
    others = ends.copy()
    others[pos] = 0
    run_wo = np.concatenate([[0], np.maximum.accumulate(others)[:-1]])   # exclusive, without the long match
    idx = np.arange(len(K))
    alone = (idx > pos) & (K < ends[pos]) & (K >= run_wo)
    tiles = sorted({int(t) for t in idx[alone] // EO_TILE if t * EO_TILE > pos})
    assert len(tiles) >= 3, tiles
    assert max(tiles) >= pos // EO_TILE + 2


@pytest.mark.parametrize("name", sorted(EDGE_LISTS))
def test_eliminate_overlaps_edge_lists(model, name):
    lengths, starts = EDGE_LISTS[name]()
    ol, os_ = oracle.eliminate_overlaps(lengths, starts)
    ml, ms = model_eo(model, lengths, starts)
    assert len(ol) != len(lengths) or not np.array_equal(os_, starts)
    assert np.array_equal(ol, ml) and np.array_equal(os_, ms)
    if name == "above_2p32":
        assert (np.abs(os_[os_ != 0]) > 1 << 32).all()


@pytest.mark.parametrize("n", SORT_SIZES)
@pytest.mark.parametrize("order", SORT_ORDERS)
def test_std_sort_restatement_adversarial_orders(model, order, n):
    keys = adversarial_keys(order, n)
    assert np.array_equal(oracle.std_sort_ids(keys), model_sort(model, keys))
