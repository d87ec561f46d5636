"""mums_find_batch without a GPU: the ABI declares it, a null context is refused, the mirror's
grouping by default seed is host logic, and the batch's encodings (problem id above the key, the
compact seed-mer index, the per-problem table words) restated in numpy round-trip."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def test_header_declares_the_batch_calls():
    hdr = open(os.path.join(ROOT, "include", "mums.h")).read()
    assert re.search(r"int\s+mums_find_batch\(mums_ctx\* ctx, uint32_t B, uint32_t G, const char\* ascii, "
                     r"const uint64_t\* seq_off\);", hdr)
    assert re.search(r"int\s+mums_batch_info\(mums_ctx\* ctx, uint64_t\* match_off, uint64_t\* probes, "
                     r"uint64_t\* collisions, uint64_t\* restarts\);", hdr)
    assert "#define MUMS_ABI_VERSION 6" in hdr


def test_null_context_is_invalid(gpu_lib):
    lib = gpu_lib.load_library()
    off = np.zeros(3, dtype=np.uint64)
    assert lib.mums_find_batch(None, 1, 2, b"", off.ctypes.data) == -1
    assert lib.mums_batch_info(None, off.ctypes.data, None, None, None) == -1
    assert "mums_find_batch" in gpu_lib.EXPORTED_SYMBOLS and "mums_batch_info" in gpu_lib.EXPORTED_SYMBOLS


def test_grouping_by_default_seed(gpu_lib):
    """getSeed(getDefaultSeedWeight(mean length), 0) per problem (ProgressiveAligner.cpp:615-616, 625);
    weight 0 = no search (:626-633); groups keep the problems' order."""
    lens = [(10, 12), (100, 140), (0, 0), (1000, 900), (3000, 2800), (150, 90), (20000, 20000), (15, 17), (700, 1300)]
    problems = [(b"A" * a, b"C" * b) for a, b in lens]
    patterns, groups = gpu_lib.batch_seed_groups(problems)
    weights = [gpu_lib.getDefaultSeedWeight((a + b) // 2) for a, b in lens]
    assert weights == [0, 5, 0, 7, 9, 5, 11, 0, 7]
    for w, pat in zip(weights, patterns):   # (getSeed(11) is the table's 12-care pattern: SeedMasks.h)
        assert pat == (gpu_lib.getSeed(w, 0) if w else 0)
    assert list(groups) == [gpu_lib.getSeed(5), gpu_lib.getSeed(7), gpu_lib.getSeed(9), gpu_lib.getSeed(11)]
    assert [groups[gpu_lib.getSeed(w)] for w in (5, 7, 9, 11)] == [[1, 5], [3, 8], [4], [6]]
    # explicit seeds group the same way, 0 = no search
    pats, grp = gpu_lib.batch_seed_groups(problems, [7, 9, 7, 0, 9, 7, 0, 9, 7])
    assert pats == [7, 9, 7, 0, 9, 7, 0, 9, 7] and grp == {7: [0, 2, 5, 8], 9: [1, 4, 7]}
    # order restored: every problem's slot is filled from exactly one group
    seen = sorted(p for idx in groups.values() for p in idx)
    assert seen == [p for p, w in enumerate(weights) if w]


def test_batch_encodings_round_trip(oracle_mod):
    """key2 = p << (2w+1) | ckey sorts problem-major and gives (p, ckey) back; the compact index
    i = mbase[p * G + g] + position gives (p, g, position) back by the search the keys kernel
    runs; a table word bucket << 32 | entry sorts a problem's entries bucket-major, where the
    bucket of an entry is oracle.entry_buckets of the problem's own list."""
    rng = np.random.default_rng(7)
    B, G, w, L = 37, 3, 9, 15
    kbits = 2 * w + 1
    n = rng.integers(0, 60, size=B * G)
    m = np.where(n < L, 0, n - L + 1)
    mbase = np.concatenate([[0], np.cumsum(m)]).astype(np.uint32)
    N = int(mbase[-1])
    i = np.arange(N, dtype=np.uint32)
    seg = np.searchsorted(mbase, i, side="right") - 1          # the largest s with mbase[s] <= i
    pos = i - mbase[seg]
    assert (m[seg] > 0).all() and (pos < m[seg]).all()
    assert np.array_equal(np.repeat(np.arange(B * G), m), seg)
    p = (seg // G).astype(np.uint64)
    ckey = rng.integers(0, 1 << kbits, size=N, dtype=np.uint64)
    key2 = (p << np.uint64(kbits)) | ckey
    assert np.array_equal(key2 >> np.uint64(kbits), p) and np.array_equal(key2 & np.uint64((1 << kbits) - 1), ckey)
    order = np.argsort(key2, kind="stable")
    assert (np.diff(p[order].astype(np.int64)) >= 0).all()        # groups never mix problems
    rec0 = mbase[::G]                                             # problem p's records: [rec0[p], rec0[p + 1])
    assert np.array_equal(np.searchsorted(p[order], np.arange(B + 1)), rec0)
    # table words: the oracle's own lists, bucket-major
    seqs = oracle_mod.generate(3, 3000, 0.04, 99)
    for T in (40000, 7):
        ln, st, _ = oracle_mod.find_matches(seqs, oracle_mod.get_seed(9), table_size=T)
        bk = oracle_mod.entry_buckets(ln, st, T).astype(np.uint64)
        ids = rng.permutation(len(ln)).astype(np.uint64)          # pool ids are in insertion order, any order
        words = (bk << np.uint64(32)) | ids
        assert np.array_equal(words >> np.uint64(32), bk) and np.array_equal(words & np.uint64(0xFFFFFFFF), ids)
        assert (np.diff(bk.astype(np.int64)) >= 0).all()          # GetMatchList order = ascending bucket
        lo = np.searchsorted(words >> np.uint64(32), bk, side="left")
        hi = np.searchsorted(words >> np.uint64(32), bk, side="right")
        k = np.arange(len(bk))
        assert ((lo <= k) & (k < hi)).all()
