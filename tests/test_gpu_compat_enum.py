"""GPU ParallelMemHash chunk-compat mode under enumeration tolerance > 1: the odometer of
MatchFinder::EnumerateMatches (MatchFinder.cpp:342-393) inside every chunk's SearchRange, the
thread tables merged by MergeTable (ParallelMemHash.cpp:42-121) -- SetEnumerationTolerance is a
virtual MemHash member ParallelMemHash inherits (MemHash.h:139,156-159).  Against the oracle's
restatement (parallel_compat_search -> enumerate_matches), bit for bit; parity for enum_tol > 1
rests on the oracle (no reference fixture covers it).  Also the row-parallel odometer emit
(pairwise.hip) under plain MemHash at groups of tens of thousands of rows, and the 64-bit total
of the row counts."""
import numpy as np
import pytest

from tests import repeat_inputs
from tests.compat_enum_inputs import SHAPES, make_input, oracle_answer

pytestmark = pytest.mark.gpu


def gpu_parallel(lm, seqs, seed, chunk, rt, et, masked=False, mask=0, table_size=40000):
    with lm.ParallelMemHash(0, chunk) as mh:
        mh.SetSeed(seed)
        mh.SetTableSize(table_size)
        mh.SetRepeatTolerance(rt)
        mh.SetEnumerationTolerance(et)
        if masked:
            mh._check(mh._lib.mums_set_mask(mh._ctx, 1, mask))
        ml = mh.FindMatches(list(seqs))
        return ml, mh.stats()


def check(gpu_lib, oracle_mod, sid, chunk=None, table_size=40000):
    spec, w, rt, et, chunk0, masked, mask = SHAPES[sid]
    chunk = chunk or chunk0
    lengths, starts, ost = oracle_answer(spec, w, rt, et, chunk, masked, mask, table_size)
    ml, st = gpu_parallel(gpu_lib, make_input(spec), oracle_mod.get_seed(w), chunk, rt, et, masked, mask, table_size)
    print(sid, "matches", len(ml), len(lengths), "chunks", st["chunks"], ost["chunks"], "restarts", st["restarts"],
          ost["restarts"], "probes", st["probes"], ost["probes"], "collisions", st["collision_count"],
          ost["collision_count"])
    assert st["chunks"] == ost["chunks"]
    assert st["restarts"] == ost["restarts"]
    assert st["probes"] == ost["probes"]
    assert len(ml) == len(lengths)
    assert np.array_equal(ml.lengths, lengths) and np.array_equal(ml.starts, starts)
    # (collision_count: the compat mode's count is not the thread tables' sum, at enum_tol 1
    # either -- test_gpu_tie_order.py; printed above, not compared)
    return ml, st, ost


@pytest.mark.parametrize("sid", list("ABCDEFGHIJK"))
def test_compat_enum_vs_oracle(gpu_lib, oracle_mod, sid):
    _, _, ost = check(gpu_lib, oracle_mod, sid)
    assert ost["chunks"] > 1 and ost["restarts"] == 0


@pytest.mark.parametrize("sid", ["L", "M"])
def test_compat_enum_cut_chunks_vs_oracle(gpu_lib, oracle_mod, sid):
    """Chunks cut by MER_REPEAT_LIMIT (SearchRange returns false, ParallelMemHash.cpp:97 ignores
    it): the odometer runs over the groups before the cut only."""
    _, _, ost = check(gpu_lib, oracle_mod, sid)
    assert ost["restarts"] > 0


@pytest.mark.parametrize("sid", ["A", "H"])
def test_compat_enum_is_neither_other_mode(gpu_lib, oracle_mod, sid):
    """Not the enum_tol = 1 compat answer (a silently ignored setting) and not plain MemHash's
    enum_tol answer (a fall-through to the one-table enumeration pipeline)."""
    spec, w, rt, et, chunk, masked, mask = SHAPES[sid]
    ml, _, _ = check(gpu_lib, oracle_mod, sid)
    for other in (oracle_answer(spec, w, rt, 1, chunk, masked, mask), oracle_answer(spec, w, rt, et, 0, masked, mask,
                                                                                    compat=False)):
        assert not (len(ml) == len(other[0]) and np.array_equal(ml.lengths, other[0]) and
                    np.array_equal(ml.starts, other[1]))


@pytest.mark.parametrize("env", ["MUMS_DEV_COMPAT_PAIRS", "MUMS_DEV_COMPAT_RADIX", "MUMS_DEV_COMPAT_PART"])
def test_compat_enum_fallback_switches(gpu_lib, oracle_mod, monkeypatch, env):
    monkeypatch.setenv(env, "1")
    check(gpu_lib, oracle_mod, "A")


def test_compat_enum_single_chunk(gpu_lib, oracle_mod):
    _, st, _ = check(gpu_lib, oracle_mod, "A", chunk=200_000)
    assert st["chunks"] == 1


@pytest.mark.parametrize("sid", ["A", "H"])
def test_compat_enum_small_table(gpu_lib, oracle_mod, sid):
    """7 hash buckets: long bucket vectors, MergeTable interleaves every chunk's entries."""
    check(gpu_lib, oracle_mod, sid, table_size=7)


def test_compat_enum_match_log_refused(gpu_lib, oracle_mod):
    """SetMatchLog under compat with enum_tol > 1 is not reproduced (the per-chunk log order
    comes from the probe stage the row path does not run): refused, naming the match log."""
    spec, w, rt, et, chunk, _, _ = SHAPES["A"]
    with gpu_lib.ParallelMemHash(0, chunk) as mh:
        mh.SetSeed(oracle_mod.get_seed(w))
        mh.SetRepeatTolerance(rt)
        mh.SetEnumerationTolerance(et)
        mh.SetMatchLog(True)
        with pytest.raises(gpu_lib.MumsError, match="match log") as ei:
            mh.FindMatches(list(make_input(spec)))
        assert ei.value.code == gpu_lib.MUMS_E_UNSUPPORTED


def test_enum_row_parallel_emit_large_groups(gpu_lib, oracle_mod):
    """Plain MemHash on shape J's input: 4 genomes under enum_tol 16, groups of up to tens of
    thousands of odometer rows (16^4 at the most) next to one-row groups -- every row decodes its
    own combination (last genome fastest) and finds its group from the scanned offsets, group
    boundaries included."""
    spec, w, rt, et, _, _, _ = SHAPES["J"]
    lengths, starts, ost = oracle_answer(spec, w, rt, et, 0, False, 0, compat=False)
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(oracle_mod.get_seed(w))
        mh.SetRepeatTolerance(rt)
        mh.SetEnumerationTolerance(et)
        ml = mh.FindMatches(list(make_input(spec)))
        st = mh.stats()
    assert st["probes"] == ost["probes"] > 65_536
    assert st["collision_count"] == ost["collision_count"]
    assert len(ml) == len(lengths)
    assert np.array_equal(ml.lengths, lengths) and np.array_equal(ml.starts, starts)


def group_calls(oracle_mod, seqs, seed, rt, et):
    """AddHashEntry calls of every masked-key group of the whole input (one chunk: MemHash's
    groups): the product over the present genomes of min(count, enum_tol), for groups of at least
    two genomes in which no genome has more than repeat_tol + 1 records; a two-record group is
    one call (MatchFinder.cpp:344-347)."""
    G = len(seqs)
    keys = [oracle_mod.seed_keys(s, seed) >> np.uint64(1) for s in seqs]
    uniq = np.unique(np.concatenate(keys))
    cnt = np.zeros((G, len(uniq)), dtype=np.int64)
    for g in range(G):
        k, c = np.unique(keys[g], return_counts=True)
        cnt[g, np.searchsorted(uniq, k)] = c
    ok = (cnt <= rt + 1).all(axis=0) & ((cnt > 0).sum(axis=0) >= 2)
    kept = np.minimum(cnt, et)
    calls = np.where(kept > 0, kept, 1).prod(axis=0)
    calls[kept.sum(axis=0) == 2] = 1
    return calls[ok]


def test_compat_enum_total_rows_above_2_32_refused(gpu_lib, oracle_mod):
    """Every group below 2^31 AddHashEntry calls (the per-group guard passes), their sum above
    2^32: refused after the count, before any buffer sized by the total exists -- never a
    wrapped 32-bit total."""
    seqs = repeat_inputs.high_copy(G=5, n=60_000, copies=40, tandem=False, seed=5)
    seed = oracle_mod.get_seed(15)
    calls = group_calls(oracle_mod, seqs, seed, 39, 40)
    print("groups", len(calls), "largest", int(calls.max()), "total", int(calls.sum()))
    assert int(calls.max()) < 2**31
    assert int(calls.sum()) >= 2**32
    with gpu_lib.ParallelMemHash(0, 200_000) as mh:
        mh.SetSeed(seed)
        mh.SetRepeatTolerance(39)
        mh.SetEnumerationTolerance(40)
        with pytest.raises(gpu_lib.MumsError, match=r"2\^32") as ei:
            mh.FindMatches(seqs)
        assert ei.value.code == gpu_lib.MUMS_E_UNSUPPORTED
