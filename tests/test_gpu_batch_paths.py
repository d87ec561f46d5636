"""mums_find_batch on the cases of tests/batch_cases.py: the parts of the lanes' replay that random
ACGT pairs never reach (test_batch_cases_cpu.py holds every case to its path).  Per problem the
lengths, starts, AddHashEntry calls, collisions and restarts are those of the oracle's FindMatches
on that problem alone, under both routings (check_batch of test_gpu_batch.py)."""
import os

import numpy as np
import pytest

import batch_cases as bc
from test_gpu_batch import check_batch

pytestmark = pytest.mark.gpu


_FRESH = {}   # (G, table size) of case B -> its lists from a fresh object, for test_i_one_context_many_shapes


def run_case(gpu_lib, oracle_mod, case, mh=None):
    return check_batch(gpu_lib, oracle_mod, case["problems"], case["seed"], case["table_size"], case["mask"], mh=mh)


def same_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x.lengths, y.lengths) and np.array_equal(x.starts, y.starts)
                                    for x, y in zip(a, b))


def test_a_every_byte_value_through_the_lanes_table(gpu_lib, oracle_mod):
    case = bc.alphabet()
    lists, _ = run_case(gpu_lib, oracle_mod, case)
    assert all(len(ml) >= 1 for ml in lists)
    # a gap among bytes outside ACGT still names its problem
    at = case["bytes"].index(0xF0)
    bad = list(case["problems"])
    bad[at] = (bad[at][0][:200] + b"-" + bad[at][0][200:], bad[at][1])
    with gpu_lib.MemHash(0) as mh:
        with pytest.raises(gpu_lib.GapInSequence) as e:
            mh.FindMatchesBatch(bad, [case["seed"]] * len(bad))
        assert f"problem {at} " in str(e.value)


@pytest.mark.parametrize("G,table_size", bc.INSTANTIATION_CASES)
def test_b_every_replay_instantiation(gpu_lib, oracle_mod, G, table_size):
    lists, _ = run_case(gpu_lib, oracle_mod, bc.instantiation_case(G, table_size))
    assert all(len(ml) > 0 for ml in lists)
    _FRESH[(G, table_size)] = lists


@pytest.mark.parametrize("name", list(bc.MASK_CASES))
def test_c_masks_at_33_and_64_genomes(gpu_lib, oracle_mod, name):
    lists, _ = run_case(gpu_lib, oracle_mod, bc.mask_case(name))
    assert all(len(ml) >= 3 for ml in lists)


@pytest.mark.parametrize("name", list(bc.SORT_WIDTH_CASES))
def test_d_sort_width_at_and_over_64_bits(gpu_lib, oracle_mod, name):
    case = bc.sort_width_case(name)
    B = len(case["problems"])
    with gpu_lib.MemHash(0) as mh:
        lists, _ = run_case(gpu_lib, oracle_mod, case, mh=mh)
        # the context's list is the problems' lists in problem order (over 64 bits: no lanes'
        # pass at all, every row comes from a problem run alone)
        whole = mh.GetMatchList()
        mo = np.zeros(B + 1, dtype=np.uint64)
        mh._check(mh._lib.mums_batch_info(mh._ctx, mo.ctypes.data, None, None, None))
        st = mh.stats()
    assert all(len(ml) > 0 for ml in lists)
    assert np.array_equal(whole.lengths, np.concatenate([ml.lengths for ml in lists]))
    assert np.array_equal(whole.starts, np.concatenate([ml.starts for ml in lists]))
    assert mo.tolist() == np.concatenate([[0], np.cumsum([len(ml) for ml in lists])]).tolist()
    assert st["mem_count"] == len(whole)


def test_e_entry_pool_full(gpu_lib, oracle_mod):
    """More entries than the pool holds: which lanes find it full depends on scheduling, the
    result does not.  Twice on one object: through FindMatchesBatch with every problem kept in
    the lanes, then (the mirror's per-problem bookkeeping is most of this test's time) through
    mums_find_batch itself with the default routing."""
    case = bc.pool_case()
    problems, seed = case["problems"], case["seed"]
    B, K = len(problems), bc.POOL_CLASSES
    refs = [oracle_mod.find_matches([x, x], seed) for x in case["classes"]]
    cls = np.arange(B) % K

    def compare(whole, matches, probes, collisions, restarts):
        first = np.concatenate([[0], np.cumsum(matches.astype(np.int64))])
        assert int(first[-1]) == len(whole)
        for k, (rl, rs, st) in enumerate(refs):
            mine = cls == k
            assert (matches[mine] == len(rl)).all()
            assert (probes[mine] == st["probes"]).all()
            assert (collisions[mine] == st["collision_count"]).all()
            assert (restarts[mine] == st["restarts"]).all()
            rows = first[:-1][mine][:, None] + np.arange(len(rl))[None, :]
            assert (whole.lengths[rows] == rl[None, :]).all()
            assert (whole.starts[rows] == rs[None, :, :]).all()

    try:
        with gpu_lib.MemHash(0) as mh:
            os.environ["MUMS_DEV_BATCH_NO_SPLIT"] = "1"
            lists = mh.FindMatchesBatch(problems, [seed] * B)
            info = mh.BatchInfo()
            one = mh.GetMatchList()
            assert len(lists) == B and mh.stats()["mem_count"] == B and int(info["probes"].sum()) == B
            compare(one, info["matches"], info["probes"], info["collisions"], info["restarts"])
            for p in (0, 1, B // 2, B - 1):
                assert np.array_equal(lists[p].lengths, refs[p % K][0]) and np.array_equal(lists[p].starts, refs[p % K][1])
            os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT")
            blob = b"".join(s for prob in problems for s in prob)
            off = np.zeros(2 * B + 1, dtype=np.uint64)
            off[1:] = np.cumsum(np.fromiter((len(s) for prob in problems for s in prob), dtype=np.uint64, count=2 * B))
            mh._check(mh._lib.mums_find_batch(mh._ctx, B, 2, blob, off.ctypes.data))
            two = mh.GetMatchList()
            mo = np.zeros(B + 1, dtype=np.uint64)
            pr, co, rs = (np.zeros(B, dtype=np.uint64) for _ in range(3))
            mh._check(mh._lib.mums_batch_info(mh._ctx, mo.ctypes.data, pr.ctypes.data, co.ctypes.data, rs.ctypes.data))
            assert mh.stats()["mem_count"] == B and int(pr.sum()) == B
            compare(two, np.diff(mo.astype(np.int64)), pr, co, rs)
    finally:
        os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)
    assert np.array_equal(one.lengths, two.lengths) and np.array_equal(one.starts, two.starts)


def test_f_repeat_limit_edge(gpu_lib, oracle_mod):
    """A group of exactly MER_REPEAT_LIMIT stays in the lanes; one of 1001 goes through the
    single-problem pipeline although the reference does not restart on it (no head is left on
    the key, MatchFinder.cpp:253-277), and so does the genome order that restarts."""
    case = bc.repeat_limit_case()
    _, refs = run_case(gpu_lib, oracle_mod, case)
    for p, (group, restarts, _) in case["expect"].items():
        assert (refs[p]["max_group"], refs[p]["restarts"]) == (group, restarts)


def test_g_degenerate_sequences_in_wider_problems(gpu_lib, oracle_mod):
    case = bc.degenerate_case()
    lists, _ = run_case(gpu_lib, oracle_mod, case)
    for p, cols in case["empty"].items():
        assert len(lists[p]) >= 1 and (lists[p].starts[:, list(cols)] == 0).all()


@pytest.mark.parametrize("table_size", [40000, 7])
def test_h_repeat_rich_problems_in_the_lanes(gpu_lib, oracle_mod, table_size):
    case = bc.repeat_rich_case(table_size)
    _, refs = run_case(gpu_lib, oracle_mod, case)
    assert all(refs[p]["collision_count"] > 0.9 * refs[p]["probes"] for p in case["rich"])


def test_i_one_context_many_shapes(gpu_lib, oracle_mod):
    """Batches of other G, size and routing one after the other on one object (grow-only
    buffers, per-problem words, the pool's row stride): each as on a fresh object, whose result
    check_batch has compared with the oracle.  The reused object keeps every problem it can in
    the lanes, where the buffers are."""
    try:
        with gpu_lib.MemHash(0) as mh:
            for case in bc.context_sequence():
                fresh = _FRESH.get((case.get("G"), case["table_size"])) or run_case(gpu_lib, oracle_mod, case)[0]
                os.environ["MUMS_DEV_BATCH_NO_SPLIT"] = "1"
                mh.SetTableSize(case["table_size"])
                reused = mh.FindMatchesBatch(case["problems"], [case["seed"]] * len(case["problems"]))
                assert same_lists(reused, fresh)
    finally:
        os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)
