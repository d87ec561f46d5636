"""ParallelMemHash compat over several ranks (mums_shard_run on a compat context,
compat_ranks.hip) under enumeration tolerance > 1: every rank enumerates the
odometer rows of its chunk range into tables of its own, the bucket owners re-add the ranks'
tables rank after rank.  The ranks' lists in rank order = the one-thread oracle's MatchList, bit
for bit.  Ranks are threads of one process sharing device 0 (the in-process communicator)."""
import numpy as np
import pytest

from tests.compat_enum_inputs import SHAPES, make_input, oracle_answer

pytestmark = pytest.mark.gpu


def check(gpu_lib, oracle_mod, spec, w, rt, et, chunk, world, table_size=40000):
    lengths, starts, ost = oracle_answer(spec, w, rt, et, chunk, False, 0, table_size)
    with gpu_lib.ShardedMemHash([0] * world, comm="local", table_size=table_size, parallel_compat=True,
                                chunk_size=chunk) as sh:
        sh.SetSeed(oracle_mod.get_seed(w))
        sh.SetRepeatTolerance(rt)
        sh.SetEnumerationTolerance(et)
        ml = sh.FindMatches(list(make_input(spec)))
        st = sh.stats_per_rank
    assert all(s["chunks"] == ost["chunks"] for s in st)
    assert len(ml) == len(lengths)
    assert np.array_equal(ml.lengths, lengths) and np.array_equal(ml.starts, starts)
    return ost


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("sid", ["A", "C", "H"])
def test_compat_enum_ranks_vs_oracle(gpu_lib, oracle_mod, sid, world):
    spec, w, rt, et, chunk, _, _ = SHAPES[sid]
    check(gpu_lib, oracle_mod, spec, w, rt, et, chunk, world)


def test_compat_enum_ranks_cut_chunks(gpu_lib, oracle_mod):
    """Chunks cut at their first group above MER_REPEAT_LIMIT, decided per chunk before the
    ranks take their ranges."""
    spec, w, rt, et, chunk, _, _ = SHAPES["L"]
    ost = check(gpu_lib, oracle_mod, spec, w, rt, et, chunk, 3)
    assert ost["restarts"] > 0


def test_compat_enum_ranks_small_table(gpu_lib, oracle_mod):
    spec, w, rt, et, chunk, _, _ = SHAPES["A"]
    check(gpu_lib, oracle_mod, spec, w, rt, et, chunk, 2, table_size=7)


def test_compat_enum_ranks_more_ranks_than_chunks(gpu_lib, oracle_mod):
    """3 chunks over 4 ranks: a rank with an empty chunk range holds an empty table."""
    ost = check(gpu_lib, oracle_mod, ("rep", 3, 60_000, 0.02, 34), 15, 1, 2, 25_000, 4)
    assert ost["chunks"] == 3


@pytest.mark.parametrize("world", [2])
def test_compat_enum_ranks_match_log_refused(gpu_lib, oracle_mod, world):
    spec, w, rt, et, chunk, _, _ = SHAPES["A"]
    with gpu_lib.ShardedMemHash([0] * world, comm="local", parallel_compat=True, chunk_size=chunk) as sh:
        sh.SetSeed(oracle_mod.get_seed(w))
        sh.SetRepeatTolerance(rt)
        sh.SetEnumerationTolerance(et)
        sh.SetMatchLog(True)
        with pytest.raises(gpu_lib.MumsError, match="match log"):
            sh.FindMatches(list(make_input(spec)))
        assert sh.rank_status == [gpu_lib.MUMS_E_UNSUPPORTED] * world, sh.rank_status
