"""GPU parity on rearranged genomes (tests/rearranged_inputs.py): hundreds to thousands of lines
per MatchList (chains.hip's line sort, links and segment scan between neighbours of different
lines; replay.hip's buckets filled from many offsets; bucket owners that really share the work
in the sharded path) and walks of tens of thousands of columns (the short tier, the 16-lane
tier's hand-off and the whole-wave launch of chain_walk_kernel).  Every comparison is bit for
bit against the oracle, whose MatchLists on these inputs tests/test_rearranged_cpu.py checks
from the sequences alone."""
import shutil

import numpy as np
import pytest

from tests import rearranged_inputs as ri
from tests.test_gpu_row_paths import VARIANTS

pytestmark = pytest.mark.gpu


def make_finder(lm, opts):
    cls = opts.get("cls", "MemHash")
    mh = lm.ParallelMemHash(0, chunk_size=opts["chunk_size"]) if cls == "ParallelMemHash" else getattr(lm, cls)(0)
    mh.SetTableSize(opts.get("table_size", 40000))
    mh.SetRepeatTolerance(opts.get("repeat_tol", 0))
    mh.SetEnumerationTolerance(opts.get("enum_tol", 1))
    if cls == "MaskedMemHash":
        mh.SetMask(opts["seq_mask"])
    return mh


def assert_parity(ml, st, ref, opts, note=None):
    """MatchList and counters of a GPU find against the oracle's, bit for bit."""
    lengths, starts, ost = ref
    assert len(ml) == len(lengths), (note, len(ml), len(lengths))
    assert np.array_equal(ml.lengths, lengths) and np.array_equal(ml.starts, starts), note
    assert st["probes"] == ost["probes"], note
    if opts.get("cls") == "ParallelMemHash":
        # (the compat mode's collision count is not the thread tables' sum: test_gpu_tie_order.py)
        assert st["chunks"] == ost["chunks"] and st["mem_count"] == len(lengths), note
    else:
        assert st["collision_count"] == ost["collision_count"], note
        assert st["mem_count"] == ost["mem_count"], note


@pytest.mark.parametrize("name", sorted(ri.CASES))
def test_modes(gpu_lib, oracle_mod, name):
    """Every case through its class, with the match log (the order-sensitive check of the
    replay) and, for MemHash under the default tolerances, the seed stage's probe sequence."""
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, ost = ri.oracle_result(oracle_mod, name)
    with make_finder(gpu_lib, opts) as mh:
        mh.SetSeed(seed)
        mh.SetMatchLog(True)
        ml = mh.FindMatches(seqs)
        st = mh.stats()
        log = mh.MatchLog()
    assert_parity(ml, st, (lengths, starts, ost), opts)
    ref_len, ref_s = ost["match_log"]
    assert len(log) == len(ref_len)
    assert np.array_equal(log.lengths, ref_len) and np.array_equal(log.starts, ref_s)
    # (mums_probe_copy exists on the packed-record path only: 2w + 1 <= 43 key bits; the
    # solid w25 / w27 / w31 seeds are refused there with MUMS_E_UNSUPPORTED)
    if ri.is_default_memhash(opts) and 2 * bin(seed).count("1") + 1 <= 43:
        ob, orf, pst = oracle_mod.seed_probes(seqs, seed, table_size=opts.get("table_size", 40000))
        with make_finder(gpu_lib, opts) as mh:
            mh.SetSeed(seed)
            for s in seqs:
                mh.AddSequence(s)
            mh.FindStage(gpu_lib.STAGE_SEEDS)
            b, r = mh.Probes()
        assert len(b) == pst["probes"] == ost["probes"]
        assert np.array_equal(b, ob) and np.array_equal(r, orf)


def path_variants(chunk):
    """test_gpu_row_paths.VARIANTS with this case's slice size, plus the line order forced exact
    or onto the pair sort, the walks' generic hit words and the big-bucket replay forced onto
    small buckets (the values of test_gpu_replay_big.py)."""
    out = [{k: (str(chunk) if k == "MUMS_DEV_FIND_CHUNK" else v) for k, v in var.items()} for var in VARIANTS]
    out += [{"MUMS_DEV_LINE_EXACT": "1"}, {"MUMS_DEV_WALK_GEN": "1"},
            {"MUMS_DEV_BIG_BUCKET": "8"}, {"MUMS_DEV_BIG_BUCKET": "8", "MUMS_DEV_GRID_SLOW": "0"},
            {"MUMS_DEV_LINE_EXACT": "1", "MUMS_DEV_FIND_CHUNK": str(chunk)},
            # the line order by the 64-bit pair sort (the full product: test_gpu_chain_paths.py)
            {"MUMS_DEV_LINE_RADIX": "1"}, {"MUMS_DEV_LINE_RADIX": "1", "MUMS_DEV_FIND_CHUNK": str(chunk)}]
    return out


@pytest.mark.parametrize("name", ["ev_G4_w15", "ev_G4_w15_t7", "ev_G9_w13", "ls_G3_x40k_w15"])
def test_paths_one_process(gpu_lib, oracle_mod, monkeypatch, name):
    """One context, the development switches toggled per call, CreateMatches per variant: every
    path gives the oracle's MatchList and counters."""
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, ost = ri.oracle_result(oracle_mod, name)
    chunk = max(ost["probes"] // 4, 1)
    with make_finder(gpu_lib, opts) as mh:
        mh.SetSeed(seed)
        for s in seqs:
            mh.AddSequence(s)
        for var in path_variants(chunk):
            with monkeypatch.context() as m:
                for k, v in var.items():
                    m.setenv(k, v)
                mh.CreateMatches()
                st = mh.stats()
                ml = mh.GetMatchList()
            assert_parity(ml, st, (lengths, starts, ost), opts, var)
            if "MUMS_DEV_FIND_CHUNK" in var:
                assert st["probes"] > chunk, var


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
@pytest.mark.parametrize("name", ri.STRETCH)
def test_long_walk_tiers(gpu_lib, oracle_mod, monkeypatch, name, sliced):
    """Walks through a probe-free copy of X: longer than the short tier (8 words) and the 16-lane
    tier's 16 steps of 16 words cover, so they end in the whole-wave launch after the hand-off.
    The counter floors come from the input's geometry (the CPU precondition's stretches), not
    from a GPU measurement.  sliced: MUMS_DEV_FIND_CHUNK cuts the probes into slices, a long
    chain's probes fall into different ones and are merged by entry content."""
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, ost = ri.oracle_result(oracle_mod, name)
    found = [f for f in ri.stretches(oracle_mod, name) if f[1] >= opts["xlen"] - ri.STRETCH_SLACK]
    assert len(found) >= 2
    chunk = max(ost["probes"] // 5, 1)
    if sliced:
        monkeypatch.setenv("MUMS_DEV_FIND_CHUNK", str(chunk))
    with make_finder(gpu_lib, opts) as mh:
        mh.SetSeed(seed)
        ml = mh.FindMatches(seqs)
        st = mh.stats()
    print(name, "sliced" if sliced else "whole", {k: st[k] for k in ("short_walks", "short_walk_words", "chain_walks",
                                                                     "chain_walk_words", "chains", "probes")},
          "stretches", [f[1] for f in found])
    assert_parity(ml, st, (lengths, starts, ost), opts)
    if sliced:
        assert st["probes"] > chunk
    assert st["short_walks"] > 0
    assert st["chain_walks"] >= len(found)
    assert st["chain_walk_words"] >= sum(f[1] for f in found) // 64


@pytest.mark.parametrize("name,world,layout", [("ev_G4_w15", 2, "blocks"), ("ev_G4_w15", 4, "blocks"),
                                               ("ev_G4_w15_t7", 2, "blocks"), ("ev_G4_w15_t7", 4, "blocks"),
                                               ("ev_G2_w15", 2, "slices")])
def test_sharded(gpu_lib, oracle_mod, name, world, layout):
    """The sharded path with many diagonals: the ranks' lists in rank order are the oracle's
    list, and more than one bucket owner has replay work (on collinear inputs one rank owns it
    all, test_gpu_shard_abi.py)."""
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, ost = ri.oracle_result(oracle_mod, name)
    T = opts.get("table_size", 40000)
    with gpu_lib.ShardedMemHash([0] * world, comm="local", table_size=T, layout=layout) as sh:
        sh.SetSeed(seed)
        ml = sh.FindMatches(seqs)
        per_rank = [(s["mem_count"], s["collision_count"]) for s in sh.stats_per_rank]
    print(name, world, layout, "per rank (mem_count, collision_count):", per_rank)
    assert len(ml) == len(lengths)
    assert np.array_equal(ml.lengths, lengths) and np.array_equal(ml.starts, starts)
    assert sum(c for _, c in per_rank) == ost["collision_count"]
    assert sum(m for m, _ in per_rank) == ost["mem_count"]
    assert sum(1 for m, c in per_rank if m or c) > 1


def check_batch(gpu_lib, oracle_mod):
    """FindMatchesBatch over small rearranged problems: each list equals a single find's and the
    oracle's, with its counters."""
    problems = ri.batch_problems()
    patterns, _ = gpu_lib.batch_seed_groups(problems)
    with gpu_lib.MemHash(0) as mh:
        lists = mh.FindMatchesBatch(problems)
        info = mh.BatchInfo()
    total = 0
    for p, prob in enumerate(problems):
        assert patterns[p] != 0
        lengths, starts, ost = oracle_mod.find_matches(list(prob), patterns[p])
        assert np.array_equal(lists[p].lengths, lengths) and np.array_equal(lists[p].starts, starts), p
        assert int(info["probes"][p]) == ost["probes"] and int(info["collisions"][p]) == ost["collision_count"], p
        with gpu_lib.MemHash(0) as mh:
            mh.SetSeed(patterns[p])
            single = mh.FindMatches(list(prob))
        assert np.array_equal(single.lengths, lengths) and np.array_equal(single.starts, starts), p
        total += len(lengths)
    assert total > 40


def check_family(gpu_lib, oracle_mod):
    """One seed family (ClearSequences keeps the table; seed ranks 0, 1, 2) on a rearranged input,
    every round against the model of tests/seed_family_cases.py."""
    import seed_family_cases as sf
    if not sf.have_compiler():
        pytest.skip("no gcc: the seed family model cannot be built")
    rounds = ri.family_rounds(oracle_mod)
    model = sf.run_model(sf.load_model(), rounds)
    with gpu_lib.MemHash(0) as mh:
        mh.SetMatchLog(True)
        mh.Clear()
        for r, (seqs, seed, _) in enumerate(rounds):
            mh.ClearSequences()
            mh.SetSeed(seed)
            ml = mh.FindMatches(seqs)
            log, st = mh.MatchLog(), mh.stats()
            assert np.array_equal(ml.lengths, model[r]["lengths"]) and np.array_equal(ml.starts, model[r]["starts"]), r
            assert np.array_equal(log.lengths, model[r]["log"][0]) and np.array_equal(log.starts, model[r]["log"][1]), r
            assert st["mem_count"] == model[r]["mem_count"] and st["collision_count"] == model[r]["collisions"], r
            assert np.array_equal(mh.MemTableCount(), model[r]["table_counts"]), r


def test_batch_and_family(gpu_lib, oracle_mod):
    check_batch(gpu_lib, oracle_mod)
    check_family(gpu_lib, oracle_mod)


def test_eliminate_overlaps_on_device_list(gpu_lib, oracle_mod):
    """EliminateOverlaps and EliminateOverlaps_v2 on the device-resident MatchList of a find whose
    entries really overlap (w11 on rearranged genomes: duplications, tandem arrays, subsets)."""
    import test_eliminate_overlaps_v2_cpu as eo2
    name = ri.OVERLAP_CASE
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, _ = ri.oracle_result(oracle_mod, name)
    ref_l, ref_s = oracle_mod.eliminate_overlaps(lengths, starts)
    assert len(ref_l) != len(lengths) or not np.array_equal(ref_s, starts)
    model = eo2.load_model() if shutil.which("g++") else None
    with make_finder(gpu_lib, opts) as mh:
        mh.SetSeed(seed)
        for s in seqs:
            mh.AddSequence(s)
        mh.CreateMatches()
        mh.EliminateOverlaps()
        got = mh.GetMatchList()
        assert len(got) == len(ref_l)
        assert np.array_equal(got.lengths, ref_l) and np.array_equal(got.starts, ref_s)
        if model is None:
            pytest.skip("no g++: EliminateOverlaps_v2's model cannot be built (v1 compared)")
        for both in (False, True):
            ml, ms, cnt = eo2.model_eo2(model, lengths, starts, None, both)
            assert cnt["pairs"] > 0 and (len(ml) != len(lengths) or not np.array_equal(ms, starts))
            mh.CreateMatches()
            mh.EliminateOverlaps_v2(None, both)
            got = mh.GetMatchList()
            assert len(got) == len(ml), both
            assert np.array_equal(got.lengths, ml) and np.array_equal(got.starts, ms), both
