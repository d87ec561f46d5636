"""Seed families on the GPU: ClearSequences keeps the MemHash table, so the rounds of
progressiveMauve's pairwiseAnchorSearch (ProgressiveAligner.cpp:619-653: Clear, then per seed rank
ClearSequences + FindMatches) hash into one table.  After every round GetMatchList, MemCount,
MemCollisionCount, MemTableCount and the match log are compared with the recorded results of
tests/seed_family_model.c (golden/seed_family_cases.json, pinned to the live model and the oracle by
test_seed_family_cpu.py) and, where gcc is present, with the live model's arrays."""
import os
import subprocess

import numpy as np
import pytest

import seed_family_cases as sf
import test_eliminate_overlaps_v2_cpu as eo2
from conftest import ROOT

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def recorded():
    return sf.fixture()


@pytest.fixture(scope="module")
def live():
    """name -> the live model's rounds (None without gcc: the fixture alone decides)."""
    if not sf.have_compiler():
        return None
    L = sf.load_model()
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sf.run_model(L, sf.rounds_of(name))
        return cache[name]
    return get


def make_finder(lib, case):
    c = sf.CASES[case]
    mode = c.get("mode", {})
    if mode.get("pairwise"):
        mh = lib.PairwiseMatchFinder(0)
    elif mode.get("masked"):
        mh = lib.MaskedMemHash(0)
        mh.SetMask(mode["seq_mask"])
    else:
        mh = lib.MemHash(0)
    mh.SetTableSize(c["T"])
    if "repeat_tol" in mode:
        mh.SetRepeatTolerance(mode["repeat_tol"])
    if "enum_tol" in mode:
        mh.SetEnumerationTolerance(mode["enum_tol"])
    mh.SetMatchLog(True)
    return mh


def gpu_round(mh):
    ml = mh.GetMatchList()
    log = mh.MatchLog()
    st = mh.stats()
    return dict(lengths=ml.lengths, starts=ml.starts, mem_count=st["mem_count"], collisions=st["collision_count"],
                probes=st["probes"], table_counts=mh.MemTableCount(), log=(log.lengths, log.starts))


def check_round(got, rec, model_round, case):
    """One round against the live model's arrays (they locate a difference) and the fixture (it
    decides).  stats()["probes"] counts AddHashEntry calls only for a plain MemHash."""
    if model_round is not None:
        assert len(got["lengths"]) == len(model_round["lengths"])
        assert np.array_equal(got["lengths"], model_round["lengths"])
        assert np.array_equal(got["starts"], model_round["starts"])
        assert np.array_equal(got["table_counts"], model_round["table_counts"])
        assert np.array_equal(got["log"][0], model_round["log"][0])
        assert np.array_equal(got["log"][1], model_round["log"][1])
    d, rec = sf.digest(got), dict(rec)
    if case.get("mode"):
        d.pop("probes")
        rec.pop("probes")
    assert d == rec


def run_case(lib, recorded, live, name, after_round=None):
    model = live(name) if live is not None else None
    out = []
    with make_finder(lib, name) as mh:
        mh.Clear()
        for r, (seqs, seed, _) in enumerate(sf.rounds_of(name)):
            mh.ClearSequences()
            mh.SetSeed(seed)
            mh.FindMatches(seqs)
            got = gpu_round(mh)
            check_round(got, recorded[name][r], model[r] if model else None, sf.CASES[name])
            out.append(got)
            if after_round:
                after_round(mh, r, got)
    return out


@pytest.mark.parametrize("name", list(sf.CASES))
def test_family_rounds(gpu_lib, recorded, live, name):
    """Every round of every case against the fixture and the live model."""
    run_case(gpu_lib, recorded, live, name)


def test_repeated_seed_collides(gpu_lib, recorded, live):
    """Case 9: seed rank 0 a second time makes collisions only -- the list is unchanged and the
    collision count grows by that round's AddHashEntry calls.  (Rank 1 a second time inserts 7
    entries in the reference's algorithm, see test_seed_family_cpu.py; the model decides it.)"""
    r = run_case(gpu_lib, recorded, live, "c9_five_rounds")
    assert np.array_equal(r[3]["lengths"], r[2]["lengths"]) and np.array_equal(r[3]["starts"], r[2]["starts"])
    assert len(r[3]["log"][0]) == 0
    assert r[3]["collisions"] == r[2]["collisions"] + r[3]["probes"]


def test_full_anchor_chain(gpu_lib, live):
    """Case 10: three rounds, then EliminateOverlaps_v2 and LengthFilter(MIN_ANCHOR_LENGTH + 3) on
    the device list (ProgressiveAligner.cpp:646-659) = tests/eo2_model.cpp on the model's family
    list, then the length filter on the host (recorded; the live models' arrays where gcc is)."""
    with make_finder(gpu_lib, sf.FIRST) as mh:
        mh.Clear()
        for seqs, seed, _ in sf.rounds_of(sf.FIRST):
            mh.ClearSequences()
            mh.SetSeed(seed)
            mh.FindMatches(seqs)
        family = len(mh.GetMatchList())
        mh.EliminateOverlaps_v2()
        mh.LengthFilter(sf.CHAIN_MIN_LENGTH)
        got = mh.GetMatchList()
    assert 0 < len(got) < family
    if live is not None:
        el, es = sf.chain_of_model(eo2, eo2.load_model(), live(sf.FIRST)[-1])
        assert np.array_equal(got.lengths, el) and np.array_equal(got.starts, es)
    rec = sf.fixture_chain()
    assert sf.CHAIN_MIN_LENGTH == rec["min_length"]
    assert dict(count=len(got), md5=sf.list_md5(got.lengths, got.starts)) == dict(count=rec["count"], md5=rec["md5"])


# ---- the carried replay's paths (the k cases; test_seed_family_cpu.py holds each case to the path
# it exists for) -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k7_g32", "k8_g33"])
def test_mask_key_edge_buckets(gpu_lib, recorded, live, name):
    """G = 32 (every bit of entry_slot's presence mask) and G = 33 (the first count on dense block
    keys): after the last round every entry sits in its own bucket -- MemTableCount is the
    bincount of the returned list's entry buckets -- and each bucket's slice of the list is the
    model's, in the model's order.  The digests imply it; here a failure names the bucket."""
    T = sf.CASES[name]["T"]
    with make_finder(gpu_lib, name) as mh:
        mh.Clear()
        for seqs, seed, _ in sf.rounds_of(name):
            mh.ClearSequences()
            mh.SetSeed(seed)
            mh.FindMatches(seqs)
        got = gpu_round(mh)
    buckets = sf.oracle.entry_buckets(got["lengths"], got["starts"], T)
    counts = np.bincount(buckets, minlength=T)
    for b in range(T):
        assert got["table_counts"][b] == counts[b], f"bucket {b}"
    assert np.all(np.diff(buckets) >= 0)   # the list is the table, bucket-major
    if live is not None:
        m = live(name)[-1]
        ends = np.cumsum(counts)
        for b in range(T):
            sl = slice(int(ends[b] - counts[b]), int(ends[b]))
            assert np.array_equal(got["lengths"][sl], m["lengths"][sl]) and \
                np.array_equal(got["starts"][sl], m["starts"][sl]), f"bucket {b}"
    assert sf.digest(got) == recorded[name][-1]


def test_spill_in_mid_replay_reaches_the_anchor_chain(gpu_lib, recorded, live):
    """k1: the one bucket holds 6625 entries when round 1 starts and 13084 when it ends, so its
    vector leaves LDS between two inserts of one window.  The list after round 1 is the model's
    (check_round), and EliminateOverlaps_v2 + LengthFilter on it equal tests/eo2_model.cpp on the
    model's list: the spilled vector's ids made it into the table."""
    rounds = sf.rounds_of(sf.SPILL)[:2]
    with make_finder(gpu_lib, sf.SPILL) as mh:
        mh.Clear()
        for r, (seqs, seed, _) in enumerate(rounds):
            mh.ClearSequences()
            mh.SetSeed(seed)
            mh.FindMatches(seqs)
            check_round(gpu_round(mh), recorded[sf.SPILL][r], live(sf.SPILL)[r] if live else None, sf.CASES[sf.SPILL])
        family = len(mh.GetMatchList())
        mh.EliminateOverlaps_v2()
        mh.LengthFilter(sf.CHAIN_MIN_LENGTH)
        got = mh.GetMatchList()
    assert 0 < len(got) < family
    if live is not None:
        el, es = sf.chain_of_model(eo2, eo2.load_model(), live(sf.SPILL)[1])
        assert np.array_equal(got.lengths, el) and np.array_equal(got.starts, es)
    rec = sf.fixture_chain("chain_k1")
    assert sf.CHAIN_MIN_LENGTH == rec["min_length"]
    assert dict(count=len(got), md5=sf.list_md5(got.lengths, got.starts)) == dict(count=rec["count"], md5=rec["md5"])


def test_restart_round_after_a_refused_find(gpu_lib, recorded, oracle_mod):
    """k10 (one MER_REPEAT_LIMIT restart per round): a find with the wrong genome count onto the
    kept table is refused, the table stays, and round 1 onto it is the fixture's round 1."""
    (s0, seed0, _), (s1, seed1, _) = sf.rounds_of("k10_n_gapped")[:2]
    with make_finder(gpu_lib, "k10_n_gapped") as mh:
        mh.Clear()
        mh.ClearSequences()
        mh.SetSeed(seed0)
        mh.FindMatches(s0)
        assert sf.digest(gpu_round(mh)) == recorded["k10_n_gapped"][0]
        mh.ClearSequences()
        mh.SetSeed(seed1)
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.FindMatches(list(s1) + [s1[0]])
        assert e.value.code == gpu_lib.MUMS_E_INVALID
        mh.ClearSequences()
        mh.SetSeed(seed1)
        mh.FindMatches(s1)
        assert mh.stats()["restarts"] == oracle_mod.find_matches(s1, seed1, table_size=sf.CASES["k10_n_gapped"]["T"])[2]["restarts"] >= 1
        assert sf.digest(gpu_round(mh)) == recorded["k10_n_gapped"][1]


def test_family_without_the_match_log(gpu_lib, recorded):
    """k3 with SetMatchLog(False) (log_insert is a no-op then; every other test logs): the
    list, the counters and the table counts of every round are the fixture's."""
    name = "k3_small_edge_T300"
    with make_finder(gpu_lib, name) as mh:
        mh.SetMatchLog(False)
        mh.Clear()
        for r, (seqs, seed, _) in enumerate(sf.rounds_of(name)):
            mh.ClearSequences()
            mh.SetSeed(seed)
            mh.FindMatches(seqs)
            with pytest.raises(gpu_lib.MumsError):
                mh.MatchLog()   # nothing was logged
            ml, st = mh.GetMatchList(), mh.stats()
            empty = (np.zeros(0, np.uint64), np.zeros((0, 2), np.int64))
            d = sf.digest(dict(lengths=ml.lengths, starts=ml.starts, mem_count=st["mem_count"],
                               collisions=st["collision_count"], probes=st["probes"],
                               table_counts=mh.MemTableCount(), log=empty))
            for k in ("count", "list_md5", "mem_count", "collisions", "probes", "table_md5"):
                assert d[k] == recorded[name][r][k], (r, k)


# ---- case 11: edges -------------------------------------------------------------------------

def test_clear_sequences_on_a_fresh_context(gpu_lib, recorded, oracle_mod):
    seqs, seed, kw = sf.rounds_of(sf.FIRST)[0]
    ref_l, ref_s, st = oracle_mod.find_matches(seqs, seed, **kw)
    with make_finder(gpu_lib, sf.FIRST) as mh:
        mh.ClearSequences()
        mh.ClearSequences()
        mh.SetSeed(seed)
        ml = mh.FindMatches(seqs)
        assert np.array_equal(ml.lengths, ref_l) and np.array_equal(ml.starts, ref_s)
        assert mh.MemCollisionCount() == st["collision_count"]
        assert sf.digest(gpu_round(mh)) == recorded[sf.FIRST][0]


def test_clear_drops_the_table(gpu_lib, recorded):
    rounds = sf.rounds_of(sf.FIRST)
    with make_finder(gpu_lib, sf.FIRST) as mh:
        for seqs, seed, _ in rounds[:2]:
            mh.ClearSequences()
            mh.SetSeed(seed)
            mh.FindMatches(seqs)
        assert len(mh.GetMatchList()) == recorded[sf.FIRST][1]["count"]
        mh.Clear()
        st = mh.stats()
        assert st["mem_count"] == 0 and st["collision_count"] == 0
        mh.ClearSequences()
        mh.SetSeed(rounds[0][1])
        mh.FindMatches(rounds[0][0])   # from an empty table again: round 0
        assert sf.digest(gpu_round(mh)) == recorded[sf.FIRST][0]


def test_two_finds_without_clear_sequences_start_empty(gpu_lib, recorded):
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[0]
    with make_finder(gpu_lib, sf.FIRST) as mh:
        mh.SetSeed(seed)
        mh.FindMatches(seqs)
        assert sf.digest(gpu_round(mh)) == recorded[sf.FIRST][0]
        mh.FindMatches(None)
        assert sf.digest(gpu_round(mh)) == recorded[sf.FIRST][0]


def kept_table_after_round0(lib):
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[0]
    mh = make_finder(lib, sf.FIRST)
    mh.ClearSequences()
    mh.SetSeed(seed)
    mh.FindMatches(seqs)
    mh.ClearSequences()
    return mh


def finish_round1(mh, recorded):
    """A plain round 1 onto the kept table: it was left intact."""
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[1]
    mh.SetSeed(seed)
    mh.FindMatches(seqs)
    assert sf.digest(gpu_round(mh)) == recorded[sf.FIRST][1]


def test_other_genome_count_is_invalid(gpu_lib, recorded):
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[1]
    with kept_table_after_round0(gpu_lib) as mh:
        mh.SetSeed(seed)
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.FindMatches(list(seqs) + [seqs[0]])
        assert e.value.code == gpu_lib.MUMS_E_INVALID
        mh.ClearSequences()   # the three genomes go, the kept table stays
        finish_round1(mh, recorded)


def test_other_table_size_is_invalid(gpu_lib, recorded):
    with kept_table_after_round0(gpu_lib) as mh:
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.SetTableSize(sf.CASES[sf.FIRST]["T"] + 1)
        assert e.value.code == gpu_lib.MUMS_E_INVALID
        mh.SetRepeatTolerance(0)                # re-sends the kept table's size: fine
        finish_round1(mh, recorded)


def test_clear_sequences_after_a_filter_is_invalid(gpu_lib):
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[0]
    with make_finder(gpu_lib, sf.FIRST) as mh:
        mh.SetSeed(seed)
        mh.FindMatches(seqs)
        mh.LengthFilter(30)
        before = mh.GetMatchList()
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.ClearSequences()
        assert e.value.code == gpu_lib.MUMS_E_INVALID
        after = mh.GetMatchList()
        assert 0 < len(before) and np.array_equal(before.lengths, after.lengths) and \
            np.array_equal(before.starts, after.starts)


def test_compat_mode_is_unsupported_and_keeps_the_table(gpu_lib, recorded):
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[1]
    with kept_table_after_round0(gpu_lib) as mh:
        mh._check(mh._lib.mums_set_parallel_compat(mh._ctx, 1, 0))
        mh.SetSeed(seed)
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.FindMatches(seqs)
        assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED
        mh._check(mh._lib.mums_set_parallel_compat(mh._ctx, 0, 0))
        mh.ClearSequences()
        finish_round1(mh, recorded)


def test_chunked_mode_is_unsupported_and_keeps_the_table(gpu_lib, recorded, monkeypatch):
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[1]
    with kept_table_after_round0(gpu_lib) as mh:
        monkeypatch.setenv("MUMS_DEV_CHUNK_RECORDS", "8192")
        mh.SetSeed(seed)
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.FindMatches(seqs)
        assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED
        monkeypatch.delenv("MUMS_DEV_CHUNK_RECORDS")
        mh.ClearSequences()
        finish_round1(mh, recorded)


@pytest.mark.parametrize("first,second", [(7, 40000), (40000, 7)])
def test_table_size_changed_before_clear_sequences_empties_the_table(gpu_lib, oracle_mod, first, second):
    """FindMatches, SetTableSize(other), ClearSequences, FindMatches: SetTableSize empties the
    table (MemHash.cpp:95-102), so nothing is carried and the second find is a plain find at the
    new size -- a larger and a smaller size (the finished find's own counts are what is kept)."""
    (s0, seed0, _), (s1, seed1, _) = sf.rounds_of(sf.FIRST)[:2]
    ref_l, ref_s, st = oracle_mod.find_matches(s1, seed1, table_size=second)
    with gpu_lib.MemHash(0) as mh:
        mh.SetTableSize(first)
        mh.SetSeed(seed0)
        assert len(mh.FindMatches(s0)) > 0
        mh.SetTableSize(second)
        mh.ClearSequences()
        assert int(mh.MemTableCount().sum()) == 0
        mh.SetSeed(seed1)
        ml = mh.FindMatches(s1)
        assert np.array_equal(ml.lengths, ref_l) and np.array_equal(ml.starts, ref_s)
        assert mh.MemCollisionCount() == st["collision_count"]


def test_genomes_added_after_the_find_do_not_change_the_kept_table(gpu_lib, recorded):
    """A genome added after the find and a seed-stage-only run in between: ClearSequences still
    keeps the finished find's table, with that find's sequence count."""
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[0]
    with make_finder(gpu_lib, sf.FIRST) as mh:
        mh.SetSeed(seed)
        mh.FindMatches(seqs)
        mh.AddSequence(seqs[0])
        mh.FindStage(gpu_lib.STAGE_SEEDS)
        mh.ClearSequences()
        finish_round1(mh, recorded)


def test_table_counts_readable_after_clear_sequences(gpu_lib, live, recorded):
    """mem_table_count survives ClearSequences (MemHash.cpp:71-74) and can be read before the next find."""
    import hashlib
    with kept_table_after_round0(gpu_lib) as mh:
        counts = mh.MemTableCount()
        assert hashlib.md5(np.ascontiguousarray(counts, dtype="<u4").tobytes()).hexdigest() == \
            recorded[sf.FIRST][0]["table_md5"]
        assert int(counts.sum()) == recorded[sf.FIRST][0]["count"]
        finish_round1(mh, recorded)


def test_clear_sequences_after_a_compat_find_refuses_at_the_next_find(gpu_lib):
    """ParallelMemHash: ClearSequences itself is fine, the find onto the kept table is refused."""
    seqs, seed, _ = sf.rounds_of(sf.FIRST)[0]
    with gpu_lib.ParallelMemHash(0) as mh:
        mh.SetSeed(seed)
        assert len(mh.FindMatches(seqs)) > 0
        mh.ClearSequences()
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.FindMatches(seqs)
        assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED
        mh.Clear()
        assert len(mh.FindMatches(seqs)) > 0


# ---- case 12: the C++ mirror ------------------------------------------------------------------

def test_cpp_family_loop(recorded):
    """include/mums_memhash.hpp: Clear, three times ClearSequences + FindMatches, GetMatchList
    (tools/mums_find family) = the fixture's last round of case 1."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools")], check=True)
    c = sf.CASES[sf.FIRST]
    r = subprocess.run([os.path.join(ROOT, "tools", "mums_find"), "family", str(c["G"]), str(c["n"]), str(c["w"]),
                        str(c["p"])], check=True, capture_output=True, timeout=300)
    rows = np.array([[int(x) for x in l.split("\t")] for l in r.stdout.decode().splitlines()], dtype=np.int64)
    rec = recorded[sf.FIRST][-1]
    assert len(rows) == rec["count"]
    assert sf.list_md5(rows[:, 0].astype(np.uint64), rows[:, 1:]) == rec["list_md5"]
    assert f"mems {rec['mem_count']} collisions {rec['collisions']}".encode() in r.stderr, r.stderr


def test_round_without_probes_keeps_the_table(gpu_lib, recorded, live):
    """A round whose sequences share no seed makes no AddHashEntry call: GetMatchList is still
    the whole (kept) table, the counters stay, the match log is empty."""
    seqs, seed, kw = sf.rounds_of(sf.FIRST)[0]
    empty = [b"A" * 60, b"C" * 60]
    if live is not None:
        m = sf.run_model(sf.load_model(), [(seqs, seed, kw), (empty, seed, kw)])[1]
        assert m["probes"] == 0 and sf.digest(m) == dict(recorded[sf.FIRST][0], log_count=0, log_md5=sf.list_md5([], []),
                                                          log_set_md5=sf.log_set_md5(([], np.zeros((0, 2)))), probes=0)
    with kept_table_after_round0(gpu_lib) as mh:
        mh.FindMatches(empty)
        got = gpu_round(mh)
        assert sf.digest(got) == dict(recorded[sf.FIRST][0], log_count=0, log_md5=sf.list_md5([], []),
                                      log_set_md5=sf.log_set_md5(([], np.zeros((0, 2)))), probes=0)
        mh.ClearSequences()
        finish_round1(mh, recorded)
