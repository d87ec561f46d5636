"""Seed families, CPU side: tests/seed_family_model.c (the oracle's find_match_seeds looped over
the seed ranks on one memhash_t, as ClearSequences + FindMatches do on one MemHash,
ProgressiveAligner.cpp:619-653) is pinned to the oracle by its first round, the recorded fixture
golden/seed_family_cases.json equals the live model, and the family result is neither a
single-seed result nor independent of the seed order."""
from __future__ import annotations

import numpy as np
import pytest

import seed_family_cases as sf
from oracle import oracle

@pytest.fixture(scope="module")
def model():
    return sf.load_model()


@pytest.fixture(scope="module")
def results(model):
    """The live model on every case, computed once."""
    return {name: sf.run_model(model, sf.rounds_of(name)) for name in sf.CASES}


@pytest.mark.parametrize("name", list(sf.CASES))
def test_first_round_is_the_oracle(results, name):
    seqs, seed, kw = sf.rounds_of(name)[0]
    ref_len, ref_s, st = oracle.find_matches(seqs, seed, **kw)
    r0 = results[name][0]
    assert np.array_equal(r0["lengths"], ref_len) and np.array_equal(r0["starts"], ref_s)
    assert r0["mem_count"] == st["mem_count"] == len(ref_len)
    assert r0["collisions"] == st["collision_count"]
    assert r0["probes"] == st["probes"]
    assert int(r0["table_counts"].sum()) == len(ref_len)
    log_len, log_s = st["match_log"]
    # (PairwiseMatchFinder too: the oracle hashes a seed group's pairs in the reference's order,
    # sorted by sequence id, PairwiseMatchFinder.cpp:39, as the model always did)
    assert np.array_equal(r0["log"][0], log_len) and np.array_equal(r0["log"][1], log_s)


@pytest.mark.parametrize("name", list(sf.CASES))
def test_fixture_equals_live_model(results, name):
    fx = sf.fixture()
    assert set(fx) == set(sf.CASES)
    assert [sf.digest(r) for r in results[name]] == fx[name]


def test_chain_fixture_equals_live_models(results):
    import test_eliminate_overlaps_v2_cpu as eo2
    cl, cs = sf.chain_of_model(eo2, eo2.load_model(), results[sf.FIRST][-1])
    rec = sf.fixture_chain()
    assert rec == dict(count=int(len(cl)), md5=sf.list_md5(cl, cs), min_length=sf.CHAIN_MIN_LENGTH)
    assert 0 < len(cl) < len(results[sf.FIRST][-1]["lengths"])
    # the spilled vector of k1 after round 1
    cl, cs = sf.chain_of_model(eo2, eo2.load_model(), results[sf.SPILL][1])
    assert sf.fixture_chain("chain_k1") == dict(count=int(len(cl)), md5=sf.list_md5(cl, cs), min_length=sf.CHAIN_MIN_LENGTH)
    assert 0 < len(cl) < len(results[sf.SPILL][1]["lengths"])


def test_counters_are_cumulative(results):
    for name, rounds in results.items():
        coll = 0
        for r in rounds:
            assert r["mem_count"] == len(r["lengths"]) == int(r["table_counts"].sum())
            assert coll <= r["collisions"] <= coll + r["probes"]
            assert r["collisions"] - coll + len(r["log"][0]) == r["probes"]   # every call collides or inserts
            coll = r["collisions"]


def test_family_is_no_single_seed_result_and_depends_on_the_order(model, results):
    fam = results[sf.FIRST][-1]
    fam_md5 = sf.list_md5(fam["lengths"], fam["starts"])
    for seqs, seed, kw in sf.rounds_of(sf.FIRST):
        one = sf.run_model(model, [(seqs, seed, kw)])[0]
        assert sf.list_md5(one["lengths"], one["starts"]) != fam_md5
        assert len(one["lengths"]) != len(fam["lengths"])
    other = results["c1_order_201"][-1]
    assert sf.list_md5(other["lengths"], other["starts"]) != fam_md5
    assert len(other["lengths"]) != len(fam["lengths"])


def test_repeated_seed_only_collides(results):
    """Rank 0 again (round 3) only collides: the list is unchanged and the collision count grows
    by the round's AddHashEntry calls.  Rank 1 again (round 4) does NOT only collide in the
    reference's algorithm: entries of rank 2 that partly overlap a rank-1 chain now stand
    between lower_bound and the chain's own entry (the non-transitive MheCompare), so a few
    probes (7 on this input) are extended and inserted a second time.  The model decides."""
    r = results["c9_five_rounds"]
    assert np.array_equal(r[3]["lengths"], r[2]["lengths"]) and np.array_equal(r[3]["starts"], r[2]["starts"])
    assert len(r[3]["log"][0]) == 0
    assert r[3]["collisions"] == r[2]["collisions"] + r[3]["probes"]
    assert len(r[4]["lengths"]) == len(r[3]["lengths"]) + len(r[4]["log"][0])
    assert r[4]["collisions"] == r[3]["collisions"] + r[4]["probes"] - len(r[4]["log"][0])


def test_spill_case_starts_above_the_lds_vector(results):
    """Case 4 exists for a carried vector larger than the replay's LDS capacity (kReplayLdsIds)."""
    import re
    import os
    src = open(os.path.join(sf.ROOT, "libmems_amd", "csrc", "mums_capi.hip")).read()
    cap = int(re.search(r"kReplayLdsIds\s*=\s*(\d+)", src).group(1))
    assert len(results["c4_one_bucket_spill"][0]["lengths"]) > cap


# condition of the carried replay (replay_carried_kernel / launch_replay_carried) -> the case
# that exists for it; test_cases_reach_the_carried_replays_paths holds each case to its condition
PATHS = {
    "spill in mid-replay": "k1_spill_mid_replay",
    "vector starts in global memory": "c4_one_bucket_spill",
    "v == kSmall": "k3_small_edge_T300",
    "v == kSmall + 1": "k3_small_edge_T300",
    "long LDS-resident vector": "k2_lds_carried_T3",
    "K > 1024": "k2_lds_carried_T3",
    "K > 512": "k4_g6",
    "K > 256": "k5_g12",
    "carried-only bucket": "k6_g24",
    "new-only bucket": "c1_pairwise_anchor",
    "G in 1..4": "c5_g4_diagonal",
    "G in 5..8": "k4_g6",
    "G in 9..16": "k5_g12",
    "G in 17..32": "k6_g24",
    "G in 33..64": "c6_g34_dense_blocks",
    "G == 32": "k7_g32",
    "G == 33": "k8_g33",
    "one probe": "k12_one_probe",
    "restarts": ("k10_n_gapped", "k11_high_copy"),
}


def carried_paths(results, cases, cap, small, lanes):
    """condition -> set of the plain cases (no `mode`: oracle.seed_probes is a plain MemHash)
    with a carried round that meets it.  Per bucket of a carried round: nc carried entries, K
    probes, v = nc + K (what launch_replay_carried dispatches on), t entries after the round."""
    hit = {}

    def mark(what, name, cond):
        if np.any(cond):
            hit.setdefault(what, set()).add(name)

    for name, c in cases.items():
        if c.get("mode"):
            continue
        G, T = c["G"], c["T"]
        rb = lanes(G)
        for lo, hi in ((1, 4), (5, 8), (9, 16), (17, 32), (33, 64)):
            mark(f"G in {lo}..{hi}", name, lo <= G <= hi)
        mark("G == 32", name, G == 32)
        mark("G == 33", name, G == 33)
        rounds = sf.rounds_of(c)
        restarts = []
        for r, (seqs, seed, kw) in enumerate(rounds):
            res = results[name][r]
            if "gen" in c:
                restarts.append(oracle.find_matches(seqs, seed, **kw)[2]["restarts"])
            if r == 0:
                continue
            bucket, _, st = oracle.seed_probes(seqs, seed, table_size=T)
            assert st["probes"] == res["probes"] == len(bucket)
            nc = results[name][r - 1]["table_counts"].astype(np.int64)
            K = np.bincount(bucket, minlength=T).astype(np.int64)
            t = res["table_counts"].astype(np.int64)
            v = nc + K
            assert np.all(nc <= t) and np.all(t <= v)
            mark("spill in mid-replay", name, (nc <= cap) & (cap < t))
            mark("vector starts in global memory", name, nc > cap)
            mark("v == kSmall", name, v == small)
            mark("v == kSmall + 1", name, v == small + 1)
            mark("long LDS-resident vector", name, (v > small) & (1000 <= nc) & (t - nc >= 1000) & (t <= cap))
            mark(f"K > {rb}", name, K > rb)
            mark("carried-only bucket", name, (K == 0) & (nc > 0))
            mark("new-only bucket", name, (nc == 0) & (K > 0))
            mark("one probe", name, res["probes"] == 1)
            mark("no probe", name, res["probes"] == 0)
        mark("restarts", name, len(restarts) > 0 and min(restarts) >= 1)
    return hit


def replay_constants():
    """(kReplayLdsIds, kSmall of launch_replay_carried, lanes of the wide launch by G) read out of
    the sources; replay_block is pinned by its text, a change of the lane counts fails here
    instead of silently moving the edges the cases were chosen for."""
    import os
    import re
    csrc = os.path.join(sf.ROOT, "libmems_amd", "csrc")
    capi = open(os.path.join(csrc, "mums_capi.hip")).read()
    replay = open(os.path.join(csrc, "replay.hip")).read()
    cap = int(re.search(r"kReplayLdsIds\s*=\s*(\d+)", capi).group(1))
    carried = replay[replay.index("hipError_t launch_replay_carried("):]
    small = int(re.search(r"constexpr uint32_t kSmall\s*=\s*(\d+);", carried).group(1))
    assert "constexpr int replay_block() { return MG <= 4 ? 1024 : (MG <= 8 ? 512 : 256); }" in replay
    assert re.search(r"if \(G <= 4\) return find_replay<4>.*\n\s*if \(G <= 8\) return find_replay<8>.*\n"
                     r"\s*if \(G <= 16\) return find_replay<16>.*\n\s*if \(G <= 32\) return find_replay<32>.*\n"
                     r"\s*return find_replay<64>", capi)
    return cap, small, lambda G: 1024 if G <= 4 else (512 if G <= 8 else 256)


def test_cases_reach_the_carried_replays_paths(model, results):
    """Every path replay_carried_kernel and launch_replay_carried choose among is reached by a
    case, and by the case that exists for it (PATHS).  Conditions on the inputs, from the model
    and the oracle's probes alone."""
    cap, small, lanes = replay_constants()
    assert (cap, small) == (8192, 64)
    hit = carried_paths(results, sf.CASES, cap, small, lanes)
    for what, names in PATHS.items():
        for name in (names if isinstance(names, tuple) else (names,)):
            assert name in hit.get(what, set()), f"{what}: not reached by {name} (reached by {sorted(hit.get(what, ()))})"
    # round 1 of k12 makes one AddHashEntry call and it inserts
    k12 = results["k12_one_probe"]
    assert k12[1]["probes"] == 1 and len(k12[1]["log"][0]) == 1 and len(k12[1]["lengths"]) == len(k12[0]["lengths"]) + 1
    # a round without probes (test_gpu_seed_family.py::test_round_without_probes_keeps_the_table)
    seqs, seed, kw = sf.rounds_of(sf.FIRST)[0]
    none = sf.run_model(model, [(seqs, seed, kw), ([b"A" * 60, b"C" * 60], seed, kw)])[1]
    assert none["probes"] == 0 and len(none["lengths"]) == len(results[sf.FIRST][0]["lengths"]) > 0
    # k1: the bucket is in LDS when round 1 starts and in global memory when round 2 starts
    k1 = results["k1_spill_mid_replay"]
    assert len(k1[0]["lengths"]) <= cap < len(k1[1]["lengths"])
    assert "k1_spill_mid_replay" in hit["vector starts in global memory"]
