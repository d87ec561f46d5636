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
    if sf.CASES[name].get("mode", {}).get("pairwise"):
        # the model hashes a seed group's pairs in the reference's order (sorted by sequence id,
        # PairwiseMatchFinder.cpp:39), the oracle in the merge's run order: the same inserts, the
        # calls of one group (at most G (G - 1) / 2, consecutive) permuted
        assert sf.log_set_md5(r0["log"]) == sf.log_set_md5((log_len, log_s))
        a = np.column_stack([r0["log"][0].astype(np.int64), r0["log"][1]]).tolist()
        b = np.column_stack([log_len.astype(np.int64), log_s]).tolist()
        reach = sf.CASES[name]["G"] * (sf.CASES[name]["G"] - 1) // 2 - 1
        assert all(row in b[max(0, i - reach):i + reach + 1] for i, row in enumerate(a))
        assert a != b   # (else the special case is dead)
    else:
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
