"""EliminateOverlaps_v2 (ProgressiveAligner.h:300-406) on the GPU against the recorded results
of the literal C++ model (tests/golden/eo_v2_cases.json, pinned to the live model by
tests/test_eliminate_overlaps_v2_cpu.py) and, where g++ is present, against the live model's
arrays; the device-resident chain FindMatches -> EliminateOverlaps_v2 -> LengthFilter of
progressiveMauve's pairwiseAnchorSearch (ProgressiveAligner.cpp:646-659); the edges of the C ABI."""
import json
import shutil

import numpy as np
import pytest

import test_eliminate_overlaps_v2_cpu as cpu
from test_eliminate_overlaps_cpu import random_matchlist

pytestmark = pytest.mark.gpu

RUNS = cpu.fixture_runs()


@pytest.fixture(scope="module")
def recorded():
    with open(cpu.FIXTURE) as f:
        return json.load(f)["runs"]


@pytest.fixture(scope="module")
def live_model():
    return cpu.load_model() if shutil.which("g++") else None


@pytest.fixture(scope="module")
def inputs():
    return cpu.all_inputs()


def check(got, recorded_run, live_model, lengths, starts, ids, both):
    if live_model is not None:   # locates a difference; the fixture decides
        ml, ms, _ = cpu.model_eo2(live_model, lengths, starts, ids, both)
        assert len(got) == len(ml)
        assert np.array_equal(got.lengths, ml) and np.array_equal(got.starts, ms)
    assert {"count": len(got), "md5": cpu.digest(got.lengths, got.starts)} == recorded_run


@pytest.mark.parametrize("key,case,ids,both", RUNS, ids=[r[0] for r in RUNS])
def test_eliminate_overlaps_v2_random(gpu_lib, recorded, live_model, inputs, key, case, ids, both):
    lengths, starts = inputs[case]
    got = gpu_lib.EliminateOverlaps_v2(gpu_lib.MatchList(lengths, starts), ids, both)
    check(got, recorded[key], live_model, lengths, starts, ids, both)


@pytest.mark.parametrize("G", cpu.CHAIN_GS)
def test_device_resident_chain(gpu_lib, oracle_mod, recorded, live_model, G):
    seqs = cpu.repeat_rich(G)
    ref_l, ref_s, _ = oracle_mod.find_matches(seqs, oracle_mod.get_seed(11))
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(oracle_mod.get_seed(11))
        for both in (False, True):
            ml = mh.FindMatches(None if both else seqs)   # the second find reuses the sequences
            assert np.array_equal(ml.lengths, ref_l) and np.array_equal(ml.starts, ref_s)
            mh.EliminateOverlaps_v2(eliminate_both=both)   # on the device-resident MatchList
            mh.LengthFilter(cpu.CHAIN_MIN_LENGTH)
            got = mh.GetMatchList()                        # the one copy of the final list
            if live_model is not None:
                el, es, _ = cpu.model_eo2(live_model, ref_l, ref_s, None, both)
                keep = el >= cpu.CHAIN_MIN_LENGTH
                assert np.array_equal(got.lengths, el[keep]) and np.array_equal(got.starts, es[keep])
            assert {"count": len(got), "md5": cpu.digest(got.lengths, got.starts)} == \
                recorded[f"chain_G{G}_both{int(both)}_min{cpu.CHAIN_MIN_LENGTH}"]


@pytest.mark.parametrize("M", [0, 1])
@pytest.mark.parametrize("both", [False, True])
def test_degenerate_lists_are_unchanged(gpu_lib, M, both):
    lengths, starts = random_matchlist(np.random.default_rng(5), M, 3, start_span=100)
    got = gpu_lib.EliminateOverlaps_v2(gpu_lib.MatchList(lengths, starts), None, both)
    assert np.array_equal(got.lengths, lengths) and np.array_equal(got.starts, starts.reshape(M, 3))
    got = gpu_lib.EliminateOverlaps_v2(gpu_lib.MatchList(lengths, starts), [2, 0], both)
    assert np.array_equal(got.lengths, lengths) and np.array_equal(got.starts, starts.reshape(M, 3))


def test_bad_sequence_id_is_invalid(gpu_lib, inputs):
    lengths, starts = inputs[(200, 3, 2000, 3)]
    with gpu_lib.MemHash(0) as mh:
        mh.LoadMatches(gpu_lib.MatchList(lengths, starts))
        for ids in ([3], [0, 1, 7], [2 ** 32 - 1]):
            with pytest.raises(gpu_lib.MumsError) as e:
                mh.EliminateOverlaps_v2(ids)
            assert e.value.code == gpu_lib.MUMS_E_INVALID
        got = mh.GetMatchList()   # the refused calls changed nothing
    assert np.array_equal(got.lengths, lengths) and np.array_equal(got.starts, starts)


def test_empty_id_list_does_nothing(gpu_lib, inputs):
    lengths, starts = inputs[(200, 3, 2000, 3)]
    got = gpu_lib.EliminateOverlaps_v2(gpu_lib.MatchList(lengths, starts), [], True)
    assert np.array_equal(got.lengths, lengths) and np.array_equal(got.starts, starts)


def test_v1_unaffected_after_v2(gpu_lib, oracle_mod, recorded, inputs):
    # one context: v2, then v1 on a reloaded list (shared work arrays), then v2 on a wider list
    case = (3000, 4, 30000, 4)
    lengths, starts = inputs[case]
    wide = (5000, 8, 20000, 5)
    with gpu_lib.MemHash(0) as mh:
        mh.LoadMatches(gpu_lib.MatchList(lengths, starts))
        mh.EliminateOverlaps_v2(eliminate_both=True)
        v2 = mh.GetMatchList()
        mh.LoadMatches(gpu_lib.MatchList(lengths, starts))
        mh.EliminateOverlaps()
        v1 = mh.GetMatchList()
        mh.LoadMatches(gpu_lib.MatchList(*inputs[wide]))
        mh.EliminateOverlaps_v2()
        v2_wide = mh.GetMatchList()
    assert {"count": len(v2), "md5": cpu.digest(v2.lengths, v2.starts)} == recorded[cpu.case_key(*case, True)]
    rl, rs = oracle_mod.eliminate_overlaps(lengths, starts)
    assert np.array_equal(v1.lengths, rl) and np.array_equal(v1.starts, rs)
    assert {"count": len(v2_wide), "md5": cpu.digest(v2_wide.lengths, v2_wide.starts)} == \
        recorded[cpu.case_key(*wide, False)]
