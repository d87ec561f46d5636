"""mums_anchor_batch / mums_anchor_tail_batch on the device: the whole body of
ProgressiveAligner::pairwiseAnchorSearch for B problems in one call.  Every problem's final list
and counters against the fixture golden/anchor_batch_cases.json (which decides) and, where a
compiler is present, against the live CPU models' arrays (which locate a difference), under both
routings of the size rule (MUMS_DEV_BATCH_NO_SPLIT=1 and unset)."""
import os

import numpy as np
import pytest

import anchor_batch_cases as ab

pytestmark = pytest.mark.gpu

ROUTINGS = ("1", None)


class routing:
    def __init__(self, no_split):
        self.no_split = no_split

    def __enter__(self):
        if self.no_split:
            os.environ["MUMS_DEV_BATCH_NO_SPLIT"] = self.no_split
        else:
            os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)

    def __exit__(self, *a):
        os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)


def open_hash(gpu_lib, case):
    mh = gpu_lib.MaskedMemHash(0) if case["mask"] is not None else gpu_lib.MemHash(0)
    mh.SetTableSize(case["table_size"])
    if case["mask"] is not None:
        mh.SetMask(case["mask"])
    return mh


def compare(lists, info, recorded, live, variant, what):
    """recorded: the fixture's digests per problem; live: the models' results per problem or None."""
    assert len(lists) == len(recorded)
    for p, (ml, d) in enumerate(zip(lists, recorded)):
        if live is not None:
            el, es = live[p]["final"][variant]
            assert np.array_equal(ml.lengths, el), f"{what}, problem {p}: lengths"
            assert np.array_equal(np.asarray(ml.starts).reshape(-1), np.asarray(es).reshape(-1)), f"{what}, problem {p}: starts"
        assert len(ml) == d["count"] and ab.sf.list_md5(ml.lengths, ml.starts) == d["list_md5"], f"{what}, problem {p}"
        assert int(info["matches"][p]) == d["count"]
        for k in ("table_entries", "probes", "collisions", "restarts"):
            if k in d:
                assert int(info[k][p]) == d[k], f"{what}, problem {p}: {k}"


@pytest.mark.parametrize("name", list(ab.FIND_CASES))
def test_find_cases(gpu_lib, name):
    case = ab.find_case(name)
    recorded = ab.fixture()["find"][name]
    live = ab.model_case(name) if ab.have_compiler() else None
    with open_hash(gpu_lib, case) as mh:
        for no_split in ROUTINGS:
            for variant in case["variants"]:
                with routing(no_split):
                    lists, info = ab.run_find_case(mh, case, ab.VARIANTS[variant])
                compare(lists, info, recorded[variant], live, variant, f"{name} {variant} no_split={no_split}")


def test_a200_through_the_mirror(gpu_lib):
    """AnchorSearchBatch groups by default weight and makes one call per weight; the sums in
    mums_get_stats and mums_batch_info answer for the last group."""
    case = ab.find_case("a200")
    recorded = ab.fixture()["find"]["a200"]
    with gpu_lib.MemHash(0) as mh:
        for variant, eb in ab.VARIANTS.items():
            lists = mh.AnchorSearchBatch(case["problems"], eliminate_both=eb)
            compare(lists, mh.AnchorBatchInfo(), recorded[variant], None, variant, f"mirror {variant}")
        ws, groups, _ = gpu_lib.anchor_seed_groups(case["problems"])
        last = list(groups.values())[-1]
        info, st = mh.AnchorBatchInfo(), mh.stats()
        assert st["mem_count"] == int(info["table_entries"][last].sum()) and st["probes"] == int(info["probes"][last].sum())
        assert st["collision_count"] == int(info["collisions"][last].sum())
        assert st["ms_total"] >= st["ms_replay"] > 0 and st["ms_output"] > 0
        mo, pr = np.zeros(len(last) + 1, dtype=np.uint64), np.zeros(len(last), dtype=np.uint64)
        mh._check(mh._lib.mums_batch_info(mh._ctx, mo.ctypes.data, pr.ctypes.data, None, None))
        assert np.array_equal(np.diff(mo), info["matches"][last]) and np.array_equal(pr, info["probes"][last])
        rank0 = mh.AnchorSearchBatch(case["problems"][:20], seed_families=False)
        one = ab.run_find_case(mh, dict(case, problems=case["problems"][:20], patterns=[p[:1] for p in case["patterns"][:20]]),
                               False)[0]
        for a, b in zip(rank0, one):
            assert np.array_equal(a.lengths, b.lengths) and np.array_equal(a.starts, b.starts)


@pytest.mark.parametrize("no_split", ROUTINGS)
def test_full_pool_in_round_1(gpu_lib, no_split):
    case = ab.pool_case()
    per_class = ab.fixture()["pool"]
    recorded = [per_class[p % ab.POOL_CLASSES] for p in range(len(case["problems"]))]
    with gpu_lib.MemHash(0) as mh:
        with routing(no_split):
            lists, info = ab.run_find_case(mh, case, False)
        compare(lists, info, recorded, None, "eb0", "pool")
        assert int(info["table_entries"].sum()) == len(case["problems"])


@pytest.mark.parametrize("name", ["random_g2", "random_g3", "random_g8", "random_wide_g3", "adversarial", "tail_cap"])
def test_tail_only_lists(gpu_lib, name):
    lists_in = ab.tail_cases()[name]
    recorded = ab.fixture()["tail"][name]
    mls = [gpu_lib.MatchList(l, s) for l, s in lists_in]
    with gpu_lib.MemHash(0) as mh:
        for variant, eb in ab.VARIANTS.items():
            out = mh.AnchorTailBatch(mls, eb, ab.MIN_LENGTH)
            info = mh.AnchorBatchInfo()
            live = None
            if ab.have_compiler():
                live = [dict(final={variant: ab.model_tail(l, s, eb)}) for l, s in lists_in]
            compare(out, info, recorded[variant], live, variant, f"{name} {variant}")
            assert info["table_entries"].tolist() == [len(l) for l, _ in lists_in]
            assert not info["probes"].any() and not info["collisions"].any() and not info["restarts"].any()
            if ab.have_compiler():   # min_length 0 keeps everything v2 leaves
                out0 = mh.AnchorTailBatch(mls, eb, 0)
                for p, (l, s) in enumerate(lists_in):
                    el, es = ab.model_tail(l, s, eb, 0)
                    assert np.array_equal(out0[p].lengths, el) and np.array_equal(out0[p].starts, es), (name, variant, p)


def loop_of_existing_calls(mh, problem, patterns, eliminate_both, min_length):
    mh.Clear()
    for pat in patterns:
        mh.ClearSequences()
        mh.SetSeed(pat)
        mh.FindMatches(list(problem))
    mh.EliminateOverlaps_v2(None, eliminate_both)
    mh.LengthFilter(min_length)
    return mh.GetMatchList()


@pytest.mark.parametrize("table_size", [40000, 7])
def test_batch_of_one_equals_the_loop_of_existing_calls(gpu_lib, table_size):
    case = ab.find_case("a200")
    p = max(range(200), key=lambda q: len(case["problems"][q][0]))
    prob, pats = case["problems"][p], case["patterns"][p]
    one = dict(problems=[prob], patterns=[pats], table_size=table_size, mask=None)
    with open_hash(gpu_lib, one) as mh, open_hash(gpu_lib, one) as ref:
        for eb in (False, True):
            want = loop_of_existing_calls(ref, prob, pats, eb, ab.MIN_LENGTH)
            assert len(want) > 0
            for no_split in ROUTINGS:
                with routing(no_split):
                    (got,), _ = ab.run_find_case(mh, one, eb)
                assert np.array_equal(got.lengths, want.lengths) and np.array_equal(got.starts, want.starts)


def test_one_round_without_filter_is_the_tail_of_find_batch(gpu_lib):
    case = ab.find_case("g3")
    seed = case["patterns"][0][0]
    one = dict(case, patterns=[(seed,)] * len(case["problems"]))
    with gpu_lib.MemHash(0) as mh:
        for eb in (False, True):
            lists, info = ab.run_find_case(mh, one, eb, 0)
            found = mh.FindMatchesBatch(case["problems"], [seed] * len(case["problems"]))
            assert info["table_entries"].tolist() == [len(ml) for ml in found]
            tails = mh.AnchorTailBatch(found, eb, 0)
            assert sum(len(ml) for ml in tails) > 0
            for a, b in zip(lists, tails):
                assert np.array_equal(a.lengths, b.lengths) and np.array_equal(a.starts, b.starts)


def test_identical_problems_give_identical_lists(gpu_lib):
    case = ab.find_case("ranks_r012")
    prob = case["problems"][1]
    same = dict(case, problems=[prob] * 3, patterns=case["patterns"][:3])
    with gpu_lib.MemHash(0) as mh:
        lists, info = ab.run_find_case(mh, same, False)
    assert len(lists[0]) > 0
    for ml in lists[1:]:
        assert np.array_equal(ml.lengths, lists[0].lengths) and np.array_equal(ml.starts, lists[0].starts)
    assert len(set(info["probes"].tolist())) == 1


def test_gap_names_the_problem(gpu_lib):
    case = ab.find_case("ranks_r012")
    bad = list(case["problems"])
    a, b = bad[2]
    bad[2] = (a, b[:100] + b"-" + b[100:])
    bad[3] = (bad[3][0][:50] + b"-", bad[3][1])
    with gpu_lib.MemHash(0) as mh:
        with pytest.raises(gpu_lib.GapInSequence) as e:
            ab.run_find_case(mh, dict(case, problems=bad), False)
        assert "problem 2" in str(e.value)
        assert mh._lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_E_INVALID
        lists, info = ab.run_find_case(mh, case, False)
        compare(lists, info, ab.fixture()["find"]["ranks_r012"]["eb0"], None, "eb0", "after the gap")


def _appendix_c_find(gpu_lib, oracle_mod, mh):
    """An ordinary FindMatches on the same object still returns its known answer."""
    seqs = oracle_mod.generate(3, 200_000, 0.03, 12345)
    mh.Clear()
    mh.SetSeed(oracle_mod.get_seed(15))
    assert len(mh.FindMatches(seqs)) == 365


def _find_batch_known(gpu_lib, oracle_mod, mh, case):
    seed = case["patterns"][0][0]
    lists = mh.FindMatchesBatch(case["problems"], [seed] * len(case["problems"]))
    for ml, prob in zip(lists, case["problems"]):
        rl, rs, _ = oracle_mod.find_matches(list(prob), seed)
        assert np.array_equal(ml.lengths, rl) and np.array_equal(ml.starts, rs)


def test_refused_modes_and_bad_arguments(gpu_lib, oracle_mod):
    case = ab.find_case("ranks_r012")

    def refused(mh, code=None):
        with pytest.raises(gpu_lib.MumsError) as e:
            ab.run_find_case(mh, case, False)
        assert e.value.code == (code or gpu_lib.MUMS_E_UNSUPPORTED), e.value

    with gpu_lib.MemHash(0) as mh:
        mh.SetRepeatTolerance(1)
        refused(mh)
        mh.SetRepeatTolerance(0)
        mh.SetEnumerationTolerance(2)
        refused(mh)
        mh.SetEnumerationTolerance(1)
        sp = np.array([3, 4], dtype=np.uint64)
        mh._check(mh._lib.mums_set_start_points(mh._ctx, sp.ctypes.data, 2))
        refused(mh)
        mh._check(mh._lib.mums_set_start_points(mh._ctx, None, 0))
        mh.SetMatchLog(True)
        refused(mh)
        mh.SetMatchLog(False)
        mh.LogProgress(True)
        refused(mh)
        mh.LogProgress(False)
        _appendix_c_find(gpu_lib, oracle_mod, mh)   # the refusals left the context as it was
        lists, info = ab.run_find_case(mh, case, False)
        compare(lists, info, ab.fixture()["find"]["ranks_r012"]["eb0"], None, "eb0", "after the refusals")
    with gpu_lib.PairwiseMatchFinder(0) as mh:
        refused(mh)
    with gpu_lib.ParallelMemHash(0) as mh:
        refused(mh)
    with gpu_lib.MemHash(0) as mh:   # a sharded context
        mh.AddSequence(case["problems"][0][0])
        lens = np.array([len(case["problems"][0][0])] * 2, dtype=np.uint64)
        mh._check(mh._lib.mums_shard_layout(mh._ctx, 2, 0, lens.ctypes.data))
        refused(mh)
    with gpu_lib.MemHash(0) as mh:   # bad arguments
        lib, INV = mh._lib, gpu_lib.MUMS_E_INVALID
        off = np.zeros(5, dtype=np.uint64)
        pats = np.asarray(case["patterns"][0], dtype=np.uint64)
        zero = np.array([pats[0], 0, pats[2]], dtype=np.uint64)
        nine = np.repeat(pats[:1], 9)
        assert lib.mums_anchor_batch(mh._ctx, 2, 1, b"", off.ctypes.data, pats.ctypes.data, 3, 0, 12) == INV
        assert lib.mums_anchor_batch(mh._ctx, 2, 2, b"", off.ctypes.data, pats.ctypes.data, 0, 0, 12) == INV
        assert lib.mums_anchor_batch(mh._ctx, 2, 2, b"", off.ctypes.data, nine.ctypes.data, 9, 0, 12) == INV
        assert lib.mums_anchor_batch(mh._ctx, 2, 2, b"", off.ctypes.data, zero.ctypes.data, 3, 0, 12) == INV
        assert lib.mums_anchor_batch(mh._ctx, 2, 2, b"", off.ctypes.data, None, 3, 0, 12) == INV
        assert lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == INV   # no such result yet
        mh.SetSeed(0x7AC9AF)
        assert lib.mums_anchor_batch(mh._ctx, 0, 2, None, None, pats.ctypes.data, 3, 0, 12) == gpu_lib.MUMS_OK
        assert len(mh.GetMatchList()) == 0
        assert lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_OK
        assert lib.mums_anchor_tail_batch(mh._ctx, 0, 2, None, None, None, 0, 12) == gpu_lib.MUMS_OK
        down = np.array([0, 5, 3], dtype=np.uint64)
        assert lib.mums_anchor_tail_batch(mh._ctx, 2, 2, down.ctypes.data, None, None, 0, 12) == INV
        # the context's own seed pattern is neither read nor changed: the next find uses it
        ab.run_find_case(mh, case, False)
        mh.Clear()
        ml = mh.FindMatches(list(case["problems"][0]))
        rl, rs, _ = oracle_mod.find_matches(list(case["problems"][0]), 0x7AC9AF)
        assert np.array_equal(ml.lengths, rl) and np.array_equal(ml.starts, rs)


def test_refused_calls_on_an_anchor_result(gpu_lib, oracle_mod):
    case = ab.find_case("ranks_r012")
    with gpu_lib.MemHash(0) as mh:
        for make in (lambda: ab.run_find_case(mh, case, False)[0],
                     lambda: mh.AnchorTailBatch([gpu_lib.MatchList(l, s) for l, s in ab.tail_cases()["random_wide_g3"]])):
            lists = make()
            before = mh.GetMatchList()
            calls = [lambda: mh.MultiplicityFilter(2), lambda: mh.LengthFilter(20), mh.EliminateOverlaps,
                     mh.EliminateOverlaps_v2, mh.ClearSequences, mh.MemTableCount, mh.Probes,
                     lambda: mh.SeedKeys(0, 10), lambda: mh.SeedKeysRange(0, 0, 10), lambda: mh.SortedMerList(0, 10),
                     lambda: mh.SeedOccurrence(0, 10)]
            for call in calls:
                with pytest.raises(gpu_lib.MumsError) as e:
                    call()
                assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED, e.value
            after = mh.GetMatchList()
            assert np.array_equal(before.lengths, after.lengths) and np.array_equal(before.starts, after.starts)
            assert len(before) == sum(len(ml) for ml in lists) > 0
            _appendix_c_find(gpu_lib, oracle_mod, mh)
            mh.LengthFilter(20)   # an ordinary result again
            assert mh._lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_E_INVALID
            _find_batch_known(gpu_lib, oracle_mod, mh, case)
            assert mh._lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_E_INVALID
