"""mums_find_batch / MemHash.FindMatchesBatch: B independent FindMatches in one device pass.
Problem p of a batch must be what the oracle's MemHash::FindMatches returns for p's sequences
alone with the same seed, table size and mask: lengths, starts, AddHashEntry calls, collisions
and MER_REPEAT_LIMIT restarts."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")
BATCH_CAP = 200000   # seed-mers of one problem the batched pass takes (include/mums.h)


def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    hit = rng.random(len(a)) < rate
    a[hit] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(hit.sum()))
    return a.tobytes()


def rc(seq):
    return seq.translate(COMP)[::-1]


def pair(rng, n, rate=0.1, flip=False):
    a = rand_seq(rng, n)
    b = mutate(rng, a, rate)
    return (a, rc(b) if flip else b)


def check_batch(gpu_lib, oracle_mod, problems, seeds, table_size=40000, mask=None, mh=None):
    """Run the batch and compare every problem with the oracle; returns the lists and the oracle stats."""
    own = mh is None
    if own:
        mh = gpu_lib.MaskedMemHash(0) if mask is not None else gpu_lib.MemHash(0)
    try:
        mh.SetTableSize(table_size)
        if mask is not None:
            mh.SetMask(mask)
        if isinstance(seeds, int):
            seeds = [seeds] * len(problems)
        refs = [None if seeds[p] == 0 else
                oracle_mod.find_matches(list(prob), seeds[p], table_size=table_size, masked=mask is not None,
                                        seq_mask=mask or 0) for p, prob in enumerate(problems)]
        # the library runs the largest problems of a batch alone when that is faster;
        # MUMS_DEV_BATCH_NO_SPLIT keeps every problem up to the cap in the batched pass: both ways
        for no_split in ("1", None):
            if no_split:
                os.environ["MUMS_DEV_BATCH_NO_SPLIT"] = no_split
            else:
                os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)
            lists = mh.FindMatchesBatch(problems, seeds)
            info = mh.BatchInfo()
            assert len(lists) == len(problems)
            for p in range(len(problems)):
                if refs[p] is None:
                    assert len(lists[p]) == 0
                    continue
                rl, rs, st = refs[p]
                assert np.array_equal(lists[p].lengths, rl), f"problem {p}: lengths"
                assert np.array_equal(lists[p].starts, rs), f"problem {p}: starts"
                assert int(info["probes"][p]) == st["probes"], f"problem {p}: probes"
                assert int(info["collisions"][p]) == st["collision_count"], f"problem {p}: collisions"
                assert int(info["restarts"][p]) == st["restarts"], f"problem {p}: restarts"
                assert int(info["matches"][p]) == len(rl)
        return lists, [r[2] if r else None for r in refs]
    finally:
        os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)
        if own:
            mh.close()


@pytest.mark.parametrize("table_size", [40000, 7, 1])
def test_batch_of_one_equals_single_find(gpu_lib, oracle_mod, table_size):
    rng = np.random.default_rng(101)
    prob = pair(rng, 2000)
    seed = oracle_mod.get_seed(7)
    lists, _ = check_batch(gpu_lib, oracle_mod, [prob], seed, table_size)
    assert len(lists[0]) > 10
    with gpu_lib.MemHash(0) as mh:
        mh.SetTableSize(table_size)
        mh.SetSeed(seed)
        ml = mh.FindMatches(list(prob))
    assert np.array_equal(ml.lengths, lists[0].lengths) and np.array_equal(ml.starts, lists[0].starts)


def test_identical_problems_give_identical_local_lists(gpu_lib, oracle_mod):
    rng = np.random.default_rng(102)
    prob = pair(rng, 1500, flip=True)
    lists, _ = check_batch(gpu_lib, oracle_mod, [prob, prob, prob], oracle_mod.get_seed(7))
    assert len(lists[0]) > 5
    for ml in lists[1:]:
        assert np.array_equal(ml.lengths, lists[0].lengths) and np.array_equal(ml.starts, lists[0].starts)


def test_bait_across_problems(gpu_lib, oracle_mod):
    """Problem 0's first sequence equals problem 1's second; the true partners are unrelated."""
    rng = np.random.default_rng(103)
    x = rand_seq(rng, 1200)
    problems = [(x, rand_seq(rng, 1200)), (rand_seq(rng, 1100), x), pair(rng, 900)]
    check_batch(gpu_lib, oracle_mod, problems, oracle_mod.get_seed(7))


@pytest.mark.parametrize("flip", [False, True])
def test_match_ending_at_a_junction(gpu_lib, oracle_mod, flip):
    """Matches run to the last base of both sequences and the bytes after each sequence continue
    the same bases: a walk or a window crossing the junction would lengthen them."""
    rng = np.random.default_rng(104)
    r = rand_seq(rng, 900)
    s0, s1 = r[0:300], r[300:400] + r[0:300]
    t0 = r[300:700]
    t1 = mutate(rng, t0, 0.03)
    if flip:
        problems = [(s0, rc(s1)), (rc(t0), t1), (s0, rc(s0))]
    else:
        problems = [(s0, s1), (t0, t1), (s0, s0)]
    lists, _ = check_batch(gpu_lib, oracle_mod, problems, oracle_mod.get_seed(7))
    assert int(lists[0].lengths.max()) == 300
    if flip:
        assert (lists[0].starts[:, 1] < 0).any()


def test_degenerate_segments(gpu_lib, oracle_mod):
    rng = np.random.default_rng(105)
    seed = oracle_mod.get_seed(9)
    good = [pair(rng, 700), pair(rng, 900, flip=True)]
    problems = [(b"", rand_seq(rng, 500)), good[0], (b"", b""), (b"ACGTAC", b"ACGTAC"), good[1],
                (rand_seq(rng, 400), b""), (b"", b"")]
    lists, _ = check_batch(gpu_lib, oracle_mod, problems, seed)
    assert [len(ml) == 0 for ml in lists] == [True, False, True, True, False, True, True]
    with gpu_lib.MemHash(0) as mh:
        mh.SetSeed(seed)
        mh.FindMatchesBatch(problems, [seed] * len(problems))
        mo = np.zeros(len(problems) + 1, dtype=np.uint64)
        mh._check(mh._lib.mums_batch_info(mh._ctx, mo.ctypes.data, None, None, None))
    assert mo[0] == mo[1] == 0 and mo[2] == mo[3] == mo[4] and mo[5] == mo[6] == mo[7]
    assert mo[2] == len(lists[1]) and mo[7] == len(lists[1]) + len(lists[4])


def partial_problem(rng, G, n):
    """G sequences sharing parts of one ancestor: subset matches with NO_MATCH columns."""
    anc = rand_seq(rng, n)
    out = []
    for g in range(G):
        lo = int(rng.integers(0, n // 3))
        hi = int(rng.integers(2 * n // 3, n))
        s = mutate(rng, anc[lo:hi], 0.03)
        out.append(rc(s) if g % 3 == 2 else s)
    return tuple(out)


@pytest.mark.parametrize("G,table_size,mask", [(3, 40000, None), (4, 40000, None), (4, 7, None), (3, 40000, 0b101),
                                               (9, 40000, None)])
def test_more_than_two_sequences(gpu_lib, oracle_mod, G, table_size, mask):
    rng = np.random.default_rng(106 + G)
    problems = [partial_problem(rng, G, 1200), partial_problem(rng, G, 700), partial_problem(rng, G, 1500)]
    lists, _ = check_batch(gpu_lib, oracle_mod, problems, oracle_mod.get_seed(7), table_size, mask)
    total = sum(len(ml) for ml in lists)
    assert total > 0
    if mask is None:
        assert any((ml.starts == 0).any() for ml in lists), "no subset match in the case"


@pytest.mark.parametrize("w,rank", [(7, 1), (7, 2), (11, 1), (8, 0)])
def test_seed_ranks_and_even_weight(gpu_lib, oracle_mod, w, rank):
    rng = np.random.default_rng(107)
    problems = [pair(rng, 1800), pair(rng, 1300, flip=True), pair(rng, 600)]
    lists, _ = check_batch(gpu_lib, oracle_mod, problems, oracle_mod.get_seed(w, rank))
    assert sum(len(ml) for ml in lists) > 0


def test_mer_repeat_limit_problems(gpu_lib, oracle_mod):
    """A poly-A run of 1500 and an N run of 1200 in both sequences: the merge restarts
    (MatchFinder.cpp:253-277) in exactly those problems."""
    rng = np.random.default_rng(108)
    a, b = pair(rng, 800)
    c, d = pair(rng, 900)
    problems = [pair(rng, 1000), (a[:400] + b"A" * 1500 + a[400:], b[:300] + b"A" * 1500 + b[300:]), pair(rng, 500),
                (c[:200] + b"N" * 1200 + c[200:], d[:500] + b"N" * 1200 + d[500:]), pair(rng, 1200, flip=True)]
    _, refs = check_batch(gpu_lib, oracle_mod, problems, oracle_mod.get_seed(9))
    assert [st["restarts"] for st in refs] == [0, 1, 0, 1, 0]
    assert refs[1]["max_group"] > 1000 and refs[3]["max_group"] > 1000


def test_problem_size_cap(gpu_lib, oracle_mod):
    """Problems just under, at and over the seed-mer count above which a problem runs through the
    single-problem pipeline, among small ones."""
    rng = np.random.default_rng(109)
    seed = oracle_mod.get_seed(11)
    L = gpu_lib.getSeedLength(seed)
    base = rand_seq(rng, 100_100)
    mut = mutate(rng, base, 0.05)
    problems = [pair(rng, 800)]
    for extra in (-1, 0, 1):
        n0 = BATCH_CAP // 2 + (L - 1)
        n1 = BATCH_CAP - (n0 - L + 1) + (L - 1) + extra
        problems.append((base[:n0], mut[:n1]))
        assert (n0 - L + 1) + (n1 - L + 1) == BATCH_CAP + extra
    problems.append(pair(rng, 600, flip=True))
    check_batch(gpu_lib, oracle_mod, problems, seed)


def test_many_problems_default_seeds(gpu_lib, oracle_mod):
    """300 gap-sized problems, lengths uniform in [0, 3000], half the partners reverse-complemented,
    default seeds through the mirror's grouping: every problem against the oracle, the whole
    against a loop of single finds on one context."""
    rng = np.random.default_rng(110)
    problems = []
    for p in range(300):
        n = int(rng.integers(0, 3001))
        a, b = pair(rng, n, 0.04, flip=bool(p & 1))
        cut = int(rng.integers(0, n // 8 + 1))
        problems.append((a, b[cut:]))
    patterns, groups = gpu_lib.batch_seed_groups(problems)
    weights = {gpu_lib.getSeedWeight(s) for s in patterns}
    assert {0, 5, 7, 9} <= weights
    lists, _ = check_batch(gpu_lib, oracle_mod, problems, patterns)
    with gpu_lib.MemHash(0) as mh:
        default = mh.FindMatchesBatch(problems)
        for p, prob in enumerate(problems):
            assert np.array_equal(default[p].lengths, lists[p].lengths)
            assert np.array_equal(default[p].starts, lists[p].starts)
            if patterns[p] == 0:
                continue
            mh.Clear()
            mh.SetSeed(patterns[p])
            ml = mh.FindMatches(list(prob))
            assert np.array_equal(ml.lengths, lists[p].lengths), p
            assert np.array_equal(ml.starts, lists[p].starts), p


def _appendix_c_find(gpu_lib, oracle_mod, mh):
    """An ordinary FindMatches on the same object still returns its known answer."""
    seqs = oracle_mod.generate(3, 200_000, 0.03, 12345)
    mh.Clear()
    mh.SetSeed(oracle_mod.get_seed(15))
    ml = mh.FindMatches(seqs)
    assert len(ml) == 365


def test_refused_modes(gpu_lib, oracle_mod):
    rng = np.random.default_rng(111)
    problems = [pair(rng, 800), pair(rng, 600)]
    seed = oracle_mod.get_seed(7)

    def refused(mh):
        with pytest.raises(gpu_lib.MumsError) as e:
            mh.FindMatchesBatch(problems, [seed] * 2)
        assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED, e.value

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
        _appendix_c_find(gpu_lib, oracle_mod, mh)
        check_batch(gpu_lib, oracle_mod, problems, seed, mh=mh)
    with gpu_lib.PairwiseMatchFinder(0) as mh:
        refused(mh)
    with gpu_lib.ParallelMemHash(0) as mh:
        refused(mh)
    with gpu_lib.MemHash(0) as mh:   # a sharded context
        mh.AddSequence(problems[0][0])
        lens = np.array([800, 800], dtype=np.uint64)
        mh._check(mh._lib.mums_shard_layout(mh._ctx, 2, 0, lens.ctypes.data))
        refused(mh)
    with gpu_lib.MemHash(0) as mh:   # bad arguments
        mh.SetSeed(seed)
        off = np.zeros(3, dtype=np.uint64)
        assert mh._lib.mums_find_batch(mh._ctx, 2, 1, b"", off.ctypes.data) == gpu_lib.MUMS_E_INVALID
        assert mh._lib.mums_find_batch(mh._ctx, 0, 2, None, None) == gpu_lib.MUMS_OK
        assert len(mh.GetMatchList()) == 0
        mh.SetSeed(0)
        off = np.zeros(5, dtype=np.uint64)
        assert mh._lib.mums_find_batch(mh._ctx, 2, 2, b"", off.ctypes.data) == gpu_lib.MUMS_E_INVALID


def test_refused_calls_on_a_batch_result(gpu_lib, oracle_mod):
    rng = np.random.default_rng(112)
    problems = [pair(rng, 800), pair(rng, 600)]
    seed = oracle_mod.get_seed(7)
    with gpu_lib.MemHash(0) as mh:
        lists = mh.FindMatchesBatch(problems, [seed] * 2)
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
        assert len(before) == len(lists[0]) + len(lists[1])
        st = mh.stats()
        info = mh.BatchInfo()
        assert st["mem_count"] == len(before) and st["probes"] == int(info["probes"].sum())
        assert st["collision_count"] == int(info["collisions"].sum())
        _appendix_c_find(gpu_lib, oracle_mod, mh)
        mh.LengthFilter(20)   # an ordinary result again


def test_gap_names_the_problem(gpu_lib, oracle_mod):
    rng = np.random.default_rng(113)
    problems = [pair(rng, 500) for _ in range(5)]
    seed = oracle_mod.get_seed(7)
    bad = list(problems)
    a, b = bad[3]
    bad[3] = (a, b[:100] + b"-" + b[100:])
    bad[4] = (bad[4][0][:50] + b"-", bad[4][1])
    with gpu_lib.MemHash(0) as mh:
        with pytest.raises(gpu_lib.GapInSequence) as e:
            mh.FindMatchesBatch(bad, [seed] * 5)
        assert "problem 3" in str(e.value)
        check_batch(gpu_lib, oracle_mod, problems, seed, mh=mh)


def _mixed_routings(rng):
    """A lane problem, one above the MUMS_DEV_BATCH_CAP the test sets, and test_mer_repeat_limit_problems'
    poly-A problem, which a lane gives up (below that cap: 4600 seed-mers)."""
    a, b = pair(rng, 800)
    return [pair(rng, 1000), pair(rng, 3500), (a[:400] + b"A" * 1500 + a[400:], b[:300] + b"A" * 1500 + b[300:])]


@pytest.mark.parametrize("batch", ["g3", "mixed"])
def test_find_batch_and_one_round_anchor_batch_agree(gpu_lib, oracle_mod, batch):
    """mums_find_batch and mums_anchor_batch share one host engine: with one round and min_length 0
    the anchor call's table is the find call's list.  Per problem and in mums_get_stats the two agree,
    every find list is the oracle's, and the anchor call's final lists are mums_anchor_tail_batch of
    the find lists: one MemHash, both routings of the size rule."""
    import anchor_batch_cases as ab
    if batch == "g3":
        case = ab.find_case("g3")
        problems, seed, cap = case["problems"], case["patterns"][0][0], None
    else:
        problems, seed, cap = _mixed_routings(np.random.default_rng(114)), oracle_mod.get_seed(9), "6000"
    B = len(problems)
    refs = [oracle_mod.find_matches(list(prob), seed, table_size=40000) for prob in problems]
    if batch == "mixed":
        assert [r[2]["restarts"] for r in refs] == [0, 0, 1]
    one_round = dict(problems=problems, patterns=[(seed,)] * B)
    totals = ("seedmers", "probes", "collision_count", "restarts", "sort_passes", "key_bytes")
    with gpu_lib.MemHash(0) as mh:
        mh.SetTableSize(40000)
        try:
            if cap:
                os.environ["MUMS_DEV_BATCH_CAP"] = cap
            for no_split in ("1", None):
                if no_split:
                    os.environ["MUMS_DEV_BATCH_NO_SPLIT"] = no_split
                else:
                    os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)
                found = mh.FindMatchesBatch(problems, [seed] * B)
                f_info, f_st = mh.BatchInfo(), mh.stats()
                anchored, a_info = ab.run_find_case(mh, one_round, False, min_length=0)
                a_st = mh.stats()
                tails = mh.AnchorTailBatch(found, eliminate_both=False, min_length=0)
                for p, (rl, rs, st) in enumerate(refs):
                    assert np.array_equal(found[p].lengths, rl) and np.array_equal(found[p].starts, rs), p
                    assert int(f_info["probes"][p]) == int(a_info["probes"][p]) == st["probes"], p
                    assert int(f_info["collisions"][p]) == int(a_info["collisions"][p]) == st["collision_count"], p
                    assert int(f_info["restarts"][p]) == int(a_info["restarts"][p]) == st["restarts"], p
                    assert int(f_info["matches"][p]) == int(a_info["table_entries"][p]) == len(rl), p
                    assert np.array_equal(anchored[p].lengths, tails[p].lengths), p
                    assert np.array_equal(anchored[p].starts, tails[p].starts), p
                for k in totals:
                    assert f_st[k] == a_st[k], (k, f_st[k], a_st[k])
                assert f_st["probes"] == sum(r[2]["probes"] for r in refs) and f_st["key_bytes"] == 8
        finally:
            os.environ.pop("MUMS_DEV_BATCH_CAP", None)
            os.environ.pop("MUMS_DEV_BATCH_NO_SPLIT", None)
