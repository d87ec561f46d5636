"""mums_recursion_batch / mums_recursion_tail_batch on the device: the gap search of
Aligner::Recursion for B problems in one call.  Every problem's final list and counters against the
fixture golden/recursion_batch_cases.json (which decides) and, where a compiler is present, against
the live CPU models' arrays (which locate a difference), under both routings of the size rule
(MUMS_DEV_BATCH_NO_SPLIT=1 and unset)."""
import os

import numpy as np
import pytest

import recursion_batch_cases as rb

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


def same(a, b):
    return np.array_equal(a.lengths, b.lengths) and np.array_equal(np.asarray(a.starts).reshape(-1), np.asarray(b.starts).reshape(-1))


def compare(lists, info, recorded, live, variant, what):
    """recorded: the fixture's digests per problem; live: the models' results per problem or None."""
    assert len(lists) == len(recorded)
    for p, (ml, d) in enumerate(zip(lists, recorded)):
        if live is not None:
            el, es = live[p]["final"][variant]
            assert np.array_equal(ml.lengths, el), f"{what}, problem {p}: lengths"
            assert np.array_equal(np.asarray(ml.starts).reshape(-1), np.asarray(es).reshape(-1)), f"{what}, problem {p}: starts"
        assert len(ml) == d["count"] and rb.sf.list_md5(ml.lengths, ml.starts) == d["list_md5"], f"{what}, problem {p}"
        if info is None:
            continue
        assert int(info["matches"][p]) == d["count"]
        for k in ("table_entries", "probes", "collisions", "restarts"):
            if k in d:
                assert int(info[k][p]) == d[k], f"{what}, problem {p}: {k}"


def find_case_params():
    """(case, routing, variants of one test): R200's variants run as tests of their own."""
    for name in rb.FIND_CASES:
        variants = rb.find_case(name)["variants"]
        for no_split in ROUTINGS:
            for vs in ([(v,) for v in variants] if name == "r200" else [variants]):
                yield pytest.param(name, no_split, vs, id=f"{name}-{no_split}-{'+'.join(vs)}")


@pytest.mark.parametrize("name,no_split,variants", list(find_case_params()))
def test_find_cases(gpu_lib, name, no_split, variants):
    case = rb.find_case(name)
    recorded = rb.fixture()["find"][name]
    live = rb.model_case(name) if rb.have_compiler() else None
    with open_hash(gpu_lib, case) as mh:
        for variant in variants:
            with routing(no_split):
                lists, info = rb.run_find_case(mh, case, rb.VARIANTS[variant])
            compare(lists, info, recorded[variant], live, variant, f"{name} {variant} no_split={no_split}")
    if name == "restart":
        assert int(info["restarts"][1]) > 0 and len(lists[1]) > 0


def test_r200_through_the_mirror(gpu_lib):
    """RecursionBatch derives every problem's rounds from its sequence lengths (or the given
    weights), groups by pattern tuple and makes one call per group; explicit weights reproduce the
    fixture's rounds."""
    case = rb.find_case("r200")
    G_of = [len(p) for p in case["problems"]]
    recorded = rb.fixture()["find"]["r200"]
    weights_of = {rb.patterns_of(ws): ws for ws in rb.R200_ROUNDS}
    with gpu_lib.MemHash(0) as mh:
        for G in rb.R200_GS:
            idx = [p for p in range(200) if G_of[p] == G]
            probs = [case["problems"][p] for p in idx]
            # weights that give exactly the case's rounds: the first round's weight on the sequences
            # to spare (two at least: a round needs two sequences), then one sequence per later round
            ws = []
            for p in idx:
                rw = list(weights_of[case["patterns"][p]])
                ws.append([rw[0]] * (G - len(rw) + 1) + rw[1:] if G > len(rw) or len(rw) == 1 else None)
            keep = [i for i, w in enumerate(ws) if w is not None and gpu_lib.recursion_rounds([0] * G, False, w) ==
                    list(weights_of[case["patterns"][idx[i]]])]
            assert len(keep) >= len(idx) // 3
            lists = mh.RecursionBatch([probs[i] for i in keep], nway_only=False, weights=[ws[i] for i in keep])
            info = mh.RecursionBatchInfo()
            compare(lists, info, [recorded["m0"][idx[i]] for i in keep], None, "m0", f"mirror G={G}")
            # the default weights: whatever rounds they give, the result is the C call's with those rounds
            got = mh.RecursionBatch(probs[:6], nway_only=True)
            pats, _ = gpu_lib.recursion_groups(probs[:6], True)
            want, _ = rb.run_find_case(mh, dict(case, problems=probs[:6], patterns=pats), G)
            assert all(same(a, b) for a, b in zip(got, want))
        assert mh.stats()["ms_total"] > 0
        assert mh._lib.mums_batch_info(mh._ctx, None, None, None, None) == gpu_lib.MUMS_OK


@pytest.mark.parametrize("name", list(rb.tail_cases()))
def test_tail_only_lists(gpu_lib, name):
    lists_in = rb.tail_cases()[name]
    recorded = rb.fixture()["tail"][name]
    mls = [gpu_lib.MatchList(l, s) for l, s in lists_in]
    G = lists_in[0][1].shape[1]
    with gpu_lib.MemHash(0) as mh:
        for variant in rb.VARIANTS:
            for ml in rb.TAIL_MIN_LENGTHS:
                mult = rb.VARIANTS[variant](G)
                out = mh.RecursionTailBatch(mls, mult, ml)
                info = mh.RecursionBatchInfo()
                live = None
                if rb.have_compiler():
                    live = [dict(final={variant: rb.model_tail(l, s, mult, ml)}) for l, s in lists_in]
                compare(out, info, recorded[rb.tail_key(variant, ml)], live, variant, f"{name} {variant} min_length={ml}")
                assert info["table_entries"].tolist() == [len(l) for l, _ in lists_in]
                assert not info["probes"].any() and not info["collisions"].any() and not info["restarts"].any()


def test_overflow_list_among_others_gives_the_same_rows(gpu_lib):
    """The list that outgrows its slice is flagged and runs alone; its neighbours in the same call
    are untouched by it (nothing is written past a slice)."""
    t = rb.tail_cases()
    over = t["overflow"][0]
    g8 = [x for x in t["random_g8"]]
    lists_in = g8[:5] + [over] + g8[5:]
    fx = rb.fixture()["tail"]
    key = rb.tail_key("m0", rb.MIN_LENGTH)
    recorded = fx["random_g8"][key][:5] + fx["overflow"][key] + fx["random_g8"][key][5:]
    with gpu_lib.MemHash(0) as mh:
        out = mh.RecursionTailBatch([gpu_lib.MatchList(l, s) for l, s in lists_in], 0, rb.MIN_LENGTH)
        compare(out, mh.RecursionBatchInfo(), recorded, None, "m0", "overflow among others")


def loop_of_existing_calls(mh, problem, patterns, multiplicity, min_length):
    mh.Clear()
    for pat in patterns:
        mh.ClearSequences()
        mh.SetSeed(pat)
        mh.FindMatches(list(problem))
    mh.EliminateOverlaps()
    if multiplicity:
        mh.MultiplicityFilter(multiplicity)
    mh.LengthFilter(min_length)
    return mh.GetMatchList()


def test_batch_equals_the_loop_of_existing_calls(gpu_lib):
    """20 problems of R200 (5 of every G): the batch and the single-problem calls on the same context."""
    case = rb.find_case("r200")
    with gpu_lib.MemHash(0) as mh:
        for G in rb.R200_GS:
            idx = [p for p in range(200) if len(case["problems"][p]) == G][3:8]
            sub = dict(case, problems=[case["problems"][p] for p in idx], patterns=[case["patterns"][p] for p in idx])
            for mult in (0, G):
                got, _ = rb.run_find_case(mh, sub, mult)
                for k, p in enumerate(idx):
                    want = loop_of_existing_calls(mh, case["problems"][p], case["patterns"][p], mult, rb.MIN_LENGTH)
                    assert same(got[k], want), (G, mult, p)
                assert sum(len(ml) for ml in got) > 0


def test_changing_batch_shapes_on_one_context(gpu_lib):
    fx = rb.fixture()["find"]
    with gpu_lib.MemHash(0) as mh:
        for name in ("g9", "ranks_w9_7", "degenerate", "g9", "restart", "ranks_w9"):
            case = rb.find_case(name)
            lists, info = rb.run_find_case(mh, case, 0)
            compare(lists, info, fx[name]["m0"], None, "m0", f"shapes: {name}")
        t = rb.tail_cases()["random_g3"]
        out = mh.RecursionTailBatch([gpu_lib.MatchList(l, s) for l, s in t], 0, rb.MIN_LENGTH)
        compare(out, None, rb.fixture()["tail"]["random_g3"][rb.tail_key("m0", rb.MIN_LENGTH)], None, "m0", "shapes: tail")
        lists, info = rb.run_find_case(mh, rb.find_case("g9"), 9)
        compare(lists, info, fx["g9"]["mG"], None, "mG", "shapes: g9 again")


def test_gap_names_the_problem(gpu_lib):
    case = rb.find_case("ranks_w9_7")
    bad = list(case["problems"])
    a, b, c = bad[1]
    bad[1] = (a, b[:100] + b"-" + b[100:], c)
    with gpu_lib.MemHash(0) as mh:
        with pytest.raises(gpu_lib.GapInSequence) as e:
            rb.run_find_case(mh, dict(case, problems=bad), 0)
        assert "problem 1" in str(e.value)
        assert mh._lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_E_INVALID
        lists, info = rb.run_find_case(mh, case, 0)
        compare(lists, info, rb.fixture()["find"]["ranks_w9_7"]["m0"], None, "m0", "after the gap")


def test_refused_modes_and_bad_arguments(gpu_lib):
    case = rb.find_case("ranks_w9_7")

    def refused(mh):
        with pytest.raises(gpu_lib.MumsError) as e:
            rb.run_find_case(mh, case, 0)
        assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED, e.value

    with gpu_lib.MemHash(0) as mh:
        mh.SetRepeatTolerance(1)
        refused(mh)
        mh.SetRepeatTolerance(0)
        mh.SetEnumerationTolerance(2)
        refused(mh)
        mh.SetEnumerationTolerance(1)
        mh.SetMatchLog(True)
        refused(mh)
        mh.SetMatchLog(False)
        lists, info = rb.run_find_case(mh, case, 0)
        compare(lists, info, rb.fixture()["find"]["ranks_w9_7"]["m0"], None, "m0", "after the refusals")
    with gpu_lib.PairwiseMatchFinder(0) as mh:
        refused(mh)
    with gpu_lib.ParallelMemHash(0) as mh:
        refused(mh)
    with gpu_lib.MemHash(0) as mh:
        lib, INV = mh._lib, gpu_lib.MUMS_E_INVALID
        off = np.zeros(7, dtype=np.uint64)
        pats = np.asarray(case["patterns"][0], dtype=np.uint64)
        zero = np.array([pats[0], 0], dtype=np.uint64)
        nine = np.repeat(pats[:1], 9)
        assert lib.mums_recursion_batch(mh._ctx, 2, 1, b"", off.ctypes.data, pats.ctypes.data, 2, 0, 9) == INV
        assert lib.mums_recursion_batch(mh._ctx, 2, 3, b"", off.ctypes.data, pats.ctypes.data, 0, 0, 9) == INV
        assert lib.mums_recursion_batch(mh._ctx, 2, 3, b"", off.ctypes.data, nine.ctypes.data, 9, 0, 9) == INV
        assert lib.mums_recursion_batch(mh._ctx, 2, 3, b"", off.ctypes.data, zero.ctypes.data, 2, 0, 9) == INV
        assert lib.mums_recursion_batch(mh._ctx, 2, 3, b"", off.ctypes.data, None, 2, 0, 9) == INV
        assert lib.mums_recursion_batch(mh._ctx, 2, 65, b"", off.ctypes.data, pats.ctypes.data, 2, 0, 9) == gpu_lib.MUMS_E_UNSUPPORTED
        assert lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == INV   # no such result yet
        assert lib.mums_recursion_batch(mh._ctx, 0, 3, None, None, pats.ctypes.data, 2, 0, 9) == gpu_lib.MUMS_OK
        assert len(mh.GetMatchList()) == 0
        assert lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_OK
        assert lib.mums_recursion_tail_batch(mh._ctx, 0, 3, None, None, None, 0, 9) == gpu_lib.MUMS_OK
        down = np.array([0, 5, 3], dtype=np.uint64)
        assert lib.mums_recursion_tail_batch(mh._ctx, 2, 3, down.ctypes.data, None, None, 0, 9) == INV
        assert lib.mums_recursion_tail_batch(mh._ctx, 2, 0, off.ctypes.data, None, None, 0, 9) == INV


def test_refused_calls_and_info_on_a_recursion_result(gpu_lib, oracle_mod):
    case = rb.find_case("ranks_w9_7")
    B = len(case["problems"])
    with gpu_lib.MemHash(0) as mh:
        for make in (lambda: rb.run_find_case(mh, case, 0)[0],
                     lambda: mh.RecursionTailBatch([gpu_lib.MatchList(l, s) for l, s in rb.tail_cases()["random_wide_g3"]])):
            lists = make()
            before = mh.GetMatchList()
            n = len(lists)
            a_off, b_off = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
            a_pr, b_pr = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            mh._check(mh._lib.mums_batch_info(mh._ctx, a_off.ctypes.data, a_pr.ctypes.data, None, None))
            mh._check(mh._lib.mums_anchor_batch_info(mh._ctx, b_off.ctypes.data, None, b_pr.ctypes.data, None, None))
            assert np.array_equal(a_off, b_off) and np.array_equal(a_pr, b_pr)
            assert np.diff(a_off).tolist() == [len(ml) for ml in lists]
            calls = [lambda: mh.MultiplicityFilter(2), lambda: mh.LengthFilter(20), mh.EliminateOverlaps,
                     mh.EliminateOverlaps_v2, mh.ClearSequences, mh.MemTableCount, mh.Probes,
                     lambda: mh.SeedKeys(0, 10), lambda: mh.SortedMerList(0, 10), lambda: mh.SeedOccurrence(0, 10)]
            for call in calls:
                with pytest.raises(gpu_lib.MumsError) as e:
                    call()
                assert e.value.code == gpu_lib.MUMS_E_UNSUPPORTED, e.value
            after = mh.GetMatchList()
            assert same(before, after) and len(before) == sum(len(ml) for ml in lists) > 0
            # an ordinary find ends the state
            seqs = list(case["problems"][0])
            mh.Clear()
            mh.SetSeed(case["patterns"][0][0])
            ml = mh.FindMatches(seqs)
            rl, rs, _ = oracle_mod.find_matches(seqs, case["patterns"][0][0])
            assert np.array_equal(ml.lengths, rl) and np.array_equal(ml.starts, rs)
            mh.LengthFilter(20)
            assert mh._lib.mums_anchor_batch_info(mh._ctx, None, None, None, None, None) == gpu_lib.MUMS_E_INVALID
    assert B == 3
