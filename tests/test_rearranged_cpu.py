"""The rearranged corpus (tests/rearranged_inputs.py) on the CPU.

1. Preconditions: every case is what tests/test_gpu_rearranged.py relies on -- hundreds of
   distinct lines, reverse components, every multiplicity (evolved cases); matches whose probes
   leave a probe-free stretch longer than the first two walk tiers cover (long-stretch cases).
   Each is computed from the oracle's result and is a condition, not a tolerance.
2. Properties of a correct MatchList checked from the sequences alone, with none of the
   oracle's logic beyond oracle_seed_length and the seed's bit pattern: bounds, soundness of
   the first and last seed window, and for solid seeds exactness and maximality.  The same
   checker runs over the three committed Appendix-C MatchLists of tests/golden/.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from tests import rearranged_inputs as ri

_COMP = np.zeros(256, dtype=np.uint8)
for _x, _y in zip(b"ACGT", b"TGCA"):
    _COMP[_x] = _y


# ---- the property checker (numpy; sequences, MatchList and seed pattern only) -----------------
def care_positions(seed: int, L: int):
    """Care positions of the pattern (bit L-1-k of the seed = position k) and of its mirror
    image, which is what a reverse component is sampled with: the reverse complement of the w
    sampled bases reads the strand-corrected window at the mirrored positions (equal to the
    care positions for a palindromic pattern)."""
    care = np.array([k for k in range(L) if (seed >> (L - 1 - k)) & 1], dtype=np.int64)
    return care, np.sort(L - 1 - care)


def component(seq: np.ndarray, start: int, off: int, ln: int) -> np.ndarray:
    """Columns [off, off + ln) of a component's strand-corrected string: forward
    seq[s-1 : s-1+len], reverse the reverse complement of seq[|s|-1 : |s|-1+len]; `start` and
    the match length give where column 0 is."""
    s, mlen = start
    if s > 0:
        return seq[s - 1 + off:s - 1 + off + ln]
    lo = -s - 1 + mlen - off - ln
    return _COMP[seq[lo:lo + ln][::-1]]


def check_matchlist(seqs, lengths, starts, seed, L, solid=False, maximal=False):
    """Violations of bounds / soundness (/ exactness / maximality) as a dict of match index
    lists, and the number of matches with a component ending at a sequence end."""
    arr = [np.frombuffer(s, dtype=np.uint8) for s in seqs]
    n = np.array([len(s) for s in seqs], dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    care, mirror = care_positions(seed, L)
    bad = {"bounds": [], "short": [], "sound": [], "exact": [], "maximal": []}
    at_end = 0
    defined = starts != 0
    ok = (~defined) | ((np.abs(starts) - 1 + lengths[:, None]) <= n[None, :])
    for i in range(len(lengths)):
        ln = int(lengths[i])
        gs = np.nonzero(defined[i])[0]
        if not ok[i].all() or len(gs) < 2:
            bad["bounds"].append(i)
            continue
        if ln < L:
            bad["short"].append(i)
            continue
        comps = [(arr[g], (int(starts[i, g]), ln)) for g in gs]
        pats = [care if st[0] > 0 else mirror for _, st in comps]
        for off in (0, ln - L):
            ref = component(*comps[0], off, L)[pats[0]]
            if any((component(*c, off, L)[p] != ref).any() for c, p in zip(comps[1:], pats[1:])):
                bad["sound"].append(i)
                break
        if solid:
            ref = component(*comps[0], 0, ln)
            if any((component(*c, 0, ln) != ref).any() for c in comps[1:]):
                bad["exact"].append(i)
        if maximal:
            ended = False
            for side in (-1, +1):
                cols = []
                for g, (sq, (s, _)) in zip(gs, comps):
                    # the forward-coordinate position of the column next to the match on this side
                    fwd = (s - 1 + (ln if side > 0 else -1)) if s > 0 else (-s - 1 + (-1 if side > 0 else ln))
                    if fwd < 0 or fwd >= n[g]:
                        cols = None
                        break
                    cols.append(int(sq[fwd]) if s > 0 else int(_COMP[sq[fwd]]))
                if cols is None:
                    ended = True
                elif len(set(cols)) == 1:
                    bad["maximal"].append(i)
            at_end += ended
    return bad, at_end


def _seed_of(oracle_mod, opts):
    seed = oracle_mod.get_seed(opts["w"], opts.get("rank", 0))
    return seed, oracle_mod.lib().oracle_seed_length(seed)


def _is_solid(seed, L):
    return seed == (1 << L) - 1


# ---- preconditions ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ri.EVOLVED)
def test_evolved_preconditions(oracle_mod, name):
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, st = ri.oracle_result(oracle_mod, name)
    G = len(seqs)
    lines = ri.count_lines(lengths, starts)
    neg = int((starts < 0).any(axis=1).sum())
    mult = (starts != 0).sum(axis=1)
    sets = {tuple(np.nonzero(r)[0].tolist()) for r in starts}
    print(f"{name}: {len(lengths)} matches, {lines} lines, {neg} with a negative start, "
          f"multiplicities {sorted(set(mult.tolist()))}, {len(sets)} genome sets, {st['probes']} probes")
    assert lines >= 300
    _, L = _seed_of(oracle_mod, opts)
    care, mirror = care_positions(seed, L)
    if (care == mirror).all():
        assert neg >= 100
    else:
        # A non-palindromic pattern keys a reverse window by the mirrored pattern, so a true
        # reverse-complement homology shares no seed with the forward strand: the reference
        # finds no reverse component there, whatever the seed or the counts;
        # the inverted blocks and the reverse-complemented genome are decoys that must stay
        # unmatched (blocks inverted inside the reversed genome match forward).
        assert neg == 0
    if opts.get("cls") == "PairwiseMatchFinder":
        assert set(mult.tolist()) == {2} and len(sets) >= 3
    elif opts.get("cls") == "MaskedMemHash":
        # (the mask admits one genome set only: the multiplicity floor cannot apply)
        assert len(sets) == 1 and set(mult.tolist()) == {bin(opts["seq_mask"]).count("1")}
    elif G == 9:
        assert len(set(mult.tolist())) >= 4
    else:
        assert set(mult.tolist()) == set(range(2, G + 1))


@pytest.mark.parametrize("name", ri.STRETCH)
def test_long_stretch_preconditions(oracle_mod, name):
    _, opts = ri.CASES[name]
    xlen = opts["xlen"]
    found = ri.stretches(oracle_mod, name)
    print(f"{name}: matches >= xlen and their probe-free stretches (index, columns, probes left, right): {found}")
    assert len(found) >= 2
    # beyond the short tier and the 16-lane tier's steps: 512 + 16 * 16 * 64 = 16 896 columns
    assert ri.TIER_COLUMNS == 512 + 16 * 16 * 64 == 16_896
    assert xlen - ri.STRETCH_SLACK > ri.TIER_COLUMNS
    for _, gap, left, right in found:
        assert gap >= xlen - ri.STRETCH_SLACK
    if opts["bridge"]:
        assert any(left > 0 and right > 0 for _, _, left, right in found)
    else:   # one-sided walks: the probes of U1 walk right, those of U2 walk left
        assert any(left > 0 and right == 0 for _, _, left, right in found)
        assert any(left == 0 and right > 0 for _, _, left, right in found)


# ---- properties -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ri.CASES))
def test_matchlist_properties(oracle_mod, name):
    _, opts = ri.CASES[name]
    seqs, seed, lengths, starts, _ = ri.oracle_result(oracle_mod, name)
    _, L = _seed_of(oracle_mod, opts)
    solid = _is_solid(seed, L)
    bad, at_end = check_matchlist(seqs, lengths, starts, seed, L, solid=solid,
                                  maximal=solid and ri.is_default_memhash(opts))
    print(f"{name}: {len(lengths)} matches, violations { {k: len(v) for k, v in bad.items()} }, "
          f"{at_end} ending at a sequence end")
    assert len(lengths) > 0
    assert all(len(v) == 0 for v in bad.values()), {k: v[:5] for k, v in bad.items() if v}


def test_checker_sees_a_broken_list(oracle_mod):
    """The checker is not vacuous: a shifted start, a shortened solid match and a start past
    the sequence end are each reported."""
    name = "ev_G3_w25"
    seqs, seed, lengths, starts, _ = ri.oracle_result(oracle_mod, name)
    L = oracle_mod.lib().oracle_seed_length(seed)
    i = int(np.argmax((starts > 0).all(axis=1) & (lengths > L + 2)))
    s = starts.copy()
    s[i, 1] += 1
    assert i in check_matchlist(seqs, lengths, s, seed, L, solid=True)[0]["exact"]
    ln = lengths.copy()
    ln[i] -= 1
    assert i in check_matchlist(seqs, ln, starts, seed, L, solid=True, maximal=True)[0]["maximal"]
    s = starts.copy()
    s[i, 0] = len(seqs[0])
    assert i in check_matchlist(seqs, lengths, s, seed, L)[0]["bounds"]
    seqs2, seed2, l2, s2, _ = ri.oracle_result(oracle_mod, "ev_G3_w15")
    L2 = oracle_mod.lib().oracle_seed_length(seed2)
    sh = s2.copy()
    j = int(np.argmax((s2[:, 0] > 0) & (s2[:, 1] > 1)))
    sh[j, 1] -= 1
    assert j in check_matchlist(seqs2, l2, sh, seed2, L2)[0]["sound"]


GOLDEN_LISTS = [("c1_related", 2, 1_000_000, 0.01, 15), ("c1_iid", 2, 1_000_000, 1.0, 15),
                ("g3_200k_p003", 3, 200_000, 0.03, 15)]   # (tests/golden/make_golden.py SMALL)


@pytest.mark.parametrize("name,G,n,p,w", GOLDEN_LISTS, ids=[g[0] for g in GOLDEN_LISTS])
def test_golden_matchlists_have_the_properties(oracle_mod, name, G, n, p, w):
    """The committed Appendix-C MatchList texts under the same checker."""
    rows = np.loadtxt(os.path.join(GOLDEN, name + ".txt"), dtype=np.int64, ndmin=2)
    assert rows.shape[1] == G + 1 and len(rows) > 0
    seqs = oracle_mod.generate(G, n, p, 12345)
    seed = oracle_mod.get_seed(w)
    L = oracle_mod.lib().oracle_seed_length(seed)
    bad, _ = check_matchlist(seqs, rows[:, 0], rows[:, 1:], seed, L)
    assert all(len(v) == 0 for v in bad.values()), {k: v[:5] for k, v in bad.items() if v}


# ---- what the GPU tests' other inputs rely on -------------------------------------------------
def test_batch_problems_have_matches(oracle_mod):
    """The 40 small problems of test_gpu_rearranged.py::test_batch_and_family: the default seed
    exists for each, most hold several matches, some a reverse one."""
    import libmems_amd
    problems = ri.batch_problems()
    assert len(problems) == 40 and all(500 <= len(p[0]) <= 3000 for p in problems)
    patterns, groups = libmems_amd.batch_seed_groups(
        problems, default_weight=oracle_mod.lib().oracle_default_seed_weight, get_seed=oracle_mod.get_seed)
    assert all(patterns) and len(groups) >= 2
    counts, neg = [], 0
    for prob, pat in zip(problems, patterns):
        lengths, starts, _ = oracle_mod.find_matches(list(prob), pat)
        counts.append(len(lengths))
        neg += int((starts < 0).any(axis=1).sum())
    assert sum(c >= 3 for c in counts) >= 30 and neg >= 10, (counts, neg)


def test_family_rounds_insert(oracle_mod):
    """The seed family of the GPU test on the model of tests/seed_family_cases.py: round 0 is
    the oracle's find, the later ranks insert further entries into the kept table."""
    import seed_family_cases as sf
    if not sf.have_compiler():
        pytest.skip("no gcc: the seed family model cannot be built")
    rounds = ri.family_rounds(oracle_mod)
    model = sf.run_model(sf.load_model(), rounds)
    _, _, lengths, starts, st = ri.oracle_result(oracle_mod, ri.FAMILY_CASE)
    assert np.array_equal(model[0]["lengths"], lengths) and np.array_equal(model[0]["starts"], starts)
    assert model[0]["collisions"] == st["collision_count"]
    for r in (1, 2):
        assert len(model[r]["log"][0]) > 0 and len(model[r]["lengths"]) > len(model[r - 1]["lengths"])


def test_overlap_case_really_overlaps(oracle_mod):
    """EliminateOverlaps has work on the w11 MatchList (v2: where g++ is, on the live model)."""
    import shutil
    import test_eliminate_overlaps_v2_cpu as eo2
    _, _, lengths, starts, _ = ri.oracle_result(oracle_mod, ri.OVERLAP_CASE)
    ol, os_ = oracle_mod.eliminate_overlaps(lengths, starts)
    assert len(ol) < len(lengths) or not np.array_equal(os_, starts)
    if not shutil.which("g++"):
        pytest.skip("no g++: EliminateOverlaps_v2's model cannot be built (v1 checked)")
    model = eo2.load_model()
    for both in (False, True):
        ml, ms, cnt = eo2.model_eo2(model, lengths, starts, None, both)
        assert cnt["pairs"] > 0 and cnt["kept"] == 0
        assert cnt["del_i"] + cnt["del_j"] + cnt["crop_i"] + cnt["crop_j"] > 0
        assert len(ml) < len(lengths) or not np.array_equal(ms, starts)


def test_pairwise_log_follows_sequence_id_order(oracle_mod):
    """PairwiseMatchFinder sorts a seed group by sequence id before it hashes the pairs
    (PairwiseMatchFinder.cpp:39), so the match log lists the entries by the first call, in
    (group by key, first sequence, second sequence) order, that falls inside each.  The groups
    are rebuilt here from the per-position seed keys alone.  (The oracle once kept the merge's
    arrival order inside a group; the HIP path disagreed with it on every rearranged input.)"""
    seqs = ri.evolved(4, 6000, 31, inversions=2, translocations=1, duplications=1, tandems=1, indels=20)
    G = len(seqs)
    seed = oracle_mod.get_seed(15)
    L = oracle_mod.lib().oracle_seed_length(seed)
    _, _, st = oracle_mod.find_matches(seqs, seed, pairwise=True)
    log_len, log_s = st["match_log"]
    assert len(log_len) > 20 and (log_s < 0).any()
    keys = [oracle_mod.seed_keys(s, seed) for s in seqs]
    key = np.concatenate(keys)
    gid = np.concatenate([np.full(len(k), g) for g, k in enumerate(keys)])
    pos = np.concatenate([np.arange(len(k)) for k in keys])
    order = np.lexsort((pos, gid, key >> np.uint64(1)))   # (bit 0: the strand of the canonical key)
    mk, gid, pos, par = (key >> np.uint64(1))[order], gid[order], pos[order], (key & np.uint64(1))[order]
    entries = {}
    for i, (ln, row) in enumerate(zip(log_len.tolist(), log_s.tolist())):
        a, b = [g for g in range(G) if row[g] != 0]
        entries.setdefault((a, b), []).append((i, row[a], row[b], ln))
    heads = np.nonzero(np.concatenate([[True], mk[1:] != mk[:-1], [True]]))[0]
    seen = []
    for s, e in zip(heads[:-1], heads[1:]):
        count = np.bincount(gid[s:e], minlength=G)
        uniq = [k for k in range(s, e) if count[gid[k]] == 1]
        for x in range(len(uniq)):
            for y in range(x + 1, len(uniq)):
                a, b = int(gid[uniq[x]]), int(gid[uniq[y]])
                sa, sb = int(pos[uniq[x]]) + 1, int(pos[uniq[y]]) + 1
                if par[uniq[x]] != par[uniq[y]]:
                    sb = -sb
                for i, ea, eb, ln in entries.get((a, b), []):
                    d = sa - ea   # the call lies inside entry i: same diagonal, inside its columns
                    inside = 0 <= d <= ln - L and ((eb > 0 and sb - eb == d) or (eb < 0 and sb < 0 and eb - sb == ln - L - d))
                    if inside and i not in seen:
                        seen.append(i)
    assert seen == list(range(len(log_len)))
