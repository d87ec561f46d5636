"""The inputs of tests/test_gpu_chain_paths.py (tests/chain_path_cases.py) on the CPU: every
case is what the GPU tests rely on, asserted from the oracle's output alone, so that an edit of
a generator cannot hollow them out.  Each figure is a floor under what the reference gives (the
evolved runs: 1.2k-6.8k lines, >= 1100 collisions, 5.1k-18.1k probes, >= 1400 reverse matches
under the palindromic seeds and 0-3 under the non-palindromic w19 rank 2; the stretch cases: 10 / 28 / 50 / 94 / 193 matches through a whole copy of X, 2 of them with
every genome) -- a condition, not a measurement."""
import numpy as np
import pytest

from tests import chain_path_cases as cp
from tests import rearranged_inputs as ri


def test_case_list():
    """Every genome-count class above 4 (two G per class where the class has room), four seeds
    per evolved shape."""
    assert sorted({cp.genome_class(G) for G, _ in cp.EVOLVED_SHAPES}) == [8, 16, 32, 64]
    assert sorted({cp.genome_class(G) for G in cp.STRETCH_G}) == [8, 16, 32, 64]
    assert len(cp.EVOLVED) == 32 and len(cp.STRETCH) == 5 and len(cp.STRETCH_XMUT) == 2
    assert [cp.genome_class(G) for G in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]


def test_seed_walk_forms(oracle_mod):
    """seed_is_lean mirrors chains.hip's seed_bitpar_odd: the odd-weight palindromic patterns
    (w13 ranks 0 and 1, w15) take the lean walks, the even-weight w12 and a non-palindromic
    pattern (w19 rank 2) the generic hit words."""
    def lean(w, rank):
        seed = oracle_mod.get_seed(w, rank)
        return cp.seed_is_lean(seed, oracle_mod.lib().oracle_seed_length(seed))
    assert lean(13, 0) and lean(15, 0) and lean(13, 1)
    assert not lean(12, 0) and not lean(19, 2)
    assert not cp.seed_is_lean(0b1101, 4) and cp.seed_is_lean(0b10101, 5) and not cp.seed_is_lean(0b1001, 4)


@pytest.mark.parametrize("name", cp.EVOLVED)
def test_evolved_preconditions(oracle_mod, name):
    seqs, seed, lengths, starts, st = cp.oracle_result(oracle_mod, name)
    assert len(seqs) == cp.CASES[name][1]["G"]
    lines = ri.count_lines(lengths, starts)
    neg = int((starts < 0).any(axis=1).sum())
    print(f"{name}: {len(lengths)} matches, {lines} lines, {neg} with a reverse component, "
          f"{st['collision_count']} collisions, {st['probes']} probes")
    assert lines >= 1000
    L = oracle_mod.lib().oracle_seed_length(seed)
    bits = [(seed >> k) & 1 for k in range(L)]
    if bits == bits[::-1]:
        assert neg >= 500
    else:
        # A non-palindromic pattern keys a reverse window by the mirrored pattern: a reverse
        # homology shares no seed with the forward strand and the few reverse
        # components are chance coincidences of two windows.  What the case is for is the walk
        # form: generic with no switch set, through hit_word's column-by-column branch.
        assert not cp.seed_is_lean(seed, L)
        assert neg * 100 <= len(lengths)
    assert st["collision_count"] >= 1000
    assert st["probes"] >= 4000
    assert st["probes"] // 4 >= 1000   # the sliced variants' slice size: four or five real slices


@pytest.mark.parametrize("name", cp.STRETCH + cp.STRETCH_XMUT)
def test_stretch_preconditions(oracle_mod, name):
    seqs, seed, lengths, starts, st = cp.oracle_result(oracle_mod, name)
    opts = cp.CASES[name][1]
    assert len(seqs) == opts["G"]
    assert ri.TIER_COLUMNS == 512 + 16 * 16 * 64 == 16_896 < opts["xlen"]
    found = ri.stretches_of(oracle_mod, seqs, seed, lengths, starts, ri.TIER_COLUMNS, cp.TABLE_SIZE)
    long_runs = [f for f in found if f[1] >= ri.TIER_COLUMNS]
    all_genomes = [f for f in long_runs if (starts[f[0]] != 0).all()]
    print(f"{name}: {len(lengths)} matches, {len(long_runs)} with a probe-free run >= {ri.TIER_COLUMNS} columns, "
          f"{len(all_genomes)} of them with every genome; {st['probes']} probes")
    assert len(long_runs) >= 10
    assert len(all_genomes) >= 2
    # each such run lies between probes of its match or between a probe and the match's end: a
    # walk of that many columns, whichever side it starts from
    assert all(left + right > 0 for _, _, left, right in long_runs)
    assert st["probes"] // 4 >= 1000
