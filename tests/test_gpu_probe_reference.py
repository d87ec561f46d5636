"""GPU: the reference genome of a seed probe (the smallest genome present in the group, whose
strand fixes the probe's orientation: MemHash.cpp:167-203) against the oracle, for groups without
genome 0 and groups whose smallest genome is reverse-complemented, under the default tolerances
(Probes(), MatchList, counters) and under MaskedMemHash (MatchList), in the MG 4, 8, 16 and 32
instances of the probe kernel (G = 3, 8, 9 and 17)."""
import random

import pytest

from tests.test_gpu_probe_edges import _check, _check_matchlist, _mutate, _revcomp

pytestmark = pytest.mark.gpu

N = 2_400
CASES = {}


def _genomes(oracle_mod, G, rc):
    """G related genomes; genome 0 shares only the first third with the others (the groups of the
    rest hold no genome 0), genome 1 only the first two thirds; genome rc is reverse-complemented"""
    if (G, rc) not in CASES:
        rng = random.Random(100 * G + rc)
        base, other0, other1 = oracle_mod.generate(3, N, 1.0, 5100 + G)
        seqs = [_mutate(base, 0.01, rng) for _ in range(G)]
        seqs[0] = seqs[0][:N // 3] + other0[N // 3:]
        seqs[1] = seqs[1][:2 * N // 3] + other1[2 * N // 3:]
        seqs[rc] = _revcomp(seqs[rc])
        CASES[(G, rc)] = seqs
    return CASES[(G, rc)]


def _rc_of(G, which):
    return {"first": 0, "second": 1, "third": 2, "last": G - 1}[which]


@pytest.mark.parametrize("which", ["first", "second", "third", "last"])
@pytest.mark.parametrize("G", [3, 8, 9, 17])
def test_default_tolerances(gpu_lib, oracle_mod, G, which):
    seqs = _genomes(oracle_mod, G, _rc_of(G, which))
    ost = _check(gpu_lib, oracle_mod, seqs, oracle_mod.get_seed(15))
    assert ost["probes"] > 1000   # (more than the first third alone can give: N // 3 positions)


@pytest.mark.parametrize("w", [19, 13])
def test_default_tolerances_other_sorts(gpu_lib, oracle_mod, w):
    """w19: 128 MSD buckets; w13: a 27-bit key (other pass counts of the sort, which leaves the
    strand bit of equal keys sorted or not)"""
    for which in ("first", "second"):
        _check(gpu_lib, oracle_mod, _genomes(oracle_mod, 8, _rc_of(8, which)), oracle_mod.get_seed(w))


@pytest.mark.parametrize("which", ["first", "second", "last"])
@pytest.mark.parametrize("G", [3, 8, 9, 17])
def test_masked_memhash(gpu_lib, oracle_mod, G, which):
    seqs = _genomes(oracle_mod, G, _rc_of(G, which))
    seed = oracle_mod.get_seed(15)
    no0 = (1 << (G - 1)) - 1          # every genome but genome 0 (genome 0 = the top bit)
    # no selection; the groups without genome 0; those without genomes 0 and 1
    for mask in (0, no0) + ((no0 >> 1,) if G > 3 else ()):
        ref = _check_matchlist(gpu_lib, oracle_mod, seqs, seed, mask=mask)
        assert len(ref[0]) > 0
